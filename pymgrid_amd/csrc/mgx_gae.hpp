// mgx_gae.hpp -- what mgx_abi.hip hands mgx_gae.hip: the arguments of gae_kernel (mgx_gae, include/mgx.h) and its launch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mgx {

struct GaeArgs {
    int64_t N;
    int32_t K;
    const double *reward;            // [K, N]
    const uint8_t *done;             // [K, N]
    const double *value;             // [K, N]
    const double *final_value;       // [K, N] or NULL
    const double *last_value;        // [N]
    double gamma, c;                 // c = gamma * lambda, formed once on the host
    double *advantage;               // [K, N]
    double *returns;                 // [K, N] or NULL
};

void launch_gae(const GaeArgs &g, hipStream_t stream);

}  // namespace mgx
