// mgx_gae.hip -- generalised advantage estimation over the [K, N] outputs of the closed-loop launches (mgx_gae, include/mgx.h):
// one lane per grid, so every [k, :] access is coalesced, walking k backwards with the two values the recurrence carries (the
// advantage of the step behind, the value of the state behind) in registers.  A pure stream -- 25 bytes in per element (33 with
// final_value) and 8 out (16 with returns), six fp64 operations -- so what matters is how many loads are in flight: the reverse
// loop goes in groups of GAE_GROUP steps whose loads are all issued before the first of them is used, instead of one dependent
// round trip per step.  Plain C++, vector stores.
#include "mgx_gae.hpp"

namespace mgx {

constexpr int GAE_BLOCK = 64;        // one wave per workgroup: N / 64 waves is all the parallelism there is, spread over every CU
constexpr int GAE_GROUP = 8;         // steps whose loads are in flight together (3 or 4 loads each)

// one step of the rule, on values already loaded
template <bool FV>
__device__ __forceinline__ double gae_step(double r, bool d, double v, double fv, double gamma, double c, double &carry, double &next)
{
    const double nv = d ? (FV ? fv : 0.0) : next;
    const double delta = (r + gamma * nv) - v;
    const double A = d ? delta : delta + c * carry;              // (a select: a NaN carry does not cross an episode boundary)
    carry = A;
    next = v;
    return A;
}

template <bool FV, bool RET>
__global__ __launch_bounds__(GAE_BLOCK) void gae_kernel(const GaeArgs g)
{
    const int64_t N = g.N;
    const int64_t i = (int64_t)blockIdx.x * GAE_BLOCK + threadIdx.x;
    if (i >= N) return;
    const double *__restrict__ reward = g.reward;
    const uint8_t *__restrict__ done = g.done;
    const double *__restrict__ value = g.value;
    const double *__restrict__ final_value = g.final_value;
    double *__restrict__ advantage = g.advantage;
    double *__restrict__ returns = g.returns;
    const double gamma = g.gamma, c = g.c;
    double next = g.last_value[i], carry = 0.0;
    int32_t k = g.K;                                             // steps k - 1, k - 2, ... are still to do
    int64_t e = (int64_t)(k - 1) * N + i;                        // element (k - 1, i): 64 bits, [K, N] passes 2^31 elements
#pragma nounroll
    for (; k >= GAE_GROUP; k -= GAE_GROUP) {
        double r[GAE_GROUP], v[GAE_GROUP], fv[GAE_GROUP];
        uint8_t d[GAE_GROUP];
#pragma unroll
        for (int j = 0; j < GAE_GROUP; j++) {                    // every load of the group, before anything waits for one
            const int64_t q = e - (int64_t)j * N;
            r[j] = reward[q];
            d[j] = done[q];
            v[j] = value[q];
            fv[j] = FV ? final_value[q] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < GAE_GROUP; j++) {
            const int64_t q = e - (int64_t)j * N;
            const double A = gae_step<FV>(r[j], d[j] != 0, v[j], fv[j], gamma, c, carry, next);
            advantage[q] = A;
            if (RET) returns[q] = A + v[j];
        }
        e -= (int64_t)GAE_GROUP * N;
    }
#pragma nounroll
    for (; k > 0; k--) {                                         // the K mod GAE_GROUP steps at the front
        const double r = reward[e], v = value[e], fv = FV ? final_value[e] : 0.0;
        const bool d = done[e] != 0;
        const double A = gae_step<FV>(r, d, v, fv, gamma, c, carry, next);
        advantage[e] = A;
        if (RET) returns[e] = A + v;
        e -= N;
    }
}

void launch_gae(const GaeArgs &g, hipStream_t stream)
{
    const unsigned blocks = (unsigned)((g.N + GAE_BLOCK - 1) / GAE_BLOCK);
    if (g.final_value) {
        if (g.returns) gae_kernel<true, true><<<blocks, GAE_BLOCK, 0, stream>>>(g);
        else gae_kernel<true, false><<<blocks, GAE_BLOCK, 0, stream>>>(g);
    } else {
        if (g.returns) gae_kernel<false, true><<<blocks, GAE_BLOCK, 0, stream>>>(g);
        else gae_kernel<false, false><<<blocks, GAE_BLOCK, 0, stream>>>(g);
    }
}

}  // namespace mgx
