// mgx_step_hot.hpp -- what the host side (mgx_abi.hip) and mgx_step_hot.hip share: the launch of step_k_hot_kernel, the kernel of
// the lock-step hot K-step launch (factorised series, reward + SoC only, no GridModule, K within one LDS image of base rows).
#pragma once
#include "mgx_kernels.hpp"

namespace mgx {

// the most steps one launch of step_k_hot_kernel takes: the rows of one LDS image (no chunk loop in that kernel)
constexpr int32_t STEP_HOT_MAX_K = FACT_ROWS;

// Launches step_k_hot_kernel for L (shape, streams and outputs as fused_launch_for set them); false: no such kernel for L.flags.
// The caller has checked the rest of the predicate (step_k_hot_takes in mgx_abi.hip).
bool launch_step_k_hot(const FusedLaunch &L);

}  // namespace mgx
