// mgx_lookahead.hpp -- what the two what-if launches over per-grid in-place episodes share (mgx_lookahead_episodes:
// lookahead_episodes_kernel, mgx_lookahead_episodes.hip; mgx_lookahead_step_k_episodes: lookahead_step_k_episodes_kernel,
// mgx_lookahead_step_episodes.hip) and what mgx_abi.hip hands them.  Sibling loops of rollout_episodes_kernel and
// step_k_episodes_kernel on the pieces of mgx_episode_loop.hpp, with the same per-step arithmetic, that COMMIT NOTHING: a lane is a
// (grid i, candidate c) pair -- blockIdx.y = c, the launches' line of gpb grids along x, so a wave holds consecutive grids of one
// candidate: state, parameter and row loads stay coalesced, the C re-reads of a grid's rows hit the L2, ret[c, :] is a coalesced
// store -- that simulates its plan from the handle's current state and counter on the rows of the grid's running episode and keeps
// only the discounted return.  No store_state, no restart (the draw belongs to another episode: nothing beyond the end of the
// running episode is simulated), no statistics, no per-step stores.
#pragma once
#include "mgx_episode_loop.hpp"

namespace mgx {

// The steps a lane counts from counter value t0 in an episode that ends with step fin - 1: min(H, fin - t0), at least 1 (a grid
// that stands on or behind its last step and has not been restarted counts the one step it would take).  It depends on the grid
// alone, so every candidate of a grid stops at the same step.
__host__ __device__ __forceinline__ int32_t lookahead_steps(int32_t t0, int32_t fin, int32_t H)
{
    int32_t n = fin - t0;
    n = n < H ? n : H;
    return n < 1 ? 1 : n;
}

// THE RULE of the return (include/mgx.h, mgx_lookahead): in step order, plain fp64, one multiply and one add per step
__device__ __forceinline__ void lookahead_count(double r, double gamma, double &ret, double &w)
{
    ret = ret + w * r;
    w = w * gamma;
}

// A launch as the host side hands it to the slices of the two units; a call fills the fields of its kind.
struct LookaheadLaunch {
    int flags;                       // layout (template parameter F)
    int src;                         // EP_SRC_*
    unsigned blocks;                 // along x: lines of gpb grids
    int32_t gpb;
    hipStream_t stream;
    const KArgs *k;
    bool per_grid;                   // a plan per grid (else the C plans are shared by all grids)
    const PLWords *tab;              // discrete: priority-list table
    const uint8_t *ids;              // discrete: plans [C, H] or [C, H, N]
    const void *actions;             // continuous: plans [C, H, A] or [C, H, N, A] in the handle's action format
    bool act_f32;
    uint64_t cem_key;                // drawn candidates (mgx_cem): the key and the [H, N, A] rows the controls are formed from
    const double *cem_mean, *cem_sigma;
    int normalized;
    int32_t t, C, H;
    double gamma;
    double *ret;                     // [C, N]
    double *end_soc;                 // [C, N] or NULL
};
constexpr int LOOKAHEAD_MAX_Y = 65535;       // candidates per launch (gridDim.y); more: further launches from candidate c0 on

bool launch_lookahead_episodes_p0(const LookaheadLaunch &L); bool launch_lookahead_episodes_p1(const LookaheadLaunch &L);
bool launch_lookahead_step_k_episodes_p0(const LookaheadLaunch &L); bool launch_lookahead_step_k_episodes_p1(const LookaheadLaunch &L);
// ... and their sibling with drawn candidates (mgx_lookahead_gaussian_episodes: lookahead_gaussian_episodes_kernel,
// mgx_lookahead_gaussian_episodes.hip, on top of mgx_cem.hpp)
bool launch_lookahead_gaussian_episodes_p0(const LookaheadLaunch &L); bool launch_lookahead_gaussian_episodes_p1(const LookaheadLaunch &L);

}  // namespace mgx
