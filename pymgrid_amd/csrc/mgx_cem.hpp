// mgx_cem.hpp -- the CEM planner's draw and candidate value (mgx_cem, include/mgx.h), stated once for their three users: the what-if
// launch that draws its candidates in registers (lookahead_gaussian_episodes_kernel, mgx_lookahead_gaussian_episodes.hip), its pick
// and the refit (cem_pick_kernel, cem_elite_kernel, cem_refit_kernel: mgx_cem.hip) -- and what mgx_abi.hip hands mgx_cem.hip.
// A candidate control is a function of (key, grid, candidate, plan step, column): whoever needs one forms it again.
#pragma once
#include "mgx_policy.hpp"

namespace mgx {

// normal pair p of grid i, candidate c, plan step k: the Box-Muller pair of mgx_gaussian on a draw keyed by all three
__device__ __forceinline__ void cem_pair(uint64_t key, int64_t i, int64_t c, int32_t k, uint32_t p, double &z0, double &z1)
{
    uint32_t r[4];
    philox4x32_10((uint32_t)i, (uint32_t)c, (uint32_t)k, 0xCE300000u + p, (uint32_t)key, (uint32_t)(key >> 32), r);
    gaussian_pair_of_words(r, z0, z1);
}

// x[c, k, i, 0 .. A) out of the row (m, s) = (mean, sigma)[k, i, :].  c == 0 is the mean plan (wave-uniform where the candidate
// is the workgroup's); a pair's draw is made only where one of its columns is live.  f32: the value a float32 plan would hold.
template <int A>
__device__ __forceinline__ void cem_candidate(uint64_t key, int64_t i, int64_t c, int32_t k, const double (&m)[A], const double (&s)[A],
                                              bool f32, double (&x)[A])
{
#pragma unroll
    for (int o = 0; o < A; o++) x[o] = m[o];
    if (c != 0) {
#pragma unroll
        for (int p = 0; 2 * p < A; p++) {
            const bool two = 2 * p + 1 < A;                                               // (false: the pair's second column does not exist)
            const int o0 = 2 * p, o1 = two ? 2 * p + 1 : 2 * p;
            const bool l0 = s[o0] > 0.0, l1 = two && s[o1] > 0.0;
            if (l0 || l1) {
                double z0, z1;
                cem_pair(key, i, c, k, (uint32_t)p, z0, z1);
                x[o0] = l0 ? m[o0] + s[o0] * z0 : x[o0];
                if (two) x[o1] = l1 ? m[o1] + s[o1] * z1 : x[o1];
            }
        }
    }
#pragma unroll
    for (int o = 0; o < A; o++) {
        const double v = policy_clip(x[o]);
        x[o] = f32 ? (double)(float)v : v;
    }
}

// the row (mean, sigma)[k, i, :] of a lane: A contiguous doubles each, coalesced across grids.  `mrow`, `srow`: the [N, A] blocks of
// plan step k (wave-uniform)
template <int A>
struct CemRow {
    double m[A], s[A];
};
template <int A>
__device__ __forceinline__ void load_cem_row(const double *mrow, const double *srow, int64_t i, CemRow<A> &r)
{
#pragma unroll
    for (int o = 0; o < A; o++) { r.m[o] = mrow[i * A + o]; r.s[o] = srow[i * A + o]; }
}

// A as a template argument: fn(std::integral_constant<int, A>) for A in 1 .. 4 (the callers have refused every other A)
template <typename FN>
static inline void with_action_dim(int32_t A, FN &&fn)
{
    if (A == 1) fn(std::integral_constant<int, 1>{});
    else if (A == 2) fn(std::integral_constant<int, 2>{});
    else if (A == 3) fn(std::integral_constant<int, 3>{});
    else fn(std::integral_constant<int, 4>{});
}

// ---- host side: what mgx_abi.hip hands mgx_cem.hip ----
// the pick behind mgx_lookahead_gaussian_episodes: lookahead_pick_kernel's results, first_action regenerated instead of copied
struct CemPick {
    int64_t N;
    int32_t C, H, t0, A;
    bool f32;                        // first_action is float32 (and the candidates are rounded to it)
    uint64_t key;
    const double *mean, *sigma;      // [H, N, A]: row 0 is read
    const double *ret;               // [C, N]
    const int32_t *ep_final;
    int32_t *steps, *best;
    double *best_ret;
    void *first_action;
};
void launch_cem_pick(const CemPick &q, hipStream_t stream);

// mgx_cem_refit, checked
struct CemRefitArgs {
    int64_t N;
    int32_t A, C, H, E;
    bool f32;
    uint64_t key;
    double alpha, beta, sigma_min;   // beta = 1.0 - alpha, formed once on the host
    const double *mean, *sigma;      // [H, N, A] (may be mean_out / sigma_out)
    const double *ret;               // [C, N]
    const int32_t *steps;            // [N] or NULL
    int32_t *elite;                  // [E, N]
    double *mean_out, *sigma_out;    // [H, N, A]
    void *best_plan;                 // [H, N, A] or NULL
};
void launch_cem_elite(const CemRefitArgs &g, hipStream_t stream);
void launch_cem_refit(const CemRefitArgs &g, hipStream_t stream);

}  // namespace mgx
