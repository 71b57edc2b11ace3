// mgx_lookahead_gaussian_episodes.hip -- the CEM what-if launch over per-grid in-place episodes (mgx_lookahead_gaussian_episodes):
// lookahead_step_k_episodes_kernel (mgx_lookahead_step_episodes.hip) with the candidates' controls DRAWN in registers round a
// per-grid mean instead of read from a plan tensor [C, H, N, A].  A sibling loop on the pieces of mgx_episode_loop.hpp and
// mgx_lookahead.hpp (the mapping: a lane per (grid, candidate), blockIdx.y = candidate); the draw and the candidate value are
// mgx_cem.hpp's.  Compiled like the other episode units (-DMGX_EPISODE_PART=p).
#include "mgx_lookahead.hpp"
#include "mgx_cem.hpp"

namespace mgx {

// Depths of the two rings.  A step with its Box-Muller pairs is several times as long as the sibling's, so it hides a load behind
// fewer steps, and registers are what this kernel is short of: with the sibling's depths (series rows 4 / 8, controls 2) the
// genset+battery+grid form took 187 VGPRs (2 waves per SIMD); at series rows 2 and ONE row of (mean, sigma) -- 2 A doubles, the row
// of the next step, loaded while this step computes -- it takes 159 (3 waves).  profiles/exp_cem.txt has both forms' times.
#ifndef MGX_CEM_SERIES_RING
#define MGX_CEM_SERIES_RING 2        // 0: ROW_RING<F>, the sibling's depth
#endif
#ifndef MGX_CEM_ROW_RING
#define MGX_CEM_ROW_RING 1
#endif
constexpr int CEM_ROW_RING = MGX_CEM_ROW_RING;

// F: layout.  U: depth of the series row ring.  UA: depth of the (mean, sigma) ring.  SRC: where the series rows come from.
// The lane of (grid i, candidate c = c0 + blockIdx.y) takes lookahead_steps steps on a register copy of the grid's state, step k
// under the controls cem_candidate forms from row (k, i) of mean / sigma -- formed where the step consumes them, so a draw holds no
// register across the step; c == 0 (the mean plan, no draw) is a wave-uniform branch.  It leaves ret[c, i] (and the end SoC).
template <int F, int U, int UA, int SRC>
__global__ __launch_bounds__(BLOCK_K) void lookahead_gaussian_episodes_kernel(const KArgs a, uint64_t key, const double *mean,
                                                                              const double *sigma, int f32, int32_t t0, int32_t H,
                                                                              int32_t c0, double gamma, double *__restrict__ ret,
                                                                              double *__restrict__ end_soc, int32_t gpb)
{
    constexpr int A_DIM = 2 * ((F & F_GENSET) != 0) + ((F & F_BATTERY) != 0) + ((F & F_GRID) != 0);
    static_assert(A_DIM >= 1, "a layout with a control");
    const int64_t i = (int64_t)blockIdx.x * gpb + threadIdx.x;
    const int64_t c = (int64_t)c0 + blockIdx.y;
    if ((int32_t)threadIdx.x >= gpb || i >= a.N) return;
    const int64_t N = a.N;
    const int64_t arow_len = N * A_DIM;                          // doubles of a plan step's block of mean / sigma
    Params p; State s; Derived d;
    load_state<F>(a.c, i, false, s);
    load_params<F>(a.c, i, p);
    derive<F>(p, d);
    const bool GI = genset_wave_is_instant<F>(p, s);
    const int32_t off = a.ep_off[i];
    const int32_t n = lookahead_steps(t0, a.ep_final[i], H);
    GridFactors f;
    load_lane_factors<F, SRC>(a.c, i, f);

    RowSlot ring[U];
    CemRow<A_DIM> act[UA];
    fill_row_ring<F, SRC>(a, f, i, t0, off, n, ring);
    // the blocks of the plan step that enters the (mean, sigma) ring next (wave-uniform)
    const double *mrow = mean, *srow = sigma;
#pragma unroll
    for (int u = 0; u < UA; u++)
        if (u < n) { load_cem_row<A_DIM>(mrow, srow, i, act[u]); mrow += arow_len; srow += arow_len; }
    double acc = 0.0, w = 1.0;
#pragma nounroll
    for (int32_t k = 0; k < n; k++) {
        const int32_t t = t0 + k;
        Inputs in;
        widen_row_slot<F, SRC>(a, f, ring[0], t, off, in);
        {
            double x[A_DIM];
            cem_candidate<A_DIM>(key, i, c, k, act[0].m, act[0].s, f32 != 0, x);
            int q = 0;
            if constexpr (F & F_GENSET) { in.a_goal = x[q]; in.a_gen = x[q + 1]; q += 2; }
            if constexpr (F & F_BATTERY) { in.a_bat = x[q]; q += 1; }
            if constexpr (F & F_GRID) in.a_grid = x[q];
        }
        rotate_ring(ring);
        rotate_ring(act);
        if (k + UA < n) { load_cem_row<A_DIM>(mrow, srow, i, act[UA - 1]); mrow += arow_len; srow += arow_len; }
        Outputs o;
        step_core<F>(p, d, s, in, true, false, GI, o);
        lookahead_count(shaped_reward<F>(a.shaper, o), gamma, acc, w);
        advance_row_ring<F, SRC>(a, f, i, t, k, off, n, false, ring);
    }
    const int64_t e = c * N + i;
    ret[e] = acc;
    if constexpr (F & F_BATTERY) { if (end_soc) end_soc[e] = s.charge / p.bat_cmax; }
}

template <int F>
static void lookahead_gaussian_episodes_dispatch(const LookaheadLaunch &L)
{
    if constexpr ((F & (F_GENSET | F_BATTERY | F_GRID)) != 0) {      // (a layout without a control: refused before the launch)
        with_episode_src(L.src, [&](auto src) {
            constexpr int SRC = decltype(src)::value, U = MGX_CEM_SERIES_RING ? MGX_CEM_SERIES_RING : ROW_RING<F>, UA = CEM_ROW_RING;
            for (int32_t c0 = 0; c0 < L.C; c0 += LOOKAHEAD_MAX_Y) {
                const dim3 grid(L.blocks, (unsigned)(L.C - c0 < LOOKAHEAD_MAX_Y ? L.C - c0 : LOOKAHEAD_MAX_Y));
                lookahead_gaussian_episodes_kernel<F, U, UA, SRC><<<grid, BLOCK_K, 0, L.stream>>>(
                    *L.k, L.cem_key, L.cem_mean, L.cem_sigma, L.act_f32 ? 1 : 0, L.t, L.H, c0, L.gamma, L.ret, L.end_soc, L.gpb);
            }
        });
    }
}

MGX_EPISODE_LAUNCH_FN(lookahead_gaussian_episodes, LookaheadLaunch, L.flags)

}  // namespace mgx
