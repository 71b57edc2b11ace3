// mgx_lookahead_step_episodes.hip -- the continuous what-if launch over per-grid in-place episodes (mgx_lookahead_step_k_episodes):
// C candidate plans of controls per grid, simulated at most H steps of Microgrid.run(control, normalized) ahead from the handle's
// current state, none of them committed.  A sibling of step_k_episodes_kernel (mgx_step_episodes.hip) on the pieces of
// mgx_episode_loop.hpp; mgx_lookahead.hpp states the mapping and what the two what-if units share.  Compiled like the other
// episode units (-DMGX_EPISODE_PART=p).
#include "mgx_lookahead.hpp"

namespace mgx {

// F: layout.  U: depth of the row ring.  UA: depth of the action ring.  AT: storage type of the controls (widened when the step
// consumes the slot).  PER_GRID: plans [C, H, N, A] (else [C, H, A]: the controls of a step are wave-uniform, every lane reads
// element 0 of the step's row).  SRC: where the series rows come from (EP_SRC_*: fetch_row_slot).
// The lane of (grid i, candidate c0 + blockIdx.y) takes lookahead_steps steps -- step_core<F> and shaped_reward<F> on the operands
// step_k_episodes_kernel's step has -- on a register copy of the grid's state and leaves ret[c, i] (and charge / max_capacity, the
// SoC soc_trace would hold at the last counted step).  Neither ring reaches beyond the lane's last step.
template <int F, int U, int UA, typename AT, bool PER_GRID, int SRC>
__global__ __launch_bounds__(BLOCK_K) void lookahead_step_k_episodes_kernel(const KArgs a, const AT *__restrict__ plans, int32_t t0,
                                                                            int32_t H, int32_t c0, int normalized, double gamma,
                                                                            double *__restrict__ ret, double *__restrict__ end_soc,
                                                                            int32_t gpb)
{
    constexpr int A_DIM = 2 * ((F & F_GENSET) != 0) + ((F & F_BATTERY) != 0) + ((F & F_GRID) != 0);
    const int64_t i = (int64_t)blockIdx.x * gpb + threadIdx.x;
    const int64_t c = (int64_t)c0 + blockIdx.y;
    if ((int32_t)threadIdx.x >= gpb || i >= a.N) return;
    const int64_t N = a.N;
    const uint32_t ia = PER_GRID ? (uint32_t)i : 0u;           // the lane's place in a step's row of controls
    const int64_t arow_len = (PER_GRID ? N : 1) * A_DIM;        // ... and the length of that row
    Params p; State s; Derived d;
    load_state<F>(a.c, i, false, s);
    load_params<F>(a.c, i, p);
    derive<F>(p, d);
    const bool GI = genset_wave_is_instant<F>(p, s);
    const bool norm = normalized != 0;
    const int32_t off = a.ep_off[i];
    const int32_t n = lookahead_steps(t0, a.ep_final[i], H);
    GridFactors f;
    load_lane_factors<F, SRC>(a.c, i, f);

    RowSlot ring[U];
    RawActions<AT> act[UA];
    fill_row_ring<F, SRC>(a, f, i, t0, off, n, ring);
    // the control row of the step that enters the action ring next (wave-uniform): the candidate's H rows lie one after the other
    const AT *arow = plans + c * H * arow_len;
#pragma unroll
    for (int u = 0; u < UA; u++)
        if (u < n) { load_actions_at<F>(arow, ia, act[u]); arow += arow_len; }
    double acc = 0.0, w = 1.0;
#pragma nounroll
    for (int32_t k = 0; k < n; k++) {
        const int32_t t = t0 + k;
        Inputs in;
        widen_row_slot<F, SRC>(a, f, ring[0], t, off, in);
        if constexpr (F & F_GENSET) { in.a_goal = (double)act[0].a_goal; in.a_gen = (double)act[0].a_gen; }
        if constexpr (F & F_BATTERY) in.a_bat = (double)act[0].a_bat;
        if constexpr (F & F_GRID) in.a_grid = (double)act[0].a_grid;
        rotate_ring(ring);
        rotate_ring(act);
        if (k + UA < n) { load_actions_at<F>(arow, ia, act[UA - 1]); arow += arow_len; }
        Outputs o;
        step_core<F>(p, d, s, in, norm, false, GI, o);
        lookahead_count(shaped_reward<F>(a.shaper, o), gamma, acc, w);
        advance_row_ring<F, SRC>(a, f, i, t, k, off, n, false, ring);
    }
    const int64_t e = c * N + i;
    ret[e] = acc;
    if constexpr (F & F_BATTERY) { if (end_soc) end_soc[e] = s.charge / p.bat_cmax; }
}

template <int F, typename AT>
static void lookahead_step_k_episodes_launch(const LookaheadLaunch &L)
{
    with_episode_src(L.src, [&](auto src) {
        constexpr int SRC = decltype(src)::value, U = ROW_RING<F>, UA = MGX_RING_STEP_EPISODES;
        for (int32_t c0 = 0; c0 < L.C; c0 += LOOKAHEAD_MAX_Y) {
            const dim3 grid(L.blocks, (unsigned)(L.C - c0 < LOOKAHEAD_MAX_Y ? L.C - c0 : LOOKAHEAD_MAX_Y));
            if (L.per_grid)
                lookahead_step_k_episodes_kernel<F, U, UA, AT, true, SRC><<<grid, BLOCK_K, 0, L.stream>>>(
                    *L.k, (const AT *)L.actions, L.t, L.H, c0, L.normalized, L.gamma, L.ret, L.end_soc, L.gpb);
            else
                lookahead_step_k_episodes_kernel<F, U, UA, AT, false, SRC><<<grid, BLOCK_K, 0, L.stream>>>(
                    *L.k, (const AT *)L.actions, L.t, L.H, c0, L.normalized, L.gamma, L.ret, L.end_soc, L.gpb);
        }
    });
}

template <int F>
static void lookahead_step_k_episodes_dispatch(const LookaheadLaunch &L)
{
    if (L.act_f32) lookahead_step_k_episodes_launch<F, float>(L);
    else lookahead_step_k_episodes_launch<F, double>(L);
}

MGX_EPISODE_LAUNCH_FN(lookahead_step_k_episodes, LookaheadLaunch, L.flags)

}  // namespace mgx
