// mgx_step_episodes.hip -- the fused continuous K-step over per-grid in-place episodes (mgx_step_k_episodes): K steps of
// Microgrid.run(control, normalized) per launch, the controls out of an action stream [K, N, A], every lane on the rows of its OWN
// episode and restarting inside the launch.  The continuous twin of rollout_episodes_kernel (mgx_episodes.hip).
// One of the six translation units of mgx_episode_loop.hpp, which states what their loops share and how a unit is compiled.
#include "mgx_episode_loop.hpp"

namespace mgx {

// F: layout.  U: depth of the row ring.  UA: depth of the action ring.  AT: storage type of the controls (widened when the step
// consumes the slot, as in step_k_kernel).  SRC: where the series rows come from (EP_SRC_*: fetch_row_slot).
// Row k of `actions` belongs to step k of the launch whatever episode a grid is in: the action rows are wave-uniform (an SGPR row
// base + the lane's offset) and a restart does not touch them -- only the series rows, which move with the lane's episode, are
// read again in the restart branch.
// The shared counter of this mode never ends; `done` is the lane's own (counter >= ep_final[i] - 1 on a register copy of
// ep_final[i] that a restart refreshes).  After every step: the statistics, then episode_auto_restart with the counter value of the
// step -- the call step_body<F, true> makes -- so K steps here leave what K calls of mgx_step leave.
template <int F, int U, int UA, typename AT, int SRC>
__global__ __launch_bounds__(BLOCK_K) void step_k_episodes_kernel(const KArgs a, const AT *__restrict__ actions, int32_t t0, int32_t K,
                                                                  int normalized, const FusedOut out, const mgx_episode_stats es,
                                                                  int32_t gpb, const KArgs *__restrict__ a_dev)
{
    constexpr int A_DIM = 2 * ((F & F_GENSET) != 0) + ((F & F_BATTERY) != 0) + ((F & F_GRID) != 0);
    const int64_t i = (int64_t)blockIdx.x * gpb + threadIdx.x;
    if ((int32_t)threadIdx.x >= gpb || i >= a.N) return;
    const int64_t N = a.N;
    const uint32_t i32 = (uint32_t)i;
    Params p; State s; Derived d;
    load_state<F>(a.c, i, false, s);
    load_params<F>(a.c, i, p);
    derive<F>(p, d);
    const bool gen_instant = genset_wave_is_instant<F>(p, s);
    const bool norm = normalized != 0;
    const bool want_soc = out.soc_trace != nullptr;
    const bool ar_on = a.ar_mode != 0;
    int32_t off = a.ep_off[i], fin = a.ep_final[i];
    GridFactors f;
    load_lane_factors<F, SRC>(a.c, i, f);
    LaneStats st;
    st.load(es, i);

    // One loop body, `gen_instant` a run-time (wave-uniform) flag, both rings rotate (rotate_ring): the lessons of
    // rollout_episodes_kernel.
    {
        const bool GI = gen_instant;
        RowSlot ring[U];
        RawActions<AT> act[UA];
        fill_row_ring<F, SRC>(a, f, i, t0, off, K, ring);
        // the action row of the step that enters the action ring next (wave-uniform)
        const AT *arow = actions;
#pragma unroll
        for (int u = 0; u < UA; u++)
            if (u < K) { load_actions_at<F>(arow, i32, act[u]); arow += N * A_DIM; }
        int64_t o64 = i;
#pragma nounroll
        for (int32_t k = 0; k < K; k++) {
            const int32_t t = t0 + k;
            Inputs in;
            widen_row_slot<F, SRC>(a, f, ring[0], t, off, in);
            if constexpr (F & F_GENSET) { in.a_goal = (double)act[0].a_goal; in.a_gen = (double)act[0].a_gen; }
            if constexpr (F & F_BATTERY) in.a_bat = (double)act[0].a_bat;
            if constexpr (F & F_GRID) in.a_grid = (double)act[0].a_grid;
            rotate_ring(ring);
            rotate_ring(act);
            if (k + UA < K) { load_actions_at<F>(arow, i32, act[UA - 1]); arow += N * A_DIM; }
            Outputs o;
            step_core<F>(p, d, s, in, norm, want_soc, GI, o);
            const double r = shaped_reward<F>(a.shaper, o);
            const bool dn = t >= fin - 1;                       // done_at(a, i, t)
            store_step_outputs<F>(out, o64, r, dn, s);
            o64 += N;
            st.update(r, t, fin);
            if (ar_on && dn) {
                restart_lane(a_dev, i, t, off, fin);
                advance_row_ring<F, SRC>(a, f, i, t, k, off, K, true, ring);      // (the controls stay)
            } else {
                advance_row_ring<F, SRC>(a, f, i, t, k, off, K, false, ring);
            }
        }
    }
    if constexpr (F & F_BATTERY) { if (!want_soc) s.soc = s.charge / p.bat_cmax; }
    store_state<F>(a_dev->c, i, s);           // (the same columns; their addresses need no scalar registers across the loop)
    st.store(es.ret_running, es.ret_sum, es.ret_last, es.episodes, i);
}

template <int F, typename AT>
static void step_k_episodes_launch(const EpisodeLaunch &L)
{
    with_episode_src(L.src, [&](auto src) {
        step_k_episodes_kernel<F, ROW_RING<F>, MGX_RING_STEP_EPISODES, AT, decltype(src)::value><<<L.blocks, BLOCK_K, 0, L.stream>>>(
            *L.k, (const AT *)L.actions, L.t, L.K, L.normalized, L.out, L.stats, L.gpb, L.k_dev);
    });
}

template <int F>
static void step_k_episodes_dispatch(const EpisodeLaunch &L)
{
    if (L.act_f32) step_k_episodes_launch<F, float>(L);
    else step_k_episodes_launch<F, double>(L);
}

MGX_EPISODE_LAUNCH_FN(step_k_episodes, EpisodeLaunch, L.flags)

}  // namespace mgx
