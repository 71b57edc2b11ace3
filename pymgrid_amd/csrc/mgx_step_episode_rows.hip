// mgx_step_episode_rows.hip -- the fused continuous K-step over per-grid in-place episodes WITH observation rows
// (mgx_step_k_episodes_rows): step_k_episodes_kernel (mgx_step_episodes.hip) + per step the H = 0 row the step returned and, where
// a grid restarts, the row before the restart.  The continuous twin of rollout_episodes_rows_kernel (mgx_episode_rows.hip).
// One of the six translation units of mgx_episode_loop.hpp, which states what their loops share and how a unit is compiled; what
// the rows add is in mgx_episode_rows.hpp.
#include "mgx_episode_rows.hpp"

namespace mgx {

// Template parameters, rings, statistics and restart as step_k_episodes_kernel; the rows as rollout_episodes_rows_kernel writes
// them: final_obs[k, i, :] where step k restarts grid i (ring slot 0 after the rotation, under the old offset), obs[k, i, :] for
// every grid (slot 0 under the offset the restart left).  The row ring reaches one row further than the plain kernel's (K + 1: the
// ring's reach, mgx_episode_loop.hpp); the action ring keeps its guard, there is no action row K.  SoC is formed every step.
// The arguments as ONE struct, what the loop does not need read late, the row's columns packed in one word: the scalar-register
// diet of rollout_episodes_rows_kernel.
template <int F, int U, int UA, typename AT, int SRC>
__global__ __launch_bounds__(BLOCK_K) void step_k_episodes_rows_kernel(const StepRowsArgs g)
{
    const KArgs &a = g.a;
    const AT *__restrict__ actions = (const AT *)g.actions;
    const int32_t t0 = g.t0, K = g.K, gpb = g.gpb;
    const int normalized = g.normalized;
    const FusedOut &out = g.out;
    const mgx_episode_stats &es = g.es;
    void *__restrict__ obs = g.obs;
    const bool want_final = g.final_obs != nullptr;
    uint32_t desc = g.desc;
    const auto *late = late_kernargs<StepRowsArgs>();
    constexpr int A_DIM = 2 * ((F & F_GENSET) != 0) + ((F & F_BATTERY) != 0) + ((F & F_GRID) != 0);
    // one wave-private tile per wave for the rows of a step (store_episode_row)
    __shared__ __attribute__((aligned(16))) double row_tiles[MGX_EPISODE_ROWS_TILE ? (BLOCK_K / 64) * 64 * ROW_TILE_MAX_D : 1];
    const int64_t i = (int64_t)blockIdx.x * gpb + threadIdx.x;
    if ((int32_t)threadIdx.x >= gpb || i >= a.N) return;
    double *tile = row_tiles + (MGX_EPISODE_ROWS_TILE ? (threadIdx.x >> 6) * (64 * ROW_TILE_MAX_D) : 0);
    const int64_t N = a.N;
    const uint32_t i32 = (uint32_t)i;
    Params p; State s; Derived d;
    load_state<F>(a.c, i, false, s);
    load_params<F>(a.c, i, p);
    derive<F>(p, d);
    const bool gen_instant = genset_wave_is_instant<F>(p, s);
    const bool norm = normalized != 0;
    const bool ar_on = a.ar_mode != 0;
    int32_t off = a.ep_off[i], fin = a.ep_final[i];
    GridFactors f;
    load_lane_factors<F, SRC>(a.c, i, f);
    RowBounds<F> rb;
    load_row_bounds<F>(a.c, N, i, rb);
    LaneStats st;
    st.load(es, i);
    {
        const bool GI = gen_instant;
        RowSlot ring[U];
        RawActions<AT> act[UA];
        fill_row_ring<F, SRC>(a, f, i, t0, off, K + 1, ring);
        // the action row of the step that enters the action ring next (wave-uniform)
        const AT *arow = actions;
#pragma unroll
        for (int u = 0; u < UA; u++)
            if (u < K) { load_actions_at<F>(arow, i32, act[u]); arow += N * A_DIM; }
        int64_t o64 = i;
        int64_t r64 = i * row_desc_dim(desc);      // element offset of row (k, i) of obs / final_obs
#pragma nounroll
        for (int32_t k = 0; k < K; k++) {
            const int32_t t = t0 + k;
            asm volatile("" : "+s"(desc));             // (opaque: the fields are taken out where a row is built, every step)
            Inputs in;
            widen_row_slot<F, SRC>(a, f, ring[0], t, off, in);
            if constexpr (F & F_GENSET) { in.a_goal = (double)act[0].a_goal; in.a_gen = (double)act[0].a_gen; }
            if constexpr (F & F_BATTERY) in.a_bat = (double)act[0].a_bat;
            if constexpr (F & F_GRID) in.a_grid = (double)act[0].a_grid;
            rotate_ring(ring);
            rotate_ring(act);
            if (k + UA < K) { load_actions_at<F>(arow, i32, act[UA - 1]); arow += N * A_DIM; }
            Outputs o;
            step_core<F>(p, d, s, in, norm, true, GI, o);
            const double r = shaped_reward<F>(a.shaper, o);
            const bool dn = t >= fin - 1;                       // done_at(a, i, t)
            store_step_outputs<F>(out, o64, r, dn, s);
            o64 += N;
            st.update(r, t, fin);
            if (ar_on && dn) {
                const KArgs *__restrict__ a_dev = late->a_dev;
                if (want_final) {                               // the row of the episode that ends here: slot 0, still the old rows
                    Inputs inf;
                    widen_row_slot<F, SRC>(a, f, ring[0], t + 1, off, inf);
                    store_final_row<F>(a_dev, a.T, desc, late->final_obs, r64, i, t + 1 + off, inf, rb, p, s);
                }
                restart_lane(a_dev, i, t, off, fin);
                // advance_row_ring (mgx_episode_loop.hpp, reach K + 1) written out: under the helper the forms <7 | 15, 4, 4, double,
                // FACT> of this kernel take 7 accumulation registers instead of 5 (split in two likewise) -- a change there is made
                // here too
#pragma unroll
                for (int v = 0; v < U; v++)
                    if (k + 1 + v <= K) fetch_row_slot<F, SRC>(a, f, i, t + 1 + v, off, ring[v]);
            } else if (k + U <= K) {
                fetch_row_slot<F, SRC>(a, f, i, t + U, off, ring[U - 1]);
            }
            if (obs) {
                Inputs inn;
                widen_row_slot<F, SRC>(a, f, ring[0], t + 1, off, inn);
                store_episode_row<F>(late->a_dev, a.T, desc, obs, r64, i, t + 1 + off, inn, rb, p, s, tile);
            }
            r64 += N * row_desc_dim(desc);
        }
    }
    store_state<F>(late->a_dev->c, i, s);     // (the same columns; their addresses need no scalar registers across the loop)
    // (the statistics' addresses a second time, from the kernarg segment: the first copies ended their lives before the loop)
    st.store(late->es.ret_running, late->es.ret_sum, late->es.ret_last, late->es.episodes, i);
}

template <int F, typename AT>
static void step_k_episodes_rows_launch(const EpisodeRowsLaunch &R)
{
    const EpisodeLaunch &L = R.e;
    const StepRowsArgs g{*L.k, L.actions, L.t, L.K, L.normalized, L.gpb, L.out, L.stats, pack_row_desc(*L.k), L.k_dev, R.obs, R.final_obs};
    with_episode_src(L.src, [&](auto src) {
        step_k_episodes_rows_kernel<F, ROW_RING<F>, MGX_RING_STEP_EPISODES, AT, decltype(src)::value><<<L.blocks, BLOCK_K, 0, L.stream>>>(g);
    });
}

template <int F>
static void step_k_episodes_rows_dispatch(const EpisodeRowsLaunch &R)
{
    if (R.e.act_f32) step_k_episodes_rows_launch<F, float>(R);
    else step_k_episodes_rows_launch<F, double>(R);
}

MGX_EPISODE_LAUNCH_FN(step_k_episodes_rows, EpisodeRowsLaunch, L.e.flags)

}  // namespace mgx
