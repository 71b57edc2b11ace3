// mgx_step_episode_rows.hip -- the fused continuous K-step over per-grid in-place episodes WITH observation rows
// (mgx_step_k_episodes_rows): step_k_episodes_kernel (mgx_step_episodes.hip) + per step the H = 0 row the step returned and, where
// a grid restarts, the row before the restart.  The continuous twin of rollout_episodes_rows_kernel (mgx_episode_rows.hip).
// Translation units of their own (MGX_EPISODE_PARTS slices of the layouts):
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c -DMGX_STEP_EPISODE_ROWS_PART=p mgx_step_episode_rows.hip -o mgx_step_episode_rows_p.o
// so every other kernel comes out of the compiler exactly as it did without this file.
#include "mgx_episode_rows.hpp"

#ifndef MGX_STEP_EPISODE_ROWS_PART
#error "compile with -DMGX_STEP_EPISODE_ROWS_PART=<0..MGX_EPISODE_PARTS-1>"
#endif

// layouts (template parameter F) of this slice: MGX_EPISODE_FLAGS_<part> (mgx_kernels.hpp)
#define MGX_PART_FLAGS MGX_CAT(MGX_EPISODE_FLAGS_, MGX_STEP_EPISODE_ROWS_PART)

// depth of the action ring (steps of control loads in flight), as step_k_episodes_kernel's
#ifndef MGX_RING_STEP_EPISODES
#define MGX_RING_STEP_EPISODES 4
#endif

namespace mgx {

// Template parameters, rings, statistics and restart as step_k_episodes_kernel; the rows as rollout_episodes_rows_kernel writes
// them: final_obs[k, i, :] where step k restarts grid i (ring slot 0 after the rotation, under the old offset), obs[k, i, :] for
// every grid (slot 0 under the offset the restart left).  The row ring reaches one row further than the plain kernel's (row
// t0 + K: guards `<= K`); the action ring keeps its guard, there is no action row K.  SoC is formed every step.
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
    f.lr = 0.0; f.pr = 0.0; f.lp = 0u; f.pp = 0u; f.cp = 0u; f.pat = 0u;
    if constexpr (SRC == EP_SRC_FACT) load_factors<F>(a.c, i, f);
    RowBounds<F> rb;
    load_row_bounds<F>(a.c, N, i, rb);
    double run = es.ret_running ? es.ret_running[i] : 0.0;
    double sum = es.ret_sum ? es.ret_sum[i] : 0.0;
    double last = es.ret_last ? es.ret_last[i] : 0.0;
    int32_t eps = es.episodes ? es.episodes[i] : 0;
    {
        const bool GI = gen_instant;
        RowSlot ring[U];
        RawActions<AT> act[UA];
#pragma unroll
        for (int u = 0; u < U; u++)
            if (u <= K) fetch_row_slot<F, SRC>(a, f, i, t0 + u, off, ring[u]);
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
#pragma unroll
            for (int u = 0; u + 1 < U; u++) ring[u] = ring[u + 1];
#pragma unroll
            for (int u = 0; u + 1 < UA; u++) act[u] = act[u + 1];
            if (k + UA < K) { load_actions_at<F>(arow, i32, act[UA - 1]); arow += N * A_DIM; }
            Outputs o;
            step_core<F>(p, d, s, in, norm, true, GI, o);
            const double r = shaped_reward<F>(a.shaper, o);
            const bool dn = t >= fin - 1;                       // done_at(a, i, t)
            if (out.reward) out.reward[o64] = r;
            if (out.done) out.done[o64] = (uint8_t)dn;
            if constexpr (F & F_BATTERY) { if (out.soc_trace) out.soc_trace[o64] = s.soc; }
            if constexpr (F & F_GENSET) { if (out.status_trace) out.status_trace[o64] = s.status; }
            o64 += N;
            run += r;
            if (t == fin - 1) { last = run; sum += run; eps += 1; run = 0.0; }
            if (ar_on && dn) {
                const KArgs *__restrict__ a_dev = late->a_dev;
                if (want_final) {                               // the row of the episode that ends here: slot 0, still the old rows
                    Inputs inf;
                    widen_row_slot<F, SRC>(a, f, ring[0], t + 1, off, inf);
                    store_final_row<F>(a_dev, a.T, desc, late->final_obs, r64, i, t + 1 + off, inf, rb, p, s);
                }
                // (the arguments of the draw out of the handle's device copy of the KArgs, read here, in the branch)
                off = episode_auto_restart(*a_dev, i, t, off, true);
                fin = a_dev->ep_final[i];
                // row slot v now stands for step k + 1 + v: all of them again, at the rows of the new episode (the controls stay)
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
    if (double *q = late->es.ret_running) q[i] = run;
    if (double *q = late->es.ret_sum) q[i] = sum;
    if (double *q = late->es.ret_last) q[i] = last;
    if (int32_t *q = late->es.episodes) q[i] = eps;
}

template <int F, typename AT>
static void step_k_episodes_rows_dispatch(const EpisodeRowsLaunch &R)
{
    const EpisodeLaunch &L = R.e;
    // row ring as rollout_episodes_kernel's: a slot of a layout with a GridModule holds up to six values (depth 4), else two (depth 8)
    const StepRowsArgs g{*L.k, L.actions, L.t, L.K, L.normalized, L.gpb, L.out, L.stats, pack_row_desc(*L.k), L.k_dev, R.obs, R.final_obs};
#define MGX_STEP_EPISODES(SRC) step_k_episodes_rows_kernel<F, (F & F_GRID) ? 4 : MGX_RING_ROLLOUT, MGX_RING_STEP_EPISODES, AT, SRC><<<L.blocks, BLOCK_K, 0, L.stream>>>(g)
    if (L.src == EP_SRC_FACT) MGX_STEP_EPISODES(EP_SRC_FACT);
    else if (L.src == EP_SRC_GRID_MAJOR) MGX_STEP_EPISODES(EP_SRC_GRID_MAJOR);
    else MGX_STEP_EPISODES(EP_SRC_GATHER);
#undef MGX_STEP_EPISODES
}

bool MGX_CAT(launch_step_k_episodes_rows_p, MGX_STEP_EPISODE_ROWS_PART)(const EpisodeRowsLaunch &R)
{
    switch (R.e.flags) {
#define X(FV) case FV: if (R.e.act_f32) step_k_episodes_rows_dispatch<FV, float>(R); else step_k_episodes_rows_dispatch<FV, double>(R); return true;
        MGX_PART_FLAGS(X)
#undef X
        default: return false;
    }
}

}  // namespace mgx
