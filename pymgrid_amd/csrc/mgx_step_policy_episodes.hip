// mgx_step_policy_episodes.hip -- the CLOSED-LOOP fused continuous K-step over per-grid in-place episodes
// (mgx_step_k_policy_episodes): step_k_episodes_rows_kernel (mgx_step_episode_rows.hip) with the normalised controls of every step
// chosen inside the launch, by the policy of include/mgx.h applied to the row the grid stands on.  The continuous twin of
// rollout_policy_episodes_kernel (mgx_policy_episodes.hip).  Translation units of their own (MGX_EPISODE_PARTS slices of the layouts):
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c -DMGX_STEP_POLICY_EPISODE_PART=p mgx_step_policy_episodes.hip -o mgx_step_policy_episodes_p.o
// so every other kernel comes out of the compiler exactly as it did without this file.
#include "mgx_policy.hpp"

#ifndef MGX_STEP_POLICY_EPISODE_PART
#error "compile with -DMGX_STEP_POLICY_EPISODE_PART=<0..MGX_EPISODE_PARTS-1>"
#endif

// layouts (template parameter F) of this slice: MGX_EPISODE_FLAGS_<part> (mgx_kernels.hpp)
#define MGX_PART_FLAGS MGX_CAT(MGX_EPISODE_FLAGS_, MGX_STEP_POLICY_EPISODE_PART)

namespace mgx {

// Template parameters, row ring, statistics, restart and final_obs as step_k_episodes_rows_kernel; there is no action stream and no
// action ring.  The row, the strip and obs as rollout_policy_episodes_kernel; the policy's A outputs, clipped to [0, 1], are the
// step's controls in the layout's action order (genset goal, genset, battery, grid) and the step takes them normalised.
template <int F, int U, int SRC>
__global__ __launch_bounds__(BLOCK_K) void step_k_policy_episodes_kernel(const StepPolicyArgs g)
{
    constexpr int D = policy_row_dim<F>();
    constexpr int A_DIM = 2 * ((F & F_GENSET) != 0) + ((F & F_BATTERY) != 0) + ((F & F_GRID) != 0);
    constexpr int NO = A_DIM > 0 ? A_DIM : 1;
    const KArgs &a = g.a;
    const int32_t t0 = g.t0, K = g.K, gpb = g.gpb;
    const FusedOut &out = g.out;
    const mgx_episode_stats &es = g.es;
    void *__restrict__ obs = g.obs;
    double *__restrict__ actions_out = g.actions_out;
    const bool want_final = g.final_obs != nullptr;
    uint32_t desc = g.desc;
    int32_t nh = g.pol.n_hidden;
    const auto *late = late_kernargs<StepPolicyArgs>();
    // one wave-private tile per wave: the lanes' row strips
    __shared__ __attribute__((aligned(16))) double row_tiles[(BLOCK_K / 64) * 64 * ROW_TILE_MAX_D];
    extern __shared__ __attribute__((aligned(16))) double policy_lds[];
    const int64_t i = (int64_t)blockIdx.x * gpb + threadIdx.x;
    stage_policy(g.pol, D, policy_lds);                         // (ends in the only barrier: before any lane leaves)
    if ((int32_t)threadIdx.x >= gpb || i >= a.N) return;
    double *tile = row_tiles + (threadIdx.x >> 6) * (64 * ROW_TILE_MAX_D);
    const double *my_set = policy_lds + policy_lane_offset(g.pol, i);
    const int64_t N = a.N;
    Params p; State s; Derived d;
    load_state<F>(a.c, i, true, s);              // (the SoC too: the first row shows it before any step has formed it)
    load_params<F>(a.c, i, p);
    derive<F>(p, d);
    const bool gen_instant = genset_wave_is_instant<F>(p, s);
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
#pragma unroll
        for (int u = 0; u < U; u++)
            if (u <= K) fetch_row_slot<F, SRC>(a, f, i, t0 + u, off, ring[u]);
        int64_t o64 = i;
        int64_t r64 = i * D - N * D;               // element offset of row (k - 1, i) of obs; + N * D: row (k, i) of final_obs
#pragma nounroll
        for (int32_t k = 0; k < K; k++) {
            const int32_t t = t0 + k;
            asm volatile("" : "+s"(desc));             // (opaque: the fields are taken out where a row is built, every step)
            asm volatile("" : "+s"(nh));
            Inputs in;
            widen_row_slot<F, SRC>(a, f, ring[0], t, off, in);
            {
                double x[D], y[NO];
                policy_row<F>(late->a_dev, a.T, desc, i, t + off, in, rb, p, s, tile, x);
                if (obs && k > 0) emit_policy_row<D>(desc, obs, r64, tile);
                policy_outputs<D, NO>(my_set, nh, A_DIM, x, y);
                int c = 0;
                if constexpr (F & F_GENSET) { in.a_goal = policy_clip(y[c]); in.a_gen = policy_clip(y[c + 1]); c += 2; }
                if constexpr (F & F_BATTERY) { in.a_bat = policy_clip(y[c]); c += 1; }
                if constexpr (F & F_GRID) { in.a_grid = policy_clip(y[c]); c += 1; }
                if constexpr (A_DIM > 0) {
                    if (actions_out) {
                        double *q = actions_out + o64 * A_DIM;
                        c = 0;
                        if constexpr (F & F_GENSET) { q[c] = in.a_goal; q[c + 1] = in.a_gen; c += 2; }
                        if constexpr (F & F_BATTERY) { q[c] = in.a_bat; c += 1; }
                        if constexpr (F & F_GRID) { q[c] = in.a_grid; c += 1; }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u + 1 < U; u++) ring[u] = ring[u + 1];
            Outputs o;
            step_core<F>(p, d, s, in, true, true, GI, o);
            const double r = shaped_reward<F>(a.shaper, o);
            const bool dn = t >= fin - 1;                       // done_at(a, i, t)
            if (out.reward) out.reward[o64] = r;
            if (out.done) out.done[o64] = (uint8_t)dn;
            if constexpr (F & F_BATTERY) { if (out.soc_trace) out.soc_trace[o64] = s.soc; }
            if constexpr (F & F_GENSET) { if (out.status_trace) out.status_trace[o64] = s.status; }
            o64 += N;
            r64 += N * D;
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
                // row slot v now stands for step k + 1 + v: all of them again, at the rows of the new episode
#pragma unroll
                for (int v = 0; v < U; v++)
                    if (k + 1 + v <= K) fetch_row_slot<F, SRC>(a, f, i, t + 1 + v, off, ring[v]);
            } else if (k + U <= K) {
                fetch_row_slot<F, SRC>(a, f, i, t + U, off, ring[U - 1]);
            }
        }
        if (obs) {                                              // the row the last step returned
            Inputs inn;
            double x[D];
            widen_row_slot<F, SRC>(a, f, ring[0], t0 + K, off, inn);
            policy_row<F>(late->a_dev, a.T, desc, i, t0 + K + off, inn, rb, p, s, tile, x);
            emit_policy_row<D>(desc, obs, r64, tile);
        }
    }
    store_state<F>(late->a_dev->c, i, s);     // (the same columns; their addresses need no scalar registers across the loop)
    // (the statistics' addresses a second time, from the kernarg segment: the first copies ended their lives before the loop)
    if (double *q = late->es.ret_running) q[i] = run;
    if (double *q = late->es.ret_sum) q[i] = sum;
    if (double *q = late->es.ret_last) q[i] = last;
    if (int32_t *q = late->es.episodes) q[i] = eps;
}

template <int F>
static void step_k_policy_episodes_dispatch(const EpisodePolicyLaunch &P)
{
    const EpisodeLaunch &L = P.r.e;
    // row ring as rollout_episodes_kernel's: a slot of a layout with a GridModule holds up to six values (depth 4), else two (depth 8)
    const StepPolicyArgs g{*L.k, P.pol, L.t, L.K, L.gpb, pack_row_desc(*L.k), L.out, L.stats, L.k_dev, P.r.obs, P.r.final_obs,
                           (double *)P.actions_out};
#define MGX_STEP_EPISODES(SRC) step_k_policy_episodes_kernel<F, (F & F_GRID) ? 4 : MGX_RING_ROLLOUT, SRC><<<L.blocks, BLOCK_K, P.lds_bytes, L.stream>>>(g)
    if (L.src == EP_SRC_FACT) MGX_STEP_EPISODES(EP_SRC_FACT);
    else if (L.src == EP_SRC_GRID_MAJOR) MGX_STEP_EPISODES(EP_SRC_GRID_MAJOR);
    else MGX_STEP_EPISODES(EP_SRC_GATHER);
#undef MGX_STEP_EPISODES
}

bool MGX_CAT(launch_step_k_policy_episodes_p, MGX_STEP_POLICY_EPISODE_PART)(const EpisodePolicyLaunch &P)
{
    switch (P.r.e.flags) {
#define X(FV) case FV: step_k_policy_episodes_dispatch<FV>(P); return true;
        MGX_PART_FLAGS(X)
#undef X
        default: return false;
    }
}

}  // namespace mgx
