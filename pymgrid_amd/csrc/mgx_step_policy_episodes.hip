// mgx_step_policy_episodes.hip -- the CLOSED-LOOP fused continuous K-step over per-grid in-place episodes
// (mgx_step_k_policy_episodes): step_k_episodes_rows_kernel (mgx_step_episode_rows.hip) with the normalised controls of every step
// chosen inside the launch, by the policy of include/mgx.h applied to the row the grid stands on.  The continuous twin of
// rollout_policy_episodes_kernel (mgx_policy_episodes.hip).  One of the six translation units of mgx_episode_loop.hpp, which states
// what their loops share and how a unit is compiled; what the rows add is in mgx_episode_rows.hpp, the policy in mgx_policy.hpp.
// This loop with a head on the policy's outputs (exploring, Gaussian, Gaussian with a critic): mgx_step_policy_head_episodes.hip.
#include "mgx_policy.hpp"

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
    // THE RING OF THIS KERNEL IS WRITTEN OUT -- the lane's factors, the ring's fill, rotation and advance and the restart are the text
    // of load_lane_factors / fill_row_ring / rotate_ring / restart_lane + advance_row_ring (mgx_episode_loop.hpp, reach K + 1), not calls:
    // on the helpers the form <7, 4, GRID_MAJOR> took 2.98 us per step of 100 000 grids at K = 64 against 2.77 (+7.6 %, linear policy;
    // +4.0 % with 16 hidden units: profiles/exp_episode_loop_refactor.txt) while <7, 4, FACT> gained 2.7 %; which of the pieces moves it is not isolated.
    // A change to one of those helpers is made here too.
    GridFactors f;
    f.lr = 0.0; f.pr = 0.0; f.lp = 0u; f.pp = 0u; f.cp = 0u; f.pat = 0u;
    if constexpr (SRC == EP_SRC_FACT) load_factors<F>(a.c, i, f);
    RowBounds<F> rb;
    load_row_bounds<F>(a.c, N, i, rb);
    LaneStats st;
    st.load(es, i);
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
            store_step_outputs<F>(out, o64, r, dn, s);
            o64 += N;
            r64 += N * D;
            st.update(r, t, fin);
            if (ar_on && dn) {
                const KArgs *__restrict__ a_dev = late->a_dev;
                if (want_final) {                               // the row of the episode that ends here: slot 0, still the old rows
                    Inputs inf;
                    widen_row_slot<F, SRC>(a, f, ring[0], t + 1, off, inf);
                    store_final_row<F>(a_dev, a.T, desc, late->final_obs, r64, i, t + 1 + off, inf, rb, p, s);
                }
                off = episode_auto_restart(*a_dev, i, t, off, true);
                fin = a_dev->ep_final[i];
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
    st.store(late->es.ret_running, late->es.ret_sum, late->es.ret_last, late->es.episodes, i);
}

template <int F>
static void step_k_policy_episodes_dispatch(const EpisodePolicyLaunch &P)
{
    const EpisodeLaunch &L = P.r.e;
    const StepPolicyArgs g{*L.k, P.pol, L.t, L.K, L.gpb, pack_row_desc(*L.k), L.out, L.stats, L.k_dev, P.r.obs, P.r.final_obs,
                           (double *)P.actions_out};
    with_episode_src(L.src, [&](auto src) {
        step_k_policy_episodes_kernel<F, ROW_RING<F>, decltype(src)::value><<<L.blocks, BLOCK_K, P.lds_bytes, L.stream>>>(g);
    });
}

MGX_EPISODE_LAUNCH_FN(step_k_policy_episodes, EpisodePolicyLaunch, L.r.e.flags)

}  // namespace mgx
