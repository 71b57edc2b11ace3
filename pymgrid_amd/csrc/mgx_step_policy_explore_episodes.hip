// mgx_step_policy_explore_episodes.hip -- the closed-loop fused continuous K-step with an EXPLORING head
// (mgx_step_k_policy_explore_episodes): step_k_policy_episodes_kernel (mgx_step_policy_episodes.hip) whose controls carry the
// additive noise of mgx_exploration (include/mgx.h) before their clip -- sigma[o] * scale[i] times a quantised twelve-uniform
// normal, by a counter-based draw of (seed, grid, step counter, action column).  The continuous twin of
// rollout_policy_explore_episodes_kernel (mgx_policy_explore_episodes.hip); a kernel of its own for the same reason.  Compiled as
// the units of mgx_episode_loop.hpp are; the policy and what exploration adds (explore_normal, policy_noisy_clip) in mgx_policy.hpp.
#include "mgx_policy.hpp"

namespace mgx {

// Everything as step_k_policy_episodes_kernel, with two differences.  (1) The controls: policy_noisy_clip in the place of
// policy_clip, one draw per action column, each formed next to the control it moves; seed and sigma[o] are read from the kernarg
// segment where they are used (late_kernargs), the lane carries scale[i] (one double, 1.0 where there is none).  (2) The ring of
// series rows goes through the helpers of mgx_episode_loop.hpp, as in rollout_policy_explore_episodes_kernel.
template <int F, int U, int SRC>
__global__ __launch_bounds__(BLOCK_K) void step_k_policy_explore_episodes_kernel(const StepPolicyExploreArgs gx)
{
    constexpr int D = policy_row_dim<F>();
    constexpr int A_DIM = 2 * ((F & F_GENSET) != 0) + ((F & F_BATTERY) != 0) + ((F & F_GRID) != 0);
    constexpr int NO = A_DIM > 0 ? A_DIM : 1;
    const StepPolicyArgs &g = gx.g;
    const KArgs &a = g.a;
    const int32_t t0 = g.t0, K = g.K, gpb = g.gpb;
    const FusedOut &out = g.out;
    const mgx_episode_stats &es = g.es;
    void *__restrict__ obs = g.obs;
    double *__restrict__ actions_out = g.actions_out;
    const bool want_final = g.final_obs != nullptr;
    uint32_t desc = g.desc;
    int32_t nh = g.pol.n_hidden;
    const auto *late = late_kernargs<StepPolicyExploreArgs>();
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
    const double sc_i = explore_lane_scale(gx.ex.scale, i);
    GridFactors f;
    load_lane_factors<F, SRC>(a.c, i, f);
    RowBounds<F> rb;
    load_row_bounds<F>(a.c, N, i, rb);
    LaneStats st;
    st.load(es, i);
    {
        const bool GI = gen_instant;
        RowSlot ring[U];
        fill_row_ring<F, SRC>(a, f, i, t0, off, K + 1, ring);
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
                policy_row<F>(late->g.a_dev, a.T, desc, i, t + off, in, rb, p, s, tile, x);
                if (obs && k > 0) emit_policy_row<D>(desc, obs, r64, tile);
                policy_outputs<D, NO>(my_set, nh, A_DIM, x, y);
                // control c of the layout's action order: y[c] + sigma[c] * scale[i] * z(t, c), clipped
                auto control = [&](int c) { return policy_noisy_clip(y[c], late->ex.sigma[c] * sc_i, late->ex.seed, i, t, (uint32_t)c); };
                int c = 0;
                if constexpr (F & F_GENSET) { in.a_goal = control(c); in.a_gen = control(c + 1); c += 2; }
                if constexpr (F & F_BATTERY) { in.a_bat = control(c); c += 1; }
                if constexpr (F & F_GRID) { in.a_grid = control(c); c += 1; }
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
            rotate_ring(ring);
            Outputs o;
            step_core<F>(p, d, s, in, true, true, GI, o);
            const double r = shaped_reward<F>(a.shaper, o);
            const bool dn = t >= fin - 1;                       // done_at(a, i, t)
            store_step_outputs<F>(out, o64, r, dn, s);
            o64 += N;
            r64 += N * D;
            st.update(r, t, fin);
            if (ar_on && dn) {
                const KArgs *__restrict__ a_dev = late->g.a_dev;
                if (want_final) {                               // the row of the episode that ends here: slot 0, still the old rows
                    Inputs inf;
                    widen_row_slot<F, SRC>(a, f, ring[0], t + 1, off, inf);
                    store_final_row<F>(a_dev, a.T, desc, late->g.final_obs, r64, i, t + 1 + off, inf, rb, p, s);
                }
                restart_lane(a_dev, i, t, off, fin);
                advance_row_ring<F, SRC>(a, f, i, t, k, off, K + 1, true, ring);
            } else {
                advance_row_ring<F, SRC>(a, f, i, t, k, off, K + 1, false, ring);
            }
        }
        if (obs) {                                              // the row the last step returned
            Inputs inn;
            double x[D];
            widen_row_slot<F, SRC>(a, f, ring[0], t0 + K, off, inn);
            policy_row<F>(late->g.a_dev, a.T, desc, i, t0 + K + off, inn, rb, p, s, tile, x);
            emit_policy_row<D>(desc, obs, r64, tile);
        }
    }
    store_state<F>(late->g.a_dev->c, i, s);   // (the same columns; their addresses need no scalar registers across the loop)
    // (the statistics' addresses a second time, from the kernarg segment: the first copies ended their lives before the loop)
    st.store(late->g.es.ret_running, late->g.es.ret_sum, late->g.es.ret_last, late->g.es.episodes, i);
}

template <int F>
static void step_k_policy_explore_episodes_dispatch(const EpisodePolicyLaunch &P)
{
    const EpisodeLaunch &L = P.r.e;
    const StepPolicyExploreArgs gx{{*L.k, P.pol, L.t, L.K, L.gpb, pack_row_desc(*L.k), L.out, L.stats, L.k_dev, P.r.obs, P.r.final_obs,
                                    (double *)P.actions_out}, P.ex};
    with_episode_src(L.src, [&](auto src) {
        step_k_policy_explore_episodes_kernel<F, ROW_RING<F>, decltype(src)::value><<<L.blocks, BLOCK_K, P.lds_bytes, L.stream>>>(gx);
    });
}

MGX_EPISODE_LAUNCH_FN(step_k_policy_explore_episodes, EpisodePolicyLaunch, L.r.e.flags)

}  // namespace mgx
