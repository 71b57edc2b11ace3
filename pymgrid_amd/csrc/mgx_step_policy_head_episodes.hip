// mgx_step_policy_head_episodes.hip -- the closed-loop fused continuous K-step with a HEAD on the policy's outputs:
// step_k_policy_episodes_kernel (mgx_step_policy_episodes.hip) whose controls are, by HEAD (PolicyHead, mgx_policy.hpp),
//   HEAD_EXPLORE (mgx_step_k_policy_explore_episodes): the outputs with the additive noise of mgx_exploration (include/mgx.h) before
//     their clip -- sigma[o] * scale[i] times a quantised twelve-uniform normal, by a counter-based draw of (seed, grid, step
//     counter, action column);
//   HEAD_GAUSSIAN (mgx_step_k_policy_gaussian_episodes): drawn from N(y[o], s[o]^2) by the rule of mgx_gaussian -- a true normal
//     draw by Box-Muller on a log, a sine and a cosine that are fixed sequences of IEEE operations -- and returned with the pre-clip
//     action and its exact log-density;
//   HEAD_GAUSSIAN_CRITIC (the same call with a mgx_critic): that, and the value head of the policy's trunk, as the discrete
//     HEAD_SAMPLE_CRITIC returns it.  What A2C and PPO need of a collector on the continuous head.
// The continuous twin of mgx_policy_head_episodes.hip: ONE kernel text, the head a template argument and what a head does not have
// under `if constexpr` where the statement stands; every instantiation is, instruction for instruction, the kernel that head had to
// itself (profiles/exp_policy_heads_refactor.txt).  The greedy kernel stays apart, as there.  Compiled as the units of
// mgx_episode_loop.hpp are, one object per head and slice (-DMGX_POLICY_HEAD=h -DMGX_EPISODE_PART=p); the heads (explore_normal,
// policy_noisy_clip; policy_log, policy_quarter_turn, gaussian_pair, policy_gaussian_head) and the critic's pieces in mgx_policy.hpp.
#include "mgx_policy.hpp"

namespace mgx {

// Everything as step_k_policy_episodes_kernel, on the ring helpers of mgx_episode_loop.hpp.  The controls: HEAD_EXPLORE
// policy_noisy_clip in the place of policy_clip, one draw per action column, each formed next to the control it moves; the Gaussian
// heads policy_gaussian_head -- one draw per PAIR of action columns, made only where a column of the pair is live -- and two more
// streams, raw_out [K, N, A] and logp_out [K, N], their addresses read where they are stored.  Seed and sigma[o] are read from the
// kernarg segment where they are used (late_kernargs); the lane carries scale[i] (1.0 where there is none) and, Gaussian, C_i
// (gaussian_lane_const) across the loop.  HEAD_GAUSSIAN_CRITIC: the staged sets hold the critic (stage_policy_critic), V is one more
// running sum beside y[] (policy_outputs_value), the final row's value a second trunk evaluation inside the restart branch only,
// last_value one evaluation after the loop -- each step as in rollout_policy_head_episodes_kernel.  A head of its own, not pointer
// tests in one: the form without a critic keeps the smaller staged sets (and their LDS bound) and pays nothing for the running sum
// (NOTES.md has the compiler's figures of both).
template <int F, int U, int SRC, int HEAD>
__global__ __launch_bounds__(BLOCK_K) void step_k_policy_head_episodes_kernel(const StepPolicyHeadArgs<HEAD> gx)
{
    constexpr int D = policy_row_dim<F>();
    constexpr int A_DIM = 2 * ((F & F_GENSET) != 0) + ((F & F_BATTERY) != 0) + ((F & F_GRID) != 0);
    constexpr int NO = A_DIM > 0 ? A_DIM : 1;
    constexpr bool EXPLORE = HEAD == HEAD_EXPLORE, CRITIC = HEAD == HEAD_GAUSSIAN_CRITIC;
    const StepPolicyArgs &g = greedy_part(gx);
    const KArgs &a = g.a;
    const int32_t t0 = g.t0, K = g.K, gpb = g.gpb;
    const FusedOut &out = g.out;
    const mgx_episode_stats &es = g.es;
    void *__restrict__ obs = g.obs;
    double *__restrict__ actions_out = g.actions_out;
    const bool want_final = g.final_obs != nullptr;
    uint32_t desc = g.desc;
    int32_t nh = g.pol.n_hidden;
    const auto *late = late_kernargs<StepPolicyHeadArgs<HEAD>>();
    // one wave-private tile per wave: the lanes' row strips
    __shared__ __attribute__((aligned(16))) double row_tiles[(BLOCK_K / 64) * 64 * ROW_TILE_MAX_D];
    extern __shared__ __attribute__((aligned(16))) double policy_lds[];
    const int64_t i = (int64_t)blockIdx.x * gpb + threadIdx.x;
    if constexpr (CRITIC) stage_policy_critic(g.pol, gx.cr, D, policy_lds);   // (ends in the only barrier: before any lane leaves)
    else stage_policy(g.pol, D, policy_lds);
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
    double sc_i;
    if constexpr (EXPLORE) sc_i = explore_lane_scale(gx.ex.scale, i);
    else sc_i = explore_lane_scale(gx.gs.scale, i);
    auto sigma = [&](int c) { if constexpr (EXPLORE) return late->ex.sigma[c]; else return late->gs.sigma[c]; };
    [[maybe_unused]] double C_i;
    if constexpr (!EXPLORE) C_i = gaussian_lane_const<A_DIM>(sigma, sc_i);
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
                policy_row<F>(greedy_part(*late).a_dev, a.T, desc, i, t + off, in, rb, p, s, tile, x);
                if (obs && k > 0) emit_policy_row<D>(desc, obs, r64, tile);
                if constexpr (CRITIC) {
                    double val;
                    policy_outputs_value<D, NO>(my_set, nh, A_DIM, x, y, val);
                    double *__restrict__ value_out = late->value_out;
                    if (value_out) value_out[o64] = val;
                } else {
                    policy_outputs<D, NO>(my_set, nh, A_DIM, x, y);
                }
                if constexpr (EXPLORE) {
                    // control c of the layout's action order: y[c] + sigma[c] * scale[i] * z(t, c), clipped
                    auto control = [&](int c) { return policy_noisy_clip(y[c], sigma(c) * sc_i, late->ex.seed, i, t, (uint32_t)c); };
                    int c = 0;
                    if constexpr (F & F_GENSET) { in.a_goal = control(c); in.a_gen = control(c + 1); c += 2; }
                    if constexpr (F & F_BATTERY) { in.a_bat = control(c); c += 1; }
                    if constexpr (F & F_GRID) { in.a_grid = control(c); c += 1; }
                } else {
                    // raw[c] = y[c] + sigma[c] * scale[i] * z(t, c) on the live columns: stored and clipped into control c of the layout's
                    // action order pair by pair (c is a constant wherever this is inlined); the log-density of the whole draw
                    double *__restrict__ raw_out = late->raw_out;
                    auto control = [&](int c, double raw) {
                        if (raw_out) raw_out[o64 * A_DIM + c] = raw;
                        const double u = policy_clip(raw);
                        constexpr int GEN = (F & F_GENSET) ? 2 : 0, BAT = (F & F_BATTERY) ? 1 : 0;
                        if constexpr (F & F_GENSET) { if (c == 0) in.a_goal = u; if (c == 1) in.a_gen = u; }
                        if constexpr (F & F_BATTERY) { if (c == GEN) in.a_bat = u; }
                        if constexpr (F & F_GRID) { if (c == GEN + BAT) in.a_grid = u; }
                    };
                    const double logp = policy_gaussian_head<A_DIM, NO>(y, sigma, sc_i, C_i, late->gs.seed, i, t, control);
                    double *__restrict__ logp_out = late->logp_out;
                    if (logp_out) logp_out[o64] = logp;
                }
                if constexpr (A_DIM > 0) {
                    if (actions_out) {
                        double *q = actions_out + o64 * A_DIM;
                        int c = 0;
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
                const KArgs *__restrict__ a_dev = greedy_part(*late).a_dev;
                double *__restrict__ final_value_out = nullptr;
                if constexpr (CRITIC) final_value_out = late->final_value_out;
                if (want_final || final_value_out) {            // the row of the episode that ends here: slot 0, still the old rows
                    Inputs inf;
                    widen_row_slot<F, SRC>(a, f, ring[0], t + 1, off, inf);
                    if (want_final) store_final_row<F>(a_dev, a.T, desc, greedy_part(*late).final_obs, r64, i, t + 1 + off, inf, rb, p, s);
                    if constexpr (CRITIC) {
                        if (final_value_out) {                  // ... once more into the lane's strip (the tile is free here), and V of it
                            double xf[D];
                            policy_row<F>(a_dev, a.T, desc, i, t + 1 + off, inf, rb, p, s, tile, xf);
                            final_value_out[o64 - N] = policy_value<D>(my_set, nh, A_DIM, xf);
                        }
                    }
                }
                restart_lane(a_dev, i, t, off, fin);
                advance_row_ring<F, SRC>(a, f, i, t, k, off, K + 1, true, ring);
            } else {
                advance_row_ring<F, SRC>(a, f, i, t, k, off, K + 1, false, ring);
            }
        }
        double *__restrict__ last_value_out = nullptr;
        if constexpr (CRITIC) last_value_out = late->last_value_out;
        if (obs || last_value_out) {                            // the row the last step returned
            Inputs inn;
            double x[D];
            widen_row_slot<F, SRC>(a, f, ring[0], t0 + K, off, inn);
            policy_row<F>(greedy_part(*late).a_dev, a.T, desc, i, t0 + K + off, inn, rb, p, s, tile, x);
            if (obs) emit_policy_row<D>(desc, obs, r64, tile);
            if constexpr (CRITIC) {
                if (last_value_out) last_value_out[i] = policy_value<D>(my_set, nh, A_DIM, x);
            }
        }
    }
    const auto &lg = greedy_part(*late);
    store_state<F>(lg.a_dev->c, i, s);          // (the same columns; their addresses need no scalar registers across the loop)
    // (the statistics' addresses a second time, from the kernarg segment: the first copies ended their lives before the loop)
    st.store(lg.es.ret_running, lg.es.ret_sum, lg.es.ret_last, lg.es.episodes, i);
}

// the head's struct: the greedy kernel's, filled here for every head, and what the head adds behind it
template <int F, int HEAD>
static void step_k_policy_head_episodes_dispatch(const EpisodePolicyLaunch &P)
{
    const EpisodeLaunch &L = P.r.e;
    const StepPolicyArgs g{*L.k, P.pol, L.t, L.K, L.gpb, pack_row_desc(*L.k), L.out, L.stats, L.k_dev, P.r.obs, P.r.final_obs,
                           (double *)P.actions_out};
    const StepPolicyHeadArgs<HEAD> gx = [&] {
        if constexpr (HEAD == HEAD_EXPLORE) return StepPolicyExploreArgs{g, P.ex};
        else return StepPolicyGaussianArgs{g, P.gs, P.raw_out, P.logp_out, P.cr, P.value_out, P.final_value_out, P.last_value_out};
    }();
    with_episode_src(L.src, [&](auto src) {
        step_k_policy_head_episodes_kernel<F, ROW_RING<F>, decltype(src)::value, HEAD><<<L.blocks, BLOCK_K, P.lds_bytes, L.stream>>>(gx);
    });
}

#if !defined(MGX_POLICY_HEAD) || (MGX_POLICY_HEAD != 1 && MGX_POLICY_HEAD != 4 && MGX_POLICY_HEAD != 5)
#error "compile with -DMGX_POLICY_HEAD=<1, 4 or 5> (PolicyHead: exploring, Gaussian, Gaussian with a critic)"
#endif
template <>
bool launch_step_k_policy_head_episodes<MGX_POLICY_HEAD, MGX_EPISODE_PART>(const EpisodePolicyLaunch &L)
{
    return with_part_layout(L.r.e.flags, [&](auto layout) { step_k_policy_head_episodes_dispatch<decltype(layout)::value, MGX_POLICY_HEAD>(L); });
}

}  // namespace mgx
