// mgx_policy_head_episodes.hip -- the closed-loop fused discrete roll-out with a HEAD on the policy's outputs:
// rollout_policy_episodes_kernel (mgx_policy_episodes.hip) whose id of every step is, by HEAD (PolicyHead, mgx_policy.hpp),
//   HEAD_EXPLORE (mgx_rollout_policy_explore_episodes): the epsilon-greedy choice of mgx_exploration (include/mgx.h) -- the greedy
//     id, or with probability epsilon * scale[i] one of the table's ids, by a counter-based draw of (seed, grid, step counter);
//   HEAD_SAMPLE (mgx_rollout_policy_sample_episodes): drawn from softmax(y / tau) by the rule of mgx_sampling -- exp as a fixed
//     sequence of IEEE operations, the inverse CDF on the unnormalised weights with such a draw -- and returned with its probability;
//   HEAD_SAMPLE_CRITIC (mgx_rollout_policy_critic_episodes): that, and the value head of mgx_critic on the trunk of the policy -- V
//     of the row every id was chosen on, of the last row of every episode that ends inside the launch and of the row the last step
//     returned: what A2C and PPO need of a collector beside the ids and their probabilities.
// ONE kernel text, the head a template argument and what a head does not have under `if constexpr` where the statement stands: every
// instantiation is, instruction for instruction, the kernel that head had to itself (profiles/exp_policy_heads_refactor.txt; a body
// function behind kernels of the old names is not: the same file).  The greedy kernel stays apart: it keeps the ring's text written
// out, for the reason its file states.  Compiled as the units of mgx_episode_loop.hpp are, one object per head and slice
// (-DMGX_POLICY_HEAD=h -DMGX_EPISODE_PART=p); the policy and what the heads add (explore_draw, policy_epsilon_greedy, policy_exp,
// policy_sample, stage_policy_critic, policy_outputs_value, policy_value) in mgx_policy.hpp.
#include "mgx_policy.hpp"

namespace mgx {

// Everything as rollout_policy_episodes_kernel, on the ring helpers of mgx_episode_loop.hpp (load_lane_factors, fill_row_ring,
// rotate_ring, restart_lane, advance_row_ring; reach K + 1) instead of their text: the draws dominate what these kernels add.
// The id: HEAD_EXPLORE policy_argmax, then policy_epsilon_greedy on it -- the draw is formed after the outputs are dead and before
// the step begins, so it holds no register across either; the sampling heads policy_sample -- the weights are written over the
// outputs in place, the draw is formed after they are summed -- and prob_out, one more [K, N] stream beside the ids.  The seed is
// read from the kernarg segment where it is used (late_kernargs); the lane carries one double, epsilon * scale[i] or
// beta = 1 / (temperature * scale[i]).  HEAD_SAMPLE_CRITIC: (1) the staged sets hold the critic's bias beside b2 and its weight in
// every unit's record (stage_policy_critic), and V is one more running sum beside y[] (policy_outputs_value): one [K, N] store per
// step, value_out.  (2) In the restart branch -- divergent already -- the final row is built once more into the lane's strip of the
// tile, which is free there, and the trunk evaluated on it (policy_value), only where final_value_out is given; the entries of
// grids that do not restart are not written.  (3) After the loop one evaluation on the row the last step returned, last_value_out.
// The critic's addresses are read from the kernarg segment where they are used.  Register figures per head: DESIGN.md's kernel table.
template <int F, int U, int SRC, int HEAD>
__global__ __launch_bounds__(BLOCK_K) void rollout_policy_head_episodes_kernel(const RolloutPolicyHeadArgs<HEAD> gx)
{
    constexpr int D = policy_row_dim<F>();
    constexpr int NO = 12;                                      // ids of a PLWords table
    constexpr bool EXPLORE = HEAD == HEAD_EXPLORE, CRITIC = HEAD == HEAD_SAMPLE_CRITIC;
    const RolloutPolicyArgs &g = greedy_part(gx);
    const KArgs &a = g.a;
    const int32_t t0 = g.t0, K = g.K, gpb = g.gpb;
    const FusedOut &out = g.out;
    const mgx_episode_stats &es = g.es;
    void *__restrict__ obs = g.obs;
    uint8_t *__restrict__ ids_out = g.ids_out;
    double *__restrict__ prob_out = nullptr;
    if constexpr (!EXPLORE) prob_out = sampling_part(gx).prob_out;
    double *__restrict__ value_out = nullptr;
    if constexpr (CRITIC) value_out = gx.value_out;
    const bool want_final = g.final_obs != nullptr;
    uint32_t desc = g.desc;
    uint32_t dims = (uint32_t)g.pol.n_hidden | (uint32_t)g.pol.n_out << 8 | (uint32_t)g.pol.n_real << 16;
    const auto *late = late_kernargs<RolloutPolicyHeadArgs<HEAD>>();
    const int64_t i = (int64_t)blockIdx.x * gpb + threadIdx.x;
    __shared__ uint32_t word_of_id[NO];
    // one wave-private tile per wave: the lanes' row strips
    __shared__ __attribute__((aligned(16))) double row_tiles[(BLOCK_K / 64) * 64 * ROW_TILE_MAX_D];
    extern __shared__ __attribute__((aligned(16))) double policy_lds[];
    if (threadIdx.x < NO) word_of_id[threadIdx.x] = pl_select(g.tab, (int32_t)threadIdx.x);
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
    double head_i;                               // eps_i = epsilon * scale[i], or beta_i
    if constexpr (EXPLORE) head_i = gx.ex.epsilon * explore_lane_scale(gx.ex.scale, i);
    else head_i = sample_lane_beta(sampling_part(gx).sa, i);
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
            asm volatile("" : "+s"(dims));
            Inputs in;
            widen_row_slot<F, SRC>(a, f, ring[0], t, off, in);
            uint32_t word;
            {
                double x[D], y[NO];
                policy_row<F>(greedy_part(*late).a_dev, a.T, desc, i, t + off, in, rb, p, s, tile, x);
                if (obs && k > 0) emit_policy_row<D>(desc, obs, r64, tile);
                if constexpr (CRITIC) {
                    double val;
                    policy_outputs_value<D, NO>(my_set, (int32_t)(dims & 0xffu), (int32_t)((dims >> 8) & 0xffu), x, y, val);
                    if (value_out) value_out[o64] = val;
                } else {
                    policy_outputs<D, NO>(my_set, (int32_t)(dims & 0xffu), (int32_t)((dims >> 8) & 0xffu), x, y);
                }
                int32_t id;
                [[maybe_unused]] double prob;
                if constexpr (EXPLORE) {
                    const int32_t greedy = policy_argmax<NO>(y, (int32_t)(dims >> 16));
                    id = policy_epsilon_greedy(greedy, (int32_t)(dims >> 16), head_i, late->ex.seed, i, t);
                } else {
                    id = policy_sample<NO>(y, (int32_t)(dims >> 16), head_i, sampling_part(*late).sa.seed, i, t, prob);
                }
                word = word_of_id[id];
                if (ids_out) ids_out[o64] = (uint8_t)id;
                if constexpr (!EXPLORE) {
                    if (prob_out) prob_out[o64] = prob;
                }
            }
            rotate_ring(ring);
            double bat_q;
            uint32_t xv = 0u;
            populate_core<F, false>(p, s, word, in, bat_q, 0.0 + -1 * in.load, in.pv, GI, &xv);
            Outputs o;
            step_core<F, true>(p, d, s, in, false, true, GI, o, bat_q);
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
                            final_value_out[o64 - N] = policy_value<D>(my_set, (int32_t)(dims & 0xffu), (int32_t)((dims >> 8) & 0xffu), xf);
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
                if (last_value_out) last_value_out[i] = policy_value<D>(my_set, (int32_t)(dims & 0xffu), (int32_t)((dims >> 8) & 0xffu), x);
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
static void rollout_policy_head_episodes_dispatch(const EpisodePolicyLaunch &P)
{
    const EpisodeLaunch &L = P.r.e;
    const RolloutPolicyArgs g{*L.k, *L.tab, P.pol, L.t, L.K, L.out, L.stats, L.gpb, pack_row_desc(*L.k), L.k_dev, P.r.obs,
                              P.r.final_obs, (uint8_t *)P.actions_out};
    const RolloutPolicyHeadArgs<HEAD> gx = [&] {
        if constexpr (HEAD == HEAD_EXPLORE) return RolloutPolicyExploreArgs{g, P.ex};
        else if constexpr (HEAD == HEAD_SAMPLE) return RolloutPolicySampleArgs{g, P.sa, P.prob_out};
        else return RolloutPolicyCriticArgs{{g, P.sa, P.prob_out}, P.cr, P.value_out, P.final_value_out, P.last_value_out};
    }();
    with_episode_src(L.src, [&](auto src) {
        rollout_policy_head_episodes_kernel<F, ROW_RING<F>, decltype(src)::value, HEAD><<<L.blocks, BLOCK_K, P.lds_bytes, L.stream>>>(gx);
    });
}

#if !defined(MGX_POLICY_HEAD) || MGX_POLICY_HEAD < 1 || MGX_POLICY_HEAD > 3
#error "compile with -DMGX_POLICY_HEAD=<1..3> (PolicyHead: exploring, sampling, sampling with a critic)"
#endif
template <>
bool launch_rollout_policy_head_episodes<MGX_POLICY_HEAD, MGX_EPISODE_PART>(const EpisodePolicyLaunch &L)
{
    return with_part_layout(L.r.e.flags, [&](auto layout) { rollout_policy_head_episodes_dispatch<decltype(layout)::value, MGX_POLICY_HEAD>(L); });
}

}  // namespace mgx
