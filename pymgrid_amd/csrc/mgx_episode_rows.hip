// mgx_episode_rows.hip -- the fused discrete roll-out over per-grid in-place episodes WITH observation rows
// (mgx_rollout_episodes_rows): rollout_episodes_kernel (mgx_episodes.hip) + per step the H = 0 row the step returned and, where a
// grid restarts, the row before the restart.  One of the six translation units of mgx_episode_loop.hpp, which states what their
// loops share and how a unit is compiled; what the rows add is in mgx_episode_rows.hpp.
#include "mgx_episode_rows.hpp"

namespace mgx {

// Template parameters, ring, statistics and restart as rollout_episodes_kernel.  What the rows add, per step k (counter t = t0 + k,
// row offset `off` before the step):
//   final_obs[k, i, :]   only where the step restarts grid i: the row of series row t + 1 + off with the post-step state -- the row
//                        episode_tail writes through mgx_set_final_obs.  After the rotation ring slot 0 holds exactly that series
//                        row, until the restart branch reads the slots again.
//   obs[k, i, :]         the row of series row t + 1 + off_new: ring slot 0 again, under the offset the restart left.
// Hence the ring here reaches ONE row further than the plain kernel's: K + 1 (the ring's reach, mgx_episode_loop.hpp).  The id ring
// keeps its guard: there is no id row K.
// SoC is formed every step (the row shows it).
// Scalar registers: rollout_episodes_kernel leaves five of them free.  So the arguments come as ONE struct and whatever is not
// needed inside the loop is read late, through late_kernargs: the statistics' addresses for the write-back, the device copy of the
// KArgs and final_obs inside the restart branch; the row's column bases travel packed in one word (RolloutRowsArgs.desc) that is
// kept opaque inside the loop, or its seven fields would be hoisted into seven registers again.
template <int F, int U, bool PER_STEP, int SRC>
__global__ __launch_bounds__(BLOCK_K) void rollout_episodes_rows_kernel(const RolloutRowsArgs g)
{
    static_assert(U <= 8, "the id ring is one 64-bit register");
    const KArgs &a = g.a;
    const PLWords &tab = g.tab;
    const uint8_t *__restrict__ ids = g.ids;
    const int32_t t0 = g.t0, K = g.K, gpb = g.gpb;
    const FusedOut &out = g.out;
    const mgx_episode_stats &es = g.es;
    void *__restrict__ obs = g.obs;
    const bool want_final = g.final_obs != nullptr;
    uint32_t desc = g.desc;
    const auto *late = late_kernargs<RolloutRowsArgs>();
    const int64_t i = (int64_t)blockIdx.x * gpb + threadIdx.x;
    __shared__ uint32_t word_of_id[PER_STEP ? BLOCK_K : 1];
    // one wave-private tile per wave for the rows of a step (store_episode_row)
    __shared__ __attribute__((aligned(16))) double row_tiles[MGX_EPISODE_ROWS_TILE ? (BLOCK_K / 64) * 64 * ROW_TILE_MAX_D : 1];
    if constexpr (PER_STEP) {
        static_assert(BLOCK_K == 256, "one thread per id byte");
        word_of_id[threadIdx.x] = pl_select(tab, (int32_t)threadIdx.x);
        __syncthreads();                                        // (the only barrier: before any lane leaves)
    }
    if ((int32_t)threadIdx.x >= gpb || i >= a.N) return;
    double *tile = row_tiles + (MGX_EPISODE_ROWS_TILE ? (threadIdx.x >> 6) * (64 * ROW_TILE_MAX_D) : 0);
    const int64_t N = a.N;
    const uint32_t i32 = (uint32_t)i;
    Params p; State s; Derived d;
    load_state<F>(a.c, i, false, s);
    load_params<F>(a.c, i, p);
    derive<F>(p, d);
    const bool gen_instant = genset_wave_is_instant<F>(p, s);
    const bool ar_on = a.ar_mode != 0;
    int32_t off = a.ep_off[i], fin = a.ep_final[i];
    uint32_t word = PER_STEP ? 0u : pl_select(tab, ids[i]);
    // THE RING OF THIS KERNEL IS WRITTEN OUT -- the lane's factors, the ring's fill, rotation and advance and the restart are the text
    // of load_lane_factors / fill_row_ring / rotate_ring / restart_lane + advance_row_ring (mgx_episode_loop.hpp, reach K + 1), not calls:
    // on the helpers the form <7, 4, *, GRID_MAJOR> took 4.66 us per step of 100 000 grids at K = 64 against 4.33-4.40 (+6.8 %:
    // profiles/exp_episode_loop_refactor.txt); the compiler's code differs in a few dozen instructions, which of the pieces costs the time is not isolated.
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
        uint64_t idq = 0;                 // PER_STEP: the id bytes of the U ring slots
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (u <= K) fetch_row_slot<F, SRC>(a, f, i, t0 + u, off, ring[u]);
            if constexpr (PER_STEP) { if (u < K) idq |= (uint64_t)(ids + (int64_t)u * N)[i32] << (8 * u); }
        }
        uint32_t word_next = 0u;
        if constexpr (PER_STEP) word_next = word_of_id[idq & 0xffu];
        int64_t o64 = i;
        int64_t r64 = i * row_desc_dim(desc);      // element offset of row (k, i) of obs / final_obs
#pragma nounroll
        for (int32_t k = 0; k < K; k++) {
            const int32_t t = t0 + k;
            asm volatile("" : "+s"(desc));             // (opaque: the fields are taken out where a row is built, every step)
            Inputs in;
            widen_row_slot<F, SRC>(a, f, ring[0], t, off, in);
#pragma unroll
            for (int u = 0; u + 1 < U; u++) ring[u] = ring[u + 1];
            if constexpr (PER_STEP) {
                word = word_next;
                idq >>= 8;
                word_next = word_of_id[idq & 0xffu];            // (the coming step's; beyond the last step: unused)
                if (k + U < K) idq |= (uint64_t)(ids + (int64_t)(k + U) * N)[i32] << (8 * (U - 1));
            } else {
                asm volatile("" : "+v"(word));                  // (the list decoding stays inside the loop: rollout_episodes_kernel)
            }
            double bat_q;
            uint32_t xv = 0u;
            populate_core<F, false>(p, s, word, in, bat_q, 0.0 + -1 * in.load, in.pv, GI, &xv);
            Outputs o;
            step_core<F, true>(p, d, s, in, false, true, GI, o, bat_q);
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
                off = episode_auto_restart(*a_dev, i, t, off, true);
                fin = a_dev->ep_final[i];
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

template <int F>
static void rollout_episodes_rows_dispatch(const EpisodeRowsLaunch &R)
{
    const EpisodeLaunch &L = R.e;
    const RolloutRowsArgs g{*L.k, *L.tab, L.ids, L.t, L.K, L.out, L.stats, L.gpb, pack_row_desc(*L.k), L.k_dev, R.obs, R.final_obs};
    with_episode_src(L.src, [&](auto src) {
        constexpr int SRC = decltype(src)::value;
        if (L.per_step) rollout_episodes_rows_kernel<F, ROW_RING<F>, true, SRC><<<L.blocks, BLOCK_K, 0, L.stream>>>(g);
        else rollout_episodes_rows_kernel<F, ROW_RING<F>, false, SRC><<<L.blocks, BLOCK_K, 0, L.stream>>>(g);
    });
}

MGX_EPISODE_LAUNCH_FN(rollout_episodes_rows, EpisodeRowsLaunch, L.e.flags)

}  // namespace mgx
