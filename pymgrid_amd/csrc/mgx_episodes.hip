// mgx_episodes.hip -- the fused discrete roll-out over per-grid in-place episodes (mgx_rollout_episodes): K steps per launch,
// the priority list expanded in the kernel, every lane on the rows of its OWN episode and restarting inside the launch.
// One of the six translation units of mgx_episode_loop.hpp, which states what their loops share and how a unit is compiled.
#include "mgx_episode_loop.hpp"

namespace mgx {

// F: layout.  U: ring depth (steps of loads in flight).  PER_STEP: ids [K, N] (else one id per grid, the list decoding hoisted out
// of the loop).  SRC: where the rows come from (EP_SRC_*: fetch_row_slot).
// The shared counter of this mode never ends; `done` is the lane's own (counter >= ep_final[i] - 1, done_at's test on a register
// copy of ep_final[i] that a restart refreshes).  After every step: the statistics, then episode_auto_restart with the counter value
// of the step -- the call step_body<F, true> makes -- so K steps here leave what K single steps leave.
// A restart moves the lane to other rows: advance_row_ring reads the ring again under the new offset.
template <int F, int U, bool PER_STEP, int SRC>
__global__ __launch_bounds__(BLOCK_K) void rollout_episodes_kernel(const KArgs a, const PLWords tab, const uint8_t *__restrict__ ids,
                                                                   int32_t t0, int32_t K, const FusedOut out,
                                                                   const mgx_episode_stats es, int32_t gpb,
                                                                   const KArgs *__restrict__ a_dev)
{
    static_assert(U <= 8, "the id ring is one 64-bit register");
    const int64_t i = (int64_t)blockIdx.x * gpb + threadIdx.x;
    // PER_STEP: the list words of all 256 id bytes in LDS (ids outside the table: list 0, as pl_select) -- a step looks its word up
    // with one ds_read, a step ahead; the table in kernel arguments is 13 scalar registers live across the loop and a select chain
    __shared__ uint32_t word_of_id[PER_STEP ? BLOCK_K : 1];
    if constexpr (PER_STEP) {
        static_assert(BLOCK_K == 256, "one thread per id byte");
        word_of_id[threadIdx.x] = pl_select(tab, (int32_t)threadIdx.x);
        __syncthreads();                                        // (the only barrier: before any lane leaves)
    }
    if ((int32_t)threadIdx.x >= gpb || i >= a.N) return;
    const int64_t N = a.N;
    const uint32_t i32 = (uint32_t)i;
    Params p; State s; Derived d;
    load_state<F>(a.c, i, false, s);
    load_params<F>(a.c, i, p);
    derive<F>(p, d);
    const bool gen_instant = genset_wave_is_instant<F>(p, s);
    const bool want_soc = out.soc_trace != nullptr;
    const bool ar_on = a.ar_mode != 0;
    int32_t off = a.ep_off[i], fin = a.ep_final[i];
    uint32_t word = PER_STEP ? 0u : pl_select(tab, ids[i]);
    GridFactors f;
    load_lane_factors<F, SRC>(a.c, i, f);
    LaneStats st;
    st.load(es, i);

    // One loop; `gen_instant` stays a run-time (wave-uniform) flag: the two compile-time forms rollout_kernel keeps cost this kernel
    // scalar-register spills.  The ring rotates (rotate_ring), so the loop body exists once, not once per slot as in rollout_kernel.
    {
        const bool GI = gen_instant;
        RowSlot ring[U];
        fill_row_ring<F, SRC>(a, f, i, t0, off, K, ring);
        uint64_t idq = 0;                 // PER_STEP: the id bytes of the U ring slots (an array would live in scratch memory)
        if constexpr (PER_STEP) {
#pragma unroll
            for (int u = 0; u < U; u++)
                if (u < K) idq |= (uint64_t)(ids + (int64_t)u * N)[i32] << (8 * u);
        }
        uint32_t word_next = 0u;
        if constexpr (PER_STEP) word_next = word_of_id[idq & 0xffu];
        int64_t o64 = i;
#pragma nounroll
        for (int32_t k = 0; k < K; k++) {
            const int32_t t = t0 + k;
            Inputs in;
            widen_row_slot<F, SRC>(a, f, ring[0], t, off, in);
            rotate_ring(ring);
            if constexpr (PER_STEP) {
                word = word_next;
                idq >>= 8;
                word_next = word_of_id[idq & 0xffu];            // (the coming step's; beyond the last step: unused)
                if (k + U < K) idq |= (uint64_t)(ids + (int64_t)(k + U) * N)[i32] << (8 * (U - 1));
            } else {
                // a fixed list: its decoding stays INSIDE the loop (hoisted, the per-lane conditions of the three list elements
                // live in scalar-register pairs across the loop -- 20 to 30 spilled registers with genset + battery + grid)
                asm volatile("" : "+v"(word));
            }
            double bat_q;
            uint32_t xv = 0u;
            populate_core<F, false>(p, s, word, in, bat_q, 0.0 + -1 * in.load, in.pv, GI, &xv);
            Outputs o;
            step_core<F, true>(p, d, s, in, false, want_soc, GI, o, bat_q);
            const double r = shaped_reward<F>(a.shaper, o);
            const bool dn = t >= fin - 1;                       // done_at(a, i, t)
            store_step_outputs<F>(out, o64, r, dn, s);
            o64 += N;
            st.update(r, t, fin);
            if (ar_on && dn) {
                restart_lane(a_dev, i, t, off, fin);
                advance_row_ring<F, SRC>(a, f, i, t, k, off, K, true, ring);
            } else {
                advance_row_ring<F, SRC>(a, f, i, t, k, off, K, false, ring);
            }
        }
    }
    if constexpr (F & F_BATTERY) { if (!want_soc) s.soc = s.charge / p.bat_cmax; }
    store_state<F>(a_dev->c, i, s);           // (the same columns; their addresses need no scalar registers across the loop)
    st.store(es.ret_running, es.ret_sum, es.ret_last, es.episodes, i);
}

template <int F>
static void rollout_episodes_dispatch(const EpisodeLaunch &L)
{
    with_episode_src(L.src, [&](auto src) {
        constexpr int SRC = decltype(src)::value, U = ROW_RING<F>;
        if (L.per_step)
            rollout_episodes_kernel<F, U, true, SRC><<<L.blocks, BLOCK_K, 0, L.stream>>>(*L.k, *L.tab, L.ids, L.t, L.K, L.out, L.stats, L.gpb, L.k_dev);
        else
            rollout_episodes_kernel<F, U, false, SRC><<<L.blocks, BLOCK_K, 0, L.stream>>>(*L.k, *L.tab, L.ids, L.t, L.K, L.out, L.stats, L.gpb, L.k_dev);
    });
}

MGX_EPISODE_LAUNCH_FN(rollout_episodes, EpisodeLaunch, L.flags)

}  // namespace mgx
