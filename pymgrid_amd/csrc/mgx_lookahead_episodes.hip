// mgx_lookahead_episodes.hip -- the discrete what-if launch over per-grid in-place episodes (mgx_lookahead_episodes): C candidate
// plans of priority-list ids per grid, simulated at most H steps ahead from the handle's current state, none of them committed.
// A sibling of rollout_episodes_kernel (mgx_episodes.hip) on the pieces of mgx_episode_loop.hpp; mgx_lookahead.hpp states the
// mapping and what the two what-if units share.  Compiled like the other episode units (-DMGX_EPISODE_PART=p).
#include "mgx_lookahead.hpp"

namespace mgx {

// F: layout.  U: depth of the row ring.  PER_GRID: plans [C, H, N] (else [C, H]: the id of a step is wave-uniform, a scalar load
// and pl_select's select chain on scalar registers).  SRC: where the rows come from (EP_SRC_*: fetch_row_slot).
// The lane of (grid i, candidate c0 + blockIdx.y) takes lookahead_steps steps -- populate_core<F, false>, step_core<F, true>,
// shaped_reward<F>, the arithmetic of rollout_episodes_kernel's step on the same operands -- on a register copy of the grid's state
// and leaves ret[c, i] (and the SoC soc_trace would hold at the last counted step: charge / max_capacity, step_core's own
// quotient).  The ring never reaches beyond the lane's last step: reach = its step count, the non-restarting arm of
// advance_row_ring only.
template <int F, int U, bool PER_GRID, int SRC>
__global__ __launch_bounds__(BLOCK_K) void lookahead_episodes_kernel(const KArgs a, const PLWords tab, const uint8_t *__restrict__ plans,
                                                                     int32_t t0, int32_t H, int32_t c0, double gamma,
                                                                     double *__restrict__ ret, double *__restrict__ end_soc, int32_t gpb)
{
    static_assert(U <= 8, "the id ring is one 64-bit register");
    const int64_t i = (int64_t)blockIdx.x * gpb + threadIdx.x;
    const int64_t c = (int64_t)c0 + blockIdx.y;
    // PER_GRID: the list words of all 256 id bytes in LDS, as rollout_episodes_kernel's per-step form (ids outside the table: list 0)
    __shared__ uint32_t word_of_id[PER_GRID ? BLOCK_K : 1];
    if constexpr (PER_GRID) {
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
    const bool GI = genset_wave_is_instant<F>(p, s);
    const int32_t off = a.ep_off[i];
    const int32_t n = lookahead_steps(t0, a.ep_final[i], H);
    GridFactors f;
    load_lane_factors<F, SRC>(a.c, i, f);
    // the plan of this candidate: H ids, or H rows of N ids
    const uint8_t *__restrict__ plan = plans + c * H * (PER_GRID ? N : 1);

    RowSlot ring[U];
    fill_row_ring<F, SRC>(a, f, i, t0, off, n, ring);
    uint64_t idq = 0;                     // PER_GRID: the id bytes of the U ring slots
    if constexpr (PER_GRID) {
#pragma unroll
        for (int u = 0; u < U; u++)
            if (u < n) idq |= (uint64_t)(plan + (int64_t)u * N)[i32] << (8 * u);
    }
    uint32_t word_next = 0u;
    if constexpr (PER_GRID) word_next = word_of_id[idq & 0xffu];
    double acc = 0.0, w = 1.0;
#pragma nounroll
    for (int32_t k = 0; k < n; k++) {
        const int32_t t = t0 + k;
        Inputs in;
        widen_row_slot<F, SRC>(a, f, ring[0], t, off, in);
        rotate_ring(ring);
        uint32_t word;
        if constexpr (PER_GRID) {
            word = word_next;
            idq >>= 8;
            word_next = word_of_id[idq & 0xffu];                // (the coming step's; beyond the last step: unused)
            if (k + U < n) idq |= (uint64_t)(plan + (int64_t)(k + U) * N)[i32] << (8 * (U - 1));
        } else {
            word = pl_select(tab, (int32_t)plan[k]);
        }
        double bat_q;
        uint32_t xv = 0u;
        populate_core<F, false>(p, s, word, in, bat_q, 0.0 + -1 * in.load, in.pv, GI, &xv);
        Outputs o;
        step_core<F, true>(p, d, s, in, false, false, GI, o, bat_q);
        lookahead_count(shaped_reward<F>(a.shaper, o), gamma, acc, w);
        advance_row_ring<F, SRC>(a, f, i, t, k, off, n, false, ring);
    }
    const int64_t e = c * N + i;
    ret[e] = acc;
    if constexpr (F & F_BATTERY) { if (end_soc) end_soc[e] = s.charge / p.bat_cmax; }
}

template <int F>
static void lookahead_episodes_dispatch(const LookaheadLaunch &L)
{
    with_episode_src(L.src, [&](auto src) {
        constexpr int SRC = decltype(src)::value, U = ROW_RING<F>;
        for (int32_t c0 = 0; c0 < L.C; c0 += LOOKAHEAD_MAX_Y) {
            const dim3 grid(L.blocks, (unsigned)(L.C - c0 < LOOKAHEAD_MAX_Y ? L.C - c0 : LOOKAHEAD_MAX_Y));
            if (L.per_grid)
                lookahead_episodes_kernel<F, U, true, SRC><<<grid, BLOCK_K, 0, L.stream>>>(*L.k, *L.tab, L.ids, L.t, L.H, c0, L.gamma, L.ret, L.end_soc, L.gpb);
            else
                lookahead_episodes_kernel<F, U, false, SRC><<<grid, BLOCK_K, 0, L.stream>>>(*L.k, *L.tab, L.ids, L.t, L.H, c0, L.gamma, L.ret, L.end_soc, L.gpb);
        }
    });
}

MGX_EPISODE_LAUNCH_FN(lookahead_episodes, LookaheadLaunch, L.flags)

}  // namespace mgx
