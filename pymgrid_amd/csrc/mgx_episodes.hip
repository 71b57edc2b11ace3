// mgx_episodes.hip -- the fused discrete roll-out over per-grid in-place episodes (mgx_rollout_episodes): K steps per launch,
// the priority list expanded in the kernel, every lane on the rows of its OWN episode and restarting inside the launch.
// Translation units of their own (MGX_EPISODE_PARTS slices of the layouts, compiled in parallel like mgx_fused.hip):
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c -DMGX_EPISODE_PART=p mgx_episodes.hip -o mgx_episodes_p.o
// so the lock-step kernels of mgx_fused.hip come out of the compiler exactly as they did without this file.
#include "mgx_kernels.hpp"

#ifndef MGX_EPISODE_PART
#error "compile with -DMGX_EPISODE_PART=<0..MGX_EPISODE_PARTS-1>"
#endif

// layouts (template parameter F) of this slice: MGX_EPISODE_FLAGS_<part> (mgx_kernels.hpp)
#define MGX_PART_FLAGS MGX_CAT(MGX_EPISODE_FLAGS_, MGX_EPISODE_PART)

namespace mgx {

// What a ring slot holds until its step consumes it: the raw values of one series row of the lane's grid.  SRC = EP_SRC_FACT:
// the base-table values (load / pv / co2 profile columns out of the profile-major copies) + the 64-row outage word of the row;
// the ratios, the tariff and the status bit are applied when the step consumes the slot.  Materialised series: the row itself.
struct EpisodeSlot {
    double load, pv, g_pimp, g_pexp, g_co2, g_stat;
    uint64_t outage;
};

// F: layout.  U: ring depth (steps of loads in flight).  PER_STEP: ids [K, N] (else one id per grid, the list decoding hoisted out
// of the loop).  SRC: where the rows come from --
//   EP_SRC_FACT        factorised series: the profile-major base tables of the in-place handle (KArgs.pm_pitch rows per profile);
//                      the lock-step kernel's shared LDS chunk does not apply, the rows differ from lane to lane
//   EP_SRC_GRID_MAJOR  [T, N] series through the handle's grid-major copy [N, pm_pitch, 2 or 6]: a row is 16 or 48 adjacent bytes
//   EP_SRC_GATHER      [T, N] series read where they lie (no copy: allocation refused, or tunable grid_major_copy = 0): a lane
//                      takes 8 bytes out of its own row's line per component -- same values, slower
// The shared counter of this mode never ends; `done` is the lane's own (counter >= ep_final[i] - 1, done_at's test on a register
// copy of ep_final[i] that a restart refreshes).  After every step: the statistics, then episode_auto_restart with the counter value
// of the step -- the call step_body<F, true> makes -- so K steps here leave what K single steps leave.
// A restart moves the lane to other rows: what the ring read ahead under the old offset is read again under the new one, in a
// divergent branch only the restarting lanes enter.
template <int F, int U, bool PER_STEP, int SRC>
__global__ __launch_bounds__(BLOCK_K) void rollout_episodes_kernel(const KArgs a, const PLWords tab, const uint8_t *__restrict__ ids,
                                                                   int32_t t0, int32_t K, const FusedOut out,
                                                                   const mgx_episode_stats es, int32_t gpb,
                                                                   const KArgs *__restrict__ a_dev)
{
    static_assert(U <= 8, "the id ring is one 64-bit register");
    constexpr bool FACT = SRC == EP_SRC_FACT;
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
    const int32_t pm = a.pm_pitch;
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
    f.lr = 0.0; f.pr = 0.0; f.lp = 0u; f.pp = 0u; f.cp = 0u; f.pat = 0u;
    if constexpr (FACT) load_factors<F>(a.c, i, f);
    double run = es.ret_running ? es.ret_running[i] : 0.0;
    double sum = es.ret_sum ? es.ret_sum[i] : 0.0;
    double last = es.ret_last ? es.ret_last[i] : 0.0;
    int32_t eps = es.episodes ? es.episodes[i] : 0;

    // the raw row of counter value t under the lane's current offset
    auto fetch = [&](EpisodeSlot &r, int32_t t) __attribute__((always_inline)) {
        const int64_t row = episode_row(a, t, off);
        if constexpr (SRC == EP_SRC_FACT) {
            r.load = a.c.base_load[(int64_t)f.lp * pm + row];
            r.pv = a.c.base_pv[(int64_t)f.pp * pm + row];
            if constexpr (F & F_GRID) {
                r.g_co2 = a.c.base_co2[(int64_t)f.cp * pm + row];
                r.outage = 0;
                if (a.c.outage_bits) r.outage = a.c.outage_bits[(row >> 6) * N + i];
            }
        } else if constexpr (SRC == EP_SRC_GRID_MAJOR) {
            // rows of 16 / 48 bytes in a 16-byte aligned copy: whole 16-byte loads
            constexpr int C = (F & F_GRID) ? 6 : 2;
            const double2 *q = reinterpret_cast<const double2 *>(a.c.load_ts + (i * pm + row) * C);
            const double2 v0 = q[0];
            r.load = v0.x; r.pv = v0.y;
            if constexpr (F & F_GRID) {
                const double2 v1 = q[1], v2 = q[2];
                r.g_pimp = v1.x; r.g_pexp = v1.y; r.g_co2 = v2.x; r.g_stat = v2.y;
            }
        } else {
            r.load = a.c.load_ts[row * N + i];
            r.pv = a.c.pv_ts[row * N + i];
            if constexpr (F & F_GRID) {
                const double *g = a.c.grid_ts + (row * 4) * N + i;
                r.g_pimp = g[0]; r.g_pexp = g[N]; r.g_co2 = g[2 * N]; r.g_stat = g[3 * N];
            }
        }
    };
    // ... and the step's series inputs out of it (the values fact_series / load_series_row give a single step)
    auto widen_slot = [&](const EpisodeSlot &r, int32_t t, Inputs &in) __attribute__((always_inline)) {
        in.g_stat = 1.0;
        if constexpr (FACT) {
            in.load = fact_load(r.load, f.lr);
            in.pv = fact_pv(r.pv, f.pr);
            if constexpr (F & F_GRID) {
                const int64_t row = episode_row(a, t, off);
                in.g_pimp = tariff_price((int32_t)f.pat, (int32_t)row); in.g_pexp = 0.0;
                in.g_co2 = r.g_co2;
                in.g_stat = ((r.outage >> (row & 63)) & 1ull) ? 0.0 : 1.0;
            }
        } else {
            in.load = r.load; in.pv = r.pv;
            if constexpr (F & F_GRID) { in.g_pimp = r.g_pimp; in.g_pexp = r.g_pexp; in.g_co2 = r.g_co2; in.g_stat = r.g_stat; }
        }
    };

    // One loop; `gen_instant` stays a run-time (wave-uniform) flag: the two compile-time forms rollout_kernel keeps cost this kernel
    // scalar-register spills.  The ring ROTATES:
    // slot 0 is always the coming step, a consumed slot leaves by register moves -- so the loop body exists once (not once per slot
    // as in rollout_kernel) and with it the restart branch, which reads all U slots again: unrolled per slot that branch alone
    // was U x U loads of code and the kernel spilled scalar registers.
    {
        const bool GI = gen_instant;
        EpisodeSlot ring[U];
        uint64_t idq = 0;                 // PER_STEP: the id bytes of the U ring slots (an array would live in scratch memory)
#pragma unroll
        for (int u = 0; u < U; u++)
            if (u < K) {
                fetch(ring[u], t0 + u);
                if constexpr (PER_STEP) idq |= (uint64_t)(ids + (int64_t)u * N)[i32] << (8 * u);
            }
        uint32_t word_next = 0u;
        if constexpr (PER_STEP) word_next = word_of_id[idq & 0xffu];
        int64_t o64 = i;
#pragma nounroll
        for (int32_t k = 0; k < K; k++) {
            const int32_t t = t0 + k;
            Inputs in;
            widen_slot(ring[0], t, in);
#pragma unroll
            for (int u = 0; u + 1 < U; u++) ring[u] = ring[u + 1];
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
            if (out.reward) out.reward[o64] = r;
            if (out.done) out.done[o64] = (uint8_t)dn;
            if constexpr (F & F_BATTERY) { if (out.soc_trace) out.soc_trace[o64] = s.soc; }
            if constexpr (F & F_GENSET) { if (out.status_trace) out.status_trace[o64] = s.status; }
            o64 += N;
            run += r;
            if (t == fin - 1) { last = run; sum += run; eps += 1; run = 0.0; }
            if (ar_on && dn) {
                // (the arguments of the draw out of the handle's device copy of the KArgs: read here, in the branch, they occupy
                // scalar registers only while a lane restarts -- as kernel arguments they stay live across the whole loop)
                off = episode_auto_restart(*a_dev, i, t, off, true);
                fin = a_dev->ep_final[i];
                // slot v now stands for step k + 1 + v: all of them again, at the rows of the new episode
#pragma unroll
                for (int v = 0; v < U; v++)
                    if (k + 1 + v < K) fetch(ring[v], t + 1 + v);
            } else if (k + U < K) {
                fetch(ring[U - 1], t + U);
            }
        }
    }
    if constexpr (F & F_BATTERY) { if (!want_soc) s.soc = s.charge / p.bat_cmax; }
    store_state<F>(a_dev->c, i, s);           // (the same columns; their addresses need no scalar registers across the loop)
    if (es.ret_running) es.ret_running[i] = run;
    if (es.ret_sum) es.ret_sum[i] = sum;
    if (es.ret_last) es.ret_last[i] = last;
    if (es.episodes) es.episodes[i] = eps;
}

template <int F>
static void rollout_episodes_dispatch(const EpisodeLaunch &L)
{
    // ring depth as rollout_kernel's: a slot of a layout with a GridModule holds up to six values (depth 4), else two (depth 8)
#define MGX_EPISODES(PS, SRC) rollout_episodes_kernel<F, (F & F_GRID) ? 4 : MGX_RING_ROLLOUT, PS, SRC><<<L.blocks, BLOCK_K, 0, L.stream>>>( \
        *L.k, *L.tab, L.ids, L.t, L.K, L.out, L.stats, L.gpb, L.k_dev)
    if (L.per_step) {
        if (L.src == EP_SRC_FACT) MGX_EPISODES(true, EP_SRC_FACT);
        else if (L.src == EP_SRC_GRID_MAJOR) MGX_EPISODES(true, EP_SRC_GRID_MAJOR);
        else MGX_EPISODES(true, EP_SRC_GATHER);
    } else {
        if (L.src == EP_SRC_FACT) MGX_EPISODES(false, EP_SRC_FACT);
        else if (L.src == EP_SRC_GRID_MAJOR) MGX_EPISODES(false, EP_SRC_GRID_MAJOR);
        else MGX_EPISODES(false, EP_SRC_GATHER);
    }
#undef MGX_EPISODES
}

bool MGX_CAT(launch_rollout_episodes_p, MGX_EPISODE_PART)(const EpisodeLaunch &L)
{
    switch (L.flags) {
#define X(FV) case FV: rollout_episodes_dispatch<FV>(L); return true;
        MGX_PART_FLAGS(X)
#undef X
        default: return false;
    }
}

}  // namespace mgx
