// mgx_episode_loop.hpp -- every step the six fused launches over per-grid in-place episodes have in common, stated once:
//   rollout_episodes_kernel (mgx_episodes.hip)               step_k_episodes_kernel (mgx_step_episodes.hip)
//   rollout_episodes_rows_kernel (mgx_episode_rows.hip)      step_k_episodes_rows_kernel (mgx_step_episode_rows.hip)
//   rollout_policy_episodes_kernel (mgx_policy_episodes.hip) step_k_policy_episodes_kernel (mgx_step_policy_episodes.hip)
// Each kernel keeps its own loop, written out in its file; what a loop does under a name of this header it does as the other five:
// the ring of series rows (slot, fetch, widening, fill, rotation, advance), the lane's restart, the per-lane episode statistics,
// the per-step output stores and the lane's series factors -- and, on the host side, the tail of each translation unit (the row
// source and the layout of a launch as template parameters).  The kernels with observation rows add mgx_episode_rows.hpp, the
// closed-loop ones mgx_policy.hpp on top of that.
// WRITTEN OUT where a helper cost a kernel registers or speed (profiles/exp_episode_loop_refactor.txt), each under a comment that names
// the form and the figure: the factors, fill, rotation, restart and advance in rollout_episodes_rows_kernel,
// rollout_policy_episodes_kernel and step_k_policy_episodes_kernel, the advance in step_k_episodes_rows_kernel.  A change to
// load_lane_factors, fill_row_ring, rotate_ring, restart_lane or advance_row_ring is made there too.
// The two exploring twins of the policy kernels (rollout_policy_explore_episodes_kernel: mgx_policy_explore_episodes.hip,
// step_k_policy_explore_episodes_kernel: mgx_step_policy_explore_episodes.hip) are a seventh and eighth loop on the same pieces,
// compiled the same way; they CALL all five ring helpers (their register figures on them: DESIGN.md's kernel table).  So does the
// sampling twin of the discrete policy kernel (rollout_policy_sample_episodes_kernel: mgx_policy_sample_episodes.hip), a ninth.
#pragma once
#include "mgx_kernels.hpp"

#include <type_traits>

// depth of the action ring of the two K-step kernels with an action stream (steps of control loads in flight)
#ifndef MGX_RING_STEP_EPISODES
#define MGX_RING_STEP_EPISODES 4
#endif

namespace mgx {

// What a slot of the row ring holds until its step consumes it: the raw values of one series row of the lane's grid.
// SRC = EP_SRC_FACT: the base-table values (load / pv / co2 profile columns out of the profile-major copies) + the 64-row outage
// word of the row; the ratios, the tariff and the status bit are applied when the slot is widened.  Materialised series: the row
// itself.
struct RowSlot {
    double load, pv, g_pimp, g_pexp, g_co2, g_stat;
    uint64_t outage;
};

// The raw row of counter value t under the lane's offset `off`.  SRC: where the rows come from --
//   EP_SRC_FACT        factorised series: the profile-major base tables of the in-place handle (KArgs.pm_pitch rows per profile);
//                      the lock-step kernel's shared LDS chunk does not apply, the rows differ from lane to lane
//   EP_SRC_GRID_MAJOR  [T, N] series through the handle's grid-major copy [N, pm_pitch, 2 or 6]: a row is 16 or 48 adjacent bytes
//   EP_SRC_GATHER      [T, N] series read where they lie (no copy: allocation refused, or tunable grid_major_copy = 0): a lane
//                      takes 8 bytes out of its own row's line per component -- same values, slower
template <int F, int SRC>
__device__ __forceinline__ void fetch_row_slot(const KArgs &a, const GridFactors &f, int64_t i, int32_t t, int32_t off, RowSlot &r)
{
    const int64_t N = a.N;
    const int32_t pm = a.pm_pitch;
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
}

// ... and the series values out of it: what fact_series / load_series_row give a single step and what series_component gives
// observe_row_h0 (the same operations on the same operands)
template <int F, int SRC>
__device__ __forceinline__ void widen_row_slot(const KArgs &a, const GridFactors &f, const RowSlot &r, int32_t t, int32_t off, Inputs &in)
{
    in.g_stat = 1.0;
    if constexpr (SRC == EP_SRC_FACT) {
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
}

// The ring's REACH: how many rows from counter value t0 on a launch of K steps reads.  The plain kernels consume row t0 + k in
// step k: reach K.  The kernels that build observation rows show, after step k, series row t0 + k + 1 -- the row after the last
// step, and the first row of an episode that starts at step K - 1, too: reach K + 1 (guards `<= K` where the plain kernels have
// `< K`).  episode_row clamps every row to the series, so the extra fetch stays inside it.  The id and action rings of a launch
// keep reach K: there is no id or action row K.

// depth of the row ring, as rollout_kernel's: a slot of a layout with a GridModule holds up to six values (depth 4), else two (depth 8)
template <int F>
constexpr int ROW_RING = (F & F_GRID) ? 4 : MGX_RING_ROLLOUT;

// the prologue: slot u holds the row of step u
template <int F, int SRC, int U>
__device__ __forceinline__ void fill_row_ring(const KArgs &a, const GridFactors &f, int64_t i, int32_t t0, int32_t off, int32_t reach,
                                              RowSlot (&ring)[U])
{
#pragma unroll
    for (int u = 0; u < U; u++)
        if (u < reach) fetch_row_slot<F, SRC>(a, f, i, t0 + u, off, ring[u]);
}

// A ring ROTATES: slot 0 is always the coming step, a consumed slot leaves by register moves -- so a loop body exists once (not
// once per slot) and with it the restart branch, which reads all U slots again: unrolled per slot that branch alone was U x U
// loads of code and the kernels spilled scalar registers.
template <typename SLOT, int U>
__device__ __forceinline__ void rotate_ring(SLOT (&ring)[U])
{
#pragma unroll
    for (int u = 0; u + 1 < U; u++) ring[u] = ring[u + 1];
}

// After step k (counter value t) and the rotation, slot v stands for step k + 1 + v.  A lane that went on in its episode reads
// the one row that enters at the far end; a lane that `restarted` has moved to other rows: what the ring read ahead under the old
// offset is read again under the new one (`off`), in the divergent branch only the restarting lanes are in.  Call it with a
// literal `restarted` from either side of that branch.
template <int F, int SRC, int U>
__device__ __forceinline__ void advance_row_ring(const KArgs &a, const GridFactors &f, int64_t i, int32_t t, int32_t k, int32_t off,
                                                 int32_t reach, bool restarted, RowSlot (&ring)[U])
{
    if (restarted) {
#pragma unroll
        for (int v = 0; v < U; v++)
            if (k + 1 + v < reach) fetch_row_slot<F, SRC>(a, f, i, t + 1 + v, off, ring[v]);
    } else if (k + U < reach) {
        fetch_row_slot<F, SRC>(a, f, i, t + U, off, ring[U - 1]);
    }
}

// The lane's restart after the step of counter value t: episode_auto_restart as step_body<F, true> calls it, and the register copy
// of ep_final[i] refreshed.  `a_dev`: the handle's device copy of the KArgs -- the arguments of the draw read here, inside the
// branch, occupy scalar registers only while a lane restarts (as kernel arguments they stay live across the whole loop).
__device__ __forceinline__ void restart_lane(const KArgs *__restrict__ a_dev, int64_t i, int32_t t, int32_t &off, int32_t &fin)
{
    off = episode_auto_restart(*a_dev, i, t, off, true);
    fin = a_dev->ep_final[i];
}

// The per-lane episode statistics mgx_episode_stats carries from launch to launch (each array may be NULL): the return of the
// running episode, the sum and the last of the returns of the finished ones, their number.
struct LaneStats {
    double run, sum, last;
    int32_t eps;

    __device__ __forceinline__ void load(const mgx_episode_stats &es, int64_t i)
    {
        run = es.ret_running ? es.ret_running[i] : 0.0;
        sum = es.ret_sum ? es.ret_sum[i] : 0.0;
        last = es.ret_last ? es.ret_last[i] : 0.0;
        eps = es.episodes ? es.episodes[i] : 0;
    }
    // the step of counter value t returned r; the lane's episode ends with step fin - 1
    __device__ __forceinline__ void update(double r, int32_t t, int32_t fin)
    {
        run += r;
        if (t == fin - 1) { last = run; sum += run; eps += 1; run = 0.0; }
    }
    // (the four addresses: out of the kernel's mgx_episode_stats, or -- where those copies ended their lives before the loop -- a
    // second time out of the kernarg segment, late_kernargs)
    __device__ __forceinline__ void store(double *ret_running, double *ret_sum, double *ret_last, int32_t *episodes, int64_t i) const
    {
        if (ret_running) ret_running[i] = run;
        if (ret_sum) ret_sum[i] = sum;
        if (ret_last) ret_last[i] = last;
        if (episodes) episodes[i] = eps;
    }
};

// what a step leaves in the launch's [K, N] outputs, at element o64 = k * N + i
template <int F>
__device__ __forceinline__ void store_step_outputs(const FusedOut &out, int64_t o64, double r, bool dn, const State &s)
{
    if (out.reward) out.reward[o64] = r;
    if (out.done) out.done[o64] = (uint8_t)dn;
    if constexpr (F & F_BATTERY) { if (out.soc_trace) out.soc_trace[o64] = s.soc; }
    if constexpr (F & F_GENSET) { if (out.status_trace) out.status_trace[o64] = s.status; }
}

// the lane's factors of factorised series (zero where the rows are materialised: fetch and widening do not look at them)
template <int F, int SRC>
__device__ __forceinline__ void load_lane_factors(const mgx_columns &c, int64_t i, GridFactors &f)
{
    f.lr = 0.0; f.pr = 0.0; f.lp = 0u; f.pp = 0u; f.cp = 0u; f.pat = 0u;
    if constexpr (SRC == EP_SRC_FACT) load_factors<F>(c, i, f);
}

// ---- host side: the tail of each of the six translation units ----
// fn(std::integral_constant<int, EP_SRC_*>) for the row source of a launch: `decltype(src)::value` is a template argument
template <typename FN>
static inline void with_episode_src(int src, FN &&fn)
{
    if (src == EP_SRC_FACT) fn(std::integral_constant<int, EP_SRC_FACT>{});
    else if (src == EP_SRC_GRID_MAJOR) fn(std::integral_constant<int, EP_SRC_GRID_MAJOR>{});
    else fn(std::integral_constant<int, EP_SRC_GATHER>{});
}

// Each unit is compiled in MGX_EPISODE_PARTS slices of the layouts, in parallel like mgx_fused.hip:
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c -DMGX_EPISODE_PART=p <unit>.hip -o <unit>_p.o
// MGX_EPISODE_LAUNCH_FN(name, Launch, flags) defines `bool launch_<name>_p<part>(const Launch &L)` of the slice: <name>_dispatch<F>(L)
// for the layout `flags` (an expression in L) if it is one of MGX_EPISODE_FLAGS_<part> (mgx_kernels.hpp), else false.
#ifdef MGX_EPISODE_PART
#define MGX_PART_FLAGS MGX_CAT(MGX_EPISODE_FLAGS_, MGX_EPISODE_PART)
// fn(std::integral_constant<int, F>) if `flags` is a layout F of this slice; whether it was
template <typename FN>
static inline bool with_part_layout(int flags, FN &&fn)
{
    switch (flags) {
#define X(FV) case FV: fn(std::integral_constant<int, FV>{}); return true;
        MGX_PART_FLAGS(X)
#undef X
        default: return false;
    }
}
#define MGX_EPISODE_LAUNCH_FN(NAME, LAUNCH, FLAGS)                                                          \
    bool MGX_CAT(launch_##NAME##_p, MGX_EPISODE_PART)(const LAUNCH &L)                                      \
    {                                                                                                       \
        return with_part_layout(FLAGS, [&](auto layout) { NAME##_dispatch<decltype(layout)::value>(L); });  \
    }
#else                                            // (mgx_abi.hip, which only calls the launch functions)
#define MGX_EPISODE_LAUNCH_FN(NAME, LAUNCH, FLAGS) static_assert(false, "compile with -DMGX_EPISODE_PART=<0..MGX_EPISODE_PARTS-1>");
#endif

}  // namespace mgx
