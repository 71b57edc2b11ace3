// mgx_step_episodes.hip -- the fused continuous K-step over per-grid in-place episodes (mgx_step_k_episodes): K steps of
// Microgrid.run(control, normalized) per launch, the controls out of an action stream [K, N, A], every lane on the rows of its OWN
// episode and restarting inside the launch.  The continuous twin of rollout_episodes_kernel (mgx_episodes.hip).
// Translation units of their own (MGX_EPISODE_PARTS slices of the layouts, compiled in parallel like mgx_episodes.hip):
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c -DMGX_STEP_EPISODE_PART=p mgx_step_episodes.hip -o mgx_step_episodes_p.o
// so every other kernel comes out of the compiler exactly as it did without this file.
#include "mgx_kernels.hpp"

#ifndef MGX_STEP_EPISODE_PART
#error "compile with -DMGX_STEP_EPISODE_PART=<0..MGX_EPISODE_PARTS-1>"
#endif

// layouts (template parameter F) of this slice: MGX_EPISODE_FLAGS_<part> (mgx_kernels.hpp)
#define MGX_PART_FLAGS MGX_CAT(MGX_EPISODE_FLAGS_, MGX_STEP_EPISODE_PART)

// depth of the action ring (steps of control loads in flight); the row ring's depth is the discrete kernel's
#ifndef MGX_RING_STEP_EPISODES
#define MGX_RING_STEP_EPISODES 4
#endif

namespace mgx {

// What a slot of the row ring holds until its step consumes it: the raw values of one series row of the lane's grid (restated from
// mgx_episodes.hip, which stays as it is).  SRC = EP_SRC_FACT: the base-table values + the 64-row outage word of the row; the
// ratios, the tariff and the status bit are applied when the step consumes the slot.  Materialised series: the row itself.
struct SeriesSlot {
    double load, pv, g_pimp, g_pexp, g_co2, g_stat;
    uint64_t outage;
};

// F: layout.  U: depth of the row ring.  UA: depth of the action ring.  AT: storage type of the controls (widened when the step
// consumes the slot, as in step_k_kernel).  SRC: where the series rows come from (EP_SRC_*, as in rollout_episodes_kernel).
// Row k of `actions` belongs to step k of the launch whatever episode a grid is in: the action rows are wave-uniform (an SGPR row
// base + the lane's offset) and a restart does not touch them -- only the series rows, which move with the lane's episode, are
// read again in the restart branch.
// The shared counter of this mode never ends; `done` is the lane's own (counter >= ep_final[i] - 1 on a register copy of
// ep_final[i] that a restart refreshes).  After every step: the statistics, then episode_auto_restart with the counter value of the
// step -- the call step_body<F, true> makes -- so K steps here leave what K calls of mgx_step leave.
template <int F, int U, int UA, typename AT, int SRC>
__global__ __launch_bounds__(BLOCK_K) void step_k_episodes_kernel(const KArgs a, const AT *__restrict__ actions, int32_t t0, int32_t K,
                                                                  int normalized, const FusedOut out, const mgx_episode_stats es,
                                                                  int32_t gpb, const KArgs *__restrict__ a_dev)
{
    constexpr bool FACT = SRC == EP_SRC_FACT;
    constexpr int A_DIM = 2 * ((F & F_GENSET) != 0) + ((F & F_BATTERY) != 0) + ((F & F_GRID) != 0);
    const int64_t i = (int64_t)blockIdx.x * gpb + threadIdx.x;
    if ((int32_t)threadIdx.x >= gpb || i >= a.N) return;
    const int64_t N = a.N;
    const int32_t pm = a.pm_pitch;
    const uint32_t i32 = (uint32_t)i;
    Params p; State s; Derived d;
    load_state<F>(a.c, i, false, s);
    load_params<F>(a.c, i, p);
    derive<F>(p, d);
    const bool gen_instant = genset_wave_is_instant<F>(p, s);
    const bool norm = normalized != 0;
    const bool want_soc = out.soc_trace != nullptr;
    const bool ar_on = a.ar_mode != 0;
    int32_t off = a.ep_off[i], fin = a.ep_final[i];
    GridFactors f;
    f.lr = 0.0; f.pr = 0.0; f.lp = 0u; f.pp = 0u; f.cp = 0u; f.pat = 0u;
    if constexpr (FACT) load_factors<F>(a.c, i, f);
    double run = es.ret_running ? es.ret_running[i] : 0.0;
    double sum = es.ret_sum ? es.ret_sum[i] : 0.0;
    double last = es.ret_last ? es.ret_last[i] : 0.0;
    int32_t eps = es.episodes ? es.episodes[i] : 0;

    // the raw row of counter value t under the lane's current offset
    auto fetch = [&](SeriesSlot &r, int32_t t) __attribute__((always_inline)) {
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
    auto widen_slot = [&](const SeriesSlot &r, int32_t t, Inputs &in) __attribute__((always_inline)) {
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

    // One loop body, `gen_instant` a run-time (wave-uniform) flag, both rings ROTATE (slot 0 is always the coming step, a consumed
    // slot leaves by register moves): the lessons of rollout_episodes_kernel -- a body per slot multiplies the restart branch and
    // spills scalar registers.
    {
        const bool GI = gen_instant;
        SeriesSlot ring[U];
        RawActions<AT> act[UA];
#pragma unroll
        for (int u = 0; u < U; u++)
            if (u < K) fetch(ring[u], t0 + u);
        // the action row of the step that enters the action ring next (wave-uniform)
        const AT *arow = actions;
#pragma unroll
        for (int u = 0; u < UA; u++)
            if (u < K) { load_actions_at<F>(arow, i32, act[u]); arow += N * A_DIM; }
        int64_t o64 = i;
#pragma nounroll
        for (int32_t k = 0; k < K; k++) {
            const int32_t t = t0 + k;
            Inputs in;
            widen_slot(ring[0], t, in);
            if constexpr (F & F_GENSET) { in.a_goal = (double)act[0].a_goal; in.a_gen = (double)act[0].a_gen; }
            if constexpr (F & F_BATTERY) in.a_bat = (double)act[0].a_bat;
            if constexpr (F & F_GRID) in.a_grid = (double)act[0].a_grid;
#pragma unroll
            for (int u = 0; u + 1 < U; u++) ring[u] = ring[u + 1];
#pragma unroll
            for (int u = 0; u + 1 < UA; u++) act[u] = act[u + 1];
            if (k + UA < K) { load_actions_at<F>(arow, i32, act[UA - 1]); arow += N * A_DIM; }
            Outputs o;
            step_core<F>(p, d, s, in, norm, want_soc, GI, o);
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
                // row slot v now stands for step k + 1 + v: all of them again, at the rows of the new episode (the controls stay)
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

template <int F, typename AT>
static void step_k_episodes_dispatch(const EpisodeLaunch &L)
{
    // row ring as rollout_episodes_kernel's: a slot of a layout with a GridModule holds up to six values (depth 4), else two (depth 8)
#define MGX_STEP_EPISODES(SRC) step_k_episodes_kernel<F, (F & F_GRID) ? 4 : MGX_RING_ROLLOUT, MGX_RING_STEP_EPISODES, AT, SRC><<<L.blocks, BLOCK_K, 0, L.stream>>>( \
        *L.k, (const AT *)L.actions, L.t, L.K, L.normalized, L.out, L.stats, L.gpb, L.k_dev)
    if (L.src == EP_SRC_FACT) MGX_STEP_EPISODES(EP_SRC_FACT);
    else if (L.src == EP_SRC_GRID_MAJOR) MGX_STEP_EPISODES(EP_SRC_GRID_MAJOR);
    else MGX_STEP_EPISODES(EP_SRC_GATHER);
#undef MGX_STEP_EPISODES
}

bool MGX_CAT(launch_step_k_episodes_p, MGX_STEP_EPISODE_PART)(const EpisodeLaunch &L)
{
    switch (L.flags) {
#define X(FV) case FV: if (L.act_f32) step_k_episodes_dispatch<FV, float>(L); else step_k_episodes_dispatch<FV, double>(L); return true;
        MGX_PART_FLAGS(X)
#undef X
        default: return false;
    }
}

}  // namespace mgx
