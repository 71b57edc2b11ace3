// mgx_episode_rows.hpp -- what the fused episode launches that build observation rows add to mgx_episode_loop.hpp
// (mgx_rollout_episodes_rows: mgx_episode_rows.hip, mgx_step_k_episodes_rows: mgx_step_episode_rows.hip, and the two closed-loop
// launches of mgx_policy.hpp): the H = 0 row built from series values that are already in registers, the wave's row tile, the
// kernel arguments read late and the one-struct arguments of the two kernels.
#pragma once
#include "mgx_episode_loop.hpp"

namespace mgx {

// Lower bound and spread of the series columns of an H = 0 row (load, pv, the four grid components): loop-invariant, so the fused
// kernels hold them in registers -- 4 or 12 doubles -- instead of 4 or 12 loads per step.
template <int F>
struct RowBounds {
    static constexpr int NC = (F & F_GRID) ? 6 : 2;
    double lo[NC], sp[NC];
};

template <int F>
__device__ __forceinline__ void load_row_bounds(const mgx_columns &c, int64_t N, int64_t i, RowBounds<F> &b)
{
    b.lo[0] = c.load_lo[i]; b.sp[0] = space_spread(b.lo[0], c.load_hi[i]);
    b.lo[1] = c.pv_lo[i]; b.sp[1] = space_spread(b.lo[1], c.pv_hi[i]);
    if constexpr (F & F_GRID) {
#pragma unroll
        for (int cc = 0; cc < 4; cc++) {
            b.lo[2 + cc] = c.grid_lo[cc * N + i];
            b.sp[2 + cc] = space_spread(b.lo[2 + cc], c.grid_hi[cc * N + i]);
        }
    }
}

// The five column bases of a flat row, its length and its element type in ONE wave-uniform word (4 bits each: an H = 0 row has at
// most 12 columns): the fused loops have no scalar registers to spare for seven loop-invariant values -- they carry this word and
// take it apart where a row is built (pack_row_desc on the host).
__host__ __device__ inline uint32_t pack_row_desc(const KArgs &a)
{
    return (uint32_t)a.col_load | (uint32_t)a.col_pv << 4 | (uint32_t)a.col_gen << 8 | (uint32_t)a.col_bat << 12 |
           (uint32_t)a.col_grid << 16 | (uint32_t)a.obs_dim << 20 | (uint32_t)(a.obs_f32 != 0) << 28;
}
__device__ __forceinline__ int32_t row_desc_dim(uint32_t desc) { return (int32_t)((desc >> 20) & 0xffu); }
__device__ __forceinline__ bool row_desc_f32(uint32_t desc) { return (desc >> 28) != 0u; }

// The kernel arguments again, as MEMORY: a pointer to the kernarg segment the compiler cannot see through.  What is read through
// it is loaded where it is used -- the statistics' addresses after the loop, the addresses a restart needs inside its (rare)
// branch -- instead of at the kernel's entry, from where it would occupy scalar registers across the whole loop.  The kernels
// here take ONE struct by value, so the segment starts with that struct.
template <typename ARGS>
__device__ __forceinline__ const __attribute__((address_space(4))) ARGS *late_kernargs()
{
    const __attribute__((address_space(4))) ARGS *q = (const __attribute__((address_space(4))) ARGS *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(q));
    return q;
}

// The H = 0 row of series row t_row (= counter + 1 + offset) with the post-step state, the series values taken out of `in` (the
// widened ring slot of that row) instead of loaded: observe_row_h0's values bit for bit -- (v - lo) / spread and observe_state_cols'
// expressions with the same operands, at the same columns.  A row at or beyond T shows the padding value: that (rare) lane goes
// through observe_row_h0 itself, which reads no series there, on the handle's device copy of the KArgs (a_dev: read inside the branch).
template <int F, typename OT>
__device__ __forceinline__ void episode_row_h0(const KArgs *__restrict__ a_dev, int32_t T, uint32_t desc, int64_t i, int32_t t_row,
                                               const Inputs &in, const RowBounds<F> &b, const Params &p, const State &s,
                                               OT *__restrict__ dst)
{
    if (t_row < T) {
        dst[desc & 15u] = (OT)((in.load - b.lo[0]) / b.sp[0]);
        dst[(desc >> 4) & 15u] = (OT)((in.pv - b.lo[1]) / b.sp[1]);
        if constexpr (F & F_GENSET) {
            OT *g = dst + ((desc >> 8) & 15u);
            const double su = (double)(p.gen_times & 0xff), wd = (double)((p.gen_times >> 16) & 0xff);
            g[0] = (OT)space_norm(0.0, 1.0, (double)(s.status & 0xff));
            g[1] = (OT)space_norm(0.0, 1.0, (double)((s.status >> 8) & 0xff));
            g[2] = (OT)space_norm(0.0, su, (double)((s.status >> 16) & 0xff));
            g[3] = (OT)space_norm(0.0, wd, (double)(s.status >> 24));
        }
        if constexpr (F & F_BATTERY) {
            OT *q = dst + ((desc >> 12) & 15u);
            const double min_soc = p.bat_cmin / p.bat_cmax;
            q[0] = (OT)space_norm(min_soc, 1.0, s.soc);
            q[1] = (OT)space_norm(p.bat_cmin, p.bat_cmax, s.charge);
        }
        if constexpr (F & F_GRID) {
            OT *g = dst + ((desc >> 16) & 15u);
            g[0] = (OT)((in.g_pimp - b.lo[2]) / b.sp[2]);
            g[1] = (OT)((in.g_pexp - b.lo[3]) / b.sp[3]);
            g[2] = (OT)((in.g_co2 - b.lo[4]) / b.sp[4]);
            g[3] = (OT)((in.g_stat - b.lo[5]) / b.sp[5]);
        }
    } else {
        observe_row_h0<F>(*a_dev, i, t_row, p, s, dst, a_dev->pm_pitch);
    }
}

// A FULL wave's 64 rows out of its LDS tile (row-major, as they lie in memory) with 16-byte non-temporal stores: the streaming
// half of observe_row_h0_tiled, which builds its rows itself.  `out`: row 0 of the wave.
template <typename OT>
__device__ __forceinline__ void stream_row_tile(const OT *tile, OT *__restrict__ out, int32_t D)
{
    const int lane = threadIdx.x & 63;
    typedef OT vec2 __attribute__((ext_vector_type(2)));
    typedef OT vec4 __attribute__((ext_vector_type(4)));
    const int32_t total = 64 * D;
    if constexpr (sizeof(OT) == 8) {                     // D is even: a 16-byte pair never straddles the tile's end
        if ((reinterpret_cast<uintptr_t>(out) & 15) == 0) {
            for (int32_t e = 2 * lane; e < total; e += 128)
                __builtin_nontemporal_store(*reinterpret_cast<const vec2 *>(tile + e), reinterpret_cast<vec2 *>(out + e));
        } else {                                         // a caller's buffer at an odd 8-byte offset: word stores, same bytes
            for (int32_t e = lane; e < total; e += 64) out[e] = tile[e];
        }
    } else {
        if ((total & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
            for (int32_t e = 4 * lane; e < total; e += 256)
                __builtin_nontemporal_store(*reinterpret_cast<const vec4 *>(tile + e), reinterpret_cast<vec4 *>(out + e));
        } else {
            for (int32_t e = lane; e < total; e += 64) out[e] = tile[e];
        }
    }
}

// Whether the fused episode kernels send the per-step rows of a full wave through its LDS tile (1) or store them lane by lane (0)
#ifndef MGX_EPISODE_ROWS_TILE
#define MGX_EPISODE_ROWS_TILE 1
#endif

// Row `r64` (element offset (k * N + i) * D, 64-bit: [K, N, D] passes 2^32 bytes) of `obs` for this lane: through the wave's tile
// when the whole wave is here (wave-uniform test), else -- the last wave of a batch that is no multiple of 64 -- lane by lane.
template <int F>
__device__ __forceinline__ void store_episode_row(const KArgs *__restrict__ a_dev, int32_t T, uint32_t desc, void *__restrict__ obs,
                                                  int64_t r64, int64_t i, int32_t t_row, const Inputs &in, const RowBounds<F> &b,
                                                  const Params &p, const State &s, double *tile)
{
    const int32_t D = row_desc_dim(desc);
    if (MGX_EPISODE_ROWS_TILE && __builtin_amdgcn_read_exec() == ~0ull) {
        const int lane = threadIdx.x & 63;
        if (row_desc_f32(desc)) {
            float *tl = reinterpret_cast<float *>(tile);
            episode_row_h0<F>(a_dev, T, desc, i, t_row, in, b, p, s, tl + lane * D);
            __builtin_amdgcn_wave_barrier();
            stream_row_tile(tl, (float *)obs + (r64 - (int64_t)lane * D), D);
        } else {
            episode_row_h0<F>(a_dev, T, desc, i, t_row, in, b, p, s, tile + lane * D);
            __builtin_amdgcn_wave_barrier();
            stream_row_tile(tile, (double *)obs + (r64 - (int64_t)lane * D), D);
        }
        __builtin_amdgcn_wave_barrier();                 // (the next step's rows go into the same tile)
    } else if (row_desc_f32(desc)) episode_row_h0<F>(a_dev, T, desc, i, t_row, in, b, p, s, (float *)obs + r64);
    else episode_row_h0<F>(a_dev, T, desc, i, t_row, in, b, p, s, (double *)obs + r64);
}

// the row before a restart: only the restarting lanes are here (a divergent branch), so lane by lane
template <int F>
__device__ __forceinline__ void store_final_row(const KArgs *__restrict__ a_dev, int32_t T, uint32_t desc, void *__restrict__ final_obs,
                                                int64_t r64, int64_t i, int32_t t_row, const Inputs &in, const RowBounds<F> &b,
                                                const Params &p, const State &s)
{
    if (row_desc_f32(desc)) episode_row_h0<F>(a_dev, T, desc, i, t_row, in, b, p, s, (float *)final_obs + r64);
    else episode_row_h0<F>(a_dev, T, desc, i, t_row, in, b, p, s, (double *)final_obs + r64);
}

// The arguments of the two kernels, ONE struct by value each (late_kernargs)
struct RolloutRowsArgs {
    KArgs a;
    PLWords tab;
    const uint8_t *ids;
    int32_t t0, K;
    FusedOut out;
    mgx_episode_stats es;
    int32_t gpb;
    uint32_t desc;                   // pack_row_desc(a)
    const KArgs *a_dev;
    void *obs, *final_obs;
};
struct StepRowsArgs {
    KArgs a;
    const void *actions;
    int32_t t0, K;
    int32_t normalized, gpb;
    FusedOut out;
    mgx_episode_stats es;
    uint32_t desc;                   // pack_row_desc(a)
    const KArgs *a_dev;
    void *obs, *final_obs;
};

// ---- host side: what mgx_abi.hip hands the slices of the two translation units ----
struct EpisodeRowsLaunch {
    EpisodeLaunch e;                 // as for rollout_episodes_kernel / step_k_episodes_kernel
    void *obs, *final_obs;           // [K, N, D] in the handle's observation format; each may be NULL (not both)
};
bool launch_rollout_episodes_rows_p0(const EpisodeRowsLaunch &L); bool launch_rollout_episodes_rows_p1(const EpisodeRowsLaunch &L);
bool launch_step_k_episodes_rows_p0(const EpisodeRowsLaunch &L); bool launch_step_k_episodes_rows_p1(const EpisodeRowsLaunch &L);

}  // namespace mgx
