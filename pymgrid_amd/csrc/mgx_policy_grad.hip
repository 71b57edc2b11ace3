// mgx_policy_grad.hip -- the gradient of the PPO-clip / A2C loss with respect to the parameters of a discrete mgx_policy and its
// mgx_critic (mgx_policy_grad, include/mgx.h), from what the sampling launch returned.  One lane per sample; a wave owns 64
// consecutive grids and a chunk of k (blockIdx.y).  The forward pass is the text of the launch itself (stage_policy_critic,
// policy_outputs_value, policy_argmax, policy_exp: mgx_policy.hpp), so the probability ratio of an un-updated policy is exactly 1.0.
// The sum over the samples is a product of two tall matrices -- g_w1 = dH^T X, g_w2 | g_cw = (dY | dv)^T H -- and goes through the
// matrix cores: every step each lane writes its row of X, dY, H_t, dH_t into the wave's LDS tile [64][16 (+ 1)], the wave reads the
// tile back in operand order, four samples per v_mfma_f64_16x16x4_f64, and the 16 x 16 accumulators stay in registers for the whole
// chunk.  One tile serves all four operands in turn: the operands of X and dY are kept in registers (16 doubles each) across the
// hidden tiles.  At the end the four waves of a workgroup are added in wave order and the workgroup's partial goes to the workspace
// with vector stores; policy_grad_finish_kernel adds the partials in a fixed order, multiplies by 1 / M and scatters.  No atomics.
#include "mgx_policy_grad.hpp"

#ifndef MGX_POLICY_GRAD_PART
#define MGX_POLICY_GRAD_PART 0
#endif

namespace mgx {

typedef double pg_f64x4 __attribute__((ext_vector_type(4)));

constexpr int PG_PITCH = PG_TILE + 1;                         // doubles between the rows of two lanes: 64 b64 writes meet no bank twice
constexpr int PG_WAVES = BLOCK_K / 64;
static_assert(64 * PG_PITCH >= PG_TILE_DOUBLES, "a wave's tile holds one accumulator tile in the epilogue");

// what the lanes wrote is what the wave reads back (and the other way round): LDS accesses of one wave complete in order
__device__ __forceinline__ void pg_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the 16 operands of a [64][16] tile: step s takes element (sample 4s + (lane >> 4), column lane & 15) -- A[row = lane & 15][k = lane >> 4]
// and B[k = lane >> 4][col = lane & 15] of v_mfma_f64_16x16x4_f64 alike
__device__ __forceinline__ void pg_read_operands(const double *tile, int lane, double (&op)[16])
{
    const double *q = tile + (lane >> 4) * PG_PITCH + (lane & 15);
#pragma unroll
    for (int s = 0; s < 16; s++) op[s] = q[s * 4 * PG_PITCH];
}

// acc += A^T B over the wave's 64 samples, A and B as pg_read_operands holds them
__device__ __forceinline__ void pg_mfma(const double (&a)[16], const double (&b)[16], pg_f64x4 &acc)
{
#pragma unroll
    for (int s = 0; s < 16; s++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[s], acc, 0, 0, 0);
}

// The workgroup's sum of one accumulator tile into the workspace: every wave lays its tile out as [row][col] (C/D of the f64 MFMA:
// col = lane & 15, row = (lane >> 4) + 4 * reg), thread e adds element e of waves 0 .. 3 in this order.  Two workgroup barriers.
__device__ __forceinline__ void pg_store_tile(const pg_f64x4 &acc, double *tiles, double *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    double *mine = tiles + (threadIdx.x >> 6) * (64 * PG_PITCH);
#pragma unroll
    for (int r = 0; r < 4; r++) mine[((lane >> 4) + 4 * r) * PG_TILE + (lane & 15)] = acc[r];
    __syncthreads();
    double v = tiles[threadIdx.x];
#pragma unroll
    for (int w = 1; w < PG_WAVES; w++) v = v + tiles[w * (64 * PG_PITCH) + threadIdx.x];
    out[threadIdx.x] = v;
    __syncthreads();
}

template <int D, bool CRITIC>
__global__ __launch_bounds__(BLOCK_K) void policy_grad_kernel(const PolicyGradArgs g)
{
    constexpr int NO = PG_NO;
    static_assert(BLOCK_K == PG_TILE_DOUBLES, "one thread per element of an accumulator tile");
    extern __shared__ __attribute__((aligned(16))) double policy_lds[];
    __shared__ __attribute__((aligned(16))) double tiles[PG_WAVES * 64 * PG_PITCH];
    __shared__ long long counts[PG_WAVES][2];
    if constexpr (CRITIC) stage_policy_critic(g.pol, g.cr, D, policy_lds);      // (ends in a barrier; no lane leaves before the end)
    else stage_policy(g.pol, D, policy_lds);
    const int lane = threadIdx.x & 63;
    double *tile = tiles + (threadIdx.x >> 6) * (64 * PG_PITCH);
    double *row = tile + lane * PG_PITCH;
    const int64_t N = g.N;
    const int64_t i = (int64_t)blockIdx.x * BLOCK_K + threadIdx.x;
    const bool in = i < N;
    const int64_t ic = in ? i : N - 1;                                          // a lane past N reads grid N - 1 and supplies zeros
    const int32_t nh = g.pol.n_hidden, no = g.pol.n_out, nr = g.pol.n_real;
    const int32_t nt = (nh + PG_TILE - 1) / PG_TILE;
    const int32_t rec = D + 1 + no + (CRITIC ? 1 : 0);                          // a unit's record in the staged set
    const double *units = policy_lds + no + (CRITIC ? 1 : 0);
    const double beta = sample_lane_beta(g.sa, ic);
    const bool sampling = beta >= 0.0;                                          // (false: the greedy head, no policy and entropy terms)
    const double b = sampling ? beta : 0.0;
    const uint8_t *__restrict__ mask = g.mask;
    const double hi = g.hi, lo = g.lo, vf = g.vf_coef, ec = g.ent_coef;
    pg_f64x4 acc0 = {0.0, 0.0, 0.0, 0.0};
    pg_f64x4 acc_w2[PG_MAX_HIDDEN_TILES], acc_w1[PG_MAX_HIDDEN_TILES];
#pragma unroll
    for (int t = 0; t < PG_MAX_HIDDEN_TILES; t++) acc_w2[t] = acc_w1[t] = acc0;
    long long n_live = 0, n_clip = 0;
    const int32_t k0 = (int32_t)blockIdx.y * g.kc;
    const int32_t k1 = k0 + g.kc < g.K ? k0 + g.kc : g.K;
#pragma nounroll
    for (int32_t k = k0; k < k1; k++) {
        const int64_t e64 = (int64_t)k * N + ic;
        const bool live = in && (!mask || mask[e64] != 0);
        double x[D], y[NO];
        if (g.x_f32) {
            const float *__restrict__ xp = (const float *)g.x + e64 * D;
#pragma unroll
            for (int j = 0; j < D; j++) x[j] = (double)xp[j];
        } else {
            const double *__restrict__ xp = (const double *)g.x + e64 * D;
#pragma unroll
            for (int j = 0; j < D; j++) x[j] = xp[j];
        }
        const int32_t a = (int32_t)g.action_id[e64];
        const double old = g.old_prob[e64], A = g.advantage[e64];
        // ---- forward: the launch's own text ----
        [[maybe_unused]] double V = 0.0;
        if constexpr (CRITIC) policy_outputs_value<D, NO>(policy_lds, nh, no, x, y, V);
        else policy_outputs<D, NO>(policy_lds, nh, no, x, y);
        double best;
        const int32_t gid = policy_argmax<NO>(y, nr, best);
        double d[NO], e[NO];                                                    // d[o], and the weights e[o] of mgx_sampling
        double S = 0.0;
#pragma unroll
        for (int c = 0; c < NO; c += 4) {
            if (c < nr) {
#pragma unroll
                for (int o = c; o < c + 4; o++) {
                    const double dd = (y[o] - best) * b;
                    const bool inr = dd >= -708.0;                              // (false for a NaN)
                    const double E = policy_exp(inr ? dd : -708.0);
                    e[o] = o < nr ? (o == gid ? 1.0 : (inr ? E : 0.0)) : 0.0;
                    d[o] = o == gid ? 0.0 : dd;
                    S = S + e[o];
                }
            } else {
#pragma unroll
                for (int o = c; o < c + 4; o++) e[o] = d[o] = 0.0;
            }
        }
        double e_a = 0.0;
#pragma unroll
        for (int o = 0; o < NO; o++) e_a = o == a ? e[o] : e_a;
        const double rho = (sampling ? e_a / S : 1.0) / old;
        const bool active = !((A > 0.0 && rho > hi) || (A < 0.0 && rho < lo));
        const double c_s = sampling && active ? -(A * rho) : 0.0;
        const double pl = sampling ? (active ? c_s : -(A * (A > 0.0 ? hi : lo))) : 0.0;
        const double lnS = policy_log(S);
        double pi[NO], Hs = 0.0;
#pragma unroll
        for (int o = 0; o < NO; o++) {
            pi[o] = e[o] / S;
            d[o] = d[o] - lnS;                                                  // logpi[o], where e[o] > 0
            Hs = e[o] > 0.0 ? Hs + pi[o] * d[o] : Hs;
        }
        const double H = -Hs;
        double dy[NO];
#pragma unroll
        for (int o = 0; o < NO; o++) {
            const double ent = e[o] > 0.0 ? pi[o] * (d[o] + H) : 0.0;
            const double v = b * (c_s * ((o == a ? 1.0 : 0.0) - pi[o]) + ec * ent);
            dy[o] = live && sampling ? v : 0.0;
        }
        double dv = 0.0, vl = 0.0;
        if constexpr (CRITIC) {
            const double diff = V - g.returns[e64];
            dv = live ? vf * diff : 0.0;
            vl = 0.5 * (diff * diff);
        }
        if (live && g.ratio_out) g.ratio_out[e64] = rho;
        n_live += __builtin_popcountll(__ballot(live));
        n_clip += __builtin_popcountll(__ballot(live && sampling && !active));
        // ---- the reduction: X | 1, then dY | dv | the three statistics, then per hidden tile H_t and dH_t through the wave's tile ----
        double xop[16], dyop[16], op[16];
#pragma unroll
        for (int j = 0; j < PG_TILE; j++) row[j] = j < D ? (live ? x[j] : 0.0) : (j == 12 && live ? 1.0 : 0.0);
        pg_wave_sync();
        pg_read_operands(tile, lane, xop);
        pg_wave_sync();
#pragma unroll
        for (int o = 0; o < NO; o++) row[o] = dy[o];
        row[12] = dv;
        row[13] = live ? pl : 0.0;
        row[14] = live ? vl : 0.0;
        row[15] = live && sampling ? H : 0.0;
        pg_wave_sync();
        pg_read_operands(tile, lane, dyop);
        pg_wave_sync();
        pg_mfma(dyop, xop, acc0);
#pragma unroll
        for (int t = 0; t < PG_MAX_HIDDEN_TILES; t++) {
            if (t < nt) {
                // H_t: the units of this tile by the rule of mgx_policy, zero past n_hidden and on a dead lane
#pragma nounroll
                for (int32_t uu = 0; uu < PG_TILE; uu++) {
                    const int32_t u = t * PG_TILE + uu;
                    const double *w = units + (u < nh ? u : nh - 1) * rec;
                    double h = w[D];
#pragma unroll
                    for (int j = 0; j < D; j++) h = h + w[j] * x[j];
                    row[uu] = live && u < nh && h > 0.0 ? h : 0.0;
                }
                pg_wave_sync();
                pg_read_operands(tile, lane, op);
                pg_wave_sync();
                pg_mfma(dyop, op, acc_w2[t]);
                // dH_t over it: a lane reads its own h back and writes dh in its place
#pragma nounroll
                for (int32_t uu = 0; uu < PG_TILE; uu++) {
                    const int32_t u = t * PG_TILE + uu;
                    const double *w = units + (u < nh ? u : nh - 1) * rec + D + 1 + (CRITIC ? 1 : 0);
                    double s = 0.0;
#pragma unroll
                    for (int c = 0; c < NO; c += 4)
                        if (c < no) {
#pragma unroll
                            for (int o = c; o < c + 4; o++) s = s + w[o] * dy[o];
                        }
                    if constexpr (CRITIC) s = s + w[-1] * dv;
                    row[uu] = row[uu] > 0.0 ? s : 0.0;
                }
                pg_wave_sync();
                pg_read_operands(tile, lane, op);
                pg_wave_sync();
                pg_mfma(op, xop, acc_w1[t]);
            }
        }
    }
    // ---- the workgroup's partial: its tiles, waves added in wave order, then the two counts ----
    __syncthreads();
    double *__restrict__ out = g.ws + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * policy_grad_block_doubles(nh);
    pg_store_tile(acc0, tiles, out);
#pragma unroll
    for (int t = 0; t < PG_MAX_HIDDEN_TILES; t++) {
        if (t < nt) {
            pg_store_tile(acc_w2[t], tiles, out + (1 + 2 * t) * PG_TILE_DOUBLES);
            pg_store_tile(acc_w1[t], tiles, out + (2 + 2 * t) * PG_TILE_DOUBLES);
        }
    }
    if (lane == 0) {
        counts[threadIdx.x >> 6][0] = n_live;
        counts[threadIdx.x >> 6][1] = n_clip;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        long long c = 0;
#pragma unroll
        for (int w = 0; w < PG_WAVES; w++) c += counts[w][threadIdx.x];
        reinterpret_cast<long long *>(out + policy_grad_tiles(nh) * PG_TILE_DOUBLES)[threadIdx.x] = c;
    }
}

template <int D>
static void policy_grad_launch(const PolicyGradArgs &g, bool critic, unsigned lds_bytes, hipStream_t stream)
{
    const PolicyGradShape s = policy_grad_shape(g.N, g.K);
    const dim3 grid(s.bx, s.by);
    if (critic) policy_grad_kernel<D, true><<<grid, BLOCK_K, lds_bytes, stream>>>(g);
    else policy_grad_kernel<D, false><<<grid, BLOCK_K, lds_bytes, stream>>>(g);
}

#define MGX_PG_CAT2(a, b) a##b
#define MGX_PG_CAT(a, b) MGX_PG_CAT2(a, b)
bool MGX_PG_CAT(launch_policy_grad_p, MGX_POLICY_GRAD_PART)(const PolicyGradArgs &g, int32_t D, bool critic, unsigned lds_bytes, hipStream_t stream)
{
    constexpr int D0 = MGX_POLICY_GRAD_PART * PG_PART_DIMS + 1;
    switch (D - D0) {
        case 0: policy_grad_launch<D0>(g, critic, lds_bytes, stream); return true;
        case 1: policy_grad_launch<D0 + 1>(g, critic, lds_bytes, stream); return true;
        case 2: policy_grad_launch<D0 + 2>(g, critic, lds_bytes, stream); return true;
        default: return false;
    }
}

#if MGX_POLICY_GRAD_PART == 0
// The partials added up, times 1 / M, into the caller's arrays.  A workgroup serves FIN_ELEMS elements of the tiles: thread
// (seg, el) adds the partials of its segment of workgroups in ascending order, thread (0, el) the segments in ascending order -- a
// fixed tree, the same from run to run.  M and the clipped count are integer sums, formed by every workgroup for itself.
constexpr int FIN_ELEMS = 16, FIN_SEGS = BLOCK_K / FIN_ELEMS;

__global__ __launch_bounds__(BLOCK_K) void policy_grad_finish_kernel(const PolicyGradFinishArgs f)
{
    __shared__ double part[FIN_SEGS][FIN_ELEMS];
    __shared__ long long cnt[2][BLOCK_K];
    const int32_t nh = f.n_hidden, B = f.n_blocks;
    const int32_t bd = policy_grad_block_doubles(nh), n_el = policy_grad_tiles(nh) * PG_TILE_DOUBLES;
    const double *__restrict__ ws = f.ws;
    const int32_t el = (int32_t)blockIdx.x * FIN_ELEMS + ((int32_t)threadIdx.x & (FIN_ELEMS - 1)), seg = (int32_t)threadIdx.x / FIN_ELEMS;
    long long live = 0, clip = 0;
    for (int32_t q = (int32_t)threadIdx.x; q < B; q += BLOCK_K) {
        const long long *c = reinterpret_cast<const long long *>(ws + (int64_t)q * bd + n_el);
        live += c[0];
        clip += c[1];
    }
    cnt[0][threadIdx.x] = live;
    cnt[1][threadIdx.x] = clip;
    const int32_t per = (B + FIN_SEGS - 1) / FIN_SEGS;
    const int32_t q0 = seg * per, q1 = q0 + per < B ? q0 + per : B;
    double v = 0.0;
    if (el < n_el)
        for (int32_t q = q0; q < q1; q++) v = v + ws[(int64_t)q * bd + el];
    part[seg][threadIdx.x & (FIN_ELEMS - 1)] = v;
    __syncthreads();
    if (seg != 0 || el >= n_el) return;
    long long M = 0, C = 0;
    for (int32_t q = 0; q < BLOCK_K; q++) {
        M += cnt[0][q];
        C += cnt[1][q];
    }
    const double inv = M > 0 ? 1.0 / (double)M : 0.0;
    double sum = part[0][threadIdx.x];
    for (int32_t s = 1; s < FIN_SEGS; s++) sum = sum + part[s][threadIdx.x];
    const double val = inv * sum;
    const int32_t D = f.D, nr = f.n_out;
    const int32_t ti = el / PG_TILE_DOUBLES, r = (el / PG_TILE) % PG_TILE, c = el % PG_TILE;
    double *dst = nullptr;
    if (ti == 0) {                                               // (dY | dv | stats)^T (X | 1): row o / 12 / 13 .. 15, column j / 12
        if (c == 12) {
            if (r < nr) dst = f.g_b2 ? f.g_b2 + r : nullptr;
            else if (r == 12) dst = f.g_cb;
            else if (r >= 13) dst = f.stats ? f.stats + (r - 13) : nullptr;
        } else if (nh == 0 && c < D) {
            if (r < nr) dst = f.g_w2 ? f.g_w2 + r * D + c : nullptr;
            else if (r == 12) dst = f.g_cw ? f.g_cw + c : nullptr;
        }
        if (el == 0 && f.stats) f.stats[3] = inv * (double)C;
    } else {
        const int32_t t = (ti - 1) >> 1;
        if ((ti - 1) & 1) {                                      // dH_t^T (X | 1): row u, column j / 12
            const int32_t u = t * PG_TILE + r;
            if (u < nh) {
                if (c < D) dst = f.g_w1 ? f.g_w1 + u * D + c : nullptr;
                else if (c == 12) dst = f.g_b1 ? f.g_b1 + u : nullptr;
            }
        } else {                                                 // (dY | dv)^T H_t: row o / 12, column u
            const int32_t u = t * PG_TILE + c;
            if (u < nh) {
                if (r < nr) dst = f.g_w2 ? f.g_w2 + r * nh + u : nullptr;
                else if (r == 12) dst = f.g_cw ? f.g_cw + u : nullptr;
            }
        }
    }
    if (dst) *dst = val;
}

void launch_policy_grad_finish(const PolicyGradFinishArgs &f, hipStream_t stream)
{
    const unsigned blocks = (unsigned)(policy_grad_tiles(f.n_hidden) * PG_TILE_DOUBLES / FIN_ELEMS);
    policy_grad_finish_kernel<<<blocks, BLOCK_K, 0, stream>>>(f);
}
#endif

}  // namespace mgx
