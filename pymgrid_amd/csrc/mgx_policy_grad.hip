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
// ONE kernel text for the two heads (PolicyGradHead, the last template argument): the softmax head of the discrete policy
// (mgx_policy_grad) and the Gaussian head of the continuous one (mgx_policy_grad_gaussian: the density of the pre-clip action by the
// rule of mgx_gaussian, policy_log / policy_exp / gaussian_lane_const of mgx_policy.hpp).  A head (PgHead) is what lies between the
// forward outputs and dy, the statistic rows and rows 0 .. 11 of the dY tile; everything else -- the operand reads, the MFMAs, the
// hidden-tile passes, the epilogue, the finish kernel -- is stated once.  An object holds one head of one slice.
#include "mgx_policy_grad.hpp"

#ifndef MGX_POLICY_GRAD_PART
#define MGX_POLICY_GRAD_PART 0
#endif
#ifndef MGX_POLICY_GRAD_HEAD
#define MGX_POLICY_GRAD_HEAD 0
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

// ---- the heads: from the forward outputs y of one sample to dy, its ratio, policy loss and entropy, and to rows 0 .. 11 of the
// dY tile.  `on`: the head is on for the lane (off: no policy and entropy terms, the value term stays); `active`: the surrogate's gate.
template <int HEAD>
struct PgHead;

// The softmax head of the discrete policy: the rule of mgx_policy_grad, the forward text that of the sampling launch (policy_argmax,
// policy_exp: mgx_policy.hpp), so the probability ratio of an un-updated policy is exactly 1.0.
template <>
struct PgHead<PG_HEAD_SOFTMAX> {
    static constexpr int NO = PG_NO;
    struct Sample {
        double rho, pl, H;
        bool on, active;
    };
    double beta;                                                                // of the lane's grid; negative: the greedy head (off)
    __device__ __forceinline__ PgHead(const PolicyGradArgs &g, int64_t ic) : beta(sample_lane_beta(g.sa, ic)) {}
    __device__ __forceinline__ Sample sample(const PolicyGradArgs &g, int64_t e64, int32_t nr, bool live, double A, const double (&y)[NO],
                                             double (&dy)[NO]) const
    {
        const bool sampling = beta >= 0.0;                                      // (false: the greedy head, no policy and entropy terms)
        const double b = sampling ? beta : 0.0;
        const double hi = g.hi, lo = g.lo, ec = g.ent_coef;
        const int32_t a = (int32_t)g.action_id[e64];
        const double old = g.old_prob[e64];
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
        Sample r;
        r.on = sampling;
        r.rho = (sampling ? e_a / S : 1.0) / old;
        r.active = !((A > 0.0 && r.rho > hi) || (A < 0.0 && r.rho < lo));
        const double c_s = sampling && r.active ? -(A * r.rho) : 0.0;
        r.pl = sampling ? (r.active ? c_s : -(A * (A > 0.0 ? hi : lo))) : 0.0;
        const double lnS = policy_log(S);
        double pi[NO], Hs = 0.0;
#pragma unroll
        for (int o = 0; o < NO; o++) {
            pi[o] = e[o] / S;
            d[o] = d[o] - lnS;                                                  // logpi[o], where e[o] > 0
            Hs = e[o] > 0.0 ? Hs + pi[o] * d[o] : Hs;
        }
        r.H = -Hs;
#pragma unroll
        for (int o = 0; o < NO; o++) {
            const double ent = e[o] > 0.0 ? pi[o] * (d[o] + r.H) : 0.0;
            const double v = b * (c_s * ((o == a ? 1.0 : 0.0) - pi[o]) + ec * ent);
            dy[o] = live && sampling ? v : 0.0;
        }
        return r;
    }
    __device__ __forceinline__ void rows(double *row, bool, const double (&dy)[NO], const Sample &) const
    {
#pragma unroll
        for (int o = 0; o < NO; o++) row[o] = dy[o];
    }
};

// The Gaussian head of the continuous policy: the rule of mgx_policy_grad_gaussian.  s[o], the live columns and the constant C are
// those of mgx_gaussian (gaussian_lane_const); the density is that of the pre-clip action the launch returned.  sigma[o] past the
// policy's n_out is 0.0 (the host side sees to it): such a column is dead, and its raw action is never read.
template <>
struct PgHead<PG_HEAD_GAUSSIAN> {
    static constexpr int NO = PG_NO_GAUSSIAN;
    struct Sample {
        double rho, pl, H;
        bool on, active;
        double dls[NO], kl;
    };
    double sc, C, Hc;                                                           // the lane's scale, its C and its entropy: constants of the grid
    __device__ __forceinline__ PgHead(const PolicyGradArgs &g, int64_t ic)
    {
        sc = explore_lane_scale(g.gs.scale, ic);
        C = gaussian_lane_const<NO>([&](int o) { return g.gs.sigma[o]; }, sc);
        double H = 0.0;
#pragma unroll
        for (int o = 0; o < NO; o++) {
            const double s = g.gs.sigma[o] * sc;
            const bool lv = s > 0.0;
            const double term = policy_log(lv ? s : 1.0) + 1.4189385332046727;  // (1 + log(2 pi)) / 2
            H = lv ? H + term : H;
        }
        Hc = H;
    }
    __device__ __forceinline__ Sample sample(const PolicyGradArgs &g, int64_t e64, int32_t nr, bool live, double A, const double (&y)[NO],
                                             double (&dy)[NO]) const
    {
        const double hi = g.hi, lo = g.lo, ec = g.ent_coef;
        const double *__restrict__ rp = g.raw_action + e64 * nr;
        double zeta[NO], sd[NO], Q = 0.0;
        bool lv[NO], any = false;
#pragma unroll
        for (int o = 0; o < NO; o++) {
            const double s = g.gs.sigma[o] * sc;
            lv[o] = s > 0.0;                                                    // (false past n_out: sigma is 0.0 there)
            sd[o] = lv[o] ? s : 1.0;
            const double raw = o < nr ? rp[o] : 0.0;
            zeta[o] = (raw - y[o]) / sd[o];
            Q = lv[o] ? Q + zeta[o] * zeta[o] : Q;
            any = any || lv[o];
        }
        const double logp = (-0.5 * Q) - C;
        const double Dl = logp - g.old_prob[e64];
        const bool nan = Dl != Dl;
        const double Dz = nan ? 0.0 : Dl;
        const bool down = Dz <= 0.0;
        const double m = down ? Dz : -Dz;
        const double E = policy_exp(m < -708.0 ? -708.0 : m);
        Sample r;
        r.on = any;
        r.rho = nan ? __builtin_nan("") : (down ? E : 1.0 / E);
        r.active = !((A > 0.0 && r.rho > hi) || (A < 0.0 && r.rho < lo));
        const double c_s = any && r.active ? -(A * r.rho) : 0.0;
        r.pl = any ? (r.active ? c_s : -(A * (A > 0.0 ? hi : lo))) : 0.0;
        r.H = Hc;
        r.kl = any ? (r.rho - 1.0) - Dl : 0.0;
#pragma unroll
        for (int o = 0; o < NO; o++) {
            const bool on = live && lv[o];
            dy[o] = on ? c_s * (zeta[o] / sd[o]) : 0.0;
            r.dls[o] = on ? (c_s * (zeta[o] * zeta[o] - 1.0)) - ec : 0.0;
        }
        return r;
    }
    __device__ __forceinline__ void rows(double *row, bool live, const double (&dy)[NO], const Sample &r) const
    {
#pragma unroll
        for (int o = 0; o < NO; o++) {
            row[o] = dy[o];
            row[PG_ROW_DLS + o] = r.dls[o];
        }
        row[PG_ROW_KL] = live ? r.kl : 0.0;
#pragma unroll
        for (int j = PG_ROW_KL + 1; j < PG_ROW_DV; j++) row[j] = 0.0;
    }
};

template <int D, bool CRITIC, int HEAD>
__global__ __launch_bounds__(BLOCK_K) void policy_grad_kernel(const PolicyGradArgs g)
{
    constexpr int NO = PgHead<HEAD>::NO;
    static_assert(BLOCK_K == PG_TILE_DOUBLES, "one thread per element of an accumulator tile");
    static_assert(NO <= PG_ROW_DV && PG_ROW_DV == 12 && PG_ROW_STATS == 13, "the rows of the dY tile");
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
    const PgHead<HEAD> head(g, ic);
    const uint8_t *__restrict__ mask = g.mask;
    const double vf = g.vf_coef;
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
        const double A = g.advantage[e64];
        // ---- forward: the launch's own text ----
        [[maybe_unused]] double V = 0.0;
        if constexpr (CRITIC) policy_outputs_value<D, NO>(policy_lds, nh, no, x, y, V);
        else policy_outputs<D, NO>(policy_lds, nh, no, x, y);
        // ---- the head: dy, the ratio, the sample's policy loss and entropy ----
        double dy[NO];
        const typename PgHead<HEAD>::Sample smp = head.sample(g, e64, nr, live, A, y, dy);
        double dv = 0.0, vl = 0.0;
        if constexpr (CRITIC) {
            const double diff = V - g.returns[e64];
            dv = live ? vf * diff : 0.0;
            vl = 0.5 * (diff * diff);
        }
        if (live && g.ratio_out) g.ratio_out[e64] = smp.rho;
        n_live += __builtin_popcountll(__ballot(live));
        n_clip += __builtin_popcountll(__ballot(live && smp.on && !smp.active));
        // ---- the reduction: X | 1, then dY | dv | the three statistics, then per hidden tile H_t and dH_t through the wave's tile ----
        double xop[16], dyop[16], op[16];
#pragma unroll
        for (int j = 0; j < PG_TILE; j++) row[j] = j < D ? (live ? x[j] : 0.0) : (j == 12 && live ? 1.0 : 0.0);
        pg_wave_sync();
        pg_read_operands(tile, lane, xop);
        pg_wave_sync();
        head.rows(row, live, dy, smp);
        row[PG_ROW_DV] = dv;
        row[PG_ROW_STATS] = live ? smp.pl : 0.0;
        row[PG_ROW_STATS + 1] = live ? vl : 0.0;
        row[PG_ROW_STATS + 2] = live && smp.on ? smp.H : 0.0;
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
    if (critic) policy_grad_kernel<D, true, MGX_POLICY_GRAD_HEAD><<<grid, BLOCK_K, lds_bytes, stream>>>(g);
    else policy_grad_kernel<D, false, MGX_POLICY_GRAD_HEAD><<<grid, BLOCK_K, lds_bytes, stream>>>(g);
}

#define MGX_PG_CAT2(a, b) a##b
#define MGX_PG_CAT(a, b) MGX_PG_CAT2(a, b)
#if MGX_POLICY_GRAD_HEAD == 0
#define MGX_PG_LAUNCH launch_policy_grad_p
#else
#define MGX_PG_LAUNCH launch_policy_grad_gaussian_p
#endif
bool MGX_PG_CAT(MGX_PG_LAUNCH, MGX_POLICY_GRAD_PART)(const PolicyGradArgs &g, int32_t D, bool critic, unsigned lds_bytes, hipStream_t stream)
{
    constexpr int D0 = MGX_POLICY_GRAD_PART * PG_PART_DIMS + 1;
    switch (D - D0) {
        case 0: policy_grad_launch<D0>(g, critic, lds_bytes, stream); return true;
        case 1: policy_grad_launch<D0 + 1>(g, critic, lds_bytes, stream); return true;
        case 2: policy_grad_launch<D0 + 2>(g, critic, lds_bytes, stream); return true;
        default: return false;
    }
}

#if MGX_POLICY_GRAD_PART == 0 && MGX_POLICY_GRAD_HEAD == 0
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
            else if (r == PG_ROW_DV) dst = f.g_cb;
            else if (r >= PG_ROW_STATS) dst = f.stats ? f.stats + (r - PG_ROW_STATS) : nullptr;
            else if (r >= PG_ROW_DLS && r < PG_ROW_DLS + PG_NO_GAUSSIAN) dst = f.g_ls ? f.g_ls + (r - PG_ROW_DLS) : nullptr;   // (the Gaussian head's rows)
            else if (r == PG_ROW_KL) dst = f.kl;
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
