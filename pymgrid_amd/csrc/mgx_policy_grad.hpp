// mgx_policy_grad.hpp -- what mgx_abi.hip hands mgx_policy_grad.hip: the arguments of policy_grad_kernel and policy_grad_finish_kernel
// (mgx_policy_grad and mgx_policy_grad_gaussian, include/mgx.h), the shape of the launch and the size of its workspace.
#pragma once
#include "mgx_policy.hpp"

namespace mgx {

constexpr int PG_TILE = 16;                                   // rows and columns of an accumulator tile (v_mfma_f64_16x16x4_f64)
constexpr int PG_TILE_DOUBLES = PG_TILE * PG_TILE;
constexpr int PG_NO = 12;                                     // outputs of a discrete policy, at most
constexpr int PG_NO_GAUSSIAN = 4;                             // ... of a continuous one: the action columns (staged as four, the padding with zero weights)
constexpr int PG_MAX_HIDDEN_TILES = MGX_POLICY_MAX_HIDDEN / PG_TILE;
constexpr int PG_MIN_CHUNK = 4;                               // steps of a workgroup, at least: staging and the epilogue are paid per chunk
constexpr int PG_TARGET_BLOCKS = 2048;                        // workgroups the launch aims at (8 per CU) before a chunk grows past PG_MIN_CHUNK

// The head of the kernel: what lies between the forward outputs and dy, dv and the statistic rows -- the last template argument of
// policy_grad_kernel, its objects' -DMGX_POLICY_GRAD_HEAD
enum PolicyGradHead : int { PG_HEAD_SOFTMAX = 0, PG_HEAD_GAUSSIAN = 1 };

// The accumulator tiles of a wave, in the order of the workspace: tile 0 = (dY | dv | stats)^T (X | 1); per hidden tile t:
// tile 1 + 2t = (dY | dv)^T H_t, tile 2 + 2t = dH_t^T (X | 1).  The rows of dY | dv | stats: 0 .. 11 the head's (the softmax head:
// dy[0 .. 12); the Gaussian head: dy[0 .. 4), dls[0 .. 4) at PG_ROW_DLS, kl at PG_ROW_KL, zeros), 12 dv, 13 .. 15 the policy loss,
// the value loss and the entropy.
constexpr int PG_ROW_DLS = 4, PG_ROW_KL = 8, PG_ROW_DV = 12, PG_ROW_STATS = 13;
__host__ __device__ inline int32_t policy_grad_tiles(int32_t n_hidden) { return 1 + 2 * ((n_hidden + PG_TILE - 1) / PG_TILE); }
// doubles a workgroup leaves in the workspace: its tiles, then the live and the clipped count (two 64-bit integers)
__host__ __device__ inline int32_t policy_grad_block_doubles(int32_t n_hidden) { return policy_grad_tiles(n_hidden) * PG_TILE_DOUBLES + 2; }

struct PolicyGradShape {
    int32_t kc;                      // steps per chunk
    unsigned bx, by;                 // workgroups over the grids, chunks over k
};
inline PolicyGradShape policy_grad_shape(int64_t N, int32_t K)
{
    PolicyGradShape s;
    s.bx = (unsigned)((N + BLOCK_K - 1) / BLOCK_K);
    const int64_t want = (PG_TARGET_BLOCKS + (int64_t)s.bx - 1) / (int64_t)s.bx;   // chunks that would reach the target
    int64_t kc = ((int64_t)K + want - 1) / want;
    if (kc < PG_MIN_CHUNK) kc = PG_MIN_CHUNK;
    if (kc > K) kc = K;
    s.kc = (int32_t)kc;
    s.by = (unsigned)((K + s.kc - 1) / s.kc);
    return s;
}

struct PolicyGradArgs {
    PolicyArgs pol;                  // one set (n_policies = 1, index NULL); stride: doubles of the staged set
    CriticArgs cr;                   // read by the forms with a critic alone
    SampleArgs sa;                   // the softmax head: temperature and scale (no draw is made)
    GaussianArgs gs;                 // the Gaussian head: sigma (0.0 past n_out) and scale (no draw is made)
    int64_t N;
    int32_t K, kc;
    int32_t x_f32;                   // the rows are float32 (widened as a policy launch widens them)
    const void *x;                   // [K, N, D]
    const uint8_t *action_id;        // [K, N]: the softmax head
    const double *raw_action;        // [K, N, n_out]: the Gaussian head
    const double *old_prob, *advantage;   // [K, N]; old_prob: the Gaussian head's old_logp
    const double *returns;           // [K, N]; NULL without a critic
    const uint8_t *mask;             // [K, N] or NULL
    double hi, lo, vf_coef, ent_coef;     // hi = 1 + eps, lo = 1 - eps: formed once on the host
    double *ratio_out;               // [K, N] or NULL
    double *ws;                      // [by * bx][policy_grad_block_doubles]
};

struct PolicyGradFinishArgs {
    const double *ws;
    int32_t n_blocks, n_hidden, n_out, D;
    double *g_w1, *g_b1, *g_w2, *g_b2, *g_cw, *g_cb, *stats;   // each may be NULL
    double *g_ls, *kl;               // rows PG_ROW_DLS .. + 3 and PG_ROW_KL of the "1" column: the Gaussian head's; NULL in the discrete call
};

// one slice of the kernels of one head each: slice p holds the row widths D = 3p + 1 .. 3p + 3 (-DMGX_POLICY_GRAD_PART=p
// -DMGX_POLICY_GRAD_HEAD=h); the finish kernel lies in slice 0 of the softmax head
constexpr int PG_PART_DIMS = 3;
bool launch_policy_grad_p0(const PolicyGradArgs &g, int32_t D, bool critic, unsigned lds_bytes, hipStream_t stream);
bool launch_policy_grad_p1(const PolicyGradArgs &g, int32_t D, bool critic, unsigned lds_bytes, hipStream_t stream);
bool launch_policy_grad_p2(const PolicyGradArgs &g, int32_t D, bool critic, unsigned lds_bytes, hipStream_t stream);
bool launch_policy_grad_p3(const PolicyGradArgs &g, int32_t D, bool critic, unsigned lds_bytes, hipStream_t stream);
bool launch_policy_grad_gaussian_p0(const PolicyGradArgs &g, int32_t D, bool critic, unsigned lds_bytes, hipStream_t stream);
bool launch_policy_grad_gaussian_p1(const PolicyGradArgs &g, int32_t D, bool critic, unsigned lds_bytes, hipStream_t stream);
bool launch_policy_grad_gaussian_p2(const PolicyGradArgs &g, int32_t D, bool critic, unsigned lds_bytes, hipStream_t stream);
bool launch_policy_grad_gaussian_p3(const PolicyGradArgs &g, int32_t D, bool critic, unsigned lds_bytes, hipStream_t stream);
void launch_policy_grad_finish(const PolicyGradFinishArgs &f, hipStream_t stream);

}  // namespace mgx
