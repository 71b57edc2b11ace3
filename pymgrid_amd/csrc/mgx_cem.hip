// mgx_cem.hip -- the small kernels round the CEM what-if launch (mgx_cem / mgx_cem_refit, include/mgx.h): the pick that regenerates
// step 0 of the best candidate, the elites of a grid, and the refit of (mean, sigma) on them.  None of them reads a plan tensor:
// a candidate's controls are formed again from the draw (cem_candidate, mgx_cem.hpp).  Plain C++, vector stores.
#include "mgx_cem.hpp"
#include "mgx_lookahead.hpp"

namespace mgx {

constexpr int CEM_MAX_Y = 65535;     // plan steps per refit launch (gridDim.y); more: further launches from step k0 on

// x (A doubles) as row `e` (element offset) of `dst`, in the action format
template <int A>
__device__ __forceinline__ void store_cem_controls(void *dst, int64_t e, bool f32, const double (&x)[A])
{
#pragma unroll
    for (int o = 0; o < A; o++) {
        if (f32) ((float *)dst)[e + o] = (float)x[o];
        else ((double *)dst)[e + o] = x[o];
    }
}

// One lane per grid, as lookahead_pick_kernel: the steps counted, the first maximum over ret[:, i] by the rule of mgx_lookahead,
// and step 0 of that candidate out of row 0 of (mean, sigma).
template <int A>
__global__ __launch_bounds__(BLOCK) void cem_pick_kernel(const CemPick q)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= q.N) return;
    if (q.steps) q.steps[i] = lookahead_steps(q.t0, q.ep_final[i], q.H);
    if (!q.best && !q.best_ret && !q.first_action) return;
    int32_t b = 0;
    double bv = q.ret[i];
    for (int32_t c = 1; c < q.C; c++) {
        const double v = q.ret[(int64_t)c * q.N + i];
        if (v > bv) { bv = v; b = c; }
    }
    if (q.best) q.best[i] = b;
    if (q.best_ret) q.best_ret[i] = bv;
    if (q.first_action) {
        CemRow<A> row;
        load_cem_row<A>(q.mean, q.sigma, i, row);
        double x[A];
        cem_candidate<A>(q.key, i, b, 0, row.m, row.s, q.f32, x);
        store_cem_controls<A>(q.first_action, i * A, q.f32, x);
    }
}

void launch_cem_pick(const CemPick &q, hipStream_t stream)
{
    const unsigned blocks = (unsigned)((q.N + BLOCK - 1) / BLOCK);
    with_action_dim(q.A, [&](auto a) { cem_pick_kernel<decltype(a)::value><<<blocks, BLOCK, 0, stream>>>(q); });
}

// One lane per grid: elite[e, i] for e = 0 .. E - 1, the pick's rule among the candidates not yet taken.  "Taken" is read back from
// the lane's own column of `elite` (E <= 32 entries, written by this lane): E scans of ret[:, i], coalesced across grids.
__global__ __launch_bounds__(BLOCK) void cem_elite_kernel(const CemRefitArgs g)
{
    const int64_t N = g.N;
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= N) return;
    const double *__restrict__ ret = g.ret;
    int32_t *elite = g.elite;
    for (int32_t e = 0; e < g.E; e++) {
        int32_t b = -1;
        double bv = 0.0;
        for (int32_t c = 0; c < g.C; c++) {
            bool taken = false;
            for (int32_t j = 0; j < e; j++) taken = taken || elite[(int64_t)j * N + i] == c;
            if (taken) continue;
            const double v = ret[(int64_t)c * N + i];
            if (b < 0 || v > bv) { bv = v; b = c; }
        }
        elite[(int64_t)e * N + i] = b;                               // (E <= C: there is always a candidate left)
    }
}

void launch_cem_elite(const CemRefitArgs &g, hipStream_t stream)
{
    cem_elite_kernel<<<(unsigned)((g.N + BLOCK - 1) / BLOCK), BLOCK, 0, stream>>>(g);
}

// One lane per (grid i, plan step k = k0 + blockIdx.y).  The lane reads row (k, i) of mean / sigma before it writes row (k, i) of
// the outputs and nothing else of either, so the outputs may be the inputs.  The elites' controls are regenerated twice -- once for
// the mean, once for the deviation -- instead of held (E x A doubles a lane).
template <int A>
__global__ __launch_bounds__(BLOCK) void cem_refit_kernel(const CemRefitArgs g, int32_t k0)
{
    const int64_t N = g.N;
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= N) return;
    const int32_t k = k0 + (int32_t)blockIdx.y;
    const int64_t row = (int64_t)k * N * A;
    CemRow<A> r;
    load_cem_row<A>(g.mean + row, g.sigma + row, i, r);
    const int32_t n = g.steps ? g.steps[i] : g.H;
    const int32_t *elite = g.elite;
    const int32_t E = g.E;
    double x[A];
    if (g.best_plan) {
        cem_candidate<A>(g.key, i, elite[i], k, r.m, r.s, g.f32, x);
        store_cem_controls<A>(g.best_plan, row + i * A, g.f32, x);
    }
    double mo[A], so[A];
    if (k < n) {
        const double En = (double)E;
        double mu[A], q[A];
#pragma unroll
        for (int o = 0; o < A; o++) { mu[o] = 0.0; q[o] = 0.0; }
#pragma nounroll
        for (int32_t e = 0; e < E; e++) {
            cem_candidate<A>(g.key, i, elite[(int64_t)e * N + i], k, r.m, r.s, g.f32, x);
#pragma unroll
            for (int o = 0; o < A; o++) mu[o] = mu[o] + x[o];
        }
#pragma unroll
        for (int o = 0; o < A; o++) mu[o] = mu[o] / En;
#pragma nounroll
        for (int32_t e = 0; e < E; e++) {
            cem_candidate<A>(g.key, i, elite[(int64_t)e * N + i], k, r.m, r.s, g.f32, x);
#pragma unroll
            for (int o = 0; o < A; o++) {
                const double d = x[o] - mu[o];
                q[o] = q[o] + d * d;
            }
        }
#pragma unroll
        for (int o = 0; o < A; o++) {
            const double d = policy_sqrt(q[o] / En);
            mo[o] = g.alpha * mu[o] + g.beta * r.m[o];
            const double sg = g.alpha * d + g.beta * r.s[o];
            so[o] = sg > g.sigma_min ? sg : g.sigma_min;
        }
    } else {
#pragma unroll
        for (int o = 0; o < A; o++) { mo[o] = r.m[o]; so[o] = r.s[o]; }
    }
#pragma unroll
    for (int o = 0; o < A; o++) {
        g.mean_out[row + i * A + o] = mo[o];
        g.sigma_out[row + i * A + o] = so[o];
    }
}

void launch_cem_refit(const CemRefitArgs &g, hipStream_t stream)
{
    const unsigned blocks = (unsigned)((g.N + BLOCK - 1) / BLOCK);
    with_action_dim(g.A, [&](auto a) {
        for (int32_t k0 = 0; k0 < g.H; k0 += CEM_MAX_Y) {
            const dim3 grid(blocks, (unsigned)(g.H - k0 < CEM_MAX_Y ? g.H - k0 : CEM_MAX_Y));
            cem_refit_kernel<decltype(a)::value><<<grid, BLOCK, 0, stream>>>(g, k0);
        }
    });
}

}  // namespace mgx
