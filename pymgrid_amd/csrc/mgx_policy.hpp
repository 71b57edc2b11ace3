// mgx_policy.hpp -- what the two CLOSED-LOOP fused episode launches share (mgx_rollout_policy_episodes: mgx_policy_episodes.hip,
// mgx_step_k_policy_episodes: mgx_step_policy_episodes.hip): the policy of include/mgx.h (a small fp64 network of plain IEEE
// operations) staged in LDS once per workgroup and evaluated per lane between "row of the coming step" and "step", and the
// lane's row strip -- the H = 0 row is built ONCE per step into the wave's tile, read back as the policy's input and, where
// the launch returns observations, streamed out of the same tile as the row the step before returned.  Their twins with
// a head on the policy's outputs (one kernel text per family, the head a template argument: mgx_policy_head_episodes.hip,
// mgx_step_policy_head_episodes.hip) add, each stated once below: the exploring heads (mgx_rollout_policy_explore_episodes,
// mgx_step_k_policy_explore_episodes) the draw, the epsilon choice and the noise of mgx_exploration; the sampling head of the
// discrete launch (mgx_rollout_policy_sample_episodes) the exp and the softmax-sampling head of mgx_sampling; that head with a
// critic (mgx_rollout_policy_critic_episodes) the value head of mgx_critic, in functions of its own; the Gaussian heads of the
// continuous launch (mgx_step_k_policy_gaussian_episodes) the log, the quarter turn, the normal pair and the head of mgx_gaussian.
// On top of mgx_episode_rows.hpp (the rows) and, through it, mgx_episode_loop.hpp (what all six episode loops share).
#pragma once
#include "mgx_episode_rows.hpp"

namespace mgx {

// mgx_policy as the kernels see it.  `n_out`: the outputs of a STAGED set -- mgx_policy.n_out (`n_real`), which the discrete call
// rounds up to a multiple of four (policy_outputs).  `stride`: doubles of one staged set (policy_set_doubles, rounded up to even).
struct PolicyArgs {
    const double *w1, *b1, *w2, *b2;
    const int32_t *index;            // [N] or NULL
    int32_t n_policies, n_hidden, n_out, n_real, stride;
};

// One parameter set as it lies in LDS (doubles), for a row of D values:
//   n_hidden > 0:  b2[0 .. n_out) | per hidden unit u: W1[u, 0 .. D), b1[u], W2[0 .. n_out, u]
//   n_hidden = 0:  b2[0 .. n_out) | per input j: W2[0 .. n_out, j]
// -- in the order the evaluation walks it: a unit's pre-activation, then its contribution to every output.  The hidden vector is
// never stored: unit u is folded into the n_out running sums as soon as it is known, and every sum still receives its addends
// in the order u = 0, 1, ... the rule of include/mgx.h fixes.
__host__ __device__ inline int32_t policy_set_doubles(int32_t D, int32_t n_hidden, int32_t n_out)
{
    return n_out + (n_hidden > 0 ? n_hidden * (D + 1 + n_out) : D * n_out);
}

// The P sets out of the caller's arrays into `lds`, by all threads of the workgroup; ends in the workgroup's barrier (call it
// before any lane leaves).
__device__ __forceinline__ void stage_policy(const PolicyArgs &pa, int32_t D, double *lds)
{
    const int32_t nh = pa.n_hidden, no = pa.n_out, nr = pa.n_real;
    const int32_t rec = D + 1 + no;
    const int32_t used = policy_set_doubles(D, nh, no);
    const int32_t total = pa.n_policies * pa.stride;
    for (int32_t e = (int32_t)threadIdx.x; e < total; e += BLOCK_K) {
        const int32_t ps = e / pa.stride, r = e - ps * pa.stride;
        double v = 0.0;                                          // (a padding output; the padding double of an odd set)
        if (r < no) {
            if (r < nr) v = pa.b2[ps * nr + r];
        } else if (r < used) {
            const int32_t q = r - no;
            if (nh > 0) {
                const int32_t u = q / rec, c = q - u * rec;
                if (c < D) v = pa.w1[(ps * nh + u) * D + c];
                else if (c == D) v = pa.b1[ps * nh + u];
                else if (c - D - 1 < nr) v = pa.w2[(ps * nr + (c - D - 1)) * nh + u];
            } else {
                const int32_t j = q / no, o = q - j * no;
                if (o < nr) v = pa.w2[(ps * nr + o) * D + j];
            }
        }
        lds[e] = v;
    }
    __syncthreads();
}

// where the lane's set starts in the staged image: policy_index[i], 0 where it is absent or outside [0, P)
__device__ __forceinline__ int32_t policy_lane_offset(const PolicyArgs &pa, int64_t i)
{
    int32_t ps = pa.index ? pa.index[i] : 0;
    if (ps < 0 || ps >= pa.n_policies) ps = 0;
    return ps * pa.stride;
}

// y[0 .. no) of the rule of include/mgx.h for the input x[0 .. D): separate multiplies and adds (the build has -ffp-contract=off),
// every sum in index order.  `w`: the lane's set in LDS -- lanes of one set read the same address (a broadcast).  `no`: the width
// of the staged set (PolicyArgs.n_out), NO its static bound.  The outputs go in groups of four behind ONE wave-uniform branch
// each (the discrete call stages a multiple of four, the padding outputs with zero weights and never looked at): a test per
// output becomes a select under a mask of its own, and twelve masks across the loop over the hidden units spilled scalar registers.
template <int D, int NO>
__device__ __forceinline__ void policy_outputs(const double *w, int32_t nh, int32_t no, const double (&x)[D], double (&y)[NO])
{
    constexpr int G = NO < 4 ? NO : 4;
    static_assert(NO % G == 0, "whole groups");
#pragma unroll
    for (int o = 0; o < NO; o++) y[o] = 0.0;
#pragma unroll
    for (int c = 0; c < NO; c += G)
        if (c < no) {
#pragma unroll
            for (int o = c; o < c + G; o++) y[o] = w[o];
        }
    w += no;
    if (nh > 0) {
        const int32_t rec = D + 1 + no;
#pragma nounroll
        for (int32_t u = 0; u < nh; u++) {
            double h = w[D];
#pragma unroll
            for (int j = 0; j < D; j++) h = h + w[j] * x[j];
            h = h > 0.0 ? h : 0.0;                                // (NaN and -0.0 become +0.0)
#pragma unroll
            for (int c = 0; c < NO; c += G)
                if (c < no) {
#pragma unroll
                    for (int o = c; o < c + G; o++) y[o] = y[o] + w[D + 1 + o] * h;
                }
            w += rec;
        }
    } else {
#pragma unroll
        for (int j = 0; j < D; j++) {
#pragma unroll
            for (int c = 0; c < NO; c += G)
                if (c < no) {
#pragma unroll
                    for (int o = c; o < c + G; o++) y[o] = y[o] + w[o] * x[j];
                }
            w += no;
        }
    }
}

// the discrete head: the lowest o whose y[o] is strictly greater than everything before it, from -inf (a NaN never wins);
// `best`: that greatest value (-inf where nothing won)
template <int NO>
__device__ __forceinline__ int32_t policy_argmax(const double (&y)[NO], int32_t no, double &best)
{
    best = -__builtin_inf();
    int32_t id = 0;
#pragma unroll
    for (int o = 0; o < NO; o++)
        if (o < no) {
            const bool m = y[o] > best;
            best = m ? y[o] : best;
            id = m ? o : id;
        }
    return id;
}
template <int NO>
__device__ __forceinline__ int32_t policy_argmax(const double (&y)[NO], int32_t no)
{
    double best;
    return policy_argmax<NO>(y, no, best);
}

// the continuous head: a normalised control
__device__ __forceinline__ double policy_clip(double y) { return !(y > 0.0) ? 0.0 : (y > 1.0 ? 1.0 : y); }

// ---- exploration: the rule of mgx_exploration (include/mgx.h), for the exploring heads (mgx_policy_head_episodes.hip,
// mgx_step_policy_head_episodes.hip).  Every piece is a function of (seed, grid, step counter, number) and of values the step
// has at hand: a draw is formed where it is used and holds no register across the step. ----
// mgx_exploration as the kernels see it, by value in their argument struct
struct ExploreArgs {
    uint64_t seed;
    double epsilon, sigma[4];
    const double *scale;             // [N] or NULL
};

// scale[i], 1.0 where there is none: x * 1.0 is x bit for bit, so the loops carry one product and no branch on the pointer
__device__ __forceinline__ double explore_lane_scale(const double *__restrict__ scale, int64_t i) { return scale ? scale[i] : 1.0; }

// the draw: r[0 .. 3] of grid i at step counter t, number j
__device__ __forceinline__ void explore_draw(uint64_t seed, int64_t i, int32_t t, uint32_t j, uint32_t (&r)[4])
{
    philox4x32_10((uint32_t)i, (uint32_t)((uint64_t)i >> 32), (uint32_t)t, 0xE9100000u + j, (uint32_t)seed, (uint32_t)(seed >> 32), r);
}

// the discrete head: `greedy` (policy_argmax) or, with probability e, one of the `no` REAL ids (not the staged multiple of four)
__device__ __forceinline__ int32_t policy_epsilon_greedy(int32_t greedy, int32_t no, double e, uint64_t seed, int64_t i, int32_t t)
{
    uint32_t r[4];
    explore_draw(seed, i, t, 0u, r);
    const double u1 = uniform53(r[0], r[1]), u2 = uniform53(r[2], r[3]);
    const int32_t k = (int32_t)floor(u2 * (double)no);
    return u1 < e ? (k < no - 1 ? k : no - 1) : greedy;
}

// the continuous head's noise for action column j: the twelve 10-bit fields of the draw summed, centred, in units of 2^-10
__device__ __forceinline__ double explore_normal(uint64_t seed, int64_t i, int32_t t, uint32_t j)
{
    uint32_t r[4];
    explore_draw(seed, i, t, j, r);
    uint32_t S = 0u;
#pragma unroll
    for (int w = 0; w < 4; w++) S += (r[w] & 1023u) + ((r[w] >> 10) & 1023u) + ((r[w] >> 20) & 1023u);
    return ((double)S - 6138.0) * (1.0 / 1024.0);
}

// ... and the control it gives: the clip of y + s * z (a multiply, then an add: the build has -ffp-contract=off)
__device__ __forceinline__ double policy_noisy_clip(double y, double s, uint64_t seed, int64_t i, int32_t t, uint32_t j)
{
    const double z = explore_normal(seed, i, t, j);
    return policy_clip(y + s * z);
}

// ---- sampling: the rule of mgx_sampling (include/mgx.h), for the sampling heads of rollout_policy_head_episodes_kernel (mgx_policy_head_episodes.hip) ----
// mgx_sampling as the kernel sees it, by value in its argument struct
struct SampleArgs {
    uint64_t seed;
    double temperature;
    const double *scale;             // [N] or NULL
};

// what a lane carries across the loop: beta = 1 / tau, or -1.0 where !(tau > 0) -- the lane takes the greedy id (a beta is never negative)
__device__ __forceinline__ double sample_lane_beta(const SampleArgs &sa, int64_t i)
{
    const double tau = sa.temperature * explore_lane_scale(sa.scale, i);
    return tau > 0.0 ? 1.0 / tau : -1.0;
}

// E(d) for -708 <= d <= 0: exp as a fixed sequence of IEEE operations (the build has -ffp-contract=off), no libm
__device__ __forceinline__ double policy_exp(double d)
{
    const double k = floor(d * 1.4426950408889634 + 0.5);
    const double r = (d - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
    double p = 1.6059043836821613e-10;                                                   // the doubles nearest 1/n!, n = 13 .. 0
    p = p * r + 2.08767569878681e-09;
    p = p * r + 2.505210838544172e-08;
    p = p * r + 2.755731922398589e-07;
    p = p * r + 2.7557319223985893e-06;
    p = p * r + 2.48015873015873e-05;
    p = p * r + 0.0001984126984126984;
    p = p * r + 0.001388888888888889;
    p = p * r + 0.008333333333333333;
    p = p * r + 0.041666666666666664;
    p = p * r + 0.16666666666666666;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return p * __longlong_as_double((long long)((uint64_t)((int32_t)k + 1023) << 52));  // 2^k, k in [-1021, 0]: a normal number
}

// the sampling head: the weights e[o] written OVER y[o] (static indices, no second array), their sum, then -- only now, so that the
// draw holds no register beside the outputs -- the draw and the inverse CDF.  Returns the id taken, `prob` its probability.
// `no`: the REAL ids; the outputs go in the groups of four of policy_outputs (a padding output weighs 0.0 and is never taken).
template <int NO>
__device__ __forceinline__ int32_t policy_sample(double (&y)[NO], int32_t no, double beta, uint64_t seed, int64_t i, int32_t t, double &prob)
{
    constexpr int G = NO < 4 ? NO : 4;
    double best;
    const int32_t g = policy_argmax<NO>(y, no, best);
    const double b = beta >= 0.0 ? beta : 0.0;                                            // (a greedy lane: weights nobody reads, d in range)
    double S = 0.0;
#pragma unroll
    for (int c = 0; c < NO; c += G) {
        if (c < no) {
#pragma unroll
            for (int o = c; o < c + G; o++) {
                const double d = (y[o] - best) * b;
                const bool in = d >= -708.0;                                              // (false for a NaN)
                const double e = policy_exp(in ? d : -708.0);
                y[o] = o < no ? (o == g ? 1.0 : (in ? e : 0.0)) : 0.0;
                S = S + y[o];
            }
        } else {
#pragma unroll
            for (int o = c; o < c + G; o++) y[o] = 0.0;
        }
    }
    uint32_t r[4];
    explore_draw(seed, i, t, 1u, r);
    const double v = uniform53(r[0], r[1]) * S;
    double c = 0.0, e_id = 1.0;
    int32_t id = g;
    bool open = beta >= 0.0;                                                              // (a greedy lane takes nothing)
#pragma unroll
    for (int o = 0; o < NO; o++) {
        c = c + y[o];
        const bool take = open && v < c;
        id = take ? o : id;
        e_id = take ? y[o] : e_id;
        open = open && !take;
    }
    prob = beta >= 0.0 ? e_id / S : 1.0;
    return id;
}

// ---- the critic: the rule of mgx_critic (include/mgx.h), for the heads with a critic (HEAD_SAMPLE_CRITIC, HEAD_GAUSSIAN_CRITIC).
// New functions beside the ones above, which the greedy, exploring and sampling kernels keep to themselves. ----
// mgx_critic as the kernel sees it, by value in its argument struct
struct CriticArgs {
    const double *w, *b;             // [P, n_mid], [P]
};

// One parameter set WITH a critic as it lies in LDS (doubles), for a row of D values -- the set of policy_set_doubles with the
// critic's bias beside b2 and its weight in the record of the unit (or input) it multiplies, at a static offset:
//   n_hidden > 0:  b2[0 .. n_out), b | per hidden unit u: W1[u, 0 .. D), b1[u], w[u], W2[0 .. n_out, u]
//   n_hidden = 0:  b2[0 .. n_out), b | per input j: w[j], W2[0 .. n_out, j]
// -- 1 + n_mid doubles more than the set without one.
__host__ __device__ inline int32_t policy_critic_set_doubles(int32_t D, int32_t n_hidden, int32_t n_out)
{
    return policy_set_doubles(D, n_hidden, n_out) + 1 + (n_hidden > 0 ? n_hidden : D);
}

// stage_policy for that image (`pa.stride` is the stride of the sets with a critic); ends in the workgroup's barrier
__device__ __forceinline__ void stage_policy_critic(const PolicyArgs &pa, const CriticArgs &cr, int32_t D, double *lds)
{
    const int32_t nh = pa.n_hidden, no = pa.n_out, nr = pa.n_real;
    const int32_t rec = nh > 0 ? D + 2 + no : 1 + no;
    const int32_t used = policy_critic_set_doubles(D, nh, no);
    const int32_t total = pa.n_policies * pa.stride;
    for (int32_t e = (int32_t)threadIdx.x; e < total; e += BLOCK_K) {
        const int32_t ps = e / pa.stride, r = e - ps * pa.stride;
        double v = 0.0;                                          // (a padding output; the padding double of an odd set)
        if (r < no) {
            if (r < nr) v = pa.b2[ps * nr + r];
        } else if (r == no) {
            v = cr.b[ps];
        } else if (r < used) {
            const int32_t q = r - no - 1;
            const int32_t u = q / rec, c = q - u * rec;          // (the unit, or the input of a linear policy)
            if (nh > 0) {
                if (c < D) v = pa.w1[(ps * nh + u) * D + c];
                else if (c == D) v = pa.b1[ps * nh + u];
                else if (c == D + 1) v = cr.w[ps * nh + u];
                else if (c - D - 2 < nr) v = pa.w2[(ps * nr + (c - D - 2)) * nh + u];
            } else {
                if (c == 0) v = cr.w[ps * D + u];
                else if (c - 1 < nr) v = pa.w2[(ps * nr + (c - 1)) * D + u];
            }
        }
        lds[e] = v;
    }
    __syncthreads();
}

// policy_outputs on a set with a critic: y[0 .. no) as there, operation by operation, and V of mgx_critic as one more running sum
// beside them -- a hidden unit is folded into it while h is live, an input of a linear policy while its weights are walked.
template <int D, int NO>
__device__ __forceinline__ void policy_outputs_value(const double *w, int32_t nh, int32_t no, const double (&x)[D], double (&y)[NO], double &V)
{
    constexpr int G = NO < 4 ? NO : 4;
    static_assert(NO % G == 0, "whole groups");
#pragma unroll
    for (int o = 0; o < NO; o++) y[o] = 0.0;
#pragma unroll
    for (int c = 0; c < NO; c += G)
        if (c < no) {
#pragma unroll
            for (int o = c; o < c + G; o++) y[o] = w[o];
        }
    double val = w[no];
    w += no + 1;
    if (nh > 0) {
        const int32_t rec = D + 2 + no;
#pragma nounroll
        for (int32_t u = 0; u < nh; u++) {
            double h = w[D];
#pragma unroll
            for (int j = 0; j < D; j++) h = h + w[j] * x[j];
            h = h > 0.0 ? h : 0.0;                                // (NaN and -0.0 become +0.0)
            val = val + w[D + 1] * h;
#pragma unroll
            for (int c = 0; c < NO; c += G)
                if (c < no) {
#pragma unroll
                    for (int o = c; o < c + G; o++) y[o] = y[o] + w[D + 2 + o] * h;
                }
            w += rec;
        }
    } else {
#pragma unroll
        for (int j = 0; j < D; j++) {
            val = val + w[0] * x[j];
#pragma unroll
            for (int c = 0; c < NO; c += G)
                if (c < no) {
#pragma unroll
                    for (int o = c; o < c + G; o++) y[o] = y[o] + w[1 + o] * x[j];
                }
            w += no + 1;
        }
    }
    V = val;
}

// ... and V alone, on the same set with the same operations: the final row of an episode, the row the last step returned
template <int D>
__device__ __forceinline__ double policy_value(const double *w, int32_t nh, int32_t no, const double (&x)[D])
{
    double val = w[no];
    w += no + 1;
    if (nh > 0) {
        const int32_t rec = D + 2 + no;
#pragma nounroll
        for (int32_t u = 0; u < nh; u++) {
            double h = w[D];
#pragma unroll
            for (int j = 0; j < D; j++) h = h + w[j] * x[j];
            h = h > 0.0 ? h : 0.0;
            val = val + w[D + 1] * h;
            w += rec;
        }
    } else {
#pragma unroll
        for (int j = 0; j < D; j++) {
            val = val + w[0] * x[j];
            w += no + 1;
        }
    }
    return val;
}

// ---- the Gaussian head: the rule of mgx_gaussian (include/mgx.h), for the Gaussian heads of step_k_policy_head_episodes_kernel
// (mgx_step_policy_head_episodes.hip).  New functions beside the ones above; log, sine and cosine are fixed sequences of IEEE
// operations (the build has -ffp-contract=off), and so is the square root (policy_sqrt); the division is the correctly rounded one. ----
// mgx_gaussian as the kernel sees it, by value in its argument struct
struct GaussianArgs {
    uint64_t seed;
    double sigma[4];
    const double *scale;             // [N] or NULL
};

// L(a) for a positive normal a: exponent and mantissa out of the bits, m folded into (sqrt(1/2), sqrt(2)], 2 atanh(t) by Horner
__device__ __forceinline__ double policy_log(double a)
{
    const uint64_t bits = (uint64_t)__double_as_longlong(a);
    int32_t e = (int32_t)((bits >> 52) & 0x7ffu) - 1023;
    double m = __longlong_as_double((long long)((bits & 0x000fffffffffffffull) | 0x3ff0000000000000ull));
    const bool big = m > 1.4142135623730951;
    m = big ? m * 0.5 : m;
    e = big ? e + 1 : e;
    const double t = (m - 1.0) / (m + 1.0);
    const double w = t * t;
    double p = 0.09523809523809523;                                                      // the doubles nearest 2 / (2n + 1), n = 10 .. 0
    p = p * w + 0.10526315789473684;
    p = p * w + 0.11764705882352941;
    p = p * w + 0.13333333333333333;
    p = p * w + 0.15384615384615385;
    p = p * w + 0.18181818181818182;
    p = p * w + 0.2222222222222222;
    p = p * w + 0.2857142857142857;
    p = p * w + 0.4;
    p = p * w + 0.6666666666666666;
    p = p * w + 2.0;
    const double ed = (double)e;
    return ed * 6.93147180369123816490e-01 + (ed * 1.90821492927058770002e-10 + t * p);
}

// (sin, cos) of f quarter turns, f a multiple of 2^-52 in [0, 1): folded at the eighth of a turn, two Horner sums in x^2
__device__ __forceinline__ void policy_quarter_turn(double f, double &sn, double &cs)
{
    const bool hi = f > 0.5;
    const double g = hi ? 1.0 - f : f;
    const double x = g * 1.5707963267948966;
    const double w = x * x;
    double q = -7.647163731819816e-13;                                                   // the doubles nearest -+1/k!, k = 15, 13 .. 3
    q = q * w + 1.6059043836821613e-10;
    q = q * w + -2.505210838544172e-08;
    q = q * w + 2.7557319223985893e-06;
    q = q * w + -0.0001984126984126984;
    q = q * w + 0.008333333333333333;
    q = q * w + -0.16666666666666666;
    const double s = x * (q * w + 1.0);
    double c = 4.779477332387385e-14;                                                    // ... k = 16, 14 .. 2, then the constant 1.0
    c = c * w + -1.1470745597729725e-11;
    c = c * w + 2.08767569878681e-09;
    c = c * w + -2.755731922398589e-07;
    c = c * w + 2.48015873015873e-05;
    c = c * w + -0.001388888888888889;
    c = c * w + 0.041666666666666664;
    c = c * w + -0.5;
    c = c * w + 1.0;
    sn = hi ? c : s;
    cs = hi ? s : c;
}

// S(v): the square root as a fixed sequence -- 1 / sqrt(v) from its bits, four Newton steps of multiplies and adds, one correction
__device__ __forceinline__ double policy_sqrt(double v)
{
    const bool pos = v > 0.0;
    const double a = pos ? v : 1.0;
    double y = __longlong_as_double((long long)(0x5FE6EB50C7B537A9ull - ((uint64_t)__double_as_longlong(a) >> 1)));
    const double h = 0.5 * a;
    y = y * (1.5 - (h * y) * y);
    y = y * (1.5 - (h * y) * y);
    y = y * (1.5 - (h * y) * y);
    y = y * (1.5 - (h * y) * y);
    const double r = a * y;
    const double S = r + (0.5 * y) * (a - r * r);
    return pos ? S : 0.0;
}

// four words of a draw -> a normal pair: z0 = R cos, z1 = R sin (Box-Muller).  Shared by the Gaussian head's draw below and the CEM
// candidates' (mgx_cem.hpp), which differ in the counter words alone.
__device__ __forceinline__ void gaussian_pair_of_words(const uint32_t (&r)[4], double &z0, double &z1)
{
    const double u1 = 1.0 - uniform53(r[0], r[1]);                                        // (exact; in (0, 1])
    const double R = policy_sqrt(-2.0 * policy_log(u1));
    const uint64_t a64 = (uint64_t)r[2] << 32 | r[3];
    const uint32_t q = (uint32_t)(a64 >> 62);
    const double f = (double)((a64 >> 10) & 0x000fffffffffffffull) * (1.0 / 4503599627370496.0);
    double s, c;
    policy_quarter_turn(f, s, c);
    const double sn = q == 0u ? s : (q == 1u ? c : (q == 2u ? -s : -c));
    const double cs = q == 0u ? c : (q == 1u ? -s : (q == 2u ? -c : s));
    z0 = R * cs;
    z1 = R * sn;
}

// normal pair p of grid i at step counter t: z0 = z[2p], z1 = z[2p + 1], out of draw number 8 + p
__device__ __forceinline__ void gaussian_pair(uint64_t seed, int64_t i, int32_t t, uint32_t p, double &z0, double &z1)
{
    uint32_t r[4];
    explore_draw(seed, i, t, 8u + p, r);
    gaussian_pair_of_words(r, z0, z1);
}

// C_i of the lane, formed once in the prologue: the sum over the live columns (s > 0) of L(s) + log(2 pi) / 2, in column order
template <int A, class SIGMA>
__device__ __forceinline__ double gaussian_lane_const(SIGMA sigma, double sc)
{
    double C = 0.0;
#pragma unroll
    for (int o = 0; o < A; o++) {
        const double s = sigma(o) * sc;
        const bool live = s > 0.0;
        const double term = policy_log(live ? s : 1.0) + 0.9189385332046727;
        C = live ? C + term : C;
    }
    return C;
}

// the Gaussian head on y[0 .. A): raw[o] = y[o] + s[o] * z[o] on the live columns (y[o] on the others), a pair's draw only where
// one of its columns is live; every raw[o] goes to `sink(o, raw)` as soon as its pair is known (o a constant once the loop is
// unrolled), so that nothing of a pair outlives it.  Returns logp = (-0.5 * Q) - C, Q the sum of z[o]^2 over the live columns in
// order.  `sigma(o)`: where the kernel reads sigma[o] (the kernarg segment), `sc`: the lane's scale, `C`: its gaussian_lane_const.
template <int A, int NO, class SIGMA, class SINK>
__device__ __forceinline__ double policy_gaussian_head(const double (&y)[NO], SIGMA sigma, double sc, double C, uint64_t seed, int64_t i,
                                                       int32_t t, SINK sink)
{
    double Q = 0.0;
#pragma unroll
    for (int p = 0; 2 * p < A; p++) {
        const bool two = 2 * p + 1 < A;                                                   // (false: the pair's second column does not exist)
        const int o0 = 2 * p, o1 = two ? 2 * p + 1 : 2 * p;
        const double s0 = sigma(o0) * sc;
        const double s1 = two ? sigma(o1) * sc : 0.0;
        const bool l0 = s0 > 0.0, l1 = s1 > 0.0;
        double r0 = y[o0], r1 = y[o1];
        if (l0 || l1) {
            double z0, z1;
            gaussian_pair(seed, i, t, (uint32_t)p, z0, z1);
            r0 = l0 ? r0 + s0 * z0 : r0;
            Q = l0 ? Q + z0 * z0 : Q;
            r1 = l1 ? r1 + s1 * z1 : r1;
            Q = l1 ? Q + z1 * z1 : Q;
        }
        sink(o0, r0);
        if (two) sink(o1, r1);
    }
    return (-0.5 * Q) - C;
}

// columns of an H = 0 row of layout F
template <int F>
constexpr int policy_row_dim() { return 2 + 4 * ((F & F_GENSET) != 0) + 2 * ((F & F_BATTERY) != 0) + 4 * ((F & F_GRID) != 0); }

// The row the lane's grid stands on -- series row t_row, state `s`, series values out of `in` -- into the lane's strip of the
// wave's tile, in the handle's observation format (episode_row_h0: observe_row_h0's values bit for bit, the padding rows too),
// and out of the strip again as the policy's input: float32 rows are widened back, so the policy sees what the caller is given.
template <int F>
__device__ __forceinline__ void policy_row(const KArgs *__restrict__ a_dev, int32_t T, uint32_t desc, int64_t i, int32_t t_row,
                                           const Inputs &in, const RowBounds<F> &b, const Params &p, const State &s, double *tile,
                                           double (&x)[policy_row_dim<F>()])
{
    constexpr int D = policy_row_dim<F>();
    const int lane = threadIdx.x & 63;
    if (row_desc_f32(desc)) {
        float *q = reinterpret_cast<float *>(tile) + lane * D;
        episode_row_h0<F>(a_dev, T, desc, i, t_row, in, b, p, s, q);
#pragma unroll
        for (int j = 0; j < D; j++) x[j] = (double)q[j];
    } else {
        double *q = tile + lane * D;
        episode_row_h0<F>(a_dev, T, desc, i, t_row, in, b, p, s, q);
#pragma unroll
        for (int j = 0; j < D; j++) x[j] = q[j];
    }
}

// ... and the strips as row `r64` (element offset) of `obs`: a full wave's 64 rows as 16-byte non-temporal stores out of the tile
// (stream_row_tile), the last wave of a batch that is no multiple of 64 lane by lane -- the bytes store_episode_row writes.
template <int D>
__device__ __forceinline__ void emit_policy_row(uint32_t desc, void *__restrict__ obs, int64_t r64, const double *tile)
{
    const int lane = threadIdx.x & 63;
    if (MGX_EPISODE_ROWS_TILE && __builtin_amdgcn_read_exec() == ~0ull) {
        __builtin_amdgcn_wave_barrier();
        if (row_desc_f32(desc)) stream_row_tile(reinterpret_cast<const float *>(tile), (float *)obs + (r64 - (int64_t)lane * D), D);
        else stream_row_tile(tile, (double *)obs + (r64 - (int64_t)lane * D), D);
        __builtin_amdgcn_wave_barrier();                 // (the next row goes into the same tile)
    } else if (row_desc_f32(desc)) {
        const float *q = reinterpret_cast<const float *>(tile) + lane * D;
#pragma unroll
        for (int j = 0; j < D; j++) ((float *)obs)[r64 + j] = q[j];
    } else {
        const double *q = tile + lane * D;
#pragma unroll
        for (int j = 0; j < D; j++) ((double *)obs)[r64 + j] = q[j];
    }
}

// The arguments of the two kernels, ONE struct by value each (late_kernargs)
struct RolloutPolicyArgs {
    KArgs a;
    PLWords tab;
    PolicyArgs pol;
    int32_t t0, K;
    FusedOut out;
    mgx_episode_stats es;
    int32_t gpb;
    uint32_t desc;                   // pack_row_desc(a)
    const KArgs *a_dev;
    void *obs, *final_obs;
    uint8_t *ids_out;                // [K, N] or NULL
};
struct StepPolicyArgs {
    KArgs a;
    PolicyArgs pol;
    int32_t t0, K;
    int32_t gpb;
    uint32_t desc;                   // pack_row_desc(a)
    FusedOut out;
    mgx_episode_stats es;
    const KArgs *a_dev;
    void *obs, *final_obs;
    double *actions_out;             // [K, N, A] or NULL
};

// ... and of the two exploring kernels: the greedy kernel's struct first (its fields keep their offsets), the exploration behind it
struct RolloutPolicyExploreArgs {
    RolloutPolicyArgs g;
    ExploreArgs ex;
};
struct StepPolicyExploreArgs {
    StepPolicyArgs g;
    ExploreArgs ex;
};

// ... and of the sampling kernel: the same way, the sampling and the stream of probabilities behind the greedy kernel's struct
struct RolloutPolicySampleArgs {
    RolloutPolicyArgs g;
    SampleArgs sa;
    double *prob_out;                // [K, N] or NULL
};

// ... and of the critic kernel: the sampling kernel's struct first, the critic and its three outputs behind it
struct RolloutPolicyCriticArgs {
    RolloutPolicySampleArgs s;
    CriticArgs cr;
    double *value_out, *final_value_out;   // [K, N] or NULL
    double *last_value_out;                // [N] or NULL
};

// ... and of the Gaussian kernel: the greedy continuous kernel's struct first, the head, its two streams, the critic and its three
// outputs behind it (the critic's fields are read by the CRITIC forms alone)
struct StepPolicyGaussianArgs {
    StepPolicyArgs g;
    GaussianArgs gs;
    double *raw_out;                 // [K, N, A] or NULL
    double *logp_out;                // [K, N] or NULL
    CriticArgs cr;
    double *value_out, *final_value_out;   // [K, N] or NULL
    double *last_value_out;                // [N] or NULL
};

// The head of a closed-loop launch: what the two head kernels (mgx_policy_head_episodes.hip: exploring, sampling, sampling with a
// critic; mgx_step_policy_head_episodes.hip: exploring, Gaussian, Gaussian with a critic) take as their last template argument and
// their objects as -DMGX_POLICY_HEAD.  The greedy kernels (mgx_policy_episodes.hip, mgx_step_policy_episodes.hip) take none.
enum PolicyHead : int { HEAD_GREEDY = 0, HEAD_EXPLORE = 1, HEAD_SAMPLE = 2, HEAD_SAMPLE_CRITIC = 3, HEAD_GAUSSIAN = 4, HEAD_GAUSSIAN_CRITIC = 5 };
constexpr bool head_has_critic(int head) { return head == HEAD_SAMPLE_CRITIC || head == HEAD_GAUSSIAN_CRITIC; }

// ... and the struct each head's kernel takes: every head keeps the layout of its kernarg segment
template <int HEAD>
using RolloutPolicyHeadArgs = std::conditional_t<HEAD == HEAD_EXPLORE, RolloutPolicyExploreArgs,
                              std::conditional_t<HEAD == HEAD_SAMPLE, RolloutPolicySampleArgs, RolloutPolicyCriticArgs>>;
template <int HEAD>
using StepPolicyHeadArgs = std::conditional_t<HEAD == HEAD_EXPLORE, StepPolicyExploreArgs, StepPolicyGaussianArgs>;

// The path from a head's struct to a part the heads share, stated once per struct: `greedy_part` the greedy kernel's struct at its
// front, `sampling_part` the sampling kernel's (of the heads that sample).  Each for the parameter and for late_kernargs' view of
// the kernarg segment (its address space), so the kernels' text spells no path of one head.
#define MGX_KERNARG __attribute__((address_space(4)))
#define MGX_ARGS_PART(FN, ARGS, PART, PATH)                                                                      \
    __host__ __device__ __forceinline__ const PART &FN(const ARGS &x) { return PATH; }                          \
    __device__ __forceinline__ const MGX_KERNARG PART &FN(const MGX_KERNARG ARGS &x) { return PATH; }
MGX_ARGS_PART(greedy_part, RolloutPolicyExploreArgs, RolloutPolicyArgs, x.g)
MGX_ARGS_PART(greedy_part, RolloutPolicySampleArgs, RolloutPolicyArgs, x.g)
MGX_ARGS_PART(greedy_part, RolloutPolicyCriticArgs, RolloutPolicyArgs, x.s.g)
MGX_ARGS_PART(greedy_part, StepPolicyExploreArgs, StepPolicyArgs, x.g)
MGX_ARGS_PART(greedy_part, StepPolicyGaussianArgs, StepPolicyArgs, x.g)
MGX_ARGS_PART(sampling_part, RolloutPolicySampleArgs, RolloutPolicySampleArgs, x)
MGX_ARGS_PART(sampling_part, RolloutPolicyCriticArgs, RolloutPolicySampleArgs, x.s)
#undef MGX_ARGS_PART

// ---- host side: what mgx_abi.hip hands the slices of the translation units ----
struct EpisodePolicyLaunch {
    EpisodeRowsLaunch r;             // as for the kernels with rows (obs / final_obs may both be NULL here)
    PolicyArgs pol;
    unsigned lds_bytes;              // n_policies * stride doubles: the dynamic LDS of the launch
    void *actions_out;               // the ids (uint8 [K, N]) or controls (double [K, N, A]) the policy chose, or NULL
    ExploreArgs ex;                  // the exploring kernels alone read it
    SampleArgs sa;                   // ... the sampling kernel and the critic kernel these two,
    double *prob_out;
    CriticArgs cr;                   // ... the critic kernel alone the rest (lds_bytes / pol.stride then hold policy_critic_set_doubles)
    double *value_out, *final_value_out, *last_value_out;
    GaussianArgs gs;                 // ... the Gaussian kernel these, `cr` and the three outputs above with its critic
    double *raw_out, *logp_out;
    int head;                        // PolicyHead: which kernel of the family
};
bool launch_rollout_policy_episodes_p0(const EpisodePolicyLaunch &L); bool launch_rollout_policy_episodes_p1(const EpisodePolicyLaunch &L);
bool launch_step_k_policy_episodes_p0(const EpisodePolicyLaunch &L); bool launch_step_k_policy_episodes_p1(const EpisodePolicyLaunch &L);
// ... and of the two head files, whose objects hold one head of one slice each (-DMGX_POLICY_HEAD=h -DMGX_EPISODE_PART=p) and define
// their instance of these; the launch of slice PART of a family picks the instance of the launch's head
template <int HEAD, int PART> bool launch_rollout_policy_head_episodes(const EpisodePolicyLaunch &L);
template <int HEAD, int PART> bool launch_step_k_policy_head_episodes(const EpisodePolicyLaunch &L);
template <int PART>
inline bool launch_rollout_policy_head_episodes_p(const EpisodePolicyLaunch &L)
{
    switch (L.head) {
        case HEAD_EXPLORE: return launch_rollout_policy_head_episodes<HEAD_EXPLORE, PART>(L);
        case HEAD_SAMPLE: return launch_rollout_policy_head_episodes<HEAD_SAMPLE, PART>(L);
        case HEAD_SAMPLE_CRITIC: return launch_rollout_policy_head_episodes<HEAD_SAMPLE_CRITIC, PART>(L);
        default: return false;
    }
}
template <int PART>
inline bool launch_step_k_policy_head_episodes_p(const EpisodePolicyLaunch &L)
{
    switch (L.head) {
        case HEAD_EXPLORE: return launch_step_k_policy_head_episodes<HEAD_EXPLORE, PART>(L);
        case HEAD_GAUSSIAN: return launch_step_k_policy_head_episodes<HEAD_GAUSSIAN, PART>(L);
        case HEAD_GAUSSIAN_CRITIC: return launch_step_k_policy_head_episodes<HEAD_GAUSSIAN_CRITIC, PART>(L);
        default: return false;
    }
}

}  // namespace mgx
