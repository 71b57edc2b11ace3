// mgx_step_hot.hip -- step_k_hot_kernel: the hot form of the lock-step K-step launch in a kernel of its own.
//
// What it serves (the host's predicate: step_k_hot_takes, mgx_abi.hip): factorised series, a lock-step handle, no reward
// shaper, layouts without a GridModule, outputs exactly reward (+ SoC where the layout has a battery), K <= STEP_HOT_MAX_K (the
// base rows of the whole launch fit one LDS image).  Everything else stays with step_k_kernel (mgx_kernels.hpp), and so does
// the arithmetic: the same helpers in the same order, so a launch computes the bits step_k_kernel computes.
//
// What differs is the control flow around the ring of controls.  step_k_kernel picks its loop form inside the chunk loop, so
// the compiler keeps ONE loop nest for the four forms: the ring slots are live across the form switch, copied in and out of
// every group of steps, and the memory queue is drained at the group's edges.  Here
//   - the form (every genset of the wave instantaneous, or not) is chosen once, at kernel scope, and owns a plain loop;
//   - that loop runs whole groups of U steps, unrolled, with no guard per step, as long as every refill of the group reads a
//     row below K: a slot is then always a loaded value (never "loaded or kept").  The one or two whole groups after it guard
//     their refills with a scalar test (clamping the row instead -- re-reading row K - 1 for a quarter of a K = 64 launch at
//     depth 16 -- cost 1.7 % of the launch: profiles/exp_step_k_hot.txt).  No address outside rows [0, K) of the caller's
//     controls is formed;
//   - step k issues its refill before its arithmetic, into the slot step k - 1 consumed (not into its own: the old and the new
//     value of one slot would be live together, and the compiler then copies the whole ring on the loop's back edge, behind a
//     wait for nearly everything in flight).  So U - 1 steps of controls are in flight behind the slot being consumed, every
//     slot lives in the same registers for the whole launch, and every step waits with a counted vmcnt;
//   - the first group is peeled off the loop: the memory queue fills during it (loads only, then loads and stores), and a loop
//     entered from the prologue would inherit the prologue's lower counts in the waits of every later group;
//   - the K % U steps that remain consume their slots in a second unrolled body without refills.
#include "mgx_step_hot.hpp"

namespace mgx {

// Ring depth.  16 is the deepest at which the F = 3 double form stays inside 256 VGPRs without AGPRs or scratch memory at two waves
// per SIMD (218 VGPRs), but it measured slower than 8 (154 VGPRs, three waves per SIMD): 45.7 against 45.2-45.4 us per launch of the
// headline, the parent's step_k_kernel at 46.5 in the same job (profiles/exp_step_k_hot.txt).
#ifndef MGX_RING_HOT
#define MGX_RING_HOT 8
#endif

template <int F, int U, typename AT>
__global__ __launch_bounds__(BLOCK_K) void step_k_hot_kernel(const KArgs a, const AT *__restrict__ actions, int32_t t0, int32_t K,
                                                             int normalized, double *__restrict__ reward, double *__restrict__ soc_trace,
                                                             double *__restrict__ ret_acc, int32_t gpb)
{
    static_assert((F & (F_GRID | F_GRID_FIRST)) == 0 && F != 0, "layouts 1, 2, 3");
    static_assert(U >= 2 && (U - 1) * 4 < 64, "the operations of U - 1 steps behind a slot must fit the 6-bit vmcnt");
    const int32_t K_launch = K;          // what the host asked for (the counter always moves by this much)
    t0 = resolve_t(a, t0);
    K = resolve_k(a, t0, K);
    const int64_t i = (int64_t)a.g0 + (int64_t)blockIdx.x * gpb + threadIdx.x;
    const bool active = (int32_t)threadIdx.x < gpb && i < a.g1;
    const int64_t N = a.N;
    constexpr int A_DIM = 2 * ((F & F_GENSET) != 0) + ((F & F_BATTERY) != 0);
    const uint32_t i32 = (uint32_t)i;    // lane offset of every [K, N] stream: row base in SGPRs + this
    const bool norm = normalized != 0;
    const int32_t k_last = K - 1;

    __shared__ double base_lds[2 * FACT_ROWS * PP];
    Params p; State s; Derived d;
    GridFactors f;
    f.lr = 0.0; f.pr = 0.0; f.lp = 0u; f.pp = 0u; f.cp = 0u; f.pat = 0u;
    bool gen_instant = false;
    RawActions<AT> ring[U];
    if (active) {
        load_state<F>(a.c, i, false, s);
        load_params<F>(a.c, i, p);
        derive<F>(p, d);
        gen_instant = genset_wave_is_instant<F>(p, s);
        load_factors<F>(a.c, i, f);
#pragma unroll
        for (int u = 0; u < U - 1; u++) {
            const int32_t r = u < k_last ? u : k_last;
            load_actions_at<F>(actions + (int64_t)r * N * A_DIM, i32, ring[u]);
        }
    }
    __syncthreads();
    stage_base_rows<F>(a.c, (int64_t)t0, K, base_lds, BLOCK_K);
    __syncthreads();
    if (!active) return;                 // (no barrier follows: advance_counter_in_kernel's is skipped by returned waves, as in step_k_kernel)

    double ret = 0.0;
    // one step: the slot's controls, this step's series values (the base row was read one step ahead), the next base row, the step
    auto step = [&](auto gi_tag, const RawActions<AT> &ra, BaseVals &nb, int32_t k) __attribute__((always_inline)) {
        constexpr bool GI = decltype(gi_tag)::value;
        Inputs in;
        if constexpr (F & F_GENSET) { in.a_goal = (double)ra.a_goal; in.a_gen = (double)ra.a_gen; }
        if constexpr (F & F_BATTERY) in.a_bat = (double)ra.a_bat;
        in.load = fact_load(nb.load, f.lr);
        in.pv = fact_pv(nb.pv, f.pr);
        nb = read_base_row<F>(base_lds, k < k_last ? k + 1 : k_last, f);
        Outputs o;
        step_core<F>(p, d, s, in, norm, (F & F_BATTERY) != 0, GI, o);
        const double r = o.reward;
#if MGX_HOT_NT
        __builtin_nontemporal_store(r, (reward + (int64_t)k * N) + i32);
        if constexpr (F & F_BATTERY) __builtin_nontemporal_store(s.soc, (soc_trace + (int64_t)k * N) + i32);
#else
        (reward + (int64_t)k * N)[i32] = r;
        if constexpr (F & F_BATTERY) (soc_trace + (int64_t)k * N)[i32] = s.soc;
#endif
        ret += r;
    };
    auto run = [&](auto gi_tag) __attribute__((always_inline)) {
        BaseVals nb = read_base_row<F>(base_lds, 0, f);
        const int32_t k_main = K - K % U;
        auto group = [&](int32_t k0, auto guard_tag) __attribute__((always_inline)) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int32_t k = k0 + u;
                if constexpr (decltype(guard_tag)::value) {
                    if (k + U - 1 <= k_last) load_actions_at<F>(actions + (int64_t)(k + U - 1) * N * A_DIM, i32, ring[(u + U - 1) % U]);
                } else {
                    load_actions_at<F>(actions + (int64_t)(k + U - 1) * N * A_DIM, i32, ring[(u + U - 1) % U]);
                }
                step(gi_tag, ring[u], nb, k);
            }
        };
        int32_t k0 = 0;
        if (2 * U - 2 <= k_last) {
            group(0, std::false_type{});
            for (k0 = U; k0 + 2 * U - 2 <= k_last; k0 += U) group(k0, std::false_type{});
        }
        for (; k0 < k_main; k0 += U) group(k0, std::true_type{});      // (at most two groups)
#pragma unroll
        for (int u = 0; u < U - 1; u++)
            if (k0 + u < K) step(gi_tag, ring[u], nb, k0 + u);
    };
    if constexpr ((F & F_GENSET) != 0) {
        if (gen_instant) run(std::true_type{}); else run(std::false_type{});
    } else {
        run(std::false_type{});
    }
    store_state<F>(a.c, i, s);
    if (ret_acc) ret_acc[i] += ret;
    advance_counter_in_kernel(a, K_launch);
}

template <int F>
static void step_k_hot_dispatch(const FusedLaunch &L)
{
    if (L.act_f32)
        step_k_hot_kernel<F, MGX_RING_HOT, float><<<L.blocks, BLOCK_K, 0, L.stream>>>(*L.k, (const float *)L.actions, L.t, L.K, L.normalized,
                                                                                      L.out.reward, L.out.soc_trace, L.out.ret_acc, L.gpb);
    else
        step_k_hot_kernel<F, MGX_RING_HOT, double><<<L.blocks, BLOCK_K, 0, L.stream>>>(*L.k, (const double *)L.actions, L.t, L.K, L.normalized,
                                                                                       L.out.reward, L.out.soc_trace, L.out.ret_acc, L.gpb);
}

bool launch_step_k_hot(const FusedLaunch &L)
{
    switch (L.flags) {
        case 1: step_k_hot_dispatch<1>(L); return true;
        case 2: step_k_hot_dispatch<2>(L); return true;
        case 3: step_k_hot_dispatch<3>(L); return true;
        default: return false;
    }
}

}  // namespace mgx
