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
//
// The controls (24 of the 40 streamed bytes per env-step of the headline) come in wave-contiguous (profiles/exp_step_k_hot_tile.txt).
// A lane's own controls lie at a lane stride of A values, so loading them takes two instructions that each touch every 128-byte
// line of the wave's piece of the row, and the second only works because the first left the line in the caches: such loads cannot
// be streamed (non-temporal they lost 7 %).  Here a wave reads its piece of a row -- A * n consecutive elements for its n grids --
// as consecutive bytes over consecutive lanes (ActCut: one 16-byte and one 8-byte load per lane for three double controls), so
// every line is asked for once, and non-temporal.  A ring slot then holds "the piece as loaded", not "my grid's controls": while
// step k computes, the wave writes the slot of row k + 1 into a tile of its own in LDS as loaded and every lane reads its grid's A
// values back, for step k + 1 -- the LDS latency never meets a dependent instruction (the base rows use the same pattern), and
// LDS operations of one wave complete in order, so the loops hold no barrier.  The values that reach step_core, and their
// order, are load_actions_at's.  Partial waves (the 16-lane fourth wave of a 208-grid workgroup, a ragged last workgroup) cut
// their shorter piece the same way, at stride n instead of 64: the inactive lanes leave as before, and no address outside the
// piece is formed.  With it row k + U (not k + U - 1) is refilled at step k: U - 1 rows stay in flight behind the slot that is
// being handed over.
#include "mgx_step_hot.hpp"

namespace mgx {

// Ring depth.  16 is the deepest at which the F = 3 double form stays inside 256 VGPRs without AGPRs or scratch memory at two waves
// per SIMD (218 VGPRs), but it measured slower than 8 (154 VGPRs, three waves per SIMD): 45.7 against 45.2-45.4 us per launch of the
// headline, the parent's step_k_kernel at 46.5 in the same job (profiles/exp_step_k_hot.txt).
#ifndef MGX_RING_HOT
#define MGX_RING_HOT 8
#endif
// The parts of profiles/exp_step_k_hot_tile.txt, each with a switch of its own so that the forms can be built side by side:
// ACT_TILE  wave-contiguous control loads handed to the lanes through a wave-private LDS tile (0: load_actions_at, a lane's own
//           controls at a lane stride of A values);
// ACT_PAIR  with ACT_TILE: the piece is cut into loads of two elements per lane, then one (0: one element per lane throughout);
// ACT_NT    with ACT_TILE: those loads non-temporal (MGX_ACT_NT, which step_k_kernel shares, stays what it is).
// (Loading the base rows into registers with the columns, behind one barrier instead of two, lost 1 % alone and was inside the
// noise on top of these: not kept, the record is in that file.)
#ifndef MGX_HOT_ACT_TILE
#define MGX_HOT_ACT_TILE 1
#endif
#ifndef MGX_HOT_ACT_NT
#define MGX_HOT_ACT_NT 1
#endif
#ifndef MGX_HOT_ACT_PAIR
#define MGX_HOT_ACT_PAIR 1
#endif

// A ring slot of the tiled form: the controls of one row as the wave loaded them -- the values of this lane's loads, in the order
// ActCut cuts the wave's piece of the row (n grids, A * n consecutive elements) into loads.
template <typename AT, int A>
struct ActSlot {
    AT v[A];
};

// How a wave's piece of a row (n grids, A * n consecutive elements) is cut into loads.  ACT_PAIR: A / 2 loads of two elements per lane
// (lane l takes elements 2 l and 2 l + 1 of a stretch of 2 n) and, for odd A, one load of a single element per lane over the last n;
// else A loads of one element per lane.  Either way every element of the piece is read once and nothing outside it, whatever n is,
// and with n = 64 a load is one run of consecutive bytes: no line is asked for by two instructions.
template <int A>
struct ActCut {
    static constexpr int PAIRS = MGX_HOT_ACT_PAIR ? A / 2 : 0;
    static constexpr int SINGLES = A - 2 * PAIRS;
    static constexpr int LOADS = PAIRS + SINGLES;
};

// Where load c of a slot lies inside the WORKGROUP's piece of a row, in bytes (wave w's piece starts at element w * 64 * A).  The
// tiles lie in LDS as the pieces lie in a row, so one offset serves both sides, and as a 32-bit byte offset beside a wave-uniform
// base it costs no 64-bit address arithmetic.
template <typename AT, int A>
struct ActOffsets {
    uint32_t b[ActCut<A>::LOADS];
};

template <typename AT, int A>
__device__ __forceinline__ ActOffsets<AT, A> act_offsets(uint32_t wave0, uint32_t n, uint32_t lane)
{
    using Cut = ActCut<A>;
    ActOffsets<AT, A> o;
#pragma unroll
    for (int c = 0; c < Cut::PAIRS; c++) o.b[c] = (wave0 * (uint32_t)A + (uint32_t)(2 * c) * n + 2u * lane) * (uint32_t)sizeof(AT);
#pragma unroll
    for (int c = 0; c < Cut::SINGLES; c++)
        o.b[Cut::PAIRS + c] = (wave0 * (uint32_t)A + (uint32_t)(2 * Cut::PAIRS + c) * n + lane) * (uint32_t)sizeof(AT);
    return o;
}

// two elements as one access: in global memory a row of controls is only element-aligned (any N, any view), in LDS a pair is
template <typename AT> struct ActPair;
template <> struct ActPair<double> {
    typedef double global_t __attribute__((ext_vector_type(2), aligned(8)));
    typedef double lds_t __attribute__((ext_vector_type(2)));
};
template <> struct ActPair<float> {
    typedef float global_t __attribute__((ext_vector_type(2), aligned(4)));
    typedef float lds_t __attribute__((ext_vector_type(2)));
};

// A wave-uniform element offset, pinned to scalar registers: the loop optimiser otherwise turns a row base that advances per step
// into one 64-bit vector pointer per load, carried around the loop.  (The offset, not the pointer: a pointer rebuilt from integers
// would lose its address space.)
__device__ __forceinline__ int64_t scalar_offset(int64_t v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// `row`: the workgroup's piece of one row of controls (uniform)
template <typename AT, int A>
__device__ __forceinline__ void load_act_slot(const AT *__restrict__ row, const ActOffsets<AT, A> &o, ActSlot<AT, A> &s)
{
    using Cut = ActCut<A>;
    const char *base = reinterpret_cast<const char *>(row);
#pragma unroll
    for (int c = 0; c < Cut::PAIRS; c++) {
        const typename ActPair<AT>::global_t *q = reinterpret_cast<const typename ActPair<AT>::global_t *>(base + o.b[c]);
#if MGX_HOT_ACT_NT
        const typename ActPair<AT>::global_t v = __builtin_nontemporal_load(q);
#else
        const typename ActPair<AT>::global_t v = *q;
#endif
        s.v[2 * c] = v.x; s.v[2 * c + 1] = v.y;
    }
#pragma unroll
    for (int c = 0; c < Cut::SINGLES; c++) {
        const AT *q = reinterpret_cast<const AT *>(base + o.b[Cut::PAIRS + c]);
#if MGX_HOT_ACT_NT
        s.v[2 * Cut::PAIRS + c] = __builtin_nontemporal_load(q);
#else
        s.v[2 * Cut::PAIRS + c] = *q;
#endif
    }
}

// The hand-over: the slot goes into the wave's tile as loaded (consecutive lanes, consecutive bytes), and a lane reads its own
// grid's A controls back.  LDS operations of one wave complete in order, so neither needs a barrier.
template <typename AT, int A>
__device__ __forceinline__ void tile_put(AT *tiles, const ActOffsets<AT, A> &o, const ActSlot<AT, A> &s)
{
    using Cut = ActCut<A>;
    char *base = reinterpret_cast<char *>(tiles);
#pragma unroll
    for (int c = 0; c < Cut::PAIRS; c++) {
        typename ActPair<AT>::lds_t v;
        v.x = s.v[2 * c]; v.y = s.v[2 * c + 1];
        *reinterpret_cast<typename ActPair<AT>::lds_t *>(base + o.b[c]) = v;
    }
#pragma unroll
    for (int c = 0; c < Cut::SINGLES; c++) *reinterpret_cast<AT *>(base + o.b[Cut::PAIRS + c]) = s.v[2 * Cut::PAIRS + c];
}

template <typename AT, int A>
__device__ __forceinline__ void tile_get(const AT *tiles, ActSlot<AT, A> &own)
{
    const AT *m = tiles + threadIdx.x * (uint32_t)A;
#pragma unroll
    for (int j = 0; j < A; j++) own.v[j] = m[j];
}

// a grid's controls in the order a row holds them: genset (goal, request), battery
template <int F, typename AT, int A>
__device__ __forceinline__ RawActions<AT> raw_actions(const ActSlot<AT, A> &own)
{
    RawActions<AT> r;
    int k = 0;
    if constexpr (F & F_GENSET) { r.a_goal = own.v[k]; r.a_gen = own.v[k + 1]; k += 2; }
    if constexpr (F & F_BATTERY) { r.a_bat = own.v[k]; k += 1; }
    return r;
}

template <int F, int U, typename AT>
__global__ __launch_bounds__(BLOCK_K) void step_k_hot_kernel(const KArgs a, const AT *__restrict__ actions, int32_t t0, int32_t K,
                                                             int normalized, double *__restrict__ reward, double *__restrict__ soc_trace,
                                                             double *__restrict__ ret_acc, int32_t gpb)
{
    static_assert((F & (F_GRID | F_GRID_FIRST)) == 0 && F != 0, "layouts 1, 2, 3");
    constexpr bool TILE = MGX_HOT_ACT_TILE != 0;
    constexpr int A_DIM = 2 * ((F & F_GENSET) != 0) + ((F & F_BATTERY) != 0);
    // memory operations of one step: its refill (TILE: the loads ActCut cuts a piece into, else at most two) and its stores
    constexpr int VM_OPS = (TILE ? ActCut<A_DIM>::LOADS : 2) + 1 + ((F & F_BATTERY) != 0);
    static_assert(U >= 2 && (U - 1) * VM_OPS < 64, "the operations of U - 1 steps behind a slot must fit the 6-bit vmcnt");
    const int32_t K_launch = K;          // what the host asked for (the counter always moves by this much)
    t0 = resolve_t(a, t0);
    K = resolve_k(a, t0, K);
    const int64_t i = (int64_t)a.g0 + (int64_t)blockIdx.x * gpb + threadIdx.x;
    const bool active = (int32_t)threadIdx.x < gpb && i < a.g1;
    const int64_t N = a.N;
    const uint32_t i32 = (uint32_t)i;    // lane offset of every [K, N] stream: row base in SGPRs + this
    const bool norm = normalized != 0;
    const int32_t k_last = K - 1;

    // TILE: the wave's first grid and how many grids it has (wave-uniform; active <=> lane < n_wave, the inactive lanes leave below)
    const int32_t wave0 = __builtin_amdgcn_readfirstlane((int32_t)threadIdx.x) & ~63;
    const int64_t wg_first = (int64_t)a.g0 + (int64_t)blockIdx.x * gpb;
    const int64_t wave_room = (int64_t)gpb - wave0 < a.g1 - wg_first - wave0 ? (int64_t)gpb - wave0 : a.g1 - wg_first - wave0;
    const uint32_t n_wave = wave_room < 64 ? (wave_room > 0 ? (uint32_t)wave_room : 0u) : 64u;
    const ActOffsets<AT, A_DIM> aoff = act_offsets<AT, A_DIM>((uint32_t)wave0, n_wave, threadIdx.x & 63u);
    // row r of the workgroup's controls (workgroup bases are multiples of 16 grids: a wave's piece starts on a line of doubles)
    auto piece = [&](int32_t r) __attribute__((always_inline)) { return actions + scalar_offset(((int64_t)r * N + wg_first) * A_DIM); };

    __shared__ double base_lds[2 * FACT_ROWS * PP];
    __shared__ __attribute__((aligned(16))) AT act_tiles[TILE ? (BLOCK_K / 64) * 64 * A_DIM : 1];
    Params p; State s; Derived d;
    GridFactors f;
    f.lr = 0.0; f.pr = 0.0; f.lp = 0u; f.pp = 0u; f.cp = 0u; f.pat = 0u;
    bool gen_instant = false;
    // the ring: (TILE) U rows as loaded, row r in slot r % U; (else) U - 1 rows of the lane's own controls in ring[], slot r % U
    ActSlot<AT, A_DIM> slots[TILE ? U : 1];
    RawActions<AT> ring[TILE ? 1 : U];
    if (active) {
        load_state<F>(a.c, i, false, s);
        load_params<F>(a.c, i, p);
        derive<F>(p, d);
        gen_instant = genset_wave_is_instant<F>(p, s);
        load_factors<F>(a.c, i, f);
        // the ring's first rows (clamped to row K - 1: no address outside the caller's controls is formed)
#pragma unroll
        for (int u = 0; u < (TILE ? U : U - 1); u++) {
            const int32_t r = u < k_last ? u : k_last;
            if constexpr (TILE) load_act_slot<AT, A_DIM>(piece(r), aoff, slots[u]);
            else load_actions_at<F>(actions + (int64_t)r * N * A_DIM, i32, ring[u]);
        }
    }
    __syncthreads();
    stage_base_rows<F>(a.c, (int64_t)t0, K, base_lds, BLOCK_K);
    __syncthreads();
    if (!active) return;                 // (no barrier follows: advance_counter_in_kernel's is skipped by returned waves, as in step_k_kernel)

    // TILE: the controls of the step at hand, read out of the tile one step ahead (row 0: here)
    ActSlot<AT, A_DIM> cur;
    if constexpr (TILE) {
        tile_put<AT, A_DIM>(act_tiles, aoff, slots[0]);
        tile_get<AT, A_DIM>(act_tiles, cur);
    }
    BaseVals nb = read_base_row<F>(base_lds, 0, f);

    double ret = 0.0;
    // one step: the slot's controls, this step's series values (the base row was read one step ahead), the next base row, the step
    auto step = [&](auto gi_tag, const RawActions<AT> &ra, int32_t k) __attribute__((always_inline)) {
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
    // step k, u = k % U.  TILE: row k + U goes into slot u (row k's, handed over during step k - 1), and row k + 1 goes through the
    // tile while step k computes: U - 1 rows stay in flight behind the slot being handed over.  Else: row k + U - 1 goes into the
    // slot step k - 1 consumed.  mode 0: whole groups whose refills stay below row K; 1: the last whole groups, the refill (and the
    // hand-over of a row K) behind a scalar test; 2: the tail, no refills.
    auto one = [&](auto gi_tag, auto mode_tag, int u, int32_t k) __attribute__((always_inline)) {
        constexpr int mode = decltype(mode_tag)::value;
        if constexpr (TILE) {
            if constexpr (mode == 0) load_act_slot<AT, A_DIM>(piece(k + U), aoff, slots[u]);
            if constexpr (mode == 1) { if (k + U <= k_last) load_act_slot<AT, A_DIM>(piece(k + U), aoff, slots[u]); }
            ActSlot<AT, A_DIM> nxt;
#pragma unroll
            for (int j = 0; j < A_DIM; j++) nxt.v[j] = cur.v[j];
            if (mode == 0 || k < k_last) {
                tile_put<AT, A_DIM>(act_tiles, aoff, slots[(u + 1) % U]);
                tile_get<AT, A_DIM>(act_tiles, nxt);
            }
            step(gi_tag, raw_actions<F, AT, A_DIM>(cur), k);
#pragma unroll
            for (int j = 0; j < A_DIM; j++) cur.v[j] = nxt.v[j];
        } else {
            if constexpr (mode == 0) load_actions_at<F>(actions + (int64_t)(k + U - 1) * N * A_DIM, i32, ring[(u + U - 1) % U]);
            if constexpr (mode == 1) { if (k + U - 1 <= k_last) load_actions_at<F>(actions + (int64_t)(k + U - 1) * N * A_DIM, i32, ring[(u + U - 1) % U]); }
            step(gi_tag, ring[u], k);
        }
    };
    auto run = [&](auto gi_tag) __attribute__((always_inline)) {
        const int32_t k_main = K - K % U;
        constexpr int AHEAD = TILE ? U : U - 1;                        // how far ahead of its step a refill reads
        auto group = [&](int32_t k0, auto mode_tag) __attribute__((always_inline)) {
#pragma unroll
            for (int u = 0; u < U; u++) one(gi_tag, mode_tag, u, k0 + u);
        };
        int32_t k0 = 0;
        if (U - 1 + AHEAD <= k_last) {
            group(0, std::integral_constant<int, 0>{});
            for (k0 = U; k0 + U - 1 + AHEAD <= k_last; k0 += U) group(k0, std::integral_constant<int, 0>{});
        }
        for (; k0 < k_main; k0 += U) group(k0, std::integral_constant<int, 1>{});      // (at most two groups)
#pragma unroll
        for (int u = 0; u < U - 1; u++)
            if (k0 + u < K) one(gi_tag, std::integral_constant<int, 2>{}, u, k0 + u);
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
