"""The policy of the closed-loop fused launches (``mgx_rollout_policy_episodes`` / ``mgx_step_k_policy_episodes``,
``PerGridWindowEnv.rollout_policy`` / ``step_k_policy``): a small float64 network of plain IEEE operations, evaluated inside the
launch on the observation row every grid stands on.  ``MLPPolicy.act`` states the same rule with torch operations, one multiply
and one add at a time in the order the kernels take them, so a host loop ``a = policy.act(obs); obs, r, done, _ = env.step(a)``
reproduces every decision of a fused launch bit for bit (the rule: ``include/mgx.h``, ``mgx_policy``)."""
import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_IN = 12                 # columns of an H = 0 observation row, at most
MAX_ACTIONS = 12            # rows of a priority-list table, at most (the discrete head)
MAX_CONTROLS = 4            # action columns of a layout with one module of every kind, at most (the continuous head)


def _f64(name, a, ndim):
    """``a`` (torch or numpy, float64) with a leading population axis: [P, ...] of ``ndim`` dimensions."""
    if a is None:
        return None
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    if t.dtype != torch.float64:
        raise ValueError(f"{name} must be float64 (the policy is evaluated in float64 on host and device), not {t.dtype}")
    if t.dim() == ndim - 1:
        t = t.unsqueeze(0)
    if t.dim() != ndim:
        raise ValueError(f"{name} must have {ndim - 1} dimensions, or {ndim} with the population axis first; it has shape {tuple(t.shape)}")
    return t.contiguous()


EXPLORE_TAG = 0xE9100000    # fourth Philox counter word of exploration draw number 0 (include/mgx.h, mgx_exploration)
SYNTH_TAG = 0x5EED          # ... of the series and episode draws (pymgrid_amd.generator.synth_uniform_host)
_M32 = 0xFFFFFFFF


def philox_words(seed, grid, counter, tag, device=None):
    """``r[0 .. 3]`` (int64 tensor ``[4, ...]``, each word in ``[0, 2**32)``) of Philox4x32-10 with the counter words
    ``(lo32(grid), hi32(grid), uint32(counter), tag)`` and the key ``(lo32(seed), hi32(seed))``, in torch integer arithmetic on
    ``device``: the device's ``philox4x32_10`` bit for bit.  ``tag = SYNTH_TAG`` gives the words of ``synth_uniform_host``."""
    grid = torch.as_tensor(grid, device=device).to(torch.int64)
    counter = torch.as_tensor(counter, device=grid.device).to(torch.int64)
    grid, counter = torch.broadcast_tensors(grid, counter)
    c0, c1 = grid & _M32, (grid >> 32) & _M32
    c2, c3 = counter & _M32, torch.full_like(grid, int(tag) & _M32)
    k0, k1 = int(seed) & _M32, (int(seed) >> 32) & _M32

    def mul(m, c):               # (hi, lo) words of the 64-bit product m * c, m and c below 2**32: by halves, nothing leaves int64
        lo, hi = m * (c & 0xFFFF), m * (c >> 16)
        full_lo = lo + ((hi & 0xFFFF) << 16)
        return ((hi >> 16) + (full_lo >> 32)) & _M32, full_lo & _M32
    for _ in range(10):
        (h0, l0), (h1, l1) = mul(0xD2511F53, c0), mul(0xCD9E8D57, c2)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return torch.stack([c0, c1, c2, c3])


def uniform53(a, b):
    """U[0, 1) out of two Philox words: ``((a << 21) ^ (b >> 11)) * 2**-53``, the 53-bit value of the device's draws."""
    return ((a << 21) ^ (b >> 11)).to(torch.float64) * (1.0 / 9007199254740992.0)


def explore_normal(seed, grid, counter, column, device=None):
    """``z`` of the continuous head (include/mgx.h, mgx_exploration): the twelve 10-bit fields of draw number ``column`` summed,
    ``(S - 6138) / 1024`` -- mean 0, standard deviation 0.9999995, a multiple of 2**-10 within +-6."""
    r = philox_words(seed, grid, counter, EXPLORE_TAG + int(column), device)
    S = ((r & 1023) + ((r >> 10) & 1023) + ((r >> 20) & 1023)).sum(dim=0)
    return (S.to(torch.float64) - 6138.0) * (1.0 / 1024.0)


def _seed(seed):
    """``seed`` as the 64-bit unsigned key of a counter-based draw."""
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"seed = {seed}: a 64-bit unsigned key")
    return int(seed)


def _scale(scale):
    """``scale`` (None, or float64 ``[N]``, numpy or torch) as a contiguous tensor."""
    if scale is None:
        return None
    t = scale if torch.is_tensor(scale) else torch.as_tensor(np.asarray(scale))
    if t.dtype != torch.float64 or t.dim() != 1:
        raise ValueError(f"scale must be a float64 vector [N], not {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def _sigma_columns(sg, shared):
    """The four ``sigma`` columns of the C structs: one value for every column (``shared``), or ``sg`` with 0.0 behind it."""
    return tuple(sg * MAX_CONTROLS if shared else sg + [0.0] * (MAX_CONTROLS - len(sg)))


class _Draws:
    """What ``Exploration``, ``Sampling`` and ``GaussianSampling`` share: the per-grid ``scale`` and the head of their C struct."""

    def scale_on(self, device, n):
        """``scale`` on ``device`` (None: there is none), checked against the ``n`` grids it names."""
        if self.scale is None:
            return None
        if self.scale.shape[0] != n:
            raise ValueError(f"scale names {self.scale.shape[0]} grids, not {n}")
        return self.scale.to(device)

    def _c_struct(self, cls, device, n_grids):
        """``(cls, keep-alive)`` with its size, ``seed``, the ``sigma`` columns if it has any and ``scale`` on ``device``."""
        st = cls()
        st.struct_size, st.seed = C.sizeof(cls), self.seed
        for o, v in enumerate(getattr(self, "sigma", ())):
            st.sigma[o] = v
        sc = self.scale_on(device, n_grids)
        st.scale = None if sc is None else sc.data_ptr()
        return st, sc


class Exploration(_Draws):
    """What the exploring closed-loop launches add to an ``MLPPolicy`` (``mgx_exploration``, include/mgx.h): epsilon-greedy on the
    discrete head, additive noise ``sigma[o] * z`` on control ``o`` of the continuous head before its clip, both drawn from a
    counter-based generator keyed by ``seed`` -- a draw depends on (seed, grid, step counter, number) alone.  ``sigma``: one value
    for every action column or up to four, one per column; ``scale`` (float64 ``[N]``, numpy or torch): multiplies ``epsilon`` and
    every ``sigma`` of grid i (an exploration ladder; 0 switches a grid back to the greedy head).  Validated as the C calls do."""

    def __init__(self, seed, epsilon=0.0, sigma=None, scale=None):
        self.seed = _seed(seed)
        self.epsilon = float(epsilon)
        if not 0.0 <= self.epsilon <= 1.0:
            raise ValueError(f"epsilon = {epsilon}: a probability in [0, 1]")
        sg = [0.0] if sigma is None else [float(v) for v in np.atleast_1d(np.asarray(sigma, dtype=np.float64))]
        if len(sg) > MAX_CONTROLS:
            raise ValueError(f"sigma holds {len(sg)} values: a layout has at most {MAX_CONTROLS} action columns")
        if not all(v >= 0.0 for v in sg):
            raise ValueError(f"sigma = {sigma}: standard deviations are >= 0")
        self.sigma = _sigma_columns(sg, sigma is None or np.ndim(sigma) == 0)
        self.scale = _scale(scale)

    def c_struct(self, device, n_grids):
        """``(mgx_exploration, keep-alive)`` with ``scale`` on ``device``."""
        st, sc = self._c_struct(_lib.Exploration, device, n_grids)
        st.epsilon = self.epsilon
        return st, sc


EXP_COEFFS = (1.0, 1.0, 0.5, 0.16666666666666666, 0.041666666666666664, 0.008333333333333333, 0.001388888888888889,
              0.0001984126984126984, 2.48015873015873e-05, 2.7557319223985893e-06, 2.755731922398589e-07, 2.505210838544172e-08,
              2.08767569878681e-09, 1.6059043836821613e-10)      # the doubles nearest 1/n!, n = 0 .. 13 (include/mgx.h, mgx_sampling)
EXP_MIN = -708.0


def policy_exp(d):
    """``E(d)`` of ``mgx_sampling`` (include/mgx.h) for a float64 tensor ``-708 <= d <= 0``: the device's ``policy_exp`` operation by
    operation -- separate multiplies and adds, the scale ``2**k`` built from its bits -- so the two agree bit for bit."""
    k = torch.floor(d * 1.4426950408889634 + 0.5)
    r = (d - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10
    p = torch.full_like(d, EXP_COEFFS[13])
    for n in range(12, -1, -1):
        p = p * r + EXP_COEFFS[n]
    return p * ((k.to(torch.int64) + 1023) << 52).view(torch.float64)


class Sampling(_Draws):
    """What the sampling closed-loop launch adds to a discrete ``MLPPolicy`` (``mgx_sampling``, include/mgx.h): the id of every step is
    drawn from ``softmax(y / temperature)`` by a counter-based draw keyed by ``seed``, and the launch returns the probability of the id
    taken.  ``scale`` (float64 ``[N]``, numpy or torch) multiplies the temperature of grid i (a ladder; 0 switches a grid back to the
    greedy head, as ``temperature=0`` does for all).  Validated as the C call does."""

    def __init__(self, seed, temperature=1.0, scale=None):
        self.seed = _seed(seed)
        self.temperature = float(temperature)
        if not 0.0 <= self.temperature < float("inf"):
            raise ValueError(f"temperature = {temperature}: finite and >= 0")
        self.scale = _scale(scale)

    def c_struct(self, device, n_grids):
        """``(mgx_sampling, keep-alive)`` with ``scale`` on ``device``."""
        st, sc = self._c_struct(_lib.Sampling, device, n_grids)
        st.temperature = self.temperature
        return st, sc


LN2_HI, LN2_LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10     # the two ln 2 constants of E and L
SQRT2, HALF_PI, HALF_LOG_2PI = 1.4142135623730951, 1.5707963267948966, 0.9189385332046727
LOG_COEFFS = tuple(2.0 / (2 * n + 1) for n in range(11))           # the doubles nearest 2 / (2n + 1) (include/mgx.h, mgx_gaussian)
SIN_COEFFS = (-0.16666666666666666, 0.008333333333333333, -0.0001984126984126984, 2.7557319223985893e-06, -2.505210838544172e-08,
              1.6059043836821613e-10, -7.647163731819816e-13)      # ... nearest -+1/k!, k = 3, 5 .. 15
COS_COEFFS = (-0.5, 0.041666666666666664, -0.001388888888888889, 2.48015873015873e-05, -2.755731922398589e-07, 2.08767569878681e-09,
              -1.1470745597729725e-11, 4.779477332387385e-14)      # ... nearest -+1/k!, k = 2, 4 .. 16
GAUSS_DRAW = 8              # draw number of normal pair 0 (numbers 0 .. 3: the exploring head, 1: softmax sampling)


def policy_log(a):
    """``L(a)`` of ``mgx_gaussian`` (include/mgx.h) for a float64 tensor of positive normal numbers: the device's ``policy_log``
    operation by operation -- exponent and mantissa out of the bits, one division, separate multiplies and adds -- so the two agree
    bit for bit.  Within 4 ulp of ``torch.log``; ``policy_log(1.0) == 0.0``."""
    bits = a.contiguous().view(torch.int64)
    e = ((bits >> 52) & 0x7FF) - 1023
    m = ((bits & ((1 << 52) - 1)) | (1023 << 52)).view(torch.float64)
    big = m > SQRT2
    m = torch.where(big, m * 0.5, m)
    e = (e + big.to(torch.int64)).to(torch.float64)
    t = (m - 1.0) / (m + 1.0)
    w = t * t
    p = torch.full_like(t, LOG_COEFFS[10])
    for n in range(9, -1, -1):
        p = p * w + LOG_COEFFS[n]
    return e * LN2_HI + (e * LN2_LO + t * p)


def policy_quarter_turn(f):
    """``(sin, cos)`` of ``f`` quarter turns (the angle ``f * pi / 2``) by the rule of ``mgx_gaussian`` (include/mgx.h), for a
    float64 tensor of multiples of 2**-52 in [0, 1): the device's ``policy_quarter_turn`` operation by operation."""
    hi = f > 0.5
    g = torch.where(hi, 1.0 - f, f)
    x = g * HALF_PI
    w = x * x
    q = torch.full_like(x, SIN_COEFFS[6])
    for n in range(5, -1, -1):
        q = q * w + SIN_COEFFS[n]
    s = x * (q * w + 1.0)
    c = torch.full_like(x, COS_COEFFS[7])
    for n in range(6, -1, -1):
        c = c * w + COS_COEFFS[n]
    c = c * w + 1.0
    return torch.where(hi, c, s), torch.where(hi, s, c)


RSQRT_MAGIC = 0x5FE6EB50C7B537A9


def policy_sqrt(v):
    """``S(v)`` of ``mgx_gaussian`` (include/mgx.h) for a finite float64 tensor: the square root as a fixed sequence of multiplies and
    adds -- ``1 / sqrt(v)`` from its bits, four Newton steps, one correction -- so host and device agree bit for bit; within 1 ulp of
    ``torch.sqrt``, 0.0 where ``not v > 0``."""
    pos = v > 0
    a = torch.where(pos, v, torch.ones_like(v))
    y = (RSQRT_MAGIC - (a.contiguous().view(torch.int64) >> 1)).view(torch.float64)
    h = 0.5 * a
    for _ in range(4):
        y = y * (1.5 - (h * y) * y)
    r = a * y
    return torch.where(pos, r + (0.5 * y) * (a - r * r), torch.zeros_like(v))


def uniforms_of_words(r):
    """``(u1, q, f)`` out of the four words ``r`` of one draw (``mgx_gaussian``): the radius' uniform in (0, 1], the quadrant (int64,
    0 .. 3) and the fraction of a quarter turn."""
    u1 = 1.0 - uniform53(r[0], r[1])
    q = r[2] >> 30                                                  # (bits 63, 62 of a64 = r[2] << 32 | r[3])
    f = ((((r[2] & 0x3FFFFFFF) << 22) | (r[3] >> 10)).to(torch.float64)) * (1.0 / 4503599627370496.0)
    return u1, q, f


def pair_of_words(r):
    """Four words of one draw -> a normal pair by Box-Muller on the rule's own logarithm, square root, sine and cosine
    (``mgx_gaussian``): the device's ``gaussian_pair_of_words`` bit for bit.  What ``gaussian_pair`` and ``cem_pair`` share."""
    u1, q, f = uniforms_of_words(r)
    R = policy_sqrt(-2.0 * policy_log(u1))
    s, c = policy_quarter_turn(f)
    sin = torch.where(q == 0, s, torch.where(q == 1, c, torch.where(q == 2, -s, -c)))
    cos = torch.where(q == 0, c, torch.where(q == 1, -s, torch.where(q == 2, -c, s)))
    return R * cos, R * sin


def gaussian_uniforms(seed, grid, counter, pair, device=None):
    """``(u1, q, f)`` of normal pair ``pair`` (``mgx_gaussian``), out of draw number ``GAUSS_DRAW + pair``."""
    return uniforms_of_words(philox_words(seed, grid, counter, EXPLORE_TAG + GAUSS_DRAW + int(pair), device))


def gaussian_pair(seed, grid, counter, pair, device=None):
    """``(z[2 * pair], z[2 * pair + 1])`` of ``mgx_gaussian`` (include/mgx.h): two independent standard normal draws of grid
    ``grid`` at step counter ``counter`` by Box-Muller on the rule's own logarithm, sine and cosine -- the device's
    ``gaussian_pair`` bit for bit."""
    return pair_of_words(philox_words(seed, grid, counter, EXPLORE_TAG + GAUSS_DRAW + int(pair), device))


CEM_TAG = 0xCE300000        # fourth Philox counter word of normal pair 0 of a CEM candidate (include/mgx.h, mgx_cem)


def policy_clip(v):
    """The clip of ``mgx_policy``: ``0.0`` where ``not v > 0`` (a NaN too), ``1.0`` where ``v > 1``, else ``v``."""
    return torch.where(~(v > 0), torch.zeros_like(v), torch.where(v > 1, torch.ones_like(v), v))


def cem_pair(key, grid, cand, step, pair, device=None):
    """``(z[2 * pair], z[2 * pair + 1])`` of grid ``grid`` (below 2**32), candidate ``cand``, plan step ``step`` (``mgx_cem``,
    include/mgx.h): the counter words ``(lo32(grid), cand, step, CEM_TAG + pair)`` under ``key``, turned into a pair as
    ``gaussian_pair`` turns its words -- the device's ``cem_pair`` bit for bit."""
    grid = torch.as_tensor(grid, device=device).to(torch.int64)
    cand = torch.as_tensor(cand, device=grid.device).to(torch.int64)
    return pair_of_words(philox_words(key, grid + (cand << 32), step, CEM_TAG + int(pair), grid.device))


def _cem_check(mean, sigma):
    for name, t in (("mean", mean), ("sigma", sigma)):
        if not torch.is_tensor(t) or t.dtype != torch.float64 or t.dim() != 3:
            raise ValueError(f"{name} must be a float64 tensor [H, N, A], not {getattr(t, 'dtype', type(t))} {list(getattr(t, 'shape', ()))}")
    if mean.shape != sigma.shape or mean.device != sigma.device:
        raise ValueError(f"mean {list(mean.shape)} on {mean.device} and sigma {list(sigma.shape)} on {sigma.device} must agree")
    H, N, A = mean.shape
    if H < 1 or N < 1 or not 1 <= A <= MAX_CONTROLS:
        raise ValueError(f"mean must be [H, N, A] with H, N >= 1 and 1 <= A <= {MAX_CONTROLS}, not {list(mean.shape)}")
    return int(H), int(N), int(A)


def _cem_values(mean, sigma, key, cand, grid, dtype):
    """``x[cand, k, grid, o]`` of ``mgx_cem`` for ``mean`` / ``sigma`` ``[H, N, A]``, ``cand`` int64 broadcastable against
    ``[..., H, N]`` and ``grid`` int64 ``[N]`` (the grids' numbers): float64 ``[..., H, N, A]``, rounded once where ``dtype`` is
    float32."""
    if dtype not in (torch.float64, torch.float32):
        raise ValueError("dtype must be torch.float64 or torch.float32")
    H, N, A = mean.shape
    step = torch.arange(H, dtype=torch.int64, device=mean.device).view(H, 1)
    drawn = cand >= 1
    cols = []
    for p in range((A + 1) // 2):
        for o, z in zip((2 * p, 2 * p + 1), cem_pair(key, grid, cand, step, p)):
            if o < A:
                m, s = mean[..., o], sigma[..., o]
                cols.append(torch.where((s > 0) & drawn, m + s * z, m))
    x = policy_clip(torch.stack(torch.broadcast_tensors(*cols), dim=-1))
    return x.to(torch.float32).to(torch.float64) if dtype == torch.float32 else x


def cem_candidates_host(mean, sigma, C, key, dtype=torch.float64, grid=None, first=0):
    """The candidates ``mgx_lookahead_gaussian_episodes`` draws inside its launch, as the plan tensor it never builds (``mgx_cem``,
    include/mgx.h, operation by operation in torch, on any device): ``[C, H, N, A]`` in ``dtype`` from ``mean`` / ``sigma`` float64
    ``[H, N, A]`` -- candidate 0 the clipped mean, candidate ``c >= 1`` ``clip(mean + sigma * z)`` on the columns with
    ``sigma > 0``, ``z`` a function of ``(key, grid, c, plan step, column)`` alone.  float32: the float64 values rounded once.
    ``grid`` (int64 ``[N]``, default ``0 .. N - 1``): the numbers of the grids the rows belong to; ``first``: the number of the
    first candidate (a subset evaluated on its own gives the same values)."""
    H, N, A = _cem_check(mean, sigma)
    C = int(C)
    if C < 1 or int(first) < 0:
        raise ValueError("C must be positive and first non-negative")
    dev = mean.device
    grid = torch.arange(N, dtype=torch.int64, device=dev) if grid is None else torch.as_tensor(grid, device=dev).to(torch.int64)
    if grid.shape != (N,):
        raise ValueError(f"grid must name the {N} grids of mean")
    cand = torch.arange(int(first), int(first) + C, dtype=torch.int64, device=dev).view(C, 1, 1)
    return _cem_values(mean, sigma, int(key), cand, grid, dtype).to(dtype).contiguous()


def cem_refit_host(ret, steps, mean, sigma, key, n_elite, alpha=1.0, sigma_min=0.0, dtype=torch.float64):
    """The rule of ``mgx_cem_refit`` (include/mgx.h) in torch, on any device, operation by operation: from the returns ``ret``
    float64 ``[C, N]`` of a launch over the candidates of ``(mean, sigma, key)`` and the steps it counted (``steps`` int32 ``[N]``
    or None: H) to ``elite`` int32 ``[n_elite, N]`` (the explicit loop: the first maximum among the candidates not yet taken, a
    later one replaces it where GREATER), the refitted ``mean`` / ``sigma`` ``[H, N, A]`` (rows ``k >= steps`` pass through) and
    ``best_plan`` ``[H, N, A]`` in ``dtype`` (candidate ``elite[0]``)."""
    H, N, A = _cem_check(mean, sigma)
    if not torch.is_tensor(ret) or ret.dtype != torch.float64 or ret.dim() != 2 or ret.shape[1] != N or ret.shape[0] < 1:
        raise ValueError(f"ret must be a float64 tensor [C, {N}], not {getattr(ret, 'dtype', type(ret))} {list(getattr(ret, 'shape', ()))}")
    Cn, E = int(ret.shape[0]), int(n_elite)
    if not 1 <= E <= min(Cn, 32):
        raise ValueError(f"n_elite = {n_elite} is outside [1, min(C, 32)], C = {Cn}")
    alpha, sigma_min = float(alpha), float(sigma_min)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha = {alpha} is outside [0, 1]")
    if not sigma_min >= 0.0:
        raise ValueError(f"sigma_min = {sigma_min} is negative or NaN")
    if steps is not None and (not torch.is_tensor(steps) or steps.dtype != torch.int32 or tuple(steps.shape) != (N,)):
        raise ValueError(f"steps must be an int32 tensor [{N}] or None")
    dev = mean.device
    grid = torch.arange(N, dtype=torch.int64, device=dev)
    taken = torch.zeros((Cn, N), dtype=torch.bool, device=dev)
    elite = torch.empty((E, N), dtype=torch.int32, device=dev)
    for e in range(E):
        b = torch.full((N,), -1, dtype=torch.int32, device=dev)
        bv = torch.zeros(N, dtype=torch.float64, device=dev)
        for c in range(Cn):
            take = ~taken[c] & ((b < 0) | (ret[c] > bv))
            b = torch.where(take, torch.full_like(b, c), b)
            bv = torch.where(take, ret[c], bv)
        elite[e] = b
        taken[b.long(), grid] = True
    xs = [_cem_values(mean, sigma, int(key), elite[e].long().view(1, N), grid, dtype) for e in range(E)]     # each [H, N, A]
    tot = torch.zeros_like(mean)
    for x in xs:
        tot = tot + x
    En = torch.full_like(mean, float(E))          # (a tensor: torch divides by a NUMBER on the GPU as a multiply by its reciprocal)
    m = tot / En
    q = torch.zeros_like(mean)
    for x in xs:
        d = x - m
        q = q + d * d
    d = policy_sqrt(q / En)
    sg = alpha * d + (1.0 - alpha) * sigma
    n = torch.full((N,), H, dtype=torch.int32, device=dev) if steps is None else steps
    fit = (torch.arange(H, dtype=torch.int32, device=dev).view(H, 1) < n.view(1, N)).unsqueeze(-1)
    return {"elite": elite,
            "mean": torch.where(fit, alpha * m + (1.0 - alpha) * mean, mean),
            "sigma": torch.where(fit, torch.where(sg > sigma_min, sg, torch.full_like(sg, sigma_min)), sigma),
            "best_plan": xs[0].to(dtype).contiguous()}


class GaussianSampling(_Draws):
    """What the Gaussian closed-loop launch adds to a continuous ``MLPPolicy`` (``mgx_gaussian``, include/mgx.h): control ``o`` is
    drawn from ``N(y[o], s[o]**2)``, ``s[o] = sigma[o] * scale[i]``, by a counter-based Box-Muller draw keyed by ``seed``, clipped
    as the greedy head clips; the launch returns the pre-clip action and its exact log-density.  ``sigma``: one value for every
    action column or up to four, one per column (0: that column stays greedy and drops out of the log-probability); ``scale``
    (float64 ``[N]``, numpy or torch) multiplies every sigma of grid i (0 switches a grid back to the greedy head).  Validated as
    the C call does: a sigma is 0 or a positive NORMAL float64 (the rule's logarithm reads exponent and mantissa)."""

    def __init__(self, seed, sigma, scale=None):
        self.seed = _seed(seed)
        sg = [float(v) for v in np.atleast_1d(np.asarray(sigma, dtype=np.float64))]
        if not 1 <= len(sg) <= MAX_CONTROLS:
            raise ValueError(f"sigma holds {len(sg)} values: one, or one per action column (at most {MAX_CONTROLS})")
        if not all(v == 0.0 or np.finfo(np.float64).tiny <= v < float("inf") for v in sg):
            raise ValueError(f"sigma = {sigma}: standard deviations are 0 or positive, finite and not subnormal")
        self.sigma = _sigma_columns(sg, np.ndim(sigma) == 0)
        self.scale = _scale(scale)

    def c_struct(self, device, n_grids):
        """``(mgx_gaussian, keep-alive)`` with ``scale`` on ``device``."""
        return self._c_struct(_lib.Gaussian, device, n_grids)


class MLPPolicy:
    """``y = W2 . relu(W1 . x + b1) + b2`` (``W1 = b1 = None``: the linear policy ``y = W2 . x + b2``) on the observation row ``x``,
    every sum taken in index order with a separate multiply and add; ``relu(h) = h if h > 0 else +0.0``.

    ``head="discrete"``: the action is the lowest ``o`` whose ``y[o]`` is strictly greater than everything before it, starting from
    ``-inf`` -- ties go to the lowest index, a NaN never wins, all-NaN is id 0; ``n_out`` is the number of rows of the env's
    priority-list table.  ``head="continuous"``: ``u[o] = 0 if not y[o] > 0 else min(y[o], 1)``, normalised controls in the order of
    ``layout.action_names``.

    Shapes: ``W1 [n_hidden, n_in]``, ``b1 [n_hidden]``, ``W2 [n_out, n_hidden or n_in]``, ``b2 [n_out]`` -- or each with a leading
    population axis ``P``; ``policy_index`` (int32 ``[N]``) then names the parameter set of every grid (absent: set 0 for all; an
    index outside ``[0, P)``: set 0).  All parameters are float64."""

    def __init__(self, W1, b1, W2, b2, policy_index=None, head="discrete"):
        if head not in ("discrete", "continuous"):
            raise ValueError(f"head must be 'discrete' or 'continuous', not {head!r}")
        self.head = head
        if (W1 is None) != (b1 is None):
            raise ValueError("W1 and b1 come together (both None: a linear policy)")
        self.W1, self.b1 = _f64("W1", W1, 3), _f64("b1", b1, 2)
        self.W2, self.b2 = _f64("W2", W2, 3), _f64("b2", b2, 2)
        if self.W2 is None or self.b2 is None:
            raise ValueError("W2 and b2 are required")
        P, n_out, n_mid = self.W2.shape
        self.n_policies, self.n_out = int(P), int(n_out)
        if self.W1 is not None:
            self.n_hidden, self.n_in = int(self.W1.shape[1]), int(self.W1.shape[2])
            if self.n_hidden < 1:
                raise ValueError("W1 holds no hidden unit (a linear policy: W1 = b1 = None)")
            if tuple(self.W1.shape) != (P, n_mid, self.n_in) or tuple(self.b1.shape) != (P, self.n_hidden):
                raise ValueError(f"W1 {tuple(self.W1.shape)} / b1 {tuple(self.b1.shape)} do not fit W2 {tuple(self.W2.shape)}: "
                                 f"W1 [P, n_hidden, n_in], b1 [P, n_hidden], W2 [P, n_out, n_hidden]")
        else:
            self.n_hidden, self.n_in = 0, int(n_mid)
        if tuple(self.b2.shape) != (P, n_out):
            raise ValueError(f"b2 {tuple(self.b2.shape)} does not fit W2 {tuple(self.W2.shape)}: b2 [P, n_out]")
        if P < 1:
            raise ValueError("an empty population")
        if not 1 <= self.n_in <= MAX_IN:
            raise ValueError(f"n_in = {self.n_in}: an observation row without a forecast holds 1 to {MAX_IN} columns")
        if self.n_hidden > _lib.POLICY_MAX_HIDDEN:
            raise ValueError(f"n_hidden = {self.n_hidden}: at most {_lib.POLICY_MAX_HIDDEN} (MGX_POLICY_MAX_HIDDEN)")
        if head == "discrete" and not 1 <= self.n_out <= MAX_ACTIONS:
            raise ValueError(f"n_out = {self.n_out}: a priority-list table holds 1 to {MAX_ACTIONS} actions")
        if head == "continuous" and self.n_out > MAX_CONTROLS:
            raise ValueError(f"n_out = {self.n_out}: a layout has at most {MAX_CONTROLS} action columns")
        if self.lds_bytes > _lib.POLICY_LDS_BYTES:
            raise ValueError(f"{P} parameter sets take {self.lds_bytes} bytes where the kernels keep them, at most "
                             f"{_lib.POLICY_LDS_BYTES} (MGX_POLICY_LDS_BYTES)")
        devices = {t.device for t in (self.W1, self.b1, self.W2, self.b2) if t is not None}
        if len(devices) != 1:
            raise ValueError(f"the parameters lie on different devices: {sorted(map(str, devices))}")
        self.policy_index = None
        if policy_index is not None:
            idx = policy_index if torch.is_tensor(policy_index) else torch.as_tensor(np.asarray(policy_index))
            if idx.dtype != torch.int32 or idx.dim() != 1:
                raise ValueError(f"policy_index must be an int32 vector [N], not {idx.dtype} {tuple(idx.shape)}")
            self.policy_index = idx.contiguous()

    @property
    def lds_bytes(self):
        """Bytes of the parameter sets as the kernels stage them (include/mgx.h, MGX_POLICY_LDS_BYTES)."""
        m = (self.n_out + 3) // 4 * 4 if self.head == "discrete" else self.n_out
        per_set = m + (self.n_hidden * (self.n_in + 1 + m) if self.n_hidden else self.n_in * m)
        return self.n_policies * ((per_set + 1) // 2 * 2) * 8

    def to(self, device):
        """The policy with its parameters on ``device``: ``self`` where they already lie there, else a COPY made now.  Nothing is
        cached -- numpy parameters share their memory with the caller's arrays, so a search loop may update them in place between
        launches and ``act`` and every fused launch see the current values (the launch copies them to the device each time; keep
        the parameters on the device, as torch tensors, to avoid the copy)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.W2.device == device and (self.policy_index is None or self.policy_index.device == device):
            return self
        mv = lambda t: None if t is None else t.to(device)     # noqa: E731
        return MLPPolicy(mv(self.W1), mv(self.b1), mv(self.W2), mv(self.b2), mv(self.policy_index), head=self.head)

    def _sets(self, n, device):
        """None (one set for all grids) or the long index [n] of every grid's set, out-of-range indices mapped to 0."""
        if self.policy_index is None:
            return None
        idx = self.policy_index.to(device).long()
        if idx.shape[0] != n:
            raise ValueError(f"policy_index names {idx.shape[0]} grids, the observations {n}")
        return torch.where((idx >= 0) & (idx < self.n_policies), idx, torch.zeros_like(idx))

    @staticmethod
    def _layer(W, b, idx, v):
        """[N, O]: b + sum over j in order of W[..., j] * v[:, j], one multiply and one add at a time."""
        if idx is None:
            Wn, acc = W[0].unsqueeze(0), b[0].unsqueeze(0).expand(v.shape[0], -1)
        else:
            Wn, acc = W[idx], b[idx]
        for j in range(W.shape[2]):
            acc = acc + Wn[:, :, j] * v[:, j:j + 1]
        return acc

    def _trunk(self, x, idx):
        """``(h, y)`` for float64 rows ``x`` [n, n_in] on the parameters' device: the hidden vector after its ReLU (``x`` itself for a
        linear policy) and the outputs [n, n_out]; ``idx``: what ``_sets`` gave."""
        h = x
        if self.n_hidden:
            hp = self._layer(self.W1, self.b1, idx, x)
            h = torch.where(hp > 0, hp, torch.zeros_like(hp))
        return h, self._layer(self.W2, self.b2, idx, h)

    def _forward(self, obs):
        """``(h, y, idx)`` of ``_trunk`` for observation rows ``obs`` [N, n_in], row n the row of grid n."""
        if not torch.is_tensor(obs):
            obs = torch.as_tensor(np.asarray(obs))
        if obs.dim() != 2 or obs.shape[1] != self.n_in or obs.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"obs must be float32 or float64 rows [N, {self.n_in}], not {obs.dtype} {tuple(obs.shape)}")
        me = self.to(obs.device)
        x = obs.to(torch.float64)
        idx = me._sets(x.shape[0], x.device)
        return me._trunk(x, idx) + (idx,)

    def outputs(self, obs):
        """``y`` [N, n_out] for observation rows ``obs`` [N, n_in] (float32 rows are widened to float64, not re-rounded)."""
        return self._forward(obs)[1]

    def act(self, obs, exploration=None, counter=None, return_prob=False, return_logp=False, return_raw=False):
        """The actions for observation rows ``obs`` [N, n_in]: priority-list ids (int32 [N]) or normalised controls (float64
        [N, n_out]) -- what the fused launches take, bit for bit.  ``exploration`` (an ``Exploration``) with ``counter``, the int the
        handle's shared step counter holds BEFORE the step (``env.current_step``): the host statement of the rule of
        ``mgx_exploration`` (include/mgx.h) -- row n of ``obs`` is grid n -- and what the exploring launches take, bit for bit.
        A ``Sampling`` in its place (discrete head only): the rule of ``mgx_sampling``, what the sampling launch takes;
        ``return_prob=True`` then returns ``(ids, prob)``, ``prob`` (float64 [N]) the probability of the id taken.
        A ``GaussianSampling`` (continuous head only): the rule of ``mgx_gaussian``, what the Gaussian launch takes;
        ``return_logp=True`` / ``return_raw=True`` then return ``(u, logp, raw)`` (the ones asked for, in this order): ``logp``
        (float64 [N]) the log-density of the pre-clip action ``raw`` (float64 [N, n_out])."""
        if isinstance(exploration, GaussianSampling):
            if self.head != "continuous":
                raise ValueError("a GaussianSampling goes with the continuous head (the discrete head samples with Sampling)")
            if counter is None:
                raise ValueError("sampling needs `counter`, the handle's step counter before the step (env.current_step)")
            if return_prob:
                raise ValueError("return_prob=True goes with a Sampling (a density has no probability: return_logp=True)")
            u, logp, raw = self._gaussian(self.outputs(obs), exploration, int(counter))
            res = (u,) + ((logp,) if return_logp else ()) + ((raw,) if return_raw else ())
            return res if len(res) > 1 else u
        if return_logp or return_raw:
            raise ValueError("return_logp=True / return_raw=True go with a GaussianSampling")
        if isinstance(exploration, Sampling):
            if self.head != "discrete":
                raise ValueError("sampling is offered on the discrete head (the continuous head explores with Exploration.sigma)")
            if counter is None:
                raise ValueError("sampling needs `counter`, the handle's step counter before the step (env.current_step)")
            ids, prob = self._sample(self.outputs(obs), exploration, int(counter))
            return (ids, prob) if return_prob else ids
        if return_prob:
            raise ValueError("return_prob=True goes with a Sampling")
        y = self.outputs(obs)
        n, dev = y.shape[0], y.device
        if exploration is not None:
            if counter is None:
                raise ValueError("exploration needs `counter`, the handle's step counter before the step (env.current_step)")
            grid = torch.arange(n, dtype=torch.int64, device=dev)
            scale = exploration.scale_on(dev, n)
        if self.head == "continuous":
            if exploration is not None and self.n_out:
                cols = []
                for o in range(self.n_out):
                    s = exploration.sigma[o] if scale is None else exploration.sigma[o] * scale
                    cols.append(y[:, o] + s * explore_normal(exploration.seed, grid, int(counter), o))
                y = torch.stack(cols, dim=1)
            return policy_clip(y)
        ids, _ = self._greedy(y)
        if exploration is not None:
            r = philox_words(exploration.seed, grid, int(counter), EXPLORE_TAG)
            u1, u2 = uniform53(r[0], r[1]), uniform53(r[2], r[3])
            e = exploration.epsilon if scale is None else exploration.epsilon * scale
            k = torch.clamp((u2 * float(self.n_out)).floor().to(torch.int32), max=self.n_out - 1)
            ids = torch.where(u1 < e, k, ids)
        return ids

    def _greedy(self, y):
        """``(ids, best)`` of the discrete head on ``y`` [N, n_out]."""
        n, dev = y.shape[0], y.device
        best = torch.full((n,), float("-inf"), dtype=torch.float64, device=dev)
        ids = torch.zeros(n, dtype=torch.int32, device=dev)
        for o in range(self.n_out):
            m = y[:, o] > best
            best = torch.where(m, y[:, o], best)
            ids = torch.where(m, torch.full_like(ids, o), ids)
        return ids, best

    def sample_weights(self, y, sampling):
        """``(e, S, g, live)`` of the sampling head (``mgx_sampling``) on the outputs ``y`` [N, n_out]: the unnormalised weights
        ``e`` [N, n_out], their sum in index order, the greedy ids and which grids sample at all (``tau > 0``; the others' weights
        are not used)."""
        e, _, S, g, live, _ = self._softmax(y, sampling)
        return torch.stack(e, dim=1), S, g, live

    def _softmax(self, y, sampling, K=1):
        """What lies between the outputs ``y`` [K * N, n_out] (K rows per grid, grid-minor) and the probabilities of the sampling head
        (``mgx_sampling``): ``(e, d, S, g, live, beta)`` -- the columns ``e[o]`` of the unnormalised weights and ``d[o]`` of their
        exponents (1.0 and 0.0 on the greedy id), the sum of the weights in index order, the greedy ids, which rows sample at all
        (``tau > 0``) and ``1 / tau`` of every row (1.0 where it does not sample: nothing of such a row is used)."""
        n, dev = y.shape[0], y.device
        g, best = self._greedy(y)
        scale = sampling.scale_on(dev, n // K)
        tau = torch.full((n,), sampling.temperature, dtype=torch.float64, device=dev)
        if scale is not None:
            tau = tau * scale.repeat(K)
        live = tau > 0
        zero, one = torch.zeros_like(tau), torch.ones_like(tau)
        beta = 1.0 / torch.where(live, tau, one)
        e, d, S = [], [], zero
        for o in range(self.n_out):
            dd = (y[:, o] - best) * beta
            ok = dd >= EXP_MIN                                         # (False for a NaN)
            eo = torch.where(ok, policy_exp(torch.where(ok, dd, torch.full_like(dd, EXP_MIN))), zero)
            e.append(torch.where(g == o, one, eo))
            d.append(torch.where(g == o, zero, dd))
            S = S + e[-1]
        return e, d, S, g, live, beta

    def _sample(self, y, sampling, counter):
        """``(ids, prob)`` by the rule of ``mgx_sampling``: inverse CDF on the unnormalised weights with draw number 1."""
        n, dev = y.shape[0], y.device
        e, S, g, live = self.sample_weights(y, sampling)
        r = philox_words(sampling.seed, torch.arange(n, dtype=torch.int64, device=dev), counter, EXPLORE_TAG + 1)
        v = uniform53(r[0], r[1]) * S
        c = torch.zeros_like(S)
        ids, e_id = g.clone(), torch.ones_like(S)
        open_ = torch.ones(n, dtype=torch.bool, device=dev)
        for o in range(self.n_out):
            c = c + e[:, o]
            take = open_ & (v < c)
            ids = torch.where(take, torch.full_like(ids, o), ids)
            e_id = torch.where(take, e[:, o], e_id)
            open_ = open_ & ~take
        return torch.where(live, ids, g), torch.where(live, e_id / S, torch.ones_like(S))

    def _gaussian(self, y, gs, counter):
        """``(u, logp, raw)`` by the rule of ``mgx_gaussian`` on the outputs ``y`` [N, n_out]: ``raw = y + s * z`` on the live
        columns (``s > 0``), its clip, and the log-density of ``raw`` over the live columns."""
        n, dev = y.shape[0], y.device
        grid = torch.arange(n, dtype=torch.int64, device=dev)
        s, live, _, _, Cn = self._gaussian_consts(gs, n, dev)
        Q, cols = torch.zeros_like(Cn), []
        for p in range((self.n_out + 1) // 2):
            for o, z in zip((2 * p, 2 * p + 1), gaussian_pair(gs.seed, grid, counter, p)):
                if o < self.n_out:
                    cols.append(torch.where(live[o], y[:, o] + s[o] * z, y[:, o]))
                    Q = torch.where(live[o], Q + z * z, Q)
        raw = torch.stack(cols, dim=1) if cols else y
        return policy_clip(raw), (-0.5 * Q) - Cn, raw

    def _gaussian_consts(self, gs, n, dev, K=1):
        """What the Gaussian head (``mgx_gaussian``) knows of a row before it sees ``y``, for ``n = K * N`` rows (K per grid,
        grid-minor): ``(s, live, sd, L, Cn)`` -- per action column ``s[o] = sigma[o] * scale``, whether it is live (``s > 0``), ``sd[o]``
        (``s[o]``, 1.0 on a dead column) and ``L[o] = policy_log(sd[o])``; ``Cn`` the normalising constant over the live columns."""
        scale = gs.scale_on(dev, n // K)
        if scale is not None:
            scale = scale.repeat(K)
        zero = torch.zeros(n, dtype=torch.float64, device=dev)
        s = [zero + gs.sigma[o] if scale is None else gs.sigma[o] * scale for o in range(self.n_out)]
        live = [v > 0 for v in s]
        sd = [torch.where(live[o], s[o], torch.ones_like(zero)) for o in range(self.n_out)]
        L = [policy_log(v) for v in sd]
        Cn = zero
        for o in range(self.n_out):
            Cn = torch.where(live[o], Cn + (L[o] + HALF_LOG_2PI), Cn)
        return s, live, sd, L, Cn

    def c_struct(self, device, n_grids):
        """``(mgx_policy, keep-alive)`` with the parameters on ``device``."""
        me = self.to(device)
        if me.policy_index is not None and me.policy_index.shape[0] != n_grids:
            raise ValueError(f"policy_index names {me.policy_index.shape[0]} grids, the env {n_grids}")
        # (no controllable module, n_out = 0: nothing of W2 / b2 is read, but the C call takes no NULL weights)
        spare = torch.zeros(1, dtype=torch.float64, device=me.W2.device) if me.n_out == 0 else None
        ptr = lambda t: None if t is None else (t.data_ptr() if t.numel() else spare.data_ptr())
        st = _lib.Policy()
        st.struct_size = C.sizeof(_lib.Policy)
        st.n_policies, st.n_in, st.n_hidden, st.n_out = me.n_policies, me.n_in, me.n_hidden, me.n_out
        st.w1, st.b1, st.w2, st.b2, st.policy_index = ptr(me.W1), ptr(me.b1), ptr(me.W2), ptr(me.b2), ptr(me.policy_index)
        return st, (me, spare)


class ValueHead:
    """A critic beside an ``MLPPolicy`` (``mgx_critic``, include/mgx.h): one more output row on the policy's trunk,
    ``V(x) = b + sum over j in order of w[j] * v[j]`` with ``v`` the policy's hidden vector after its ReLU, or ``x`` for a linear
    policy -- a separate multiply and add each.  ``w`` float64 ``[n_mid]`` or ``[P, n_mid]`` (``n_mid`` = the policy's ``n_hidden``,
    or its ``n_in`` without a hidden layer), ``b`` a float64 scalar or ``[P]``; the parameter set of a grid is the policy's own
    (``policy_index``).  The sampling launch evaluates it inside the kernel (``critic=`` of ``rollout_policy``); ``value`` is the same
    rule on the host.  Validated as the C call does.  ``head`` names the head of the policy it sits
    beside: "discrete" (the sampling launch) or "continuous" (the Gaussian launch, ``critic=`` of ``step_k_policy``)."""

    def __init__(self, w, b, head="discrete"):
        if head not in ("discrete", "continuous"):
            raise ValueError(f"head must be 'discrete' or 'continuous', not {head!r}")
        self.head = head
        self.w = _f64("w", w, 2)
        if self.w is None or b is None:
            raise ValueError("w and b are required")
        tb = b if torch.is_tensor(b) else torch.as_tensor(np.asarray(b))
        if tb.dtype != torch.float64:
            raise ValueError(f"b must be float64 (the critic is evaluated in float64 on host and device), not {tb.dtype}")
        if tb.dim() > 1:
            raise ValueError(f"b must be a scalar or a vector [P]; it has shape {tuple(tb.shape)}")
        self.b = tb.reshape(-1).contiguous()
        self.n_policies, self.n_mid = int(self.w.shape[0]), int(self.w.shape[1])
        if self.n_policies < 1 or self.n_mid < 1:
            raise ValueError(f"w {tuple(self.w.shape)}: an empty critic")
        if self.b.shape[0] != self.n_policies:
            raise ValueError(f"b {tuple(self.b.shape)} does not fit w {tuple(self.w.shape)}: b [P]")
        if self.w.device != self.b.device:
            raise ValueError(f"the parameters lie on different devices: {sorted(map(str, (self.w.device, self.b.device)))}")

    def check(self, policy):
        """Whether the head fits ``policy``: an ``MLPPolicy`` of the same ``head`` with as many parameter sets and ``n_mid`` trunk outputs."""
        if not isinstance(policy, MLPPolicy) or policy.head != self.head:
            raise ValueError(f"a ValueHead with head={self.head!r} goes with an MLPPolicy of that head (the sampling launch; "
                             "head='continuous': the Gaussian launch)")
        n_mid = policy.n_hidden or policy.n_in
        if self.n_mid != n_mid or self.n_policies != policy.n_policies:
            raise ValueError(f"w {tuple(self.w.shape)} does not fit the policy: [P, n_mid] = [{policy.n_policies}, {n_mid}]")

    def lds_bytes(self, policy):
        """Bytes of the parameter sets as the critic launch stages them (include/mgx.h, ``mgx_rollout_policy_critic_episodes``)."""
        m = (policy.n_out + 3) // 4 * 4 if policy.head == "discrete" else policy.n_out
        per_set = m + 1 + (policy.n_hidden * (policy.n_in + 2 + m) if policy.n_hidden else policy.n_in * (m + 1))
        return policy.n_policies * ((per_set + 1) // 2 * 2) * 8

    def value(self, policy, obs):
        """``V`` (float64 [N]) for observation rows ``obs`` [N, n_in] (float32 rows are widened): the host statement of the rule,
        what the critic launch writes bit for bit -- row n of ``obs`` is grid n."""
        self.check(policy)
        h, _, idx = policy._forward(obs)
        return self._on(h, idx)

    def _on(self, h, idx):
        """``V`` [n] on the trunk's ``h`` [n, n_mid] (``MLPPolicy._trunk``), ``idx`` the parameter set of every row or None."""
        return MLPPolicy._layer(self.w.to(h.device).unsqueeze(1), self.b.to(h.device).unsqueeze(1), idx, h)[:, 0]

    def c_struct(self, device, n_grids):
        """``(mgx_critic, keep-alive)`` with the parameters on ``device``."""
        w, b = self.w.to(device), self.b.to(device)
        st = _lib.Critic()
        st.struct_size = C.sizeof(_lib.Critic)
        st.w, st.b = w.data_ptr(), b.data_ptr()
        return st, (w, b)


def _gae_args(reward, done, value, last_value, final_value, gamma, lam):
    """The checks ``gae`` and ``gae_host`` share; ``done`` comes back as it was given (bool or uint8)."""
    gamma, lam = float(gamma), float(lam)
    if not 0.0 <= gamma <= 1.0 or not 0.0 <= lam <= 1.0:
        raise ValueError(f"gamma = {gamma}, lam = {lam}: both lie in [0, 1]")
    for name, t in (("reward", reward), ("value", value), ("last_value", last_value), ("final_value", final_value)):
        if t is None and name == "final_value":
            continue
        if not torch.is_tensor(t) or t.dtype != torch.float64:
            raise ValueError(f"{name} must be a float64 tensor, not {getattr(t, 'dtype', type(t))}")
    if not torch.is_tensor(done) or done.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"done must be a bool or uint8 tensor, not {getattr(done, 'dtype', type(done))}")
    if reward.dim() != 2 or reward.shape[0] < 1 or reward.shape[1] < 1:
        raise ValueError(f"reward must be [K, N] with K, N >= 1, not {tuple(reward.shape)}")
    K, N = reward.shape
    for name, t, shape in (("done", done, (K, N)), ("value", value, (K, N)), ("last_value", last_value, (N,)),
                           ("final_value", final_value, (K, N))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name} must have shape {list(shape)}, not {list(t.shape)}")
        if t is not None and t.device != reward.device:
            raise ValueError(f"{name} lies on {t.device}, reward on {reward.device}")
    return int(K), int(N), gamma, lam


def gae_host(reward, done, value, last_value, final_value=None, gamma=0.99, lam=0.95):
    """The rule of ``mgx_gae`` (include/mgx.h) in torch, on any device, operation by operation: ``{"advantages", "returns"}``
    (float64 [K, N]).  ``reward`` / ``value`` / ``final_value`` [K, N], ``done`` bool or uint8 [K, N], ``last_value`` [N]; where
    ``done[k]`` the step bootstraps from ``final_value[k]`` (``None``: 0.0) and the advantage behind it is not carried across."""
    K, N, gamma, lam = _gae_args(reward, done, value, last_value, final_value, gamma, lam)
    c = gamma * lam
    adv, ret = torch.empty_like(reward), torch.empty_like(reward)
    nxt, carry = last_value, torch.zeros_like(last_value)
    for k in range(K - 1, -1, -1):
        d = done[k] != 0
        nv = torch.where(d, final_value[k] if final_value is not None else torch.zeros_like(nxt), nxt)
        delta = (reward[k] + gamma * nv) - value[k]
        A = torch.where(d, delta, delta + c * carry)
        adv[k], ret[k] = A, A + value[k]
        carry, nxt = A, value[k]
    return {"advantages": adv, "returns": ret}


def gae(reward, done, value, last_value, final_value=None, gamma=0.99, lam=0.95, out=None):
    """Generalised advantage estimation over the ``[K, N]`` outputs of a critic launch in ONE kernel (``mgx_gae``; one lane per
    grid, backwards over k): ``{"advantages", "returns"}``, float64 ``[K, N]`` -- ``gae_host``'s values bit for bit.  Device
    tensors: ``done`` bool or uint8, the rest contiguous float64; ``final_value`` (``out["final_values"]`` of the launch) is read
    only where ``done``, ``None`` bootstraps 0.0 there.  ``out``: a dict with your own ``advantages`` and / or ``returns`` (they
    must not overlap the inputs); ``out={"returns": None}`` skips the returns."""
    K, N, gamma, lam = _gae_args(reward, done, value, last_value, final_value, gamma, lam)
    dev = reward.device
    for name, t in (("reward", reward), ("done", done), ("value", value), ("last_value", last_value), ("final_value", final_value)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if dev.type != "cuda":
        raise ValueError(f"gae runs on the GPU (mgx_gae); the tensors lie on {dev} -- gae_host states the same rule anywhere")
    out = out or {}
    unknown = set(out) - {"advantages", "returns"}
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    res = {}
    for name in ("advantages", "returns"):
        if name in out and out[name] is None and name == "returns":
            continue
        t = out.get(name)
        if t is None:
            t = torch.empty((K, N), dtype=torch.float64, device=dev)
        elif not torch.is_tensor(t) or t.dtype != torch.float64 or t.device != dev or not t.is_contiguous() or tuple(t.shape) != (K, N):
            raise ValueError(f"out[{name!r}] must be a contiguous float64 tensor {[K, N]} on {dev}")
        res[name] = t
    d8 = done.view(torch.uint8) if done.dtype == torch.bool else done
    ptr = lambda t: None if t is None else t.data_ptr()     # noqa: E731
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mgx_gae(N, K, ptr(reward), ptr(d8), ptr(value), ptr(final_value), ptr(last_value), gamma, lam,
                                      ptr(res["advantages"]), ptr(res.get("returns")), torch.cuda.current_stream(dev).cuda_stream))
    return res


def decision_rows(obs_before, obs):
    """The rows the K decisions of a closed-loop launch were taken on, ``[K, N, D]``: ``cat(obs_before[None], obs[:-1])`` --
    ``obs_before`` ``[N, D]`` is the observation the env showed before the launch, ``obs`` ``[K, N, D]`` what the launch returned
    (``observations=True``).  ``obs[k]`` is what step k returned, hence the row decision k + 1 read, restarts included: after a restart
    it is the first row of the new episode."""
    if obs.dim() != 3 or obs_before.dim() != 2 or tuple(obs_before.shape) != tuple(obs.shape[1:]) or obs_before.dtype != obs.dtype:
        raise ValueError(f"obs_before {tuple(obs_before.shape)} {obs_before.dtype} is not a row set of obs {tuple(obs.shape)} {obs.dtype}")
    return torch.cat([obs_before.unsqueeze(0), obs[:-1]], dim=0).contiguous()


PPO_GRAD_NAMES = ("W1", "b1", "W2", "b2", "w", "b")      # the gradients in the order ``ppo_grad_flat`` lays them out
PPO_GRAD_NAMES_GAUSSIAN = PPO_GRAD_NAMES + ("log_sigma",)  # ... of the Gaussian head: ``log_sigma`` [4] behind them


def _ppo_checks(head, policy, critic, rows, taken, old, advantages, returns, sampling, clip, vf_coef, ent_coef, mask):
    """The checks of a gradient of ``head`` (a ``_SoftmaxGrad`` or ``_GaussianGrad``: those of ``mgx_policy_grad`` /
    ``mgx_policy_grad_gaussian``), on the host and on the device: ``(K, N, clip, vf_coef, ent_coef)``."""
    if not isinstance(policy, MLPPolicy) or policy.head != head.policy_head:
        raise ValueError(f"this gradient is offered for an MLPPolicy with the {head.policy_head} head (the "
                         f"{'continuous' if head.policy_head == 'discrete' else 'discrete'} head: {head.other})")
    if policy.n_policies != 1 or policy.policy_index is not None:
        raise ValueError("the gradient of a population (several parameter sets, a policy_index) is not offered")
    if not isinstance(sampling, head.sampling):
        raise ValueError(f"sampling must be the {head.sampling.__name__} of the launch that collected the data "
                         f"({head.reads} and scale are read)")
    per_sample = ((head.taken, taken, (head.taken_dtype,), (policy.n_out,) if head.taken_columns else ()),
                  (head.old, old, (torch.float64,), ()), ("advantages", advantages, (torch.float64,), ()))
    if critic is not None:
        if not isinstance(critic, ValueHead):
            raise ValueError("critic must be a ValueHead or None")
        critic.check(policy)
        if returns is None:
            raise ValueError("a critic needs `returns`")
    elif returns is not None:
        raise ValueError("`returns` goes with a critic")
    clip, vf_coef, ent_coef = float(clip), float(vf_coef), float(ent_coef)
    if not clip >= 0.0:
        raise ValueError(f"clip = {clip}: >= 0 (inf: no clipping)")
    if vf_coef != vf_coef or ent_coef != ent_coef:
        raise ValueError("a NaN coefficient")
    if not torch.is_tensor(rows) or rows.dim() != 3 or rows.shape[2] != policy.n_in or rows.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"rows must be float32 or float64 [K, N, {policy.n_in}], not {getattr(rows, 'dtype', type(rows))} "
                         f"{tuple(getattr(rows, 'shape', ()))}")
    K, N = int(rows.shape[0]), int(rows.shape[1])
    if K < 1 or N < 1:
        raise ValueError(f"rows {tuple(rows.shape)}: K and N must be positive")
    for name, t, dts, tail in per_sample + (("returns", returns, (torch.float64,), ()), ("mask", mask, (torch.uint8, torch.bool), ())):
        if t is None and name in ("returns", "mask"):
            continue
        if not torch.is_tensor(t) or t.dtype not in dts or tuple(t.shape) != (K, N) + tail:
            raise ValueError(f"{name} must be a {' or '.join(str(d) for d in dts)} tensor {[K, N] + list(tail)}, not "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
        if t.device != rows.device:
            raise ValueError(f"{name} lies on {t.device}, rows on {rows.device}")
    if head.taken_columns and policy.n_out < 1:
        raise ValueError("a policy without an action column has no density")
    return K, N, clip, vf_coef, ent_coef


def ppo_grad_flat(grads):
    """The gradients of a ``ppo_grad`` / ``ppo_grad_host`` result as one vector ``[P]``, in the order ``PPO_GRAD_NAMES`` (absent ones
    skipped): the columns of ``ppo_grad_host(per_sample=True)["terms"]``.  A result of the Gaussian head (``ppo_grad_gaussian`` /
    ``ppo_grad_gaussian_host``) carries ``log_sigma`` [4] behind them."""
    return torch.cat([grads[n].reshape(-1) for n in PPO_GRAD_NAMES_GAUSSIAN if grads.get(n) is not None])


def _ppo_shapes(head, policy, critic):
    """The shapes of the gradients of ``head`` in the order of ``ppo_grad_flat`` (None: the policy has no such parameter)."""
    n_mid = policy.n_hidden or policy.n_in
    return {"W1": (policy.n_hidden, policy.n_in) if policy.n_hidden else None, "b1": (policy.n_hidden,) if policy.n_hidden else None,
            "W2": (policy.n_out, n_mid), "b2": (policy.n_out,), "w": (n_mid,) if critic is not None else None,
            "b": (1,) if critic is not None else None, **head.extra}


def _ppo_result(flat, stats, shapes):
    """``flat`` (in the order of ``ppo_grad_flat``) cut into the result of a host rule."""
    res, at = {}, 0
    for name, shape in shapes.items():
        if shape is None:
            res[name] = None
            continue
        size = int(np.prod(shape))
        res[name] = flat[at:at + size].reshape(shape)
        at += size
    res["stats"] = stats
    return res


ENTROPY_CONST = 1.4189385332046727     # (1 + log(2 pi)) / 2: the entropy of a unit normal (include/mgx.h, mgx_policy_grad_gaussian)


class _SoftmaxGrad:
    """What the softmax head of the discrete policy adds to the gradient rule (``PgHead<PG_HEAD_SOFTMAX>`` of the kernel).  ``sample``:
    from ``y`` [n, n_out], the ids taken and their old probabilities to ``(rho, on, H, further statistics, back)`` -- ``on``: the
    row samples at all; ``back(c)`` turns the gated ``c`` into ``(dy, further term columns)``.  The forward is ``MLPPolicy._softmax``,
    the sampling launch's own, so the ratio of an un-updated policy is exactly 1.0."""
    policy_head, other, sampling, reads = "discrete", "ppo_grad_gaussian", Sampling, "temperature"
    taken, taken_dtype, taken_columns, old = "actions", torch.uint8, False, "old_probs"
    extra, n_stats = {}, 4
    struct, fields, symbol = _lib.PolicyGrad, ("action_id", "old_prob"), "mgx_policy_grad"

    @staticmethod
    def sample(me, y, actions, old_probs, sampling, K, ent_coef):
        n = y.shape[0]
        e, d, S, _, samp, beta = me._softmax(y, sampling, K)
        zero, one = torch.zeros_like(S), torch.ones_like(S)
        b = torch.where(samp, beta, zero)
        a = actions.reshape(n).long()
        e_a = zero
        for o in range(me.n_out):
            e_a = torch.where(a == o, e[o], e_a)
        lnS = policy_log(S)
        pi, logpi, Hs = [], [], zero
        for o in range(me.n_out):
            pi.append(e[o] / S)
            logpi.append(d[o] - lnS)
            Hs = torch.where(e[o] > 0, Hs + pi[o] * logpi[o], Hs)
        H = -Hs

        def back(c):
            dy = []
            for o in range(me.n_out):
                t = torch.where(e[o] > 0, pi[o] * (logpi[o] + H), zero)
                v = b * (c * ((a == o).to(torch.float64) - pi[o]) + ent_coef * t)
                dy.append(torch.where(samp, v, zero))
            return torch.stack(dy, dim=1), []
        return torch.where(samp, e_a / S, one) / old_probs.reshape(n), samp, torch.where(samp, H, zero), [], back


class _GaussianGrad:
    """... and the Gaussian head of the continuous one (``PgHead<PG_HEAD_GAUSSIAN>``): from ``y``, the pre-clip actions and their old
    log-densities; ``on``: a column is live; the further statistic is ``kl``, the further term columns ``dls`` [n, 4] of ``log
    sigma``.  The constants are ``MLPPolicy._gaussian_consts``, the Gaussian launch's own."""
    policy_head, other, sampling, reads = "continuous", "ppo_grad", GaussianSampling, "sigma"
    taken, taken_dtype, taken_columns, old = "raw_actions", torch.float64, True, "old_logp"
    extra, n_stats = {"log_sigma": (MAX_CONTROLS,)}, 5
    struct, fields, symbol = _lib.PolicyGradGaussian, ("raw_action", "old_logp"), "mgx_policy_grad_gaussian"

    @staticmethod
    def sample(me, y, raw_actions, old_logp, sampling, K, ent_coef):
        n, nA = y.shape[0], me.n_out
        _, lv, sd, L, Cn = me._gaussian_consts(sampling, n, y.device, K)
        zero = torch.zeros_like(Cn)
        Hc, anyl = zero, torch.zeros(n, dtype=torch.bool, device=y.device)
        for o in range(nA):
            Hc = torch.where(lv[o], Hc + (L[o] + ENTROPY_CONST), Hc)
            anyl = anyl | lv[o]
        raw = raw_actions.reshape(n, nA)
        zeta, Q = [], zero
        for o in range(nA):
            zeta.append((raw[:, o] - y[:, o]) / sd[o])
            Q = torch.where(lv[o], Q + zeta[o] * zeta[o], Q)
        logp = (-0.5 * Q) - Cn
        Dl = logp - old_logp.reshape(n)
        nan = Dl != Dl
        Dz = torch.where(nan, zero, Dl)
        down = Dz <= 0
        m = torch.where(down, Dz, -Dz)
        E = policy_exp(torch.where(m < EXP_MIN, torch.full_like(m, EXP_MIN), m))
        rho = torch.where(nan, torch.full_like(E, float("nan")), torch.where(down, E, 1.0 / E))

        def back(c):
            dy = torch.stack([torch.where(lv[o], c * (zeta[o] / sd[o]), zero) for o in range(nA)], dim=1)
            dls = torch.stack([torch.where(lv[o], (c * (zeta[o] * zeta[o] - 1.0)) - ent_coef, zero) if o < nA else zero
                               for o in range(MAX_CONTROLS)], dim=1)
            return dy, [dls]
        return rho, anyl, Hc, [torch.where(anyl, (rho - 1.0) - Dl, zero)], back


def _ppo_grad_host(head, policy, critic, rows, taken, old, advantages, returns, sampling, clip, vf_coef, ent_coef, mask, ratio, per_sample):
    """The host gradient rule, stated once for both heads (``head``: ``_SoftmaxGrad`` or ``_GaussianGrad``): the trunk, the head's
    ``rho``, the clip gate, the critic's term, the back-propagation into the trunk, the term columns in the order of ``ppo_grad_flat``,
    the mask and the mean over the live samples."""
    K, N, clip, vf_coef, ent_coef = _ppo_checks(head, policy, critic, rows, taken, old, advantages, returns, sampling, clip, vf_coef,
                                                ent_coef, mask)
    dev = rows.device
    me = policy.to(dev)
    n = K * N
    x = rows.reshape(n, me.n_in).to(torch.float64)
    h, y = me._trunk(x, None)
    zero = torch.zeros(n, dtype=torch.float64, device=dev)
    rho, on, H, more_stats, back = head.sample(me, y, taken, old, sampling, K, ent_coef)
    A = advantages.reshape(n)
    hi, lo = 1.0 + clip, 1.0 - clip
    active = ~(((A > 0) & (rho > hi)) | ((A < 0) & (rho < lo)))
    c = torch.where(on & active, -(A * rho), zero)
    pl = torch.where(on, torch.where(active, c, -(A * torch.where(A > 0, zero + hi, zero + lo))), zero)
    dy, more_cols = back(c)
    dv = vl = None
    if critic is not None:
        diff = critic._on(h, None) - returns.reshape(n)
        dv, vl = vf_coef * diff, 0.5 * (diff * diff)
    cols = []
    if me.n_hidden:
        q = torch.zeros_like(h)
        for o in range(me.n_out):
            q = q + me.W2[0][o].unsqueeze(0) * dy[:, o:o + 1]
        if critic is not None:
            q = q + critic.w.to(dev)[0].unsqueeze(0) * dv.unsqueeze(1)
        dh = torch.where(h > 0, q, torch.zeros_like(q))
        cols += [(dh.unsqueeze(2) * x.unsqueeze(1)).reshape(n, -1), dh]
    cols += [(dy.unsqueeze(2) * h.unsqueeze(1)).reshape(n, -1), dy]
    if critic is not None:
        cols += [dv.unsqueeze(1) * h, dv.unsqueeze(1)]
    terms = torch.cat(cols + more_cols, dim=1)
    st = torch.stack([pl, vl if vl is not None else zero, H, (on & ~active).to(torch.float64)] + more_stats, dim=1)
    if mask is not None:
        keep = mask.reshape(n) != 0
        terms, st = terms[keep], st[keep]
    M = terms.shape[0]
    inv = 1.0 / M if M else 0.0
    res = _ppo_result(inv * terms.sum(dim=0), inv * st.sum(dim=0), _ppo_shapes(head, me, critic))
    if ratio:
        res["ratio"] = rho.reshape(K, N)
    if per_sample:
        res["terms"], res["stat_terms"] = terms, st
    return res


def ppo_grad_host(policy, critic, rows, actions, old_probs, advantages, returns=None, sampling=None, clip=0.2, vf_coef=0.5, ent_coef=0.0,
                  mask=None, ratio=False, per_sample=False):
    """The rule of ``mgx_policy_grad`` (include/mgx.h) in torch, on any device, operation by operation: the gradient of
    ``mean(policy loss) + vf_coef * mean(value loss) - ent_coef * mean(entropy)`` over the live samples with respect to the
    parameters, ``{"W1", "b1", "W2", "b2", "w", "b", "stats"[, "ratio"]}`` (``W1`` / ``b1`` None for a linear policy, ``w`` / ``b`` None
    without a critic; ``stats``: the means of policy loss, value loss, entropy, clipped fraction).  Per sample every operation is the
    device's; the sum over the samples is torch's (the device's goes through the matrix cores: the two agree within the any-order
    summation bound, and exactly for one live sample).  ``per_sample=True`` adds ``"terms"`` ``[M, P]``, the unreduced terms of the M
    live samples in the column order of ``ppo_grad_flat``, and ``"stat_terms"`` ``[M, 4]``."""
    return _ppo_grad_host(_SoftmaxGrad, policy, critic, rows, actions, old_probs, advantages, returns, sampling, clip, vf_coef, ent_coef,
                          mask, ratio, per_sample)


def ppo_grad_gaussian_host(policy, critic, rows, raw_actions, old_logp, advantages, returns=None, sampling=None, clip=0.2, vf_coef=0.5,
                           ent_coef=0.0, mask=None, ratio=False, per_sample=False):
    """The rule of ``mgx_policy_grad_gaussian`` (include/mgx.h) in torch, on any device, operation by operation: ``ppo_grad_host`` for the
    Gaussian head of a continuous ``MLPPolicy`` -- the gradient of ``mean(policy loss) + vf_coef * mean(value loss) - ent_coef *
    mean(entropy)`` with respect to the parameters and to ``log sigma``, ``{"W1", "b1", "W2", "b2", "w", "b", "log_sigma", "stats"[,
    "ratio"]}``: ``log_sigma`` ``[4]`` (0.0 past ``n_out`` and on a column with sigma 0), ``stats`` ``[5]``: the means of policy loss,
    value loss, entropy, clipped fraction and ``kl = (rho - 1) - (logp - old_logp)``.  ``per_sample=True`` adds ``"terms"`` ``[M, P]`` in
    the column order of ``ppo_grad_flat`` and ``"stat_terms"`` ``[M, 5]``."""
    return _ppo_grad_host(_GaussianGrad, policy, critic, rows, raw_actions, old_logp, advantages, returns, sampling, clip, vf_coef,
                          ent_coef, mask, ratio, per_sample)


def _ppo_outputs(shapes, out, dev, masked):
    """The output tensors of a device gradient call: the caller's (``out``) where given and fitting, fresh ones elsewhere."""
    out = out or {}
    unknown = set(out) - set(shapes)
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    res = {}
    for name, shape in shapes.items():
        t = out.get(name)
        if shape is None:
            if t is not None:
                raise ValueError(f"out[{name!r}] given, but this call has no such output")
            if name != "ratio":
                res[name] = None
            continue
        if t is None:                                      # (a masked sample's ratio is not written: NaN there)
            t = torch.full(shape, float("nan"), dtype=torch.float64, device=dev) if name == "ratio" and masked else \
                torch.empty(shape, dtype=torch.float64, device=dev)
        elif not torch.is_tensor(t) or t.dtype != torch.float64 or t.device != dev or not t.is_contiguous() or t.numel() != int(np.prod(shape)):
            raise ValueError(f"out[{name!r}] must be a contiguous float64 tensor of {list(shape)} on {dev}")
        res[name] = t
    return res


def _ppo_grad_device(head, fn, policy, critic, rows, taken, old, advantages, returns, sampling, clip, vf_coef, ent_coef, mask, ratio, out):
    """The device call of ``fn`` (``ppo_grad`` / ``ppo_grad_gaussian``), stated once: ``head`` names the struct, its two fields for the
    action taken and the old density, the gradients and statistics beyond the common ones, and the symbol."""
    K, N, clip, vf_coef, ent_coef = _ppo_checks(head, policy, critic, rows, taken, old, advantages, returns, sampling, clip, vf_coef,
                                                ent_coef, mask)
    dev = rows.device
    if dev.type != "cuda":
        raise ValueError(f"{fn} runs on the GPU ({head.symbol}); the tensors lie on {dev} -- {fn}_host states the same rule anywhere")
    for name, t in (("rows", rows), (head.taken, taken), (head.old, old), ("advantages", advantages), ("returns", returns), ("mask", mask)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    shapes = {**_ppo_shapes(head, policy, critic), "stats": (head.n_stats,), "ratio": (K, N) if ratio else None}
    res = _ppo_outputs(shapes, out, dev, mask is not None)
    lib = _lib.lib()
    ptr = lambda t: None if t is None else t.data_ptr()     # noqa: E731
    with torch.cuda.device(dev):
        pol, keep_p = policy.c_struct(dev, N)
        smp, keep_s = sampling.c_struct(dev, N)
        cr, keep_c = critic.c_struct(dev, N) if critic is not None else (None, None)
        need = C.c_int64()
        _lib.check(lib.mgx_policy_grad_workspace(N, K, C.byref(pol), C.byref(need)))
        ws = torch.empty((need.value + 7) // 8, dtype=torch.float64, device=dev)
        m8 = mask.view(torch.uint8) if mask is not None and mask.dtype == torch.bool else mask
        pg = head.struct()
        pg.struct_size = C.sizeof(head.struct)
        pg.x_f32 = int(rows.dtype == torch.float32)
        pg.x, pg.advantage, pg.returns, pg.mask = ptr(rows), ptr(advantages), ptr(returns), ptr(m8)
        for field, t in zip(head.fields, (taken, old)):
            setattr(pg, field, ptr(t))
        pg.clip_eps, pg.vf_coef, pg.ent_coef = clip, vf_coef, ent_coef
        pg.g_w1, pg.g_b1, pg.g_w2, pg.g_b2 = ptr(res["W1"]), ptr(res["b1"]), ptr(res["W2"]), ptr(res["b2"])
        pg.g_cw, pg.g_cb, pg.stats, pg.ratio_out = ptr(res["w"]), ptr(res["b"]), ptr(res["stats"]), ptr(res.get("ratio"))
        for name in head.extra:
            setattr(pg, "g_" + name, ptr(res[name]))
        pg.workspace, pg.workspace_bytes = ws.data_ptr(), ws.numel() * 8
        _lib.check(getattr(lib, head.symbol)(N, K, C.byref(pol), C.byref(cr) if cr is not None else None, C.byref(smp), C.byref(pg),
                                             torch.cuda.current_stream(dev).cuda_stream))
    return res


def ppo_grad(policy, critic, rows, actions, old_probs, advantages, returns=None, sampling=None, clip=0.2, vf_coef=0.5, ent_coef=0.0,
             mask=None, ratio=False, out=None):
    """The gradient of the PPO-clip loss (``clip=float("inf")``: A2C, the unclipped surrogate) of a discrete ``MLPPolicy`` and the
    ``ValueHead`` on its trunk over the ``[K, N]`` samples of a collection, on the device (``mgx_policy_grad``: one kernel over the
    samples, the sum on the matrix cores, and a small one that adds the partials in a fixed order): ``ppo_grad_host``'s values, exactly
    for one live sample and within the any-order summation bound for many, identical from run to run.  The forward pass is the
    sampling launch's own, so with the parameters that collected the data ``ratio`` is exactly 1.0.

    ``rows`` ``[K, N, n_in]`` float64 or float32 (``decision_rows``), ``actions`` uint8, ``old_probs`` / ``advantages`` / ``returns``
    float64 ``[K, N]`` (``out["action_ids"]``, ``out["probs"]`` of ``rollout_policy`` and ``gae``'s results), ``sampling`` the launch's
    ``Sampling``, ``mask`` uint8 or bool ``[K, N]`` (0: the sample contributes nothing -- minibatches).  Returns ``{"W1", "b1", "W2",
    "b2", "w", "b", "stats"[, "ratio"]}``: tensors shaped like the parameters without the population axis (None where there is none),
    ``stats`` = the means of policy loss, value loss, entropy, clipped fraction.  ``out``: a dict with your own contiguous float64
    tensors for any of them (e.g. the ``.grad`` of the parameters).  Contiguous device tensors only."""
    return _ppo_grad_device(_SoftmaxGrad, "ppo_grad", policy, critic, rows, actions, old_probs, advantages, returns, sampling, clip,
                            vf_coef, ent_coef, mask, ratio, out)


def ppo_grad_gaussian(policy, critic, rows, raw_actions, old_logp, advantages, returns=None, sampling=None, clip=0.2, vf_coef=0.5,
                      ent_coef=0.0, mask=None, ratio=False, out=None):
    """``ppo_grad`` for the Gaussian head: the gradient of the PPO-clip loss (``clip=float("inf")``: A2C) of a continuous ``MLPPolicy``,
    the ``ValueHead`` on its trunk and ``log sigma`` over the ``[K, N]`` samples of a collection, on the device
    (``mgx_policy_grad_gaussian``: the kernels of ``ppo_grad`` with the Gaussian head) -- ``ppo_grad_gaussian_host``'s values, exactly
    for one live sample and within the any-order summation bound for many, identical from run to run.

    ``rows`` ``[K, N, n_in]`` float64 or float32 (``decision_rows``), ``raw_actions`` float64 ``[K, N, n_out]`` and ``old_logp`` float64
    ``[K, N]`` (``out["raw_actions"]``, ``out["logp"]`` of ``step_k_policy``), ``advantages`` / ``returns`` as ``gae`` made them,
    ``sampling`` the launch's ``GaussianSampling`` (sigma and scale are read).  Returns what ``ppo_grad`` returns plus ``"log_sigma"``
    ``[4]``, the gradient with respect to ``log sigma[o]`` (0.0 past ``n_out`` and where sigma is 0), with ``stats`` ``[5]``: policy
    loss, value loss, entropy, clipped fraction, ``kl``.  Who learns sigma keeps a ``log_sigma`` tensor, steps it with this gradient
    and builds the next ``GaussianSampling`` from ``log_sigma.exp().tolist()``.  With the parameters that collected the data ``ratio``
    is 1.0 up to the rounding of ``raw = y + s * z`` (the bound: include/mgx.h), not exactly."""
    return _ppo_grad_device(_GaussianGrad, "ppo_grad_gaussian", policy, critic, rows, raw_actions, old_logp, advantages, returns, sampling,
                            clip, vf_coef, ent_coef, mask, ratio, out)
