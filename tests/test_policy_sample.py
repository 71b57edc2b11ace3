"""Softmax sampling inside the fused closed-loop discrete roll-out (mgx_rollout_policy_sample_episodes, ``sampling=`` / ``probs=`` of
StepEngine.rollout_policy_episodes and PerGridWindowEnv.rollout_policy): the rule of ``mgx_sampling`` (include/mgx.h) on the host
(``policy_exp``, ``MLPPolicy.act(obs, sampling, counter, return_prob=True)``) and K steps in one launch == a twin stepped K times
with it, bit for bit (torch.equal: exp is a fixed sequence of IEEE operations on both sides, the draws are integer Philox words, the
probability one IEEE division, so there is no tolerance).  The forms of the kernels these cases leave out -- all ten layouts x the three row sources -- run in
tests/test_layout_matrix_policy.py, which also replays the launches on the CPU oracle."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from test_episode_rows import HostStats, _same_bits, _snapshot, _state_equal, _untouched
from test_policy_explore import DOCUMENTED as EXPLORE_DOCUMENTED
from test_policy_explore import _compare, _envs_equal, _forms_of
from test_policy_rollout import DOCUMENTED as GREEDY_DOCUMENTED
from test_policy_rollout import WANT, _batch, _c_policy, _n_out, _policy, _trace_end, _trace_launch, _trace_start

F64, F32 = torch.float64, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, LENGTH = 200, 8760, 24        # three full waves and a last wave of 8 lanes; restarts fall inside a 64-step launch
LAUNCHES = (1, 7, 64)
LN2 = math.log(2.0)


def _sampling(seed=5, **kw):
    from pymgrid_amd import Sampling
    return Sampling(seed, **kw)


def _rows(n, n_in, seed=3):
    return torch.as_tensor(np.random.default_rng(seed).uniform(0.0, 1.0, size=(n, n_in)))


def _fixed_logits(logits, n_in=4):
    """A linear discrete policy whose outputs are ``logits`` at every input (zero weights: y = b2 + 0 * x)."""
    from pymgrid_amd import MLPPolicy
    b2 = np.asarray(logits, dtype=np.float64)
    return MLPPolicy(None, None, np.zeros((len(b2), n_in)), b2, head="discrete")


# ---- CPU: exp as part of the rule --------------------------------------------------------------------------------------------------
def _exp_points():
    """The endpoints, +-0.0, 1e5 seeded uniform points in every band of [-708, 0] (decades up to 100, then [-708, -100]), every
    k * ln 2 and (k - 1/2) * ln 2 (where the reduction changes k) with their neighbours up to 3 ulp away."""
    g = torch.Generator().manual_seed(20)
    edges = [0.0] + [10.0 ** p for p in range(-12, 3)] + [708.0]
    parts = [torch.tensor([0.0, -0.0, -708.0, -1e-300, -5e-324], dtype=F64)]
    for lo, hi in zip(edges[:-1], edges[1:]):
        parts.append(-(lo + (hi - lo) * torch.rand(100_000, generator=g, dtype=F64)))
    k = torch.arange(0, 1022, dtype=F64)
    for centre in (-k * LN2, -(k + 0.5) * LN2):
        near = [centre]
        for _ in range(3):
            near.append(torch.nextafter(near[-1], torch.full_like(centre, -1000.0)))
        lower = centre
        for _ in range(3):
            lower = torch.nextafter(lower, torch.full_like(centre, 1000.0))
            near.append(lower)
        parts.append(torch.cat(near))
    d = torch.cat(parts)
    return d[(d >= -708.0) & (d <= 0.0)]


def test_policy_exp_is_within_an_ulp_monotone_and_never_above_one():
    """Relative error <= 2^-51 against libm (the rule itself stays below 2^-52 of the true value; the bound allows for the
    comparator's own error), exactly 1.0 at +-0.0, never above 1.0, non-decreasing over the sorted sample."""
    from pymgrid_amd.policy import policy_exp
    d = _exp_points()
    assert d.numel() > 1_600_000 and float(d.min()) == -708.0 and float(d.max()) == 0.0
    e, ref = policy_exp(d), torch.exp(d)
    assert e.dtype == F64 and bool((e > 0).all()) and bool((e <= 1.0).all())
    rel = ((e - ref).abs() / ref).max()
    print("policy_exp: worst relative error vs torch.exp", float(rel) * 2.0 ** 52, "x 2^-52 over", d.numel(), "points")
    assert float(rel) <= 2.0 ** -51
    few = torch.cat([d[:5], d[5::1013]])
    ref_m = torch.tensor([math.exp(v) for v in few.tolist()], dtype=F64)
    assert float(((policy_exp(few) - ref_m).abs() / ref_m).max()) <= 2.0 ** -51
    one = policy_exp(torch.tensor([0.0, -0.0], dtype=F64))
    assert one.tolist() == [1.0, 1.0]
    s, _ = d.sort()
    es = policy_exp(s)
    assert bool((es[1:] >= es[:-1]).all())
    assert float(policy_exp(torch.tensor([-708.0], dtype=F64))) > 0.0             # (a normal number: 2^k is built from its bits)


# ---- CPU: the head on the host -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hidden", [0, 16])
def test_temperature_zero_and_zero_scale_are_the_greedy_head(n_hidden):
    n = 600
    obs = _rows(n, 8)
    pol = _policy(7, 8, n_hidden, 6, "discrete")
    greedy = pol.act(obs)
    for t in (0, 19):
        ids, prob = pol.act(obs, _sampling(temperature=0.0), t, return_prob=True)
        assert ids.dtype == torch.int32 and prob.dtype == F64
        assert torch.equal(ids, greedy) and torch.equal(prob, torch.ones(n, dtype=F64))
        assert torch.equal(pol.act(obs, _sampling(temperature=0.0), t), greedy)
    scale = torch.as_tensor(np.where(np.arange(n) % 3 == 0, 0.0, np.linspace(0.5, 2.0, n)))
    zero = scale == 0
    ids, prob = pol.act(obs, _sampling(temperature=1.0, scale=scale), 4, return_prob=True)
    assert torch.equal(ids[zero], greedy[zero]) and torch.equal(prob[zero], torch.ones(int(zero.sum()), dtype=F64))
    assert not torch.equal(ids[~zero], greedy[~zero]) and bool((prob[~zero] < 1.0).all())
    # the ladder multiplies the temperature: grid i samples at temperature scale[i]
    for i in (1, 200, 599):
        one, p1 = pol.act(obs, _sampling(temperature=float(scale[i])), 4, return_prob=True)
        assert int(one[i]) == int(ids[i]) and float(p1[i]) == float(prob[i])
    with pytest.raises(ValueError, match="counter"):
        pol.act(obs, _sampling())
    with pytest.raises(ValueError, match="scale names"):
        pol.act(obs[:10], _sampling(scale=scale), 4)
    with pytest.raises(ValueError, match="discrete"):
        _policy(7, 8, n_hidden, 3, "continuous").act(obs, _sampling(), 4)


def test_the_counter_and_the_seed_move_the_draw_and_the_draw_is_number_one():
    from pymgrid_amd.policy import EXPLORE_TAG, philox_words, uniform53
    n = 4000
    obs = _rows(n, 8)
    pol = _policy(7, 8, 16, 6, "discrete")
    a = pol.act(obs, _sampling(seed=9), 31)
    assert torch.equal(a, pol.act(obs, _sampling(seed=9), 31))
    assert not torch.equal(a, pol.act(obs, _sampling(seed=9), 32)) and not torch.equal(a, pol.act(obs, _sampling(seed=10), 31))
    # the id is the inverse CDF of the weights at u = U(r[0], r[1]) of draw number 1
    e, S, g, live = pol.sample_weights(pol.outputs(obs), _sampling(seed=9))
    r = philox_words(9, torch.arange(n), 31, EXPLORE_TAG + 1)
    v = uniform53(r[0], r[1]) * S
    cdf = torch.zeros(n, dtype=F64)
    want = g.clone()
    done = torch.zeros(n, dtype=torch.bool)
    for o in range(6):
        cdf = cdf + e[:, o]
        hit = ~done & (v < cdf)
        want[hit] = o
        done |= hit
    assert bool(live.all()) and torch.equal(a, want)


@pytest.mark.parametrize("temperature", [0.5, 1.0, 3.0])
def test_the_probability_is_the_weight_of_the_id_over_the_sum(temperature):
    from pymgrid_amd.policy import policy_exp
    n, n_out = 3000, 7
    obs = _rows(n, 8)
    pol = _policy(11, 8, 16, n_out, "discrete")
    ids, prob = pol.act(obs, _sampling(temperature=temperature), 12, return_prob=True)
    assert bool((prob > 0).all()) and bool((prob <= 1.0).all())
    y = pol.outputs(obs)
    g = pol.act(obs)
    best = y.max(dim=1).values
    beta = 1.0 / temperature
    S = torch.zeros(n, dtype=F64)
    cols = []
    for o in range(n_out):
        d = (y[:, o] - best) * beta
        e = torch.where(g == o, torch.ones(n, dtype=F64), policy_exp(d))         # (these logits keep every d far above -708)
        cols.append(e)
        S = S + e
    e = torch.stack(cols, dim=1)
    assert torch.equal(prob, e.gather(1, ids.long()[:, None])[:, 0] / S)
    soft = torch.softmax(y / temperature, dim=1).gather(1, ids.long()[:, None])[:, 0]
    assert float(((prob - soft).abs() / soft).max()) < 1e-13
    assert ids.unique().numel() > 1


def test_an_id_of_weight_zero_is_never_taken():
    n = 100_000
    pol = _fixed_logits([0.0, -1e4, 0.5, -1.0])          # (id 1: 1e4 below the best, d < -708, weight 0)
    obs = _rows(n, 4)
    ids, prob = pol.act(obs, _sampling(seed=3), 7, return_prob=True)
    assert sorted(ids.unique().tolist()) == [0, 2, 3]
    e, S, g, _ = pol.sample_weights(pol.outputs(obs), _sampling(seed=3))
    assert bool((e[:, 1] == 0).all()) and bool((g == 2).all()) and bool((prob > 0).all())


def test_the_corners_nan_inf_and_ties():
    n = 20_000
    obs = _rows(n, 4)
    nan, inf = float("nan"), float("inf")
    ones = torch.ones(n, dtype=F64)

    def run(logits):
        return _fixed_logits(logits).act(obs, _sampling(seed=1), 2, return_prob=True)
    for logits, g in (([nan, nan, nan], 0), ([-inf, -inf, -inf], 0), ([1.0, inf, 2.0], 1), ([nan, -inf, nan], 0), ([0.0, inf, inf], 1)):
        ids, prob = run(logits)                                   # best = +-inf or all NaN: id = g, prob = 1.0 / S = 1.0
        assert bool((ids == g).all()) and torch.equal(prob, ones), logits
    ids, prob = run([0.3, nan, 0.3, -0.2])                        # a NaN weighs nothing; the tie at the maximum shares the mass
    assert sorted(ids.unique().tolist()) == [0, 2, 3]
    w = [1.0, 0.0, 1.0, math.exp(-0.5)]
    share = torch.bincount(ids.long(), minlength=4).double() / n
    for o in range(4):
        p = w[o] / sum(w)
        assert abs(float(share[o]) - p) <= 5 * math.sqrt(p * (1 - p) / n), (o, float(share[o]), p)
    assert bool((prob[ids == 0] == prob[ids == 2][0]).all())      # E(+-0.0) == 1.0: the tied ids weigh the same
    ids, prob = run([-3.25] * 5)                                  # all equal: uniform, every prob exactly 1 / 5
    assert ids.unique().numel() == 5 and torch.equal(prob, torch.full((n,), 1.0 / 5.0, dtype=F64))


@pytest.mark.parametrize("temperature", [0.5, 1.0, 2.0])
def test_the_ids_follow_the_softmax(temperature):
    """200 000 grids at one counter: every empirical frequency within 5 sqrt(p (1 - p) / n) of softmax(y / tau) (five standard
    deviations of a binomial share: a bound from the distribution itself, not from what the code returned)."""
    n = 200_000
    logits = [0.3, -1.2, 2.0, 0.9, -0.4]
    pol = _fixed_logits(logits)
    ids, prob = pol.act(_rows(n, 4), _sampling(seed=17, temperature=temperature), 5, return_prob=True)
    p = torch.softmax(torch.tensor(logits, dtype=F64) / temperature, dim=0)
    share = torch.bincount(ids.long(), minlength=5).double() / n
    for o in range(5):
        po = float(p[o])
        assert abs(float(share[o]) - po) <= 5 * math.sqrt(po * (1 - po) / n), (o, float(share[o]), po)
        assert float((prob[ids == o] - po).abs().max()) < 1e-14


# ---- CPU: validation, layout, the C entry ----------------------------------------------------------------------------------------
def test_validation_errors():
    for bad in (dict(temperature=-0.1), dict(temperature=float("inf")), dict(temperature=float("nan")),
                dict(scale=np.zeros(4, dtype=np.float32)), dict(scale=np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            _sampling(**bad)
    for seed in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            _sampling(seed=seed)
    sa = _sampling(seed=2 ** 64 - 1, temperature=0.25)
    st, _ = sa.c_struct(torch.device("cpu"), 4)
    assert st.struct_size == C.sizeof(type(st)) and st.seed == 2 ** 64 - 1 and st.temperature == 0.25 and not st.scale
    assert _sampling().temperature == 1.0
    pol = _policy(7, 8, 0, 6, "discrete")
    with pytest.raises(ValueError, match="return_prob"):
        pol.act(_rows(4, 8), None, None, return_prob=True)


class _NoLaunch:
    """An engine stand-in for the checks StepEngine.rollout_policy_episodes makes before it touches a handle."""
    N, device = 4, torch.device("cpu")


def test_sampling_with_exploration_raises():
    from pymgrid_amd import Exploration
    from pymgrid_amd.engine import StepEngine
    from pymgrid_amd.hetero import PerGridWindowEnv
    import inspect
    pol = _policy(7, 8, 0, 6, "discrete")
    with pytest.raises(ValueError, match="exclude each other"):
        StepEngine._launch_policy_episodes(_NoLaunch(), "mgx_rollout_policy_episodes", pol, Exploration(1, epsilon=0.1), (), 4, {}, (),
                                           None, None, {}, False, False, sampling=_sampling(), probs=None)
    for fn in (StepEngine.rollout_policy_episodes, PerGridWindowEnv.rollout_policy):
        par = inspect.signature(fn).parameters
        assert par["sampling"].default is None and par["probs"].default is False
    assert "sampling" in inspect.signature(PerGridWindowEnv.step_k_policy).parameters
    assert "sampling" not in inspect.signature(StepEngine.step_k_policy_episodes).parameters


def test_symbol_struct_and_header():
    from pymgrid_amd import Sampling, _lib, policy
    assert Sampling is policy.Sampling
    _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "mgx.h")) as fh:
        header = fh.read()
    name = "mgx_rollout_policy_sample_episodes"
    assert name in _lib.SYMBOLS and getattr(L, name) is not None and f"int {name}(" in header
    assert "typedef struct mgx_sampling" in header and "0xE9100000u + 1" in header
    assert _lib.lib().mgx_abi_minor() == 3 == _lib.ABI_MINOR
    assert C.sizeof(_lib.Policy) == 24 + 5 * C.sizeof(C.c_void_p) and C.sizeof(_lib.Exploration) == 64    # (both keep their sizes)
    fields = re.search(r"typedef struct mgx_sampling \{(.*?)\} mgx_sampling;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert re.findall(r"([a-z_]+);", fields) == [n for n, _ in _lib.Sampling._fields_]
    assert re.findall(r"(\w+) \*?[a-z_]+;", fields) == ["int32_t", "int32_t", "uint64_t", "double", "double"]
    assert C.sizeof(_lib.Sampling) == 4 + 4 + 8 + 8 + C.sizeof(C.c_void_p) == 32
    assert _lib.Sampling.seed.offset == 8 and _lib.Sampling.temperature.offset == 16 and _lib.Sampling.scale.offset == 24
    # the coefficients of the rule, as the header writes them, are the doubles nearest 1 / n!
    from fractions import Fraction
    assert len(policy.EXP_COEFFS) == 14
    for k, c in enumerate(policy.EXP_COEFFS):
        exact = Fraction(1, math.factorial(k))
        assert c == exact.numerator / exact.denominator and (repr(c) in header or c in (1.0, 0.5)), k
    lib = _lib.lib()
    x = _lib.Sampling()
    assert lib.mgx_rollout_policy_sample_episodes(None, None, C.byref(x), None, 0, 4, None, None, None, None, None, None, None, None,
                                                  None) == _lib.MGX_ERR_INVALID
    assert b"mgx_rollout_policy_sample_episodes" in lib.mgx_last_error()


SAMPLE = 2      # PolicyHead (csrc/mgx_policy.hpp)
DOCUMENTED = {   # (kernel, head): (forms, most AGPRs, most spilled SGPRs, least occupancy in waves per SIMD) -- the figures of DESIGN.md
    ("rollout_policy_head_episodes_kernel", SAMPLE): (30, 52, 41, 1),
}


def test_the_sampling_kernel_uses_what_design_md_says():
    """The 30 forms of the sampling head (ten layouts x three row sources): no scratch memory, no vector register spilled, LDS within the siblings'
    bound; AGPRs, spilled SGPRs and occupancy no worse than DESIGN.md's kernel table records them.  The greedy and exploring
    kernels keep the figures their own tests record."""
    from pymgrid_amd import _lib
    _lib.build()
    usage = _lib.resource_usage()
    if usage is None:
        pytest.skip("libmgx.so was not built on this machine (no resource_usage.json beside the objects)")
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        design = fh.read()

    def forms_of(kernel):
        return _forms_of(usage, kernel)
    for kernel, (n_forms, agpr, sgpr_spill, occupancy) in DOCUMENTED.items():
        assert f"`{kernel[0]}<7,4,0,{kernel[1]}>`" in design
        forms = forms_of(kernel)
        assert len(forms) == n_forms, (kernel, sorted(forms))
        for name, u in forms.items():
            assert u["scratch"] == 0 and u["vgpr_spill"] == 0, (name, u)
            assert u["vgpr"] <= 256 and u["agpr"] <= agpr and u["vgpr"] + u["agpr"] <= 512, (name, u)
            assert u["sgpr_spill"] <= sgpr_spill and u["occupancy"] >= occupancy, (name, u)
            assert u["lds"] <= 24576 + 64, (name, u)
    for kernel, (n_forms, agpr, sgpr_spill, occupancy) in {**GREEDY_DOCUMENTED, **EXPLORE_DOCUMENTED}.items():
        forms = forms_of(kernel)                                  # the siblings: exactly their recorded extremes
        assert len(forms) == n_forms, (kernel, sorted(forms))
        assert max(u["agpr"] for u in forms.values()) == agpr and max(u["sgpr_spill"] for u in forms.values()) == sgpr_spill, kernel
        assert min(u["occupancy"] for u in forms.values()) == occupancy, kernel
        assert all(u["scratch"] == 0 and u["vgpr_spill"] == 0 for u in forms.values()), kernel


# ---- GPU: fused == stepped ---------------------------------------------------------------------------------------------------------
def _envs(device, arch, series, obs_dtype, count, twin=1, n=N, length=LENGTH, t=T):
    """``count`` discrete PerGridWindowEnv of the same batch, seed and first draw; number ``twin`` (the stepped one; None: none)
    reports the rows before the restarts."""
    from pymgrid_amd.hetero import PerGridWindowEnv
    kw = dict(trajectory_length=length, discrete=True, auto_reset=True, seed=23, obs_dtype=obs_dtype)
    envs = [PerGridWindowEnv(_batch(device, arch, series, n, t=t), final_observation=(q == twin), **kw) for q in range(count)]
    for e in envs:
        torch.manual_seed(41)                   # the same first draw
        e.obs0 = e.reset()
    return envs


def _spread_policy(seed, obs0, n_hidden, n_out, P=1, index=None):
    """``_policy(...)`` with its output layer divided by one factor, found by bisection on the rows the envs start from, so that the
    greedy id holds on average the share 1 - 0.7 (1 - 1 / n_out) of torch.softmax: at temperature 1 a sampled id then differs
    from the greedy one at roughly 0.7 (1 - 1 / n_out) of the (step, grid) pairs -- 35 % over two ids, 64 % over twelve -- and every
    id carries mass.  (The raw logits of _policy favour one id so much on some tables that sampling would rarely leave it.)"""
    from pymgrid_amd import MLPPolicy
    raw = _policy(seed, obs0.shape[1], n_hidden, n_out, "discrete", P=P, index=index)
    y = raw.outputs(obs0)
    target = 1.0 - 0.7 * (1.0 - 1.0 / n_out)
    lo, hi = -10.0, 10.0                         # log2 of the factor: the greedy share falls as the factor grows
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        share = float(torch.softmax(y / 2.0 ** mid, dim=1).max(dim=1).values.mean())
        lo, hi = (mid, hi) if share > target else (lo, mid)
    f = 2.0 ** (0.5 * (lo + hi))
    return MLPPolicy(raw.W1, raw.b1, raw.W2 / f, raw.b2 / f, policy_index=raw.policy_index, head="discrete")


def _twin_steps(twin, policy, sa, obs, K, hs, seen=None, walked=None):
    """K times ``a, p = policy.act(obs, sa, counter, return_prob=True); obs, r, done, info = twin.step(a)``, the counter read from the
    env before the step; ``seen`` receives the greedy id beside every id taken, ``walked`` every grid's series row before each step."""
    rows = {k: [] for k in ("reward", "done", "soc_trace", "status_trace", "actions", "probs", "obs", "final_obs")}
    cols = twin.env.batch.cols
    for _ in range(K):
        if walked is not None:
            walked.append(twin.env.current_steps.clone())
        t = twin.env.current_step
        assert isinstance(t, int)
        a, p = policy.act(obs, sa, counter=t, return_prob=True)
        if seen is not None:
            seen.append((a.clone(), policy.act(obs)))
        obs, r, d, info = twin.step(a)
        rows["actions"].append(a.to(torch.uint8)); rows["probs"].append(p.clone())
        rows["reward"].append(r.clone()); rows["done"].append(d.clone()); rows["obs"].append(obs.clone())
        fo = info["final_observation"]
        rows["final_obs"].append(torch.where(d[:, None], fo, torch.full_like(fo, float("nan"))))
        if "soc" in cols:
            rows["soc_trace"].append(cols["soc"].clone())
        if "gen_status" in cols:
            rows["status_trace"].append(cols["gen_status"].clone().view(torch.int32))
        hs.add(r, d)
    return {k: torch.stack(v) for k, v in rows.items() if v}, obs


def _nan_rows(K, n, D, dtype, device):
    return dict(final_obs=torch.full((K, n, D), float("nan"), dtype=dtype, device=device))


def _fused_equals_stepped(device, arch, series, n_hidden, obs_dtype=F64, P=1, temperature=1.0, vacuous=True, n=N, length=LENGTH,
                          t=T, launches=LAUNCHES, trace=None):
    """The sampling launch, in launches of 1, 7 and 64 steps on one env, == its stepped twin after every launch -- traces, ids,
    probs, rows, state, episode arrays, statistics; then one more single step.  ``vacuous``: the conditions on the test itself,
    from the stepped twin alone.  ``n``, ``length``, ``t``, ``launches``: another batch size, episode length, series length and
    other launches; ``trace``: a dict that receives what test_policy_rollout._trace_launch records."""
    from pymgrid_amd import _lib
    old = _lib.get_tunable("grid_major_copy")[0]
    if series == "gather":
        _lib.set_tunable("grid_major_copy", 0)
    try:
        fused, twin = _envs(device, arch, series, obs_dtype, 2, n=n, length=length, t=t)
        assert torch.equal(fused.obs0, twin.obs0) and fused.obs0.dtype == obs_dtype
        D, n_out = fused.env.engine.obs_dim, _n_out(fused, True)
        index = None
        if P > 1:
            index = torch.randint(-1, P + 1, (n,), generator=torch.Generator().manual_seed(11)).to(torch.int32)
        policy = _spread_policy(7, twin.obs0, n_hidden, n_out, P=P, index=index)
        sa = _sampling(seed=23, temperature=temperature)              # (the auto-reset seed of the envs: the tag separates the streams)
        hs = HostStats(n, device)
        obs, seen = twin.obs0, []
        _trace_start(trace, fused, True)
        for K in launches:
            out = fused.rollout_policy(policy, K, sampling=sa, probs=True, out=_nan_rows(K, n, D, obs_dtype, device), **WANT)
            walked = [] if trace is not None else None
            ref, obs = _twin_steps(twin, policy, sa, obs, K, hs, seen, walked)
            _trace_launch(trace, walked, out, ref)
            assert out["probs"].dtype == F64 and out["probs"].shape == (K, n)
            _compare(out, ref, K)
            d = out["done"]
            assert bool(torch.isnan(out["final_obs"][~d]).all()) and not bool(torch.isnan(out["final_obs"][d]).any()), K
            _envs_equal(fused, twin, K)
            hs.check(fused.episode_stats)
            if K == 64:
                assert int(ref["done"].sum()) >= 1                     # a grid restarts inside the 64-step launch
        _trace_end(trace, fused)
        if trace is not None:
            trace["greedy"] = torch.stack([g for _, g in seen])
        if vacuous:                                                    # the stepped twin ALONE says whether the test can pass vacuously
            taken, greedy = torch.stack([a for a, _ in seen]), torch.stack([g for _, g in seen])
            share = float((taken != greedy).double().mean())
            print(f"layout {arch}, {series}, {n_hidden} hidden, P = {P}: {n_out} ids, non-greedy share {share:.3f}, ids taken "
                  f"{taken.unique().tolist()}")
            assert 0.2 <= share <= 0.8, share
            assert taken.unique().numel() == n_out, taken.unique().tolist()
        # the env stands where the twin stands: one more single step
        a = policy.act(obs, sa, counter=twin.env.current_step)
        assert torch.equal(a, policy.act(out["obs"][-1], sa, counter=fused.env.current_step))
        (o1, r1, d1, _), (o2, r2, d2, _) = fused.step(a), twin.step(a)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
        _state_equal(fused.env, twin.env)
        fused.env.close(); twin.env.close()
    finally:
        _lib.set_tunable("grid_major_copy", old)


ARCHS = ["genset+battery+grid", "genset+battery", 5]           # layouts 7, 3 and 5 (genset + grid: no battery)
SERIES = ["factorised", "materialised", "gather"]
# arch x series crossed; hidden units (0 / 16) and the row format rotate so that every arch and every source sees both of each
CASES = [(arch, series, (0, 16)[(ai + si) % 2], (F64, F32)[(ai + 2 * si) % 3 % 2])
         for ai, arch in enumerate(ARCHS) for si, series in enumerate(SERIES)]


def test_the_cases_cover_every_source_width_and_format():
    assert {c[0] for c in CASES} == set(ARCHS) and {c[1] for c in CASES} == set(SERIES)
    for key in (0, 1):
        for v in {c[key] for c in CASES}:
            mine = [c for c in CASES if c[key] == v]
            assert {c[2] for c in mine} == {0, 16} and {c[3] for c in mine} == {F64, F32}, (v, mine)


@pytest.mark.gpu
@pytest.mark.parametrize("arch,series,n_hidden,obs_dtype", CASES)
def test_fused_equals_stepped(arch, series, n_hidden, obs_dtype, device):
    _fused_equals_stepped(device, arch, series, n_hidden, obs_dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("n_hidden", [0, 16])
def test_a_population_samples_per_grid(n_hidden, device):
    """P = 3 parameter sets with a policy_index (indices outside the population among them: set 0)."""
    _fused_equals_stepped(device, "genset+battery+grid", "factorised", n_hidden, P=3)


@pytest.mark.gpu
@pytest.mark.parametrize("temperature", [0.25, 4.0])
def test_other_temperatures(temperature, device):
    _fused_equals_stepped(device, "genset+battery+grid", "materialised", 16, temperature=temperature, vacuous=False)


@pytest.mark.gpu
def test_a_temperature_ladder_with_zeros(device):
    """A scale with zeros on every third grid: those grids take the greedy launch's ids with probability 1.0 -- and everything else
    of the greedy launch, a grid's episodes depending on its own ids alone; the others differ."""
    K = 64
    fused, twin, greedy = _envs(device, "genset+battery+grid", "factorised", F64, 3)
    D = fused.env.engine.obs_dim
    policy = _spread_policy(7, twin.obs0, 16, _n_out(fused, True))
    ladder = torch.as_tensor(np.where(np.arange(N) % 3 == 0, 0.0, np.linspace(0.5, 2.0, N))).to(device)
    zero = ladder == 0
    sa = _sampling(seed=99, temperature=1.5, scale=ladder)
    out = fused.rollout_policy(policy, K, sampling=sa, probs=True, out=_nan_rows(K, N, D, F64, device), **WANT)
    hs = HostStats(N, device)
    ref, _ = _twin_steps(twin, policy, sa, twin.obs0, K, hs)
    _compare(out, ref, K)
    _envs_equal(fused, twin, K)
    hs.check(fused.episode_stats)
    plain = greedy.rollout_policy(policy, K, out=_nan_rows(K, N, D, F64, device), **WANT)
    assert torch.equal(out["probs"][:, zero], torch.ones(K, int(zero.sum()), dtype=F64, device=device))
    assert bool((out["probs"][:, ~zero] < 1.0).any()) and bool((out["probs"] > 0).all()) and bool((out["probs"] <= 1.0).all())
    same = lambda a, b: _same_bits(a, b) if a.is_floating_point() else torch.equal(a, b)     # noqa: E731  (final_obs keeps its NaN)
    for name in plain:
        assert same(out[name][:, zero], plain[name][:, zero]), name
    assert not torch.equal(out["actions"][:, ~zero], plain["actions"][:, ~zero])
    assert not torch.equal(out["reward"][:, ~zero], plain["reward"][:, ~zero])
    for e in (fused, twin, greedy):
        e.env.close()


@pytest.mark.gpu
def test_cuts_and_replay(device):
    """The draws do not depend on how a roll-out is cut: 64 steps as 1 + 7 + 56 == the single launch.  And the open-loop rollout
    replays the ids taken: everything but the ids and probs."""
    K, cuts = 64, (1, 7, 56)
    one, cut, replay = _envs(device, "genset+battery+grid", "gather", F64, 3, twin=None)
    D = one.env.engine.obs_dim
    policy = _spread_policy(7, one.obs0, 16, _n_out(one, True))
    sa = _sampling(seed=4, temperature=0.8)
    out = one.rollout_policy(policy, K, sampling=sa, probs=True, out=_nan_rows(K, N, D, F64, device), **WANT)
    parts = [cut.rollout_policy(policy, k, sampling=sa, probs=True, out=_nan_rows(k, N, D, F64, device), **WANT) for k in cuts]
    _compare({name: torch.cat([q[name] for q in parts]) for name in out}, out, K)
    _envs_equal(cut, one, K)
    rep = replay.rollout(out["actions"], reward=True, done=True, soc_trace=True, status_trace=True, observations=True,
                         final_observations=True, out=_nan_rows(K, N, D, F64, device))
    _compare(rep, {k: v for k, v in out.items() if k not in ("actions", "probs")}, K)
    _envs_equal(replay, one, K)
    for e in (cut, replay):
        for name in one.episode_stats:
            assert torch.equal(e.episode_stats[name], one.episode_stats[name]), name
        e.env.close()
    one.env.close()


@pytest.mark.gpu
def test_temperature_zero_is_the_greedy_launch(device):
    K = 64
    plain, cold = _envs(device, "genset+battery+grid", "factorised", F64, 2, twin=None)
    D = plain.env.engine.obs_dim
    policy = _spread_policy(7, plain.obs0, 16, _n_out(plain, True))
    ref = plain.rollout_policy(policy, K, out=_nan_rows(K, N, D, F64, device), **WANT)
    out = cold.rollout_policy(policy, K, sampling=_sampling(seed=8, temperature=0.0), probs=True, out=_nan_rows(K, N, D, F64, device), **WANT)
    assert torch.equal(out.pop("probs"), torch.ones(K, N, dtype=F64, device=device))
    _compare(out, ref, K)
    _envs_equal(cold, plain, K)
    for name in plain.episode_stats:
        assert torch.equal(cold.episode_stats[name], plain.episode_stats[name]), name
    with pytest.raises(ValueError, match="exclude each other"):
        from pymgrid_amd import Exploration
        cold.rollout_policy(policy, 4, sampling=_sampling(), exploration=Exploration(1, epsilon=0.1))
    with pytest.raises(ValueError, match="probs"):
        cold.rollout_policy(policy, 4, probs=True)
    with pytest.raises(ValueError, match="sampling.scale names"):
        cold.rollout_policy(policy, 4, sampling=_sampling(scale=np.ones(N - 1)))
    _envs_equal(cold, plain, K)                                   # (nothing was launched)
    plain.env.close(); cold.env.close()


@pytest.mark.gpu
def test_step_k_policy_refuses_sampling(device):
    from pymgrid_amd.hetero import PerGridWindowEnv
    pe = PerGridWindowEnv(_batch(device, "genset+battery", "factorised", N, t=60), trajectory_length=9, discrete=False, auto_reset=True, seed=2)
    pe.reset()
    pol = _policy(1, pe.env.engine.obs_dim, 16, pe.env.engine.action_dim, "continuous")
    snap = _snapshot(pe.env)
    with pytest.raises(ValueError, match="sampling"):
        pe.step_k_policy(pol, 4, sampling=_sampling())
    _untouched(pe.env, snap)
    pe.env.close()


@pytest.mark.gpu
def test_refusals_of_the_c_abi(device):
    """The call refuses -- nothing launched: state, counter and the caller's buffers untouched -- a forecast horizon, a lock-step
    handle, n_out != n_actions, several modules of a kind with the codes of mgx_rollout_policy_episodes, and a NULL or wrong-sized
    mgx_sampling and a negative, infinite or NaN temperature with MGX_ERR_INVALID."""
    from pymgrid_amd import DiscreteBatchedMicrogridEnv, _lib
    from pymgrid_amd.generator import generate, widen
    from pymgrid_amd.hetero import PerGridWindowEnv
    n, K = N, 5
    name = b"mgx_rollout_policy_sample_episodes"
    nan = float("nan")
    bufs = [torch.full((K, n), nan, dtype=F64, device=device), torch.full((K, n), nan, dtype=F64, device=device),
            torch.full((K, n), 255, dtype=torch.uint8, device=device)]

    def struct(**kw):
        st, _ = _sampling(seed=3, temperature=1.0).c_struct(device, n)
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    def refused(env, code, word, sst=None, pst=None, table=None, null=False):
        e = env.engine
        table = env._table if table is None else table
        if pst is None:
            pst, keep = _c_policy(device, min(e.obs_dim, 12), 16, len(table))
        sst = struct() if sst is None else sst
        tptr, n_lists = e._table_ptr(table)
        snap = _snapshot(env)
        rc = e._lib.mgx_rollout_policy_sample_episodes(e._h, C.byref(pst), None if null else C.byref(sst), tptr, n_lists, K,
                                                       bufs[0].data_ptr(), None, None, None, bufs[2].data_ptr(), bufs[1].data_ptr(),
                                                       None, None, None)
        msg = e._lib.mgx_last_error()
        assert rc == code and name in msg and word in msg, (rc, msg)
        torch.cuda.synchronize()
        _untouched(env, snap)
        assert bool(torch.isnan(bufs[0]).all()) and bool(torch.isnan(bufs[1]).all()) and bool((bufs[2] == 255).all())
    pe = PerGridWindowEnv(_batch(device, "genset+battery+grid", "factorised", n, H=6, t=60), trajectory_length=9, discrete=True,
                          auto_reset=True, seed=2)
    pe.reset()
    refused(pe.env, _lib.MGX_ERR_UNSUPPORTED, b"horizon")                           # a forecast horizon
    pe.env.close()
    env = DiscreteBatchedMicrogridEnv(_batch(device, "genset+battery+grid", "factorised", n, t=60))
    env.reset()
    refused(env, _lib.MGX_ERR_INVALID, b"in-place episodes")                        # a lock-step handle
    env.reset_windows(torch.zeros(n, dtype=torch.int32, device=device), None, max_length=9, rolling="inplace")
    e = env.engine
    n_out = len(env._table)
    refused(env, _lib.MGX_ERR_INVALID, b"n_out", pst=_c_policy(device, e.obs_dim, 16, n_out - 1)[0])
    refused(env, _lib.MGX_ERR_INVALID, b"NULL", null=True)
    refused(env, _lib.MGX_ERR_INVALID, b"struct_size", struct(struct_size=C.sizeof(_lib.Sampling) - 8))
    refused(env, _lib.MGX_ERR_INVALID, b"struct_size", struct(struct_size=0))
    for bad in (-0.5, -1e-300, float("inf"), nan):
        refused(env, _lib.MGX_ERR_INVALID, b"temperature", struct(temperature=bad))
    # ... and the handle is taken once nothing stands in the way
    pst, keep = _c_policy(device, e.obs_dim, 16, n_out)
    sst = struct()
    tptr, n_lists = e._table_ptr(env._table)
    t_before = e._lib.mgx_current_step(e._h)
    assert e._lib.mgx_rollout_policy_sample_episodes(e._h, C.byref(pst), C.byref(sst), tptr, n_lists, K, bufs[0].data_ptr(), None, None, None,
                                                     bufs[2].data_ptr(), bufs[1].data_ptr(), None, None, None) == _lib.MGX_OK, e._lib.mgx_last_error()
    torch.cuda.synchronize()
    assert e._lib.mgx_current_step(e._h) == t_before + K
    # (zero parameters: all logits equal, every id weighs 1.0)
    assert not bool(torch.isnan(bufs[0]).any()) and torch.equal(bufs[1], torch.full((K, n), 1.0 / n_out, dtype=F64, device=device))
    assert int(bufs[2].max()) == n_out - 1 and int(bufs[2].min()) == 0
    env.close()
    bufs[0].fill_(nan); bufs[1].fill_(nan); bufs[2].fill_(255)
    wide = widen(generate(n, n_steps=60, seed=4, arch="genset+battery", device=device), n_battery=2)
    env = DiscreteBatchedMicrogridEnv(wide)
    env.reset_windows(torch.zeros(n, dtype=torch.int32, device=device), None, max_length=9, rolling="inplace")
    refused(env, _lib.MGX_ERR_UNSUPPORTED, b"one module of every kind", table=np.zeros((1, 3, 2), dtype=np.int32))
    env.close()
