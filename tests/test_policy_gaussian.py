"""The Gaussian policy head inside the fused continuous K-step (mgx_step_k_policy_gaussian_episodes, ``sampling=GaussianSampling`` /
``logp=`` / ``raw_actions=`` / ``critic=`` / ``values=`` of StepEngine.step_k_policy_episodes and PerGridWindowEnv.step_k_policy): K
steps in one launch == a twin stepped K times with ``policy.act(obs, gs, counter, return_logp=True, return_raw=True)``, bit for bit
(torch.equal: log, sine, cosine and the square root are fixed sequences of IEEE operations on both sides, the draws integer Philox
words, the division correctly rounded -- so there is no tolerance).  Small on purpose: 193 grids (three waves and a partial one),
five-step episodes so that grids restart inside a launch, 12 steps.  The forms of the kernels these cases leave out -- all ten layouts x the three row sources -- run in
tests/test_layout_matrix_policy.py, which also replays the launches on the CPU oracle."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_episode_rows import HostStats, _same_bits, _snapshot, _state_equal, _untouched
from test_policy_explore import _compare, _envs_equal, _forms_of
from test_policy_rollout import WANT, _c_policy, _envs, _policy, _trace_end, _trace_launch, _trace_start

F64, F32 = torch.float64, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, LENGTH, K = 193, 5, 12
SIGMA = [0.3, 0.1, 0.2, 0.05]
VALUES = ("values", "final_values", "last_value")
MORE = dict(logp=True, raw_actions=True)


def _gs(seed=23, sigma=SIGMA, **kw):
    from pymgrid_amd import GaussianSampling
    return GaussianSampling(seed, sigma, **kw)


def _head(seed, policy):
    """A ValueHead of random parameters on the trunk of the continuous ``policy``."""
    from pymgrid_amd import ValueHead
    rng = np.random.default_rng(seed)
    P, n_mid = policy.n_policies, policy.n_hidden or policy.n_in
    return ValueHead(rng.normal(0.0, 1.0, size=(P, n_mid)), rng.normal(0.0, 0.5, size=(P,)), head="continuous")


def _nan(K, n, D, dtype, device, values=False):
    """NaN-filled final_obs (and final_values): what a launch does not write keeps these bits."""
    out = dict(final_obs=torch.full((K, n, D), float("nan"), dtype=dtype, device=device))
    if values:
        out["final_values"] = torch.full((K, n), float("nan"), dtype=F64, device=device)
    return out


def _twin_steps(twin, policy, gs, obs, K, hs, walked=None):
    """K times ``u, logp, raw = policy.act(obs, gs, counter, ...); obs, r, done, info = twin.step(u)``, the counter read from the env
    before the step: what the fused call offers, per step.  ``walked``: a list that receives every grid's series row before each
    step."""
    rows = {k: [] for k in ("reward", "done", "soc_trace", "status_trace", "actions", "raw_actions", "logp", "obs", "final_obs")}
    cols = twin.env.batch.cols
    for _ in range(K):
        if walked is not None:
            walked.append(twin.env.current_steps.clone())
        t = twin.env.current_step
        assert isinstance(t, int)
        u, logp, raw = policy.act(obs, gs, counter=t, return_logp=True, return_raw=True)
        obs, r, d, info = twin.step(u, normalized=True)
        rows["actions"].append(u.clone()); rows["raw_actions"].append(raw.clone()); rows["logp"].append(logp.clone())
        rows["reward"].append(r.clone()); rows["done"].append(d.clone()); rows["obs"].append(obs.clone())
        fo = info["final_observation"]
        rows["final_obs"].append(torch.where(d[:, None], fo, torch.full_like(fo, float("nan"))))
        if "soc" in cols:
            rows["soc_trace"].append(cols["soc"].clone())
        if "gen_status" in cols:
            rows["status_trace"].append(cols["gen_status"].clone().view(torch.int32))
        hs.add(r, d)
    return {k: torch.stack(v) for k, v in rows.items() if v}, obs


class _gather:
    """``series == "gather"``: the materialised series without their grid-major copy, for the time of the block."""

    def __init__(self, series):
        self.series = series

    def __enter__(self):
        from pymgrid_amd import _lib
        self.old = _lib.get_tunable("grid_major_copy")[0]
        if self.series == "gather":
            _lib.set_tunable("grid_major_copy", 0)

    def __exit__(self, *exc):
        from pymgrid_amd import _lib
        _lib.set_tunable("grid_major_copy", self.old)


def _population(device, fused, n_hidden, P, n=N, seed=7):
    D, A = fused.env.engine.obs_dim, fused.env.engine.action_dim
    index = None
    if P > 1:
        index = torch.randint(-1, P + 1, (n,), generator=torch.Generator().manual_seed(11)).to(torch.int32)
        assert int(index.min()) == -1 and int(index.max()) == P
    return _policy(seed, D, n_hidden, A, "continuous", P=P, index=index)


# (layout flags: 2 battery, A = 1; 1 genset, A = 2; 6 battery + grid, A = 2; 3 genset + battery, A = 3; 5 genset + grid, A = 3;
#  7 and 15 all three, A = 4) x the three row sources x hidden units x the row format x the population
CASES = [(2, "factorised", 0, F64, 1), (1, "materialised", 16, F64, 1), (6, "gather", 0, F32, 1), (3, "gather", 16, F64, 1),
         (5, "factorised", 0, F64, 1), (7, "factorised", 16, F64, 1), (7, "materialised", 0, F32, 1), (7, "factorised", 16, F64, 3),
         (15, "materialised", 16, F32, 3)]


def test_the_cases_cover_what_they_should():
    A = {2: 1, 1: 2, 6: 2, 3: 3, 5: 3, 7: 4, 15: 4}
    assert {A[c[0]] for c in CASES} == {1, 2, 3, 4} and {c[1] for c in CASES} == {"factorised", "materialised", "gather"}
    assert {c[2] for c in CASES} == {0, 16} and {c[3] for c in CASES} == {F64, F32} and {c[4] for c in CASES} == {1, 3}


def _fused_equals_stepped(device, flags, series, n_hidden, obs_dtype, P, critic=False, n=N, length=LENGTH, steps=K, trace=None, seed=7,
                          sigma=SIGMA):
    """One Gaussian launch of ``steps`` steps == its stepped twin: everything the greedy test compares, the raw draws and the
    log-probabilities; ``critic``: the launch with a value head (the other kernel form) -- the three value outputs against
    ``head.value`` on the twin's rows, everything else as without one; then one more single step.  ``length`` None: own lengths
    (then only some grids restart).  ``trace``: a dict that receives what test_policy_rollout._trace_launch records; ``seed``: of
    the policy's parameters."""
    K = steps
    with _gather(series):
        fused, twin = _envs(device, False, flags, series, length, obs_dtype, n)
        e = fused.env.engine
        D, A = e.obs_dim, e.action_dim
        policy, gs = _population(device, fused, n_hidden, P, n, seed), _gs(sigma=sigma)
        head = _head(9, policy) if critic else None
        hs = HostStats(n, device)
        _trace_start(trace, fused, False)
        more = dict(critic=head, values=True) if critic else {}
        out = fused.step_k_policy(policy, K, sampling=gs, out=_nan(K, n, D, obs_dtype, device, values=critic), **more, **MORE, **WANT)
        walked = [] if trace is not None else None
        ref, obs = _twin_steps(twin, policy, gs, twin.obs0, K, hs, walked)
        _trace_launch(trace, walked, out, ref)
        _trace_end(trace, fused)
        if trace is not None:
            trace["raw"] = ref["raw_actions"]
        assert out["logp"].shape == (K, n) and out["raw_actions"].shape == (K, n, A) and out["logp"].dtype == F64
        d = ref["done"]
        if critic:
            got = {name: out.pop(name) for name in VALUES}
            chosen_on = [twin.obs0] + list(ref["obs"][:-1])
            assert got["values"].shape == (K, n) and got["last_value"].shape == (n,)
            assert torch.equal(got["values"], torch.stack([head.value(policy, o) for o in chosen_on]))
            finals = torch.stack([head.value(policy, o) for o in ref["final_obs"]])
            assert torch.equal(got["final_values"][d], finals[d])
            assert bool(torch.isnan(got["final_values"][~d]).all()) and not bool(torch.isnan(got["final_values"][d]).any())
            assert torch.equal(got["last_value"], head.value(policy, ref["obs"][-1]))
        _compare(out, ref, K)
        d = out["done"]
        if length is not None and length < K:
            assert int(d.sum()) >= n                                      # every grid restarts inside the launch, most of them twice
        assert bool(torch.isnan(out["final_obs"][~d]).all()) and not bool(torch.isnan(out["final_obs"][d]).any())
        _envs_equal(fused, twin, K)
        hs.check(fused.episode_stats)
        # the conditions on the test itself, from the stepped twin alone: the draws move the controls, both edges of the clip occur
        raw, u = ref["raw_actions"], ref["actions"]
        if A:
            assert bool(torch.isfinite(ref["logp"]).all()) and ref["logp"].unique().numel() > K * n // 2
            assert bool((raw != u).any()) and bool((u == 0).any()) and bool(((u > 0) & (u < 1)).any())
        # the env stands where the twin stands: one more single step
        a = policy.act(obs, gs, counter=twin.env.current_step)
        assert torch.equal(a, policy.act(out["obs"][-1], gs, counter=fused.env.current_step))
        (o1, r1, d1, _), (o2, r2, d2, _) = fused.step(a, normalized=True), twin.step(a, normalized=True)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
        _state_equal(fused.env, twin.env)
        fused.env.close(); twin.env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags,series,n_hidden,obs_dtype,P", CASES)
def test_fused_equals_stepped(flags, series, n_hidden, obs_dtype, P, device):
    _fused_equals_stepped(device, flags, series, n_hidden, obs_dtype, P)


@pytest.mark.gpu
def test_one_launch_equals_two(device):
    """12 steps == 5 + 7: the draws are functions of the counter, C_i and the scale are formed again in every launch."""
    whole, parts = _envs(device, False, 7, "factorised", LENGTH, F64, N, twin=None)
    D = whole.env.engine.obs_dim
    policy = _population(device, whole, 16, 1)
    scale = torch.as_tensor(np.linspace(0.5, 2.0, N)).to(device)
    gs = _gs(scale=scale)
    out = whole.step_k_policy(policy, K, sampling=gs, out=_nan(K, N, D, F64, device), **MORE, **WANT)
    cut = [parts.step_k_policy(policy, k, sampling=gs, out=_nan(k, N, D, F64, device), **MORE, **WANT) for k in (5, 7)]
    _compare({name: torch.cat([q[name] for q in cut]) for name in out}, out, K)
    _envs_equal(parts, whole, K)
    for name in whole.episode_stats:
        assert torch.equal(parts.episode_stats[name], whole.episode_stats[name]), name
    whole.env.close(); parts.env.close()


@pytest.mark.gpu
def test_the_rule_on_the_device_is_the_rule_on_the_host(device):
    """policy_log, policy_quarter_turn, policy_sqrt and gaussian_pair on 2^16 arguments: the device's values == the CPU's, bit for
    bit -- the check on the device's division (everything else is adds, multiplies and integer words; the square root is a fixed
    sequence of them because this test failed on the pair with the library roots)."""
    from pymgrid_amd.policy import gaussian_pair, policy_log, policy_quarter_turn, policy_sqrt
    n = 2 ** 16
    g = torch.Generator().manual_seed(4)
    a = torch.cat([1.0 - torch.rand(n // 2 - 3, dtype=F64, generator=g), 10.0 ** (torch.rand(n // 2, dtype=F64, generator=g) * 600.0 - 300.0),
                   torch.tensor([1.0, 2.0 ** -53, 1.0 - 2.0 ** -53], dtype=F64)])
    assert a.numel() == n
    assert _same_bits(policy_log(a.to(device)).cpu(), policy_log(a))
    f = torch.cat([torch.randint(0, 2 ** 52, (n - 3,), generator=g).to(F64) * 2.0 ** -52, torch.tensor([0.0, 0.5, 1.0 - 2.0 ** -52], dtype=F64)])
    for dev, host in zip(policy_quarter_turn(f.to(device)), policy_quarter_turn(f)):
        assert _same_bits(dev.cpu(), host)
    grid = torch.arange(n)
    for seed, t, p in ((1, 0, 0), (2 ** 64 - 1, 8759, 1)):
        for dev, host in zip(gaussian_pair(seed, grid.to(device), t, p), gaussian_pair(seed, grid, t, p)):
            assert _same_bits(dev.cpu(), host)
    v = torch.cat([torch.rand(n // 2, dtype=F64, generator=g) * 74.0, 10.0 ** (torch.rand(n // 2 - 3, dtype=F64, generator=g) * 18.0 - 16.0),
                   torch.tensor([0.0, -0.0, 2.0 ** -52], dtype=F64)])
    assert _same_bits(policy_sqrt(v.to(device)).cpu(), policy_sqrt(v))
    # (measured, not asserted -- the rule no longer calls it: where the library roots of device and host differ)
    print("torch.sqrt, device against host:", int((torch.sqrt(v.to(device)).cpu() != torch.sqrt(v)).sum()), "of", n, "values differ")


@pytest.mark.gpu
@pytest.mark.parametrize("n_hidden,P,obs_dtype", [(16, 1, F64), (0, 3, F32)])
def test_values(n_hidden, P, obs_dtype, device):
    """values, final_values where done (and only there: the other entries keep the NaN they were given) and last_value ==
    ValueHead.value on the rows the launch returns; the launch with a critic leaves every other output as the one without."""
    fused, plain = _envs(device, False, 7, "factorised", LENGTH, obs_dtype, N, twin=None)
    D = fused.env.engine.obs_dim
    policy, gs = _population(device, fused, n_hidden, P), _gs()
    head = _head(9, policy)
    out = fused.step_k_policy(policy, K, sampling=gs, critic=head, values=True, out=_nan(K, N, D, obs_dtype, device, values=True), **MORE, **WANT)
    same = plain.step_k_policy(policy, K, sampling=gs, out=_nan(K, N, D, obs_dtype, device), **MORE, **WANT)
    got = {name: out.pop(name) for name in VALUES}
    _compare(out, same, K)
    _envs_equal(fused, plain, K)
    for name in fused.episode_stats:
        assert torch.equal(plain.episode_stats[name], fused.episode_stats[name]), name
    d = out["done"]
    assert int(d.sum()) >= N and not bool(d.all())
    chosen_on = [fused.obs0] + list(out["obs"][:-1])
    assert got["values"].shape == (K, N) and got["last_value"].shape == (N,)
    assert torch.equal(got["values"], torch.stack([head.value(policy, o) for o in chosen_on]))
    finals = torch.stack([head.value(policy, o) for o in out["final_obs"]])
    assert torch.equal(got["final_values"][d], finals[d])
    assert bool(torch.isnan(got["final_values"][~d]).all()) and not bool(torch.isnan(got["final_values"][d]).any())
    assert torch.equal(got["last_value"], head.value(policy, out["obs"][-1]))
    # at a restart the final row's value is not the new episode's first row's
    first = torch.stack([head.value(policy, o) for o in out["obs"]])
    assert bool((finals[d] != first[d]).any())
    # one output alone, and an allocated final_values: zeros where nothing restarted
    only = plain.step_k_policy(policy, 3, sampling=gs, critic=head, values=("final_values",), done=True)
    assert set(only) == {"reward", "done", "final_values"}
    assert torch.equal(only["final_values"][~only["done"]], torch.zeros_like(only["final_values"][~only["done"]]))
    fused.env.close(); plain.env.close()


@pytest.mark.gpu
def test_sigma_zero_is_the_greedy_launch_and_a_ladder_with_zeros(device):
    greedy, zero, ladder, twin = _envs(device, False, 7, "factorised", LENGTH, F64, N, count=4, twin=3)
    D = greedy.env.engine.obs_dim
    policy = _population(device, greedy, 16, 1)
    ref = greedy.step_k_policy(policy, K, out=_nan(K, N, D, F64, device), **WANT)
    out = zero.step_k_policy(policy, K, sampling=_gs(sigma=0.0), out=_nan(K, N, D, F64, device), **MORE, **WANT)
    assert torch.equal(out.pop("logp"), torch.zeros(K, N, dtype=F64, device=device))
    assert torch.equal(out.pop("raw_actions"), torch.stack([policy.outputs(o) for o in [zero.obs0] + list(out["obs"][:-1])]))
    _compare(out, ref, K)
    _envs_equal(zero, greedy, K)
    # a ladder with zeros: exactly those grids are greedy (their draws are never made), the others follow the host rule
    scale = torch.as_tensor(np.where(np.arange(N) % 4 == 0, 0.0, 0.4 ** (7 * np.arange(N) / (N - 1)))).to(device)
    dead = scale == 0
    gs = _gs(seed=99, scale=scale)
    out = ladder.step_k_policy(policy, K, sampling=gs, out=_nan(K, N, D, F64, device), **MORE, **WANT)
    want, _ = _twin_steps(twin, policy, gs, twin.obs0, K, HostStats(N, device))
    _compare(out, want, K)
    same = lambda a, b: _same_bits(a, b) if a.is_floating_point() else torch.equal(a, b)     # noqa: E731  (final_obs keeps its NaN)
    for name in ref:
        assert same(out[name][:, dead], ref[name][:, dead]), name
    assert bool((out["logp"][:, dead] == 0).all()) and bool((out["logp"][:, ~dead] != 0).all())
    assert bool((out["raw_actions"][:, ~dead] != torch.stack([policy.outputs(o) for o in [ladder.obs0] + list(out["obs"][:-1])])[:, ~dead]).all())
    for e in (greedy, zero, ladder, twin):
        e.env.close()


@pytest.mark.gpu
def test_nan_logits_give_a_nan_raw_a_zero_control_and_a_finite_logp(device):
    from pymgrid_amd import MLPPolicy
    (pe,) = _envs(device, False, 3, "factorised", LENGTH, F64, N, count=1, twin=None)
    D, A = pe.env.engine.obs_dim, pe.env.engine.action_dim
    base = _policy(7, D, 0, A, "continuous")
    b2 = base.b2.clone(); b2[0, 1] = float("nan")
    policy = MLPPolicy(None, None, base.W2, b2, head="continuous")
    out = pe.step_k_policy(policy, K, sampling=_gs(), actions=True, **MORE)
    assert bool(torch.isnan(out["raw_actions"][:, :, 1]).all()) and bool((out["actions"][:, :, 1] == 0).all())
    assert bool(torch.isfinite(out["raw_actions"][:, :, [0, 2]]).all()) and bool(torch.isfinite(out["logp"]).all())
    assert bool(torch.isfinite(out["reward"]).all())
    pe.env.close()


@pytest.mark.gpu
def test_the_outputs_feed_gae(device):
    from pymgrid_amd import gae
    from pymgrid_amd.policy import gae_host
    (pe,) = _envs(device, False, 7, "factorised", LENGTH, F64, N, count=1, twin=None)
    policy = _population(device, pe, 16, 1)
    out = pe.step_k_policy(policy, K, sampling=_gs(), critic=_head(9, policy), values=True, done=True, logp=True,
                           out=dict(final_values=torch.full((K, N), float("nan"), dtype=F64, device=device)))
    assert 0.0 < float(out["done"].double().mean()) < 1.0
    for gamma, lam in ((0.99, 0.95), (1.0, 1.0), (0.9, 0.0)):
        got = gae(out["reward"], out["done"], out["values"], out["last_value"], final_value=out["final_values"], gamma=gamma, lam=lam)
        ref = gae_host(out["reward"], out["done"], out["values"], out["last_value"], final_value=out["final_values"], gamma=gamma, lam=lam)
        assert _same_bits(got["advantages"], ref["advantages"]) and _same_bits(got["returns"], ref["returns"])
        assert bool(torch.isfinite(got["advantages"]).all())
    pe.env.close()


# ---- the refusals, on a live handle ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_of_the_c_abi_and_of_the_python_surface(device):
    """MGX_ERR_INVALID for a NULL or wrong-sized mgx_gaussian, a bad sigma, a value output without a critic; MGX_ERR_UNSUPPORTED where
    the sets WITH the critic pass MGX_POLICY_LDS_BYTES (without it they fit, and launch); the Python refusals.  Nothing is launched:
    state, counter and the caller's buffers stay untouched, and the next valid launch still equals its twin."""
    from pymgrid_amd import Exploration, MgxError, Sampling, ValueHead, _lib
    fused, twin = _envs(device, False, 7, "factorised", LENGTH, F64, N)
    env, e = fused.env, fused.env.engine
    D, A = e.obs_dim, e.action_dim
    name = b"mgx_step_k_policy_gaussian_episodes"
    pst, keep = _c_policy(device, D, 16, A)
    reward = torch.full((K, N), float("nan"), dtype=F64, device=device)

    def call(gst, values=(None, None, None)):
        return e._lib.mgx_step_k_policy_gaussian_episodes(e._h, C.byref(pst), None if gst is None else C.byref(gst), None, K,
                                                          reward.data_ptr(), None, None, None, None, None, None, *values, None, None, None)

    def struct(**kw):
        st, _ = _gs().c_struct(device, N)
        for k, v in kw.items():
            if k.startswith("sigma"):
                st.sigma[int(k[5:])] = v
            else:
                setattr(st, k, v)
        return st
    bad = [("NULL argument", None, {}), ("struct_size", struct(struct_size=0), {}), ("sigma[0]", struct(sigma0=-0.1), {}),
           ("sigma[2]", struct(sigma2=float("nan")), {}), ("sigma[1]", struct(sigma1=float("inf")), {}),
           ("sigma[3]", struct(sigma3=1e-310), {}), ("without a critic", struct(), dict(values=(reward.data_ptr(), None, None)))]
    for word, gst, kw in bad:
        snap = _snapshot(env)
        rc = call(gst, **kw)
        msg = e._lib.mgx_last_error()
        assert rc == _lib.MGX_ERR_INVALID and name in msg and word.encode() in msg, (word, rc, msg)
        torch.cuda.synchronize()
        _untouched(env, snap)
        assert bool(torch.isnan(reward).all())
    # four sets of 60 hidden units fill MGX_POLICY_LDS_BYTES exactly; the critic's 1 + 60 doubles per set pass it
    wide = _policy(7, D, 60, A, "continuous", P=4)
    assert wide.lds_bytes == _lib.POLICY_LDS_BYTES and _head(9, wide).lds_bytes(wide) > _lib.POLICY_LDS_BYTES
    snap = _snapshot(env)
    with pytest.raises(MgxError, match="MGX_POLICY_LDS_BYTES") as err:
        fused.step_k_policy(wide, K, sampling=_gs(), critic=_head(9, wide), values=True)
    assert err.value.code == _lib.MGX_ERR_UNSUPPORTED
    pol = _population(device, fused, 16, 1)
    for kw, word in ((dict(sampling=Sampling(1)), "sampling"), (dict(sampling=_gs(), exploration=Exploration(1, sigma=0.1)), "exclude"),
                     (dict(logp=True), "logp"), (dict(raw_actions=True), "raw_actions"), (dict(critic=_head(9, pol)), "critic="),
                     (dict(sampling=_gs(), values=True), "critic="), (dict(sampling=_gs(scale=np.ones(N - 1))), "sampling.scale names"),
                     (dict(sampling=_gs(), critic=_head(9, wide)), "does not fit"),
                     (dict(sampling=_gs(), critic=ValueHead(np.zeros(16), np.float64(0.0))), "head='discrete'")):
        with pytest.raises(ValueError, match=word):
            fused.step_k_policy(pol, K, **kw)
    with pytest.raises(ValueError, match="GaussianSampling"):
        e.step_k_policy_episodes(pol, K, sampling=Sampling(1))
    with pytest.raises(TypeError, match="probs"):
        fused.step_k_policy(pol, K, sampling=_gs(), probs=True)
    torch.cuda.synchronize()
    _untouched(env, snap)
    # nothing was left behind: the wide policy without a critic launches, and the launch equals its twin
    gs = _gs(seed=3)
    out = fused.step_k_policy(wide, K, sampling=gs, out=_nan(K, N, D, F64, device), **MORE, **WANT)
    ref, _ = _twin_steps(twin, wide, gs, twin.obs0, K, HostStats(N, device))
    _compare(out, ref, K)
    _envs_equal(fused, twin, K)
    fused.env.close(); twin.env.close()


# ---- what the compiler made of the new forms -----------------------------------------------------------------------------------------
# head (PolicyHead, csrc/mgx_policy.hpp: Gaussian, Gaussian with a critic): (forms, most AGPRs, most spilled SGPRs, least occupancy
# in waves per SIMD) -- DESIGN.md's table
DOCUMENTED = {4: (30, 0, 48, 2), 5: (30, 0, 51, 2)}


def test_the_gaussian_kernel_uses_what_design_md_says():
    """The 60 forms of the Gaussian heads (ten layouts x three row sources, without and with the critic): no scratch memory, no vector register spilled,
    vgpr + agpr <= 512, LDS within the siblings' bound; AGPRs, spilled SGPRs and occupancy no worse than DESIGN.md records them."""
    from pymgrid_amd import _lib
    _lib.build()
    usage = _lib.resource_usage()
    if usage is None:
        pytest.skip("libmgx.so was not built on this machine (no resource_usage.json beside the objects)")
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        design = fh.read()
    kernel = "step_k_policy_head_episodes_kernel"
    assert f"`{kernel}<7,4,0,4>`" in design and f"`{kernel}<7,4,0,5>`" in design
    for head, (n_forms, agpr, sgpr_spill, occupancy) in DOCUMENTED.items():
        forms = _forms_of(usage, (kernel, head))
        assert len(forms) == n_forms, (head, sorted(forms))
        for name, u in forms.items():
            assert u["scratch"] == 0 and u["vgpr_spill"] == 0, (name, u)
            assert u["vgpr"] <= 256 and u["agpr"] <= agpr and u["vgpr"] + u["agpr"] <= 512, (name, u)
            assert u["sgpr_spill"] <= sgpr_spill and u["occupancy"] >= occupancy, (name, u)
            assert u["lds"] <= 24576 + 64, (name, u)
