"""Exploring policies inside the fused closed-loop launches (mgx_rollout_policy_explore_episodes /
mgx_step_k_policy_explore_episodes, ``exploration=`` of StepEngine.rollout_policy_episodes / step_k_policy_episodes and
PerGridWindowEnv.rollout_policy / step_k_policy): the rule of ``mgx_exploration`` (include/mgx.h) on the host
(``MLPPolicy.act(obs, exploration, counter)``) and K steps in one launch == a twin stepped K times with it, bit for bit
(torch.equal: the draws are integer Philox words, the noise a sum of their fields, so there is no tolerance).  The forms of the kernels these cases leave out -- all ten layouts x the three row sources -- run in
tests/test_layout_matrix_policy.py, which also replays the launches on the CPU oracle."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from layouts import LAYOUTS
from test_episode_rows import HostStats, _same_bits, _snapshot, _state_equal, _untouched
from test_policy_rollout import WANT, _c_policy, _envs, _launch, _n_out, _policy, _trace_end, _trace_launch, _trace_start

F64, F32 = torch.float64, torch.float32
LAUNCHES = (1, 7, 64)
EPSILON, SIGMA = 0.25, 0.15
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _explore(seed=5, **kw):
    from pymgrid_amd import Exploration
    return Exploration(seed, **kw)


def _rows(n, n_in, seed=3):
    return torch.as_tensor(np.random.default_rng(seed).uniform(0.0, 1.0, size=(n, n_in)))


# ---- CPU: the host statement of the rule ---------------------------------------------------------------------------------------
def test_host_philox_reproduces_synth_uniform_and_the_tag_separates_the_streams():
    from pymgrid_amd.generator import synth_uniform_host
    from pymgrid_amd.policy import EXPLORE_TAG, SYNTH_TAG, philox_words, uniform53
    rng = np.random.default_rng(1)
    grid = np.concatenate([rng.integers(0, 2 ** 40, size=1500), np.arange(500)])
    row = np.concatenate([rng.integers(0, 2 ** 31, size=1500), rng.integers(0, 9000, size=500)])
    for seed in (0, 23, 2 ** 63 + 12345, 2 ** 64 - 1):
        ref = synth_uniform_host(seed, grid, row)
        r = philox_words(seed, grid, row, SYNTH_TAG)
        assert r.dtype == torch.int64 and int(r.min()) >= 0 and int(r.max()) < 2 ** 32
        assert np.array_equal(uniform53(r[0], r[1]).numpy(), ref)
        x = philox_words(seed, grid, row, EXPLORE_TAG)
        assert not bool((uniform53(x[0], x[1]) == torch.as_tensor(ref)).any())
        assert not torch.equal(philox_words(seed, grid, row, EXPLORE_TAG + 1), x)          # the draw's number is in the tag


def test_the_noise_is_a_quantised_unit_normal():
    from pymgrid_amd.policy import explore_normal
    n = 200_000
    z = torch.cat([explore_normal(77, torch.arange(n // 4), t, o) for t, o in ((0, 0), (0, 1), (1, 0), (12345, 3))])
    assert z.numel() == n and z.dtype == F64
    assert abs(float(z.mean())) < 4 / math.sqrt(n)
    assert abs(float(z.var()) - 1.0) < 0.02
    assert torch.equal(z * 1024.0, (z * 1024.0).round()) and float(z.abs().max()) <= 6.0
    assert float(z.abs().max()) > 3.5                                                    # (tails exist)


@pytest.mark.parametrize("n_hidden", [0, 16])
def test_no_exploration_is_the_greedy_rule(n_hidden):
    obs = _rows(500, 8)
    disc, cont = _policy(7, 8, n_hidden, 6, "discrete"), _policy(7, 8, n_hidden, 3, "continuous")
    for t in (0, 19):
        assert torch.equal(disc.act(obs, _explore(epsilon=0.0, sigma=0.3), t), disc.act(obs))
        assert torch.equal(cont.act(obs, _explore(epsilon=1.0, sigma=0.0), t), cont.act(obs))
        assert torch.equal(cont.act(obs, _explore(epsilon=1.0), t), cont.act(obs))
    assert not torch.equal(disc.act(obs, _explore(epsilon=0.5), 0), disc.act(obs))
    assert not torch.equal(cont.act(obs, _explore(sigma=0.3), 0), cont.act(obs))
    with pytest.raises(ValueError, match="counter"):
        disc.act(obs, _explore(epsilon=0.5))


def test_epsilon_one_takes_the_uniform_ids():
    from pymgrid_amd.policy import EXPLORE_TAG, philox_words, uniform53
    n = 4000
    obs = _rows(n, 8)
    for n_out in (1, 5, 12):
        pol = _policy(7, 8, 0, n_out, "discrete")
        ids = pol.act(obs, _explore(seed=9, epsilon=1.0), 31)
        r = philox_words(9, torch.arange(n), 31, EXPLORE_TAG)
        want = torch.clamp((uniform53(r[2], r[3]) * n_out).floor().to(torch.int32), max=n_out - 1)
        assert ids.dtype == torch.int32 and torch.equal(ids, want)
        assert int(ids.min()) == 0 and int(ids.max()) == n_out - 1 and ids.unique().numel() == n_out
        assert not torch.equal(ids, pol.act(obs, _explore(seed=9, epsilon=1.0), 32)) or n_out == 1     # the counter moves the draw


def test_scale_zeros_switch_single_grids_back_to_greedy():
    n = 600
    obs = _rows(n, 8)
    scale = torch.as_tensor(np.where(np.arange(n) % 3 == 0, 0.0, np.linspace(0.5, 2.0, n)))
    zero = scale == 0
    disc, cont = _policy(7, 8, 16, 6, "discrete"), _policy(7, 8, 16, 3, "continuous")
    a, g = disc.act(obs, _explore(epsilon=0.5, scale=scale), 4), disc.act(obs)
    assert torch.equal(a[zero], g[zero]) and not torch.equal(a[~zero], g[~zero])
    u, v = cont.act(obs, _explore(sigma=[0.2, 0.0, 0.4], scale=scale), 4), cont.act(obs)
    assert torch.equal(u[zero], v[zero]) and torch.equal(u[:, 1], v[:, 1])
    assert not torch.equal(u[~zero][:, 0], v[~zero][:, 0]) and not torch.equal(u[~zero][:, 2], v[~zero][:, 2])
    # the ladder multiplies sigma: one grid's noise is scale[i] times the unscaled one's (interior controls)
    one = cont.outputs(obs)[:, 0]
    from pymgrid_amd.policy import explore_normal
    z = explore_normal(5, torch.arange(n), 4, 0)
    w = one + (0.2 * scale) * z
    assert torch.equal(u[:, 0], torch.where(~(w > 0), torch.zeros_like(w), torch.where(w > 1, torch.ones_like(w), w)))
    with pytest.raises(ValueError, match="scale names"):
        disc.act(obs[:10], _explore(epsilon=0.5, scale=scale), 4)


def test_validation_errors():
    for bad in (dict(epsilon=-0.1), dict(epsilon=1.5), dict(epsilon=float("nan")), dict(sigma=-0.1), dict(sigma=float("nan")),
                dict(sigma=[0.1, -0.2]), dict(sigma=[0.1] * 5), dict(scale=np.zeros(4, dtype=np.float32)), dict(scale=np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            _explore(**bad)
    with pytest.raises(ValueError):
        _explore(seed=-1)
    ex = _explore(seed=2 ** 64 - 1, epsilon=1.0, sigma=0.5)
    assert ex.sigma == (0.5,) * 4 and _explore(sigma=[0.1, 0.2]).sigma == (0.1, 0.2, 0.0, 0.0)
    st, _ = ex.c_struct(torch.device("cpu"), 4)
    assert st.struct_size == C.sizeof(type(st)) and st.seed == 2 ** 64 - 1 and st.epsilon == 1.0 and list(st.sigma) == [0.5] * 4
    assert not st.scale


def test_symbols_struct_and_header():
    from pymgrid_amd import _lib
    _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "mgx.h")) as fh:
        header = fh.read()
    for name in ("mgx_rollout_policy_explore_episodes", "mgx_step_k_policy_explore_episodes"):
        assert name in _lib.SYMBOLS and getattr(L, name) is not None and f"int {name}(" in header
    assert "typedef struct mgx_exploration" in header and "0xE9100000u" in header
    assert _lib.lib().mgx_abi_minor() == 3 == _lib.ABI_MINOR
    assert C.sizeof(_lib.Policy) == 24 + 5 * C.sizeof(C.c_void_p)                       # (mgx_policy keeps its size)
    # sizeof(mgx_exploration) as a C compiler lays it out == the ctypes struct
    fields = re.search(r"typedef struct mgx_exploration \{(.*?)\} mgx_exploration;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"([a-z_]+)(?:\[4\])?;", fields)
    assert names == [n for n, _ in _lib.Exploration._fields_]
    assert C.sizeof(_lib.Exploration) == 4 + 4 + 8 + 8 + 4 * 8 + C.sizeof(C.c_void_p) == 64
    assert _lib.Exploration.seed.offset == 8 and _lib.Exploration.sigma.offset == 24 and _lib.Exploration.scale.offset == 56
    lib = _lib.lib()
    x = _lib.Exploration()
    assert lib.mgx_rollout_policy_explore_episodes(None, None, C.byref(x), None, 0, 4, None, None, None, None, None, None, None,
                                                   None) == _lib.MGX_ERR_INVALID
    assert b"mgx_rollout_policy_explore_episodes" in lib.mgx_last_error()
    assert lib.mgx_step_k_policy_explore_episodes(None, None, C.byref(x), 4, None, None, None, None, None, None, None, None) == _lib.MGX_ERR_INVALID
    assert b"mgx_step_k_policy_explore_episodes" in lib.mgx_last_error()


EXPLORE = 1     # PolicyHead (csrc/mgx_policy.hpp): the last template argument of the two head kernels
DOCUMENTED = {   # (kernel, head): (forms, most AGPRs, most spilled SGPRs, least occupancy in waves per SIMD) -- the figures of DESIGN.md
    ("rollout_policy_head_episodes_kernel", EXPLORE): (30, 52, 10, 1),
    ("step_k_policy_head_episodes_kernel", EXPLORE): (30, 0, 23, 2),
}


def _forms_of(usage, kernel):
    """The forms of ``kernel`` in a table of ``_lib.resource_usage()``: a kernel's name, or (name of a head kernel, head) for the
    forms of that head alone."""
    kernel, head = kernel if isinstance(kernel, tuple) else (kernel, None)
    return {name: u for name, u in usage.items()
            if name.split("<")[0].split("::")[-1] == kernel and (head is None or name.endswith(f", {head}>"))}


def test_the_exploring_kernels_use_what_design_md_says():
    """The 60 forms of the exploring head (two kernels x ten layouts x three row sources): no scratch memory, no vector register spilled; AGPRs,
    spilled SGPRs and occupancy no worse than DESIGN.md's kernel table records them."""
    from pymgrid_amd import _lib
    _lib.build()
    usage = _lib.resource_usage()
    if usage is None:
        pytest.skip("libmgx.so was not built on this machine (no resource_usage.json beside the objects)")
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        design = fh.read()
    for kernel, (n_forms, agpr, sgpr_spill, occupancy) in DOCUMENTED.items():
        assert f"`{kernel[0]}<7,4,0,{kernel[1]}>`" in design
        forms = _forms_of(usage, kernel)
        assert len(forms) == n_forms, (kernel, sorted(forms))
        for name, u in forms.items():
            assert u["scratch"] == 0 and u["vgpr_spill"] == 0, (name, u)
            assert u["vgpr"] <= 256 and u["agpr"] <= agpr and u["vgpr"] + u["agpr"] <= 512, (name, u)
            assert u["sgpr_spill"] <= sgpr_spill and u["occupancy"] >= occupancy, (name, u)
            assert u["lds"] <= 24576 + 64, (name, u)


# ---- GPU: fused == stepped ---------------------------------------------------------------------------------------------------------
def _twin_steps(twin, policy, ex, obs, K, hs, seen, walked=None):
    """K times ``a = policy.act(obs, ex, counter); obs, r, done, info = twin.step(a)``, the counter read from the env before the
    step; ``seen`` receives the greedy action beside every action taken, ``walked`` every grid's series row before each step."""
    rows = {k: [] for k in ("reward", "done", "soc_trace", "status_trace", "actions", "obs", "final_obs")}
    cols = twin.env.batch.cols
    for _ in range(K):
        if walked is not None:
            walked.append(twin.env.current_steps.clone())
        t = twin.env.current_step
        assert isinstance(t, int)
        a = policy.act(obs, ex, t)
        seen.append((t, a.clone(), policy.act(obs)))
        obs, r, d, info = twin.step(a) if a.dtype == torch.int32 else twin.step(a, normalized=True)
        rows["actions"].append(a.to(torch.uint8) if a.dtype == torch.int32 else a.clone())
        rows["reward"].append(r.clone()); rows["done"].append(d.clone()); rows["obs"].append(obs.clone())
        fo = info["final_observation"]
        rows["final_obs"].append(torch.where(d[:, None], fo, torch.full_like(fo, float("nan"))))
        if "soc" in cols:
            rows["soc_trace"].append(cols["soc"].clone())
        if "gen_status" in cols:
            rows["status_trace"].append(cols["gen_status"].clone().view(torch.int32))
        hs.add(r, d)
    return {k: torch.stack(v) for k, v in rows.items() if v}, obs


def _compare(out, ref, K):
    assert set(out) == set(ref), (sorted(out), sorted(ref))
    for name in out:
        if name == "final_obs":
            assert _same_bits(out[name], ref[name]), (K, name)
        else:
            assert out[name].shape == ref[name].shape and out[name].dtype == ref[name].dtype, (K, name)
            assert torch.equal(out[name], ref[name]), (K, name)


def _envs_equal(fused, twin, K):
    assert torch.equal(fused.starts, twin.starts), K
    assert (fused.lengths is None) == (twin.lengths is None)
    if twin.lengths is not None:
        assert torch.equal(fused.lengths, twin.lengths), K
    assert torch.equal(fused.env.current_steps, twin.env.current_steps), K
    assert fused.env.current_step == twin.env.current_step
    _state_equal(fused.env, twin.env)


def _explored_mask(ex, t, n, device, scale=None):
    """Which grids the rule makes explore at counter t (discrete head): u1 < epsilon (* scale)."""
    from pymgrid_amd.policy import EXPLORE_TAG, philox_words, uniform53
    r = philox_words(ex.seed, torch.arange(n, device=device), t, EXPLORE_TAG)
    return uniform53(r[0], r[1]) < (ex.epsilon if scale is None else ex.epsilon * scale)


def _fused_equals_stepped(device, discrete, arch, series, length, n_hidden, n, obs_dtype=F64, launches=LAUNCHES, vacuous=False,
                          third=False, split=None, trace=None):
    """The exploring launch, in launches of uneven size on one env, == its stepped twin after every launch; then one more single
    step.  ``vacuous``: the conditions on the test itself, from the stepped twin alone.  ``third``: a third env replays the returned
    actions through the open-loop rollout / step_k.  ``split``: a third env takes every launch in pieces of these sizes.
    ``trace``: a dict that receives what test_policy_rollout._trace_launch records, and per step the greedy action (``greedy``)."""
    from pymgrid_amd import _lib
    old = _lib.get_tunable("grid_major_copy")[0]
    if series == "gather":
        _lib.set_tunable("grid_major_copy", 0)
    try:
        envs = _envs(device, discrete, arch, series, length, obs_dtype, n, count=3 if (third or split) else 2)
        fused, twin = envs[0], envs[1]
        D = fused.env.engine.obs_dim
        policy = _policy(7, D, n_hidden, _n_out(fused, discrete), "discrete" if discrete else "continuous")
        ex = _explore(seed=23, epsilon=EPSILON, sigma=SIGMA)           # (the auto-reset seed of _envs: the tag separates the streams)
        hs = HostStats(n, device)
        obs, seen, restarts = twin.obs0, [], 0
        _trace_start(trace, fused, discrete)
        for K in launches:
            bufs = dict(final_obs=torch.full((K, n, D), float("nan"), dtype=obs_dtype, device=device))
            out = _launch(fused, policy, K, discrete, out=bufs, exploration=ex, **WANT)
            walked = [] if trace is not None else None
            ref, obs = _twin_steps(twin, policy, ex, obs, K, hs, seen, walked)
            _trace_launch(trace, walked, out, ref)
            _compare(out, ref, K)
            d = out["done"]
            assert bool(torch.isnan(out["final_obs"][~d]).all()) and not bool(torch.isnan(out["final_obs"][d]).any()), K
            _envs_equal(fused, twin, K)
            hs.check(fused.episode_stats)
            nan = lambda: dict(final_obs=torch.full_like(bufs["final_obs"], float("nan")))     # noqa: E731
            if third:                                                  # the open loop on the actions the exploring loop took
                kw = dict(reward=True, done=True, soc_trace=True, status_trace=True, observations=True, final_observations=True, out=nan())
                rep = envs[2].rollout(out["actions"], **kw) if discrete else envs[2].step_k(out["actions"], normalized=True, **kw)
                _compare(rep, {k: v for k, v in out.items() if k != "actions"}, K)
                for name in fused.episode_stats:
                    assert torch.equal(envs[2].episode_stats[name], fused.episode_stats[name]), (K, name)
                _state_equal(envs[2].env, fused.env)
            if split and K == sum(split):                              # the draws do not depend on how a roll-out is cut
                parts = [_launch(envs[2], policy, k, discrete, exploration=ex, out=dict(final_obs=nan()["final_obs"][:k]), **WANT) for k in split]
                _compare({name: torch.cat([q[name] for q in parts]) for name in out}, out, K)
                _envs_equal(envs[2], fused, K)
            elif split:
                _launch(envs[2], policy, K, discrete, exploration=ex)
            restarts += int(ref["done"].sum())
        assert int(fused.episode_stats["episodes"].sum()) == restarts
        _trace_end(trace, fused)
        if trace is not None:
            trace["greedy"] = torch.stack([g for _, _, g in seen])
        if vacuous:                                                    # the stepped twin ALONE says whether the test can pass vacuously
            if length == 9:
                assert restarts > n, restarts
            taken, greedy = torch.stack([a for _, a, _ in seen]), torch.stack([g for _, _, g in seen])
            if discrete:
                explored = torch.stack([_explored_mask(ex, t, n, device) for t, _, _ in seen])
                share = float(explored.double().mean())
                assert 0.15 < share < 0.35, share
                assert torch.equal(taken[~explored], greedy[~explored])
                assert bool((taken[explored] != greedy[explored]).any())
            else:
                inner = (greedy > 0) & (greedy < 1)
                assert bool(inner.any()) and float((taken[inner] != greedy[inner]).double().mean()) > 0.9
                assert bool((taken == 0).any()) and bool((taken == 1).any()) and bool(((taken > 0) & (taken < 1)).any())
        # the env stands where the twin stands: one more single step
        a = policy.act(obs, ex, twin.env.current_step)
        assert torch.equal(a, policy.act(out["obs"][-1], ex, fused.env.current_step))
        kw = {} if discrete else dict(normalized=True)
        (o1, r1, d1, _), (o2, r2, d2, _) = fused.step(a, **kw), twin.step(a, **kw)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
        _state_equal(fused.env, twin.env)
        for e in envs:
            e.env.close()
    finally:
        _lib.set_tunable("grid_major_copy", old)


ARCHS = ["genset+battery+grid", "genset+battery", 5]           # layouts 7, 3 and 5 (genset + grid: no battery)
SERIES = ["factorised", "materialised", "gather"]
# (discrete, arch, series) crossed; hidden units (0 / 16), the batch size (300: a partial last wave, 256: full waves) and the
# episode length (9 / own lengths) rotate so that every head sees every source, arch, size and length
CASES = [(disc, arch, series, (0, 16)[(ai + si) % 2], (300, 256)[(ai + si + di) % 2], (9, None)[(ai + 2 * si + di) % 2])
         for di, disc in enumerate((True, False)) for ai, arch in enumerate(ARCHS) for si, series in enumerate(SERIES)]


def test_the_cases_cover_every_source_size_and_length_per_head():
    for disc in (True, False):
        mine = [c for c in CASES if c[0] == disc]
        assert {c[2] for c in mine} == set(SERIES) and {c[1] for c in mine} == set(ARCHS)
        assert {c[4] for c in mine} == {300, 256} and {c[5] for c in mine} == {9, None} and {c[3] for c in mine} == {0, 16}


@pytest.mark.gpu
@pytest.mark.parametrize("discrete,arch,series,n_hidden,n,length", CASES)
def test_fused_equals_stepped(discrete, arch, series, n_hidden, n, length, device):
    _fused_equals_stepped(device, discrete, arch, series, length, n_hidden, n, vacuous=True)


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [True, False])
@pytest.mark.parametrize("flags", LAYOUTS)
def test_all_ten_layouts(flags, discrete, device):
    li = LAYOUTS.index(flags)
    _fused_equals_stepped(device, discrete, flags, SERIES[li % 3], (9, None)[li % 2], (0, 16)[(li // 2) % 2], (300, 256)[li % 2],
                          launches=(7,))


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [True, False])
def test_float32_rows(discrete, device):
    _fused_equals_stepped(device, discrete, "genset+battery+grid", "factorised", 9, 16, 300, obs_dtype=F32, vacuous=True)


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [True, False])
def test_the_open_loop_replays_the_actions_taken(discrete, device):
    _fused_equals_stepped(device, discrete, "genset+battery+grid", "materialised", 9, 16, 300, launches=(7, 64), third=True)


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [True, False])
def test_one_launch_equals_two(discrete, device):
    _fused_equals_stepped(device, discrete, "genset+battery+grid", "factorised", 9, 16, 300, launches=(64,), split=(7, 57))


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [True, False])
def test_no_exploration_is_the_existing_launch(discrete, device):
    """exploration=None, epsilon = 0 and sigma = 0 (through the exploring kernels) == rollout_policy / step_k_policy, bit for bit."""
    n, K = 300, 40
    envs = _envs(device, discrete, "genset+battery+grid", "factorised", 9, F64, n, count=4, twin=None)
    D = envs[0].env.engine.obs_dim
    policy = _policy(7, D, 16, _n_out(envs[0], discrete), "discrete" if discrete else "continuous")
    ref = _launch(envs[0], policy, K, discrete, **WANT)
    ladder = torch.zeros(n, dtype=F64, device=device)
    for q, ex in enumerate((None, _explore(epsilon=0.0, sigma=0.0), _explore(epsilon=1.0, sigma=1.0, scale=ladder))):
        out = _launch(envs[1 + q], policy, K, discrete, exploration=ex, **WANT)
        _compare(out, ref, q)
        _envs_equal(envs[1 + q], envs[0], q)
        for name in envs[0].episode_stats:
            assert torch.equal(envs[1 + q].episode_stats[name], envs[0].episode_stats[name]), (q, name)
    for e in envs:
        e.env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [True, False])
def test_a_population_on_an_exploration_ladder(discrete, device):
    """Three parameter sets by policy_index and a per-grid scale ladder with zeros: the whole launch == the host rule, and the
    zero-scale grids == the greedy launch."""
    n, K, P = 300, 40, 3
    envs = _envs(device, discrete, "genset+battery+grid", "factorised", 9, F64, n, count=3, twin=1)
    fused, twin, greedy = envs
    D = fused.env.engine.obs_dim
    index = torch.randint(-1, P + 1, (n,), generator=torch.Generator().manual_seed(11)).to(torch.int32)
    pop = _policy(13, D, 16, _n_out(fused, discrete), "discrete" if discrete else "continuous", P=P, index=index)
    ladder = torch.as_tensor(np.where(np.arange(n) % 4 == 0, 0.0, 0.4 ** (1 + 7 * np.arange(n) / (n - 1)) / 0.4)).to(device)
    zero = ladder == 0
    assert bool(zero.any()) and bool((~zero).any())
    ex = _explore(seed=99, epsilon=0.4, sigma=[0.3, 0.1, 0.2, 0.05], scale=ladder)
    bufs = lambda: dict(final_obs=torch.full((K, n, D), float("nan"), dtype=F64, device=device))     # noqa: E731
    out = _launch(fused, pop, K, discrete, exploration=ex, out=bufs(), **WANT)
    hs, seen = HostStats(n, device), []
    ref, _ = _twin_steps(twin, pop, ex, twin.obs0, K, hs, seen)
    _compare(out, ref, K)
    _envs_equal(fused, twin, K)
    hs.check(fused.episode_stats)
    plain = _launch(greedy, pop, K, discrete, out=bufs(), **WANT)
    differ = False
    same = lambda a, b: _same_bits(a, b) if a.is_floating_point() else torch.equal(a, b)     # noqa: E731  (final_obs keeps its NaN)
    for name in out:
        assert same(out[name][:, zero], plain[name][:, zero]), name
        differ |= not same(out[name][:, ~zero], plain[name][:, ~zero])
    assert differ
    taken, base = torch.stack([a for _, a, _ in seen]), torch.stack([g for _, _, g in seen])
    assert torch.equal(taken[:, zero], base[:, zero]) and not torch.equal(taken[:, ~zero], base[:, ~zero])
    for e in envs:
        e.env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [True, False])
def test_refusals_of_the_c_abi(discrete, device):
    """A wrong struct_size, epsilon = -0.1 / 1.5 / NaN, a negative or NaN sigma: MGX_ERR_INVALID, the message names the call, the
    handle and the caller's buffers untouched -- and the next valid launch still equals its twin."""
    from pymgrid_amd import _lib
    n, K = 300, 5
    fused, twin = _envs(device, discrete, "genset+battery+grid", "factorised", 9, F64, n)
    env, e = fused.env, fused.env.engine
    name = b"mgx_rollout_policy_explore_episodes" if discrete else b"mgx_step_k_policy_explore_episodes"
    pst, keep = _c_policy(device, e.obs_dim, 16, len(env._table) if discrete else e.action_dim)
    reward = torch.full((K, n), float("nan"), dtype=F64, device=device)

    def call(xst):
        if discrete:
            tptr, n_lists = e._table_ptr(env._table)
            return e._lib.mgx_rollout_policy_explore_episodes(e._h, C.byref(pst), C.byref(xst), tptr, n_lists, K, reward.data_ptr(), None,
                                                              None, None, None, None, None, None)
        return e._lib.mgx_step_k_policy_explore_episodes(e._h, C.byref(pst), C.byref(xst), K, reward.data_ptr(), None, None, None, None,
                                                         None, None, None)

    def struct(**kw):
        st, _ = _explore(epsilon=EPSILON, sigma=SIGMA).c_struct(device, n)
        for k, v in kw.items():
            if k.startswith("sigma"):
                st.sigma[int(k[5:])] = v
            else:
                setattr(st, k, v)
        return st
    bad = [("struct_size", struct(struct_size=C.sizeof(_lib.Exploration) - 8)), ("struct_size", struct(struct_size=0)),
           ("epsilon", struct(epsilon=-0.1)), ("epsilon", struct(epsilon=1.5)), ("epsilon", struct(epsilon=float("nan"))),
           ("sigma", struct(sigma0=-0.1)), ("sigma", struct(sigma3=float("nan"))), ("sigma", struct(sigma1=-1e-300))]
    for word, xst in bad:
        snap = _snapshot(env)
        rc = call(xst)
        msg = e._lib.mgx_last_error()
        assert rc == _lib.MGX_ERR_INVALID and name in msg and word.encode() in msg, (word, rc, msg)
        torch.cuda.synchronize()
        _untouched(env, snap)
        assert bool(torch.isnan(reward).all())
    # nothing was left behind: the next valid launch equals its twin
    D = e.obs_dim
    policy = _policy(7, D, 16, _n_out(fused, discrete), "discrete" if discrete else "continuous")
    ex = _explore(seed=3, epsilon=EPSILON, sigma=SIGMA)
    out = _launch(fused, policy, 7, discrete, exploration=ex, out=dict(final_obs=torch.full((7, n, D), float("nan"), dtype=F64, device=device)),
                  **WANT)
    ref, _ = _twin_steps(twin, policy, ex, twin.obs0, 7, HostStats(n, device), [])
    _compare(out, ref, 7)
    _envs_equal(fused, twin, 7)
    fused.env.close(); twin.env.close()
