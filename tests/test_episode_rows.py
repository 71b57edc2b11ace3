"""Observation rows inside the fused per-grid-episode launches (mgx_rollout_episodes_rows / mgx_step_k_episodes_rows,
StepEngine.rollout_episodes / step_k_episodes(obs=, final_obs=), PerGridWindowEnv.rollout / step_k(observations=, final_observations=),
PerGridWindowFleet, RuleBasedControl.run_episodes): obs[k] == the observation step k of a single-stepped twin returns,
final_obs[k][done[k]] == the twin's info["final_observation"][done[k]], every other entry of final_obs untouched -- bit for bit
(torch.equal), and everything the plain launches leave is left the same."""
import itertools
import os

import numpy as np
import pytest
import torch

SOAK = int(os.environ.get("MGX_FUZZ_SEED", "0"))          # soak runs: another draw of every batch / episode / id sequence
N, T = 1000, 150                        # the last wave is partial (1000 = 15 * 64 + 40): it stores its rows lane by lane
LAUNCHES = (1, 7, 64, 64, 130)          # K = 1, a K that is no multiple of a ring depth (4 / 8), 64-step launches, one above 128
KERNELS = ("rollout_episodes_rows_kernel", "step_k_episodes_rows_kernel")
EDGES = (0.0, 1.0, 0.5)


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_minor_stays():
    """The two calls are additions found by name: exported, declared in the header, bound; the ABI minor stays 3, the tunables 12;
    a NULL handle is MGX_ERR_INVALID and the message names the call."""
    import ctypes as C
    from pymgrid_amd import _lib
    _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mgx.h")) as fh:
        header = fh.read()
    for name in ("mgx_rollout_episodes_rows", "mgx_step_k_episodes_rows"):
        assert getattr(L, name) is not None
        assert name in _lib.SYMBOLS
        assert f"int {name}(" in header
    assert "typedef struct mgx_episode_rows" in header
    assert _lib.lib().mgx_abi_minor() == 3 == _lib.ABI_MINOR
    assert len(_lib.TUNABLES) == 12
    assert C.sizeof(_lib.EpisodeRows) == 8 + 2 * C.sizeof(C.c_void_p)
    rows = _lib.EpisodeRows()
    rows.struct_size = C.sizeof(_lib.EpisodeRows)
    rows.obs = 64                        # (never dereferenced: the call is refused first)
    lib = _lib.lib()
    assert lib.mgx_rollout_episodes_rows(None, None, 1, None, 0, 4, None, None, None, None, None, C.byref(rows), None) == _lib.MGX_ERR_INVALID
    assert b"mgx_rollout_episodes_rows" in lib.mgx_last_error()
    assert lib.mgx_step_k_episodes_rows(None, None, 4, 1, None, None, None, None, None, C.byref(rows), None) == _lib.MGX_ERR_INVALID
    assert b"mgx_step_k_episodes_rows" in lib.mgx_last_error()


def test_rows_kernels_spill_nothing():
    """Every instantiation of the two rows kernels: no scratch memory, no spilled scalar or vector registers, at most 256 vector
    registers (two waves per SIMD).  Discrete: ten layouts x fixed / per-step ids x three row sources; continuous: ten layouts x
    float64 / float32 controls x three row sources."""
    from pymgrid_amd import _lib
    _lib.build()
    usage = _lib.resource_usage()
    if usage is None:
        pytest.skip("libmgx.so was not built on this machine (no resource_usage.json beside the objects)")
    for kernel in KERNELS:
        forms = {name: u for name, u in usage.items() if name.split("<")[0].split("::")[-1] == kernel}
        assert len(forms) == 10 * 2 * 3, (kernel, sorted(forms))
        for name, u in forms.items():
            assert u.get("scratch", 0) == 0 and u.get("vgpr_spill", 0) == 0 and u.get("sgpr_spill", 0) == 0, (name, u)
            assert u["vgpr"] <= 256, (name, u)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _batch(device, arch, series, H=0, seed=17, n=N, t=T):
    from pymgrid_amd.generator import generate
    return generate(n, n_steps=t, seed=seed + 1000 * SOAK, arch=arch, device=device, horizon=H, mixed_timers=True,
                    series="factorised" if series == "factorised" else "materialised")


def _shaper(on):
    from pymgrid_amd import BatteryDischargeShaper
    return BatteryDischargeShaper() if on else None


def _actions(g, K, n, names, normalized, device, dtype=torch.float64):
    """[K, n, A] controls: normalised U[0, 1) draws with an edge value in about one entry in eight; normalized=False: raw requests
    in module units of both signs and beyond every limit (the goal column stays a goal), exact zeros among them."""
    A = len(names)
    u = torch.rand(K, n, A, device=device, generator=g, dtype=torch.float64)
    edge = torch.rand(K, n, A, device=device, generator=g) < 0.125
    which = torch.randint(0, len(EDGES), (K, n, A), device=device, generator=g)
    u = torch.where(edge, torch.tensor(EDGES, dtype=torch.float64, device=device)[which], u)
    if not normalized:
        raw = (u - 0.5) * 300.0
        goal = torch.tensor(["goal" in nm for nm in names], dtype=torch.bool, device=device)      # (bool also without a control)
        u = torch.where(goal, u, raw)
    return u.to(dtype).contiguous()


class HostStats:
    """The per-grid episode statistics by the rule of include/mgx.h, accumulated from single steps."""

    def __init__(self, n, device):
        self.run = torch.zeros(n, dtype=torch.float64, device=device)
        self.sum = torch.zeros_like(self.run)
        self.last = torch.zeros_like(self.run)
        self.eps = torch.zeros(n, dtype=torch.int32, device=device)

    def add(self, r, ended):
        self.run = self.run + r
        self.last = torch.where(ended, self.run, self.last)
        self.sum = torch.where(ended, self.sum + self.run, self.sum)
        self.eps = self.eps + ended.to(torch.int32)
        self.run = torch.where(ended, torch.zeros_like(self.run), self.run)

    def check(self, stats):
        assert torch.equal(stats["ret_running"], self.run)
        assert torch.equal(stats["ret_sum"], self.sum)
        assert torch.equal(stats["ret_last"], self.last)
        assert torch.equal(stats["episodes"], self.eps)


def _state_equal(a, b):
    for name in ("charge", "soc", "gen_status"):          # (gen_status: the packed status word, timers included)
        if name in b.batch.cols:
            assert torch.equal(a.batch.cols[name], b.batch.cols[name]), name


def _twin_steps(twin, controls, hs, want, walked=None, **step_kw):
    """K single steps of the final_observation=True twin: the per-step outputs the fused call offers, the rows, the rows before the
    restarts (of the grids with done set; NaN elsewhere, as the fused call's pre-filled buffer keeps them) + the host statistics.
    ``walked``: a list that receives every grid's series row before each step."""
    rows = {k: [] for k in ("reward", "done", "soc_trace", "status_trace", "obs", "final_obs")}
    cols = twin.env.batch.cols
    for k in range(controls.shape[0]):
        if walked is not None:
            walked.append(twin.env.current_steps.clone())
        o, r, d, info = twin.step(controls[k], **step_kw)
        rows["reward"].append(r.clone()); rows["done"].append(d.clone())
        rows["obs"].append(o.clone())
        fo = info["final_observation"]
        rows["final_obs"].append(torch.where(d[:, None], fo, torch.full_like(fo, float("nan"))))
        if "soc" in cols:
            rows["soc_trace"].append(cols["soc"].clone())
        if "gen_status" in cols:
            rows["status_trace"].append(cols["gen_status"].clone().view(torch.int32))
        hs.add(r, d)
    return {k: torch.stack(v) for k, v in rows.items() if v and k in want}


def _same_bits(a, b):
    """torch.equal with NaN == NaN of the same bits (the untouched entries of final_obs hold the NaN they were filled with)."""
    it = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _rows_equal_single_steps(device, discrete, arch, series, length, obs_dtype, shaper=False, per_step=True, normalized=True,
                             action_dtype=torch.float64, make_batch=None, trace=None):
    """The fused launch with rows, in launches of uneven size, == a final_observation=True twin stepped K times (same first draw, same
    seed).  ``make_batch(device, arch, series)``: the batch factory (default: ``_batch``, a generated batch of architecture ``arch``);
    ``trace``: a dict that receives what an independent replay needs -- the controls (and the priority-list table), the series rows
    the twin walked, the fused rewards and the state after the last launch."""
    from pymgrid_amd import _lib
    from pymgrid_amd.hetero import PerGridWindowEnv
    make_batch = make_batch or _batch
    old = _lib.get_tunable("grid_major_copy")[0]
    if series == "gather":
        _lib.set_tunable("grid_major_copy", 0)
    try:
        kw = dict(trajectory_length=length, discrete=discrete, auto_reset=True, seed=23 + SOAK, reward_shaping_func=_shaper(shaper),
                  obs_dtype=obs_dtype)
        if not discrete:
            kw["action_dtype"] = action_dtype
        fused = PerGridWindowEnv(make_batch(device, arch, series), **kw)
        twin = PerGridWindowEnv(make_batch(device, arch, series), final_observation=True, **kw)
        for e in (fused, twin):
            torch.manual_seed(41 + SOAK)                   # the same first draw
            e.obs0 = e.reset()
        assert torch.equal(fused.obs0, twin.obs0) and fused.obs0.dtype == obs_dtype
        g = torch.Generator(device=device); g.manual_seed(3 + SOAK)
        D = fused.env.engine.obs_dim
        hs = HostStats(N, device)
        if discrete:
            n_act = fused.env.action_space.n
            fixed = torch.randint(0, n_act, (N,), device=device, generator=g).to(torch.uint8)
        else:
            names = fused.env.layout.action_names
        restarts, twice, first, last = 0, False, False, False
        for K in LAUNCHES:
            bufs = dict(obs=torch.full((K, N, D), float("nan"), dtype=obs_dtype, device=device),
                        final_obs=torch.full((K, N, D), float("nan"), dtype=obs_dtype, device=device))
            walked = [] if trace is not None else None
            if discrete:
                ids = torch.randint(0, n_act, (K, N), device=device, generator=g).to(torch.uint8) if per_step else fixed.expand(K, N)
                out = fused.rollout(ids if per_step else fixed, K, reward=True, done=True, soc_trace=True, status_trace=True,
                                    observations=True, final_observations=True, out=bufs)
                ref = _twin_steps(twin, ids.to(torch.int32), hs, out, walked)
            else:
                actions = _actions(g, K, N, names, normalized, device, action_dtype)
                out = fused.step_k(actions, normalized=normalized, reward=True, done=True, soc_trace=True, status_trace=True,
                                   observations=True, final_observations=True, out=bufs)
                ref = _twin_steps(twin, actions, hs, out, walked, normalized=normalized)
            if trace is not None:
                trace["table"] = fused.env._table if discrete else None
                trace.setdefault("launches", []).append(dict(controls=ids.contiguous() if discrete else actions, rows=torch.stack(walked),
                                                             reward=out["reward"]))
            assert set(out) == set(ref) and {"obs", "final_obs", "done"} <= set(out), (sorted(out), sorted(ref))
            assert out["obs"] is bufs["obs"] and out["final_obs"] is bufs["final_obs"]
            d = out["done"]
            for name in out:
                if name in ("obs", "final_obs"):
                    continue
                assert out[name].shape == (K, N) and torch.equal(out[name], ref[name]), (K, name)
            assert torch.equal(out["obs"], ref["obs"]), K                       # (no NaN left: every row was written)
            assert _same_bits(out["final_obs"], ref["final_obs"]), K           # the rows before the restarts; NaN kept elsewhere
            assert bool(torch.isnan(out["final_obs"][~d]).all()) and not bool(torch.isnan(out["final_obs"][d]).any()), K
            assert torch.equal(fused.starts, twin.starts), K
            assert (fused.lengths is None) == (twin.lengths is None)
            if twin.lengths is not None:
                assert torch.equal(fused.lengths, twin.lengths), K
            assert torch.equal(fused.env.current_steps, twin.env.current_steps), K
            hs.check(fused.episode_stats)
            _state_equal(fused.env, twin.env)
            restarts += int(d.sum())
            twice |= bool((d.sum(dim=0) >= 2).any())
            if K > 1:
                first |= bool(d[0].any()); last |= bool(d[-1].any())
        # the test's own input: it cannot pass vacuously
        assert restarts > N and twice and first and last, (restarts, twice, first, last)
        assert int(fused.episode_stats["episodes"].sum()) == restarts
        if trace is not None:
            trace["state"] = {name: fused.env.batch.cols[name].clone() for name in ("charge", "soc", "gen_status") if name in fused.env.batch.cols}
        # the env stands where the twin stands: out["obs"][-1] is what the next step builds on, and the next step agrees
        if discrete:
            a = torch.randint(0, n_act, (N,), device=device, generator=g).to(torch.int32)
            (o1, r1, d1, _), (o2, r2, d2, _) = fused.step(a), twin.step(a)
        else:
            a = _actions(g, 1, N, names, normalized, device, action_dtype)[0]
            (o1, r1, d1, _), (o2, r2, d2, _) = fused.step(a, normalized=normalized), twin.step(a, normalized=normalized)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
        _state_equal(fused.env, twin.env)
        for e in (fused, twin):
            e.env.close()
    finally:
        _lib.set_tunable("grid_major_copy", old)


ARCHS = ["genset+battery+grid", "genset+battery", "battery+grid"]
SERIES = ["factorised", "materialised", "gather"]
DTYPES = [torch.float64, torch.float32]
ROLLOUT_CASES = list(itertools.product(ARCHS, SERIES, [9, None], DTYPES, [False, True], [False, True]))


@pytest.mark.gpu
@pytest.mark.parametrize("arch,series,length,obs_dtype,per_step,shaper", ROLLOUT_CASES)
def test_rollout_rows_equal_single_steps(arch, series, length, obs_dtype, per_step, shaper, device):
    """rollout(..., observations=True, final_observations=True) == step(ids[k]) K times on a final_observation=True twin."""
    _rows_equal_single_steps(device, True, arch, series, length, obs_dtype, shaper=shaper, per_step=per_step)


STEP_K_CASES = list(itertools.product(ARCHS, SERIES, [9, None], DTYPES, [torch.float64, torch.float32], [True, False]))


@pytest.mark.gpu
@pytest.mark.parametrize("arch,series,length,obs_dtype,action_dtype,normalized", STEP_K_CASES)
def test_step_k_rows_equal_single_steps(arch, series, length, obs_dtype, action_dtype, normalized, device):
    """step_k(..., observations=True, final_observations=True) == step(actions[k]) K times on a final_observation=True twin."""
    _rows_equal_single_steps(device, False, arch, series, length, obs_dtype, normalized=normalized, action_dtype=action_dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [True, False])
@pytest.mark.parametrize("series", ["factorised", "materialised"])
@pytest.mark.parametrize("arch", ARCHS)
def test_auto_reset_off_rows_walk_on(arch, series, discrete, device):
    """In-place episodes without set_auto_reset: the engine's fused calls with obs=True == single steps past the end of the series --
    rows beyond it show the padding value -- and final_obs stays untouched, nothing restarts."""
    from pymgrid_amd import BatchedMicrogridEnv, DiscreteBatchedMicrogridEnv
    n, t, K = 500, 60, 37
    cls = DiscreteBatchedMicrogridEnv if discrete else BatchedMicrogridEnv
    envs = [cls(_batch(device, arch, series, n=n, t=t)) for _ in range(2)]
    g = torch.Generator(device=device); g.manual_seed(9 + SOAK)
    starts = torch.randint(40, 52, (n,), device=device, generator=g).to(torch.int32)       # rows 60.. are beyond the series
    lengths = torch.randint(1, 9, (n,), device=device, generator=g).to(torch.int32)
    for e in envs:
        e.reset_windows(starts, lengths, max_length=8, rolling="inplace")
    fused, twin = envs
    D = fused.engine.obs_dim
    if discrete:
        ctl = torch.randint(0, fused.action_space.n, (K, n), device=device, generator=g).to(torch.uint8)
    else:
        ctl = _actions(g, K, n, fused.layout.action_names, True, device)
    obs, fin = [], []
    for lo, hi in ((0, 5), (5, 6), (6, K)):
        bufs = dict(final_obs=torch.full((hi - lo, n, D), float("nan"), dtype=torch.float64, device=device))
        if discrete:
            part = fused.engine.rollout_episodes(ctl[lo:hi].contiguous(), fused._table, hi - lo, reward=True, obs=True, final_obs=True,
                                                 out=bufs)
        else:
            part = fused.engine.step_k_episodes(ctl[lo:hi].contiguous(), reward=True, obs=True, final_obs=True, out=bufs)
        assert part["obs"].shape == (hi - lo, n, D) and part["final_obs"] is bufs["final_obs"]
        obs.append(part["obs"]); fin.append(part["final_obs"])
    obs, fin = torch.cat(obs), torch.cat(fin)
    beyond = 0
    for k in range(K):
        o = twin.step(ctl[k].to(torch.int32) if discrete else ctl[k])[0]
        assert torch.equal(obs[k], o), k
        beyond += int((starts.long() + k + 1 >= t).sum())
    assert beyond > n                                          # most rows of the later steps are padding
    assert bool(torch.isnan(fin).all())                        # nothing restarted: not a byte of final_obs written
    assert fused.engine.current_step == twin.engine.current_step == K
    _state_equal(fused, twin)
    for e in envs:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [True, False])
def test_rows_then_no_rows_leaves_the_env_where_the_plain_launch_does(discrete, device):
    """A launch with rows, then a launch without, against a twin that never asks for rows: per-step outputs, statistics, episode
    arrays and state identical -- the rows kernel leaves what the plain kernel leaves."""
    from pymgrid_amd.hetero import PerGridWindowEnv
    kw = dict(trajectory_length=9, discrete=discrete, auto_reset=True, seed=23 + SOAK)
    a, b = (PerGridWindowEnv(_batch(device, "genset+battery+grid", "factorised"), **kw) for _ in range(2))
    for e in (a, b):
        torch.manual_seed(41 + SOAK)
        e.reset()
    g = torch.Generator(device=device); g.manual_seed(3 + SOAK)
    want = dict(reward=True, done=True, soc_trace=True, status_trace=True)
    for K, rows in ((40, True), (23, False), (9, True)):
        if discrete:
            ctl = torch.randint(0, a.env.action_space.n, (K, N), device=device, generator=g).to(torch.uint8)
            oa = a.rollout(ctl, observations=rows, final_observations=rows, **want)
            ob = b.rollout(ctl, **want)
        else:
            ctl = _actions(g, K, N, a.env.layout.action_names, True, device)
            oa = a.step_k(ctl, observations=rows, final_observations=rows, **want)
            ob = b.step_k(ctl, **want)
        assert set(oa) - set(ob) == ({"obs", "final_obs"} if rows else set())
        for name in ob:
            assert torch.equal(oa[name], ob[name]), (K, name)
        if rows:                                               # an allocated final_obs is zero-filled outside the restarts
            assert bool((oa["final_obs"][~oa["done"]] == 0).all()) and bool(oa["done"].any())
        for name in b.episode_stats:
            assert torch.equal(a.episode_stats[name], b.episode_stats[name]), (K, name)
        assert torch.equal(a.starts, b.starts) and torch.equal(a.env.current_steps, b.env.current_steps)
        _state_equal(a.env, b.env)
    for e in (a, b):
        e.env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [True, False])
def test_fleet_rows_equal_its_twins(discrete, device):
    """PerGridWindowFleet.rollout / step_k pass observations= / final_observations= through: bucket k == its PerGridWindowEnv twin
    with seed=fleet.seeds[k]."""
    from pymgrid_amd.generator import generate_fleet
    from pymgrid_amd.hetero import PerGridWindowEnv, PerGridWindowFleet

    def parts():
        return [b for b, _ in generate_fleet(3000, n_steps=200, seed=29 + 1000 * SOAK, horizon=0, device=device).values()]
    kw = dict(trajectory_length=9, discrete=discrete, auto_reset=True)
    fleet = PerGridWindowFleet.from_batches(parts(), seed=3 + SOAK, **kw)
    twins = [PerGridWindowEnv(b, **dict(kw, seed=fleet.seeds[k])) for k, b in enumerate(parts())]
    assert len(twins) >= 3
    torch.manual_seed(61 + SOAK)
    of = fleet.reset()
    torch.manual_seed(61 + SOAK)
    for b, tw in enumerate(twins):
        assert torch.equal(of[b], tw.reset()), b
    g = torch.Generator(device=device); g.manual_seed(5 + SOAK)
    for K in (3, 40):
        if discrete:
            ctl = [torch.randint(0, pe.env.action_space.n, (K, pe.n_grids), device=device, generator=g).to(torch.uint8) for pe in fleet.envs]
            outs = fleet.rollout(ctl, reward=True, done=True, observations=True, final_observations=True)
        else:
            ctl = [_actions(g, K, pe.n_grids, pe.env.layout.action_names, True, device) for pe in fleet.envs]
            outs = fleet.step_k(ctl, reward=True, done=True, observations=True, final_observations=True)
        for b, tw in enumerate(twins):
            call = tw.rollout if discrete else tw.step_k
            ref = call(ctl[b], reward=True, done=True, observations=True, final_observations=True)
            assert set(outs[b]) == set(ref) == {"reward", "done", "obs", "final_obs"}
            assert outs[b]["obs"].shape == (K, tw.n_grids, tw.env.engine.obs_dim)
            for name in ref:
                assert torch.equal(outs[b][name], ref[name]), (K, b, name)
            _state_equal(fleet.envs[b].env, tw.env)
    fleet.close()
    for tw in twins:
        tw.env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("series", ["factorised", "materialised"])
def test_rule_based_control_returns_the_trajectory(series, device):
    """RuleBasedControl.run_episodes(steps=200, chunk=64, observations=True, final_observations=True, done=True) == the env stepped 200
    times with the same lists: the rows of the chunks concatenated like the other per-step outputs."""
    from pymgrid_amd import RuleBasedControl
    from pymgrid_amd.hetero import PerGridWindowEnv
    steps = 200
    kw = dict(trajectory_length=9, discrete=True, auto_reset=True, seed=5 + SOAK)
    roll = PerGridWindowEnv(_batch(device, "genset+battery+grid", series), **kw)
    twin = PerGridWindowEnv(_batch(device, "genset+battery+grid", series), final_observation=True, **kw)
    rbc = RuleBasedControl(roll)
    torch.manual_seed(77 + SOAK)
    res = rbc.run_episodes(steps=steps, chunk=64, observations=True, final_observations=True, done=True)
    D = roll.env.engine.obs_dim
    assert res["obs"].shape == res["final_obs"].shape == (steps, N, D) and res["done"].shape == (steps, N)
    torch.manual_seed(77 + SOAK)
    twin.reset()
    ids = torch.from_numpy(rbc.priority_ids.astype(np.int32)).to(device)
    for k in range(steps):
        o, _, d, info = twin.step(ids)
        assert torch.equal(res["done"][k], d), k
        assert torch.equal(res["obs"][k], o), k
        assert torch.equal(res["final_obs"][k][d], info["final_observation"][d]), k
        assert bool((res["final_obs"][k][~d] == 0).all()), k
    assert int(res["episodes"].min()) >= steps // 9 - 1
    assert torch.equal(roll.starts, twin.starts)
    _state_equal(roll.env, twin.env)
    for e in (roll, twin):
        e.env.close()


def _snapshot(env, stats=None):
    cols = env.batch.cols
    snap = {name: cols[name].clone() for name in ("charge", "soc", "gen_status") if name in cols}
    snap["t"] = env.engine._lib.mgx_current_step(env.engine._h)
    for name, v in (stats or {}).items():
        snap["stat_" + name] = v.clone()
    return snap


def _untouched(env, snap, stats=None):
    now = _snapshot(env, stats)
    assert now.keys() == snap.keys()
    for name, v in snap.items():
        assert torch.equal(now[name], v) if torch.is_tensor(v) else now[name] == v, name


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [True, False])
def test_refusals_of_the_c_abi(discrete, device):
    """The calls with rows refuse -- before anything is launched -- a forecast horizon, a state-only observation mode, a set
    final-observation buffer (MGX_ERR_UNSUPPORTED), a wrong struct_size (MGX_ERR_INVALID), a lock-step handle (MGX_ERR_INVALID) and
    several modules of a kind (MGX_ERR_UNSUPPORTED); the plain calls still refuse what they refused."""
    import ctypes as C
    from pymgrid_amd import BatchedMicrogridEnv, DiscreteBatchedMicrogridEnv, MgxError, _lib
    from pymgrid_amd.engine import _ptr
    from pymgrid_amd.generator import generate, widen
    cls = DiscreteBatchedMicrogridEnv if discrete else BatchedMicrogridEnv
    n, K = 300, 5
    starts = torch.zeros(n, dtype=torch.int32, device=device)

    def control(env):
        if discrete:
            return torch.zeros(K, n, dtype=torch.uint8, device=device)
        return torch.zeros(K, n, env.engine.action_dim, dtype=torch.float64, device=device)

    def launch(env, **kw):
        e = env.engine
        if discrete:
            table = kw.pop("table", None)
            return e.rollout_episodes(control(env), env._table if table is None else table, K, **kw)
        kw.pop("table", None)
        return e.step_k_episodes(control(env), **kw)

    def refused(env, code, stats=None, **kw):
        snap = _snapshot(env, stats)
        rows = torch.full((K, n, env.engine.obs_dim), float("nan"), dtype=env.engine.obs_dtype, device=device)
        with pytest.raises(MgxError) as ei:
            launch(env, stats=stats, out=dict(obs=rows, final_obs=rows.clone()), **kw)
        assert ei.value.code == code, ei.value
        assert ("mgx_rollout_episodes" if discrete else "mgx_step_k_episodes") in str(ei.value)
        _untouched(env, snap, stats)
        assert bool(torch.isnan(rows).all())
    # a forecast horizon
    from pymgrid_amd.hetero import PerGridWindowEnv
    pe = PerGridWindowEnv(_batch(device, "genset+battery+grid", "factorised", H=6, n=n, t=60), trajectory_length=9, discrete=discrete,
                          auto_reset=True, seed=2)
    pe.reset()
    refused(pe.env, _lib.MGX_ERR_UNSUPPORTED, obs=True)
    pe.env.close()
    env = cls(_batch(device, "genset+battery+grid", "factorised", n=n, t=60))
    e = env.engine
    stats = {name: torch.full((n,), 3, dtype=dt, device=device) for name, dt in e.EPISODE_STATS}
    env.reset()
    refused(env, _lib.MGX_ERR_INVALID, stats, obs=True)        # lock-step episode
    env.reset_windows(starts, None, max_length=9, rolling="inplace")
    # state-only observation mode
    _lib.check(e._lib.mgx_set_obs_mode(e._h, 1))
    refused(env, _lib.MGX_ERR_UNSUPPORTED, stats, obs=True, final_obs=True)
    _lib.check(e._lib.mgx_set_obs_mode(e._h, 0))
    # mgx_set_final_obs set: refused with rows and without
    e.set_final_obs(torch.zeros(n, e.obs_dim, dtype=torch.float64, device=device))
    refused(env, _lib.MGX_ERR_UNSUPPORTED, stats, final_obs=True)
    snap = _snapshot(env, stats)
    with pytest.raises(MgxError) as ei:
        launch(env, stats=stats)
    assert ei.value.code == _lib.MGX_ERR_UNSUPPORTED
    _untouched(env, snap, stats)
    e.set_final_obs(None)
    # a wrong struct_size (the C call itself: the binding always fills it in)
    rows = _lib.EpisodeRows()
    rows.struct_size = C.sizeof(_lib.EpisodeRows) - 8
    buf = torch.full((K, n, e.obs_dim), float("nan"), dtype=torch.float64, device=device)
    rows.obs = _ptr(buf)
    ctl = control(env)
    snap = _snapshot(env, stats)
    if discrete:
        tptr, n_lists = e._table_ptr(env._table)
        rc = e._lib.mgx_rollout_episodes_rows(e._h, _ptr(ctl), 1, tptr, n_lists, K, None, None, None, None, None, C.byref(rows), None)
    else:
        rc = e._lib.mgx_step_k_episodes_rows(e._h, _ptr(ctl), K, 1, None, None, None, None, None, C.byref(rows), None)
    assert rc == _lib.MGX_ERR_INVALID and b"struct_size" in e._lib.mgx_last_error()
    torch.cuda.synchronize()
    _untouched(env, snap, stats)
    assert bool(torch.isnan(buf).all())
    # ... and the handle is taken once nothing stands in the way; rows NULL / both pointers NULL is the plain call
    out = launch(env, stats=stats, obs=True, final_obs=True)
    assert out["obs"].shape == (K, n, e.obs_dim) and e.current_step == K
    rows.struct_size = 0                                       # (not looked at: no rows asked for)
    rows.obs = None
    if discrete:
        rc = e._lib.mgx_rollout_episodes_rows(e._h, _ptr(ctl), 1, tptr, n_lists, K, None, None, None, None, None, C.byref(rows), None)
    else:
        rc = e._lib.mgx_step_k_episodes_rows(e._h, _ptr(ctl), K, 1, None, None, None, None, None, None, None)
    assert rc == _lib.MGX_OK and e._lib.mgx_current_step(e._h) == 2 * K
    env.close()
    # several modules of a kind
    wide = widen(generate(n, n_steps=60, seed=4, arch="genset+battery", device=device), n_battery=2)
    env = cls(wide)
    env.reset_windows(starts, None, max_length=9, rolling="inplace")
    refused(env, _lib.MGX_ERR_UNSUPPORTED, obs=True, table=np.zeros((1, 3, 2), dtype=np.int32))
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [True, False])
def test_refusals_of_the_python_surface(discrete, device):
    """PerGridWindowEnv.rollout / step_k with observations: ValueError that says which option stands in the way (a horizon,
    observation_keys; final_observation=True and obs_views stay refused as without rows), nothing launched; the same env takes the
    call without rows where only the rows are in the way."""
    from pymgrid_amd.hetero import PerGridWindowEnv, PerGridWindowFleet
    n, K = 300, 4

    def batch(h=0):
        return _batch(device, "genset+battery", "factorised", H=h, n=n, t=60)

    def call(pe, **kw):
        if discrete:
            return pe.rollout(torch.zeros(K, n, dtype=torch.uint8, device=device), **kw)
        return pe.step_k(torch.zeros(K, n, pe.env.engine.action_dim, dtype=torch.float64, device=device), **kw)
    cases = [("horizon", {}, batch(6), True), ("observation_keys", dict(observation_keys=["load_current", "soc"]), batch(), True),
             ("final_observation", dict(final_observation=True), batch(), False), ("obs_views", dict(obs_views=True), batch(6), False)]
    for word, kw, b, plain_ok in cases:
        pe = PerGridWindowEnv(b, trajectory_length=9, discrete=discrete, auto_reset=True, seed=2, **kw)
        if word != "obs_views":                            # (views are not offered for rolling windows at all: nothing to reset)
            pe.reset()
        for rows in (dict(observations=True), dict(final_observations=True)):
            snap = _snapshot(pe.env)
            with pytest.raises(ValueError, match=word):
                call(pe, **rows)
            _untouched(pe.env, snap)
        if word == "horizon":
            fleet = PerGridWindowFleet.from_batches([batch(), b], trajectory_length=9, discrete=discrete, auto_reset=True, seed=2)
            fleet.reset()
            snaps = [_snapshot(q.env) for q in fleet.envs]
            ctl = [torch.zeros(K, n, dtype=torch.uint8, device=device) if discrete else
                   torch.zeros(K, n, q.env.engine.action_dim, dtype=torch.float64, device=device) for q in fleet.envs]
            with pytest.raises(ValueError, match=word):
                (fleet.rollout if discrete else fleet.step_k)(ctl, observations=True)
            for q, s in zip(fleet.envs, snaps):
                _untouched(q.env, s)
            fleet.close()
        if plain_ok:
            assert pe.episode_stats is None
            assert call(pe)["reward"].shape == (K, n)
        else:
            with pytest.raises(ValueError, match=word):
                call(pe)
        pe.env.close()
