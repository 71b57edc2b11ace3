"""The fused continuous K-step over per-grid in-place episodes (mgx_step_k_episodes / StepEngine.step_k_episodes /
PerGridWindowEnv.step_k / PerGridWindowFleet.step_k): K steps of Microgrid.run(control, normalized) in one launch, restarts inside
it, == the same env stepped K times with step(actions[k]) -- rewards, done flags, traces, episode starts / lengths, per-grid
counters, module state, the per-grid episode statistics and the next step's observation, bit for bit (torch.equal on fp64: same
arithmetic, same order)."""
import itertools
import os

import numpy as np
import pytest
import torch

SOAK = int(os.environ.get("MGX_FUZZ_SEED", "0"))          # soak runs: another draw of every batch / episode / action sequence
N, T = 1000, 150
LAUNCHES = (1, 7, 64, 64, 130)          # K = 1, a K that is no multiple of a ring depth (4 / 8), 64-step launches, one above 128
KERNEL = "step_k_episodes_kernel"
EDGES = (0.0, 0.5, 1.0, -0.25, 1.3)     # exact-zero routing, the genset goal's round-half-to-even point, clipping on both sides


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_the_minor_stays():
    """mgx_step_k_episodes is an addition found by name: exported, declared in the header, bound; the ABI minor stays 3, no tunable
    is added; a NULL handle is MGX_ERR_INVALID and the message names the call."""
    import ctypes as C
    from pymgrid_amd import _lib
    _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    assert L.mgx_step_k_episodes is not None
    assert "mgx_step_k_episodes" in _lib.SYMBOLS
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mgx.h")
    with open(header) as fh:
        assert "int mgx_step_k_episodes(mgx_handle *h, const void *actions, int32_t K, int normalized" in fh.read()
    lib = _lib.lib()
    assert lib.mgx_abi_minor() == 3 == _lib.ABI_MINOR
    assert len(_lib.TUNABLES) == 12
    rc = lib.mgx_step_k_episodes(None, None, 4, 1, None, None, None, None, None, None)
    assert rc == _lib.MGX_ERR_INVALID
    assert b"mgx_step_k_episodes" in lib.mgx_last_error()


def test_step_k_episodes_kernel_spills_nothing():
    """Every instantiation of step_k_episodes_kernel: no scratch memory, no spilled scalar or vector registers; all ten layouts
    (the one without a controllable module included, as mgx_step_k treats it), float64 and float32 controls, the three row sources."""
    from pymgrid_amd import _lib
    _lib.build()
    usage = _lib.resource_usage()
    if usage is None:
        pytest.skip("libmgx.so was not built on this machine (no resource_usage.json beside the objects)")
    forms = {name: u for name, u in usage.items() if name.split("<")[0].split("::")[-1] == KERNEL}
    assert len(forms) == 10 * 2 * 3, sorted(forms)
    for name, u in forms.items():
        assert u.get("scratch", 0) == 0 and u.get("vgpr_spill", 0) == 0 and u.get("sgpr_spill", 0) == 0, (name, u)
        assert u["vgpr"] <= 256, (name, u)                # two waves per SIMD


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _batch(device, arch, series, H, seed=17, n=N, t=T):
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
        raw = (u - 0.5) * 300.0                           # -225 .. 240 energy units; u == 0.5 -> exactly 0
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


def _twin_steps(twin, actions, normalized, hs, want, walked=None):
    """K single steps of the twin: the per-step outputs the fused call offers + the host statistics.  ``walked``: a list that receives
    every grid's series row before each step."""
    rows = {k: [] for k in ("reward", "done", "soc_trace", "status_trace")}
    cols = twin.env.batch.cols
    for k in range(actions.shape[0]):
        if walked is not None:
            walked.append(twin.env.current_steps.clone())
        _, r, d, _ = twin.step(actions[k], normalized=normalized)
        rows["reward"].append(r.clone()); rows["done"].append(d.clone())
        if "soc" in cols:
            rows["soc_trace"].append(cols["soc"].clone())
        if "gen_status" in cols:
            rows["status_trace"].append(cols["gen_status"].clone().view(torch.int32))
        hs.add(r, d)
    return {k: torch.stack(v) for k, v in rows.items() if v and k in want}


def _fused_equals_single_steps(device, arch, series, length, H, shaper, normalized, dtype=torch.float64, make_batch=None, trace=None):
    """``make_batch(device, arch, series, H)``: the batch factory (default: ``_batch``, a generated batch of architecture ``arch``);
    ``trace``: a dict that receives what an independent replay needs -- the controls, the series rows the twin walked, the fused
    rewards and the state after the last launch."""
    from pymgrid_amd import _lib
    make_batch = make_batch or _batch
    from pymgrid_amd.hetero import PerGridWindowEnv
    old = _lib.get_tunable("grid_major_copy")[0]
    if series == "gather":
        _lib.set_tunable("grid_major_copy", 0)
    try:
        envs = [PerGridWindowEnv(make_batch(device, arch, series, H), trajectory_length=length, discrete=False, auto_reset=True,
                                 seed=23 + SOAK, reward_shaping_func=_shaper(shaper), action_dtype=dtype) for _ in range(2)]
        fused, twin = envs
        for e in envs:
            torch.manual_seed(41 + SOAK)                   # the same first draw
            e.obs0 = e.reset()
        assert torch.equal(fused.obs0, twin.obs0)
        assert fused.env.engine._lib.mgx_current_step(fused.env.engine._h) == 0
        g = torch.Generator(device=device); g.manual_seed(3 + SOAK)
        names = fused.env.layout.action_names
        hs = HostStats(N, device)
        restarts, twice, first, last = 0, False, False, False
        for K in LAUNCHES:
            actions = _actions(g, K, N, names, normalized, device, dtype)
            out = fused.step_k(actions, normalized=normalized, reward=True, done=True, soc_trace=True, status_trace=True)
            walked = [] if trace is not None else None
            ref = _twin_steps(twin, actions, normalized, hs, out, walked)
            if trace is not None:
                trace.setdefault("launches", []).append(dict(controls=actions, rows=torch.stack(walked), reward=out["reward"]))
            assert set(out) == set(ref), (sorted(out), sorted(ref))
            for name in out:
                assert out[name].shape == (K, N) and torch.equal(out[name], ref[name]), (K, name)
            assert torch.equal(fused.starts, twin.starts), K
            assert (fused.lengths is None) == (twin.lengths is None)
            if twin.lengths is not None:
                assert torch.equal(fused.lengths, twin.lengths), K
            assert torch.equal(fused.env.current_steps, twin.env.current_steps), K
            hs.check(fused.episode_stats)
            _state_equal(fused.env, twin.env)
            d = out["done"]
            restarts += int(d.sum())
            twice |= bool((d.sum(dim=0) >= 2).any())
            if K > 1:
                first |= bool(d[0].any()); last |= bool(d[-1].any())
        # the test's own input: it cannot pass vacuously
        assert restarts > N and twice and first and last, (restarts, twice, first, last)
        assert int(fused.episode_stats["episodes"].sum()) == restarts
        if trace is not None:
            trace["state"] = {name: fused.env.batch.cols[name].clone() for name in ("charge", "soc", "gen_status") if name in fused.env.batch.cols}
        a = _actions(g, 1, N, names, normalized, device, dtype)[0]
        (o1, r1, d1, _), (o2, r2, d2, _) = fused.step(a, normalized=normalized), twin.step(a, normalized=normalized)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
        _state_equal(fused.env, twin.env)
        for e in envs:
            e.env.close()
    finally:
        _lib.set_tunable("grid_major_copy", old)


CASES = list(itertools.product(["genset+battery+grid", "genset+battery", "battery+grid"], ["factorised", "materialised", "gather"],
                               [9, None], [0, 6], [False, True], [True, False]))


@pytest.mark.gpu
@pytest.mark.parametrize("arch,series,length,H,shaper,normalized", CASES)
def test_step_k_equals_single_steps(arch, series, length, H, shaper, normalized, device):
    """step_k(actions) in launches of uneven size == step(actions[k]) K times on a twin env with the same first draw and seed."""
    _fused_equals_single_steps(device, arch, series, length, H, shaper, normalized)


@pytest.mark.gpu
@pytest.mark.parametrize("series", ["factorised", "materialised"])
def test_float32_actions(series, device):
    """The same comparison with action_dtype=torch.float32 on both envs (mgx_set_action_format: widened when the step consumes them)."""
    _fused_equals_single_steps(device, "genset+battery+grid", series, None, 0, False, True, dtype=torch.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("series", ["factorised", "materialised"])
@pytest.mark.parametrize("arch", ["genset+battery+grid", "genset+battery", "battery+grid"])
def test_auto_reset_off_walks_on(arch, series, device):
    """In-place episodes without set_auto_reset: engine.step_k_episodes == single steps past the end of the episodes (clamped rows);
    `episodes` counts a grid once, when it crosses its final step."""
    from pymgrid_amd import BatchedMicrogridEnv
    n, K = 500, 37
    envs = [BatchedMicrogridEnv(_batch(device, arch, series, 0, n=n, t=60)) for _ in range(2)]
    g = torch.Generator(device=device); g.manual_seed(9 + SOAK)
    starts = torch.randint(40, 52, (n,), device=device, generator=g).to(torch.int32)       # rows 60.. are beyond the series: clamped
    lengths = torch.randint(1, 9, (n,), device=device, generator=g).to(torch.int32)
    for e in envs:
        e.reset_windows(starts, lengths, max_length=8, rolling="inplace")
    fused, twin = envs
    actions = _actions(g, K, n, fused.layout.action_names, True, device)
    stats = {name: torch.zeros(n, dtype=dt, device=device) for name, dt in fused.engine.EPISODE_STATS}
    hs = HostStats(n, device)
    out = {}
    for lo, hi in ((0, 5), (5, 6), (6, K)):
        part = fused.engine.step_k_episodes(actions[lo:hi].contiguous(), reward=True, done=True, stats=stats)
        for k_, v in part.items():
            out.setdefault(k_, []).append(v)
    out = {k_: torch.cat(v) for k_, v in out.items()}
    prev = torch.zeros(n, dtype=torch.bool, device=device)
    for k in range(K):
        _, r, d, _ = twin.step(actions[k])
        assert torch.equal(out["reward"][k], r) and torch.equal(out["done"][k].view(torch.bool), d), k
        hs.add(r, d & ~prev)                               # the crossing of the final step
        prev = d
    hs.check(stats)
    assert int(stats["episodes"].max()) == 1 and int(stats["episodes"].min()) == 1 and bool(prev.all())
    assert bool((starts.long() + K > 60).any())            # some grids did walk past the series
    assert fused.engine.current_step == twin.engine.current_step == K
    _state_equal(fused, twin)
    for e in envs:
        e.close()


def _grid(rs, t):
    return dict(load_ts=80 * rs.rand(t) + 5, pv_ts=60 * rs.rand(t) * (rs.rand(t) > 0.3), horizon=0, final_step=t, initial_step=0,
                unbalanced=dict(loss_load_cost=10.0, overgeneration_cost=1.0 + rs.rand()), controllable_order=["genset", "battery", "grid"],
                genset=dict(running_min_production=float(rs.choice([5.0, 12.0])), running_max_production=40.0 + 40 * rs.rand(),
                            genset_cost=0.3 + 0.3 * rs.rand(), co2_per_unit=2.0, cost_per_unit_co2=0.1, start_up_time=int(rs.randint(0, 3)),
                            wind_down_time=int(rs.randint(0, 3)), init_start_up=bool(rs.randint(0, 2))),
                battery=dict(min_capacity=10.0, max_capacity=60.0 + 80 * rs.rand(), max_charge=20.0 + 10 * rs.rand(), max_discharge=25.0,
                             efficiency=1.0, battery_cost_cycle=0.02 * rs.rand(), init_soc=0.3 + 0.6 * rs.rand()),
                grid=dict(max_import=30.0 + 40 * rs.rand(), max_export=20.0 + 30 * rs.rand(), cost_per_unit_co2=0.1),
                grid_ts=np.stack([0.1 + rs.rand(t), 0.5 * rs.rand(t), 0.3 * rs.rand(t), (rs.rand(t) > 0.2).astype(float)], axis=1))


@pytest.mark.gpu
def test_step_k_episode_returns_vs_the_oracle(device, oracle):
    """48 hand-built grids, normalised continuous controls over 20 steps of 6-step episodes in launches of 7 (every grid restarts at
    least twice): per step reward == the CPU oracle's run(control, normalized=True) replay of every grid's episodes (a restart moves
    the counter and keeps the state), and the per-episode returns / final charge equal the oracle's.  The episode starts come from a
    single-stepped twin (equal to the fused env by the tests above)."""
    from pymgrid_amd import MicrogridBatch
    from pymgrid_amd.hetero import PerGridWindowEnv
    n, t, length, steps, chunk = 48, 40, 6, 20, 7
    rs = np.random.RandomState(31 + SOAK)
    grids = [_grid(rs, t) for _ in range(n)]
    envs = [PerGridWindowEnv(MicrogridBatch.from_grids(grids, device=device), trajectory_length=length, discrete=False, auto_reset=True,
                             seed=13 + SOAK) for _ in range(2)]
    fused, twin = envs
    names = fused.env.layout.action_names
    assert names == ["genset_goal_status", "genset_energy", "battery", "grid"]
    g = torch.Generator(device=device); g.manual_seed(6 + SOAK)
    actions = _actions(g, steps, n, names, True, device)
    for e in envs:
        torch.manual_seed(8 + SOAK)
        e.reset()
    parts = [fused.step_k(actions[lo:lo + chunk].contiguous(), reward=True, done=True) for lo in range(0, steps, chunk)]
    reward = torch.cat([p["reward"] for p in parts]).cpu().numpy()
    done = torch.cat([p["done"] for p in parts]).cpu().numpy()
    assert reward.shape == (steps, n)
    episodes = [[int(s)] for s in twin.starts.cpu().numpy()]
    for k in range(steps):
        _, _, d, _ = twin.step(actions[k])
        s = twin.starts.cpu().numpy()
        for j in np.flatnonzero(d.cpu().numpy()):
            episodes[j].append(int(s[j]))
    assert min(len(e) for e in episodes) >= 3               # every grid restarts at least twice
    st = {k_: v.cpu().numpy() for k_, v in fused.episode_stats.items()}
    acts = actions.cpu().numpy()
    for j, gp in enumerate(grids):
        om = oracle.OracleMicrogrid(gp)
        ep = iter(episodes[j])
        om.reset(next(ep))
        n_left, run, total, last, cnt = length, 0.0, 0.0, 0.0, 0
        for k in range(steps):
            a = acts[k, j]
            r = om.run(dict(genset=[a[0], a[1]], battery=a[2], grid=a[3]), normalized=True).reward
            assert reward[k, j] == r, (j, k)
            run += r
            n_left -= 1
            assert bool(done[k, j]) == (n_left == 0), (j, k)
            if n_left == 0:
                last = run; total += run; cnt += 1; run = 0.0
                om.reset(next(ep)); n_left = length
        assert (st["ret_sum"][j], st["ret_last"][j], st["ret_running"][j], st["episodes"][j]) == (total, last, run, cnt), j
        assert fused.env.batch.cols["charge"][j].item() == om.s.charge, j
    for e in envs:
        e.env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("length", [9, None])
def test_fleet_step_k_equals_its_twins(length, device):
    """PerGridWindowFleet.step_k, bucket by bucket == the per-bucket PerGridWindowEnv twins' step_k."""
    from pymgrid_amd.generator import generate_fleet
    from pymgrid_amd.hetero import PerGridWindowEnv, PerGridWindowFleet

    def parts():
        return [b for b, _ in generate_fleet(3000, n_steps=200, seed=29 + 1000 * SOAK, horizon=0, device=device).values()]
    kw = dict(trajectory_length=length, discrete=False, auto_reset=True)
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
        acts = [_actions(g, K, pe.n_grids, pe.env.layout.action_names, True, device) for pe in fleet.envs]
        outs = fleet.step_k(acts, reward=True, done=True, soc_trace=True)
        for b, tw in enumerate(twins):
            ref = tw.step_k(acts[b], reward=True, done=True, soc_trace=True)
            assert set(outs[b]) == set(ref)
            for name in ref:
                assert torch.equal(outs[b][name], ref[name]), (K, b, name)
            assert torch.equal(fleet.envs[b].starts, tw.starts) and torch.equal(fleet.current_steps[b], tw.env.current_steps)
            for name in tw.episode_stats:
                assert torch.equal(fleet.envs[b].episode_stats[name], tw.episode_stats[name]), (K, b, name)
            _state_equal(fleet.envs[b].env, tw.env)
    acts = [_actions(g, 1, pe.n_grids, pe.env.layout.action_names, True, device)[0] for pe in fleet.envs]
    of, rf, df, _ = fleet.step(acts)
    for b, tw in enumerate(twins):
        ot, rt, dt, _ = tw.step(acts[b])
        assert torch.equal(of[b], ot) and torch.equal(rf[b], rt) and torch.equal(df[b], dt), b
    with pytest.raises(ValueError):
        fleet.step_k(acts[:1])                              # one entry per bucket
    fleet.close()
    for tw in twins:
        tw.env.close()


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
def test_refusals_of_the_c_abi(device):
    """mgx_step_k_episodes refuses -- before anything is launched -- a handle that is not in in-place episodes (MGX_ERR_INVALID),
    several modules of a kind, shards, device-counter mode, `done` as bit sets and a set final-observation buffer
    (MGX_ERR_UNSUPPORTED); step_k keeps refusing in-place handles."""
    from pymgrid_amd import BatchedMicrogridEnv, MgxError, _lib
    from pymgrid_amd.generator import generate, widen
    n, K = 300, 5
    env = BatchedMicrogridEnv(_batch(device, "genset+battery+grid", "factorised", 0, n=n, t=60))
    e = env.engine
    actions = torch.full((K, n, e.action_dim), 0.5, dtype=torch.float64, device=device)
    stats = {name: torch.full((n,), 3, dtype=dt, device=device) for name, dt in e.EPISODE_STATS}

    def refused(code, **kw):
        snap = _snapshot(env, stats)
        with pytest.raises(MgxError) as ei:
            e.step_k_episodes(actions, stats=stats, **kw)
        assert ei.value.code == code, ei.value
        assert "mgx_step_k_episodes" in str(ei.value)
        _untouched(env, snap, stats)
    env.reset()
    refused(_lib.MGX_ERR_INVALID)                                            # lock-step episode
    starts = torch.zeros(n, dtype=torch.int32, device=device)
    env.reset_windows(starts, None, max_length=9)
    refused(_lib.MGX_ERR_INVALID)                                            # gathered windows
    env.reset_windows(starts, None, max_length=9, rolling=True)
    refused(_lib.MGX_ERR_INVALID)                                            # rolling window buffers
    env.reset_windows(starts, None, max_length=9, rolling="inplace")
    e.set_final_obs(torch.zeros(n, e.obs_dim, dtype=torch.float64, device=device))
    refused(_lib.MGX_ERR_UNSUPPORTED)                                        # final observations
    e.set_final_obs(None)
    e.set_done_format(True)
    refused(_lib.MGX_ERR_UNSUPPORTED, done=True)                             # done as bit sets
    e.set_done_format(False)
    snap = _snapshot(env, stats)
    with pytest.raises(MgxError):                                            # the lock-step fused call still refuses the handle
        e.step_k(actions)
    _untouched(env, snap, stats)
    out = e.step_k_episodes(actions, stats=stats)                            # ... and the new one takes it
    assert out["reward"].shape == (K, n) and e.current_step == K
    env.close()
    # shards / device counter: the handle cannot enter in-place episodes there, so the call meets a handle that is not in place
    for setup in ("shards", "counter"):
        env2 = BatchedMicrogridEnv(_batch(device, "genset+battery", "factorised", 0, n=n, t=60))
        e2 = env2.engine
        env2.reset()
        if setup == "shards":
            e2.set_shards(2)
        else:
            e2.use_device_counter(True)
        snap = _snapshot(env2)
        with pytest.raises(MgxError) as ei:
            e2.step_k_episodes(torch.full((K, n, e2.action_dim), 0.5, dtype=torch.float64, device=device))
        assert ei.value.code == _lib.MGX_ERR_UNSUPPORTED, ei.value
        _untouched(env2, snap)
        env2.close()
    # several modules of a kind
    wide = widen(generate(n, n_steps=60, seed=4, arch="genset+battery", device=device), n_battery=2)
    env3 = BatchedMicrogridEnv(wide)
    env3.reset_windows(starts, None, max_length=9, rolling="inplace")
    snap = _snapshot(env3)
    with pytest.raises(MgxError) as ei:
        env3.engine.step_k_episodes(torch.full((K, n, env3.engine.action_dim), 0.5, dtype=torch.float64, device=device))
    assert ei.value.code == _lib.MGX_ERR_UNSUPPORTED, ei.value
    _untouched(env3, snap)
    env3.close()


@pytest.mark.gpu
def test_refusals_of_the_python_surface(device):
    """PerGridWindowEnv.step_k / PerGridWindowFleet.step_k: ValueError that says which option stands in the way, nothing launched."""
    from pymgrid_amd.generator import generate, widen
    from pymgrid_amd.hetero import PerGridWindowEnv, PerGridWindowFleet
    n, K = 300, 4

    def batch(h=0):
        return _batch(device, "genset+battery", "factorised", h, n=n, t=60)

    def acts(pe, dtype=torch.float64, extra=0):
        return torch.full((K, n, pe.env.engine.action_dim + extra), 0.5, dtype=dtype, device=device)
    gen = torch.Generator(device=device); gen.manual_seed(1)
    cases = [("generator", dict(generator=gen), batch()), ("raise_errors", dict(raise_errors=True), batch()),
             ("log=True", dict(log=True), batch()), ("obs_views", dict(obs_views=True), batch(6)),
             ("final_observation", dict(final_observation=True), batch()), ("native=False", dict(native=False), batch()),
             ("several modules", {}, widen(generate(n, n_steps=60, seed=4, arch="genset+battery", device=device), n_battery=2))]
    for word, kw, b in cases:
        pe = PerGridWindowEnv(b, trajectory_length=9, discrete=False, auto_reset=True, seed=2, **kw)
        if word != "obs_views":                            # (views are not offered for rolling windows at all: nothing to reset)
            pe.reset()
        snap = _snapshot(pe.env)
        with pytest.raises(ValueError, match=word):
            pe.step_k(acts(pe))
        _untouched(pe.env, snap)
        assert pe.episode_stats is None
        if word in ("raise_errors", "log=True"):
            fleet = PerGridWindowFleet.from_batches([batch(), b], trajectory_length=9, discrete=False, auto_reset=True, seed=2, **kw)
            fleet.reset()
            snaps = [_snapshot(q.env) for q in fleet.envs]
            with pytest.raises(ValueError, match=word):
                fleet.step_k([acts(q) for q in fleet.envs])
            for q, s in zip(fleet.envs, snaps):
                _untouched(q.env, s)
            fleet.close()
        pe.env.close()
    for word, kw in (("discrete=True", dict(discrete=True, auto_reset=True)), ("auto_reset=False", dict(discrete=False, auto_reset=False))):
        pe = PerGridWindowEnv(batch(), trajectory_length=9, seed=2, **kw)
        pe.reset()
        with pytest.raises(ValueError, match=word) as ei:
            pe.step_k(acts(pe))
        if word == "discrete=True":
            assert "use rollout" in str(ei.value)
        pe.env.close()
    ok = PerGridWindowEnv(batch(), trajectory_length=9, discrete=False, auto_reset=True, seed=2)
    with pytest.raises(RuntimeError, match="reset"):
        ok.step_k(acts(ok))                                 # before reset()
    ok.reset()
    snap = _snapshot(ok.env)
    with pytest.raises(ValueError):
        ok.step_k(acts(ok, dtype=torch.float32))            # the env's action_dtype is float64
    with pytest.raises(ValueError):
        ok.step_k(acts(ok, extra=1))                        # wrong last dimension
    with pytest.raises(ValueError):
        ok.step_k(acts(ok)[0])                              # [N, A]: a single step's control
    _untouched(ok.env, snap)
    assert ok.step_k(acts(ok))["reward"].shape == (K, n)
    ok.env.close()
