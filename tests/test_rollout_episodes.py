"""The fused discrete roll-out over per-grid in-place episodes (mgx_rollout_episodes / StepEngine.rollout_episodes /
PerGridWindowEnv.rollout / RuleBasedControl.run_episodes / PerGridWindowFleet.rollout): K steps in one launch, restarts inside it, ==
the same env stepped K times with step(ids[k]) -- rewards, done flags, traces, episode starts / lengths, per-grid counters, module
state, the per-grid episode statistics and the next step's observation, bit for bit (torch.equal on fp64: same arithmetic, same order)."""
import itertools
import os

import numpy as np
import pytest
import torch

SOAK = int(os.environ.get("MGX_FUZZ_SEED", "0"))          # soak runs: another draw of every batch / episode / id sequence
N, T = 1000, 150
LAUNCHES = (1, 7, 64, 64, 130)          # K = 1, a K that is no multiple of a ring depth (4 / 8), 64-step launches, one above FACT_ROWS = 128
KERNEL = "rollout_episodes_kernel"


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_the_minor_stays():
    """mgx_rollout_episodes is an addition found by name: exported, declared in the header, bound; the ABI minor stays 3."""
    import ctypes as C
    from pymgrid_amd import _lib
    _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    assert L.mgx_rollout_episodes is not None
    assert "mgx_rollout_episodes" in _lib.SYMBOLS
    assert _lib.lib().mgx_abi_minor() == 3 == _lib.ABI_MINOR
    assert len(_lib.TUNABLES) == 12
    assert C.sizeof(_lib.EpisodeStats) == 4 * C.sizeof(C.c_void_p)


def test_episode_rollout_kernel_spills_nothing():
    """Every instantiation of rollout_episodes_kernel: no scratch memory, no spilled scalar or vector registers; all ten layouts,
    fixed and per-step ids, the three row sources."""
    from pymgrid_amd import _lib
    _lib.build()
    usage = _lib.resource_usage()
    if usage is None:
        pytest.skip("libmgx.so was not built on this machine (no resource_usage.json beside the objects)")
    forms = {name: u for name, u in usage.items() if name.split("<")[0].split("::")[-1] == KERNEL}
    assert len(forms) == 10 * 2 * 3, sorted(forms)
    for name, u in forms.items():
        assert u.get("scratch", 0) == 0 and u.get("vgpr_spill", 0) == 0 and u.get("sgpr_spill", 0) == 0, (name, u)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _batch(device, arch, series, H, seed=17, n=N, t=T):
    from pymgrid_amd.generator import generate
    return generate(n, n_steps=t, seed=seed + 1000 * SOAK, arch=arch, device=device, horizon=H, mixed_timers=True,
                    series="factorised" if series == "factorised" else "materialised")


def _shaper(on):
    from pymgrid_amd import BatteryDischargeShaper
    return BatteryDischargeShaper() if on else None


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


def _twin_steps(twin, ids, hs, want, walked=None):
    """K single steps of the twin: the per-step outputs the roll-out offers + the host statistics.  ``walked``: a list that receives
    every grid's series row before each step."""
    rows = {k: [] for k in ("reward", "done", "soc_trace", "status_trace")}
    cols = twin.env.batch.cols
    for k in range(ids.shape[0]):
        if walked is not None:
            walked.append(twin.env.current_steps.clone())
        _, r, d, _ = twin.step(ids[k].to(torch.int32))
        rows["reward"].append(r.clone()); rows["done"].append(d.clone())
        if "soc" in cols:
            rows["soc_trace"].append(cols["soc"].clone())
        if "gen_status" in cols:
            rows["status_trace"].append(cols["gen_status"].clone().view(torch.int32))
        hs.add(r, d)
    return {k: torch.stack(v) for k, v in rows.items() if v and k in want}


CASES = list(itertools.product(["genset+battery+grid", "genset+battery", "battery+grid"], ["factorised", "materialised", "gather"],
                               [9, None], [0, 6], [False, True], [False, True]))


def _rollout_equals_single_steps(device, arch, series, length, H, shaper, per_step, make_batch=None, trace=None):
    """``make_batch(device, arch, series, H)``: the batch factory (default: ``_batch``, a generated batch of architecture ``arch``);
    ``trace``: a dict that receives what an independent replay needs -- the ids, the priority-list table, the series rows the twin
    walked, the roll-out's rewards and the state after the last launch."""
    from pymgrid_amd import _lib
    from pymgrid_amd.hetero import PerGridWindowEnv
    make_batch = make_batch or _batch
    old = _lib.get_tunable("grid_major_copy")[0]
    if series == "gather":
        _lib.set_tunable("grid_major_copy", 0)
    try:
        envs = [PerGridWindowEnv(make_batch(device, arch, series, H), trajectory_length=length, discrete=True, auto_reset=True,
                                 seed=23 + SOAK, reward_shaping_func=_shaper(shaper)) for _ in range(2)]
        roll, twin = envs
        for e in envs:
            torch.manual_seed(41 + SOAK)                   # the same first draw
            e.obs0 = e.reset()
        assert torch.equal(roll.obs0, twin.obs0)
        pm = roll.env.engine._lib.mgx_current_step(roll.env.engine._h)
        assert pm == 0
        g = torch.Generator(device=device); g.manual_seed(3 + SOAK)
        n_act = roll.env.action_space.n
        hs = HostStats(N, device)
        fixed = torch.randint(0, n_act, (N,), device=device, generator=g).to(torch.uint8)
        restarts, twice, first, last = 0, False, False, False
        for K in LAUNCHES:
            ids = torch.randint(0, n_act, (K, N), device=device, generator=g).to(torch.uint8) if per_step else fixed.expand(K, N)
            out = roll.rollout(ids if per_step else fixed, K, reward=True, done=True, soc_trace=True, status_trace=True)
            walked = [] if trace is not None else None
            ref = _twin_steps(twin, ids, hs, out, walked)
            if trace is not None:
                trace["table"] = roll.env._table
                trace.setdefault("launches", []).append(dict(controls=ids.contiguous(), rows=torch.stack(walked), reward=out["reward"]))
            assert set(out) == set(ref), (sorted(out), sorted(ref))
            for name in out:
                assert out[name].shape == (K, N) and torch.equal(out[name], ref[name]), (K, name)
            assert torch.equal(roll.starts, twin.starts), K
            assert (roll.lengths is None) == (twin.lengths is None)
            if twin.lengths is not None:
                assert torch.equal(roll.lengths, twin.lengths), K
            assert torch.equal(roll.env.current_steps, twin.env.current_steps), K
            hs.check(roll.episode_stats)
            _state_equal(roll.env, twin.env)
            d = out["done"]
            restarts += int(d.sum())
            twice |= bool((d.sum(dim=0) >= 2).any())
            if K > 1:
                first |= bool(d[0].any()); last |= bool(d[-1].any())
        # the test's own input: it cannot pass vacuously
        assert restarts > N and twice and first and last, (restarts, twice, first, last)
        assert int(roll.episode_stats["episodes"].sum()) == restarts
        if trace is not None:
            trace["state"] = {name: roll.env.batch.cols[name].clone() for name in ("charge", "soc", "gen_status") if name in roll.env.batch.cols}
        a = torch.randint(0, n_act, (N,), device=device, generator=g).to(torch.int32)
        (o1, r1, d1, _), (o2, r2, d2, _) = roll.step(a), twin.step(a)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
        _state_equal(roll.env, twin.env)
        for e in envs:
            e.env.close()
    finally:
        _lib.set_tunable("grid_major_copy", old)


@pytest.mark.gpu
@pytest.mark.parametrize("arch,series,length,H,shaper,per_step", CASES)
def test_rollout_equals_single_steps(arch, series, length, H, shaper, per_step, device):
    """rollout(ids) in launches of uneven size == step(ids[k]) K times on a twin env with the same first draw and seed."""
    _rollout_equals_single_steps(device, arch, series, length, H, shaper, per_step)


@pytest.mark.gpu
@pytest.mark.parametrize("series", ["factorised", "materialised"])
@pytest.mark.parametrize("arch", ["genset+battery+grid", "genset+battery", "battery+grid"])
def test_auto_reset_off_walks_on(arch, series, device):
    """In-place episodes without set_auto_reset: engine.rollout_episodes == single steps past the end of the episodes (clamped rows);
    `episodes` counts a grid once, when it crosses its final step."""
    from pymgrid_amd import DiscreteBatchedMicrogridEnv
    n, K = 500, 37
    envs = [DiscreteBatchedMicrogridEnv(_batch(device, arch, series, 0, n=n, t=60)) for _ in range(2)]
    g = torch.Generator(device=device); g.manual_seed(9 + SOAK)
    starts = torch.randint(40, 52, (n,), device=device, generator=g).to(torch.int32)       # rows 60.. are beyond the series: clamped
    lengths = torch.randint(1, 9, (n,), device=device, generator=g).to(torch.int32)
    for e in envs:
        e.reset_windows(starts, lengths, max_length=8, rolling="inplace")
    roll, twin = envs
    ids = torch.randint(0, roll.action_space.n, (K, n), device=device, generator=g).to(torch.uint8)
    stats = {name: torch.zeros(n, dtype=dt, device=device) for name, dt in roll.engine.EPISODE_STATS}
    hs = HostStats(n, device)
    out = {}
    for lo, hi in ((0, 5), (5, 6), (6, K)):
        part = roll.engine.rollout_episodes(ids[lo:hi].contiguous(), roll._table, hi - lo, reward=True, done=True, stats=stats)
        for k_, v in part.items():
            out.setdefault(k_, []).append(v)
    out = {k_: torch.cat(v) for k_, v in out.items()}
    prev = torch.zeros(n, dtype=torch.bool, device=device)
    for k in range(K):
        _, r, d, _ = twin.step(ids[k].to(torch.int32))
        assert torch.equal(out["reward"][k], r) and torch.equal(out["done"][k].view(torch.bool), d), k
        hs.add(r, d & ~prev)                               # the crossing of the final step
        prev = d
    hs.check(stats)
    assert int(stats["episodes"].max()) == 1 and bool(prev.all())
    assert bool((starts.long() + K > 60).any())            # some grids did walk past the series
    assert roll.engine.current_step == twin.engine.current_step == K
    _state_equal(roll, twin)
    for e in envs:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("series", ["factorised", "materialised"])
def test_rule_based_control_over_episodes(series, device):
    """RuleBasedControl(per_grid_env).run_episodes(steps) == the same priority ids fed to step one at a time."""
    from pymgrid_amd import RuleBasedControl
    from pymgrid_amd.hetero import PerGridWindowEnv
    steps = 150
    envs = [PerGridWindowEnv(_batch(device, "genset+battery+grid", series, 0), trajectory_length=9, discrete=True, auto_reset=True,
                             seed=5 + SOAK) for _ in range(2)]
    roll, twin = envs
    rbc = RuleBasedControl(roll)
    torch.manual_seed(77 + SOAK)
    res = rbc.run_episodes(steps, chunk=64, reward=True, done=True)
    torch.manual_seed(77 + SOAK)
    twin.reset()
    ids = torch.from_numpy(rbc.priority_ids.astype(np.int32)).to(device)
    hs = HostStats(N, device)
    for k in range(steps):
        _, r, d, _ = twin.step(ids)
        assert torch.equal(res["reward"][k], r) and torch.equal(res["done"][k], d), k
        hs.add(r, d)
    hs.check(roll.episode_stats)
    assert torch.equal(res["episode_return_sum"], hs.sum) and torch.equal(res["episode_return_last"], hs.last)
    assert torch.equal(res["episodes"], hs.eps) and torch.equal(res["return_running"], hs.run)
    assert int(res["episodes"].min()) >= steps // 9 - 1
    assert torch.equal(roll.starts, twin.starts)
    _state_equal(roll.env, twin.env)
    for e in envs:
        e.env.close()


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
def test_rule_based_episode_returns_vs_the_oracle(device, oracle):
    """48 grids, rule-based control over 20 steps of 6-step episodes (every grid restarts at least twice): the per-episode returns of
    run_episodes == the CPU oracle's populate_action + run replay of every grid's episodes (a restart moves the counter and keeps the
    state).  The episode starts come from a single-stepped twin (equal to the roll-out env by the tests above)."""
    from pymgrid_amd import MicrogridBatch, RuleBasedControl
    from pymgrid_amd.hetero import PerGridWindowEnv
    from pymgrid_amd.priority_list import MODULE_NAMES
    n, t, length, steps = 48, 40, 6, 20
    rs = np.random.RandomState(31 + SOAK)
    grids = [_grid(rs, t) for _ in range(n)]
    envs = [PerGridWindowEnv(MicrogridBatch.from_grids(grids, device=device), trajectory_length=length, discrete=True, auto_reset=True,
                             seed=13 + SOAK) for _ in range(2)]
    roll, twin = envs
    rbc = RuleBasedControl(roll)
    torch.manual_seed(8 + SOAK)
    res = rbc.run_episodes(steps, chunk=7, reward=True, done=True)
    torch.manual_seed(8 + SOAK)
    twin.reset()
    ids = torch.from_numpy(rbc.priority_ids.astype(np.int32)).to(device)
    episodes = [[int(s)] for s in twin.starts.cpu().numpy()]
    for k in range(steps):
        _, _, d, _ = twin.step(ids)
        s = twin.starts.cpu().numpy()
        for j in np.flatnonzero(d.cpu().numpy()):
            episodes[j].append(int(s[j]))
    assert min(len(e) for e in episodes) >= 3
    reward, done = res["reward"].cpu().numpy(), res["done"].cpu().numpy()
    ret_sum, ret_last = res["episode_return_sum"].cpu().numpy(), res["episode_return_last"].cpu().numpy()
    running, count = res["return_running"].cpu().numpy(), res["episodes"].cpu().numpy()
    for j, gp in enumerate(grids):
        om = oracle.OracleMicrogrid(gp)
        plist = [(MODULE_NAMES[m], a) for m, a in rbc.priority_list[j]]
        ep = iter(episodes[j])
        om.reset(next(ep))
        n_left, run, total, last, cnt = length, 0.0, 0.0, 0.0, 0
        for k in range(steps):
            r = om.run(om.populate_action(plist), normalized=False).reward
            assert reward[k, j] == r, (j, k)
            run += r
            n_left -= 1
            assert bool(done[k, j]) == (n_left == 0), (j, k)
            if n_left == 0:
                last = run; total += run; cnt += 1; run = 0.0
                om.reset(next(ep)); n_left = length
        assert (ret_sum[j], ret_last[j], running[j], count[j]) == (total, last, run, cnt), j
        assert roll.env.batch.cols["charge"][j].item() == om.s.charge, j
    for e in envs:
        e.env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("length", [9, None])
def test_fleet_rollout_equals_its_twins(length, device):
    """PerGridWindowFleet.rollout, bucket by bucket == the per-bucket PerGridWindowEnv twins' rollout."""
    from pymgrid_amd.generator import generate_fleet
    from pymgrid_amd.hetero import PerGridWindowEnv, PerGridWindowFleet

    def parts():
        return [b for b, _ in generate_fleet(3000, n_steps=200, seed=29 + 1000 * SOAK, horizon=0, device=device).values()]
    kw = dict(trajectory_length=length, discrete=True, auto_reset=True)
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
        ids = [torch.randint(0, pe.env.action_space.n, (K, pe.n_grids), device=device, generator=g).to(torch.uint8) for pe in fleet.envs]
        outs = fleet.rollout(ids, reward=True, done=True, soc_trace=True)
        for b, tw in enumerate(twins):
            ref = tw.rollout(ids[b], reward=True, done=True, soc_trace=True)
            assert set(outs[b]) == set(ref)
            for name in ref:
                assert torch.equal(outs[b][name], ref[name]), (K, b, name)
            assert torch.equal(fleet.envs[b].starts, tw.starts) and torch.equal(fleet.current_steps[b], tw.env.current_steps)
            for name in tw.episode_stats:
                assert torch.equal(fleet.envs[b].episode_stats[name], tw.episode_stats[name]), (K, b, name)
            _state_equal(fleet.envs[b].env, tw.env)
    acts = [torch.randint(0, pe.env.action_space.n, (pe.n_grids,), device=device, generator=g).to(torch.int32) for pe in fleet.envs]
    of, rf, df, _ = fleet.step(acts)
    for b, tw in enumerate(twins):
        ot, rt, dt, _ = tw.step(acts[b])
        assert torch.equal(of[b], ot) and torch.equal(rf[b], rt) and torch.equal(df[b], dt), b
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
    """mgx_rollout_episodes refuses -- before anything is launched -- a handle that is not in in-place episodes (MGX_ERR_INVALID),
    several modules of a kind, shards, device-counter mode, `done` as bit sets and a set final-observation buffer
    (MGX_ERR_UNSUPPORTED); step_k / rollout_discrete keep refusing in-place handles."""
    from pymgrid_amd import DiscreteBatchedMicrogridEnv, MgxError, _lib
    from pymgrid_amd.generator import generate, widen
    n, K = 300, 5
    env = DiscreteBatchedMicrogridEnv(_batch(device, "genset+battery+grid", "factorised", 0, n=n, t=60))
    e = env.engine
    ids = torch.zeros(K, n, dtype=torch.uint8, device=device)
    stats = {name: torch.full((n,), 3, dtype=dt, device=device) for name, dt in e.EPISODE_STATS}

    def refused(code, eng=e, table=env._table, ids_=ids, environment=env, **kw):
        snap = _snapshot(environment, stats)
        with pytest.raises(MgxError) as ei:
            eng.rollout_episodes(ids_, table, K, stats=stats, **kw)
        assert ei.value.code == code, ei.value
        _untouched(environment, snap, stats)
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
    with pytest.raises(MgxError):                                            # the lock-step fused calls still refuse the handle
        e.step_k(torch.zeros(K, n, e.action_dim, dtype=torch.float64, device=device))
    with pytest.raises(MgxError):
        e.rollout_discrete(ids, env._table, K)
    out = e.rollout_episodes(ids, env._table, K, stats=stats)               # ... and the new one takes it
    assert out["reward"].shape == (K, n) and e.current_step == K
    env.close()
    # shards / device counter: the handle cannot enter in-place episodes there, so the call meets a handle that is not in place
    for setup in ("shards", "counter"):
        env = DiscreteBatchedMicrogridEnv(_batch(device, "genset+battery", "factorised", 0, n=n, t=60))
        e2 = env.engine
        env.reset()
        if setup == "shards":
            e2.set_shards(2)
        else:
            e2.use_device_counter(True)
        snap = _snapshot(env)
        with pytest.raises(MgxError) as ei:
            e2.rollout_episodes(ids, env._table, K)
        assert ei.value.code == _lib.MGX_ERR_UNSUPPORTED, ei.value
        _untouched(env, snap)
        env.close()
    # several modules of a kind
    wide = widen(generate(n, n_steps=60, seed=4, arch="genset+battery", device=device), n_battery=2)
    env = DiscreteBatchedMicrogridEnv(wide)
    env.reset_windows(starts, None, max_length=9, rolling="inplace")
    snap = _snapshot(env)
    with pytest.raises(MgxError) as ei:
        env.engine.rollout_episodes(ids, np.zeros((1, 3, 2), dtype=np.int32), K)
    assert ei.value.code == _lib.MGX_ERR_UNSUPPORTED, ei.value
    _untouched(env, snap)
    env.close()


@pytest.mark.gpu
def test_refusals_of_the_python_surface(device):
    """PerGridWindowEnv.rollout / RuleBasedControl / PerGridWindowFleet.rollout: ValueError that says which option stands in the way,
    nothing launched."""
    from pymgrid_amd import RuleBasedControl
    from pymgrid_amd.generator import generate, widen
    from pymgrid_amd.hetero import PerGridWindowEnv, PerGridWindowFleet
    n, K = 300, 4
    ids = torch.zeros(K, n, dtype=torch.uint8, device=device)

    def batch(h=0):
        return _batch(device, "genset+battery", "factorised", h, n=n, t=60)
    gen = torch.Generator(device=device); gen.manual_seed(1)
    cases = [("generator", dict(generator=gen), batch()), ("raise_errors", dict(raise_errors=True), batch()),
             ("check_asserts", dict(check_asserts=True), batch()), ("log=True", dict(log=True), batch()),
             ("obs_views", dict(obs_views=True), batch(6)), ("final_observation", dict(final_observation=True), batch()),
             ("several modules", {}, widen(generate(n, n_steps=60, seed=4, arch="genset+battery", device=device), n_battery=2))]
    for word, kw, b in cases:
        pe = PerGridWindowEnv(b, trajectory_length=9, discrete=True, auto_reset=True, seed=2, **kw)
        if word != "obs_views":                            # (views are not offered for rolling windows at all: nothing to reset)
            pe.reset()
        snap = _snapshot(pe.env)
        with pytest.raises(ValueError, match=word):
            pe.rollout(ids)
        _untouched(pe.env, snap)
        assert pe.episode_stats is None
        with pytest.raises(ValueError, match=word):
            RuleBasedControl(pe)
        if word in ("raise_errors", "log=True"):
            fleet = PerGridWindowFleet.from_batches([batch(), b], trajectory_length=9, discrete=True, auto_reset=True, seed=2, **kw)
            fleet.reset()
            snaps = [_snapshot(q.env) for q in fleet.envs]
            with pytest.raises(ValueError, match=word):
                fleet.rollout([ids, ids])
            for q, s in zip(fleet.envs, snaps):
                _untouched(q.env, s)
            fleet.close()
        pe.env.close()
    for word, kw in (("discrete=False", dict(discrete=False, auto_reset=True)), ("auto_reset=False", dict(discrete=True, auto_reset=False))):
        pe = PerGridWindowEnv(batch(), trajectory_length=9, seed=2, **kw)
        pe.reset()
        with pytest.raises(ValueError, match=word):
            pe.rollout(ids)
        pe.env.close()
    ok = PerGridWindowEnv(batch(), trajectory_length=9, discrete=True, auto_reset=True, seed=2)
    ok.reset()
    with pytest.raises(ValueError, match="K"):
        ok.rollout(ids[0])                                  # one id per grid needs K
    with pytest.raises(ValueError):
        ok.rollout(ids, K + 1)
    assert ok.rollout(ids)["reward"].shape == (K, n)
    with pytest.raises(TypeError):
        RuleBasedControl(ok.env).run_episodes(5)            # a plain env: run() is its episode
    ok.env.close()
