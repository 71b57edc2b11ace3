"""CEM planning on the device (mgx_lookahead_gaussian_episodes / mgx_cem_refit, StepEngine.lookahead_gaussian_episodes / cem_refit,
PerGridWindowEnv.lookahead_gaussian / cem_refit, CEMPlanner): the launch that draws its candidates in registers == the per-grid
what-if launch over ``cem_candidates_host``'s plan tensor (itself pinned to twin roll-outs and the oracle by tests/test_lookahead.py),
the refit == ``cem_refit_host`` -- torch.equal on every output: same operations, same order -- and afterwards nothing has moved.  The forms of the kernels these cases leave out -- all ten layouts x the three row sources x shared / per-grid plans
x the control type -- run in tests/test_layout_matrix_whatif.py, where the CPU oracle also runs every candidate plan."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SOAK = int(os.environ.get("MGX_FUZZ_SEED", "0"))
N, T, C_ = 333, 150, 5            # two workgroups, the last wave partly empty
F64, F32 = torch.float64, torch.float32
GBG, GB, BG = "genset+battery+grid", "genset+battery", "battery+grid"      # A = 4, 3, 2
DEAD_GRID = 7                     # every sigma of this grid is 0: its candidates tie
KEY = 0x9E3779B97F4A7C15 + SOAK

# (arch, series, trajectory_length, H, shaper, gamma, action_dtype).  H = 3 is below both ring depths of the launch (2 rows of
# (mean, sigma), 4 / 8 series rows), H = 9 above the deeper one; length 6: after the prefix of 2 every episode ends inside H = 9;
# None: random lengths, lanes of a wave stop at different steps
CASES = [
    (GBG, "factorised", 6, 9, False, 1.0, F64),
    (GBG, "materialised", None, 9, True, 0.9, F32),
    (GBG, "gather", None, 3, False, 1.0, F64),
    (GB, "factorised", None, 9, True, 0.9, F32),
    (GB, "materialised", 6, 3, False, 1.0, F64),
    (GB, "gather", 6, 9, True, 0.9, F32),
    (BG, "factorised", None, 1, False, 0.9, F32),
    (BG, "materialised", None, 9, False, 1.0, F64),
    (BG, "gather", 6, 1, True, 1.0, F64),
]
PREFIX = 2
RESULTS = ("ret", "steps", "end_soc", "best", "best_ret", "first_action")


def test_cases_cover_every_value_of_every_axis():
    for j, values in enumerate(([GBG, GB, BG], ["factorised", "materialised", "gather"], [6, None], [1, 3, 9], [False, True], [1.0, 0.9],
                                [F64, F32])):
        assert {c[j] for c in CASES} == set(values), j


def _batch(device, arch, series, n=N, t=T, seed=17):
    from pymgrid_amd.generator import generate
    return generate(n, n_steps=t, seed=seed + 1000 * SOAK, arch=arch, device=device, horizon=0, mixed_timers=True,
                    series="factorised" if series == "factorised" else "materialised")


def _snapshot(pe):
    """Everything a what-if call must leave alone: the state columns, the counter, the episodes and the statistics."""
    cols = pe.env.batch.cols
    snap = {name: cols[name].clone() for name in ("charge", "soc", "gen_status") if name in cols}
    snap["t"] = pe.env.engine._lib.mgx_current_step(pe.env.engine._h)
    snap["starts"] = pe.starts.clone()
    snap["lengths"] = None if pe.lengths is None else pe.lengths.clone()
    snap["current_steps"] = pe.env.current_steps.clone()
    for name, v in (pe.episode_stats or {}).items():
        snap["stat_" + name] = v.clone()
    return snap


def _untouched(pe, snap):
    now = _snapshot(pe)
    assert now.keys() == snap.keys()
    for name, v in snap.items():
        assert torch.equal(now[name], v) if torch.is_tensor(v) else now[name] == v, name


class _Gather:
    """The ``grid_major_copy`` tunable off for series == "gather" (the rows read where they lie), restored afterwards."""

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


def _env(device, arch, series="factorised", length=None, shaper=False, dtype=F64, n=N, discrete=False, prefix=PREFIX, make_batch=None):
    """A PerGridWindowEnv of in-place episodes, reset, ``prefix`` steps on (in one launch, so the statistics exist).
    ``make_batch(device, arch, series, n=)``: the batch factory (default: ``_batch``, a generated batch of architecture ``arch``)."""
    from pymgrid_amd import BatteryDischargeShaper
    from pymgrid_amd.hetero import PerGridWindowEnv
    kw = {} if discrete else dict(action_dtype=dtype)
    pe = PerGridWindowEnv((make_batch or _batch)(device, arch, series, n=n), trajectory_length=length, discrete=discrete, auto_reset=True,
                          seed=23 + SOAK, reward_shaping_func=BatteryDischargeShaper() if shaper else None, **kw)
    torch.manual_seed(41 + SOAK)
    pe.reset()
    if prefix and not discrete:
        g = torch.Generator(device=device); g.manual_seed(3 + SOAK)
        pe.step_k(torch.rand((prefix, n, pe.env.engine.action_dim), device=device, generator=g, dtype=F64).to(dtype))
    return pe


def _distribution(device, H, n, A, seed=5, dead_column=True):
    """mean in [-0.2, 1.2] (the clip binds), sigma in (0.05, 0.35) with the last column at 0 (``dead_column``; a layout with one
    control keeps it alive, or no candidate would differ from the mean) and every column of DEAD_GRID at 0."""
    g = torch.Generator(device=device); g.manual_seed(seed + SOAK)
    mean = torch.rand((H, n, A), device=device, generator=g, dtype=F64) * 1.4 - 0.2
    sigma = torch.rand((H, n, A), device=device, generator=g, dtype=F64) * 0.3 + 0.05
    if dead_column:
        sigma[:, :, A - 1] = 0.0
    if n > DEAD_GRID:
        sigma[:, DEAD_GRID, :] = 0.0
    return mean.contiguous(), sigma.contiguous()


def _launch_equals_the_per_grid_launch(device, arch, series, length, H, shaper, gamma, dtype, make_batch=None, n_candidates=C_,
                                       trace=None):
    """The body of the test below.  ``make_batch``: the batch factory of ``_env``; ``n_candidates``: C; ``trace``: a dict that
    receives what an independent replay needs -- test_lookahead._what_if_start before the call, the host candidates [C, H, N, A]
    and what the call returned."""
    from pymgrid_amd import cem_candidates_host
    from test_lookahead import _what_if_start
    C_ = n_candidates
    with _Gather(series):
        pe = _env(device, arch, series, length, shaper, dtype, make_batch=make_batch)
        A = pe.env.engine.action_dim
        assert A == ({GBG: 4, GB: 3, BG: 2}[arch] if isinstance(arch, str) else 2 * (arch & 1) + ((arch >> 1) & 1) + ((arch >> 2) & 1))
        soc = "soc" in pe.env.batch.cols                   # (a layout without a battery has no end SoC: the call refuses it)
        results = tuple(name for name in RESULTS if soc or name != "end_soc")
        mean, sigma = _distribution(device, H, N, A, dead_column=A > 1)
        snap = _snapshot(pe)
        _what_if_start(trace, pe, False)
        out = pe.lookahead_gaussian(mean, sigma, C_, KEY, gamma=gamma, end_soc=soc)
        _untouched(pe, snap)
        plans = cem_candidates_host(mean, sigma, C_, KEY, dtype)
        assert plans.shape == (C_, H, N, A) and plans.dtype == dtype
        ref = pe.lookahead(plans, gamma=gamma, end_soc=soc)
        if trace is not None:
            trace.update(plans=plans, out=dict(out))
        assert set(out) == set(results)
        for name in results:
            assert out[name].dtype == ref[name].dtype and torch.equal(out[name], ref[name]), name
        assert out["first_action"].dtype == dtype and out["first_action"].shape == (N, A)
        # the test's own inputs: the clip binds, the candidates differ, the dead grid ties (so its best is candidate 0), its first
        # action is the clipped mean
        assert bool((plans == 0).any()) and bool((plans == 1).any())
        assert not torch.equal(out["ret"][1], out["ret"][2])
        assert bool((out["ret"][:, DEAD_GRID] == out["ret"][0, DEAD_GRID]).all()) and int(out["best"][DEAD_GRID]) == 0
        assert torch.equal(out["first_action"][DEAD_GRID], mean[0, DEAD_GRID].clamp(0.0, 1.0).to(dtype))
        assert len(out["best"].unique()) > 1
        steps = out["steps"]
        if length is not None:
            assert bool((steps == min(H, length - PREFIX)).all())
        elif H == 9:
            assert len(steps.unique()) > 2 and int(steps.max()) == H
        # pick=False: the return launch alone; out=: the caller's tensors
        mine = {"ret": torch.full((C_, N), float("nan"), dtype=F64, device=device)}
        lean = pe.lookahead_gaussian(mean, sigma, C_, KEY, gamma=gamma, pick=False, out=mine)
        assert set(lean) == {"ret", "steps"} and lean["ret"] is mine["ret"] and torch.equal(lean["ret"], out["ret"])
        _untouched(pe, snap)
        pe.env.close()


@pytest.mark.parametrize("arch,series,length,H,shaper,gamma,dtype", CASES)
def test_launch_equals_the_per_grid_launch_over_the_host_candidates(arch, series, length, H, shaper, gamma, dtype, device):
    _launch_equals_the_per_grid_launch(device, arch, series, length, H, shaper, gamma, dtype)


@pytest.mark.parametrize("n_elite,dtype,series", [(1, F64, "factorised"), (3, F32, "materialised"), (C_, F64, "factorised")])
def test_refit_equals_the_host_rule(n_elite, dtype, series, device):
    """``steps`` from random-length episodes (lanes of a wave stop at different rows); in place == out of place; returns with ties
    and NaNs; steps=None; alpha and sigma_min."""
    from pymgrid_amd import cem_refit_host
    H = 9
    pe = _env(device, GBG if dtype == F64 else GB, series, None, False, dtype)
    A = pe.env.engine.action_dim
    mean, sigma = _distribution(device, H, N, A)
    la = pe.lookahead_gaussian(mean, sigma, C_, KEY, pick=True)
    assert len(la["steps"].unique()) > 2
    odd = la["ret"].clone()
    odd[2, ::7] = float("nan")
    odd[0, 3::5] = float("nan")
    odd[1, 5::11] = odd[3, 5::11]
    snap = _snapshot(pe)
    for ret, steps, alpha, smin in ((la["ret"], la["steps"], 1.0, 0.0), (odd, la["steps"], 0.7, 0.05), (odd, None, 0.25, 0.2)):
        dev = pe.cem_refit(ret, steps, mean, sigma, KEY, n_elite, alpha=alpha, sigma_min=smin)
        host = cem_refit_host(ret, steps, mean, sigma, KEY, n_elite, alpha=alpha, sigma_min=smin, dtype=dtype)
        assert set(dev) == {"elite", "mean", "sigma", "best_plan"}
        for name in dev:
            assert dev[name].dtype == host[name].dtype and torch.equal(dev[name], host[name]), (name, alpha)
        assert dev["best_plan"].dtype == dtype
        m2, s2 = mean.clone(), sigma.clone()
        same = pe.cem_refit(ret, steps, m2, s2, KEY, n_elite, alpha=alpha, sigma_min=smin, best_plan=False, out={"mean": m2, "sigma": s2})
        assert set(same) == {"elite", "mean", "sigma"} and same["mean"] is m2 and same["sigma"] is s2
        assert torch.equal(m2, dev["mean"]) and torch.equal(s2, dev["sigma"]) and torch.equal(same["elite"], dev["elite"])
    assert torch.equal(pe.cem_refit(la["ret"], la["steps"], mean, sigma, KEY, n_elite)["elite"][0], la["best"])
    _untouched(pe, snap)
    pe.env.close()


def test_more_candidates_than_one_launch_holds(device):
    """N = 2, H = 1, C = 65 537: past the 65 535 candidates of one launch's second grid dimension."""
    from pymgrid_amd import cem_candidates_host
    n, H, Cn = 2, 1, 65537
    pe = _env(device, GBG, n=n, prefix=0)
    A = pe.env.engine.action_dim
    mean, sigma = _distribution(device, H, n, A)
    sigma[:, :, A - 1] = 0.2
    out = pe.lookahead_gaussian(mean, sigma, Cn, KEY, end_soc=True)
    plans = cem_candidates_host(mean, sigma, Cn, KEY)
    ref = pe.lookahead(plans, end_soc=True)
    for name in RESULTS:
        assert torch.equal(out[name], ref[name]), name
    assert torch.equal(out["first_action"], plans[out["best"].long(), 0, torch.arange(n, device=device)])
    assert not torch.equal(out["ret"][65535:], out["ret"][:2])
    pe.env.close()


def _planner_env(device, discrete=False):
    from pymgrid_amd.hetero import PerGridWindowEnv
    pe = PerGridWindowEnv(_batch(device, GBG, "factorised"), trajectory_length=5, discrete=discrete, auto_reset=True, seed=23 + SOAK)
    torch.manual_seed(41 + SOAK)
    pe.reset()
    return pe


def test_planner_act_is_the_loop_of_the_public_calls(device):
    """Two ``act()`` + ``step`` of a warm-started planner == the hand-written loop: n_iters x (lookahead_gaussian, cem_refit in
    place) under ``cem_key(seed, counter, it)``, a last lookahead under iteration n_iters; then the mean shifted by a step, sigma
    reset, restarted grids back on init."""
    from pymgrid_amd import CEMPlanner, cem_key
    H, Cn, E, iters, seed = 6, 8, 3, 2, 11
    a, b = _planner_env(device), _planner_env(device)
    A = a.env.engine.action_dim
    m = CEMPlanner(a, H, n_candidates=Cn, n_elite=E, n_iters=iters, seed=seed, gamma=0.9, init_mean=0.4, init_sigma=0.25,
                   sigma_min=0.02, alpha=0.8)
    mean = torch.full((H, N, A), 0.4, dtype=F64, device=device)
    restarted = torch.zeros(N, dtype=torch.bool, device=device)
    for step in range(5):                                          # (trajectory_length 5: the last step restarts every grid)
        t = b.env.current_step
        sigma = torch.full((H, N, A), 0.25, dtype=F64, device=device)
        for it in range(iters):
            key = cem_key(seed, t, it)
            o = b.lookahead_gaussian(mean, sigma, Cn, key, gamma=0.9, pick=False)
            r = b.cem_refit(o["ret"], o["steps"], mean, sigma, key, E, alpha=0.8, sigma_min=0.02, best_plan=False)
            mean, sigma = r["mean"], r["sigma"]
        last = b.lookahead_gaussian(mean, sigma, Cn, cem_key(seed, t, iters), gamma=0.9)
        snap = _snapshot(a)
        act = m.act()
        _untouched(a, snap)
        assert torch.equal(act, last["first_action"]) and torch.equal(m.mean, mean) and torch.equal(m.sigma, sigma)
        assert set(m.last) == set(last) and all(torch.equal(m.last[k], last[k]) for k in last)
        assert bool((m.last["best_ret"] >= m.last["ret"][0]).all())
        assert not torch.equal(mean, torch.full_like(mean, 0.4)) and bool((sigma >= 0.02).all())
        _, r1, d1, _ = a.step(act)
        _, r2, d2, _ = b.step(last["first_action"])
        assert torch.equal(r1, r2) and torch.equal(d1, d2)
        restarted |= d2
        mean = torch.where(d2.view(1, N, 1), torch.full_like(mean, 0.4), torch.cat([mean[1:], mean[-1:]])).contiguous()
    assert bool(restarted.all())
    for pe in (a, b):
        pe.env.close()


def test_planner_run_is_reproducible_however_it_is_cut(device):
    """run(5) on twin envs is equal, and equals run(2) then run(3); the statistics are carried; warm_start=False differs."""
    from pymgrid_amd import CEMPlanner
    kw = dict(n_candidates=8, n_elite=3, n_iters=2, seed=5, gamma=0.9)
    envs = [_planner_env(device) for _ in range(4)]
    whole, twin, cut, cold = envs
    res = CEMPlanner(whole, 6, **kw).run(5, reward=True, done=True)
    res2 = CEMPlanner(twin, 6, **kw).run(5, reward=True, done=True)
    assert res["reward"].shape == (5, N) and res["done"].dtype == torch.bool and bool(res["done"].any())
    assert torch.equal(res["reward"], res2["reward"]) and torch.equal(res["done"], res2["done"])
    m = CEMPlanner(cut, 6, **kw)
    parts = [m.run(2, reward=True, done=True), m.run(3, reward=True, done=True)]
    assert torch.equal(torch.cat([p["reward"] for p in parts]), res["reward"])
    assert torch.equal(torch.cat([p["done"] for p in parts]), res["done"])
    for name in ("episode_return_sum", "episodes", "return_running"):
        assert torch.equal(parts[1][name], res[name]), name
    assert bool((m.last["best_ret"] >= m.last["ret"][0]).all())
    res3 = CEMPlanner(cold, 6, warm_start=False, **kw).run(5)
    assert torch.equal(res3["reward"][0], res["reward"][0]) and not torch.equal(res3["reward"], res["reward"])
    for pe in envs:
        pe.env.close()


def test_planner_without_iterations_and_without_noise_steps_the_clipped_mean(device):
    from pymgrid_amd import CEMPlanner
    pe = _planner_env(device)
    A = pe.env.engine.action_dim
    init = torch.linspace(-0.2, 1.2, A, dtype=F64, device=device)
    m = CEMPlanner(pe, 4, n_candidates=3, n_elite=1, n_iters=0, init_mean=init, init_sigma=0.0)
    act = m.act()
    assert torch.equal(act, init.clamp(0.0, 1.0).expand(N, A)) and bool((m.last["best"] == 0).all())
    assert torch.equal(m.last["ret"][1], m.last["ret"][0]) and torch.equal(m.last["ret"][2], m.last["ret"][0])
    pe.env.close()


def test_shooting_mpc_run_is_unchanged_by_the_shared_loop(device):
    """ShootingMPC.run (now the planners' shared loop) == the hand-written loop of lookahead + step on a twin."""
    from pymgrid_amd import ShootingMPC
    a, b = _planner_env(device), _planner_env(device)
    m = ShootingMPC(a, 5, n_random=6, seed=3, gamma=0.9)
    res = m.run(6, reward=True, done=True)
    rows, dones = [], []
    for _ in range(6):
        out = b.lookahead(m.default_candidates(b.env.current_step), gamma=0.9)
        _, r, d, _ = b.step(out["first_action"])
        rows.append(r.clone()); dones.append(d.clone())
    assert torch.equal(res["reward"], torch.stack(rows)) and torch.equal(res["done"], torch.stack(dones))
    run, tot = torch.zeros(N, dtype=F64, device=device), torch.zeros(N, dtype=F64, device=device)
    for r, d in zip(rows, dones):
        run = run + r
        tot = torch.where(d, tot + run, tot)
        run = torch.where(d, torch.zeros_like(run), run)
    assert torch.equal(res["episode_return_sum"], tot) and torch.equal(res["return_running"], run)
    for pe in (a, b):
        pe.env.close()


def test_refusals_of_the_c_abi(device):
    """mgx_lookahead_gaussian_episodes refuses what mgx_lookahead_step_k_episodes refuses -- a lock-step handle, shards, gathered
    windows, a gamma outside [0, 1], forecast noise, end_soc without a battery, several modules of a kind -- and shared plans
    (per_grid != 1); mgx_cem_refit its own arguments.  Nothing is launched: the caller's buffers keep their bytes, the state stays."""
    from pymgrid_amd import BatchedMicrogridEnv, MgxError, _lib
    from pymgrid_amd.generator import generate, widen
    from layouts import carve
    n, H = 300, 4
    nan = float("nan")

    def snapshot(env):
        cols = env.batch.cols
        snap = {name: cols[name].clone() for name in ("charge", "soc", "gen_status") if name in cols}
        snap["t"] = env.engine._lib.mgx_current_step(env.engine._h)
        return snap

    def refused(env, code, **kw):
        e = env.engine
        mean = torch.full((H, n, e.action_dim), 0.5, dtype=F64, device=device)
        ret = torch.full((2, n), nan, dtype=F64, device=device)
        snap = snapshot(env)
        with pytest.raises(MgxError) as ei:
            e.lookahead_gaussian_episodes(mean, mean, 2, 1, out={"ret": ret}, **kw)
        assert ei.value.code == code, ei.value
        assert "mgx_lookahead_gaussian_episodes" in str(ei.value)
        assert bool(ret.isnan().all())
        now = snapshot(env)
        for name, v in snap.items():
            assert torch.equal(now[name], v) if torch.is_tensor(v) else now[name] == v, name

    starts = torch.zeros(n, dtype=torch.int32, device=device)
    env = BatchedMicrogridEnv(_batch(device, GBG, "factorised", n=n, t=60))
    env.reset()
    refused(env, _lib.MGX_ERR_INVALID)                                   # a lock-step episode
    env.engine.set_shards(2)
    refused(env, _lib.MGX_ERR_UNSUPPORTED)                               # shards
    env.engine.set_shards(1)
    env.reset_windows(starts, None, max_length=9)
    refused(env, _lib.MGX_ERR_INVALID)                                   # gathered windows
    env.reset_windows(starts, None, max_length=9, rolling="inplace")
    for gamma in (1.5, -0.1, nan):
        refused(env, _lib.MGX_ERR_INVALID, gamma=gamma)
    # shared plans, a wrong struct size and NULL rows: through ctypes
    e = env.engine
    mean = torch.full((H, n, e.action_dim), 0.5, dtype=F64, device=device)
    ret = torch.full((2, n), nan, dtype=F64, device=device)
    for per_grid, size, rows in ((0, C.sizeof(_lib.Cem), mean.data_ptr()), (1, 8, mean.data_ptr()), (1, C.sizeof(_lib.Cem), None)):
        cem, la = _lib.Cem(), _lib.Lookahead()
        cem.struct_size, cem.key, cem.mean, cem.sigma = size, 1, rows, mean.data_ptr()
        la.struct_size, la.C, la.H, la.per_grid, la.gamma, la.ret = C.sizeof(_lib.Lookahead), 2, H, per_grid, 1.0, ret.data_ptr()
        assert e._lib.mgx_lookahead_gaussian_episodes(e._h, C.byref(cem), C.byref(la), None) == _lib.MGX_ERR_INVALID
        assert b"mgx_lookahead_gaussian_episodes" in e._lib.mgx_last_error()
    torch.cuda.synchronize()
    assert bool(ret.isnan().all())
    assert e.lookahead_gaussian_episodes(mean, mean, 2, 1)["ret"].shape == (2, n)          # ... and the call they spoiled goes through
    env.engine.set_forecast_noise(seed=5)
    refused(env, _lib.MGX_ERR_UNSUPPORTED)                               # noisy forecasts
    env.close()
    env = BatchedMicrogridEnv(carve(_batch(device, GBG, "factorised", n=n, t=60), 1 | 4))   # genset + grid: no battery
    env.reset_windows(starts, None, max_length=9, rolling="inplace")
    refused(env, _lib.MGX_ERR_INVALID, end_soc=True)
    env.close()
    env = BatchedMicrogridEnv(widen(generate(n, n_steps=60, seed=4, arch=GB, device=device), n_battery=2))   # several modules of a kind
    env.reset_windows(starts, None, max_length=9, rolling="inplace")
    with pytest.raises((MgxError, ValueError)):
        env.engine.lookahead_gaussian_episodes(torch.zeros((H, n, env.engine.action_dim), dtype=F64, device=device),
                                               torch.zeros((H, n, env.engine.action_dim), dtype=F64, device=device), 2, 1)
    env.close()

    # mgx_cem_refit: every output keeps its bytes
    env = BatchedMicrogridEnv(_batch(device, GB, "factorised", n=n, t=60))
    e = env.engine
    A = e.action_dim
    mean = torch.full((H, n, A), 0.5, dtype=F64, device=device)
    ret = torch.zeros((4, n), dtype=F64, device=device)
    outs = {"elite": torch.full((2, n), -7, dtype=torch.int32, device=device), "mean": torch.full_like(mean, nan), "sigma": torch.full_like(mean, nan)}
    for kw in (dict(alpha=1.5), dict(alpha=nan), dict(sigma_min=-1.0), dict(sigma_min=nan)):
        with pytest.raises(MgxError) as ei:
            e.cem_refit(ret, None, mean, mean, 1, 2, best_plan=False, out=outs, **kw)
        assert ei.value.code == _lib.MGX_ERR_INVALID and "mgx_cem_refit" in str(ei.value)
    for E in (0, 5, 33):
        with pytest.raises(MgxError) as ei:
            e.cem_refit(ret if E < 33 else torch.zeros((40, n), dtype=F64, device=device), None, mean, mean, 1, E, best_plan=False,
                        out={"mean": outs["mean"], "sigma": outs["sigma"]})
        assert ei.value.code == _lib.MGX_ERR_INVALID and "mgx_cem_refit" in str(ei.value)
    torch.cuda.synchronize()
    assert bool((outs["elite"] == -7).all()) and bool(outs["mean"].isnan().all()) and bool(outs["sigma"].isnan().all())
    env.close()


def test_refusals_of_the_python_surface(device):
    from pymgrid_amd import CEMPlanner
    from pymgrid_amd.hetero import PerGridWindowEnv
    n = 300
    pd = PerGridWindowEnv(_batch(device, GB, "factorised", n=n, t=60), trajectory_length=9, discrete=True, auto_reset=True, seed=2)
    pd.reset()
    z = torch.zeros((3, n, 3), dtype=F64, device=device)
    with pytest.raises(ValueError, match="discrete"):
        pd.lookahead_gaussian(z, z, 2, 1)
    with pytest.raises(ValueError, match="discrete"):
        pd.cem_refit(torch.zeros((2, n), dtype=F64, device=device), None, z, z, 1, 1)
    with pytest.raises(ValueError, match="discrete"):
        CEMPlanner(pd, 3)
    pd.env.close()
    pl = PerGridWindowEnv(_batch(device, GB, "factorised", n=n, t=60), trajectory_length=9, discrete=False, auto_reset=False, seed=2)
    pl.reset()
    with pytest.raises(ValueError, match="auto_reset=False"):
        pl.lookahead_gaussian(z, z, 2, 1)
    with pytest.raises(ValueError, match="auto_reset=False"):
        CEMPlanner(pl, 3)
    pl.env.close()
    pc = PerGridWindowEnv(_batch(device, GB, "factorised", n=n, t=60), trajectory_length=9, discrete=False, auto_reset=True, seed=2)
    with pytest.raises(RuntimeError, match="reset"):
        pc.lookahead_gaussian(z, z, 2, 1)
    pc.reset()
    for bad in ((z.float(), z), (z, z[:2]), (z[:, :5], z[:, :5]), (z[..., :2].contiguous(), z[..., :2].contiguous()), (z.cpu(), z.cpu())):
        with pytest.raises(ValueError, match="mean|sigma"):
            pc.lookahead_gaussian(*bad, 2, 1)
    with pytest.raises(ValueError, match="key"):
        pc.lookahead_gaussian(z, z, 2, -1)
    with pytest.raises(ValueError, match="n_candidates"):
        pc.lookahead_gaussian(z, z, 0, 1)
    for kw in (dict(n_elite=0), dict(n_elite=9, n_candidates=8), dict(n_elite=33, n_candidates=64), dict(n_iters=-1), dict(alpha=2.0),
               dict(sigma_min=-1.0), dict(n_candidates=0)):
        with pytest.raises(ValueError):
            CEMPlanner(pc, 3, **kw)
    with pytest.raises(TypeError):
        CEMPlanner(pc.env, 3)
    pc.env.close()
