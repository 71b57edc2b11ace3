"""Per-grid auto-reset episodes on a mixed-layout fleet (PerGridWindowFleet): bucket k of the fleet == PerGridWindowEnv(batch_k, ...,
seed=fleet.seeds[k]) stepped on its own -- observations, rewards, done flags, final observations, episode starts / lengths, per-grid step
counters and module state, bit for bit.  The in-place buckets of a fleet step share ONE launch of fleet_step_kernel_v<true>
(mgx_fleet_step); the fleet_episodes tunable = 0 steps them beside it, with the same results.  Several modules of a kind step beside
the launch.  A small fleet is replayed on the CPU oracle."""
import os

import numpy as np
import pytest
import torch

SOAK = int(os.environ.get("MGX_FUZZ_SEED", "0"))          # soak runs: another draw of every fleet / episode / action sequence
N_FLEET, T_FLEET, STEPS = 3000, 200, 40


# ---- CPU: the C ABI surface of the feature -------------------------------------------------------------------------------
def test_abi_minor_and_fleet_episodes_tunable():
    """ABI minor 3 adds MGX_TUNE_FLEET_EPISODES (default 1, values 0 / 1)."""
    from pymgrid_amd import MgxError, _lib
    _lib.build()
    assert _lib.lib().mgx_abi_minor() == 3 == _lib.ABI_MINOR
    assert _lib.TUNABLES.index("fleet_episodes") == 11
    assert _lib.get_tunable("fleet_episodes") == (1, 1)
    for bad in (-1, 2, 7):
        with pytest.raises(MgxError):
            _lib.set_tunable("fleet_episodes", bad)
    _lib.set_tunable("fleet_episodes", 0)
    assert _lib.get_tunable("fleet_episodes") == (0, 1)
    _lib.set_tunable("fleet_episodes", 1)
    assert _lib.get_tunable("fleet_episodes") == (1, 1)


def test_episode_form_of_the_fleet_kernel_spills_nothing():
    """fleet_step_kernel_v<true> (the in-place episode form) exists beside the lock-step form and uses no scratch memory."""
    from pymgrid_amd import _lib
    _lib.build()
    usage = _lib.resource_usage()
    if usage is None:
        pytest.skip("libmgx.so was not built on this machine (no resource_usage.json beside the objects)")
    forms = {name: u for name, u in usage.items() if name.split("<")[0].split("::")[-1] == "fleet_step_kernel_v"}
    ep = [u for name, u in forms.items() if name.rstrip().endswith("<true>")]
    lock = [u for name, u in forms.items() if name.rstrip().endswith("<false>")]
    assert ep and lock, sorted(forms)
    for u in ep + lock:
        assert u.get("scratch", 0) == 0 and u.get("vgpr_spill", 0) == 0 and u.get("sgpr_spill", 0) == 0, u


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _parts(device, H, N=N_FLEET, T=T_FLEET):
    from pymgrid_amd.generator import generate_fleet
    parts = generate_fleet(N, n_steps=T, seed=29 + 1000 * SOAK, horizon=H, device=device)
    assert len(parts) >= 3, list(parts)
    return [b for b, _ in parts.values()]


@pytest.fixture
def fleet_episodes():
    """Sets the fleet_episodes tunable; the value it had is restored after the test."""
    from pymgrid_amd import _lib
    old = _lib.get_tunable("fleet_episodes")[0]
    yield lambda v: _lib.set_tunable("fleet_episodes", v)
    _lib.set_tunable("fleet_episodes", old)


def _actions(fleet, g):
    return fleet.sample_action(generator=g)


def _compare_step(fleet, twins, out_f, out_t, k, final=False):
    (of, rf, df, inf), outs = out_f, out_t
    for b, (tw, (ot, rt, dt, it)) in enumerate(zip(twins, outs)):
        assert torch.equal(rf[b], rt) and torch.equal(df[b], dt), (k, b)
        if ot is None:
            assert of[b] is None, (k, b)
        else:
            assert torch.equal(of[b], ot), (k, b)
        assert torch.equal(fleet.envs[b].starts, tw.starts), (k, b)
        assert (fleet.envs[b].lengths is None) == (tw.lengths is None), (k, b)
        if tw.lengths is not None:
            assert torch.equal(fleet.envs[b].lengths, tw.lengths), (k, b)
        assert torch.equal(fleet.current_steps[b], tw.env.current_steps), (k, b)
        if final:
            d = dt
            assert torch.equal(inf[b]["final_observation"][d], it["final_observation"][d]), (k, b)


def _compare_state(fleet, twins):
    for b, tw in enumerate(twins):
        for name in ("charge", "soc", "gen_status"):
            if name in tw.env.batch.cols:
                assert torch.equal(fleet.envs[b].env.batch.cols[name], tw.env.batch.cols[name]), (b, name)


def _run_pair(device, H, env_kwargs, steps=STEPS, final=False, generator_seed=None, **kw):
    """A fleet and its per-bucket twins over identical batches, stepped with the same actions; every output compared each step.
    Returns the fleet, the twins and the number of restarts seen."""
    from pymgrid_amd.hetero import PerGridWindowEnv, PerGridWindowFleet
    gf = gt = None
    if generator_seed is not None:
        gf = torch.Generator(device=device); gf.manual_seed(generator_seed)
        gt = torch.Generator(device=device); gt.manual_seed(generator_seed)
    fleet = PerGridWindowFleet.from_batches(_parts(device, H), generator=gf, final_observation=final, **kw, **env_kwargs)
    twins = [PerGridWindowEnv(b, generator=gt, final_observation=final, **dict(kw, seed=fleet.seeds[k]), **env_kwargs)
             for k, b in enumerate(_parts(device, H))]
    torch.manual_seed(61 + SOAK)               # the first episodes come from torch's default generator without a `generator`,
    of = fleet.reset()                         # drawn bucket by bucket
    torch.manual_seed(61 + SOAK)
    for b, tw in enumerate(twins):
        assert torch.equal(of[b], tw.reset()), b
    ga = torch.Generator(device=device); ga.manual_seed(5 + SOAK)
    restarts = 0
    for k in range(steps):
        acts = _actions(fleet, ga)
        out_f = fleet.step(acts)
        out_t = [tw.step(a) for tw, a in zip(twins, acts)]
        _compare_step(fleet, twins, out_f, out_t, k, final=final)
        restarts += sum(int(d.sum()) for d in out_f[2])
    _compare_state(fleet, twins)
    return fleet, twins, restarts


def _close(fleet, twins):
    fleet.close()
    for tw in twins:
        tw.env.close()


OBS_CASES = [(0, {}), (3, dict(obs_prefetch=0)), (24, {})]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("H,obs_kw", OBS_CASES)
@pytest.mark.parametrize("length", [9, None])
@pytest.mark.parametrize("discrete", [False, True])
def test_fleet_equals_its_per_bucket_twins(discrete, length, H, obs_kw, dtype, device):
    """PerGridWindowFleet(auto_reset=True) == one PerGridWindowEnv per bucket (seed = fleet.seeds[k]) stepped one by one: observations,
    rewards, done, starts, lengths, current_steps after every step, battery / genset state at the end."""
    kw = dict(trajectory_length=length, discrete=discrete, auto_reset=True, seed=11 + SOAK, obs_dtype=dtype, **obs_kw)
    if discrete:
        kw["remove_redundant_gensets"] = False
    fleet, twins, restarts = _run_pair(device, H, {}, **kw)
    assert all(pe.native and pe._device_draws for pe in fleet.envs)
    assert (fleet.envs[0].env._ring is not None) == (H == 24)
    assert len(set(fleet.seeds)) == len(fleet.seeds) and fleet.seeds[0] == 11 + SOAK
    assert restarts > N_FLEET // 2, restarts
    _close(fleet, twins)


@pytest.mark.gpu
@pytest.mark.parametrize("H,obs_kw", OBS_CASES)
def test_fleet_final_observations(H, obs_kw, device):
    """final_observation=True: the done rows of info[k]["final_observation"] == the twin's."""
    kw = dict(trajectory_length=9, auto_reset=True, seed=3 + SOAK, **obs_kw)
    fleet, twins, restarts = _run_pair(device, H, {}, final=True, steps=30, **kw)
    assert restarts > N_FLEET // 2
    _close(fleet, twins)


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [False, True])
@pytest.mark.parametrize("length", [9, None])
def test_fleet_generator_draws(discrete, length, device):
    """A torch generator: the buckets draw from it in bucket order, as twins sharing one generator stepped in bucket order."""
    kw = dict(trajectory_length=length, discrete=discrete, auto_reset=True)
    if discrete:
        kw["remove_redundant_gensets"] = False
    fleet, twins, restarts = _run_pair(device, 0, {}, generator_seed=17 + SOAK, steps=30, **kw)
    assert all(not pe._device_draws for pe in fleet.envs)
    assert restarts > 0
    _close(fleet, twins)


@pytest.mark.gpu
@pytest.mark.parametrize("H,obs_kw", [(0, {}), (24, {})])
@pytest.mark.parametrize("discrete", [False, True])
def test_fused_launch_equals_stepping_beside(discrete, H, obs_kw, device, fleet_episodes):
    """fleet_episodes = 1 (one fleet_step_kernel_v<true> launch for the in-place buckets) == 0 (one step launch per bucket beside it):
    every output and every restart identical."""
    from pymgrid_amd.hetero import PerGridWindowFleet
    kw = dict(trajectory_length=None, discrete=discrete, auto_reset=True, seed=23 + SOAK, final_observation=not discrete, **obs_kw)
    if discrete:
        kw["remove_redundant_gensets"] = False
    fused = PerGridWindowFleet.from_batches(_parts(device, H), **kw)
    beside = PerGridWindowFleet.from_batches(_parts(device, H), **kw)
    torch.manual_seed(62 + SOAK)
    o1 = fused.reset()
    torch.manual_seed(62 + SOAK)
    o2 = beside.reset()
    for a, b in zip(o1, o2):
        assert torch.equal(a, b)
    ga = torch.Generator(device=device); ga.manual_seed(9 + SOAK)
    restarts = 0
    for k in range(STEPS):
        acts = fused.sample_action(generator=ga)
        fleet_episodes(1)
        of, rf, df, inf = fused.step(acts)
        fleet_episodes(0)
        ob, rb, db, inb = beside.step(acts)
        fleet_episodes(1)
        for j in range(len(of)):
            assert torch.equal(rf[j], rb[j]) and torch.equal(df[j], db[j]) and torch.equal(of[j], ob[j]), (k, j)
            assert torch.equal(fused.starts[j], beside.starts[j]) and torch.equal(fused.lengths[j], beside.lengths[j]), (k, j)
            if not discrete:
                d = df[j]
                assert torch.equal(inf[j]["final_observation"][d], inb[j]["final_observation"][d]), (k, j)
        restarts += sum(int(d.sum()) for d in df)
    assert restarts > 0
    assert torch.equal(fused.scatter(fused.current_steps), beside.scatter(beside.current_steps))
    _close(fused, [])
    _close(beside, [])


def _mixed_batches(device, T=120, N=700):
    from pymgrid_amd.generator import generate, widen
    base = generate(N, n_steps=T, seed=31 + SOAK, arch="genset+battery+grid", device=device)
    multi = widen(base, n_genset=2, n_battery=2)
    return [generate(N + 11, n_steps=T, seed=32 + SOAK, arch="genset+battery", device=device), multi,
            generate(N - 5, n_steps=T, seed=33 + SOAK, arch="battery+grid", device=device)]


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [False, True])
def test_mixed_fleet_with_several_modules_of_a_kind(discrete, device):
    """A fleet that mixes a widen(...) bucket with single-instance buckets: the several-of-a-kind bucket steps beside the fused launch
    and every bucket equals its twin."""
    from pymgrid_amd.hetero import PerGridWindowEnv, PerGridWindowFleet
    kw = dict(trajectory_length=7, discrete=discrete, auto_reset=True, seed=41 + SOAK)
    if discrete:
        kw["remove_redundant_gensets"] = False
    fleet = PerGridWindowFleet.from_batches(_mixed_batches(device), **kw)
    twins = [PerGridWindowEnv(b, **dict(kw, seed=fleet.seeds[k])) for k, b in enumerate(_mixed_batches(device))]
    assert fleet._in_call == [True, False, True]
    assert fleet.envs[1].env.layout.multi
    torch.manual_seed(63 + SOAK)
    of = fleet.reset()
    torch.manual_seed(63 + SOAK)
    for a, tw in zip(of, twins):
        assert torch.equal(a, tw.reset())
    ga = torch.Generator(device=device); ga.manual_seed(4 + SOAK)
    for k in range(30):
        acts = fleet.sample_action(generator=ga)
        out_f = fleet.step(acts)
        out_t = [tw.step(a) for tw, a in zip(twins, acts)]
        _compare_step(fleet, twins, out_f, out_t, k)
    _compare_state(fleet, twins)
    r = fleet.scatter(out_f[1])
    assert r.shape == (fleet.n_grids,) and torch.equal(r[fleet.index[1]], out_f[1][1])
    _close(fleet, twins)


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [False, True])
def test_final_observation_refused_with_several_modules_of_a_kind(discrete, device):
    """final_observation=True with a several-of-a-kind bucket: NotImplementedError, as PerGridWindowEnv raises."""
    from pymgrid_amd.hetero import PerGridWindowFleet
    kw = dict(remove_redundant_gensets=False) if discrete else {}
    with pytest.raises(NotImplementedError):
        PerGridWindowFleet.from_batches(_mixed_batches(device, T=60, N=64), trajectory_length=9, discrete=discrete, auto_reset=True,
                                        final_observation=True, **kw)


def _grid(rs, T, gen, bat, grid):
    g = dict(load_ts=80 * rs.rand(T) + 5, pv_ts=60 * rs.rand(T) * (rs.rand(T) > 0.3), horizon=0, final_step=T, initial_step=0,
             unbalanced=dict(loss_load_cost=10.0, overgeneration_cost=1.0 + rs.rand()), controllable_order=["genset", "battery", "grid"])
    if gen:
        g["genset"] = dict(running_min_production=float(rs.choice([0.0, 5.0, 12.0])), running_max_production=40.0 + 40 * rs.rand(),
                           genset_cost=0.3 + 0.3 * rs.rand(), co2_per_unit=2.0, cost_per_unit_co2=0.1, start_up_time=int(rs.randint(0, 3)),
                           wind_down_time=int(rs.randint(0, 3)), init_start_up=bool(rs.randint(0, 2)))
    if bat:
        g["battery"] = dict(min_capacity=10.0, max_capacity=60.0 + 80 * rs.rand(), max_charge=20.0 + 10 * rs.rand(), max_discharge=25.0,
                            efficiency=float(rs.choice([0.9, 0.95, 1.0])), battery_cost_cycle=0.02 * rs.rand(), init_soc=0.3 + 0.6 * rs.rand())
    if grid:
        g["grid"] = dict(max_import=30.0 + 40 * rs.rand(), max_export=20.0 + 30 * rs.rand(), cost_per_unit_co2=0.1)
        g["grid_ts"] = np.stack([0.1 + rs.rand(T), 0.5 * rs.rand(T), 0.3 * rs.rand(T), (rs.rand(T) > 0.2).astype(float)], axis=1)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("length", [6, None])
def test_fleet_episodes_vs_the_oracle(length, device, oracle):
    """A 48-grid, three-architecture PerGridWindowFleet (device draws, in-place episodes in one fused launch): every grid's sequence of
    episodes (start, length at each restart) and controls replayed on the CPU oracle (a restart moves the counter and keeps the
    state) -- rewards, done flags, observation rows and the final battery state `==`."""
    from pymgrid_amd.hetero import PerGridWindowFleet
    N, T, K = 48, 40, 60
    rs = np.random.RandomState(19 + SOAK)
    archs = [(1, 1, 0), (0, 1, 1), (1, 1, 1)]
    grids = [_grid(rs, T, *archs[j % 3]) for j in range(N)]
    fleet = PerGridWindowFleet(grids, device=device, trajectory_length=length, auto_reset=True, seed=7 + SOAK)
    assert len(fleet.envs) == 3 and all(pe.native and pe._device_draws and not pe.env.layout.multi for pe in fleet.envs)
    obs = [[o.cpu().numpy() for o in fleet.reset()]]          # per bucket: the buckets' rows have different lengths

    def episodes_now():
        s = fleet.scatter(fleet.starts).cpu().numpy()
        ln = np.full(N, length) if length is not None else fleet.scatter(fleet.lengths).cpu().numpy()
        return s.copy(), ln.copy()
    s0, l0 = episodes_now()
    episodes = [[(int(s0[j]), int(l0[j]))] for j in range(N)]
    acts, rewards, dones = [], [], []
    for k in range(K):
        a = [torch.as_tensor(rs.rand(pe.n_grids, pe.env.layout.action_dim), device=device) for pe in fleet.envs]
        o, r, d, _ = fleet.step(a)
        acts.append([x.cpu().numpy() for x in a])
        rewards.append(fleet.scatter(r).cpu().numpy()); dones.append(fleet.scatter(d).cpu().numpy())
        obs.append([x.cpu().numpy() for x in o])
        s, ln = episodes_now()
        for j in np.flatnonzero(dones[-1]):
            episodes[j].append((int(s[j]), int(ln[j])))
    assert sum(len(e) - 1 for e in episodes) > N
    where = {}                                            # grid -> (bucket, row inside the bucket)
    for b, idx in enumerate(fleet.index):
        for r_, j in enumerate(idx.cpu().numpy()):
            where[int(j)] = (b, r_)
    charge = [pe.env.batch.cols.get("charge") for pe in fleet.envs]
    for j, gp in enumerate(grids):
        b, row = where[j]
        om = oracle.OracleMultiMicrogrid(gp)
        ep = iter(episodes[j])
        start, n_left = next(ep)
        assert np.array_equal(obs[0][b][row], om.reset(start)), j
        for k in range(K):
            out = om.run(acts[k][b][row], True)
            assert rewards[k][j] == out.common.reward, (j, k)
            n_left -= 1
            assert bool(dones[k][j]) == (n_left == 0), (j, k)
            if n_left == 0:
                start, n_left = next(ep)
                om.reset(start)
            assert np.array_equal(obs[k + 1][b][row], om.observe()), (j, k)
        if charge[b] is not None:
            assert charge[b].reshape(-1)[row].item() == om.s.battery[0].charge, j
    fleet.close()
