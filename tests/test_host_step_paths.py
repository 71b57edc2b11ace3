"""What the host paths around a single-step launch keep, whichever entry a step comes through: priority-list ids are taken in every
form that converts to an int32 [N] device tensor and leave the same step; a step refused before its launch leaves the env (and a
fleet's other buckets) where it stood; the single-step engine calls write into the tensors handed in through ``out=``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, T, STEPS = 70, 60, 8                       # one full wave plus a partial one
ARCHS = ("genset+battery", "battery+grid")
KEEP = dict(remove_redundant_gensets=False)      # (generated gensets mix running_min_production == 0 and > 0)


def _batch(device, arch, H=0, seed=7):
    from pymgrid_amd.generator import generate
    return generate(N, n_steps=T, seed=seed, arch=arch, horizon=H, device=device, mixed_timers=True, series="factorised")


def _batches(device, H=0):
    return [_batch(device, a, H, seed=7 + k) for k, a in enumerate(ARCHS)]


def _wide(device):
    from pymgrid_amd.generator import generate, widen
    return widen(generate(N, n_steps=T, seed=7, arch="genset+battery+grid", device=device, mixed_timers=True), n_genset=2, n_battery=2)


# ---- 1. ids in every accepted form -----------------------------------------------------------------------------------------
def _forms(ids):
    """The same ids as a list, a numpy int64 array, a CPU tensor, an int64 device tensor and a non-contiguous int32 view."""
    two = torch.zeros(2 * ids.numel(), dtype=torch.int32, device=ids.device)
    two[::2] = ids
    view = two[::2]
    assert not view.is_contiguous()
    return [ids.tolist(), ids.cpu().numpy().astype(np.int64), ids.cpu(), ids.to(torch.int64), view]


def _same(a, b, where):
    assert (a is None) == (b is None), where
    assert a is None or torch.equal(a, b), where


def _single(device, reuse):
    from pymgrid_amd import DiscreteBatchedMicrogridEnv
    make = lambda: DiscreteBatchedMicrogridEnv(_batch(device, ARCHS[0], 4), obs_prefetch=4, reuse_outputs=reuse, **KEEP)
    return make(), make(), False


def _instances(device):
    from pymgrid_amd import DiscreteBatchedMicrogridEnv
    a, b = DiscreteBatchedMicrogridEnv(_wide(device), **KEEP), DiscreteBatchedMicrogridEnv(_wide(device), **KEEP)
    assert a._instances and a.layout.multi
    return a, b, False


def _bucketed(device, **kw):
    from pymgrid_amd.hetero import BucketedFleet
    make = lambda: BucketedFleet.from_batches(_batches(device, 4), discrete=True, obs_prefetch=4, **KEEP, **kw)
    return make(), make(), True


def _pergrid(device):
    from pymgrid_amd.hetero import PerGridWindowFleet
    make = lambda: PerGridWindowFleet.from_batches(_batches(device, 4), discrete=True, auto_reset=True, trajectory_length=9, seed=3, **KEEP)
    return make(), make(), True


# Not pinned here: BucketedFleet's per-step-plan path (reuse_outputs=0) does not keep converted ids alive until its launch, so ids in
# another form than the canonical one may be read after their block was handed out again; and no BucketedFleet path checks the ids' length.
ENTRIES = {
    "env_per_call": lambda dev: _single(dev, 0),
    "env_bound": lambda dev: _single(dev, 4),
    "env_instances": _instances,
    "fleet_fast": lambda dev: _bucketed(dev, reuse_outputs=12, refill="chunks"),
    "fleet_bound": lambda dev: _bucketed(dev, reuse_outputs=12),
    "pergrid_fleet": _pergrid,
}
RAISING = [k for k in ENTRIES if not k.startswith("fleet_")]


def _close(*envs):
    for e in envs:
        e.close()


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_ids_in_every_accepted_form_leave_the_same_step(entry, device):
    """Step k hands the twin the ids in form k mod 5; the env beside it takes the canonical int32 device tensor."""
    ref, twin, is_fleet = ENTRIES[entry](device)
    if entry == "env_bound":
        assert ref._fp is not None
    torch.manual_seed(19)                     # (per-grid episodes without a generator draw their first episodes from torch's default)
    o1 = ref.reset()
    torch.manual_seed(19)
    o2 = twin.reset()
    for a, b in zip(o1, o2) if is_fleet else [(o1, o2)]:
        _same(a, b, "reset")
    g = torch.Generator(device=device); g.manual_seed(23)
    for k in range(STEPS):
        ids = ref.sample_action(generator=g)
        if is_fleet:
            other = [_forms(i)[k % 5] for i in ids]
        else:
            other = _forms(ids)[k % 5]
        out1, out2 = ref.step(ids), twin.step(other)
        for j in range(3):                    # obs, reward, done
            for a, b in zip(out1[j], out2[j]) if is_fleet else [(out1[j], out2[j])]:
                _same(a, b, (entry, k, j))
    if is_fleet and entry != "pergrid_fleet":
        assert (ref._bound is not None) == (twin._bound is not None) == (entry == "fleet_bound")
    _close(ref, twin)


def test_get_action_takes_ids_in_every_form(device):
    from pymgrid_amd import DiscreteBatchedMicrogridEnv
    for env in (DiscreteBatchedMicrogridEnv(_batch(device, ARCHS[0]), **KEEP), DiscreteBatchedMicrogridEnv(_wide(device), **KEEP)):
        env.reset()
        g = torch.Generator(device=device); g.manual_seed(29)
        ids = env.sample_action(generator=g)
        want = env.get_action(ids)
        for f, form in enumerate(_forms(ids)):
            assert torch.equal(env.get_action(form), want), f
        with pytest.raises(ValueError, match="action_id must be an int32 tensor of shape"):
            env.get_action(torch.zeros(N + 1, dtype=torch.int32, device=device))
        env.close()


@pytest.mark.parametrize("entry", RAISING)
def test_ids_of_the_wrong_length_are_refused(entry, device):
    ref, twin, is_fleet = ENTRIES[entry](device)
    ref.reset()
    bad = torch.zeros(N + 1, dtype=torch.int32, device=device)
    ids = ref.sample_action()
    if is_fleet:
        bad = ids[:-1] + [bad]
    with pytest.raises(ValueError, match="action_id must be an int32 tensor of shape"):
        ref.step(bad)
    _close(ref, twin)


# ---- 2. a refused step leaves the env usable -------------------------------------------------------------------------------
def _gen(device, seed=31):
    g = torch.Generator(device=device); g.manual_seed(seed)
    return g


def _too_wide(env):
    e = env.engine
    return torch.zeros(e.N, e.action_dim + 1, dtype=e.action_dtype, device=e.device)


def test_a_refused_step_leaves_the_host_path_env_usable(device):
    """A torch generator's restarts, no rings: the rows come from the observe pass behind the restarts, so the step sets the env's rows
    aside around its launch -- and must put them back when the launch is refused."""
    from pymgrid_amd.hetero import PerGridWindowEnv
    make = lambda: PerGridWindowEnv(_batch(device, ARCHS[0]), trajectory_length=9, auto_reset=True, generator=_gen(device), obs_prefetch=0)
    env, twin = make(), make()
    assert env.full.layout.horizon == 0 and not env._device_draws
    assert torch.equal(env.reset(), twin.reset())
    ga = _gen(device, 37)
    for k in range(STEPS):
        a = env.sample_action(generator=ga)
        if k in (1, 5):
            with pytest.raises(ValueError):
                env.step(_too_wide(env))
        out, want = env.step(a), twin.step(a)
        assert out[0] is not None and tuple(out[0].shape) == (N, env.engine.obs_dim), k
        for j in range(3):
            assert torch.equal(out[j], want[j]), (k, j)
    assert torch.equal(env.starts, twin.starts)
    _close(env.env, twin.env)


def test_a_refused_last_bucket_leaves_the_fleet_usable(device):
    from pymgrid_amd.hetero import PerGridWindowEnv, PerGridWindowFleet
    kw = dict(trajectory_length=9, auto_reset=True, obs_prefetch=0)
    fleet = PerGridWindowFleet.from_batches(_batches(device), generator=_gen(device), seed=3, **kw)
    gt = _gen(device)
    twins = [PerGridWindowEnv(b, generator=gt, seed=fleet.seeds[k], **kw) for k, b in enumerate(_batches(device))]
    for a, tw in zip(fleet.reset(), twins):
        assert torch.equal(a, tw.reset())
    ga = _gen(device, 37)
    for k in range(STEPS):
        acts = fleet.sample_action(generator=ga)
        if k in (1, 5):
            with pytest.raises(ValueError):
                fleet.step(acts[:-1] + [_too_wide(fleet.envs[-1])])
        out = fleet.step(acts)
        want = [tw.step(a) for tw, a in zip(twins, acts)]
        for b in range(len(twins)):
            assert out[0][b] is not None and tuple(out[0][b].shape) == (N, twins[b].engine.obs_dim), (k, b)
            for j in range(3):
                assert torch.equal(out[j][b], want[b][j]), (k, b, j)
            assert torch.equal(fleet.envs[b].starts, twins[b].starts), (k, b)
    fleet.close()
    _close(*[tw.env for tw in twins])


# ---- 3. single-step outputs through out= -----------------------------------------------------------------------------------
@pytest.mark.parametrize("call", ["step", "step_discrete", "step_many"])
def test_single_step_outputs_through_out(call, device):
    from pymgrid_amd.engine import StepEngine
    from pymgrid_amd.priority_list import get_priority_lists, table_array
    arch = "genset+battery+grid"
    ea, eb = StepEngine(_batch(device, arch)), StepEngine(_batch(device, arch))
    table = table_array(get_priority_lists(True, True, True))
    K = 3
    lead = (K,) if call == "step_many" else ()
    g = _gen(device, 41)

    def run(e, arg, **kw):
        if call == "step":
            return e.step(arg, **kw)
        if call == "step_discrete":
            return e.step_discrete(arg, table, **kw)[:4]
        if "want_done" in kw:
            kw["done"] = kw.pop("want_done")
        return e.step_many(arg, **kw)

    def arg():
        if call == "step_discrete":
            return torch.randint(0, table.shape[0], (N,), dtype=torch.int32, device=device, generator=g)
        return torch.rand(*lead, N, ea.action_dim, dtype=torch.float64, device=device, generator=g)
    mine = dict(reward=torch.empty(*lead, N, dtype=torch.float64, device=device),
                done=torch.empty(*lead, N, dtype=torch.uint8, device=device),
                obs=torch.empty(*lead, N, ea.obs_dim, dtype=torch.float64, device=device),
                log=torch.empty(*lead, ea.log_dim, N, dtype=torch.float64, device=device))
    a = arg()
    obs, reward, done, log = run(ea, a, want_obs=True, want_log=True, out=mine)
    for name, t in (("obs", obs), ("reward", reward), ("done", done), ("log", log)):
        assert t is not None and t.data_ptr() == mine[name].data_ptr() and t.shape == mine[name].shape, name
    fresh = run(eb, a, want_obs=True, want_log=True, out={})
    for name, t, f in zip(("obs", "reward", "done", "log"), (obs, reward, done, log), fresh):
        assert f is not None and f.data_ptr() != t.data_ptr() and f.dtype == t.dtype and f.shape == t.shape, name
        assert torch.equal(f, t), name
    a = arg()
    obs, reward, done, log = run(ea, a, want_obs=True, want_log=False, want_done=False, out=mine)
    assert done is None and log is None and reward.data_ptr() == mine["reward"].data_ptr()
    fresh = run(eb, a, want_obs=True, want_log=False, want_done=False)
    assert fresh[2] is None and fresh[3] is None
    assert torch.equal(fresh[0], obs) and torch.equal(fresh[1], reward)
    ea.close(); eb.close()
