"""Auto-reset discrete episodes on layouts with several modules of a kind (the general path): PerGridWindowEnv(discrete=True,
auto_reset=True) runs in place (mgx_reset_episodes) -- with device draws the step kernel restarts the grids it finishes, and a discrete
step of a layout with at most two modules of a kind is ONE launch of step_lists_small_kernel<F, true>; with a torch generator the draws
are applied behind the step (mgx_reset_grids).  Pinned against the continuous twin fed the expanded controls, against the two-launch
path (expand_multi_kernel + step_multi_kernel<F, true>), against gathered windows, and against the multi-instance CPU oracle."""
import os

import numpy as np
import pytest
import torch

from layouts import episodes_vs_oracle, random_multi_grid

pytestmark = pytest.mark.gpu
SOAK = int(os.environ.get("MGX_FUZZ_SEED", "0"))          # soak runs: another draw of every batch / episode / action sequence

# (ng, nb, nr, nl, npv), H: the register form (at most two of a kind: one launch) and the run-time-count form (two launches)
CASES = [((2, 2, 1, 1, 1), 0), ((2, 2, 1, 1, 1), 3), ((1, 2, 2, 1, 1), 1), ((3, 1, 2, 2, 1), 2)]


def _batch(counts, H, device, N, T):
    from pymgrid_amd.generator import generate, widen
    ng, nb, nr, nl, npv = counts
    base = generate(N, n_steps=T, seed=41 + 1000 * SOAK, arch="genset+battery+grid", device=device, horizon=H, mixed_timers=True)
    return widen(base, n_genset=ng, n_battery=nb, n_grid=nr, n_load=nl, n_pv=npv)


def _first_draw(layout, length, N, rs):
    """(starts, lengths) of the first episodes: FixedLengthStochasticTrajectory (lengths None) or StochasticTrajectory."""
    lo, hi = layout.initial_step, layout.final_step
    if length is not None:
        return rs.randint(lo, hi - length, size=N).astype(np.int32), None
    starts = rs.randint(lo, hi - 2, size=N)
    finals = np.array([rs.randint(s, hi) for s in starts])
    return starts.astype(np.int32), np.maximum(finals - starts, 1).astype(np.int32)


@pytest.fixture
def multi_small_own():
    """Sets the multi_small_own tunable (0: mgx_step_lists takes expand_multi_kernel + step_multi_kernel<F, true> on every layout);
    the value it had is restored after the test."""
    from pymgrid_amd import _lib
    old = _lib.get_tunable("multi_small_own")[0]
    yield lambda v: _lib.set_tunable("multi_small_own", v)
    _lib.set_tunable("multi_small_own", old)


def _run_discrete_auto_reset(counts, H, length, device, steps, twin=True, N=1000, T=200):
    """Steps a discrete auto-reset env with device draws; with `twin`, a continuous one fed the expanded controls beside it, every
    output `==`.  Returns what the discrete env produced (host copies) and the number of restarts."""
    from pymgrid_amd.hetero import PerGridWindowEnv
    disc = PerGridWindowEnv(_batch(counts, H, device, N, T), trajectory_length=length, discrete=True, auto_reset=True, seed=13 + SOAK,
                            remove_redundant_gensets=False)
    cont = PerGridWindowEnv(_batch(counts, H, device, N, T), trajectory_length=length, auto_reset=True, seed=13 + SOAK) if twin else None
    assert disc.native and disc.env._ring is None
    rs = np.random.RandomState(3 + SOAK)
    starts, lengths = _first_draw(disc.env.layout, length, N, rs)
    o_d = disc.reset(starts, lengths)
    if twin:
        assert torch.equal(o_d, cont.reset(starts, lengths))
    g = torch.Generator(device=device); g.manual_seed(7 + SOAK)
    rec, restarts = [o_d.cpu()], 0
    for k in range(steps):
        ids = torch.randint(0, disc.action_space.n, (N,), dtype=torch.int32, device=device, generator=g)
        ctrl = disc.env.get_action(ids) if twin else None       # (before the step: the rows the step reads)
        o1, r1, d1, _ = disc.step(ids)
        restarts += int(d1.sum())
        rec += [o1.cpu(), r1.cpu(), d1.cpu(), disc.starts.cpu(), disc.lengths.cpu(), disc.env.current_steps.cpu()]
        if twin:
            o2, r2, d2, _ = cont.step(ctrl, normalized=False)
            assert torch.equal(r1, r2) and torch.equal(d1, d2), k
            assert torch.equal(o1, o2), k
            assert torch.equal(disc.starts, cont.starts) and torch.equal(disc.lengths, cont.lengths), k
            assert torch.equal(disc.env.current_steps, cont.env.current_steps), k
    for name in ("charge", "soc", "gen_status"):
        rec.append(disc.env.batch.cols[name].cpu())
        if twin:
            assert torch.equal(disc.env.batch.cols[name], cont.env.batch.cols[name]), name
    disc.env.close()
    if twin:
        cont.env.close()
    return rec, restarts


@pytest.mark.parametrize("counts,H", CASES)
@pytest.mark.parametrize("length", [9, None])
def test_discrete_auto_reset_equals_its_continuous_twin(counts, H, length, device):
    """PerGridWindowEnv(discrete=True, auto_reset=True) on a widen(...) batch == PerGridWindowEnv(auto_reset=True) stepped with the
    controls the priority lists expand to: observations, rewards, done flags, the kernel's draws (starts, lengths), every grid's
    step counter, and the final state -- through more restarts than grids."""
    N = 1000
    _, restarts = _run_discrete_auto_reset(counts, H, length, device, steps=64 if length else 150, N=N)
    assert restarts > N, restarts


@pytest.mark.parametrize("counts,H", CASES[:3])
def test_one_launch_equals_two_launches(counts, H, device, multi_small_own):
    """The one-launch in-place step (step_lists_small_kernel<F, true>, the restart in the kernel) == expansion + step_multi_kernel<F,
    true> (multi_small_own = 0), bit for bit."""
    multi_small_own(1)
    one, n1 = _run_discrete_auto_reset(counts, H, 9, device, steps=64, twin=False)
    multi_small_own(0)
    two, n2 = _run_discrete_auto_reset(counts, H, 9, device, steps=64, twin=False)
    assert n1 == n2 and len(one) == len(two)
    for k, (a, b) in enumerate(zip(one, two)):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("length", [9, None])
def test_two_launches_equal_the_continuous_twin(length, device, multi_small_own):
    """The two-launch fallback (expansion, then step_multi_kernel<F, true>) honours auto-reset in-place episodes too."""
    multi_small_own(0)
    _run_discrete_auto_reset((2, 2, 1, 1, 1), 0, length, device, steps=64 if length else 150, N=600)


@pytest.mark.parametrize("counts,H", [((2, 2, 1, 1, 1), 0), ((1, 2, 2, 1, 1), 2), ((3, 1, 2, 2, 1), 2)])
def test_inplace_discrete_episodes_equal_gathered_windows(counts, H, device):
    """Discrete steps of in-place episodes without auto-reset (reset_windows(rolling="inplace"), one reset_grids restart) == the same
    episodes on gathered window buffers, step by step; then mgx_step_lists without a control buffer runs in place (one launch) where
    the layout holds at most two modules of a kind."""
    from pymgrid_amd import DiscreteBatchedMicrogridEnv
    N, T, Lg = 700, 160, 9
    inpl = DiscreteBatchedMicrogridEnv(_batch(counts, H, device, N, T), obs_prefetch=0, remove_redundant_gensets=False)
    gath = DiscreteBatchedMicrogridEnv(_batch(counts, H, device, N, T), obs_prefetch=0, remove_redundant_gensets=False)
    rs = np.random.RandomState(8 + SOAK)
    g = torch.Generator(device=device); g.manual_seed(2 + SOAK)

    def episode(first_a, first_b):
        assert torch.equal(first_a, first_b)
        for k in range(Lg):
            ids = torch.randint(0, inpl.action_space.n, (N,), dtype=torch.int32, device=device, generator=g)
            (o1, r1, d1, _), (o2, r2, d2, _) = inpl.step(ids), gath.step(ids)
            assert torch.equal(r1, r2) and torch.equal(d1, d2), k
            assert torch.equal(o1, o2), k
            assert bool(d1.all()) == (k == Lg - 1) and bool(d1.any()) == (k == Lg - 1)
    starts = rs.randint(0, T - Lg + 1, size=N).astype(np.int32)
    starts[:3] = (0, T - Lg, 1)
    episode(inpl.reset_windows(starts, None, max_length=Lg, rolling="inplace"), gath.reset_windows(starts, None, max_length=Lg))
    starts2 = rs.randint(0, T - Lg + 1, size=N).astype(np.int32)
    every = torch.ones(N, dtype=torch.uint8, device=device)
    episode(inpl.reset_grids(every, starts2, None), gath.reset_windows(starts2, None, max_length=Lg))
    for name in ("charge", "soc", "gen_status"):
        assert torch.equal(inpl.batch.cols[name], gath.batch.cols[name]), name
    if max(counts) <= 2:
        # the C ABI: a small layout in place steps without the control buffer (the two-launch form would refuse a NULL one)
        starts3 = rs.randint(0, T - Lg + 1, size=N).astype(np.int32)
        inpl.reset_grids(every, starts3, None)
        gath.reset_windows(starts3, None, max_length=Lg)
        e = inpl.engine
        ids = torch.randint(0, inpl.action_space.n, (N,), dtype=torch.int32, device=device, generator=g)
        reward = torch.empty(N, dtype=torch.float64, device=device)
        e._call(e._lib.mgx_step_lists, ids.data_ptr(), inpl._lists.data_ptr(), int(inpl._lists.shape[0]), int(inpl._lists.shape[1]),
                None, reward.data_ptr(), None, None, None)
        _, r2, _, _ = gath.step(ids)
        assert torch.equal(reward, r2)
    inpl.close(); gath.close()


@pytest.mark.parametrize("length", [6, None])
def test_generator_drawn_episodes_vs_the_oracle(length, device, oracle):
    """PerGridWindowEnv(discrete=True, auto_reset=True, generator=g) on 48 grids built from module lists: every grid's sequence of
    episodes (start, length at each restart) and priority lists replayed on the multi-instance CPU oracle (populate_action, run; a
    restart moves the counter and keeps the state) -- rewards, done flags, observation rows and the final state `==`
    (layouts.episodes_vs_oracle)."""
    from pymgrid_amd import MicrogridBatch
    from pymgrid_amd.hetero import PerGridWindowEnv
    N, T, K = 48, 40, 60
    rs = np.random.RandomState(17 + SOAK)
    grids = [random_multi_grid(rs, T, 2, 2, 1, 1, 1) for _ in range(N)]
    gen = torch.Generator(device=device); gen.manual_seed(23 + SOAK)
    env = PerGridWindowEnv(MicrogridBatch.from_grids(grids, device=device), trajectory_length=length, discrete=True, auto_reset=True,
                           generator=gen, remove_redundant_gensets=False)
    assert env.native and not env._device_draws
    restarts = episodes_vs_oracle(oracle, env, grids, K, lambda k: rs.randint(0, env.action_space.n, size=N))
    assert int(restarts.sum()) > N                                   # more restarts than grids
    env.env.close()


@pytest.mark.parametrize("discrete", [False, True])
def test_multi_auto_reset_refusals_kept(discrete, device):
    """final_observation and native=False stay refused with several modules of a kind per grid, whatever draws the episodes."""
    from pymgrid_amd.hetero import PerGridWindowEnv
    b = _batch((2, 2, 1, 1, 1), 0, device, 64, 60)
    kw = dict(remove_redundant_gensets=False) if discrete else {}
    gen = torch.Generator(device=device)
    for g in (None, gen):
        with pytest.raises(NotImplementedError):
            PerGridWindowEnv(b, trajectory_length=9, discrete=discrete, auto_reset=True, generator=g, final_observation=True, **kw)
        with pytest.raises(NotImplementedError):
            PerGridWindowEnv(b, trajectory_length=9, discrete=discrete, auto_reset=True, generator=g, native=False, **kw)
