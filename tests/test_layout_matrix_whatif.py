"""The what-if kernels -- lookahead_episodes_kernel, lookahead_step_k_episodes_kernel and lookahead_gaussian_episodes_kernel (CEM) --
in EVERY compiled form: all ten module layouts x shared / per-grid plans x the control type x the three row sources, on batches
carved out of one generated batch (tests/layouts.py), with the comparisons of test_lookahead.py and test_cem.py (the launch == twin
envs rolled out and reduced by ``lookahead_host``; the drawing launch == the per-grid launch over ``cem_candidates_host``).  Over
those files this one adds: the seven layouts beside 7, 3 and 6 with the grid-major copy and the gather, with plans shared by all
grids and with float32 controls; CEM on the six layouts it never ran on -- and, per layout, an independent replay: the CPU oracle
runs every candidate plan from the state the call found."""
import numpy as np
import pytest
import torch

import test_cem as cem_tests
import test_lookahead as lookahead_tests
from layouts import LAYOUTS, carve, walked
from test_layout_matrix_episodes import SOURCES, rotate

F64, F32 = torch.float64, torch.float32
LENGTHS, ONOFF, GAMMAS, PREFIXES, NORMALIZED = (9, None), (False, True), (1.0, 0.9), (0, 5), (True, False)
C_, H = 4, 9                      # four candidates (candidate 3 copies candidate 1), nine steps: beyond both ring depths (4 / 8)
CONTROLLED = tuple(f for f in LAYOUTS if f & 7)              # the continuous calls plan controls: layout 0 has none (REFUSED)

# (layout, series, length, shaper, gamma, prefix, per_grid) -- one case per form of lookahead_episodes_kernel
DISCRETE_CASES = rotate(LAYOUTS, (False, True), LENGTHS, ONOFF, GAMMAS, PREFIXES)
# (layout, series, length, shaper, gamma, normalized, per_grid, control type, prefix) -- one case per form of
# lookahead_step_k_episodes_kernel a call reaches; the prefix goes with the control type, flipped from layout to layout
CONTINUOUS_CASES = tuple(c + (dt, PREFIXES[(di + CONTROLLED.index(c[0])) % 2]) for di, dt in enumerate((F64, F32))
                         for c in rotate(CONTROLLED, (False, True), LENGTHS, ONOFF, GAMMAS, NORMALIZED))
# (layout, series, length, shaper, gamma, control type) -- one case per form of lookahead_gaussian_episodes_kernel
CEM_CASES = tuple(c[:-1] for c in rotate(CONTROLLED, (None,), LENGTHS, ONOFF, GAMMAS, (F64, F32)))
# Compiled forms no call reaches: the continuous what-if launch on the layout without a controllable module -- there is no control
# to plan, the plan tensor is empty and the call refuses it (test_the_refused_forms_are_refused_and_nothing_is_launched).
# (kernel, compile-time part): (layout, control type, per_grid, row source)
REFUSED = tuple(("lookahead_step_k_episodes_kernel", (0, at, pg, src)) for at in ("double", "float") for pg in (False, True) for src in (0, 1, 2))


def test_the_rotation_gives_every_layout_every_value_of_every_factor():
    for cases, layouts, per_layout, factors in (
            (DISCRETE_CASES, LAYOUTS, 6, (LENGTHS, ONOFF, GAMMAS, PREFIXES, (False, True))),
            (CONTINUOUS_CASES, CONTROLLED, 12, (LENGTHS, ONOFF, GAMMAS, NORMALIZED, (False, True), (F64, F32), PREFIXES)),
            (CEM_CASES, CONTROLLED, 3, (LENGTHS, ONOFF, GAMMAS, (F64, F32)))):
        assert len(set(cases)) == len(cases) == per_layout * len(layouts)
        by_layout = {}
        for c in cases:
            by_layout.setdefault(c[0], []).append(c[1:])
        assert set(by_layout) == set(layouts)
        for flags, cs in by_layout.items():
            assert len(cs) == per_layout and {c[0] for c in cs} == set(SOURCES)
            for column, values in zip(list(zip(*cs))[1:], factors):
                assert set(column) == set(values), (flags, column)
    # the compile-time factors are crossed with layout and source
    assert {(c[0], c[1], c[6]) for c in DISCRETE_CASES} == {(f, s, pg) for f in LAYOUTS for s in SOURCES for pg in (False, True)}
    assert {(c[0], c[1], c[6], c[7]) for c in CONTINUOUS_CASES} == {(f, s, pg, dt) for f in CONTROLLED for s in SOURCES for pg in (False, True)
                                                                   for dt in (F64, F32)}


def carved(device, flags, series, H=0, n=lookahead_tests.N):
    """The batch factory of both helpers: layout `flags` carved out of the genset+battery+grid batch they would generate
    (mixed_timers=True kept)."""
    return carve(lookahead_tests._batch(device, "genset+battery+grid", series, H, n=n), flags)


def _carved_cem(device, flags, series, n=cem_tests.N):
    return carve(cem_tests._batch(device, "genset+battery+grid", series, n=n), flags)


def _done_of(trace):
    """[H, N] done flags out of the episodes the call found (trace["left"]: step number ``left`` of a grid is its episode's last)."""
    k = torch.arange(1, H + 1, device=trace["left"].device)
    return k[:, None] == trace["left"][None, :]


def _not_vacuous(trace, length):
    """The episodes the call found ALONE: every grid has a step left; at own lengths the lanes of a wave stop at more than two
    different steps, and some reach H."""
    assert int(trace["left"].min()) >= 1
    if length is None:
        counted = trace["left"].clamp(max=H)
        assert counted.unique().numel() > 2 and int(counted.max()) == H, counted.unique().tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("flags,series,length,shaper,gamma,prefix,per_grid", DISCRETE_CASES)
def test_discrete_lookahead_equals_twin_rollouts(flags, series, length, shaper, gamma, prefix, per_grid, device):
    trace = {}
    lookahead_tests._lookahead_equals_twin_rollouts(device, flags, series, length, H, shaper, per_grid, gamma, prefix, 0, True,
                                                    make_batch=carved, n_candidates=C_, trace=trace)
    _not_vacuous(trace, length)


@pytest.mark.gpu
@pytest.mark.parametrize("flags,series,length,shaper,gamma,normalized,per_grid,dtype,prefix", CONTINUOUS_CASES)
def test_continuous_lookahead_equals_twin_step_k(flags, series, length, shaper, gamma, normalized, per_grid, dtype, prefix, device):
    trace = {}
    lookahead_tests._lookahead_equals_twin_rollouts(device, flags, series, length, H, shaper, per_grid, gamma, prefix, 0, False, dtype,
                                                    normalized, make_batch=carved, n_candidates=C_, trace=trace)
    _not_vacuous(trace, length)


@pytest.mark.gpu
@pytest.mark.parametrize("flags,series,length,shaper,gamma,dtype", CEM_CASES)
def test_cem_launch_equals_the_per_grid_launch_over_the_host_candidates(flags, series, length, shaper, gamma, dtype, device):
    trace = {}
    cem_tests._launch_equals_the_per_grid_launch(device, flags, series, length, H, shaper, gamma, dtype, make_batch=_carved_cem,
                                                 n_candidates=C_, trace=trace)
    _not_vacuous(trace, length)


@pytest.mark.gpu
def test_the_refused_forms_are_refused_and_nothing_is_launched(device):
    """REFUSED: on layout 0 the continuous what-if calls have no control to plan -- the Python surface and the C call refuse the
    empty plan tensor (and CEM the layout: it holds no kernel for it), the handle stays where it was and ``ret`` keeps its bytes."""
    import ctypes as C
    from pymgrid_amd import _lib
    from pymgrid_amd.hetero import PerGridWindowEnv
    assert {part[0] for _, part in REFUSED} == {0}
    for dtype in (F64, F32):
        pe = PerGridWindowEnv(carved(device, 0, "factorised"), trajectory_length=9, discrete=False, auto_reset=True, seed=23, action_dtype=dtype)
        pe.reset()
        e, n = pe.env.engine, lookahead_tests.N
        assert e.action_dim == 0
        snap = lookahead_tests._snapshot(pe)
        for plans in (torch.zeros(C_, H, 0, dtype=dtype, device=device), torch.zeros(C_, H, n, 0, dtype=dtype, device=device)):
            with pytest.raises(ValueError, match="plans must be"):
                e.lookahead_step_k_episodes(plans)
        with pytest.raises(Exception):
            e.lookahead_gaussian_episodes(torch.zeros(H, n, 0, dtype=F64, device=device), torch.zeros(H, n, 0, dtype=F64, device=device), C_, 1)
        ret = torch.full((C_, n), float("nan"), dtype=F64, device=device)
        la = _lib.Lookahead()
        la.struct_size, la.C, la.H, la.gamma, la.ret = C.sizeof(_lib.Lookahead), C_, H, 1.0, ret.data_ptr()
        for per_grid in (0, 1):
            la.per_grid = per_grid
            assert e._lib.mgx_lookahead_step_k_episodes(e._h, None, 1, C.byref(la), None) == _lib.MGX_ERR_INVALID
            assert b"mgx_lookahead_step_k_episodes" in e._lib.mgx_last_error()
        torch.cuda.synchronize()
        lookahead_tests._untouched(pe, snap)
        assert bool(torch.isnan(ret).all())
        pe.env.close()


# ---- the independent check: the oracle runs every candidate plan from the state the call found ------------------------------------
def _oracle_what_if(oracle, trace, gamma, normalized=True):
    """From the snapshot before the call (state columns, every grid's series row) the oracle steps every candidate plan H steps on
    rows t0 .. t0 + H - 1 of each grid (past the end of its episode: no longer counted, clamped into the series); ``lookahead_host``
    of ITS rewards and the done flags of the episodes the call found (the twins', where there are twins) must be what the call
    returned, and its SoC after the last counted step ``end_soc``."""
    from pymgrid_amd import lookahead_host
    cols, out, plans = trace["cols"], trace["out"], trace["plans"]
    n_cand, Hs = plans.shape[0], plans.shape[1]
    t0 = trace["rows"].cpu().numpy().astype(np.int64)
    rows = np.minimum(t0[None, :] + np.arange(Hs)[:, None], cols["layout"]["T"] - 1)
    series = walked(cols, rows)
    n = rows.shape[1]
    rewards, socs = [], []
    for c in range(n_cand):
        st = {k: cols[k].copy() for k in ("charge", "soc", "gen_status") if k in cols}
        failed = np.zeros(n, dtype=np.uint8)
        reward, soc = [], []
        p = plans[c].cpu().numpy() if trace["table"] is not None else plans[c].double().cpu().numpy()
        for k in range(Hs):                                   # step by step: the SoC after every step
            if trace["table"] is not None:
                reward.append(oracle.rollout_batch(series, st, k, 1, p[k:k + 1], trace["table"], nthreads=8, failed=failed)[0])
            else:
                reward.append(oracle.run_batch(series, st, k, 1, p[k:k + 1], normalized=normalized, nthreads=8, failed=failed)[0])
            if "soc" in st:
                soc.append(st["soc"].copy())
        assert int(failed.sum()) == 0, f"candidate {c}: the oracle left out {int(failed.sum())} of {n} grids"
        rewards.append(np.stack(reward))
        if soc:
            socs.append(np.stack(soc))
    device = out["ret"].device
    done = _done_of(trace)
    if "done" in trace:                                       # the twins ended their episodes where the snapshot says
        first = lambda d: torch.where(d.any(dim=0), d.int().argmax(dim=0), torch.full_like(d[0], H, dtype=torch.int64))     # noqa: E731
        assert torch.equal(first(done), first(trace["done"]))
    ref = lookahead_host(torch.as_tensor(np.stack(rewards)).to(device), done, gamma)
    for name in ("ret", "steps", "best", "best_ret"):
        assert torch.equal(out[name], ref[name]), name
    if socs:
        last = ref["last"].cpu().numpy()
        want = np.stack([s[last, np.arange(n)] for s in socs])
        assert torch.equal(out["end_soc"], torch.as_tensor(want).to(device))


# (layout, source, length, gamma): once per layout, the source, the length and gamma rotating over the layouts
# ... for each of the three families; the continuous ones where there is a control to plan (layout 0: REFUSED, asserted above)
ORACLE_CASES = tuple((flags, SOURCES[li % 3], LENGTHS[li % 2], GAMMAS[(li // 2) % 2], family) for li, flags in enumerate(LAYOUTS)
                     for family in ("discrete", "continuous", "cem") if family == "discrete" or flags in CONTROLLED)


@pytest.mark.gpu
@pytest.mark.parametrize("flags,series,length,gamma,family", ORACLE_CASES)
def test_what_if_launches_vs_the_oracle(flags, series, length, gamma, family, device, oracle):
    """No shaper, no forecast horizon (the oracle's reward is the unshaped one); per-grid plans on every other layout, raw controls
    on every third."""
    li = LAYOUTS.index(flags)
    trace = {}
    normalized = bool(li % 3)
    if family == "discrete":
        lookahead_tests._lookahead_equals_twin_rollouts(device, flags, series, length, H, False, bool(li % 2), gamma, 5, 0, True,
                                                        make_batch=carved, n_candidates=C_, trace=trace)
    elif family == "continuous":
        lookahead_tests._lookahead_equals_twin_rollouts(device, flags, series, length, H, False, bool(li % 2), gamma, 5, 0, False, F64,
                                                        normalized, make_batch=carved, n_candidates=C_, trace=trace)
    else:
        normalized = True
        cem_tests._launch_equals_the_per_grid_launch(device, flags, series, length, H, False, gamma, F64, make_batch=_carved_cem,
                                                     n_candidates=C_, trace=trace)
    _oracle_what_if(oracle, trace, gamma, normalized)
