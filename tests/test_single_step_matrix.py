"""The single-step family -- the Gym step, one launch per env-step -- against the CPU oracle on ALL ten module layouts, one case per
compiled form: step_kernel<F, EP>, step_discrete_kernel<F, EP>, observe_kernel<F>, expand_kernel<F>, obs_rows_wave_kernel<F, NOISE, OT>,
obs_windows_k_kernel<F, OT>, obs_windows_k_multi_kernel<F, OT>, patch_windows_kernel<GRID, OT>, normalise_series_kernel<C, OT> and the
three fleet kernels.  Every grid of every case is compared, bit for bit, with an ``oracle.OracleMicrogrid`` of its own
(layouts.OracleSingles: ``run``, ``observe``, ``reset``, ``populate_action``): reward, done, every log column the oracle produces,
observation rows (float32 rows: the oracle's row rounded) and the state columns at the end.  No comparison is between two device forms
and none has a tolerance; the rows of the noisy forecaster, which has no host rule, are held to properties.

The batches are carved out of one generated batch (layouts.carve): N = 333 grids are three workgroups of BLOCK = 128, the third of one
full wave -- whose H = 0 rows go through the wave-private row tile of ``store_step_obs`` -- and a wave of 13 lanes, which takes the
per-lane path; the 16-grid window groups are 20 full ones and one of 13.  A launch sequence is 6 steps from row 3, then a reset near
the end and steps to the last row: the end-of-series padding, and the last step reports done.  The reference side of every case is
built once (``*_reference``) with the conditions on its inputs asserted; tests/test_layouts.py runs them without a GPU and checks
that the case tuples below name every instantiation the library holds.

The dry run (check_kernel<F>, check_discrete_kernel<F>, action_bounds_kernel<F>) is held against recorded behaviour of the real
reference with ``raise_errors=True`` (tests/golden/raise_errors.npz), which the oracle does not produce.  The shard bounds of mgx_set_shards are multiples of 256
grids, so the two-shard cases split 333 grids into 256 + 77 and every wave still starts at a multiple of 64."""
import functools
import itertools

import numpy as np
import pytest

import layouts as ly

N, T, T0, SEED = 333, 60, 3, 21
STEPS, TAIL = 6, 3                            # steps from row T0; steps from row T - TAIL to the last row of the series
BLOCK = 128                                   # BLOCK of csrc/mgx_core.hpp: grids per workgroup of the single-step kernels
HORIZONS = (3, 30)                            # one partial round of the 28 window slots; a second round
LENGTH, EPISODE_STEPS = 5, 12                 # per-grid episodes: every grid restarts twice
PREFETCH = 4                                  # blocks per observation ring: the 6 steps cross a refill
SERIES = ("materialised", "factorised")
FLOATS = ("double", "float")


def horizon_of(flags, shift=0):
    """H = 3 and H = 30 alternating over the layouts (``shift``: the other way round), so that every layout sees both."""
    return HORIZONS[(ly.LAYOUTS.index(flags) + shift) % 2]


# ---- the cases: every tuple names compile-time parts through compiled_forms() ----------------------------------------------------
# lock-step, H = 0: (layout, row type, control type, series, rows at an odd element offset of a larger buffer, how the steps are issued)
LOCKSTEP_CASES = tuple((f, ot, at, series, odd, "step") for f in ly.LAYOUTS for ot, at, series, odd in
                       itertools.product(FLOATS, FLOATS, SERIES, (False, True))) \
    + tuple((f, FLOATS[i % 2], "double", SERIES[i % 2], False, how) for i, f in enumerate(ly.LAYOUTS) for how in ("shards", "many"))
# rows with a forecast horizon: (layout, H, row type, noise std: None = the oracle forecaster)
ROWS_CASES = tuple((f, horizon_of(f, i), ot, noise) for f in ly.LAYOUTS for i, ot in enumerate(FLOATS) for noise in (None, 0.0, 1.0))
# prefetched rings: (layout, H, row type, ring layout)
RING_CASES = tuple((f, horizon_of(f, i + j), ot, ring) for f in ly.LAYOUTS for i, ot in enumerate(FLOATS)
                   for j, ring in enumerate(("rows", "columns")))
# observation views: (layout, H, row type)
VIEW_CASES = tuple((f, horizon_of(f, i), ot) for f in ly.LAYOUTS for i, ot in enumerate(FLOATS))
# lock-step discrete steps: (layout,)
DISCRETE_CASES = tuple((f,) for f in ly.LAYOUTS)
# in-place per-grid episodes: (layout, discrete, H: 0 = whole rows written by the step kernel, else rings patched behind it, row type)
EPISODE_CASES = tuple((f, discrete, 0, FLOATS[(i + discrete) % 2]) for i, f in enumerate(ly.LAYOUTS) for discrete in (False, True)) \
    + tuple((f, bool((i + j) % 2), horizon_of(f, j), ot) for i, f in enumerate(ly.LAYOUTS) for j, ot in enumerate(FLOATS))

# the dry run against recorded behaviour of the real reference (tests/golden/raise_errors.npz): (layout, raw requests or normalised ones)
DRY_RUN_CASES = tuple((f, raw) for f in ly.LAYOUTS for raw in (True, False))

# compiled, but out of every call's reach: a layout without a controllable module has an empty control row [N, 0], whose device
# pointer is NULL, so mgx_expand_discrete has no buffer to expand into and returns MGX_ERR_INVALID (asserted below); the fused
# discrete step of that layout needs no control row and runs (DISCRETE_CASES)
# ... and the strict action bounds of a layout with a genset: the reference's sample_action(strict_bound=True) fails on a GensetModule,
# so the env raises TypeError before it asks the engine (asserted in the dry-run cases)
# (layout 0 has no action column: mgx_action_bounds has no buffer to write and returns MGX_ERR_INVALID)
REFUSED = (("expand_kernel", (0,)),) + tuple(("action_bounds_kernel", (f,)) for f in ly.LAYOUTS if f & ly.F_GENSET or not f)


def compiled_forms(kind, case):
    """{(kernel, compile-time part)} the calls of a case launch: the dispatch of csrc/mgx_abi.hip (mgx_step, mgx_step_many,
    mgx_observe, mgx_reset, mgx_step_discrete, mgx_expand_discrete, mgx_observe_windows, mgx_patch_windows, mgx_normalise_series),
    stated once.  tests/test_layouts.py holds this against the instantiations the library has."""
    f = case[0]
    if kind == "lockstep":                                      # whole H = 0 rows: the step kernel writes them, mgx_observe's kernel
        return {("step_kernel", (f, False)), ("observe_kernel", (f,))}
    if kind == "rows":                                          # H > 0 without rings: the row kernel behind every step and reset
        _, H, ot, noise = case
        return {("step_kernel", (f, False)), ("obs_rows_wave_kernel", (f, noise is not None, ot))}
    if kind == "ring":                                          # the ring refill; a step adds the state columns (state-only rows)
        return {("step_kernel", (f, False)), ("obs_windows_k_kernel", (f, case[2]))}
    if kind == "views":                                         # the series normalised once: load and pv (C = 1), the grid's four (C = 4)
        return {("step_kernel", (f, False)), ("normalise_series_kernel", (1, case[2]))} \
            | ({("normalise_series_kernel", (4, case[2]))} if f & ly.F_GRID else set())
    if kind == "discrete":
        return {("step_discrete_kernel", (f, False))} | ({("expand_kernel", (f,))} if f else set())
    if kind == "episodes":
        _, discrete, H, ot = case
        out = {("step_discrete_kernel" if discrete else "step_kernel", (f, True))}
        if H:                                                   # rings: the restarted grids' window columns are patched into them
            out.add(("patch_windows_kernel", (bool(f & ly.F_GRID), ot)))       # (the refill itself is the ring cases' to claim)
        return out
    if kind == "dry_run":                                       # mgx_check_step, mgx_check_discrete, mgx_action_bounds
        return {("check_kernel", (f,)), ("check_discrete_kernel", (f,))} | (set() if f & ly.F_GENSET or not f else {("action_bounds_kernel", (f,))})
    if kind == "fleet":                                         # (form, which fleet, discrete): the one kernel of the form
        return {FLEET_KERNELS[case[0]]}
    if kind == "multi":                                         # the ring refill of the general path
        return {("obs_windows_k_multi_kernel", case)}
    raise ValueError(kind)


# the families whose every instantiation is a case of the tables above, or named in REFUSED (tests/test_layouts.py)
FAMILIES = ("step_kernel", "step_discrete_kernel", "observe_kernel", "expand_kernel", "obs_rows_wave_kernel", "obs_windows_k_kernel",
            "patch_windows_kernel", "normalise_series_kernel", "obs_windows_k_multi_kernel", "fleet_step_kernel", "fleet_step_kernel_v",
            "check_kernel", "check_discrete_kernel", "action_bounds_kernel")


def all_cases():
    """(kind, cases) of every table of the file."""
    return (("lockstep", LOCKSTEP_CASES), ("rows", ROWS_CASES), ("ring", RING_CASES), ("views", VIEW_CASES),
            ("discrete", DISCRETE_CASES), ("episodes", EPISODE_CASES), ("fleet", FLEET_CASES), ("multi", MULTI_CASES), ("dry_run", DRY_RUN_CASES))


def _id(case):
    return "-".join("noise%g" % v if isinstance(v, float) else str(v) for v in case)


# ---- the golden of the dry run --------------------------------------------------------------------------------------------------
GOLDEN_NONE, GOLDEN_VALUE_ERROR, GOLDEN_ASSERTION_ERROR, GOLDEN_ABSENT = 0, 1, 2, -1       # exception classes, as the script writes them
GOLDEN_AT_LIMIT, GOLDEN_BEYOND = 0, 1                                                      # how a raw request was drawn
GOLDEN_TILES = 42             # the 8 raw (or the 8 normalised) grids of a layout 42 times: N = 336, two workgroups and a wave of 16 lanes


@functools.lru_cache(maxsize=None)
def raise_errors_golden(flags):
    """Layout ``flags`` of tests/golden/raise_errors.npz (make_raise_errors_goldens.py): the 16 parameter dicts, and per step and
    grid the requests, the exception class of every controllable module (genset, battery, grid) with ``raise_errors=True``, how a raw
    request was drawn, the normalised strict bounds, the same for a random priority list, and the state after the last step."""
    import json
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raise_errors.npz"), allow_pickle=False)
    grids, raw = [], []
    for mt in json.loads(str(z["meta"])):
        if mt["layout"] == flags:
            p = {k: v for k, v in mt.items() if k not in ("layout", "index", "raw")}
            for name in ("load_ts", "pv_ts") + (("grid_ts",) if "grid" in p else ()):
                p[name] = z[f"f{flags}_g{mt['index']}_{name}"]
            grids.append(p)
            raw.append(mt["raw"])
    out = {name: z[f"f{flags}_{name}"] for name in ("requests", "exception", "how", "bounds", "ids", "list_exception", "table",
                                                    "charge", "soc", "status")}
    out.update(grids=grids, raw=np.array(raw))
    return out


# ---- inputs and the reference side (no GPU) ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _full(series, H):
    from pymgrid_amd.generator import generate
    return generate(N, n_steps=T, seed=SEED, arch="genset+battery+grid", device="cpu", mixed_timers=True, series=series, horizon=H)


@functools.lru_cache(maxsize=None)
def columns(flags, H):
    """Host columns of the carved batch, the oracle's input: shared by the cases of a layout and left unchanged."""
    return ly.carve(_full("materialised", H), flags).numpy_columns()


def device_batch(flags, H, series, device, noise=None):
    """The carved batch on the device: copies of the very columns the reference side reads.  ``noise``: the std of the Gaussian
    forecaster (the three ``*_noise_std`` columns; 0.0: a noisy forecaster that adds nothing)."""
    import torch
    from pymgrid_amd import MicrogridBatch
    sub = ly.carve(_full(series, H), flags)
    cols = {k: (t[:1].to(device).expand(t.shape[0]) if t.dim() == 1 and t.shape[0] > 1 and t.stride(0) == 0 else t.to(device).contiguous())
            for k, t in sub.cols.items()}
    forecast = None
    if noise is not None:
        for name, scale in (("load_noise_std", 3.0), ("pv_noise_std", 2.0)) + ((("grid_noise_std", 0.05),) if flags & ly.F_GRID else ()):
            cols[name] = torch.full((N,), scale * noise, dtype=torch.float64, device=device)
        forecast = dict(seed=9, increase_uncertainty=True)
    return MicrogridBatch(sub.layout, cols, forecast_noise=forecast)


def action_dim(flags):
    return 2 * bool(flags & ly.F_GENSET) + bool(flags & ly.F_BATTERY) + bool(flags & ly.F_GRID)


def _frozen(ref):
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def _assert_genset_forms(rec, flags, label):
    """Every form of the genset status word the timers give occurs among the records: off, on, starting up, winding down."""
    if flags & ly.F_GENSET:
        seen = set(zip(rec["gen_cur"].ravel().tolist(), rec["gen_goal"].ravel().tolist()))
        assert seen == {(0, 0), (1, 1), (0, 1), (1, 0)}, (label, seen)
        assert (rec["gen_up"] > 0).any() and (rec["gen_down"] > 0).any(), label


@functools.lru_cache(maxsize=None)
def lockstep_reference(flags, H, ctype):
    """The launch sequence on the oracle: reset to row T0, STEPS steps, reset to row T - TAIL, TAIL steps to the last row.  Controls
    U[0, 1), every seventh row rounded to exact 0 / 1 (float32 controls: the oracle takes them widened, what the kernels do).  Any
    exception of the oracle fails: no grid is left out."""
    from oracle import oracle as orc
    orc.build()
    og = ly.OracleSingles(orc, columns(flags, H))
    rs = np.random.RandomState(1000 * flags + 10 * H + FLOATS.index(ctype))
    a = rs.rand(STEPS + TAIL, N, action_dim(flags))
    a[::7] = np.round(a[::7])
    if ctype == "float":
        a = a.astype(np.float32)
    wide = a.astype(np.float64)
    ref = dict(controls=a, obs0=og.reset(T0))
    rec, obs = og.run(wide[:STEPS], True, observe=True)
    ref["obs_end0"] = og.reset(T - TAIL)
    rec_end, obs_end = og.run(wide[STEPS:], True, observe=True)
    ref.update(rec=np.concatenate([rec, rec_end]), obs=np.concatenate([obs, obs_end]), state=og.state())
    # the conditions on the inputs
    done = ref["rec"]["done"].astype(bool)
    assert bool(done[-1].all()) and not bool(done[:-1].any()), (flags, "both values of done, the last step alone ends the series")
    assert og.rows().tolist() == [T] * N
    _assert_genset_forms(ref["rec"], flags, (flags, H, ctype))
    assert np.isfinite(ref["rec"]["reward"]).all() and np.isfinite(ref["obs"]).all()
    assert H == 0 or T - TAIL + H > T - 1, "a window of the last rows runs into the padding behind the series"
    return _frozen(ref)


def priority_lists(flags):
    from pymgrid_amd.priority_list import get_priority_lists
    return get_priority_lists(bool(flags & ly.F_GENSET), bool(flags & ly.F_BATTERY), bool(flags & ly.F_GRID), False,
                              bool(flags & ly.F_GRID_FIRST))


@functools.lru_cache(maxsize=None)
def discrete_reference(flags, H=0):
    """The same sequence with random priority-list ids of the layout's own lists (the reference's enumeration): ``populate_action`` +
    ``run(..., normalized=False)`` of the oracle."""
    from oracle import oracle as orc
    orc.build()
    lists = priority_lists(flags)
    assert len(lists) == {0: 1, 1: 2, 2: 1, 3: 4, 4: 1, 5: 4, 6: 2, 7: 12, 14: 2, 15: 12}[flags]
    og = ly.OracleSingles(orc, columns(flags, H))
    rs = np.random.RandomState(77 + flags)
    ids = rs.randint(0, len(lists), size=(STEPS + TAIL, N)).astype(np.int32)
    assert set(ids.ravel().tolist()) == set(range(len(lists))), (flags, "the ids reach every list of the layout")
    ref = dict(ids=ids, obs0=og.reset(T0))
    ctrl, recs, rows = [], [], []
    for k in range(STEPS + TAIL):
        if k == STEPS:
            ref["obs_end0"] = og.reset(T - TAIL)
        ctrl.append(og.expand([lists[i] for i in ids[k]]))
        recs.append(og.step(ctrl[-1], False))
        rows.append(og.observe())
    ref.update(control=np.stack(ctrl), rec=np.stack(recs), obs=np.stack(rows), state=og.state())
    done = ref["rec"]["done"].astype(bool)
    assert bool(done[-1].all()) and not bool(done[:-1].any()), flags
    if flags & ly.F_GENSET:
        assert {0, 1} <= set(ref["rec"]["gen_goal"].ravel().tolist()), flags
    return _frozen(ref)


def episode_starts(flags):
    """The first rows of the first episodes, drawn here so that the oracle half of their LENGTH steps replays without a GPU
    (tests/test_layouts.py); the restarts behind them are drawn on the device."""
    return np.random.RandomState(900 + flags).randint(0, T - LENGTH, size=N).astype(np.int32)


def episode_draws(flags, discrete, ctype="double"):
    """draw(k) of an episode case: ids of the layout's lists, or controls U[0, 1) with every seventh row rounded."""
    rs = np.random.RandomState(500 + 2 * flags + discrete)
    n_lists = len(priority_lists(flags))

    def draw(k):
        if discrete:
            return rs.randint(0, n_lists, size=N)
        a = rs.rand(N, action_dim(flags))
        return np.round(a) if k % 7 == 0 else a
    return draw


# ---- the GPU cases ---------------------------------------------------------------------------------------------------------------
def _tensor(a, device):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=device)


def _torch_dtype(ctype):
    import torch
    return torch.float32 if ctype == "float" else torch.float64


def _rounded(rows, ot):
    """The reference of a row: the oracle's float64 row, for float32 rows rounded to nearest (NOT the device's float64 row)."""
    return rows.astype(np.float32) if ot == "float" else rows


def _assert_state(cols, want, label):
    assert want or not any(k in cols for k in ("charge", "soc", "gen_status")), label
    for name, w in want.items():
        got = cols[name].cpu().numpy()
        assert np.array_equal(got.view(np.uint32) if name == "gen_status" else got, w), (label, name)


def _assert_step(ref, k, reward, done, obs, log, names, ot, label):
    rec = ref["rec"][k]
    assert np.array_equal(reward.cpu().numpy(), rec["reward"]), (label, k, "reward")
    assert np.array_equal(done.cpu().numpy().astype(np.int32), rec["done"]), (label, k, "done")
    if obs is not None:
        assert np.array_equal(obs.cpu().numpy(), _rounded(ref["obs"][k], ot)), (label, k, "rows")
    if log is not None:
        ly.assert_log_equals(log.cpu().numpy(), rec, names, (label, k))


class RowBuffer:
    """Where a case has its rows written: a fresh [N, D] tensor, or (``odd``) a view one element into a larger NaN-filled buffer --
    8-byte aligned float64 rows, 4-byte aligned float32 rows: the word-store branches -- outside of which nothing may change."""

    def __init__(self, engine, odd):
        import torch
        n = engine.N * engine.obs_dim
        self.flat = torch.full((n + 2,), float("nan"), dtype=engine.obs_dtype, device=engine.device) if odd else None
        self.rows = self.flat[1:n + 1].view(engine.N, engine.obs_dim) if odd else None
        assert not odd or self.rows.data_ptr() % (2 * self.rows.element_size()) == self.rows.element_size()

    def check(self, label):
        if self.flat is not None:
            edge = self.flat[[0, -1]].cpu().numpy()
            assert np.isnan(edge).all(), (label, "a store outside the rows")


@pytest.mark.gpu
@pytest.mark.parametrize("case", LOCKSTEP_CASES, ids=_id)
def test_lockstep_steps_and_rows_vs_oracle(case, device):
    """step_kernel<F, false> and observe_kernel<F> with whole H = 0 rows: mgx_reset and mgx_observe at row 3, six steps with rows and
    the log -- one mgx_step each, over two shards, or one mgx_step_many -- then the last three rows of the series."""
    import torch
    from pymgrid_amd import StepEngine
    flags, ot, at, series, odd, how = case
    ref = lockstep_reference(flags, 0, at)
    e = StepEngine(device_batch(flags, 0, series, device), obs_dtype=_torch_dtype(ot), action_dtype=_torch_dtype(at))
    try:
        names = e.log_names
        assert ly.flags_of(e.layout) == flags and e.obs_dim == ref["obs0"].shape[1] and e.batch.factorised == (series == "factorised")
        buf = RowBuffer(e, odd)
        acts = _tensor(ref["controls"], device)
        assert np.array_equal(e.reset(T0, out=buf.rows).cpu().numpy(), _rounded(ref["obs0"], ot)), (case, "reset rows")
        buf.check((case, "reset"))
        if odd:
            buf.rows.fill_(float("nan"))
        assert np.array_equal(e.observe(out=buf.rows).cpu().numpy(), _rounded(ref["obs0"], ot)), (case, "observe")
        buf.check((case, "observe"))
        if how == "many":
            obs, reward, done, log = e.step_many(acts[:STEPS], want_obs=True, want_log=True)
            for k in range(STEPS):
                _assert_step(ref, k, reward[k], done[k], obs[k], log[k], names, ot, case)
        else:
            if how == "shards":
                torch.cuda.synchronize()
                e.set_shards(2)
            for k in range(STEPS):
                if how == "shards":
                    e.fork()
                obs, reward, done, log = e.step(acts[k], want_obs=True, want_log=True, out=dict(obs=buf.rows))
                if how == "shards":
                    e.join()
                _assert_step(ref, k, reward, done, obs, log, names, ot, case)
                buf.check((case, k))
            if how == "shards":
                torch.cuda.synchronize()
                e.set_shards(1)
        assert np.array_equal(e.reset(T - TAIL, out=buf.rows).cpu().numpy(), _rounded(ref["obs_end0"], ot)), (case, "reset near the end")
        for k in range(STEPS, STEPS + TAIL):
            obs, reward, done, log = e.step(acts[k], want_obs=True, want_log=True, out=dict(obs=buf.rows))
            _assert_step(ref, k, reward, done, obs, log, names, ot, case)
            buf.check((case, k))
        assert e.current_step == T
        _assert_state(e.batch.cols, ref["state"], case)
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROWS_CASES, ids=_id)
def test_rows_with_a_horizon_vs_oracle(case, device):
    """obs_rows_wave_kernel<F, NOISE, OT> behind every reset and step.  The oracle forecaster, and the noisy one with every std 0:
    the oracle's rows.  With std > 0 (no host rule): the current-value and state columns are the oracle's, the forecasts lie in
    [0, 1], the rows are reproducible per seed and drawn again a step later."""
    from pymgrid_amd import StepEngine
    flags, H, ot, noise = case
    ref = lockstep_reference(flags, H, "double")
    e = StepEngine(device_batch(flags, H, "factorised" if H == HORIZONS[0] else "materialised", device, noise), obs_dtype=_torch_dtype(ot))
    try:
        assert e.layout.horizon == H and e.obs_dim == ref["obs0"].shape[1]
        forecast = np.array(["forecast" in name for name in e.layout.obs_names])
        assert forecast.sum() == H * (2 + 4 * bool(flags & ly.F_GRID)) and e.obs_dim - forecast.sum() == 2 + e.state_dim + 4 * bool(flags & ly.F_GRID)
        exact = ~forecast if noise else np.ones(e.obs_dim, dtype=bool)
        acts = _tensor(ref["controls"], device)

        def check(rows, want, label):
            rows = rows.cpu().numpy()
            assert np.array_equal(rows[:, exact], _rounded(want, ot)[:, exact]), (case, label)
            assert bool(((rows[:, forecast] >= 0) & (rows[:, forecast] <= 1)).all()), (case, label, "a forecast outside [0, 1]")
            return rows
        first = check(e.reset(T0), ref["obs0"], "reset rows")
        load = slice(1, 1 + H)              # the forecasts of the load window (the first block of a row): a load is never 0, so its
        if noise:                           # noisy forecast is clipped to 0 or 1 -- and then repeats itself -- on few draws only
            assert np.array_equal(e.observe().cpu().numpy(), first), (case, "the same seed, row and state: the same draws")
            assert (first[:, load] != _rounded(ref["obs0"], ot)[:, load]).mean() > 0.5, (case, "the forecasts carry noise")
        for k in range(STEPS + TAIL):
            if k == STEPS:
                check(e.reset(T - TAIL), ref["obs_end0"], "reset near the end")
            obs, reward, done, log = e.step(acts[k], want_obs=True, want_log=True)
            _assert_step(ref, k, reward, done, None, log, e.log_names, ot, case)
            rows = check(obs, ref["obs"][k], k)
            if noise and k == 0:
                # the forecast of series row T0 + 2 + j is column j + 1 of the first load window and column j of the next one:
                # a forecaster that drew once per series row would repeat itself here
                assert (first[:, load][:, 1:] != rows[:, load][:, :-1]).mean() > 0.5, (case, "drawn again a step later")
        _assert_state(e.batch.cols, ref["state"], case)
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", RING_CASES, ids=_id)
def test_prefetched_rings_vs_oracle(case, device):
    """obs_windows_k_kernel<F, OT> fills rings of four blocks, row-major or column-major; every step adds the state columns to its
    block (store_step_obs with obs_state_only == 1, its obs_colpitch form for the columns): the six steps cross a refill."""
    from pymgrid_amd import BatchedMicrogridEnv
    flags, H, ot, ring = case
    ref = lockstep_reference(flags, H, "double")
    env = BatchedMicrogridEnv(device_batch(flags, H, "factorised" if ring == "rows" else "materialised", device), log=True,
                              obs_dtype=_torch_dtype(ot), obs_prefetch=PREFETCH, obs_layout=ring)
    try:
        assert env.obs_prefetch == PREFETCH and env._ring is not None
        acts = _tensor(ref["controls"], device)
        assert np.array_equal(env.reset(T0).cpu().numpy(), _rounded(ref["obs0"], ot)), (case, "reset rows")
        for k in range(STEPS + TAIL):
            if k == STEPS:
                assert np.array_equal(env.reset(T - TAIL).cpu().numpy(), _rounded(ref["obs_end0"], ot)), (case, "reset near the end")
            obs, reward, done, info = env.step(acts[k])
            assert (obs.stride(0) == 1) == (ring == "columns"), (case, obs.stride())
            _assert_step(ref, k, reward, done, obs, info["log"], env.engine.log_names, ot, case)
        _assert_state(env.batch.cols, ref["state"], case)
    finally:
        env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", VIEW_CASES, ids=_id)
def test_observation_views_vs_oracle(case, device):
    """obs_views=True: normalise_series_kernel<1 | 4, OT> writes the normalised series once, a step the compact state columns
    (obs_state_only == 2); ``obs.flat()`` is the oracle's row."""
    from pymgrid_amd import BatchedMicrogridEnv
    flags, H, ot = case
    ref = lockstep_reference(flags, H, "double")
    env = BatchedMicrogridEnv(device_batch(flags, H, "materialised" if H == HORIZONS[0] else "factorised", device), log=True,
                              obs_dtype=_torch_dtype(ot), obs_views=True)
    try:
        acts = _tensor(ref["controls"], device)
        assert np.array_equal(env.reset(T0).flat().cpu().numpy(), _rounded(ref["obs0"], ot)), (case, "reset rows")
        for k in range(STEPS + TAIL):
            if k == STEPS:
                assert np.array_equal(env.reset(T - TAIL).flat().cpu().numpy(), _rounded(ref["obs_end0"], ot)), (case, "reset near the end")
            obs, reward, done, info = env.step(acts[k])
            _assert_step(ref, k, reward, done, obs.flat(), info["log"], env.engine.log_names, ot, case)
        _assert_state(env.batch.cols, ref["state"], case)
    finally:
        env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", DISCRETE_CASES, ids=_id)
def test_discrete_steps_vs_oracle(case, device):
    """mgx_expand_discrete alone (expand_kernel<F>) and the fused discrete step with the control row (step_discrete_kernel<F, false>)
    under random ids of the layout's own priority lists, against ``populate_action`` + ``run`` of the oracle.  Layout 0 has one, empty
    list and no control row: the fused step runs, the expansion alone is refused (REFUSED) and writes nothing."""
    import torch
    from pymgrid_amd import StepEngine, _lib
    from pymgrid_amd.priority_list import table_array
    (flags,) = case
    ref = discrete_reference(flags)
    table = table_array(priority_lists(flags))
    e = StepEngine(device_batch(flags, 0, SERIES[ly.LAYOUTS.index(flags) % 2], device))
    try:
        ids = _tensor(ref["ids"], device)
        assert np.array_equal(e.reset(T0).cpu().numpy(), ref["obs0"]), (case, "reset rows")
        for k in range(STEPS + TAIL):
            if k == STEPS:
                assert np.array_equal(e.reset(T - TAIL).cpu().numpy(), ref["obs_end0"]), (case, "reset near the end")
            if flags:
                control = torch.full((N, e.action_dim), float("nan"), dtype=torch.float64, device=device)
                assert np.array_equal(e.expand_discrete(ids[k], table, out=control).cpu().numpy(), ref["control"][k]), (case, k, "expansion")
            else:
                assert ("expand_kernel", (0,)) in REFUSED
                mask = torch.full((N,), 0x5a5a, dtype=torch.int32, device=device)
                with pytest.raises(_lib.MgxError, match="mgx_expand_discrete: NULL argument"):
                    e.expand_discrete(ids[k], table, violations=mask)
                assert bool((mask == 0x5a5a).all()) and e.current_step == (T0 if k < STEPS else T - TAIL) + k % STEPS
            control = torch.full((N, e.action_dim), float("nan"), dtype=torch.float64, device=device)
            obs, reward, done, log, control = e.step_discrete(ids[k], table, want_obs=True, want_log=True, want_control=True,
                                                              out=dict(control=control))
            assert np.array_equal(control.cpu().numpy(), ref["control"][k]), (case, k, "control")
            _assert_step(ref, k, reward, done, obs, log, e.log_names, "double", case)
        _assert_state(e.batch.cols, ref["state"], case)
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", EPISODE_CASES, ids=_id)
def test_inplace_episodes_vs_oracle(case, device, oracle):
    """step_kernel<F, true> / step_discrete_kernel<F, true>: PerGridWindowEnv(auto_reset=True, trajectory_length=5,
    final_observation=True), the finished grids restarted inside the step kernel -- replayed on the oracle with the rows every grid
    walked (layouts.episodes_vs_oracle), the rows of the finished episodes included; every grid restarts.  With a horizon the rows come
    from rings, into which patch_windows_kernel<GRID, OT> writes the window columns of the restarted grids."""
    from pymgrid_amd.hetero import PerGridWindowEnv
    flags, discrete, H, ot = case
    kw = dict(remove_redundant_gensets=False) if discrete else {}
    if H:
        kw.update(obs_prefetch=PREFETCH)
    batch = device_batch(flags, H, SERIES[(ly.LAYOUTS.index(flags) + discrete) % 2], device)
    env = PerGridWindowEnv(batch, trajectory_length=LENGTH, discrete=discrete, auto_reset=True, final_observation=True,
                           seed=3 + flags, obs_dtype=_torch_dtype(ot), **kw)
    try:
        assert env.native and env._device_draws and (env.env._ring is not None) == bool(H)
        og = ly.OracleSingles(oracle, columns(flags, H))
        restarts = ly.episodes_vs_oracle(oracle, env, og, EPISODE_STEPS, episode_draws(flags, discrete),
                                         first=(episode_starts(flags), None), label=case, final=True)
        assert bool((restarts == EPISODE_STEPS // LENGTH).all()), (case, "every grid restarts")
    finally:
        env.env.close()


# ---- fleets: five layouts share a launch (MGX_FLEET_MAX = 5), so two fleets hold the ten -----------------------------------------
FLEETS = (ly.LAYOUTS[:5], ly.LAYOUTS[5:])
# the kernel of a form; its run-time ``switch`` over the ten layouts (one for continuous, one for discrete items) is out of the
# compiled-symbol check's sight, so FLEET_CASES itself must name every (form, layout, discrete) triple (tests/test_layouts.py)
FLEET_KERNELS = {"value": ("fleet_step_kernel_v", (False,)),      # the buckets' arguments by value: the default
                 "pointer": ("fleet_step_kernel", ()),            # ... read from device copies (fleet_byvalue = 0), ring chunks riding along
                 "episodes": ("fleet_step_kernel_v", (True,))}    # in-place per-grid episodes (PerGridWindowFleet, fleet_episodes = 1)
FLEET_CASES = tuple((form, which, discrete) for form in FLEET_KERNELS for which in range(len(FLEETS)) for discrete in (False, True))


def fleet_triples(case):
    form, which, discrete = case
    return {(form, f, discrete) for f in FLEETS[which]}


class tuned:
    """A tunable of the library for the length of a ``with`` block; its default is back behind it."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        from pymgrid_amd import _lib
        self.default = _lib.get_tunable(self.name)[1]
        _lib.set_tunable(self.name, self.value)

    def __exit__(self, *exc):
        from pymgrid_amd import _lib
        _lib.set_tunable(self.name, self.default)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in FLEET_CASES if c[0] != "episodes"], ids=_id)
def test_lockstep_fleets_vs_oracle(case, device):
    """One mgx_fleet_step call per step for five layouts: fleet_step_kernel_v<false> (whole H = 0 rows), or with fleet_byvalue = 0
    the pointer form fleet_step_kernel, chunks of the next observation ring riding along (H = 3, rings of four blocks).  Every bucket
    against the oracle like a single env: reward, done, rows, every log column, the state at the end."""
    from pymgrid_amd.hetero import BucketedFleet
    form, which, discrete = case
    H = HORIZONS[0] if form == "pointer" else 0
    kw = dict(log=True, discrete=discrete, **(dict(remove_redundant_gensets=False) if discrete else {}))
    if form == "pointer":
        kw.update(refill="chunks", obs_prefetch=PREFETCH)
    refs = [discrete_reference(f, H) if discrete else lockstep_reference(f, H, "double") for f in FLEETS[which]]
    with tuned("fleet_byvalue", 0 if form == "pointer" else 1):
        fleet = BucketedFleet.from_batches([device_batch(f, H, SERIES[i % 2], device) for i, f in enumerate(FLEETS[which])], **kw)
        try:
            assert fleet.fused and [ly.flags_of(env.layout) for env in fleet.envs] == list(FLEETS[which])
            assert all((env._ring is not None) == (form == "pointer") for env in fleet.envs)
            for env, ref in zip(fleet.envs, refs):
                assert np.array_equal(env.reset(T0).cpu().numpy(), ref["obs0"]), (case, ly.flags_of(env.layout), "reset rows")
            for k in range(STEPS + TAIL):
                if k == STEPS:
                    for env, ref in zip(fleet.envs, refs):
                        assert np.array_equal(env.reset(T - TAIL).cpu().numpy(), ref["obs_end0"]), (case, ly.flags_of(env.layout))
                acts = [_tensor(ref["ids"][k] if discrete else ref["controls"][k], device) for ref in refs]
                obs, reward, done, info = fleet.step(acts)
                for b, (env, ref) in enumerate(zip(fleet.envs, refs)):
                    _assert_step(ref, k, reward[b], done[b], obs[b], info[b]["log"], env.engine.log_names, "double", (case, FLEETS[which][b]))
            for env, ref in zip(fleet.envs, refs):
                assert env.engine.current_step == T
                _assert_state(env.batch.cols, ref["state"], (case, ly.flags_of(env.layout)))
        finally:
            fleet.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in FLEET_CASES if c[0] == "episodes"], ids=_id)
def test_episode_fleets_vs_oracle(case, device, oracle):
    """fleet_step_kernel_v<true>: PerGridWindowFleet(auto_reset=True, trajectory_length=5, final_observation=True), the in-place
    episodes of five layouts in one launch; every bucket replayed on the oracle with the rows its grids walked."""
    from pymgrid_amd.hetero import PerGridWindowFleet
    form, which, discrete = case
    kw = dict(remove_redundant_gensets=False) if discrete else {}
    with tuned("fleet_episodes", 1):
        fleet = PerGridWindowFleet.from_batches([device_batch(f, 0, SERIES[(i + 1) % 2], device) for i, f in enumerate(FLEETS[which])],
                                                trajectory_length=LENGTH, discrete=discrete, auto_reset=True, final_observation=True,
                                                seed=11, **kw)
        try:
            assert all(fleet._in_call) and all(pe.native and pe._device_draws for pe in fleet.envs)
            replays = [ly.EpisodeReplay(pe, ly.OracleSingles(oracle, columns(f, 0)), (case, f), final=True)
                       for pe, f in zip(fleet.envs, FLEETS[which])]
            draws = [episode_draws(f, discrete) for f in FLEETS[which]]
            for replay, obs in zip(replays, fleet.reset(starts=[episode_starts(f) for f in FLEETS[which]])):
                replay.begin(obs)
            for k in range(EPISODE_STEPS):
                obs, reward, done, info = fleet.step([replay.oracle_step(draw(k)) for replay, draw in zip(replays, draws)])
                for b, replay in enumerate(replays):
                    replay.after(k, obs[b], reward[b], done[b], info[b])
            for replay in replays:
                assert bool((replay.finish() == EPISODE_STEPS // LENGTH).all()), (replay.label, "every grid restarts")
        finally:
            fleet.close()


# ---- the ring refill of the general path (several modules of a kind): obs_windows_k_multi_kernel<F, OT> --------------------------
MULTI_N, MULTI_T, MULTI_H = 141, 40, 3        # two workgroups of BLOCK_MULTI = 64 and a wave of 13; 8 full window groups and one of 13
MULTI_CASES = tuple((f, ot) for f in ly.LAYOUTS for ot in FLOATS)


def multi_counts(flags):
    """Two of every kind the layout has (layout 0: two loads and two pvs)."""
    return (2 * (flags & 1), (flags >> 1) & 1 and 2, (flags >> 2) & 1 and 2, 2, 2)


@functools.lru_cache(maxsize=None)
def multi_grids(flags):
    grids = ly.general_grids(flags, multi_counts(flags), MULTI_N, MULTI_T, SEED + flags, horizon=MULTI_H)
    assert ly.instances_differ(grids)
    return grids


@functools.lru_cache(maxsize=None)
def multi_reference(flags):
    """The launch sequence on ``layouts.OracleGrids``: rows behind every reset and step (``run(observe=True)``), rewards, done."""
    from oracle import oracle as orc
    orc.build()
    counts = multi_counts(flags)
    og = ly.OracleGrids(orc, multi_grids(flags))
    a = ly.general_controls(np.random.RandomState(300 + flags), STEPS + TAIL, MULTI_N, counts)
    ref = dict(controls=a, obs0=og.reset(T0))
    rec, obs = og.run(a[:STEPS], True, observe=True)
    ref["obs_end0"] = og.reset(MULTI_T - TAIL)
    rec_end, obs_end = og.run(a[STEPS:], True, observe=True)
    ref.update(rec=ly.common(np.concatenate([rec, rec_end])), obs=np.concatenate([obs, obs_end]), state=og.state())
    done = ref["rec"]["done"].astype(bool)
    assert bool(done[-1].all()) and not bool(done[:-1].any()), flags
    assert MULTI_T - TAIL + MULTI_H > MULTI_T - 1, "a window of the last rows runs into the padding behind the series"
    return _frozen(ref)


@pytest.mark.gpu
@pytest.mark.parametrize("case", MULTI_CASES, ids=_id)
def test_general_path_rings_vs_oracle(case, device):
    """The ring refill of the general path, two of every kind, H = 3, rings of four blocks: the rows of every reset and step against
    ``OracleGrids.run(observe=True)``, with rewards, done flags and the final state."""
    from pymgrid_amd import BatchedMicrogridEnv, MicrogridBatch
    flags, ot = case
    ref = multi_reference(flags)
    env = BatchedMicrogridEnv(MicrogridBatch.from_grids(multi_grids(flags), device=device), obs_dtype=_torch_dtype(ot),
                              obs_prefetch=PREFETCH)
    try:
        assert env.layout.multi and ly.flags_of(env.layout) == flags and env.obs_prefetch == PREFETCH and env._ring is not None
        acts = _tensor(ref["controls"], device)
        assert np.array_equal(env.reset(T0).cpu().numpy(), _rounded(ref["obs0"], ot)), (case, "reset rows")
        for k in range(STEPS + TAIL):
            if k == STEPS:
                assert np.array_equal(env.reset(MULTI_T - TAIL).cpu().numpy(), _rounded(ref["obs_end0"], ot)), (case, "reset near the end")
            obs, reward, done, _ = env.step(acts[k])
            _assert_step(ref, k, reward, done, obs, None, None, ot, case)
        for name, w in ref["state"].items():
            got = env.batch.cols[name].cpu().numpy().reshape(w.shape)
            assert np.array_equal(got.view(np.uint32) if name == "gen_status" else got, w), (case, name)
    finally:
        env.close()



@pytest.mark.gpu
@pytest.mark.parametrize("case", DRY_RUN_CASES, ids=_id)
def test_the_dry_run_vs_the_recorded_reference(case, device):
    """check_kernel<F>, check_discrete_kernel<F> and action_bounds_kernel<F> against what the real reference did
    (tests/golden/raise_errors.npz): before every one of the 24 steps, bit 0 / 1 / 2 of ``check_step`` is "the genset / battery / grid
    module raised ValueError with raise_errors=True" on every grid -- requests exactly at the instantaneous limit, one ulp beyond it,
    uniform, normalised -- and where the golden has an AssertionError the V_ASSERTS bits are set; ``check_discrete`` gives the same for
    the priority list the reference expanded at that moment; without a genset ``action_bounds()`` is the recorded interval, bit for
    bit, with one the env refuses to ask (REFUSED); the state after the last step is the golden's."""
    import torch
    from pymgrid_amd import BatchedMicrogridEnv, MicrogridBatch, StepEngine, _lib
    flags, raw = case
    g = raise_errors_golden(flags)
    tile = np.tile(np.flatnonzero(g["raw"] == raw), GOLDEN_TILES)
    batch = MicrogridBatch.from_grids([g["grids"][j] for j in tile], device=device)
    assert ly.flags_of(batch.layout) == flags and not batch.layout.multi and len(tile) == 336
    if raw and flags & ly.F_GENSET:
        assert ("action_bounds_kernel", (flags,)) in REFUSED
        env = BatchedMicrogridEnv(batch)
        with pytest.raises(TypeError, match="strict_bound"):
            env.sample_action(strict_bound=True)
        env.close()
    e = StepEngine(batch)
    try:
        e.reset(0, want_obs=False)
        if not flags:
            assert ("action_bounds_kernel", (0,)) in REFUSED
            with pytest.raises(_lib.MgxError, match="mgx_action_bounds: NULL argument"):
                e.action_bounds()
        present = [q for q in range(3) if flags & (1 << q)]
        for k in range(g["requests"].shape[0]):
            a = _tensor(g["requests"][k][tile], device)
            for what, mask, exc in (("check_step", e.check_step(a, normalized=not raw), g["exception"][k][tile]),
                                    ("check_discrete", e.check_discrete(_tensor(g["ids"][k][tile], device), g["table"]),
                                     g["list_exception"][k][tile])):
                mask = mask.cpu().numpy()
                for q in range(3):
                    assert np.array_equal((mask >> q) & 1, exc[:, q] == GOLDEN_VALUE_ERROR), (case, k, what, ("genset", "battery", "grid")[q])
                asserted = (exc == GOLDEN_ASSERTION_ERROR).any(axis=1)
                assert bool(((mask & _lib.V_ASSERTS) != 0)[asserted].all()), (case, k, what, "an AssertionError of the reference")
                assert flags or not mask.any(), (case, k, what)
            if not flags & ly.F_GENSET and flags:
                lo, hi = (t.cpu().numpy() for t in e.action_bounds())
                for c, q in enumerate(present):                    # the action columns: battery, grid
                    want = g["bounds"][k][tile][:, q - 1]
                    assert np.array_equal(lo[:, c], want[:, 0]) and np.array_equal(hi[:, c], want[:, 1]), (case, k, "bounds", q)
            e.step(a, normalized=not raw, want_obs=False)
        want = {}
        if flags & ly.F_BATTERY:
            want.update(charge=g["charge"][tile], soc=g["soc"][tile])
        if flags & ly.F_GENSET:
            want["gen_status"] = ly.status_words(*g["status"][tile].T)
        _assert_state(e.batch.cols, want, case)
    finally:
        e.close()
