"""The general path (microgrids with several modules of a kind) against the multi-instance CPU oracle, one case per compiled form:
step_multi_kernel<F, EP>, step_k_multi_kernel<F>, step_k_multi_small_kernel<F, CNT, M>, rollout_multi_small_kernel<F, CNT, M>,
step_lists_small_kernel<F, EP>, expand_multi_kernel<F>, check_multi_kernel<F> and observe_multi_kernel<F>.  Every comparison is
with ``oracle.OracleMultiMicrogrid``, bit for bit; none is between two device forms.  The batches come from parameter dicts
(layouts.general_grids: every instance its own parameters and series, a stressed population that fills the ``provided`` list to eight
and nine addends, where its sum takes numpy's pairwise order), and the conditions the inputs must meet -- no grid left out, the
shares of eight and nine addends, genset status words, restarts -- are asserted on the reference side of every case.
tests/test_layouts.py checks, without a GPU, that CASES and REFUSED below name every instantiation the library holds."""
import functools

import numpy as np
import pytest

import layouts as ly

# MGX_STATIC_LAYOUTS of pymgrid_amd/csrc/mgx_fused.hip (part 5), transcribed: (F, n_genset, n_battery, n_grid, n_load, n_pv) of the
# mixes with a compile-time-count form of the two fused kernels (CountsCT<...>)
STATIC_LAYOUTS = (
    (7, 2, 2, 1, 1, 1), (7, 2, 2, 2, 1, 1), (7, 2, 2, 2, 2, 2), (7, 1, 2, 1, 1, 1), (7, 1, 2, 2, 1, 1), (7, 2, 1, 1, 1, 1), (7, 1, 1, 2, 1, 1),
    (3, 2, 2, 0, 1, 1), (3, 2, 1, 0, 1, 1), (3, 1, 2, 0, 1, 1), (6, 0, 2, 1, 1, 1), (6, 0, 2, 2, 1, 1), (6, 0, 1, 2, 1, 1),
    (7, 3, 3, 1, 1, 1), (7, 3, 2, 1, 1, 1), (7, 2, 3, 1, 1, 1), (3, 3, 3, 0, 1, 1), (6, 0, 3, 1, 1, 1))
# two of every kind the layout has (layout 0: two loads and two pvs; 14 and 15 step the grids before the batteries)
TWO_OF_EVERYTHING = tuple((f, (2 * (f & 1), (f >> 1) & 1 and 2, (f >> 2) & 1 and 2, 2, 2)) for f in ly.LAYOUTS)
# unequal counts: the run-time-count register form re-reads "the last instance a layout has" for the ones it lacks
UNEQUAL = ((7, (2, 1, 2, 1, 2)), (15, (1, 2, 2, 1, 1)), (6, (0, 2, 1, 1, 2)))
# three of a kind without a compile-time-count form (static forms exclude the grid-first layouts): the run-time-count kernel with
# its LDS lists; the first carries the mirrored population, which brings the ``absorbed`` list to eight addends
MIRRORED = (7, (3, 3, 3, 1, 1))
THREE_OF_A_KIND = (MIRRORED, (15, (2, 3, 1, 1, 1)))
MIXES = tuple(dict.fromkeys(tuple((s[0], s[1:]) for s in STATIC_LAYOUTS) + TWO_OF_EVERYTHING + UNEQUAL + THREE_OF_A_KIND))

# the forms of a case, selected with the library's tunables (set before the engine is created: mgx_create decides h->multi_small)
TUNABLES = {"static": {},                                        # compile-time counts (multi_static = 1, the default)
            "runtime": {"multi_static": 0},                      # run-time counts in registers
            "generic": {"multi_static": 0, "multi_generic": 1},  # step_multi_core: the walk over the batch's columns
            "shared": {"multi_small_own": 0}}                    # step_k_multi_kernel, and mgx_step_lists in two launches
DEFAULTS = {"multi_static": 1, "multi_generic": 0, "multi_small_own": 1}


def is_small(counts):
    """multi_is_small of csrc/mgx_core.hpp: at most MS = 2 modules of every kind, a load and a pv among them."""
    ng, nb, nr, nl, npv = counts
    return 1 <= nl <= 2 and 1 <= npv <= 2 and max(ng, nb, nr) <= 2


def forms_of(flags, counts):
    """The forms that exist for a mix, i.e. select kernels of their own."""
    static = (flags, *counts) in STATIC_LAYOUTS
    return (("static",) if static else ()) + (("runtime",) if is_small(counts) else ()) + ("generic",) \
        + (("shared",) if is_small(counts) else ())


CASES = tuple((flags, counts, form) for flags, counts in MIXES for form in forms_of(flags, counts))
# one case per form family runs its fused continuous launches over two shards
SHARDED = {(7, (2, 2, 2, 2, 2), "static"), (7, (2, 2, 2, 2, 2), "runtime"), (7, (2, 2, 2, 2, 2), "shared"), MIRRORED + ("generic",)}


def lists_in_episodes(flags, counts):
    """Whether the discrete per-grid-episode env is run on a mix: the reference enumerates its priority lists over every permutation
    of the elements (two per genset, one per battery and grid), which is offered up to 8 of them here (40 320 permutations) -- the
    mixes of the register form (at most two of a kind) -- and a layout without a controllable module has no list to expand."""
    ng, nb, nr = counts[:3]
    return flags != 0 and 2 * ng + nb + nr <= 8


def compiled_forms(flags, counts, form):
    """{(kernel, compile-time part)} the calls of a case launch: the dispatch of csrc/mgx_abi.hip (mgx_step, mgx_check_step,
    mgx_observe, mgx_step_k, mgx_rollout_lists, mgx_step_lists, mgx_expand_lists), stated once.  tests/test_layouts.py holds this
    against the instantiations the library has."""
    small = is_small(counts) and form != "generic"               # h->multi_small
    own = form != "shared"                                       # the tunable multi_small_own
    cnt = counts if form == "static" else "RT"
    out = {("step_multi_kernel", (flags, False)), ("step_multi_kernel", (flags, True)), ("observe_multi_kernel", (flags,)),
           ("check_multi_kernel", (flags,))}
    if form == "static" or (small and own):                      # mgx_step_k and mgx_rollout_lists: the register loops
        out |= {("step_k_multi_small_kernel", (flags, cnt)), ("rollout_multi_small_kernel", (flags, cnt))}
    else:                                                        # ... or the loop around step_multi_core, for both
        out.add(("step_k_multi_kernel", (flags,)))
    if small and own:                                            # mgx_step_lists: one launch, lock-step ...
        out.add(("step_lists_small_kernel", (flags, False)))
        if lists_in_episodes(flags, counts) or flags == 0:       # ... and in per-grid episodes: the discrete env, or on the layout
            out.add(("step_lists_small_kernel", (flags, True)))   # without a control the engine itself (the last test below)
    elif flags != 0:                                             # or expansion into the control buffer, then the step
        out.add(("expand_multi_kernel", (flags,)))
    return out


# compiled, but out of every call's reach: a layout without a controllable module has an empty control row [N, 0], whose device
# pointer is NULL, so no call can hand the expansion a control buffer to write (mgx_expand_lists, mgx_expand_discrete and the
# two-launch mgx_step_lists return MGX_ERR_INVALID: asserted in the list and episode tests below)
REFUSED = (("expand_multi_kernel", (0,)),)

pytestmark = pytest.mark.gpu
N, T, T0, SEED, H = 200, 40, 3, 5, 2          # three workgroups of BLOCK_MULTI = 64 and a partial wave of 8
SINGLE = 4                                   # env.step calls, then the fused launches (K, controls, normalised) from the carried state:
LAUNCHES = ((1, "double", True),             # the pipeline has no next fetch
            (2, "double", True),
            (9, "float", True),              # float32 controls: the oracle takes them widened
            (3, "double", False),            # raw controls
            (T - T0 - SINGLE - 15, "double", True))   # to the last row of the series: the fetch clamp, and the last step reports done
FLOOR = 0.01                                 # share of the (step, grid) pairs of the fused launches with 8 / with 9 addends


def _mirrored(flags, counts):
    return (flags, counts) == MIRRORED


@functools.lru_cache(maxsize=None)
def grids_of(flags, counts, horizon=H):
    grids = ly.general_grids(flags, counts, N, T, SEED, horizon=horizon, mirrored=_mirrored(flags, counts))
    assert ly.instances_differ(grids), "two instances of a kind share their parameters"
    return grids


def _soc_trace(og, rec):
    """The SoC trace [K, N] of a launch the oracle just ran (records ``rec``): the first battery's SoC AFTER every step -- what step
    k + 1 logs as ``soc_pre``, and behind the last step the oracle's state itself.  None without a battery."""
    if "soc" not in og.state():
        return None
    return np.concatenate([rec["battery"][..., 0]["soc_pre"][1:], og.state()["soc"][:1]])


@functools.lru_cache(maxsize=None)
def reference(flags, counts):
    """What the oracle makes of the single steps and the fused launches of a mix (the same for every form): the controls, MStepOut
    records, observation rows, addend counts and the final state -- with the conditions on the inputs asserted."""
    from oracle import oracle as orc
    orc.build()
    grids, mirrored = grids_of(flags, counts), _mirrored(flags, counts)
    rs = np.random.RandomState(100 * flags + sum(counts))
    og = ly.OracleGrids(orc, grids)
    ref = {"obs0": og.reset(T0)}
    a = ly.general_controls(rs, SINGLE, N, counts, mirrored)
    rec, obs = og.run(a, True, observe=True)
    ref["single"] = dict(controls=a, rec=rec, obs=obs)
    ref["launches"], prov, absb = [], [], []
    for K, ctype, normalized in LAUNCHES:
        a = ly.general_controls(rs, K, N, counts, mirrored)
        if ctype == "float":
            a = a.astype(np.float32)
        if not normalized:
            a = ly.raw_controls(a, counts)
        wide = a.astype(np.float64)
        rec = og.run(wide, normalized)
        p, q = ly.addend_counts(grids, rec, wide, normalized)
        prov.append(p); absb.append(q)
        ref["launches"].append(dict(controls=a, rec=rec, normalized=normalized, soc=_soc_trace(og, rec)))
    assert og.oms[0].s.t == T and bool(ref["launches"][-1]["rec"]["common"]["done"][-1].all())     # the series is used up
    ref["state"] = og.state()
    prov, absb = np.concatenate(prov), np.concatenate(absb)
    ng, nb, nr, nl, npv = counts
    ref["shares"] = {8: float((prov == 8).mean()), 9: float((prov == 9).mean()), "absorbed": float((absb >= 8).mean())}
    for n in (8, 9):
        if ng + nb + nr + npv + 1 >= n:                           # the list can hold n addends
            assert ref["shares"][n] >= FLOOR, (flags, counts, n, ref["shares"])
    if mirrored:
        assert ref["shares"]["absorbed"] >= FLOOR, (flags, counts, ref["shares"])
    if ng:
        recs = np.concatenate([ln["rec"] for ln in ref["launches"]])["genset"][..., :ng]
        words = ly.status_words(recs["gen_cur"], recs["gen_goal"], recs["gen_up"], recs["gen_down"])
        assert len(np.unique(words)) > 2, (flags, counts, np.unique(words))
    return ref


def _tensor(a, device):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=device)


class tuned:
    """The tunables of a form for the length of a ``with`` block; the defaults are back behind it."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        from pymgrid_amd import _lib
        for name, v in {**DEFAULTS, **TUNABLES[self.form]}.items():
            _lib.set_tunable(name, v)

    def __exit__(self, *exc):
        from pymgrid_amd import _lib
        for name, v in DEFAULTS.items():
            _lib.set_tunable(name, v)


def _assert_state(cols, want, label):
    for name, w in want.items():
        got = cols[name].cpu().numpy().reshape(w.shape)
        assert np.array_equal(got.view(np.uint32) if name == "gen_status" else got, w), (label, name)


def _case_id(case):
    flags, counts, form = case
    return f"{flags}-{''.join(map(str, counts))}-{form}"


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_steps_and_fused_launches_vs_oracle(case, device, oracle):
    """Reset to row 3; four env steps with the dry-run mask before each (step_multi_kernel<F>, check_multi_kernel<F>,
    observe_multi_kernel<F>): reward, done, observation rows, every log column, the mask == the log's violations column; then the
    fused launches of LAUNCHES from the carried state (K = 1, 2, 9 with float32 controls, raw controls, to the last row), every one
    with reward, done, both traces and the log; at the end the state of every module instance."""
    import torch
    from pymgrid_amd import BatchedMicrogridEnv, MicrogridBatch
    flags, counts, form = case
    ng, nb = counts[:2]
    ref = reference(flags, counts)
    with tuned(form):
        env = BatchedMicrogridEnv(MicrogridBatch.from_grids(grids_of(flags, counts), device=device), log=True)
        try:
            e, names = env.engine, env.engine.log_names
            assert ly.flags_of(env.layout) == flags and env.layout.multi
            assert np.array_equal(env.reset(T0).cpu().numpy(), ref["obs0"]), (case, "reset rows")
            single, refusing = ref["single"], 0
            for k in range(SINGLE):
                act = _tensor(single["controls"][k], device)
                mask = e.check_step(act).cpu().numpy()
                obs, reward, done, info = env.step(act)
                rec, log = single["rec"][k], info["log"].cpu().numpy()
                assert np.array_equal(reward.cpu().numpy(), rec["common"]["reward"]), (case, k)
                assert np.array_equal(done.cpu().numpy().astype(np.int32), rec["common"]["done"]), (case, k)
                assert np.array_equal(obs.cpu().numpy(), single["obs"][k]), (case, k, "rows")
                ly.assert_log_equals(log, rec, names, (case, k))
                assert np.array_equal(mask, log[names.index("violations")].astype(mask.dtype)), (case, k, "mask")
                refusing += int((mask != 0).sum())
            # a condition on the inputs: the dry run has something to say (U[0, 1) requests pass what a genset that is off, an empty
            # battery or a grid in an outage can give), so the masks above are not compared on zeros alone
            assert refusing > 0 or flags == 0, (case, "no request of the four steps would be refused")
            if case in SHARDED:
                torch.cuda.synchronize()
                e.set_shards(2)
            for n, ln in enumerate(ref["launches"]):
                acts = _tensor(ln["controls"], device)
                e.set_action_dtype(acts.dtype)
                out = e.step_k(acts, normalized=ln["normalized"], reward=True, done=True, soc_trace=True, status_trace=True, log=True)
                if case in SHARDED:
                    e.join()
                rec = ln["rec"]
                assert np.array_equal(out["reward"].cpu().numpy(), rec["common"]["reward"]), (case, n)
                assert np.array_equal(out["done"].cpu().numpy().astype(np.int32), rec["common"]["done"]), (case, n)
                ly.assert_log_equals(out["log"].cpu().numpy(), rec, names, (case, n))
                if ng:                                            # the traces follow the first instance, after the step
                    g = rec["genset"][..., 0]
                    want = ly.status_words(g["gen_cur"], g["gen_goal"], g["gen_up"], g["gen_down"])
                    assert np.array_equal(out["status_trace"].cpu().numpy().view(np.uint32), want), (case, n, "status trace")
                if nb:                                            # every row, the last one (K = 1: the only one) included
                    assert np.array_equal(out["soc_trace"].cpu().numpy(), ln["soc"]), (case, n, "soc trace")
            if case in SHARDED:
                e.set_shards(1)
            assert e.current_step == T
            _assert_state(env.batch.cols, ref["state"], case)
        finally:
            env.close()


@functools.lru_cache(maxsize=None)
def lists_reference(flags, counts):
    """The priority lists, ids and the oracle's replay (populate_action + run(..., False)) of the list launches of a mix: a roll-out
    with an id per step and grid, one with a fixed list per grid, single steps."""
    from oracle import oracle as orc
    from pymgrid_amd.priority_list import get_instance_priority_lists, lists_array
    orc.build()
    grids = grids_of(flags, counts)
    ng, nb, nr = counts[:3]
    rs = np.random.RandomState(7 + 100 * flags + sum(counts))
    table = ly.drawn_lists(rs, counts) if ng + nb + nr else -np.ones((3, 2, 3), dtype=np.int32)
    if 0 < 2 * ng + nb + nr <= 6:                                 # the reference's own enumeration where it is not factorial
        own = lists_array(get_instance_priority_lists(ng, nb, nr, (), bool(flags & ly.F_GRID_FIRST)))
        wide = -np.ones((own.shape[0], table.shape[1], 3), dtype=np.int32)
        wide[:, :own.shape[1]] = own
        table = np.concatenate([table, wide])
    plists = ly.own_elements(table, counts)
    n = table.shape[0]
    og = ly.OracleGrids(orc, grids)
    og.reset(T0)
    ref = {"table": table, "launches": []}

    def step(ids):
        ctrl = og.expand([plists[i if 0 <= i < n else 0] for i in ids])      # (ids outside the table: list 0)
        return ctrl, og.step(ctrl, False)
    for K, per_step in ((10, True), (8, False)):
        ids = rs.randint(-1, n + 1, size=(K, N)) if per_step else rs.randint(0, n, size=N)
        done = [step(ids[k] if per_step else ids) for k in range(K)]
        ctrl, rec = np.stack([c for c, _ in done]), np.stack([r for _, r in done])
        ref["launches"].append(dict(ids=ids.astype(np.int32), K=K, rec=rec, counts=ly.addend_counts(grids, rec, ctrl, False),
                                    soc=_soc_trace(og, rec)))
    # a list asks every module for what the ones before it leave over, zero included, so its requests are sources while load is left:
    # the roll-outs fill the ``provided`` list at least as often as the stressed continuous controls do
    prov = np.concatenate([ln["counts"][0] for ln in ref["launches"]])
    ref["shares"] = {8: float((prov == 8).mean()), 9: float((prov == 9).mean())}
    for n_addends in (8, 9):
        if ng + nb + nr + counts[4] + 1 >= n_addends:
            assert ref["shares"][n_addends] >= FLOOR, (flags, counts, n_addends, ref["shares"])
    ref["steps"] = []
    for k in range(SINGLE):
        ids = rs.randint(-1, n + 1, size=N)
        ctrl, rec = step(ids)
        ref["steps"].append(dict(ids=ids.astype(np.int32), control=ctrl, rec=rec, obs=og.observe()))
    ref["state"] = og.state()
    return ref


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_list_launches_vs_oracle(case, device, oracle):
    """On a fresh engine: mgx_rollout_lists with an id per step and grid and with one fixed list per grid (rollout_multi_small_kernel,
    or step_k_multi_kernel's list arm), then mgx_step_lists single steps with the control buffer (step_lists_small_kernel<F>, or
    expand_multi_kernel<F> + step_multi_kernel<F>) -- against populate_action + run(..., False) of the oracle: rewards, done, traces,
    every log column, the expanded controls, observation rows and the final state."""
    import torch
    from pymgrid_amd import MicrogridBatch, StepEngine
    flags, counts, form = case
    ng, nb = counts[:2]
    ref = lists_reference(flags, counts)
    with tuned(form):
        e = StepEngine(MicrogridBatch.from_grids(grids_of(flags, counts), device=device))
        try:
            names = e.log_names
            lists = _tensor(ref["table"], device)
            e.reset(T0, want_obs=False)
            for n, ln in enumerate(ref["launches"]):
                out = e.rollout_lists(_tensor(ln["ids"], device), lists, ln["K"], reward=True, done=True, soc_trace=True,
                                      status_trace=True, log=True)
                rec = ln["rec"]
                assert np.array_equal(out["reward"].cpu().numpy(), rec["common"]["reward"]), (case, n)
                assert np.array_equal(out["done"].cpu().numpy().astype(np.int32), rec["common"]["done"]), (case, n)
                ly.assert_log_equals(out["log"].cpu().numpy(), rec, names, (case, n))
                if ng:
                    g = rec["genset"][..., 0]
                    want = ly.status_words(g["gen_cur"], g["gen_goal"], g["gen_up"], g["gen_down"])
                    assert np.array_equal(out["status_trace"].cpu().numpy().view(np.uint32), want), (case, n, "status trace")
                if nb:
                    assert np.array_equal(out["soc_trace"].cpu().numpy(), ln["soc"]), (case, n, "soc trace")
            if flags == 0 and form != "runtime":                  # REFUSED (expand_multi_kernel<0>): no buffer to expand into
                from pymgrid_amd import _lib
                with pytest.raises(_lib.MgxError, match="needs the control buffer"):
                    e.step_lists(_tensor(ref["steps"][0]["ids"], device), lists)
                with pytest.raises(_lib.MgxError, match="mgx_expand_lists: NULL argument"):
                    e.expand_lists(_tensor(ref["steps"][0]["ids"], device), lists)
                return
            for k, st in enumerate(ref["steps"]):
                control = torch.full((N, e.action_dim), np.nan, dtype=torch.float64, device=device)
                obs, reward, done, log = e.step_lists(_tensor(st["ids"], device), lists, want_obs=True, want_log=True,
                                                      out=dict(control=control))
                assert np.array_equal(control.cpu().numpy(), st["control"]), (case, k, "control")
                assert np.array_equal(reward.cpu().numpy(), st["rec"]["common"]["reward"]), (case, k)
                assert np.array_equal(done.cpu().numpy().astype(np.int32), st["rec"]["common"]["done"]), (case, k)
                assert np.array_equal(obs.cpu().numpy(), st["obs"]), (case, k, "rows")
                ly.assert_log_equals(log.cpu().numpy(), st["rec"], names, (case, k))
            _assert_state(e.batch.cols, ref["state"], case)
        finally:
            e.close()


# (case, discrete): the discrete env where it enumerates its lists -- and on the layout without a controllable module, where it is
# refused (the engine's own in-episode list step on that layout is the last test of the file)
EPISODE_CASES = tuple((case, discrete) for case in CASES for discrete in (False, True)
                      if not discrete or lists_in_episodes(*case[:2]) or case[0] == 0)


@pytest.mark.parametrize("case,discrete", EPISODE_CASES, ids=lambda v: _case_id(v) if isinstance(v, tuple) else ("continuous", "discrete")[v])
def test_per_grid_episodes_vs_oracle(case, discrete, device, oracle):
    """The EP forms: PerGridWindowEnv(auto_reset=True), episodes of 9 steps restarted in the kernel, 30 steps -- continuous
    (step_multi_kernel<F, true>) and discrete (step_lists_small_kernel<F, true> in one launch, or the expansion and
    step_multi_kernel<F, true>) -- replayed on the oracle with the rows every grid walked (layouts.episodes_vs_oracle); every grid
    restarts at least once."""
    from pymgrid_amd import MicrogridBatch
    from pymgrid_amd.hetero import PerGridWindowEnv
    flags, counts, form = case
    grids = grids_of(flags, counts, 1)
    rs = np.random.RandomState(11 + 100 * flags + sum(counts))
    with tuned(form):
        batch = MicrogridBatch.from_grids(grids, device=device)
        if discrete and flags == 0:       # REFUSED (expand_multi_kernel<0>): the env's one, empty list has no control row to expand into
            from pymgrid_amd import _lib
            env = PerGridWindowEnv(batch, trajectory_length=9, discrete=True, auto_reset=True, seed=3, remove_redundant_gensets=False)
            try:
                env.reset()
                with pytest.raises(_lib.MgxError, match="mgx_expand_discrete: NULL argument"):
                    env.step(_tensor(np.zeros(N, dtype=np.int32), device))
            finally:
                env.env.close()
            return
        kw = dict(remove_redundant_gensets=False) if discrete else {}
        env = PerGridWindowEnv(batch, trajectory_length=9, discrete=discrete, auto_reset=True, seed=3 + flags, **kw)
        try:
            assert env.native and env._device_draws
            if discrete:
                draw = lambda k: rs.randint(0, env.action_space.n, size=N)                         # noqa: E731
            else:
                draw = lambda k: ly.general_controls(rs, 1, N, counts, _mirrored(flags, counts))[0]  # noqa: E731
            restarts = ly.episodes_vs_oracle(oracle, env, grids, 30, draw, label=case)
            assert bool((restarts >= 1).all()), (case, int((restarts == 0).sum()))
        finally:
            env.env.close()


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == 0 and ("step_lists_small_kernel", (0, True)) in compiled_forms(*c)], ids=_case_id)
def test_list_steps_in_episodes_on_the_layout_without_a_control(case, device, oracle):
    """step_lists_small_kernel<0, true>: the discrete env cannot step this layout (its one, empty list would be expanded through
    mgx_expand_discrete: the test above), the engine can -- in-place episodes of 9 steps with device draws (reset_episodes,
    set_auto_reset), 30 mgx_step_lists steps over padding-only lists, which need no control buffer.  Replayed on the oracle (a run
    without controls) with the rows the engine reports: rewards, done flags, observation rows, every log column, every grid restarted."""
    import torch
    from pymgrid_amd import MicrogridBatch, StepEngine
    flags, counts, form = case
    grids, length, K = grids_of(flags, counts, 1), 9, 30
    rs = np.random.RandomState(13)
    with tuned(form):
        e = StepEngine(MicrogridBatch.from_grids(grids, device=device))
        try:
            assert e.action_dim == 0
            og = ly.OracleGrids(oracle, grids)
            starts = rs.randint(0, T - length, size=N).astype(np.int32)
            lengths = torch.full((N,), length, dtype=torch.int32, device=device)
            obs = e.reset_episodes(_tensor(starts, device), None, max_length=length)
            e.set_auto_reset(True, 17, length, lengths_out=lengths)
            assert np.array_equal(obs.cpu().numpy(), og.reset(starts)), (case, "first rows")
            lists = -torch.ones((3, 2, 3), dtype=torch.int32, device=device)
            rows, left, restarts = starts.astype(np.int64), np.full(N, length), np.zeros(N, dtype=np.int64)
            control = np.zeros((N, 0))
            for k in range(K):
                ids = _tensor(rs.randint(-1, 4, size=N).astype(np.int32), device)
                obs, reward, done, log = e.step_lists(ids, lists, want_obs=True, want_log=True)
                rec = og.step(control, False)
                done = done.cpu().numpy().astype(bool)
                assert np.array_equal(reward.cpu().numpy(), rec["common"]["reward"]), (case, k)
                ly.assert_log_equals(log.cpu().numpy(), rec, e.log_names, (case, k))
                left = left - 1
                assert np.array_equal(done, left == 0), (case, k)
                after = (e._window_start + (e.current_step - e._window_t0)).cpu().numpy()
                assert np.array_equal(after[~done], rows[~done] + 1), (case, k)
                assert bool((after[done] >= 0).all()) and bool((after[done] <= T - length).all()), (case, k)
                assert np.array_equal(lengths.cpu().numpy(), np.full(N, length)), (case, k)
                rows, left = after, np.where(done, length, left)
                restarts += done
                og.set_rows(rows, only=done)
                assert np.array_equal(og.rows(), rows), (case, k)
                assert np.array_equal(obs.cpu().numpy(), og.observe()), (case, k, "rows")
            assert bool((restarts >= 1).all()), (case, int((restarts == 0).sum()))
        finally:
            e.close()
