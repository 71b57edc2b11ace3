"""The inputs of the layout matrices (tests/test_layout_matrix.py, tests/test_layout_matrix_episodes.py,
tests/test_layout_matrix_policy.py, tests/test_layout_matrix_whatif.py), checked without a GPU:
layouts.carve gives every one of the ten layouts the fused kernels are compiled for, in both series forms, the CPU oracle replays
each of them without leaving a grid out, the inputs tell the grid-first layouts from the battery-first ones and reach both genset
forms of the loops -- and every instantiation of the thirty-seven kernel families of ``enumerated()`` that the library holds (the
open-loop fused kernels, the closed-loop policy kernels, the what-if kernels, the policy gradient, the hot K-step, the eight
families of the general path, tests/test_general_path_matrix.py, and the fourteen of the single-step path,
tests/test_single_step_matrix.py, whose inputs are checked at the end of this file) is a case of those matrices, or one of the forms
a matrix file names as refused with the refusal asserted.  The inputs of the general-path matrix are checked here too: their
``provided`` lists reach the eight and nine addends from which the sum takes numpy's pairwise order, and they tell the two stepping orders apart."""
import functools
import re

import numpy as np
import pytest
import torch

from layouts import LAYOUTS, carve, flags_of

N, T, SEED, K, T0 = 600, 300, 9, 140, 3
SERIES = ("materialised", "factorised")


@functools.lru_cache(maxsize=None)
def _full(series, mixed):
    from pymgrid_amd.generator import generate
    return generate(N, n_steps=T, seed=SEED, arch="genset+battery+grid", device="cpu", mixed_timers=mixed, series=series)


def _state(cols):
    return {k: cols[k].copy() for k in ("charge", "soc", "gen_status") if k in cols}


@functools.lru_cache(maxsize=None)
def _replay(flags, series, mixed):
    """(rewards of the continuous replay, grids it left out, rewards of the priority-list replay, grids that left out) of the
    oracle over K steps from row T0 of the carved batch.  The draws do not depend on the layout: two layouts with the same controls
    (6 and 14, 7 and 15) get the SAME control array and the same priority lists -- an id is drawn as an index into the battery-first
    enumeration and translated to the number that list has in the layout's own enumeration -- so their rewards differ through the
    order in which battery and grid are stepped alone."""
    from oracle import oracle as orc
    from pymgrid_amd.priority_list import get_priority_lists, table_array
    orc.build()
    sub = carve(_full(series, mixed), flags)
    L = sub.layout
    cols = sub.materialise().numpy_columns()
    rs = np.random.RandomState(1)
    failed = np.zeros(N, dtype=np.uint8)
    reward = orc.run_batch(cols, _state(cols), T0, K, rs.rand(K, N, L.action_dim), normalized=True, failed=failed)
    lists = get_priority_lists(L.has_genset, L.has_battery, L.has_grid, False, L.grid_before_battery)
    plain = get_priority_lists(L.has_genset, L.has_battery, L.has_grid, False, False)
    assert sorted(plain) == sorted(lists)
    own_number = np.array([lists.index(pl) for pl in plain], dtype=np.uint8)
    ids = own_number[rs.randint(0, len(plain), size=(K, N))]
    failed_ids = np.zeros(N, dtype=np.uint8)
    reward_ids = orc.rollout_batch(cols, _state(cols), T0, K, ids, table_array(lists), failed=failed_ids)
    return reward, failed, reward_ids, failed_ids


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("flags", LAYOUTS)
def test_carve_gives_the_layout_in_both_series_forms(flags, mixed):
    """carve(full, flags) validates as a batch of layout `flags`, keeps no column of an absent module, shares no memory with the
    full batch, and the factorised carve materialises to the materialised carve, column for column."""
    mat, fact = (carve(_full(series, mixed), flags) for series in SERIES)
    for sub in (mat, fact):
        L = sub.layout
        assert flags_of(L) == flags and not L.multi
        assert (L.n_genset, L.n_battery, L.n_grid) == (flags & 1, (flags >> 1) & 1, (flags >> 2) & 1)
        assert L.grid_before_battery == bool(flags & 8)
        assert L.action_dim == 2 * (flags & 1) + ((flags >> 1) & 1) + ((flags >> 2) & 1)
        assert any(k.startswith("gen_") for k in sub.cols) == L.has_genset
        assert any(k.startswith("bat_") or k in ("charge", "soc") for k in sub.cols) == L.has_battery
        assert any(k.startswith("grid_") or k in ("base_co2", "co2_profile", "tariff", "outage_bits") for k in sub.cols) == L.has_grid
        full = _full("factorised" if sub.factorised else "materialised", mixed)
        assert all(t.data_ptr() != full.cols[k].data_ptr() for k, t in sub.cols.items())
    assert fact.factorised and not mat.factorised
    twin = fact.materialise()
    assert set(twin.cols) == set(mat.cols), sorted(set(twin.cols) ^ set(mat.cols))
    for name, t in mat.cols.items():
        assert torch.equal(twin.cols[name], t), name


def test_carve_refuses_what_it_cannot_carve():
    from pymgrid_amd.generator import generate
    with pytest.raises(ValueError):
        carve(_full("materialised", False), 8)               # grid first without a grid and a battery is no layout of its own
    with pytest.raises(ValueError):
        carve(generate(8, n_steps=16, seed=1, arch="genset+battery", device="cpu"), 3)


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("series", SERIES)
@pytest.mark.parametrize("flags", LAYOUTS)
def test_the_oracle_replays_every_carved_batch(flags, series, mixed):
    """K = 140 steps from row 3 with U[0, 1) normalised controls, and with random priority-list ids: the oracle leaves no grid out
    (the GPU matrices compare every grid), every reward is finite, and both series forms replay alike."""
    reward, failed, reward_ids, failed_ids = _replay(flags, series, mixed)
    assert int(failed.sum()) == 0 and int(failed_ids.sum()) == 0, (int(failed.sum()), int(failed_ids.sum()))
    assert reward.shape == reward_ids.shape == (K, N) and np.isfinite(reward).all() and np.isfinite(reward_ids).all()
    other = _replay(flags, SERIES[1 - SERIES.index(series)], mixed)
    assert np.array_equal(reward, other[0]) and np.array_equal(reward_ids, other[2])


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("battery_first,grid_first", [(6, 14), (7, 15)])
def test_the_inputs_tell_grid_first_from_battery_first(battery_first, grid_first, mixed):
    """A kernel that stepped battery and grid in the wrong order would show: under the SAME controls the oracle's rewards of the two
    orders differ on at least 1 % of the (step, grid) pairs and on every grid (measured: 4.2 % for layouts 6 / 14, 7.8 % for
    7 / 15).  Under the same priority lists the fraction is structurally lower (measured: below 0.1 % of the pairs): a list's
    requests are feasible by construction -- every module is asked only for what the modules before it in the LIST leave over -- so
    nothing is clipped in either stepping order and the order shows only where it changes the rounding of the balance sums.  No
    floor follows from that; the roll-out inputs must still show the order somewhere (the kernels are compared exactly)."""
    for which in (0, 2):                                      # continuous controls, priority lists
        a, b = _replay(battery_first, "materialised", mixed)[which], _replay(grid_first, "materialised", mixed)[which]
        differ = a != b
        print(f"layouts {battery_first} / {grid_first}, mixed_timers={mixed}, {'ids' if which else 'controls'}: "
              f"{differ.mean():.4f} of the pairs, {int(differ.any(axis=0).sum())} of {N} grids")
        if which == 0:
            assert differ.mean() >= 0.01 and bool(differ.any(axis=0).all())
        else:
            assert differ.any()


def test_the_inputs_reach_both_genset_forms_of_the_loops():
    """mixed_timers=False: every genset is instantaneous and in equilibrium (timers 0, status on / goal on = 0x0101), the wave-uniform
    GI form of the loops; mixed_timers=True: the first wave (64 grids) holds a genset with a timer, the form with the status FSM."""
    plain, mixed = _full("materialised", False).cols, _full("materialised", True).cols
    assert bool((plain["gen_times"] == 0).all()) and bool((plain["gen_status"] == 257).all())
    assert bool((mixed["gen_times"][:64] != 0).any())
    for series in SERIES:                                     # both series forms hold the same gensets
        for name in ("gen_times", "gen_status"):
            assert torch.equal(_full(series, True).cols[name], mixed[name])


# ---- the inputs of the general-path matrix (tests/test_general_path_matrix.py) ---------------------------------------------------
def _general_mixes():
    import test_general_path_matrix as general
    return general.MIXES


@pytest.mark.parametrize("flags,counts", _general_mixes(), ids=lambda v: str(v).replace(" ", ""))
def test_the_general_path_inputs_meet_their_conditions(flags, counts):
    """The reference side of every mix of the matrix, run here without a GPU: the oracle leaves no grid out (any exception fails),
    two instances of a kind never share their parameters, the fused launches hold eight and nine ``provided`` addends on at least
    1 % of their (step, grid) pairs wherever the list can hold that many (the mirrored mix: eight ``absorbed`` ones), the genset
    status words take more than two values -- ``reference()`` and ``lists_reference()`` assert all of it; the shares are printed."""
    import test_general_path_matrix as general
    ref, lists = general.reference(flags, counts), general.lists_reference(flags, counts)
    print(f"layout {flags}, counts {counts}: shares of the fused launches' pairs {ref['shares']}, of the list roll-outs' {lists['shares']}")
    assert all(np.isfinite(ln["rec"]["common"]["reward"]).all() for ln in ref["launches"] + lists["launches"])


@pytest.mark.parametrize("flags,counts", [(7, (2, 2, 2, 2, 2)), (15, (2, 3, 1, 1, 1)), (0, (0, 0, 0, 2, 2))])
def test_the_vectorised_log_columns_are_the_oracles_log_row(flags, counts):
    """layouts.log_columns (the record arrays of a whole launch) against OracleMultiMicrogrid.log_row (one MStepOut), the statement of
    the log's names in oracle/oracle.py: every column log_row gives, value for value, the packed status word against the four counters
    log_row gives under their own names, and ``violations`` the only name neither has."""
    import test_general_path_matrix as general
    from layouts import log_columns
    from oracle import oracle as orc
    from pymgrid_amd import MicrogridBatch
    grids, ref = general.grids_of(flags, counts), general.reference(flags, counts)
    names = MicrogridBatch.from_grids(grids, device="cpu").layout.log_names
    rec = ref["launches"][2]["rec"]
    columns = log_columns(rec, names)
    assert list(columns) == list(names) and [n for n in names if columns[n] is None] == ["violations"]
    om = orc.OracleMultiMicrogrid(grids[0])
    for k, j in ((0, 0), (3, 17), (8, 199)):
        out = orc.MStepOut.from_buffer_copy(rec[k, j].tobytes())
        for n, v in zip(names, om.log_row(out, names)):
            if v is not None:
                assert columns[n][k, j] == v, (n, k, j)
            elif n != "violations":
                assert n.startswith("genset_status")
                sfx = n[len("genset_status"):]
                cur, goal, up, down = (int(x) for x in om.log_row(out, [c + sfx for c in ("gen_cur", "gen_goal", "gen_up", "gen_down")]))
                assert columns[n][k, j] == float(cur | (goal << 8) | (up << 16) | (down << 24)), (n, k, j)


def _provided_lists(grids, rec, controls, normalized, grid_first):
    """The ``provided`` list of every oracle step of ``rec`` [K, N], rebuilt from the log columns in the order the sweep appends
    (gensets, then the discharging batteries and the importing grids in the layout's order, the pv, the loss load): values
    [K, N, slots] and a mask of the slots the step filled.  One pv only: the log holds the sum over the pvs."""
    from layouts import requests
    g0 = grids[0]
    ng, nb, nr = len(g0.get("genset", [])), len(g0.get("battery", [])), len(g0.get("grid", []))
    assert g0["pv_ts"].shape[1] == 1
    bat, grd = requests(grids, controls, normalized)
    over = rec["common"]["overgeneration"] > 0
    vals = [rec["genset"]["genset_production"][..., j] for j in range(ng)]
    used = [np.ones_like(over)] * ng
    bats = ([rec["battery"]["discharge_amount"][..., j] for j in range(nb)], [~(bat[..., j] < 0) for j in range(nb)])
    grds = ([rec["grid"]["grid_import"][..., j] for j in range(nr)], [~(grd[..., j] < 0) for j in range(nr)])
    for v, u in ((grds, bats) if grid_first else (bats, grds)):
        vals += v; used += u
    vals += [rec["common"]["renewable_used"], rec["common"]["loss_load"]]
    used += [np.ones_like(over), ~over]
    return np.stack(vals, axis=-1), np.stack(used, axis=-1)


@pytest.mark.parametrize("flags,counts", [(7, (2, 2, 2, 1, 1)), (7, (3, 3, 1, 1, 1)), (3, (3, 3, 0, 1, 1)), (7, (3, 3, 3, 1, 1)),
                                          (15, (2, 3, 1, 1, 1))])
def test_the_general_path_inputs_reach_the_pairwise_order_of_the_sums(flags, counts):
    """Where the log holds every addend (one pv), the ``provided`` list of each oracle step of the fused launches is rebuilt in slot
    order: numpy's sum of it (oracle.np_sum: pairwise from eight addends on) IS the step's ``overall_provided`` on every pair, which
    proves the rebuild and layouts.addend_counts -- and on some of the pairs with eight or more addends the plain running sum is
    NOT: a kernel that added its slots up one after the other, or in the order of a wrong slot list, would show on these inputs."""
    import test_general_path_matrix as general
    from layouts import addend_counts
    from oracle import oracle as orc
    grids, ref = general.grids_of(flags, counts), general.reference(flags, counts)
    long_lists = differ = 0
    for ln in ref["launches"]:
        wide = ln["controls"].astype(np.float64)
        vals, used = _provided_lists(grids, ln["rec"], wide, ln["normalized"], bool(flags & 8))
        assert np.array_equal(used.sum(-1), addend_counts(grids, ln["rec"], wide, ln["normalized"])[0])
        overall = ln["rec"]["common"]["overall_provided"]
        for k, j in np.ndindex(overall.shape):
            lst = vals[k, j][used[k, j]]
            assert orc.np_sum(lst) == overall[k, j], (flags, counts, k, j, lst)
            if lst.size >= 8:
                running = 0.0
                for v in lst:
                    running += v
                long_lists += 1
                differ += running != overall[k, j]
    print(f"layout {flags}, counts {counts}: the running sum differs from numpy's on {differ} of the {long_lists} pairs with eight or "
          f"more addends ({differ / max(long_lists, 1):.4f})")
    assert long_lists > 0 and differ > 0


@pytest.mark.parametrize("battery_first,grid_first,counts", [(6, 14, (0, 2, 2, 2, 2)), (7, 15, (2, 2, 2, 2, 2))])
def test_the_general_path_inputs_tell_grid_first_from_battery_first(battery_first, grid_first, counts):
    """With two of a kind, the SAME grids (but for the order of their module list) under the SAME controls: the oracle's rewards of
    the two stepping orders differ -- a general-path kernel that took batteries and grids in the wrong order would show."""
    import test_general_path_matrix as general
    from layouts import OracleGrids, general_controls
    from oracle import oracle as orc
    orc.build()
    controls = general_controls(np.random.RandomState(2), 30, general.N, counts)
    rewards = []
    for flags in (battery_first, grid_first):
        og = OracleGrids(orc, general.grids_of(flags, counts))
        og.reset(T0)
        rewards.append(og.run(controls, True)["common"]["reward"])
    differ = rewards[0] != rewards[1]
    print(f"layouts {battery_first} / {grid_first}, counts {counts}: {differ.mean():.4f} of the pairs, "
          f"{int(differ.any(axis=0).sum())} of {general.N} grids")
    assert differ.any()


# ---- every compiled specialisation of the fused kernels is a case of a GPU matrix -----------------------------------------------
SRC = {"factorised": 0, "materialised": 1, "gather": 2}      # EP_SRC_* of the episode kernels
ARCH_FLAGS = {"genset+battery": 3, "battery+grid": 6, "genset+battery+grid": 7}
UNTEMPLATED_FAMILIES = ("fleet_step_kernel",)               # no template: one instantiation, the empty compile-time part
GENERAL_FAMILIES = ("step_multi_kernel", "step_k_multi_kernel", "step_k_multi_small_kernel", "rollout_multi_small_kernel",
                    "step_lists_small_kernel", "expand_multi_kernel", "check_multi_kernel", "observe_multi_kernel")


def _ctype(dtype):
    return "float" if dtype == torch.float32 else "double"


def enumerated():
    """kernel -> the set of compile-time parts the GPU tests enumerate, out of the tests' own case tuples."""
    import test_episode_rows as rows
    import test_layout_matrix as lock
    import test_layout_matrix_episodes as eps
    import test_rollout_episodes as roll
    import test_step_k_episodes as stepk
    import test_cem as cem
    import test_layout_matrix_policy as pol
    import test_layout_matrix_whatif as whatif
    import test_lookahead as look
    import test_policy_critic as critic
    import test_policy_explore as explore
    import test_policy_gaussian as gauss
    import test_policy_grad as grad
    import test_policy_grad_gaussian as grad_gauss
    import test_policy_rollout as greedy
    import test_policy_sample as sample
    import test_step_k_hot as hot

    def flags(arch):
        return ARCH_FLAGS.get(arch, arch)
    GREEDY, EXPLORE, SAMPLE, SAMPLE_CRITIC, GAUSSIAN, GAUSSIAN_CRITIC = range(6)         # PolicyHead (csrc/mgx_policy.hpp)
    want = {
        # (layout, row source) of the greedy closed-loop kernels; cases (discrete, arch, series, ...) / (layout, series, ..., discrete)
        "rollout_policy_episodes_kernel": {(flags(c[1]), SRC[c[2]]) for c in greedy.CASES if c[0]}
        | {(c[0], SRC[c[1]]) for c in pol.GREEDY_CASES if c[6]},
        "step_k_policy_episodes_kernel": {(flags(c[1]), SRC[c[2]]) for c in greedy.CASES if not c[0]}
        | {(c[0], SRC[c[1]]) for c in pol.GREEDY_CASES if not c[6]},
        # (layout, row source, head)
        "rollout_policy_head_episodes_kernel": {(flags(c[1]), SRC[c[2]], EXPLORE) for c in explore.CASES if c[0]}
        | {(c[0], SRC[c[1]], EXPLORE) for c in pol.EXPLORE_CASES if c[6]}
        | {(flags(c[0]), SRC[c[1]], head) for c in sample.CASES for head in (SAMPLE, SAMPLE_CRITIC)}      # (test_policy_critic runs them too)
        | {(c[0], SRC[c[1]], SAMPLE_CRITIC if c[6] else SAMPLE) for c in pol.SAMPLE_CASES},
        "step_k_policy_head_episodes_kernel": {(flags(c[1]), SRC[c[2]], EXPLORE) for c in explore.CASES if not c[0]}
        | {(c[0], SRC[c[1]], EXPLORE) for c in pol.EXPLORE_CASES if not c[6]}
        | {(c[0], SRC[c[1]], GAUSSIAN) for c in gauss.CASES}
        | {(c[0], SRC[c[1]], GAUSSIAN_CRITIC if c[6] else GAUSSIAN) for c in pol.GAUSSIAN_CASES},
        # (layout, PER_GRID, row source)
        "lookahead_episodes_kernel": {(flags(c[0]), c[5], SRC[c[1]]) for c in look.CASES}
        | {(c[0], c[6], SRC[c[1]]) for c in whatif.DISCRETE_CASES},
        # (layout, control type, PER_GRID, row source)
        "lookahead_step_k_episodes_kernel": {(flags(c[0]), _ctype(c[9]), c[5], SRC[c[1]]) for c in look.CONT_CASES}
        | {(c[0], _ctype(c[7]), c[6], SRC[c[1]]) for c in whatif.CONTINUOUS_CASES},
        # (layout, row source)
        "lookahead_gaussian_episodes_kernel": {(flags(c[0]), SRC[c[1]]) for c in cem.CASES} | {(c[0], SRC[c[1]]) for c in whatif.CEM_CASES},
        # (row width, CRITIC, head: softmax / Gaussian)
        "policy_grad_kernel": {(c[1], c[3], 0) for c in grad.ONE_SAMPLE_CASES} | {(c[2], True, 0) for c in grad.MANY_SAMPLES_CASES}
        | {(c[0], c[1], 0) for c in grad.WIDTH_CASES}
        | {(c[1], c[3], 1) for c in grad_gauss.ONE_SAMPLE_CASES} | {(c[2], True, 1) for c in grad_gauss.MANY_SAMPLES_CASES}
        | {(c[0], c[1], 1) for c in grad_gauss.WIDTH_CASES},
        # (layout, control type)
        "step_k_hot_kernel": {(f, _ctype(dt)) for f in hot.HOT_LAYOUTS for dt in hot.HOT_DTYPES},
        # (layout, control type, RICH, FACT)
        "step_k_kernel": {(f, _ctype(dt), form == "rich", series == "factorised")
                          for f, series, dt in lock.STEP_K_CASES for form in lock.FORMS},
        # (layout, PER_STEP, RICH, FACT)
        "rollout_kernel": {(f, ids == "per_step", form == "rich", series == "factorised") for f, series, ids, form in lock.ROLLOUT_CASES},
        # (layout, PER_STEP, row source)
        "rollout_episodes_kernel": {(ARCH_FLAGS[c[0]], c[5], SRC[c[1]]) for c in roll.CASES}
        | {(c[0], c[5], SRC[c[1]]) for c in eps.ROLLOUT_CASES},
        "rollout_episodes_rows_kernel": {(ARCH_FLAGS[c[0]], c[4], SRC[c[1]]) for c in rows.ROLLOUT_CASES}
        | {(c[0], c[4], SRC[c[1]]) for c in eps.ROLLOUT_ROWS_CASES},
        # (layout, control type, row source)
        "step_k_episodes_kernel": {(ARCH_FLAGS[c[0]], "double", SRC[c[1]]) for c in stepk.CASES}
        | {(c[0], _ctype(c[6]), SRC[c[1]]) for c in eps.STEP_K_CASES},
        "step_k_episodes_rows_kernel": {(ARCH_FLAGS[c[0]], _ctype(c[4]), SRC[c[1]]) for c in rows.STEP_K_CASES}
        | {(c[0], _ctype(c[4]), SRC[c[1]]) for c in eps.STEP_K_ROWS_CASES},
    }
    assert critic.CASES is sample.CASES
    # the general path: (layout, EP) of step_multi_kernel and step_lists_small_kernel, (layout, counts: "RT" or the five compile-time
    # ones) of the two register loops, (layout,) of the rest -- what the calls of every case launch, by the rule stated beside CASES
    import test_general_path_matrix as general
    for kernel in GENERAL_FAMILIES:
        want[kernel] = set()
    for case in general.CASES:
        for kernel, part in general.compiled_forms(*case):
            want[kernel].add(part)
    # the single-step family: what the calls of every case of every table launch, by the rule stated beside the tables
    import test_single_step_matrix as single
    for kernel in single.FAMILIES:
        want[kernel] = set()
    for kind, cases in single.all_cases():
        for case in cases:
            for kernel, part in single.compiled_forms(kind, case):
                want[kernel].add(part)
    assert set(want) >= set(single.FAMILIES) and all(want[k] for k in single.FAMILIES)
    return want


def refused():
    """kernel -> the compile-time parts the matrix files name as compiled but out of every call's reach (each file's REFUSED, with a
    GPU test that asserts the refusal); ``test_every_compiled_specialisation_...`` holds them apart from the cases."""
    import test_layout_matrix_policy as pol
    import test_layout_matrix_whatif as whatif
    import test_general_path_matrix as general
    import test_single_step_matrix as single
    out = {}
    for kernel, part in pol.REFUSED + whatif.REFUSED + general.REFUSED + single.REFUSED:
        out.setdefault(kernel, set()).add(part)
    return out


def compile_time_part(name):
    """(kernel, compile-time part) of a demangled instantiation such as ``mgx::step_k_kernel<7, 8, double, false, true>``; the ring
    depths (U, UA) follow from the rest and are left out."""
    # (a kernel with internal linkage may carry its namespace in brackets; one that is no template has no argument list: the
    #  pointer form of the fleet kernel, whose compile-time part is empty)
    m = re.fullmatch(r"(?:(?:\w+|\(anonymous namespace\))::)*(\w+)(?:<(.*)>)?(?: \(\.\w+\))?", name.strip())
    if not m:
        return None, None
    if m.group(2) is None:
        return m.group(1), (() if m.group(1) in UNTEMPLATED_FAMILIES else None)
    kernel, args, depth = m.group(1), [""], 0
    for ch in m.group(2):                                    # split at the commas outside nested template arguments
        depth += (ch == "<") - (ch == ">")
        if ch == "," and depth == 0:
            args.append("")
        else:
            args[-1] += ch

    def val(a):
        a = a.strip()
        counts = re.fullmatch(r"(?:\w+::)*CountsCT<(.*)>", a)
        if counts:                                           # mgx::CountsCT<2, 2, 1, 1, 1>: the five compile-time counts
            return tuple(int(c) for c in counts.group(1).split(","))
        if re.fullmatch(r"(?:\w+::)*CountsRT", a):
            return "RT"
        return {"true": True, "false": False}.get(a, int(a) if re.fullmatch(r"-?\d+", a) else a)
    args = [val(a) for a in args]
    if kernel in ("step_k_kernel", "rollout_kernel"):               # <F, U, AT | PER_STEP, RICH, FACT>
        return kernel, (args[0], args[2], args[3], args[4])
    if kernel in ("rollout_episodes_kernel", "rollout_episodes_rows_kernel"):    # <F, U, PER_STEP, SRC>
        return kernel, (args[0], args[2], args[3])
    if kernel in ("step_k_episodes_kernel", "step_k_episodes_rows_kernel"):      # <F, U, UA, AT, SRC>
        return kernel, (args[0], args[3], args[4])
    if kernel in ("rollout_policy_episodes_kernel", "step_k_policy_episodes_kernel"):              # <F, U, SRC>
        return kernel, (args[0], args[2])
    if kernel in ("rollout_policy_head_episodes_kernel", "step_k_policy_head_episodes_kernel"):    # <F, U, SRC, HEAD>
        return kernel, (args[0], args[2], args[3])
    if kernel == "lookahead_episodes_kernel":                                    # <F, U, PER_GRID, SRC>
        return kernel, (args[0], args[2], args[3])
    if kernel == "lookahead_step_k_episodes_kernel":                             # <F, U, UA, AT, PER_GRID, SRC>
        return kernel, (args[0], args[3], args[4], args[5])
    if kernel == "lookahead_gaussian_episodes_kernel":                           # <F, U, UA, SRC>
        return kernel, (args[0], args[3])
    if kernel == "policy_grad_kernel":                                           # <D, CRITIC, HEAD>
        return kernel, (args[0], args[1], args[2])
    if kernel == "step_k_hot_kernel":                                            # <F, U, AT>
        return kernel, (args[0], args[2])
    if kernel in ("step_multi_kernel", "step_lists_small_kernel"):               # <F, EP>
        return kernel, (args[0], args[1])
    if kernel in ("step_k_multi_small_kernel", "rollout_multi_small_kernel"):    # <F, CNT, M>
        return kernel, (args[0], args[1])
    if kernel in ("step_k_multi_kernel", "expand_multi_kernel", "check_multi_kernel", "observe_multi_kernel"):    # <F>
        return kernel, (args[0],)
    # the single-step family (tests/test_single_step_matrix.py)
    if kernel in ("step_kernel", "step_discrete_kernel"):                        # <F, EP>
        return kernel, (args[0], args[1])
    if kernel in ("check_kernel", "check_discrete_kernel", "expand_kernel", "observe_kernel", "action_bounds_kernel"):    # <F>
        return kernel, (args[0],)
    if kernel == "obs_rows_wave_kernel":                                         # <F, NOISE, OT>
        return kernel, (args[0], args[1], args[2])
    if kernel in ("obs_windows_k_kernel", "obs_windows_k_multi_kernel"):         # <F, OT>
        return kernel, (args[0], args[1])
    if kernel in ("patch_windows_kernel", "normalise_series_kernel"):            # <GRID, OT>, <C, OT>
        return kernel, (args[0], args[1])
    if kernel == "fleet_step_kernel_v":                                          # <EP>
        return kernel, (args[0],)
    return kernel, None


def missing_cases(usage, want, refused=None):
    """The instantiations in ``usage`` of the families of ``want`` (those of ``enumerated()``) whose compile-time part no GPU
    test enumerates and ``refused`` (kernel -> parts with an asserted refusal) does not name."""
    out = []
    for name in sorted(usage):
        kernel, part = compile_time_part(name)
        if kernel in want and part not in want[kernel] and part not in (refused or {}).get(kernel, ()):
            out.append(name)
    return out


def test_every_compiled_specialisation_is_a_case_of_a_gpu_matrix():
    """A new specialisation of a fused kernel family without a test case fails here, without a GPU; so does a case deleted from
    a matrix tuple (the message names the instantiations left without one)."""
    from pymgrid_amd import _lib
    _lib.build()
    usage = _lib.resource_usage()
    if usage is None:
        pytest.skip("libmgx.so was not built on this machine (no resource_usage.json beside the objects)")
    want = enumerated()
    found = {k: sum(1 for name in usage if compile_time_part(name)[0] == k) for k in want}
    assert all(found.values()), found                        # the parser still recognises every family
    out_of_reach = refused()
    missing = missing_cases(usage, want, out_of_reach)
    assert not missing, f"{len(missing)} compiled specialisation(s) no GPU test runs: {missing}"
    # ... and the other way round: the matrices name nothing the library does not hold (a case that cannot be dispatched)
    held = {k: {compile_time_part(name)[1] for name in usage if compile_time_part(name)[0] == k} for k in want}
    assert all(want[k] <= held[k] for k in want), {k: sorted(want[k] - held[k], key=str) for k in want if not want[k] <= held[k]}
    # a refused form is a compiled one, and no case claims to run it
    assert all(k in want and parts <= held[k] and not parts & want[k] for k, parts in out_of_reach.items()), out_of_reach
    print({k: (len(held[k]), len(out_of_reach.get(k, ()))) for k in sorted(want)})


def test_the_coverage_check_names_what_a_dropped_case_leaves_uncovered():
    """The check above on a made-up library: with one case taken out of the enumeration it names exactly that instantiation."""
    usage = {"mgx::step_k_kernel<14, 4, float, true, false>": {}, "mgx::rollout_kernel<5, 4, true, false, true>": {},
             "mgx::step_k_episodes_rows_kernel<0, 8, 4, double, 2>": {}, "mgx::step_kernel<3, true>": {}}
    want = {"step_k_kernel": {(14, "float", True, False)}, "rollout_kernel": {(5, True, False, True)},
            "step_k_episodes_rows_kernel": {(0, "double", 2)}}
    assert missing_cases(usage, want) == []
    want["rollout_kernel"] = set()
    assert missing_cases(usage, want) == ["mgx::rollout_kernel<5, 4, true, false, true>"]
    # one instantiation of each of the nine closed-loop, what-if, gradient and hot families: a case dropped from any of them
    # leaves exactly that instantiation, and a form named as refused is held apart
    made_up = {"mgx::rollout_policy_episodes_kernel<14, 4, 2>": (14, 2), "mgx::step_k_policy_episodes_kernel<0, 8, 1>": (0, 1),
               "mgx::rollout_policy_head_episodes_kernel<4, 8, 0, 3>": (4, 0, 3), "mgx::step_k_policy_head_episodes_kernel<15, 4, 2, 5>": (15, 2, 5),
               "mgx::lookahead_episodes_kernel<2, 8, true, 1>": (2, True, 1),
               "mgx::lookahead_step_k_episodes_kernel<5, 4, 4, float, false, 2>": (5, "float", False, 2),
               "mgx::lookahead_gaussian_episodes_kernel<6, 2, 1, 0>": (6, 0), "mgx::policy_grad_kernel<3, false, 1>": (3, False, 1),
               "mgx::step_k_hot_kernel<2, 8, float>": (2, "float")}
    usage = dict.fromkeys(list(made_up) + ["mgx::policy_grad_finish_kernel", "lookahead_pick_kernel"], {})
    family = lambda name: compile_time_part(name)[0]          # noqa: E731
    assert len({family(name) for name in made_up}) == 9
    full = {family(name): {part} for name, part in made_up.items()}
    assert all(compile_time_part(name) == (family(name), part) for name, part in made_up.items())
    assert missing_cases(usage, full) == []
    for name in made_up:
        assert missing_cases(usage, {**full, family(name): set()}) == [name]
        assert missing_cases(usage, {**full, family(name): set()}, {family(name): {made_up[name]}}) == []
    # ... and of the eight families of the general path (the compile-time counts nest: the arguments split at depth 0)
    made_up = {"mgx::step_multi_kernel<14, true>": (14, True), "mgx::step_k_multi_kernel<5>": (5,),
               "mgx::step_k_multi_small_kernel<7, mgx::CountsCT<2, 2, 1, 1, 1>, 2>": (7, (2, 2, 1, 1, 1)),
               "mgx::rollout_multi_small_kernel<15, mgx::CountsRT, 2>": (15, "RT"), "mgx::step_lists_small_kernel<1, false>": (1, False),
               "mgx::expand_multi_kernel<6>": (6,), "mgx::check_multi_kernel<2>": (2,), "mgx::observe_multi_kernel<0>": (0,)}
    usage = dict.fromkeys(list(made_up) + ["mgx::obs_windows_k_multi_kernel<7, float>", "mgx::action_bounds_kernel<7>"], {})
    assert {family(name) for name in made_up} == set(GENERAL_FAMILIES)
    full = {family(name): {part} for name, part in made_up.items()}
    assert all(compile_time_part(name) == (family(name), part) for name, part in made_up.items())
    assert compile_time_part("mgx::step_k_multi_small_kernel<3, mgx::CountsCT<3, 3, 0, 1, 1>, 3>")[1] == (3, (3, 3, 0, 1, 1))
    assert missing_cases(usage, full) == []
    for name in made_up:
        assert missing_cases(usage, {**full, family(name): set()}) == [name]
        assert missing_cases(usage, {**full, family(name): set()}, {family(name): {made_up[name]}}) == []
    # ... and of the families of the single-step path (tests/test_single_step_matrix.py); the pointer form of the fleet kernel is no
    # template: one instantiation, whose compile-time part is empty
    made_up = {"mgx::step_kernel<14, true>": (14, True), "mgx::step_discrete_kernel<5, false>": (5, False), "mgx::check_kernel<6>": (6,),
               "mgx::check_discrete_kernel<15>": (15,), "mgx::expand_kernel<1>": (1,), "mgx::observe_kernel<0>": (0,),
               "mgx::action_bounds_kernel<2>": (2,), "mgx::obs_rows_wave_kernel<4, true, float>": (4, True, "float"),
               "mgx::obs_windows_k_kernel<3, double>": (3, "double"), "mgx::obs_windows_k_multi_kernel<7, float>": (7, "float"),
               "mgx::patch_windows_kernel<true, float>": (True, "float"), "mgx::normalise_series_kernel<4, double>": (4, "double"),
               "mgx::fleet_step_kernel_v<true>": (True,), "mgx::fleet_step_kernel": (),
               "(anonymous namespace)::fleet_step_kernel_v<false>": (False,)}
    usage = dict.fromkeys(list(made_up) + ["mgx::fleet_step_kernel_vm", "mgx::gather_windows_kernel"], {})
    assert len({family(name) for name in made_up}) == 14
    assert all(compile_time_part(name) == (family(name), part) for name, part in made_up.items())
    full = {}
    for name, part in made_up.items():
        full.setdefault(family(name), set()).add(part)
    assert missing_cases(usage, full) == []
    for name in made_up:
        less = {**full, family(name): full[family(name)] - {made_up[name]}}
        assert missing_cases(usage, less) == [name]
        assert missing_cases(usage, less, {family(name): {made_up[name]}}) == []


# ---- the inputs of the single-step matrix (tests/test_single_step_matrix.py) ------------------------------------------------------
def test_the_columns_of_a_carved_batch_give_the_oracles_parameter_dicts():
    """layouts.single_params on layouts 7 and 14: the dicts carry the battery's charge / soc, the genset's status counters and timers,
    ``controllable_order`` (grid first on 14), horizon and final_step; an OracleMicrogrid of them, stepped, is the batch oracle's
    replay of the same columns -- reward for reward -- and its state is what ``numpy_columns()`` held."""
    import test_single_step_matrix as single
    from layouts import OracleSingles, single_params
    from oracle import oracle as orc
    orc.build()
    for flags in (7, 14):
        cols = single.columns(flags, 3)
        params = single_params(cols)
        assert len(params) == single.N and all(p["horizon"] == 3 and p["final_step"] == single.T for p in params)
        assert all(("genset" in p, "battery" in p, "grid" in p) == (bool(flags & 1), True, True) for p in params)
        assert all(p["controllable_order"].index("grid") < p["controllable_order"].index("battery") for p in params) == (flags == 14)
        assert [p["battery"]["charge"] for p in params] == cols["charge"].tolist() and [p["battery"]["soc"] for p in params] == cols["soc"].tolist()
        og = OracleSingles(orc, cols)
        for name, want in og.state().items():
            assert np.array_equal(want, cols[name]), (flags, name)
        if flags & 1:
            times = cols["gen_times"]
            assert [p["genset"]["start_up_time"] for p in params] == (times & 0xff).tolist()
            assert [p["genset"]["wind_down_time"] for p in params] == ((times >> 16) & 0xff).tolist()
            assert len(set((times & 0xff).tolist())) > 1, "mixed timers"
        rs = np.random.RandomState(flags)
        controls = rs.rand(8, single.N, og.action_dim)
        og.reset(single.T0)
        rec = og.run(controls, True)
        st = _state(cols)
        failed = np.zeros(single.N, dtype=np.uint8)
        reward = orc.run_batch(cols, st, single.T0, 8, controls, normalized=True, failed=failed)
        assert int(failed.sum()) == 0 and np.array_equal(rec["reward"], reward), flags
        for name, want in og.state().items():
            assert np.array_equal(want, st[name]), (flags, name)


def _single_references():
    import test_single_step_matrix as single
    need = sorted({(case[0], 0, case[2]) for case in single.LOCKSTEP_CASES}
                  | {(case[0], case[1], "double") for case in single.ROWS_CASES + single.RING_CASES + single.VIEW_CASES})
    return need


@pytest.mark.parametrize("flags,H,ctype", _single_references())
def test_the_single_step_inputs_meet_their_conditions(flags, H, ctype):
    """The reference side of every lock-step, row, ring and view case of the single-step matrix, run here without a GPU: the oracle
    leaves out no grid (any exception fails), both values of ``done`` occur, every form of the genset status word occurs (off, on,
    starting up, winding down), and with a horizon the windows of the last rows run into the padding behind the series --
    ``lockstep_reference`` asserts all of it."""
    import test_single_step_matrix as single
    ref = single.lockstep_reference(flags, H, ctype)
    assert ref["rec"].shape == (single.STEPS + single.TAIL, single.N)
    assert ref["obs"].shape[2] == ref["obs0"].shape[1] == carve(single._full("materialised", H), flags).layout.obs_dim
    assert ref["controls"].dtype == (np.float32 if ctype == "float" else np.float64)
    assert ((ref["controls"] == 0) | (ref["controls"] == 1)).any() or flags == 0


@pytest.mark.parametrize("flags", LAYOUTS)
def test_the_general_path_ring_inputs_meet_their_conditions(flags):
    """The reference side of the ring refill of the general path: no grid left out, the last step alone reports done, two instances
    of a kind never share their parameters -- ``multi_reference`` asserts it."""
    import test_single_step_matrix as single
    ref = single.multi_reference(flags)
    assert np.isfinite(ref["rec"]["reward"]).all() and np.isfinite(ref["obs"]).all()
    assert ref["obs"].shape[:2] == (single.STEPS + single.TAIL, single.MULTI_N)


@pytest.mark.parametrize("H", [0, 3])
@pytest.mark.parametrize("flags", LAYOUTS)
def test_the_single_step_discrete_inputs_meet_their_conditions(flags, H):
    """... and of the discrete cases: no grid left out (an assert of ``populate_action`` fails here), the ids reach every list of the
    layout, both genset goals occur, the last step alone reports done -- ``discrete_reference`` asserts it."""
    import test_single_step_matrix as single
    ref = single.discrete_reference(flags, H)
    assert ref["control"].shape == (single.STEPS + single.TAIL, single.N, single.action_dim(flags))
    assert np.isfinite(ref["rec"]["reward"]).all()


def test_the_single_step_case_tables_are_complete():
    """Every (layout, row type) of the row, ring and view tables sees one of the two horizons and every layout both; the episode table
    holds every layout continuous and discrete with whole rows, and all four forms of the ring patch; every case names forms the
    dispatch rule knows."""
    import test_single_step_matrix as single
    for table in (single.ROWS_CASES, single.RING_CASES, single.VIEW_CASES):
        assert {(c[0], c[2]) for c in table} == {(f, ot) for f in LAYOUTS for ot in single.FLOATS}
        assert all({c[1] for c in table if c[0] == f} == set(single.HORIZONS) for f in LAYOUTS)
    # the fleet kernels pick the layout's step body by a run-time switch, one for continuous and one for discrete items: the compiled
    # symbols cannot show a case label nobody runs, the table must -- every (kernel form, layout, discrete) triple, once
    triples = [t for c in single.FLEET_CASES for t in single.fleet_triples(c)]
    assert len(triples) == len(set(triples)) and set(triples) == {(form, f, d) for form in single.FLEET_KERNELS for f in LAYOUTS
                                                                   for d in (False, True)}
    assert all(len(fleet) <= 5 for fleet in single.FLEETS), "MGX_FLEET_MAX buckets share a launch"
    assert {c[:3] for c in single.EPISODE_CASES if c[2] == 0} == {(f, d, 0) for f in LAYOUTS for d in (False, True)}
    patched = {part for c in single.EPISODE_CASES for k, part in single.compiled_forms("episodes", c) if k == "patch_windows_kernel"}
    assert patched == {(g, ot) for g in (False, True) for ot in single.FLOATS}
    assert single.EPISODE_STEPS // single.LENGTH >= 2 and single.T - single.LENGTH > single.N // 16, "restarts on every grid, own rows"
    assert single.N % single.BLOCK == 64 + 13 and single.N // single.BLOCK == 2 and single.N % 16 == 13
    for kind, cases in single.all_cases():
        assert len(set(cases)) == len(cases) and all(single.compiled_forms(kind, c) for c in cases), kind


def _episode_inputs():
    import test_single_step_matrix as single
    return sorted({(c[0], c[2], c[1]) for c in single.EPISODE_CASES})


@pytest.mark.parametrize("flags,H,discrete", _episode_inputs())
def test_the_oracle_replays_the_first_episodes_of_the_episode_cases(flags, H, discrete):
    """The oracle half of the episode and episode-fleet cases as far as it is known without a GPU: the first episodes start at rows
    drawn on the host (``episode_starts``) and take the case's own draws; the oracle leaves out no grid (an exception fails), and with
    one fixed length for every grid each of them is over -- and restarted -- after exactly LENGTH steps, EPISODE_STEPS // LENGTH times
    in a case.  The rows of the later episodes are drawn on the device: an exception of the oracle there fails the GPU case."""
    import test_single_step_matrix as single
    from layouts import OracleSingles
    from oracle import oracle as orc
    orc.build()
    og = OracleSingles(orc, single.columns(flags, H))
    starts = single.episode_starts(flags)
    assert starts.min() >= 0 and starts.max() + single.LENGTH <= single.T and len(np.unique(starts)) > 10
    og.reset(starts)
    draw, lists = single.episode_draws(flags, discrete), single.priority_lists(flags)
    for k in range(single.LENGTH):
        a = draw(k)
        rec = og.step(og.expand([lists[i] for i in a]), False) if discrete else og.step(a, True)
        assert np.isfinite(rec["reward"]).all()
    assert np.array_equal(og.rows(), starts + single.LENGTH) and single.EPISODE_STEPS // single.LENGTH >= 2


@pytest.mark.parametrize("flags", LAYOUTS)
def test_the_raise_errors_golden_meets_its_conditions(flags):
    """tests/golden/raise_errors.npz (make_raise_errors_goldens.py), re-asserted from the file: 16 grids and 24 steps per layout, half
    of the grids raw; for every module kind of the layout at least 20 % of the (step, grid) pairs are refused (ValueError) and at
    least 20 % accepted; every request exactly at the instantaneous limit is accepted and every one an ulp beyond it refused; the
    recorded table is the layout's own enumeration of priority lists; the bounds are recorded where there is a battery / a grid."""
    import test_single_step_matrix as single
    from pymgrid_amd import MicrogridBatch
    from pymgrid_amd.priority_list import table_array
    g = single.raise_errors_golden(flags)
    assert len(g["grids"]) == 16 and g["requests"].shape[:2] == (24, 16) and int(g["raw"].sum()) == 8
    assert flags_of(MicrogridBatch.from_grids(g["grids"], device="cpu").layout) == flags
    assert np.array_equal(g["table"], table_array(single.priority_lists(flags)))
    assert 16 * single.GOLDEN_TILES // 2 == 336
    for q in range(3):
        exc, how = g["exception"][..., q], g["how"][..., q]
        if not flags & (1 << q):
            assert (exc == single.GOLDEN_ABSENT).all() and (g["list_exception"][..., q] == single.GOLDEN_ABSENT).all()
            continue
        refused = exc == single.GOLDEN_VALUE_ERROR
        assert 0.2 <= refused.mean() <= 0.8, (flags, q, refused.mean())
        assert np.isin(exc, (single.GOLDEN_NONE, single.GOLDEN_VALUE_ERROR, single.GOLDEN_ASSERTION_ERROR)).all()
        at, beyond = how == single.GOLDEN_AT_LIMIT, how == single.GOLDEN_BEYOND
        assert at[:, g["raw"]].any() and beyond[:, g["raw"]].any() and not at[:, ~g["raw"]].any() and not beyond[:, ~g["raw"]].any()
        assert not refused[at].any(), (flags, q, "a request at the limit was refused")
        assert refused[beyond].all(), (flags, q, "a request one ulp beyond the limit was accepted")
        if q:
            assert np.isfinite(g["bounds"][:, :, q - 1]).all()
    if flags & 1:                                            # timers and both initial states among the gensets; weak grids below
        assert len({(p["genset"]["start_up_time"], p["genset"]["wind_down_time"]) for p in g["grids"]}) > 4
    if flags & 4:
        assert any((p["grid_ts"][:, 3] == 0).any() for p in g["grids"])
