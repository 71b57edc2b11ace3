"""The closed-loop policy kernels -- rollout_policy_episodes_kernel, step_k_policy_episodes_kernel and the head kernels
rollout_policy_head_episodes_kernel (exploring / sampling / sampling + critic) and step_k_policy_head_episodes_kernel (exploring /
Gaussian / Gaussian + critic) -- in EVERY compiled form: all ten module layouts x the three row sources x every head, on batches
carved out of one generated batch (tests/layouts.py), with the comparisons of test_policy_rollout.py / test_policy_explore.py /
test_policy_sample.py / test_policy_critic.py / test_policy_gaussian.py (the fused launch == a twin stepped with the host rule, bit
for bit, through restarts).  Over those files this one adds: the greedy and exploring heads on the (layout, source) pairs their
layout sweeps leave out (each layout ran with ONE source there), the sampling and critic heads on the seven layouts beside 7, 3
and 5, the Gaussian heads on layouts 0, 4 and 14 and on most (layout, source, critic) triples -- and, per layout, an independent
replay by the CPU oracle of what the greedy, the sampling + critic and the Gaussian + critic launches did."""
import pytest
import torch

import test_policy_critic as critic_tests
import test_policy_explore as explore_tests
import test_policy_gaussian as gaussian_tests
import test_policy_rollout as greedy_tests
import test_policy_sample as sample_tests
from layouts import LAYOUTS, replay
from test_layout_matrix_episodes import SOURCES, rotate

F64, F32 = torch.float64, torch.float32
LENGTHS, HIDDEN, ROWS, SIZES, POPULATION = (9, None), (0, 16), (F64, F32), (300, 256), (1, 3)
LAUNCHES = (7, 7)                # the 7-step launch of the layout sweeps, twice: an episode of 9 steps ends inside the second
T = 200                          # test_policy_rollout.T: the series the greedy and exploring helpers generate
GAUSSIAN_STEPS = 12              # test_policy_gaussian.K: one launch, an episode of 9 steps ends inside it


def _with_population(cases):
    """``cases`` of rotate() with a fifth rotating factor behind the crossed one: the population, by the case's source and flipped by
    the layout's index, so that every layout sees one set and three."""
    return tuple(c + (POPULATION[(q % 6 // 2 + q // 6) % 2],) for q, c in enumerate(cases))


# (layout, series, length, n_hidden, row format, batch size, discrete) -- one case per form of the two greedy kernels, and of the
# exploring head of the two head kernels
GREEDY_CASES = rotate(LAYOUTS, (True, False), LENGTHS, HIDDEN, ROWS, SIZES)
EXPLORE_CASES = GREEDY_CASES
# (layout, series, length, n_hidden, row format, batch size, critic, population) -- the sampling heads of the discrete head kernel,
# the Gaussian heads of the continuous one
SAMPLE_CASES = _with_population(rotate(LAYOUTS, (False, True), LENGTHS, HIDDEN, ROWS, SIZES))
GAUSSIAN_CASES = SAMPLE_CASES
# What a layout cannot show, and why (the conditions every case asserts on its reference side, _not_vacuous):
ONE_LIST = {0: "no controllable module: the one empty list", 2: "a battery alone: one list", 4: "a grid alone: one list"}
NO_CONTROL = {0: "no controllable module: no control column"}
N_LISTS = {0: 1, 1: 2, 2: 1, 3: 4, 4: 1, 5: 4, 6: 2, 7: 12, 14: 2, 15: 12}
# discrete ids: a single list is taken at every step; controls: there is none to move, to clip or to draw
CANNOT_MOVE = {True: ONE_LIST, False: NO_CONTROL}
# The seed of the greedy policy's parameters (test_policy_rollout._policy), per layout: 7, the helpers' own, but 9 on layout 3 --
# there the policy of seed 7 takes ONE list at every row of every grid, so no id would change between two steps (9 does the same on
# layout 1 at own lengths; seen on the stepped twin alone).  With these the oracle leaves no grid out.
POLICY_SEED = {flags: 9 if flags == 3 else 7 for flags in LAYOUTS}
# Compiled forms no call reaches: none -- every head runs on every layout (a policy without outputs included)
REFUSED = ()


def test_the_rotation_gives_every_layout_every_value_of_every_factor():
    for cases, factors in ((GREEDY_CASES, (LENGTHS, HIDDEN, ROWS, SIZES, (True, False))),
                           (SAMPLE_CASES, (LENGTHS, HIDDEN, ROWS, SIZES, (False, True), POPULATION))):
        assert len(set(cases)) == len(cases) == 60
        by_layout = {}
        for c in cases:
            by_layout.setdefault(c[0], []).append(c[1:])
        assert tuple(by_layout) == LAYOUTS
        for flags, cs in by_layout.items():
            assert len(cs) == 6 and {(c[0], c[5]) for c in cs} == {(s, x) for s in SOURCES for x in (False, True)}     # crossed
            for column, values in zip(list(zip(*cs))[1:], factors):
                assert set(column) == set(values), (flags, column)


def test_the_tables_of_what_a_layout_cannot_show_are_the_layouts_own():
    from pymgrid_amd.priority_list import get_priority_lists
    for flags in LAYOUTS:
        lists = get_priority_lists(bool(flags & 1), bool(flags & 2), bool(flags & 4), False, bool(flags & 8))
        assert len(lists) == N_LISTS[flags] and (len(lists) == 1) == (flags in ONE_LIST)
        assert (flags & 7 == 0) == (flags in NO_CONTROL)


def _not_vacuous(trace, flags, discrete, length, n, sampled=False, gaussian=False):
    """The conditions on a case itself, from the stepped twin ALONE: grids restarted inside a launch; where the layout can show it
    (CANNOT_MOVE names the others), a grid's action changed between two steps; a sampling head took two ids and left the greedy
    one somewhere; a Gaussian head met both edges of the clip and its interior, and drew beyond them."""
    done = torch.cat([ln["done"] for ln in trace["launches"]])
    taken = torch.cat([ln["taken"] for ln in trace["launches"]])
    restarts = int(done.sum())
    inside = any(bool(ln["done"][:-1].any()) for ln in trace["launches"])             # ... before a launch's last step
    assert inside and (restarts >= n if length is not None else restarts >= 1), (restarts, inside)
    if discrete:
        assert len(trace["table"]) == N_LISTS[flags]
    else:
        assert taken.shape[2] == 2 * (flags & 1) + ((flags >> 1) & 1) + ((flags >> 2) & 1)
    if flags in CANNOT_MOVE[discrete]:
        assert not bool((taken[1:] != taken[:-1]).any())                              # (and the table says why)
        return
    assert bool((taken[1:] != taken[:-1]).any())
    if sampled:
        assert taken.unique().numel() >= 2 and bool((taken != trace["greedy"]).any())
    if gaussian:
        raw = trace["raw"]
        assert bool((taken == 0).any()) and bool((taken == 1).any()) and bool(((taken > 0) & (taken < 1)).any())
        assert bool((raw < 0).any()) and bool((raw > 1).any())


@pytest.mark.gpu
@pytest.mark.parametrize("flags,series,length,n_hidden,obs_dtype,n,discrete", GREEDY_CASES)
def test_greedy_fused_equals_stepped(flags, series, length, n_hidden, obs_dtype, n, discrete, device):
    trace = {}
    greedy_tests._fused_equals_stepped(device, discrete, flags, series, length, n_hidden, n, obs_dtype=obs_dtype, launches=LAUNCHES, trace=trace,
                                       seed=POLICY_SEED[flags])
    _not_vacuous(trace, flags, discrete, length, n)


@pytest.mark.gpu
@pytest.mark.parametrize("flags,series,length,n_hidden,obs_dtype,n,discrete", EXPLORE_CASES)
def test_exploring_fused_equals_stepped(flags, series, length, n_hidden, obs_dtype, n, discrete, device):
    trace = {}
    explore_tests._fused_equals_stepped(device, discrete, flags, series, length, n_hidden, n, obs_dtype=obs_dtype, launches=LAUNCHES,
                                        trace=trace)
    _not_vacuous(trace, flags, discrete, length, n)
    if flags not in CANNOT_MOVE[discrete]:                   # the exploration moved an action away from the greedy one
        assert bool((torch.cat([ln["taken"] for ln in trace["launches"]]) != trace["greedy"].to(trace["launches"][0]["taken"].dtype)).any())


@pytest.mark.gpu
@pytest.mark.parametrize("flags,series,length,n_hidden,obs_dtype,n,critic,P", SAMPLE_CASES)
def test_sampling_fused_equals_stepped(flags, series, length, n_hidden, obs_dtype, n, critic, P, device):
    """vacuous=False: the helpers' own conditions are those of layout 7's twelve lists (every id taken, a non-greedy share of 20 %);
    _not_vacuous states what holds on every layout."""
    trace = {}
    helper = (critic_tests if critic else sample_tests)._fused_equals_stepped
    helper(device, flags, series, n_hidden, obs_dtype, P=P, vacuous=False, n=n, length=length, t=T, launches=LAUNCHES, trace=trace)
    _not_vacuous(trace, flags, True, length, n, sampled=True)


@pytest.mark.gpu
@pytest.mark.parametrize("flags,series,length,n_hidden,obs_dtype,n,critic,P", GAUSSIAN_CASES)
def test_gaussian_fused_equals_stepped(flags, series, length, n_hidden, obs_dtype, n, critic, P, device):
    trace = {}
    gaussian_tests._fused_equals_stepped(device, flags, series, n_hidden, obs_dtype, P, critic=critic, n=n, length=length,
                                         steps=GAUSSIAN_STEPS, trace=trace)
    _not_vacuous(trace, flags, False, length, n, gaussian=True)


# ---- the independent check: the oracle replays what the closed loop did -----------------------------------------------------------
# (layout, source, length): once per layout, the source and the length rotating over the layouts
ORACLE_CASES = tuple((flags, SOURCES[li % 3], LENGTHS[li % 2]) for li, flags in enumerate(LAYOUTS))


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["greedy_discrete", "greedy_continuous", "sampling_critic", "gaussian_critic"])
@pytest.mark.parametrize("flags,series,length", ORACLE_CASES)
def test_closed_loop_launches_vs_the_oracle(flags, series, length, family, device, oracle):
    """The series rows every grid walked, the ids / clipped controls the launch reports and the state before the first launch, replayed
    by the CPU oracle: rewards and final state bit for bit on EVERY grid.  No shaper, no forecast horizon (the oracle's reward is
    the unshaped one)."""
    trace = {}
    n = SIZES[LAYOUTS.index(flags) % 2]
    if family == "greedy_discrete":
        greedy_tests._fused_equals_stepped(device, True, flags, series, length, 16, n, launches=LAUNCHES, trace=trace, seed=POLICY_SEED[flags])
    elif family == "greedy_continuous":
        greedy_tests._fused_equals_stepped(device, False, flags, series, length, 16, n, launches=LAUNCHES, trace=trace, seed=POLICY_SEED[flags])
    elif family == "sampling_critic":
        critic_tests._fused_equals_stepped(device, flags, series, 16, vacuous=False, n=n, length=length, t=T, launches=LAUNCHES, trace=trace)
    else:
        gaussian_tests._fused_equals_stepped(device, flags, series, 16, F64, 1, critic=True, n=n, length=length, steps=GAUSSIAN_STEPS,
                                             trace=trace)
    assert sum(ln["rows"].shape[0] for ln in trace["launches"]) == (GAUSSIAN_STEPS if family == "gaussian_critic" else sum(LAUNCHES))
    replay(oracle, trace["cols"], trace, normalized=True, label=f"{family}, layout {flags}, {series}")
