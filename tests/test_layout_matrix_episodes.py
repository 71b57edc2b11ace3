"""The four fused per-grid-episode kernel families (rollout_episodes_kernel, step_k_episodes_kernel and their forms with
observation rows) on the seven module layouts that generate(arch=...) cannot draw -- 0, 1, 2, 4, 5 and the grid-first 14 and 15 --
from all three row sources, with the comparisons of test_rollout_episodes.py / test_step_k_episodes.py / test_episode_rows.py (the
fused launches == a single-stepped twin, bit for bit, through restarts), the single-step episode kernels of those layouts against
the rolling window buffers (test_episodes_inplace.py) and, per layout, an independent replay of the series rows the grids walked
by the CPU oracle.  The batches are carved out of one generated batch (tests/layouts.py).  The closed-loop policy kernels and the
what-if kernels have matrices of the same shape: tests/test_layout_matrix_policy.py, tests/test_layout_matrix_whatif.py."""
import itertools

import pytest
import torch

import test_episode_rows as rows_tests
import test_episodes_inplace as inplace_tests
import test_rollout_episodes as rollout_tests
import test_step_k_episodes as step_k_tests
from layouts import carve, replay

EPISODE_LAYOUTS = (0, 1, 2, 4, 5, 14, 15)                    # 3, 6, 7: the generated architectures of the files above
GENERATED = (3, 6, 7)
SOURCES = ("factorised", "materialised", "gather")           # EP_SRC_FACT, the grid-major copy, gathered out of [T, N]
F64, F32 = torch.float64, torch.float32
# every compiled form has a case: the compile-time factor beside layout and source (fixed / per-step ids; the control type) is
# crossed with them, the run-time factors of the existing tests rotate
PATTERNS = ((0, 0, 0, 0), (1, 1, 1, 1), (0, 1, 0, 1), (1, 0, 1, 0), (0, 0, 1, 1), (1, 1, 0, 0))


def rotate(layouts, crossed, *factors):
    """[(layout, source, *rotating factor values, crossed value)]: layouts x SOURCES x `crossed`; the (at most four) two-valued
    `factors` take, over the six cases of a layout, each of their values at least once (PATTERNS, flipped by the layout's index so
    that the layouts do not all see the same combinations)."""
    out = []
    for li, flags in enumerate(layouts):
        for q, (series, c) in enumerate(itertools.product(SOURCES, crossed)):
            bits = [p ^ ((li >> j) & 1) for j, p in enumerate(PATTERNS[q])]
            out.append((flags, series) + tuple(f[b] for f, b in zip(factors, bits)) + (c,))
    return tuple(out)


LENGTHS, HORIZONS, ONOFF = (9, None), (0, 6), (False, True)
# (layout, series, length, H, shaper, per_step) -- the arguments of test_rollout_episodes.CASES
ROLLOUT_CASES = rotate(EPISODE_LAYOUTS, (False, True), LENGTHS, HORIZONS, ONOFF)
# (layout, series, length, H, shaper, normalized, control dtype); float32 controls also on the generated layouts, where
# test_step_k_episodes.CASES run float64 only
STEP_K_CASES = rotate(EPISODE_LAYOUTS, (F64, F32), LENGTHS, HORIZONS, ONOFF, (True, False)) \
    + tuple(c for c in rotate(GENERATED, (F64, F32), LENGTHS, HORIZONS, ONOFF, (True, False)) if c[6] == F32)
# (layout, series, length, obs dtype, per_step, shaper) -- the arguments of test_episode_rows.ROLLOUT_CASES
ROLLOUT_ROWS_CASES = tuple((f, s, ln, od, ps, sh) for f, s, ln, od, sh, ps in rotate(EPISODE_LAYOUTS, (False, True), LENGTHS, (F64, F32), ONOFF))
# (layout, series, length, obs dtype, action dtype, normalized) -- the arguments of test_episode_rows.STEP_K_CASES
STEP_K_ROWS_CASES = tuple((f, s, ln, od, ad, nm) for f, s, ln, od, nm, ad in rotate(EPISODE_LAYOUTS, (F64, F32), LENGTHS, (F64, F32), (True, False)))


def test_the_rotation_gives_every_layout_every_value_of_every_factor():
    for cases, n_layouts in ((ROLLOUT_CASES, 7), (STEP_K_CASES, 10), (ROLLOUT_ROWS_CASES, 7), (STEP_K_ROWS_CASES, 7)):
        assert len(set(cases)) == len(cases)
        by_layout = {}
        for c in cases:
            by_layout.setdefault(c[0], []).append(c[1:])
        assert len(by_layout) == n_layouts
        for flags, cs in by_layout.items():
            if flags in GENERATED:
                continue                                      # (only the float32 half: the rest is test_step_k_episodes.CASES)
            for column in zip(*cs):
                assert len(set(column)) >= 2, (flags, column)
            assert {c[0] for c in cs} == set(SOURCES) and len(cs) == 6


def carved(device, flags, series, H=0, seed=17, n=None, t=None):
    """The batch factory of the comparison helpers: layout `flags` carved out of the genset+battery+grid batch they would generate."""
    full = step_k_tests._batch(device, "genset+battery+grid", series, H, seed=seed, n=n or step_k_tests.N, t=t or step_k_tests.T)
    return carve(full, flags)


@pytest.mark.gpu
@pytest.mark.parametrize("flags,series,length,H,shaper,per_step", ROLLOUT_CASES)
def test_rollout_equals_single_steps(flags, series, length, H, shaper, per_step, device):
    rollout_tests._rollout_equals_single_steps(device, flags, series, length, H, shaper, per_step, make_batch=carved)


@pytest.mark.gpu
@pytest.mark.parametrize("flags,series,length,H,shaper,normalized,dtype", STEP_K_CASES)
def test_step_k_equals_single_steps(flags, series, length, H, shaper, normalized, dtype, device):
    step_k_tests._fused_equals_single_steps(device, flags, series, length, H, shaper, normalized, dtype=dtype, make_batch=carved)


@pytest.mark.gpu
@pytest.mark.parametrize("flags,series,length,obs_dtype,per_step,shaper", ROLLOUT_ROWS_CASES)
def test_rollout_rows_equal_single_steps(flags, series, length, obs_dtype, per_step, shaper, device):
    rows_tests._rows_equal_single_steps(device, True, flags, series, length, obs_dtype, shaper=shaper, per_step=per_step, make_batch=carved)


@pytest.mark.gpu
@pytest.mark.parametrize("flags,series,length,obs_dtype,action_dtype,normalized", STEP_K_ROWS_CASES)
def test_step_k_rows_equal_single_steps(flags, series, length, obs_dtype, action_dtype, normalized, device):
    rows_tests._rows_equal_single_steps(device, False, flags, series, length, obs_dtype, normalized=normalized, action_dtype=action_dtype,
                                        make_batch=carved)


# (layout, H, discrete, length, final observations, observation prefetch): the single-step episode kernels (EP = true) the fused
# launches are compared with, against the rolling window buffers
INPLACE_CASES = tuple((flags, (0, 5)[li % 2], bool((li // 2) % 2), (9, None)[(li + 1) % 2], bool(li % 3 == 0), (0, 4)[li % 2])
                      for li, flags in enumerate(EPISODE_LAYOUTS))


@pytest.mark.gpu
@pytest.mark.parametrize("series", ["factorised", "materialised"])
@pytest.mark.parametrize("flags,H,discrete,length,final,prefetch", INPLACE_CASES)
def test_native_auto_reset_equals_the_rolling_window_auto_reset(flags, H, discrete, length, final, prefetch, series, device):
    def factory(n, t, arch, dev, h, series):
        return carve(inplace_tests._gen(n, t, "genset+battery+grid", dev, h, series=series), arch)
    inplace_tests._native_equals_rolling(device, flags, H, discrete, length, final, prefetch, series, make_batch=factory)


# ---- the independent check: the oracle replays the rows the grids walked ---------------------------------------------------------
def _replay(oracle, device, flags, series, trace, normalized=True):
    """layouts.replay on the batch the helpers carved: every launch of LAUNCHES is in the trace."""
    assert sum(ln["rows"].shape[0] for ln in trace["launches"]) == sum(step_k_tests.LAUNCHES)
    assert len(torch.cat([ln["rows"][:, 0] for ln in trace["launches"]]).unique()) > 10          # (grid 0 alone walks more than ten rows)
    replay(oracle, carved(device, flags, series).numpy_columns(), trace, normalized, f"layout {flags}, {series}")


ORACLE_CASES = tuple((flags, SOURCES[li % 3], LENGTHS[li % 2]) for li, flags in enumerate(EPISODE_LAYOUTS))


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["rollout", "step_k", "rollout_rows", "step_k_rows"])
@pytest.mark.parametrize("flags,series,length", ORACLE_CASES)
def test_fused_episodes_vs_the_oracle(flags, series, length, family, device, oracle):
    """No forecast horizon, no shaper (the oracle's reward is the unshaped one); raw controls (normalized=False) on every other
    layout of the continuous families."""
    trace = {}
    normalized = bool(EPISODE_LAYOUTS.index(flags) % 2)
    if family == "rollout":
        rollout_tests._rollout_equals_single_steps(device, flags, series, length, 0, False, True, make_batch=carved, trace=trace)
    elif family == "step_k":
        step_k_tests._fused_equals_single_steps(device, flags, series, length, 0, False, normalized, make_batch=carved, trace=trace)
    elif family == "rollout_rows":
        rows_tests._rows_equal_single_steps(device, True, flags, series, length, F64, per_step=False, make_batch=carved, trace=trace)
    else:
        rows_tests._rows_equal_single_steps(device, False, flags, series, length, F64, normalized=normalized, action_dtype=F32,
                                            make_batch=carved, trace=trace)
    _replay(oracle, device, flags, series, trace, normalized=normalized)
