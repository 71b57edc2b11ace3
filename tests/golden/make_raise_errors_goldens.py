#!/usr/bin/env python3
"""Golden fixture for the requests the REFERENCE refuses with ``raise_errors=True`` (tests/golden/raise_errors.npz).

Run in the build container only (needs /root/reference):   python tests/golden/make_raise_errors_goldens.py

16 microgrids per module layout (F = 0, 1, 2, 3, 4, 5, 6, 7, 14, 15), built as real reference modules -- genset timers 0..3, both
initial genset states, lossless and lossy batteries, weak-grid rows (status 0) among the grid series -- take 24 steps.  Before every
step, every controllable module is copied, the copy gets ``raise_errors=True`` and is stepped with the module's request: the class of
what it raises (nothing, ValueError, AssertionError) is recorded, and for the battery and grid modules the normalised interval
[normalize(-max_consumption), normalize(max_production)] of that moment; the same copies are stepped under the raw control a random
priority list of the microgrid's DiscreteMicrogridEnv expands to at that moment (the list's id and the env's table are recorded;
every genset has a running_min_production above zero, so that the grids of a layout share one table).  Then the microgrid takes the
real step with ``raise_errors=False``.  Half of the grids take raw requests -- a third exactly AT the module's instantaneous limit, read from the
reference at that moment, a third one ``np.nextafter`` beyond it, a third uniform over 1.3 x the action range -- the other half
normalised ones, U[-0.15, 1.15).  A genset's goal stays in [0, 1) and its request at or above zero: beyond those the reference's own
step gives up with an AssertionError whatever ``raise_errors`` says, and the run could not go on.  Stored: parameters and initial state
(inputs); requests, exception classes, bounds and the state after the last step (outputs).  No reference source text.
"""
import json
import os
import sys
import warnings
from copy import deepcopy

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refenv  # noqa: E402

warnings.simplefilter("ignore")
_refenv.import_reference()

import make_goldens as mg  # noqa: E402
from pymgrid import Microgrid  # noqa: E402
from pymgrid.envs import DiscreteMicrogridEnv  # noqa: E402
from pymgrid.modules import BatteryModule, GensetModule, GridModule, LoadModule, RenewableModule  # noqa: E402

LAYOUTS = (0, 1, 2, 3, 4, 5, 6, 7, 14, 15)
N, T, STEPS = 16, 26, 24
NONE, VALUE_ERROR, ASSERTION_ERROR, ABSENT = 0, 1, 2, -1
AT_LIMIT, BEYOND, UNIFORM, NORMALISED = 0, 1, 2, 3
KINDS = (GensetModule, BatteryModule, GridModule)


def build(flags, j, rs):
    load = 20 + 60 * rs.rand(T)
    pv = 50 * rs.rand(T) * (rs.rand(T) > 0.3)
    mods = [("load", LoadModule(time_series=load)), ("pv", RenewableModule(time_series=pv))]
    ctrl = []
    if flags & 1:
        ctrl.append(("genset", GensetModule(running_min_production=float(rs.choice([3.0, 5.0, 12.0])), running_max_production=40.0 + 40 * rs.rand(),
                                            genset_cost=0.4, co2_per_unit=2.0, cost_per_unit_co2=0.1, start_up_time=j % 4,
                                            wind_down_time=(j // 4) % 4, init_start_up=bool(j % 2))))
    battery = ("battery", BatteryModule(min_capacity=10.0, max_capacity=60.0 + 80 * rs.rand(), max_charge=20.0 + 10 * rs.rand(),
                                        max_discharge=25.0, efficiency=float(rs.choice([0.9, 0.95, 1.0])),
                                        battery_cost_cycle=0.02, init_soc=0.3 + 0.6 * rs.rand()))
    status = (rs.rand(T) > (0.3 if j % 2 else 0.0)).astype(float)            # every other grid is weak: outages among its rows
    gts = np.stack([0.1 + rs.rand(T), 0.5 * rs.rand(T), 0.3 * rs.rand(T), status], axis=1)
    grid = ("grid", GridModule(max_import=30.0 + 40 * rs.rand(), max_export=20.0 + 30 * rs.rand(), time_series=gts, cost_per_unit_co2=0.1))
    both = [grid, battery] if flags & 8 else [battery, grid]
    ctrl += [m for m in both if (m[0] == "battery" and flags & 2) or (m[0] == "grid" and flags & 4)]
    return Microgrid(mods + ctrl, loss_load_cost=10.0, overgeneration_cost=1.0)


def limits(mod, goal):
    """(largest request accepted as a sink or None, largest accepted as a source) at this moment -- the genset's after its status
    followed ``goal``, as its step does first."""
    if isinstance(mod, GensetModule):
        c = deepcopy(mod)
        c.update_status(goal)
        return None, float(c.max_production)
    return float(mod.max_consumption), float(mod.max_production)


def draw(mod, raw, rs, k, j):
    """(request as Microgrid.run takes it, flat columns, how it was drawn)."""
    genset = isinstance(mod, GensetModule)
    goal = float(rs.rand()) if genset else None
    if not raw:
        x = float(rs.rand() * 1.15) if genset else float(rs.rand() * 1.3 - 0.15)
        how = NORMALISED
    else:
        how = (k + j) % 3
        sink, source = limits(mod, goal)
        as_sink = (not genset) and rs.rand() < 0.5
        if how == AT_LIMIT:
            x = -1 * sink if as_sink else source
        elif how == BEYOND:
            x = float(np.nextafter(-1 * sink, -np.inf)) if as_sink else float(np.nextafter(source, np.inf))
        else:
            lo, hi = (0.0, float(mod.running_max_production)) if genset else (float(mod.min_act), float(mod.max_act))
            x = lo + (hi - lo) * float(rs.rand() * 1.3 - (0.0 if genset else 0.15))
    return (np.array([goal, x]) if genset else float(x)), ([goal, x] if genset else [x]), how


def dry_run(mod, request, normalized):
    c = deepcopy(mod)
    c.raise_errors = True
    try:
        c.step(request, normalized=normalized)
    except ValueError:
        return VALUE_ERROR
    except AssertionError:
        return ASSERTION_ERROR
    return NONE


def list_dry_run(m, rs):
    """A random priority list of the microgrid's discrete env, expanded by the reference at this moment: (list id, the exception class
    of every controllable module's copy stepped with ``raise_errors=True`` under the expanded raw control, the env's table)."""
    env = DiscreteMicrogridEnv.from_microgrid(deepcopy(m))
    table = -np.ones((env.action_space.n, 3, 2), np.int32)
    for i, pl in enumerate(env.actions_list):
        for j, el in enumerate(pl):
            table[i, j] = (KINDS.index(type(env.modules[el.module[0]][el.module[1]])), el.action)
    a = int(rs.randint(env.action_space.n))
    exc = np.full(3, ABSENT, np.int8)
    try:
        ctrl = env._get_action(a)
    except AssertionError:
        exc[[q for q, cls in enumerate(KINDS) if mg.find(m, cls)]] = ASSERTION_ERROR
        return a, exc, table
    for q, cls in enumerate(KINDS):
        if mg.find(m, cls):
            v = ctrl[mg.mod_name(env, cls)][0]
            exc[q] = dry_run(mg.find(m, cls)[0], np.asarray(v, dtype=np.float64) if q == 0 else float(v), False)
    return a, exc, table


def main():
    out, meta = {}, []
    for flags in LAYOUTS:
        rs = np.random.RandomState(9000 + flags)
        A = 2 * (flags & 1) + ((flags >> 1) & 1) + ((flags >> 2) & 1)
        req = np.zeros((STEPS, N, A))
        exc = np.full((STEPS, N, 3), ABSENT, np.int8)
        how = np.full((STEPS, N, 3), ABSENT, np.int8)
        bounds = np.full((STEPS, N, 2, 2), np.nan)
        ids, list_exc, table = np.zeros((STEPS, N), np.int32), np.full((STEPS, N, 3), ABSENT, np.int8), None
        charge, soc, status = np.full(N, np.nan), np.full(N, np.nan), np.zeros((N, 4), np.int32)
        for j in range(N):
            m = build(flags, j, rs)
            raw = j < N // 2
            p = mg.extract_params(m)
            p["controllable_order"] = [{GensetModule: "genset", BatteryModule: "battery", GridModule: "grid"}[type(lst[0])]
                                       for _, lst in m.controllable.iterdict()]
            scalars, arrays = mg.split_params(p)
            scalars.update(layout=flags, index=j, raw=bool(raw))
            meta.append(scalars)
            for name, v in arrays.items():
                out[f"f{flags}_g{j}_{name}"] = v
            for k in range(STEPS):
                row = []
                for q, cls in enumerate(KINDS):                   # the columns of a control row: genset (goal, energy), battery, grid
                    mods = mg.find(m, cls)
                    if not mods:
                        continue
                    request, cols, how[k, j, q] = draw(mods[0], raw, rs, k, j)
                    exc[k, j, q] = dry_run(mods[0], request, not raw)
                    if q:
                        space = mods[0]._action_space
                        bounds[k, j, q - 1] = (space.normalize(-1 * mods[0].max_consumption), space.normalize(mods[0].max_production))
                    row += cols
                req[k, j] = row
                if A:                                             # (the reference builds no discrete env without a controllable module)
                    ids[k, j], list_exc[k, j], tab = list_dry_run(m, rs)
                    assert table is None or np.array_equal(table, tab)
                    table = tab
                m.run(mg.control_from_row(m, p, np.array(row)), normalized=not raw)
            charge[j], soc[j], status[j] = mg.post_state(m)
        # the conditions a test re-asserts from the file
        for q, cls in enumerate(KINDS):
            if (exc[..., q] == ABSENT).all():
                continue
            refused = exc[..., q] == VALUE_ERROR
            assert 0.2 <= refused.mean() <= 0.8, (flags, cls.__name__, refused.mean())
            assert not refused[how[..., q] == AT_LIMIT].any(), (flags, cls.__name__, "a request at the limit was refused")
            assert refused[how[..., q] == BEYOND].all(), (flags, cls.__name__, "a request one ulp beyond the limit was accepted")
        print(f"layout {flags}: refused " + ", ".join(f"{cls.__name__} {np.mean(exc[..., q] == VALUE_ERROR):.2f}" for q, cls in enumerate(KINDS)
                                                      if not (exc[..., q] == ABSENT).all()),
              f"assertion errors {int((exc == ASSERTION_ERROR).sum())}")
        out.update({f"f{flags}_requests": req, f"f{flags}_exception": exc, f"f{flags}_how": how, f"f{flags}_bounds": bounds,
                    f"f{flags}_ids": ids, f"f{flags}_list_exception": list_exc,
                    f"f{flags}_table": table if table is not None else -np.ones((1, 3, 2), np.int32), f"f{flags}_charge": charge, f"f{flags}_soc": soc, f"f{flags}_status": status})
    out["meta"] = np.array(json.dumps(meta))
    mg.save("raise_errors.npz", **out)


if __name__ == "__main__":
    main()
