"""The refusals of the single-step, K-step and fleet calls of the C ABI, pinned by return code AND exact ``mgx_last_error()`` text.

One table: (name, counter value the handles stand at, the call, expected code, expected text).  Every row is a call that is
refused before anything is launched, made through the ctypes binding directly (the Python wrappers refuse several of them first);
the texts are those of pymgrid_amd/csrc/mgx_abi.hip.  Three handles of N = 70 grids (one full wave and a partial one) over T = 24
rows: ``a`` genset + battery + grid with one module of every kind (an env plan with a priority-list table bound), ``m`` the same
with three gensets (beyond the register form: mgx_step_lists takes two launches), ``e`` stepping in-place episodes with
mgx_set_final_obs set."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, T = 70, 24
INVALID, UNSUPPORTED, RANGE = 1, 2, 3


def _outside(who, t=T):
    return f"{who}: step {t} is outside the time series (length {T})"


def _leave(who, t=T - 1, K=2):
    return f"{who}: steps [{t}, {t + K}) leave the time series (length {T})"


def _need_lists(who):
    return f"{who}: need n_lists > 0 and list_len in [1, 24]"


def _items(c, n, **fields):
    """n fleet items on handle ``a`` with continuous actions, ``fields`` set on every one of them"""
    from pymgrid_amd import _lib
    items = (_lib.FleetItem * n)()
    for it in items:
        it.struct_size = C.sizeof(_lib.FleetItem)
        it.handle, it.actions, it.reward = c.a, c.act, c.rew
        for k, v in fields.items():
            setattr(it, k, v)
    return items


def _fleet(c, items, n=None):
    return c.lib.mgx_fleet_step(items, len(items) if n is None else n, 0, None)


def _fleet_env(c, handles):
    hs = (C.c_void_p * len(handles))(*handles)
    ptrs = (C.c_void_p * len(handles))(*([c.act] * len(handles)))
    return c.lib.mgx_fleet_env_step(hs, ptrs, len(handles), 0, None)


# (name, counter value of `a` and `m`, call, code, text)
ROWS = [
    # ---- K > 1 would leave the series: the handles stand at the last row ----
    ("step_many leaves", T - 1, lambda c: c.lib.mgx_step_many(c.a, c.act, 2, 0, c.rew, None, None, None, None), RANGE, _leave("mgx_step_many")),
    ("step_k leaves", T - 1, lambda c: c.lib.mgx_step_k(c.a, c.act, 2, 0, c.rew, None, None, None, None, None, None), RANGE, _leave("mgx_step_k")),
    ("rollout_discrete leaves", T - 1,
     lambda c: c.lib.mgx_rollout_discrete(c.a, c.ids8, 0, c.tab, c.n_tab, 2, c.rew, None, None, None, None, None, None), RANGE,
     _leave("mgx_rollout_discrete")),
    ("rollout_lists leaves", T - 1,
     lambda c: c.lib.mgx_rollout_lists(c.m, c.ids, 0, c.lists, 1, 1, 2, c.rew, None, None, None, None, None, None), RANGE,
     _leave("mgx_rollout_lists")),
    # ---- the checks around the range check keep their order ----
    ("step_many K = 0", T - 1, lambda c: c.lib.mgx_step_many(c.a, c.act, 0, 0, c.rew, None, None, None, None), INVALID,
     "mgx_step_many: K must be positive"),
    ("step_many no reward", T - 1, lambda c: c.lib.mgx_step_many(c.a, c.act, 2, 0, None, None, None, None, None), INVALID,
     "mgx_step_many: NULL argument"),
    ("step_k K = 0", T - 1, lambda c: c.lib.mgx_step_k(c.a, c.act, 0, 0, c.rew, None, None, None, None, None, None), INVALID,
     "mgx_step_k: K must be positive"),
    ("rollout_discrete K = 0", T - 1,
     lambda c: c.lib.mgx_rollout_discrete(c.a, c.ids8, 0, c.tab, c.n_tab, 0, c.rew, None, None, None, None, None, None), INVALID,
     "mgx_rollout_discrete: K must be positive"),
    ("rollout_discrete on several of a kind", T - 1,
     lambda c: c.lib.mgx_rollout_discrete(c.m, c.ids8, 0, c.tab, c.n_tab, 2, c.rew, None, None, None, None, None, None), UNSUPPORTED,
     "mgx_rollout_discrete: needs exactly one module of every kind per grid; use mgx_expand_discrete / mgx_expand_lists + mgx_step"),
    # ---- the list arguments (refused before the range: K = 2 at the last row) ----
    ("expand_lists n_lists = 0", T - 1, lambda c: c.lib.mgx_expand_lists(c.m, c.ids, c.lists, 0, 1, c.ctl, None, None), INVALID,
     _need_lists("mgx_expand_lists")),
    ("step_lists list_len = 25", T - 1, lambda c: c.lib.mgx_step_lists(c.m, c.ids, c.lists, 1, 25, c.ctl, c.rew, None, None, None, None),
     INVALID, _need_lists("mgx_step_lists")),
    ("rollout_lists list_len = 0", T - 1,
     lambda c: c.lib.mgx_rollout_lists(c.m, c.ids, 0, c.lists, 1, 0, 2, c.rew, None, None, None, None, None, None), INVALID,
     _need_lists("mgx_rollout_lists")),
    ("rollout_lists K = 0 before the lists", T - 1,
     lambda c: c.lib.mgx_rollout_lists(c.m, c.ids, 0, c.lists, 0, 0, 0, c.rew, None, None, None, None, None, None), INVALID,
     "mgx_rollout_lists: K must be positive"),
    ("step_lists needs the control buffer", T - 1,
     lambda c: c.lib.mgx_step_lists(c.m, c.ids, c.lists, 1, 1, None, c.rew, None, None, None, None), INVALID,
     "mgx_step_lists: this layout steps in two launches and needs the control buffer [N, A]"),
    # ---- mgx_fleet_step ----
    ("fleet 65 items", T - 1, lambda c: _fleet(c, _items(c, 65)), INVALID, "mgx_fleet_step: at most 64 items per call"),
    ("fleet no items", T - 1, lambda c: _fleet(c, _items(c, 1), 0), INVALID, "mgx_fleet_step: no items"),
    ("fleet repeated handle", T - 1, lambda c: _fleet(c, _items(c, 2)), INVALID, "mgx_fleet_step: item 1 steps the batch of item 0 again"),
    ("fleet action_id without table", T - 1, lambda c: _fleet(c, _items(c, 1, action_id=c.ids)), INVALID, "mgx_fleet_step: item 0: NULL table"),
    ("fleet refill_K = 0", T - 1, lambda c: _fleet(c, _items(c, 1, refill_ring=c.ring, refill_K=0, refill_ahead=1)), INVALID,
     "mgx_fleet_step: item 0: bad refill_K / refill_ahead / refill_chunk(s)"),
    ("fleet refill chunk past chunks", T - 1,
     lambda c: _fleet(c, _items(c, 1, refill_ring=c.ring, refill_K=4, refill_ahead=1, refill_chunk=2, refill_chunks=2)), INVALID,
     "mgx_fleet_step: item 0: bad refill_K / refill_ahead / refill_chunk(s)"),
    ("fleet chunks with ahead = 0", T - 1,
     lambda c: _fleet(c, _items(c, 1, refill_ring=c.ring, refill_K=4, refill_ahead=0, refill_chunk=0, refill_chunks=2)), INVALID,
     "mgx_fleet_step: item 0: bad refill_K / refill_ahead / refill_chunk(s)"),
    ("fleet final_obs without obs", T - 1, lambda c: _fleet(c, _items(c, 1, handle=c.e)), INVALID,
     "mgx_fleet_step: item 0: mgx_set_final_obs is set but the step writes no observation"),
    ("fleet struct_size", T - 1, lambda c: _fleet(c, _items(c, 1, struct_size=8)), INVALID, "mgx_fleet_step: item 0 struct_size 8 vs 104"),
    # ---- mgx_fleet_env_step ----
    ("fleet_env unbound handle", T - 1, lambda c: _fleet_env(c, [c.m]), INVALID, "mgx_fleet_env_step: handle 0 has no plan bound (mgx_env_bind)"),
    ("fleet_env unbound behind a bound one", T - 1, lambda c: _fleet_env(c, [c.a, c.m]), INVALID,
     "mgx_fleet_env_step: handle 1 has no plan bound (mgx_env_bind)"),
    ("fleet_env repeated handle", T - 1, lambda c: _fleet_env(c, [c.a, c.a]), INVALID, "mgx_fleet_env_step: handle 1 is handle 0 again"),
    ("fleet_env 65 handles", T - 1, lambda c: _fleet_env(c, [c.a] * 65), INVALID, "mgx_fleet_env_step: n_handles = 65 outside [1, 64]"),
    # ---- K = 1 outside the series: the handles stand behind the last row ----
    ("step outside", T, lambda c: c.lib.mgx_step(c.a, c.act, 0, c.rew, None, None, None, None), RANGE, _outside("mgx_step")),
    ("check_step outside", T, lambda c: c.lib.mgx_check_step(c.a, c.act, 0, c.viol, None), RANGE, _outside("mgx_check_step")),
    ("action_bounds outside", T, lambda c: c.lib.mgx_action_bounds(c.a, c.ctl, c.ctl2, None), RANGE, _outside("mgx_action_bounds")),
    ("expand_discrete outside", T, lambda c: c.lib.mgx_expand_discrete(c.a, c.ids, c.tab, c.n_tab, c.ctl, None, None), RANGE,
     _outside("mgx_expand_discrete")),
    ("expand_lists outside", T, lambda c: c.lib.mgx_expand_lists(c.m, c.ids, c.lists, 1, 1, c.ctl, None, None), RANGE,
     _outside("mgx_expand_lists")),
    ("check_discrete outside", T, lambda c: c.lib.mgx_check_discrete(c.a, c.ids, c.tab, c.n_tab, c.viol, None), RANGE,
     _outside("mgx_check_discrete")),
    ("step_discrete outside", T, lambda c: c.lib.mgx_step_discrete(c.a, c.ids, c.tab, c.n_tab, None, c.rew, None, None, None, None), RANGE,
     _outside("mgx_step_discrete")),
    ("step_lists outside", T, lambda c: c.lib.mgx_step_lists(c.m, c.ids, c.lists, 1, 1, c.ctl, c.rew, None, None, None, None), RANGE,
     _outside("mgx_step_lists")),
    ("step_many K = 1 outside", T, lambda c: c.lib.mgx_step_many(c.a, c.act, 1, 0, c.rew, None, None, None, None), RANGE,
     _outside("mgx_step_many")),
    ("env_step outside", T, lambda c: c.lib.mgx_env_step(c.a, c.act, 0, None), RANGE, _outside("mgx_env_step")),
    ("env_step_discrete outside", T, lambda c: c.lib.mgx_env_step_discrete(c.a, c.ids, None), RANGE, _outside("mgx_env_step_discrete")),
    ("fleet outside", T, lambda c: _fleet(c, _items(c, 1)), RANGE, _outside("mgx_fleet_step")),
    ("fleet_env outside", T, lambda c: _fleet_env(c, [c.a]), RANGE, _outside("mgx_fleet_step")),
    ("step_k K = 1 outside", T, lambda c: c.lib.mgx_step_k(c.a, c.act, 1, 0, c.rew, None, None, None, None, None, None), RANGE,
     _leave("mgx_step_k", T, 1)),
    # ... and the list arguments still go first
    ("expand_lists list_len = 0 outside", T, lambda c: c.lib.mgx_expand_lists(c.m, c.ids, c.lists, 1, 0, c.ctl, None, None), INVALID,
     _need_lists("mgx_expand_lists")),
]


def test_refusals_keep_their_code_and_text(device):
    from pymgrid_amd import StepEngine, _lib
    from pymgrid_amd.generator import generate, widen
    from pymgrid_amd.priority_list import get_priority_lists, table_array
    mk = lambda: generate(N, n_steps=T, seed=3, arch="genset+battery+grid", device=device)
    ea, em, ee = StepEngine(mk()), StepEngine(widen(mk(), n_genset=3)), StepEngine(mk())
    f64 = dict(dtype=torch.float64, device=device)
    A = max(ea.action_dim, em.action_dim)
    keep = dict(act=torch.rand(N, A, **f64), rew=torch.empty(2, N, **f64), ctl=torch.empty(N, A, **f64), ctl2=torch.empty(N, A, **f64),
                ids=torch.zeros(N, dtype=torch.int32, device=device), ids8=torch.zeros(2, N, dtype=torch.uint8, device=device),
                viol=torch.zeros(N, dtype=torch.int32, device=device), lists=torch.zeros(1, 1, 3, dtype=torch.int32, device=device),
                ring=torch.empty(4, N, ea.obs_dim, **f64), fin=torch.empty(N, ee.obs_dim, **f64),
                done=torch.empty(N, dtype=torch.uint8, device=device))
    table = np.ascontiguousarray(table_array(get_priority_lists(True, True, True)), dtype=np.int32)
    c = SimpleNamespace(lib=_lib.lib(), a=ea._h.value, m=em._h.value, e=ee._h.value, tab=table.ctypes.data_as(_lib.c_i32_p),
                        n_tab=table.shape[0], **{k: v.data_ptr() for k, v in keep.items()})
    # `a` walks one rotating output slot by itself (mgx_env_bind), continuous and discrete actions alike
    slot = (_lib.EnvSlot * 1)()
    slot[0].reward, slot[0].done = c.rew, c.done
    plan = _lib.EnvPlan()
    plan.struct_size, plan.n_slots, plan.slots, plan.n_actions, plan.table = C.sizeof(_lib.EnvPlan), 1, slot, c.n_tab, c.tab
    _lib.check(c.lib.mgx_env_bind(c.a, C.byref(plan)))
    # `e` steps in-place episodes and is asked for the row before a restart
    ee.reset_episodes(torch.zeros(N, dtype=torch.int32, device=device), None, max_length=8, want_obs=False)
    ee.set_final_obs(keep["fin"])
    at = None
    bad = []
    for name, t, call, code, text in ROWS:
        if t != at:                                            # the counters of `a` and `m`: set by a reset, nothing is stepped
            assert t in (T - 1, T)
            for eng in (ea, em):
                eng.reset(T - 1, want_obs=False)
            if t == T:                                         # behind the last row: one (accepted) step from it
                for eng in (ea, em):
                    eng.step(torch.rand(N, eng.action_dim, **f64), want_obs=False)
            at = t
        before = (ea.current_step, em.current_step, c.lib.mgx_current_step(c.a), c.lib.mgx_current_step(c.m), c.lib.mgx_current_step(c.e))
        rc = call(c)
        got = c.lib.mgx_last_error().decode()
        after = (ea.current_step, em.current_step, c.lib.mgx_current_step(c.a), c.lib.mgx_current_step(c.m), c.lib.mgx_current_step(c.e))
        if (rc, got) != (code, text) or before != after:
            bad.append((name, rc, got, before, after))
    torch.cuda.synchronize(device)
    assert not bad, "\n".join(f"{n}: code {rc}, text {got!r}, counters {b} -> {a}" for n, rc, got, b, a in bad)
    assert len({r[0] for r in ROWS}) == len(ROWS)
    c.lib.mgx_env_bind(c.a, None)
    ea.close(); em.close(); ee.close()
