"""The host side of the what-if roll-outs (mgx_lookahead_episodes / mgx_lookahead_step_k_episodes): symbols, bindings and build
lists, the kernels' register figures, ``lookahead_host`` against a scalar loop, ``ShootingMPC``'s default candidate set and the
refusals that need no device.  The launches themselves: tests/test_lookahead.py."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mgx_lookahead_episodes", "mgx_lookahead_step_k_episodes")
UNITS = ("mgx_lookahead_episodes.hip", "mgx_lookahead_step_episodes.hip")


def test_symbols_are_exported_declared_and_bound_and_the_minor_stays():
    """Both entry points are additions found by name: exported, declared in the header, bound; ``Lookahead`` has the header's size;
    the ABI minor stays 3 and the tunables stay twelve; both units are compiled (two slices each) and hashed."""
    from pymgrid_amd import _lib
    _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "mgx.h")) as fh:
        header = fh.read()
    for name in SYMBOLS:
        assert getattr(L, name) is not None
        assert name in _lib.SYMBOLS
        assert re.search(r"^int " + name + r"\(", header, re.M), name
    assert _lib.lib().mgx_abi_minor() == 3 == _lib.ABI_MINOR
    assert len(_lib.TUNABLES) == 12
    units = {u[0]: u for u in _lib.UNITS}
    for f in UNITS:
        assert units[f] == (f, "MGX_EPISODE_PART", 2)
        assert os.path.join(ROOT, "pymgrid_amd", "csrc", f) in _lib.SOURCES
    assert os.path.join(ROOT, "pymgrid_amd", "csrc", "mgx_lookahead.hpp") in _lib.SOURCES
    # the struct of the header, field by field, under the C compiler's layout rules (int32 x 4, double, six pointers)
    body = re.search(r"typedef struct mgx_lookahead \{(.*?)\} mgx_lookahead;", header, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|double|void)\s+(\*?)\s*([\w, ]+);", body, re.M)
    names = [n.strip() for _, _, group in fields for n in group.split(",")]
    assert names == [n for n, _ in _lib.Lookahead._fields_]
    assert C.sizeof(_lib.Lookahead) == 4 * 4 + 8 + 6 * C.sizeof(C.c_void_p) == 72
    assert _lib.Lookahead.gamma.offset == 16 and _lib.Lookahead.ret.offset == 24 and _lib.Lookahead.first_action.offset == 64


def test_lookahead_kernels_spill_nothing():
    """Every instantiation of both kernels: no scratch memory, no spilled scalar or vector registers.  Discrete: ten layouts x
    shared / per-grid plans x three row sources; continuous: those x float64 / float32 controls."""
    from pymgrid_amd import _lib
    _lib.build()
    usage = _lib.resource_usage()
    if usage is None:
        pytest.skip("libmgx.so was not built on this machine (no resource_usage.json beside the objects)")
    for kernel, count in (("lookahead_episodes_kernel", 10 * 2 * 3), ("lookahead_step_k_episodes_kernel", 10 * 2 * 3 * 2)):
        forms = {name: u for name, u in usage.items() if name.split("<")[0].split("::")[-1] == kernel}
        assert len(forms) == count, (kernel, sorted(forms))
        for name, u in forms.items():
            assert u.get("scratch", 0) == 0 and u.get("vgpr_spill", 0) == 0 and u.get("sgpr_spill", 0) == 0, (name, u)
        # no LDS beyond the id-word table of the per-grid discrete form (256 words)
        for name, u in forms.items():
            per_grid_ids = kernel == "lookahead_episodes_kernel" and ", true," in name
            assert u.get("lds", 0) == (1024 if per_grid_ids else 0), (name, u)


def _scalar_rule(reward, done, gamma):
    """The rule of include/mgx.h, one grid and one candidate at a time in Python floats (IEEE doubles)."""
    Cn, H, N = len(reward), len(reward[0]), len(reward[0][0])
    ret = [[0.0] * N for _ in range(Cn)]
    steps = [0] * N
    for i in range(N):
        for c in range(Cn):
            w, acc, n = 1.0, 0.0, 0
            for k in range(H):
                acc = acc + w * reward[c][k][i]
                w = w * gamma
                n += 1
                if done[k][i]:
                    break
            ret[c][i], steps[i] = acc, n
    best, best_ret = [0] * N, [0.0] * N
    for i in range(N):
        b = 0
        for c in range(1, Cn):
            if ret[c][i] > ret[b][i]:
                b = c
        best[i], best_ret[i] = b, ret[b][i]
    return ret, steps, best, best_ret


@pytest.mark.parametrize("gamma", [1.0, 0.9, 0.0])
@pytest.mark.parametrize("n_cand", [1, 4])
def test_lookahead_host_is_the_scalar_rule(gamma, n_cand):
    """Hand-made rewards [C, H, N]: grids whose episode ends at step 0, in the middle, at H - 1 and nowhere; candidate 2 a copy of
    candidate 0 (equal returns: the lower index wins) and one grid on which a later candidate is strictly better; C = 1."""
    from pymgrid_amd import lookahead_host
    H, N = 6, 8
    g = torch.Generator(); g.manual_seed(100 + n_cand)
    reward = (torch.rand(n_cand, H, N, generator=g, dtype=torch.float64) - 0.7) * 37.0
    done = torch.zeros(H, N, dtype=torch.bool)
    done[0, 0] = True                      # grid 0: its first step ends the episode
    done[2, 1] = True                      # grid 1: in the middle
    done[H - 1, 2] = True                  # grid 2: the last step of the horizon
    done[1, 3] = True; done[2:, 3] = True  # grid 3: walks on with done set (no auto-reset): counted to the first flag
    done[3, 4] = True; done[5, 4] = True   # grid 4: a second flag belongs to the episode after the restart
    if n_cand > 1:
        reward[2] = reward[0]
        reward[3, :, 5] = reward[:3, :, 5].abs().max() + 1.0      # grid 5: candidate 3 beats all (positive rewards, gamma aside)
        reward[:3, 0, 5] = -1.0
    out = lookahead_host(reward, done, gamma)
    ret, steps, best, best_ret = _scalar_rule(reward.tolist(), done.tolist(), gamma)
    assert out["ret"].dtype == torch.float64 and torch.equal(out["ret"], torch.tensor(ret, dtype=torch.float64))
    assert out["steps"].dtype == torch.int32 and out["steps"].tolist() == steps == [1, 3, 6, 2, 4, 6, 6, 6]
    assert out["last"].tolist() == [s - 1 for s in steps]
    assert out["best"].dtype == torch.int32 and out["best"].tolist() == best
    assert torch.equal(out["best_ret"], torch.tensor(best_ret, dtype=torch.float64))
    if n_cand > 1:
        assert 2 not in best and best[5] == 3 and 0 in best
    else:
        assert best == [0] * N and torch.equal(out["best_ret"], out["ret"][0])
    # done as the bytes a launch writes
    again = lookahead_host(reward, done.to(torch.uint8), gamma)
    assert all(torch.equal(again[k], out[k]) for k in out)
    if gamma == 0.0:                       # only step 0 counts
        assert torch.equal(out["ret"], reward[:, 0] + 0.0)


def test_lookahead_host_refuses_what_is_not_the_rule():
    from pymgrid_amd import lookahead_host
    r, d = torch.zeros(2, 3, 4, dtype=torch.float64), torch.zeros(3, 4, dtype=torch.bool)
    for bad in ((r[0], d, 1.0), (r, d[:2], 1.0), (r.float(), d, 1.0), (r, d, 1.5), (r, d, -0.5), (r, d, float("nan"))):
        with pytest.raises(ValueError):
            lookahead_host(*bad)


def test_default_discrete_candidates():
    """``shooting_candidates`` (ShootingMPC's default discrete set): [n + R, H] uint8, the constant block exact, the random block a
    function of (seed, counter) only and inside the table."""
    from pymgrid_amd import shooting_candidates
    n, H, R = 6, 24, 32
    p = shooting_candidates(n, H, R, seed=7, counter=100)
    assert p.shape == (n + R, H) and p.dtype == torch.uint8 and p.is_contiguous()
    assert torch.equal(p[:n], torch.arange(n, dtype=torch.uint8).view(n, 1).expand(n, H))
    assert int(p[n:].max()) < n and len(p[n:].unique()) == n
    assert torch.equal(p, shooting_candidates(n, H, R, seed=7, counter=100))
    assert not torch.equal(p[n:], shooting_candidates(n, H, R, seed=7, counter=101)[n:])
    assert not torch.equal(p[n:], shooting_candidates(n, H, R, seed=8, counter=100)[n:])
    assert shooting_candidates(n, H).shape == (n, H)
    assert torch.equal(shooting_candidates(n, H, 0, seed=3, counter=9), p[:n])
    for bad in ((0, H, 0), (257, H, 0), (n, 0, 0), (n, H, -1)):
        with pytest.raises(ValueError):
            shooting_candidates(*bad)


def test_entry_points_refuse_without_a_device():
    """What needs no handle is checked first and before any device is touched: a NULL la, a wrong struct_size, a NULL ret, C or H
    below 1, a gamma outside [0, 1]; then the NULL handle / plans.  Every text names the entry point."""
    from pymgrid_amd import _lib
    L = _lib.lib()
    buf = (C.c_double * 8)()
    ids = (C.c_uint8 * 8)()
    table = (C.c_int32 * 6)()

    def la(**kw):
        st = _lib.Lookahead()
        st.struct_size, st.C, st.H, st.gamma, st.ret = C.sizeof(_lib.Lookahead), 2, 4, 1.0, C.addressof(buf)
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    calls = ((b"mgx_lookahead_episodes", lambda h, plans, st: L.mgx_lookahead_episodes(h, plans, table, 1, st, None)),
             (b"mgx_lookahead_step_k_episodes", lambda h, plans, st: L.mgx_lookahead_step_k_episodes(h, plans, 1, st, None)))
    for name, call in calls:
        for st, word in ((None, b"NULL la"), (la(struct_size=C.sizeof(_lib.Lookahead) - 8), b"struct_size"), (la(ret=None), b"ret"),
                         (la(C=0), b"candidates"), (la(H=0), b"horizon"), (la(gamma=1.25), b"gamma"), (la(gamma=-0.5), b"gamma"),
                         (la(gamma=float("nan")), b"gamma"), (la(), b"NULL argument")):
            assert call(None, C.cast(ids, C.c_void_p), None if st is None else C.byref(st)) == _lib.MGX_ERR_INVALID, (name, word)
            err = L.mgx_last_error()
            assert name in err and word in err, err
