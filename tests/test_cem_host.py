"""The host side of CEM planning (mgx_cem / mgx_cem_refit): the draw and the candidate value as ``pymgrid_amd.policy`` states them in
torch (``cem_pair``, ``cem_candidates_host``, ``cem_refit_host``), ``cem_key``, the bindings and build lists, and the refusals of the
two C calls that need no device.  The launches themselves: tests/test_cem.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _dist(H=5, N=7, A=4, seed=0):
    """mean in [-0.2, 1.2] (the clip binds), sigma in (0.05, 0.4)."""
    g = torch.Generator(); g.manual_seed(seed)
    mean = torch.rand(H, N, A, generator=g, dtype=F64) * 1.4 - 0.2
    sigma = torch.rand(H, N, A, generator=g, dtype=F64) * 0.35 + 0.05
    return mean, sigma


def test_symbols_structs_and_units():
    """Both entry points are additions found by name: exported, declared, bound; the two structs have the header's fields and the C
    compiler's layout; the ABI minor stays 3; the new units are compiled (the launch in two slices) and hashed."""
    from pymgrid_amd import _lib
    _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "mgx.h")) as fh:
        header = fh.read()
    for name in ("mgx_lookahead_gaussian_episodes", "mgx_cem_refit"):
        assert getattr(L, name) is not None and name in _lib.SYMBOLS
        assert re.search(r"^int " + name + r"\(", header, re.M), name
    assert _lib.lib().mgx_abi_minor() == 3 == _lib.ABI_MINOR
    units = {u[0]: u for u in _lib.UNITS}
    assert units["mgx_lookahead_gaussian_episodes.hip"] == ("mgx_lookahead_gaussian_episodes.hip", "MGX_EPISODE_PART", 2)
    assert units["mgx_cem.hip"] == ("mgx_cem.hip", None, 1)
    for f in ("mgx_lookahead_gaussian_episodes.hip", "mgx_cem.hip", "mgx_cem.hpp"):
        assert os.path.join(ROOT, "pymgrid_amd", "csrc", f) in _lib.SOURCES
    for struct, cls in (("mgx_cem", _lib.Cem), ("mgx_cem_refit", _lib.CemRefit)):
        body = re.search(r"struct " + struct + r" \{(.*?)\n\}", header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n.strip(" *") for group in re.findall(r"^\s*(?:const\s+)?\w+\s+([\w, *]+);", body, re.M) for n in group.split(",")]
        assert names == [n for n, _ in cls._fields_], struct
    assert C.sizeof(_lib.Cem) == 32 and _lib.Cem.key.offset == 8 and _lib.Cem.mean.offset == 16
    assert C.sizeof(_lib.CemRefit) == 24 + 16 + 6 * 8 and _lib.CemRefit.alpha.offset == 24 and _lib.CemRefit.ret.offset == 40


def test_cem_kernels_spill_nothing():
    """Every instantiation of the launch (nine layouts with a control x three row sources) and of the small kernels: no scratch
    memory, no spilled vector registers, no LDS.  (Scalar registers parked in vector lanes are no memory traffic; the fixed-sequence
    logarithm, sine and cosine keep their constants in scalar registers, as in the Gaussian policy kernel.)"""
    from pymgrid_amd import _lib
    _lib.build()
    usage = _lib.resource_usage()
    if usage is None:
        pytest.skip("libmgx.so was not built on this machine (no resource_usage.json beside the objects)")
    for kernel, count in (("lookahead_gaussian_episodes_kernel", 9 * 3), ("cem_pick_kernel", 4), ("cem_refit_kernel", 4),
                          ("cem_elite_kernel", 1)):
        forms = {name: u for name, u in usage.items() if name.split("<")[0].split("::")[-1] == kernel}
        assert len(forms) == count, (kernel, sorted(forms))
        for name, u in forms.items():
            assert u.get("scratch", 0) == 0 and u.get("vgpr_spill", 0) == 0 and u.get("lds", 0) == 0, (name, u)


def test_pair_of_words_is_what_gaussian_pair_forms():
    """The split of ``gaussian_pair`` into the draw and "four words -> pair": the same pair as before from the Gaussian head's draw,
    and ``cem_pair`` is that arithmetic on the words of ``philox_words(key, i + (c << 32), k, CEM_TAG + p)``."""
    from pymgrid_amd import policy as P
    grid = torch.arange(50, dtype=torch.int64)
    r = P.philox_words(9, grid, 17, P.EXPLORE_TAG + P.GAUSS_DRAW + 1)
    a, b = P.gaussian_pair(9, grid, 17, 1), P.pair_of_words(r)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    u = P.gaussian_uniforms(9, grid, 17, 1)
    assert all(torch.equal(x, y) for x, y in zip(u, P.uniforms_of_words(r)))
    assert P.CEM_TAG == 0xCE300000
    z = P.cem_pair(5, grid, 3, 11, 1)
    w = P.pair_of_words(P.philox_words(5, grid + (3 << 32), 11, P.CEM_TAG + 1))
    assert torch.equal(z[0], w[0]) and torch.equal(z[1], w[1])


def test_candidates_follow_the_rule():
    from pymgrid_amd import cem_candidates_host
    from pymgrid_amd import policy as P
    H, N, A, Cn, key = 5, 7, 4, 6, 0x1234567890ABCDEF
    mean, sigma = _dist(H, N, A)
    sigma[:, :, 1] = 0.0                   # a dead column
    sigma[:, 2, 2] = -0.5                  # negative: dead
    sigma[:, 3, 3] = float("nan")          # NaN: dead
    x = cem_candidates_host(mean, sigma, Cn, key)
    assert x.shape == (Cn, H, N, A) and x.dtype == F64 and x.is_contiguous()
    clip = mean.clamp(0.0, 1.0)
    assert bool((mean < 0).any()) and bool((mean > 1).any())
    assert torch.equal(x[0], clip)                                         # candidate 0: the mean plan, clipped
    assert bool((x >= 0).all()) and bool((x <= 1).all())
    for dead in (x[:, :, :, 1], x[:, :, 2, 2], x[:, :, 3, 3]):           # a dead column equals the mean in every candidate
        assert torch.equal(dead, dead[0:1].expand_as(dead))
    # a live column, written out: clip(mean + sigma * z) with the pair of (key, i, c, k)
    i, c, k = 4, 5, 3
    z0, z1 = P.cem_pair(key, i, c, k, 1)
    v = mean[k, i, 2] + sigma[k, i, 2] * z0
    assert x[c, k, i, 2] == min(max(v, 0.0), 1.0)
    assert x[c, k, i, 3] == min(max(mean[k, i, 3] + sigma[k, i, 3] * z1, 0.0), 1.0)
    live = x[1:, :, :, 0]
    assert len(live.unique()) > 0.5 * live.numel()                         # ... and the candidates differ from each other
    # a function of (key, i, c, k, o) alone: subsets of grids and of candidates evaluated on their own
    sub = torch.tensor([5, 1, 6])
    assert torch.equal(cem_candidates_host(mean[:, sub].contiguous(), sigma[:, sub].contiguous(), Cn, key, grid=sub), x[:, :, sub])
    assert torch.equal(cem_candidates_host(mean, sigma, 3, key), x[:3])
    assert torch.equal(cem_candidates_host(mean, sigma, 2, key, first=4), x[4:])
    assert torch.equal(cem_candidates_host(mean[:2].contiguous(), sigma[:2].contiguous(), Cn, key), x[:, :2])
    # another key: other numbers on every live entry that the clip does not pin
    y = cem_candidates_host(mean, sigma, Cn, key + 1)
    assert torch.equal(y[0], x[0]) and not torch.equal(y[1:], x[1:])
    inside = (x[1:, :, :, 0] > 0) & (x[1:, :, :, 0] < 1)
    assert bool((y[1:, :, :, 0][inside] != x[1:, :, :, 0][inside]).all())
    # float32: the float64 values rounded once
    x32 = cem_candidates_host(mean, sigma, Cn, key, torch.float32)
    assert x32.dtype == torch.float32 and torch.equal(x32, x.to(torch.float32))
    # odd column counts leave half a pair unused: the columns they have are those of the wider distribution
    for a in (1, 2, 3):
        assert torch.equal(cem_candidates_host(mean[..., :a].contiguous(), sigma[..., :a].contiguous(), Cn, key), x[..., :a])
    for bad in ((mean.float(), sigma), (mean, sigma[:2]), (mean[0], sigma[0]), (torch.zeros(2, 3, 5, dtype=F64), torch.zeros(2, 3, 5, dtype=F64))):
        with pytest.raises(ValueError):
            cem_candidates_host(*bad, Cn, key)
    with pytest.raises(ValueError):
        cem_candidates_host(mean, sigma, 0, key)


def test_draws_are_standard_normal():
    """Key 1, N = 333, C = 8, H = 9, A = 4: the n = 95 904 draws behind the candidates are finite, distinct, of mean within
    5 / sqrt(n) of 0 and variance within 5 * sqrt(2 / n) of 1 (five standard errors of either estimate)."""
    from pymgrid_amd import policy as P
    N, Cn, H = 333, 8, 9
    grid = torch.arange(N, dtype=torch.int64).view(1, 1, N)
    cand = torch.arange(Cn, dtype=torch.int64).view(Cn, 1, 1)
    step = torch.arange(H, dtype=torch.int64).view(1, H, 1)
    z = torch.stack([t for p in range(2) for t in P.cem_pair(1, grid, cand, step, p)]).flatten()
    n = z.numel()
    assert n == 95904 and bool(z.isfinite().all()) and len(z.unique()) == n
    m, var = z.mean().item(), z.var(unbiased=False).item()
    print(f"mean {m:.3e} (bound {5 / math.sqrt(n):.4f}), |var - 1| {abs(var - 1):.3e} (bound {5 * math.sqrt(2 / n):.4f})")
    assert abs(m) < 5 / math.sqrt(n) and 5 / math.sqrt(n) < 0.0162
    assert abs(var - 1.0) < 5 * math.sqrt(2 / n) and 5 * math.sqrt(2 / n) < 0.0229


def test_refit_by_hand():
    """A case small enough for numpy: C = 4, H = 2, N = 3, A = 2, two elites; grid 1 stops after one step."""
    from pymgrid_amd import cem_candidates_host, cem_refit_host
    H, N, A, Cn, key, E = 2, 3, 2, 4, 77, 2
    mean, sigma = _dist(H, N, A, seed=3)
    ret = torch.tensor([[1.0, 5.0, 2.0], [4.0, 5.0, float("nan")], [4.0, 0.0, 3.0], [0.5, 6.0, 1.0]], dtype=F64)
    steps = torch.tensor([2, 1, 2], dtype=torch.int32)
    out = cem_refit_host(ret, steps, mean, sigma, key, E)
    # grid 0: 4.0 twice, the lower c first; grid 1: 6.0, then 5.0 twice, the lower c; grid 2: the NaN never replaces anything
    assert out["elite"].dtype == torch.int32 and out["elite"].tolist() == [[1, 3, 2], [2, 0, 0]]
    x = cem_candidates_host(mean, sigma, Cn, key).numpy()
    m_ref, s_ref = mean.numpy().copy(), sigma.numpy().copy()
    for i in range(N):
        for k in range(int(steps[i])):
            for o in range(A):
                xs = [x[int(out["elite"][e, i]), k, i, o] for e in range(E)]
                mu = (xs[0] + xs[1]) / 2.0
                m_ref[k, i, o] = mu
                s_ref[k, i, o] = ((xs[0] - mu) ** 2 + (xs[1] - mu) ** 2) / 2.0
    assert np.array_equal(out["mean"].numpy(), m_ref)
    assert np.allclose(out["sigma"].numpy()[0] ** 2, s_ref[0], rtol=1e-14, atol=0)          # (S is within 1 ulp of the root)
    assert torch.equal(out["mean"][1, 1], mean[1, 1]) and torch.equal(out["sigma"][1, 1], sigma[1, 1])   # k >= steps passes through
    assert not torch.equal(out["mean"][0, 1], mean[0, 1])
    best = torch.from_numpy(x)[out["elite"][0].long(), :, torch.arange(N)].permute(1, 0, 2)
    assert torch.equal(out["best_plan"], best)                                              # ... but best_plan holds every row


def test_refit_options():
    from pymgrid_amd import cem_candidates_host, cem_refit_host
    H, N, A, Cn, key = 4, 6, 3, 5, 12345
    mean, sigma = _dist(H, N, A, seed=5)
    g = torch.Generator(); g.manual_seed(8)
    ret = torch.randn(Cn, N, generator=g, dtype=F64)
    # all-equal returns: elites 0 .. E - 1
    same = cem_refit_host(torch.zeros(Cn, N, dtype=F64), None, mean, sigma, key, 3)
    assert same["elite"].tolist() == [[e] * N for e in range(3)]
    # elite[0] is the pick's best; the elites are distinct and in descending order of return
    full = cem_refit_host(ret, None, mean, sigma, key, Cn)
    assert torch.equal(full["elite"][0].long(), ret.argmax(dim=0))
    assert torch.equal(full["elite"].long().sort(dim=0).values, torch.arange(Cn).view(Cn, 1).expand(Cn, N))
    r = ret.gather(0, full["elite"].long())
    assert bool((r[:-1] >= r[1:]).all())
    # n_elite == C: the mean and deviation of all candidates, whatever the returns
    x = cem_candidates_host(mean, sigma, Cn, key)
    assert torch.allclose(full["mean"], x.mean(dim=0), rtol=1e-13, atol=1e-15)
    assert torch.allclose(full["sigma"], x.std(dim=0, unbiased=False), rtol=1e-9, atol=1e-12)
    # steps=None is steps == H
    hs = cem_refit_host(ret, torch.full((N,), H, dtype=torch.int32), mean, sigma, key, 2)
    none = cem_refit_host(ret, None, mean, sigma, key, 2)
    assert all(torch.equal(hs[k], none[k]) for k in hs)
    # alpha mixes the old distribution in, sigma_min floors the new sigma -- on the refitted rows only
    steps = torch.tensor([4, 1, 2, 3, 4, 1], dtype=torch.int32)
    fit = (torch.arange(H).view(H, 1) < steps.view(1, N)).unsqueeze(-1).expand(H, N, A)
    one = cem_refit_host(ret, steps, mean, sigma, key, 2)
    mix = cem_refit_host(ret, steps, mean, sigma, key, 2, alpha=0.25, sigma_min=0.2)
    assert torch.equal(mix["elite"], one["elite"]) and torch.equal(mix["best_plan"], one["best_plan"])
    assert torch.equal(mix["mean"], torch.where(fit, 0.25 * one["mean"] + 0.75 * mean, mean))
    sg = 0.25 * one["sigma"] + 0.75 * sigma
    assert torch.equal(mix["sigma"], torch.where(fit, torch.where(sg > 0.2, sg, torch.full_like(sg, 0.2)), sigma))
    assert bool((mix["sigma"][fit] >= 0.2).all()) and bool((mix["sigma"][fit] == 0.2).any()) and bool((sigma[~fit] < 0.2).any())
    keep = cem_refit_host(ret, steps, mean, sigma, key, 2, alpha=0.0)
    assert torch.equal(keep["mean"], mean + 0.0) and torch.equal(keep["sigma"], torch.where(fit, 0.0 * one["sigma"] + sigma, sigma))
    # one elite: its plan is the new mean, the deviation is zero (the floor)
    solo = cem_refit_host(ret, None, mean, sigma, key, 1, sigma_min=0.01)
    assert torch.equal(solo["mean"], solo["best_plan"]) and bool((solo["sigma"] == 0.01).all())
    # float32: the candidates rounded once before the sums
    f32 = cem_refit_host(ret, None, mean, sigma, key, 1, dtype=torch.float32)
    assert f32["best_plan"].dtype == torch.float32 and torch.equal(f32["best_plan"], solo["best_plan"].to(torch.float32))
    assert torch.equal(f32["mean"], f32["best_plan"].to(F64))
    nan = float("nan")
    for bad in (dict(n_elite=0), dict(n_elite=Cn + 1), dict(alpha=1.5), dict(alpha=-0.1), dict(alpha=nan), dict(sigma_min=-1.0),
                dict(sigma_min=nan), dict(ret=ret[:, :3]), dict(ret=ret.float()), dict(ret=ret[0]), dict(steps=steps[:2]),
                dict(steps=steps.long()), dict(mean=mean[:2]), dict(sigma=sigma.float())):
        kw = dict(ret=ret, steps=steps, mean=mean, sigma=sigma, key=key, n_elite=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            cem_refit_host(**kw)
    with pytest.raises(ValueError):
        cem_refit_host(torch.zeros(40, N, dtype=F64), None, mean, sigma, key, 33)          # more than 32 elites


def test_cem_key():
    """A function of its three arguments, 64 bits wide, formed in integer arithmetic on the host: the same on every device."""
    from pymgrid_amd import cem_key
    from pymgrid_amd import policy as P
    k = cem_key(3, 100, 2)
    assert isinstance(k, int) and 0 <= k < 2 ** 64 and k == cem_key(3, 100, 2)
    assert len({k, cem_key(4, 100, 2), cem_key(3, 101, 2), cem_key(3, 100, 1), cem_key(3, 100, 3)}) == 5
    keys = [cem_key(0, t, it) for t in range(40) for it in range(5)]
    assert len(set(keys)) == len(keys) and max(keys) >= 2 ** 63 > min(keys)          # (both halves of the range are reached)
    r = P.philox_words(3, 100, 2, 0xCE3F0000)
    assert k == int(r[0]) | int(r[1]) << 32
    if torch.cuda.is_available():
        rd = P.philox_words(3, 100, 2, 0xCE3F0000, device="cuda").cpu()
        assert torch.equal(rd, r)


def test_entry_points_refuse_without_a_device():
    """What needs no handle and no device is checked first: the structs, their sizes and pointers, C / H / n_elite / A / alpha /
    sigma_min.  Every text names the entry point."""
    from pymgrid_amd import _lib
    L = _lib.lib()
    buf = (C.c_double * 64)()
    ibuf = (C.c_int32 * 64)()
    p, ip = C.addressof(buf), C.addressof(ibuf)

    def cem(**kw):
        st = _lib.Cem()
        st.struct_size, st.key, st.mean, st.sigma = C.sizeof(_lib.Cem), 1, p, p
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    def la(**kw):
        st = _lib.Lookahead()
        st.struct_size, st.C, st.H, st.per_grid, st.gamma, st.ret = C.sizeof(_lib.Lookahead), 2, 4, 1, 1.0, p
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    def rf(**kw):
        st = _lib.CemRefit()
        st.struct_size, st.C, st.H, st.n_elite, st.alpha, st.sigma_min = C.sizeof(_lib.CemRefit), 4, 2, 2, 1.0, 0.0
        st.ret, st.elite, st.mean_out, st.sigma_out = p, ip, p, p
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    ref = lambda st: None if st is None else C.byref(st)      # noqa: E731
    nan = float("nan")
    name = b"mgx_lookahead_gaussian_episodes"
    for c, l, word in ((cem(), None, b"NULL la"), (cem(), la(struct_size=8), b"struct_size"), (cem(), la(ret=None), b"ret"),
                       (cem(), la(C=0), b"candidates"), (cem(), la(H=0), b"horizon"), (cem(), la(gamma=nan), b"gamma"),
                       (None, la(), b"NULL cem"), (cem(struct_size=24), la(), b"struct_size"), (cem(mean=None), la(), b"mean"),
                       (cem(sigma=None), la(), b"sigma"), (cem(), la(per_grid=0), b"per_grid"), (cem(), la(), b"NULL argument")):
        assert L.mgx_lookahead_gaussian_episodes(None, ref(c), ref(l), None) == _lib.MGX_ERR_INVALID, word
        err = L.mgx_last_error()
        assert name in err and word in err, err
    name = b"mgx_cem_refit"
    for n, a, c, r, word in ((3, 2, None, rf(), b"NULL cem"), (3, 2, cem(struct_size=0), rf(), b"struct_size"),
                             (3, 2, cem(mean=None), rf(), b"mean"), (3, 2, cem(), None, b"NULL refit"),
                             (3, 2, cem(), rf(struct_size=80), b"struct_size"), (3, 2, cem(), rf(ret=None), b"NULL"),
                             (3, 2, cem(), rf(elite=None), b"NULL"), (3, 2, cem(), rf(mean_out=None), b"NULL"),
                             (3, 2, cem(), rf(sigma_out=None), b"NULL"), (0, 2, cem(), rf(), b"positive"),
                             (3, 2, cem(), rf(C=0), b"positive"), (3, 2, cem(), rf(H=0), b"positive"),
                             (3, 2, cem(), rf(n_elite=0), b"n_elite"), (3, 2, cem(), rf(n_elite=5), b"n_elite"),
                             (3, 2, cem(), rf(C=40, n_elite=33), b"n_elite"), (3, 0, cem(), rf(), b"action columns"),
                             (3, 5, cem(), rf(), b"action columns"), (3, 2, cem(), rf(alpha=1.5), b"alpha"),
                             (3, 2, cem(), rf(alpha=-0.5), b"alpha"), (3, 2, cem(), rf(alpha=nan), b"alpha"),
                             (3, 2, cem(), rf(sigma_min=-0.1), b"sigma_min"), (3, 2, cem(), rf(sigma_min=nan), b"sigma_min")):
        assert L.mgx_cem_refit(n, a, ref(c), ref(r), None) == _lib.MGX_ERR_INVALID, word
        err = L.mgx_last_error()
        assert name in err and word in err, err
    assert L.mgx_cem_refit(2 ** 32 + 1, 2, ref(cem()), ref(rf()), None) == _lib.MGX_ERR_UNSUPPORTED
    assert b"2^32" in L.mgx_last_error()
