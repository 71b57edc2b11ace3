"""The Gaussian policy head of the fused continuous K-step (mgx_step_k_policy_gaussian_episodes) on the host: the rule of
``mgx_gaussian`` (include/mgx.h) as ``pymgrid_amd.policy`` states it -- ``policy_log``, ``policy_quarter_turn``, ``gaussian_pair`` and
``MLPPolicy.act(obs, GaussianSampling, counter)`` -- against libm, against the moments of a standard normal, against the textbook
log-density, and every refusal of the C entry that needs no handle.  Nothing here needs a GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from test_policy_rollout import _policy

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def _gs(seed=5, sigma=0.2, **kw):
    from pymgrid_amd import GaussianSampling
    return GaussianSampling(seed, sigma, **kw)


def _rows(n, n_in, seed=3):
    return torch.as_tensor(np.random.default_rng(seed).uniform(0.0, 1.0, size=(n, n_in)))


def _ulps(got, ref):
    """|got - ref| in units of the spacing of doubles at ref."""
    spacing = (torch.nextafter(ref.abs(), torch.full_like(ref, float("inf"))) - ref.abs())
    return (got - ref).abs() / spacing


# ---- the three functions of the rule against libm ------------------------------------------------------------------------------------
def test_policy_log_stays_within_four_ulp_of_log():
    """(0, 1] -- the radius' argument, its corners 1, 2^-53, 1 - 2^-53 forced -- and 10^+-300; the worst case is printed (NOTES.md
    records it).  A wrong coefficient costs thousands of ulp."""
    from pymgrid_amd.policy import policy_log
    g = torch.Generator().manual_seed(1)
    u = torch.cat([1.0 - torch.rand(400_000, dtype=F64, generator=g), torch.tensor([1.0, 2.0 ** -53, 1.0 - 2.0 ** -53], dtype=F64)])
    wide = 10.0 ** (torch.rand(400_000, dtype=F64, generator=g) * 600.0 - 300.0)
    for name, a in (("(0, 1]", u), ("1e-300 .. 1e300", wide)):
        got, ref = policy_log(a), torch.log(a)
        assert got.dtype == F64 and got.shape == a.shape
        nz = ref != 0
        worst = float(_ulps(got[nz], ref[nz]).max())
        print(f"policy_log on {name}: worst {worst:.2f} ulp of torch.log")
        assert worst <= 4.0, (name, worst)
        assert bool((got[~nz] == 0).all())
    assert float(a.min()) < 1e-299 and float(a.max()) > 1e299
    one = policy_log(torch.tensor([1.0], dtype=F64))
    assert float(one[0]) == 0.0 and not math.copysign(1.0, float(one[0])) < 0            # exactly +0.0
    assert bool((policy_log(u) <= 0).all())                                             # (the radius never sees a negative argument)


def test_the_quarter_turn_stays_within_two_to_minus_51():
    from pymgrid_amd.policy import gaussian_uniforms, policy_quarter_turn
    g = torch.Generator().manual_seed(2)
    f = torch.cat([torch.randint(0, 2 ** 52, (400_000,), generator=g).to(F64) * EPS,
                   torch.tensor([0.0, 0.5, 1.0 - EPS, 0.5 + EPS, 0.5 - EPS, EPS], dtype=F64)])
    s, c = policy_quarter_turn(f)
    ang = f * (math.pi / 2)
    es, ec = float((s - torch.sin(ang)).abs().max()), float((c - torch.cos(ang)).abs().max())
    print(f"quarter turn: sin within {es:.3g}, cos within {ec:.3g}")
    assert es <= 2.0 ** -51 and ec <= 2.0 ** -51
    s0, c0 = policy_quarter_turn(torch.tensor([0.0], dtype=F64))
    assert float(s0[0]) == 0.0 and float(c0[0]) == 1.0
    # all four quadrants through the pair's own draw: z / R is (cos, sin) of the whole angle
    u1, q, fr = gaussian_uniforms(7, torch.arange(100_000), 3, 0)
    assert sorted(q.unique().tolist()) == [0, 1, 2, 3] and float(fr.min()) >= 0.0 and float(fr.max()) < 1.0
    assert torch.equal(fr * 2.0 ** 52, (fr * 2.0 ** 52).round()) and float(u1.min()) > 0.0 and float(u1.max()) <= 1.0
    s, c = policy_quarter_turn(fr)
    sn = torch.where(q == 0, s, torch.where(q == 1, c, torch.where(q == 2, -s, -c)))
    cs = torch.where(q == 0, c, torch.where(q == 1, -s, torch.where(q == 2, -c, s)))
    # ... against libm's pair of the same quarter-turn fraction, turned by the same exact sign flips: 2^-51 in every quadrant
    ls, lc = torch.sin(fr * (math.pi / 2)), torch.cos(fr * (math.pi / 2))
    lsn = torch.where(q == 0, ls, torch.where(q == 1, lc, torch.where(q == 2, -ls, -lc)))
    lcs = torch.where(q == 0, lc, torch.where(q == 1, -ls, torch.where(q == 2, -lc, ls)))
    for quad in range(4):
        m = q == quad
        assert float((sn[m] - lsn[m]).abs().max()) <= 2.0 ** -51 and float((cs[m] - lcs[m]).abs().max()) <= 2.0 ** -51, quad
    # ... and the turn itself is the right one: libm on the WHOLE angle (q + f) * pi / 2.  That comparator rounds its argument three times
    # (the sum, the product, the constant): up to 2 pi * 3 * 2^-53 = 2.1e-15 of angle, so the bound here is 2^-51 + 2^-48 -- a wrong
    # sign or swap costs O(1)
    whole = (q.to(F64) + fr) * (math.pi / 2)
    assert float((sn - torch.sin(whole)).abs().max()) <= 2.0 ** -51 + 2.0 ** -48
    assert float((cs - torch.cos(whole)).abs().max()) <= 2.0 ** -51 + 2.0 ** -48


def test_policy_sqrt_stays_within_an_ulp_of_sqrt():
    """S(v) on [0, 74] (the radius' argument reaches 73.5), on 1e-16 .. 100 and at the corners: within 1 ulp of the correctly rounded
    root (0.78 measured against an 80-bit root); +-0.0 and negative arguments give +0.0."""
    from pymgrid_amd.policy import policy_sqrt
    g = torch.Generator().manual_seed(3)
    v = torch.cat([torch.rand(400_000, dtype=F64, generator=g) * 74.0, 10.0 ** (torch.rand(400_000, dtype=F64, generator=g) * 18.0 - 16.0),
                   torch.tensor([1.0, 4.0, 2.0 ** -52, 73.5, 2.0 * 53 * math.log(2.0)], dtype=F64)])
    got, ref = policy_sqrt(v), torch.sqrt(v)
    worst = float(_ulps(got, ref).max())
    print(f"policy_sqrt: worst {worst:.2f} ulp of torch.sqrt; exactly the rounded root for {float((got == ref).double().mean()):.3f} of the arguments")
    assert worst <= 1.0
    z = policy_sqrt(torch.tensor([0.0, -0.0, -1.0], dtype=F64))
    assert z.tolist() == [0.0, 0.0, 0.0] and all(math.copysign(1.0, x) > 0 for x in z.tolist())
    assert float(policy_sqrt(torch.tensor([1.0], dtype=F64))[0]) == 1.0 and float(policy_sqrt(torch.tensor([4.0], dtype=F64))[0]) == 2.0


def test_the_pair_is_the_libm_box_muller_of_the_same_uniforms():
    from pymgrid_amd.policy import gaussian_pair, gaussian_uniforms
    n = 400_000
    grid = torch.arange(n)
    worst = 0.0
    for seed, t, p in ((1, 0, 0), (2 ** 64 - 1, 12345, 1)):
        z0, z1 = gaussian_pair(seed, grid, t, p)
        u1, q, f = gaussian_uniforms(seed, grid, t, p)
        R, ang = torch.sqrt(-2.0 * torch.log(u1)), (q.to(F64) + f) * (math.pi / 2)
        worst = max(worst, float((z0 - R * torch.cos(ang)).abs().max()), float((z1 - R * torch.sin(ang)).abs().max()))
        assert float(R.max()) <= 8.58
    print(f"gaussian_pair: within {worst:.3g} of the libm Box-Muller")
    assert worst <= 2.0 ** -46
    a, b = gaussian_pair(1, grid, 0, 0), gaussian_pair(1, grid, 0, 1)
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[0], gaussian_pair(1, grid, 1, 0)[0])     # pair and counter move the draw


def test_moments_of_two_to_the_twenty_draws():
    """Mean, variance and fourth moment of 2^20 draws of seed 1 within five standard errors of 0, 1 and 3 (the standard errors of a
    unit normal's moments: 1 / sqrt(n), sqrt(2 / n), sqrt(96 / n))."""
    from pymgrid_amd.policy import gaussian_pair
    n = 2 ** 20
    z = torch.cat(gaussian_pair(1, torch.arange(n // 2), 0, 0))
    assert z.numel() == n and z.dtype == F64 and bool(torch.isfinite(z).all())
    m1, m2, m4 = float(z.mean()), float((z * z).mean()), float((z ** 4).mean())
    print(f"moments: mean {m1:.3g}, variance {m2:.6g}, fourth {m4:.6g}, largest |z| {float(z.abs().max()):.3f}")
    assert abs(m1) <= 5.0 / math.sqrt(n)
    assert abs(m2 - 1.0) <= 5.0 * math.sqrt(2.0 / n)
    assert abs(m4 - 3.0) <= 5.0 * math.sqrt(96.0 / n)
    assert float(z.abs().max()) > 4.0                                                     # (tails exist: no lattice within +-6 here)
    z0, z1 = z[: n // 2], z[n // 2:]
    assert abs(float((z0 * z1).mean())) <= 5.0 / math.sqrt(n // 2)                        # the two halves of a pair do not correlate


# ---- the head ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_out", [1, 2, 3, 4])
@pytest.mark.parametrize("n_hidden", [0, 16])
def test_logp_is_the_textbook_log_density(n_out, n_hidden):
    from pymgrid_amd.policy import gaussian_pair
    n, t = 700, 17
    obs = _rows(n, 8)
    pol = _policy(7, 8, n_hidden, n_out, "continuous")
    sigma = [0.3, 0.05, 1.7, 0.4][:n_out]
    scale = torch.as_tensor(np.linspace(0.5, 2.0, n))
    gs = _gs(seed=11, sigma=sigma, scale=scale)
    u, logp, raw = pol.act(obs, gs, counter=t, return_logp=True, return_raw=True)
    y = pol.outputs(obs)
    assert u.shape == raw.shape == (n, n_out) and logp.shape == (n,) and logp.dtype == F64
    assert torch.equal(u, torch.where(~(raw > 0), torch.zeros_like(raw), torch.where(raw > 1, torch.ones_like(raw), raw)))
    assert bool((raw != u).any()) and bool(((u > 0) & (u < 1)).any())                    # the clip moves some, not all
    s = torch.stack([sg * scale for sg in sigma], dim=1)
    z = torch.stack([gaussian_pair(11, torch.arange(n), t, o // 2)[o % 2] for o in range(n_out)], dim=1)
    assert torch.equal(raw, y + s * z)
    want = -0.5 * (z * z).sum(dim=1) - torch.log(s).sum(dim=1) - (n_out / 2) * math.log(2 * math.pi)
    assert float((logp - want).abs().max()) <= 1e-12
    # ... which is the density of raw under N(y, s^2), and what torch's own Normal says
    ref = torch.distributions.Normal(y, s).log_prob(raw).sum(dim=1)
    assert float((logp - ref).abs().max()) <= 1e-9
    # the flags choose what comes back, in the order (u, logp, raw)
    assert torch.equal(pol.act(obs, gs, counter=t), u)
    a, b = pol.act(obs, gs, counter=t, return_raw=True)
    assert torch.equal(a, u) and torch.equal(b, raw)
    a, b = pol.act(obs, gs, counter=t, return_logp=True)
    assert torch.equal(a, u) and torch.equal(b, logp)
    assert not torch.equal(pol.act(obs, gs, counter=t + 1), u)


def test_dead_columns_stay_greedy_and_drop_out_of_logp():
    n, t = 600, 4
    obs = _rows(n, 8)
    pol = _policy(7, 8, 16, 3, "continuous")
    y, greedy = pol.outputs(obs), pol.act(obs)
    # sigma 0 on column 1: raw == y there, and logp is that of the two live columns
    u, logp, raw = pol.act(obs, _gs(sigma=[0.2, 0.0, 0.4]), counter=t, return_logp=True, return_raw=True)
    assert torch.equal(raw[:, 1], y[:, 1]) and torch.equal(u[:, 1], greedy[:, 1])
    assert not torch.equal(raw[:, 0], y[:, 0]) and not torch.equal(raw[:, 2], y[:, 2])
    z0, z2 = (raw[:, 0] - y[:, 0]) / 0.2, (raw[:, 2] - y[:, 2]) / 0.4
    want = -0.5 * (z0 * z0 + z2 * z2) - math.log(0.2) - math.log(0.4) - math.log(2 * math.pi)
    assert float((logp - want).abs().max()) <= 1e-9
    # scale 0 on some grids: those grids are the greedy head, logp -0.0 - 0.0 = 0; the others draw
    scale = torch.as_tensor(np.where(np.arange(n) % 3 == 0, 0.0, np.linspace(0.5, 2.0, n)))
    zero = scale == 0
    u, logp, raw = pol.act(obs, _gs(sigma=0.2, scale=scale), counter=t, return_logp=True, return_raw=True)
    assert torch.equal(raw[zero], y[zero]) and torch.equal(u[zero], greedy[zero]) and bool((logp[zero] == 0).all())
    assert bool((raw[~zero] != y[~zero]).all()) and bool((logp[~zero] != 0).all())
    # a NaN or negative scale is dead too; every sigma 0 is the greedy head
    bad = scale.clone(); bad[1], bad[2] = float("nan"), -1.0
    u2, lp2, raw2 = pol.act(obs, _gs(sigma=0.2, scale=bad), counter=t, return_logp=True, return_raw=True)
    assert torch.equal(raw2[1:3], y[1:3]) and bool((lp2[1:3] == 0).all()) and torch.equal(raw2[3:], raw[3:])
    u3, lp3, raw3 = pol.act(obs, _gs(sigma=0.0), counter=t, return_logp=True, return_raw=True)
    assert torch.equal(u3, greedy) and torch.equal(raw3, y) and bool((lp3 == 0).all())


def test_nan_logits_give_a_zero_control_and_a_finite_logp():
    from pymgrid_amd import MLPPolicy
    n = 50
    W2, b2 = np.zeros((2, 8)), np.array([float("nan"), 0.5])
    pol = MLPPolicy(None, None, W2, b2, head="continuous")
    u, logp, raw = pol.act(_rows(n, 8), _gs(sigma=0.2), counter=0, return_logp=True, return_raw=True)
    assert bool(torch.isnan(raw[:, 0]).all()) and bool((u[:, 0] == 0).all()) and bool(torch.isfinite(logp).all())
    assert bool(torch.isfinite(raw[:, 1]).all())


def test_validation_and_the_python_refusals():
    from pymgrid_amd import GaussianSampling, Sampling, ValueHead
    tiny = np.finfo(np.float64).tiny
    for bad in (-0.1, float("nan"), float("inf"), tiny / 2, [0.1, -0.2], [0.1] * 5, []):
        with pytest.raises(ValueError):
            GaussianSampling(1, bad)
    for bad in (dict(scale=np.zeros(4, dtype=np.float32)), dict(scale=np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            GaussianSampling(1, 0.1, **bad)
    with pytest.raises(ValueError):
        GaussianSampling(-1, 0.1)
    gs = GaussianSampling(2 ** 64 - 1, 0.5)
    assert gs.sigma == (0.5,) * 4 and GaussianSampling(1, [0.1, 0.2]).sigma == (0.1, 0.2, 0.0, 0.0) and GaussianSampling(1, tiny).sigma[0] == tiny
    st, _ = gs.c_struct(torch.device("cpu"), 4)
    assert st.struct_size == C.sizeof(type(st)) and st.seed == 2 ** 64 - 1 and list(st.sigma) == [0.5] * 4 and not st.scale
    obs = _rows(10, 8)
    cont, disc = _policy(7, 8, 0, 2, "continuous"), _policy(7, 8, 0, 4, "discrete")
    with pytest.raises(ValueError, match="continuous head"):
        disc.act(obs, gs, counter=0)
    with pytest.raises(ValueError, match="counter"):
        cont.act(obs, gs)
    with pytest.raises(ValueError, match="return_logp"):
        cont.act(obs, return_logp=True)
    with pytest.raises(ValueError, match="return_prob"):
        cont.act(obs, gs, counter=0, return_prob=True)
    with pytest.raises(ValueError, match="discrete head"):
        cont.act(obs, Sampling(1), counter=0)
    with pytest.raises(ValueError, match="scale names"):
        cont.act(obs, GaussianSampling(1, 0.1, scale=np.ones(9)), counter=0)
    # a ValueHead(head="continuous") serves the continuous policy: one more output row on its trunk, staged without the discrete
    # head's padding; the head of the other kind is refused both ways
    head = ValueHead(np.ones((1, 8)), np.zeros(1), head="continuous")
    with pytest.raises(ValueError, match="head='continuous'"):
        head.value(_policy(7, 8, 0, 2, "discrete"), obs)
    with pytest.raises(ValueError, match="head='discrete'"):
        ValueHead(np.ones((1, 8)), np.zeros(1)).value(cont, obs)
    with pytest.raises(ValueError):
        ValueHead(np.ones((1, 8)), np.zeros(1), head="gaussian")
    acc = torch.zeros(10, dtype=F64)
    for j in range(8):
        acc = acc + 1.0 * obs[:, j]
    assert torch.equal(head.value(cont, obs), acc)
    m = 2
    assert head.lds_bytes(cont) == ((m + 1 + 8 * (m + 1) + 1) // 2 * 2) * 8


class _NoLaunch:
    """An engine stand-in for the checks StepEngine.step_k_policy_episodes makes before it touches a handle."""
    N, device = 4, torch.device("cpu")
    GAUSSIAN_KEYWORDS = ("sampling", "logp", "raw_actions", "critic", "values")


def test_the_keywords_of_the_gaussian_head_on_the_engine():
    """``step_k_policy_gaussian_episodes`` states the keywords; ``step_k_policy_episodes`` and ``PerGridWindowEnv.step_k_policy`` take
    them by name and refuse every other name and every misuse before anything touches a handle."""
    import inspect
    from pymgrid_amd import Exploration, Sampling, ValueHead
    from pymgrid_amd.engine import StepEngine
    from pymgrid_amd.hetero import PerGridWindowEnv
    _NoLaunch.step_k_policy_gaussian_episodes = StepEngine.step_k_policy_gaussian_episodes     # (what the call forwards to)
    par = inspect.signature(StepEngine.step_k_policy_gaussian_episodes).parameters
    assert list(par)[:4] == ["self", "policy", "sampling", "K"]
    assert (par["logp"].default, par["raw_actions"].default, par["critic"].default, par["values"].default) == (False, False, None, False)
    assert StepEngine.GAUSSIAN_KEYWORDS == _NoLaunch.GAUSSIAN_KEYWORDS
    for fn in (StepEngine.step_k_policy_episodes, PerGridWindowEnv.step_k_policy):
        assert any(q.kind is inspect.Parameter.VAR_KEYWORD for q in inspect.signature(fn).parameters.values())
    cont = _policy(7, 8, 3, 4, "continuous")
    head = ValueHead(np.zeros(3), np.float64(0.0), head="continuous")
    call = lambda **kw: StepEngine.step_k_policy_episodes(_NoLaunch(), cont, 4, **kw)     # noqa: E731
    with pytest.raises(TypeError, match="prob"):
        call(probs=True)
    for kw, word in ((dict(logp=True), "logp"), (dict(raw_actions=True), "raw_actions"), (dict(critic=head), r"GaussianSampling\(seed, 0.0\)"),
                     (dict(values=True), "critic=")):
        with pytest.raises(ValueError, match=word):
            call(**kw)
    gauss = lambda **kw: StepEngine.step_k_policy_gaussian_episodes(_NoLaunch(), cont, kw.pop("sampling", _gs()), 4, **kw)     # noqa: E731
    with pytest.raises(ValueError, match="GaussianSampling"):
        gauss(sampling=Sampling(1))
    with pytest.raises(ValueError, match="GaussianSampling"):
        call(sampling=Sampling(1))
    with pytest.raises(ValueError, match="exclude"):
        gauss(exploration=Exploration(1, sigma=0.1))
    with pytest.raises(ValueError, match="critic="):
        gauss(values=True)
    with pytest.raises(ValueError, match="values names"):
        gauss(critic=head, values=("value",))
    with pytest.raises(ValueError, match="head='discrete'"):
        gauss(critic=ValueHead(np.zeros(3), np.float64(0.0)))


# ---- the C entry: symbols, the struct, every refusal that needs no handle ----------------------------------------------------------
def test_symbols_struct_and_header():
    from pymgrid_amd import _lib
    _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "mgx.h")) as fh:
        header = fh.read()
    name = "mgx_step_k_policy_gaussian_episodes"
    assert name in _lib.SYMBOLS and getattr(L, name) is not None and f"int {name}(" in header
    assert "typedef struct mgx_gaussian" in header and header.count("L(a), for a positive NORMAL double a") == 1
    assert header.count("S(v), for a finite double v") == 1 and "0x5FE6EB50C7B537A9" in header
    assert _lib.lib().mgx_abi_minor() == 3 == _lib.ABI_MINOR
    assert "mgx_step_policy_head_episodes.hip" in [u[0] for u in _lib.UNITS]
    assert {4, 5} <= set(_lib.UNIT_HEADS["mgx_step_policy_head_episodes.hip"][1])      # (PolicyHead: Gaussian, Gaussian with a critic)
    assert any(src.endswith("mgx_step_policy_head_episodes.hip") for src in _lib.SOURCES)
    fields = re.search(r"typedef struct mgx_gaussian \{(.*?)\} mgx_gaussian;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert re.findall(r"([a-z_]+)(?:\[4\])?;", fields) == [n for n, _ in _lib.Gaussian._fields_]
    assert C.sizeof(_lib.Gaussian) == 4 + 4 + 8 + 4 * 8 + C.sizeof(C.c_void_p) == 56
    assert _lib.Gaussian.seed.offset == 8 and _lib.Gaussian.sigma.offset == 16 and _lib.Gaussian.scale.offset == 48
    # the constants of the header are the ones the host rule uses
    from pymgrid_amd import policy as P
    for v in P.LOG_COEFFS + P.SIN_COEFFS + P.COS_COEFFS + (P.HALF_LOG_2PI, P.HALF_PI, P.SQRT2):
        assert repr(v) in header, v
    assert P.LOG_COEFFS == tuple(2.0 / (2 * n + 1) for n in range(11))
    assert P.SIN_COEFFS == tuple((-1.0) ** (n + 1) / math.factorial(2 * n + 3) for n in range(7))
    assert P.COS_COEFFS == tuple((-1.0) ** (n + 1) / math.factorial(2 * n + 2) for n in range(8))
    assert P.HALF_LOG_2PI == 0.5 * math.log(2 * math.pi) and P.HALF_PI == math.pi / 2 and P.SQRT2 == math.sqrt(2.0)


def test_refusals_that_need_no_handle():
    """A NULL gaussian, a wrong struct_size, a sigma that is negative, NaN, infinite or positive and subnormal, a value output without
    a critic, a critic of the wrong size or without weights: MGX_ERR_INVALID before the handle is looked at -- the message names the
    call and the field.  (On a live handle, and the LDS bound: tests/test_policy_gaussian.py.)"""
    from pymgrid_amd import _lib
    lib = _lib.lib()
    name = b"mgx_step_k_policy_gaussian_episodes"
    spare = (C.c_double * 4)()
    addr = C.addressof(spare)
    pst = _lib.Policy()
    pst.struct_size, pst.n_policies, pst.n_in, pst.n_hidden, pst.n_out = C.sizeof(_lib.Policy), 1, 8, 0, 2
    pst.w2 = pst.b2 = addr                                          # (never read: every call below is refused before a launch)

    def gauss(**kw):
        st = _lib.Gaussian()
        st.struct_size, st.seed = C.sizeof(_lib.Gaussian), 3
        for o in range(4):
            st.sigma[o] = 0.1
        for k, v in kw.items():
            if k.startswith("sigma"):
                st.sigma[int(k[5:])] = v
            else:
                setattr(st, k, v)
        return st

    def critic(**kw):
        st = _lib.Critic()
        st.struct_size, st.w, st.b = C.sizeof(_lib.Critic), addr, addr
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    def call(gst, cst=None, values=(None, None, None), policy=pst):
        return lib.mgx_step_k_policy_gaussian_episodes(None, None if policy is None else C.byref(policy), None if gst is None else C.byref(gst),
                                                       None if cst is None else C.byref(cst), 4, None, None, None, None, None, None, None,
                                                       *values, None, None, None)
    tiny = np.finfo(np.float64).tiny
    bad = [("NULL argument", dict(gst=None)), ("NULL argument", dict(gst=gauss(), policy=None)),
           ("gaussian->struct_size", dict(gst=gauss(struct_size=C.sizeof(_lib.Gaussian) - 8))),
           ("gaussian->struct_size", dict(gst=gauss(struct_size=0))),
           ("sigma[0]", dict(gst=gauss(sigma0=-0.1))), ("sigma[1]", dict(gst=gauss(sigma1=float("nan")))),
           ("sigma[2]", dict(gst=gauss(sigma2=float("inf")))), ("sigma[3]", dict(gst=gauss(sigma3=tiny / 2))),
           ("sigma[3]", dict(gst=gauss(sigma3=5e-324))),
           ("value output without a critic", dict(gst=gauss(), values=(addr, None, None))),
           ("value output without a critic", dict(gst=gauss(), values=(None, addr, None))),
           ("value output without a critic", dict(gst=gauss(), values=(None, None, addr))),
           ("critic->struct_size", dict(gst=gauss(), cst=critic(struct_size=8))),
           ("NULL critic weights", dict(gst=gauss(), cst=critic(w=None))), ("NULL critic weights", dict(gst=gauss(), cst=critic(b=None)))]
    for word, kw in bad:
        rc = call(**kw)
        msg = lib.mgx_last_error()
        assert rc == _lib.MGX_ERR_INVALID and name in msg and word.encode() in msg, (word, rc, msg)
    # what passes these checks reaches the handle: sigma 0, the smallest normal sigma, a critic with its outputs
    for kw in (dict(gst=gauss(sigma0=0.0, sigma1=tiny)), dict(gst=gauss(), cst=critic(), values=(addr, addr, addr))):
        assert call(**kw) == _lib.MGX_ERR_INVALID and b"NULL argument" in lib.mgx_last_error()
