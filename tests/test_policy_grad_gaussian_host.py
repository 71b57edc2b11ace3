"""``ppo_grad_gaussian_host`` (pymgrid_amd/policy.py), the host statement of the rule of ``mgx_policy_grad_gaussian`` (include/mgx.h):
the declaration and its binding, the gradient against torch autograd of the same loss written with ``torch.log`` / ``torch.exp`` and
the closed-form Gaussian density and entropy (``log sigma`` a leaf), the gates of the rule -- the clip, ``clip = inf``, a column with
sigma 0, a grid with scale 0, the mask, where ``ent_coef`` enters -- and the derived bound on the ratio of an un-updated policy.
No GPU."""
import ctypes as C
import math
import os

import pytest
import torch

from conftest import ROOT
from pymgrid_amd import _lib
from pymgrid_amd.policy import (GaussianSampling, MLPPolicy, Sampling, ValueHead, ppo_grad_flat, ppo_grad_gaussian,
                                ppo_grad_gaussian_host, ppo_grad_host)

F64 = torch.float64
U = 2.0 ** -53
# max_p |G_host - G_autograd| / (sum_s |g_s[p]| / M) over the cases of test_host_rule_against_autograd and the unclipped, masked
# case, measured on the CPU this was written on: 5.8e-15 (the two differ by libm's exp / log against the fixed E / L sequences and by
# the order of the sums).  The bound is four times that.
AUTOGRAD_MEASURED = 5.8e-15
AUTOGRAD_BOUND = 4 * AUTOGRAD_MEASURED
SIGMA = (0.3, 0.1, 0.2, 0.05)


def make_case_gaussian(K, N, n_in, n_hidden, A, critic=True, seed=0, sigma=SIGMA, scale=None, dtype=F64):
    """Random normal data: a continuous policy, a critic, rows, and what a Gaussian collection would have returned for them --
    ``raw = y + s * z`` with z normal, ``old_logp`` the current log-probability plus ``0.3 * randn`` so that both sides of the clip
    occur.  ``sigma``: the first ``A`` of it are used (a 0 among them: a dead column); ``scale``: float64 ``[N]`` or None."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)     # noqa: E731
    n_mid = n_hidden or n_in
    W1, b1 = (rn(n_hidden, n_in) * 0.5, rn(n_hidden) * 0.1) if n_hidden else (None, None)
    policy = MLPPolicy(W1, b1, rn(A, n_mid) * 0.5, rn(A) * 0.1, head="continuous")
    value = ValueHead(rn(n_mid) * 0.5, rn(1) * 0.1, head="continuous") if critic else None
    rows = rn(K, N, n_in).to(dtype)
    sampling = GaussianSampling(7, list(sigma[:A]), scale=scale)
    y = policy.outputs(rows.reshape(K * N, n_in)).reshape(K, N, A)
    s = torch.tensor(sigma[:A], dtype=F64).expand(K, N, A)
    if scale is not None:
        s = s * scale.view(1, N, 1)
    raw = y + s * rn(K, N, A)
    live = s > 0
    sd = torch.where(live, s, torch.ones_like(s))
    logp = (torch.where(live, -0.5 * ((raw - y) / sd) ** 2 - torch.log(sd) - 0.5 * math.log(2 * math.pi), torch.zeros_like(s))).sum(dim=2)
    return dict(policy=policy, critic=value, rows=rows, raw_actions=raw.contiguous(), old_logp=logp + 0.3 * rn(K, N), advantages=rn(K, N),
                returns=rn(K, N) if critic else None, sampling=sampling)


def autograd_grads(c, clip, vf_coef, ent_coef, mask=None):
    """The same loss with torch.log / torch.exp and the closed-form density and entropy under autograd, ``log sigma`` a leaf:
    (flat gradient in the order of ppo_grad_flat with ``log_sigma`` [A] last, stats[:3], kl)."""
    pol, cr, gs = c["policy"], c["critic"], c["sampling"]
    A_ = pol.n_out
    params = [t.clone().requires_grad_(True) for t in (pol.W1, pol.b1, pol.W2, pol.b2) if t is not None]
    W1, b1, W2, b2 = params if pol.n_hidden else [None, None] + params
    cparams = [t.clone().requires_grad_(True) for t in (cr.w, cr.b)] if cr is not None else []
    log_sigma = torch.log(torch.tensor(gs.sigma[:A_], dtype=F64)).requires_grad_(True)
    x = c["rows"].reshape(-1, pol.n_in).double()
    K, N = c["rows"].shape[:2]
    h = torch.relu(x @ W1[0].T + b1[0]) if pol.n_hidden else x
    y = h @ W2[0].T + b2[0]
    s = torch.exp(log_sigma).unsqueeze(0).expand(x.shape[0], A_)
    if gs.scale is not None:
        s = s * gs.scale.repeat(K).unsqueeze(1)
    raw = c["raw_actions"].reshape(-1, A_)
    logp = (-0.5 * ((raw - y) / s) ** 2 - torch.log(s) - 0.5 * math.log(2 * math.pi)).sum(dim=1)
    D = logp - c["old_logp"].reshape(-1)
    rho = torch.exp(D)
    Adv = c["advantages"].reshape(-1)
    pl = -torch.minimum(rho * Adv, torch.clamp(rho, 1.0 - clip, 1.0 + clip) * Adv) if clip != float("inf") else -(rho * Adv)
    H = (torch.log(s) + 0.5 + 0.5 * math.log(2 * math.pi)).sum(dim=1)
    vl = 0.5 * (h @ cparams[0][0] + cparams[1][0] - c["returns"].reshape(-1)) ** 2 if cr is not None else torch.zeros_like(pl)
    keep = mask.reshape(-1) != 0 if mask is not None else torch.ones_like(Adv, dtype=torch.bool)
    loss = pl[keep].mean() + vf_coef * vl[keep].mean() - ent_coef * H[keep].mean()
    loss.backward()
    flat = torch.cat([t.grad.reshape(-1) for t in params + cparams + [log_sigma]])
    kl = ((rho - 1.0) - D)[keep].mean().detach()
    return flat, torch.stack([pl[keep].mean(), vl[keep].mean(), H[keep].mean()]).detach(), kl


def _against_autograd(c, clip, mask=None):
    vf, ent = 0.5, 0.01
    res = ppo_grad_gaussian_host(**c, clip=clip, vf_coef=vf, ent_coef=ent, mask=mask, per_sample=True)
    A_ = c["policy"].n_out
    M = res["terms"].shape[0]
    ref, ref_stats, ref_kl = autograd_grads(c, clip, vf, ent, mask)
    P = ref.numel()                                                       # (log_sigma [A] last; the host pads it to 4 with zeros)
    got = ppo_grad_flat(res)
    assert got.numel() == P + 4 - A_ and (got[P:] == 0.0).all() and (res["terms"][:, P:] == 0.0).all()
    scale = res["terms"][:, :P].abs().sum(dim=0) / M
    err = float(((got[:P] - ref).abs() / scale).max())
    assert torch.allclose(res["stats"][:3], ref_stats, rtol=1e-13, atol=1e-15)
    assert torch.allclose(res["stats"][4], ref_kl, rtol=1e-13, atol=1e-15)
    return res, M, err


@pytest.mark.parametrize("n_hidden,A,critic", [(16, 4, True), (5, 3, True), (0, 1, True), (16, 2, False)])
def test_host_rule_against_autograd(n_hidden, A, critic):
    c = make_case_gaussian(3, 130, 10, n_hidden, A, critic=critic, seed=n_hidden + A)            # M = 390
    res, M, err = _against_autograd(c, 0.2)
    assert M == 390 and 0.0 < float(res["stats"][3]) < 1.0                                  # (both sides of the gate occur)
    print(f"n_hidden {n_hidden} A {A} critic {critic}: max_p |G_host - G_autograd| / (sum_s |g_s[p]| / M) = {err:.3e}")
    assert err <= AUTOGRAD_BOUND


def test_host_rule_against_autograd_unclipped_and_masked():
    c = make_case_gaussian(3, 130, 6, 16, 4, seed=3)
    mask = (torch.rand(3, 130, generator=torch.Generator().manual_seed(5)) < 0.6).to(torch.uint8)
    res, M, err = _against_autograd(c, float("inf"), mask)
    assert M == int(mask.sum()) and float(res["stats"][3]) == 0.0
    print(f"clip = inf, masked: {err:.3e}")
    assert err <= AUTOGRAD_BOUND


def test_header_declares_the_call_and_the_binding_binds_it():
    with open(os.path.join(ROOT, "include", "mgx.h")) as fh:
        header = fh.read()
    assert "int mgx_policy_grad_gaussian(" in header and "mgx_policy_grad_gaussian" in _lib.SYMBOLS
    assert "struct mgx_policy_grad_gaussian {" in header
    _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    assert L.mgx_policy_grad_gaussian is not None
    assert C.sizeof(_lib.PolicyGradGaussian) == 8 + 6 * 8 + 3 * 8 + 10 * 8 + 8


def _cur_logp(c):
    """The current log-probability of the case's raw actions, with the rule's own operations (mgx_gaussian)."""
    from pymgrid_amd.policy import HALF_LOG_2PI, policy_log
    pol, gs = c["policy"], c["sampling"]
    K, N = c["rows"].shape[:2]
    y = pol.outputs(c["rows"].reshape(K * N, pol.n_in))
    raw = c["raw_actions"].reshape(K * N, pol.n_out)
    Q, Cn = torch.zeros(K * N, dtype=F64), torch.zeros(K * N, dtype=F64)
    for o in range(pol.n_out):
        s = torch.full((K * N,), gs.sigma[o], dtype=F64) if gs.scale is None else gs.sigma[o] * gs.scale.repeat(K)
        live = s > 0
        sd = torch.where(live, s, torch.ones_like(s))
        z = (raw[:, o] - y[:, o]) / sd
        Q = torch.where(live, Q + z * z, Q)
        Cn = torch.where(live, Cn + (policy_log(sd) + HALF_LOG_2PI), Cn)
    return ((-0.5 * Q) - Cn).reshape(K, N)


def test_the_clip_gates_exactly():
    """A > 0 with rho > 1 + eps and A < 0 with rho < 1 - eps: exactly zero policy and log-sigma terms; the other two corners stay live."""
    c = make_case_gaussian(1, 4, 6, 16, 4, critic=False, seed=11)
    want = torch.tensor([[1.5, 0.5, 1.5, 0.5]], dtype=F64)
    c["old_logp"] = _cur_logp(c) - torch.log(want)
    c["advantages"] = torch.tensor([[1.0, -1.0, -1.0, 1.0]], dtype=F64)
    res = ppo_grad_gaussian_host(**c, clip=0.2, ent_coef=0.0, per_sample=True, ratio=True)
    assert torch.allclose(res["ratio"], want, rtol=1e-14)
    assert (res["terms"][:2] == 0.0).all() and (res["terms"][2:].abs().sum(dim=1) > 0.0).all()
    assert (res["terms"][2:, -4:].abs() > 0.0).all()                                         # (the log-sigma terms of the live corners)
    assert res["stat_terms"][:, 3].tolist() == [1.0, 1.0, 0.0, 0.0]
    assert res["stat_terms"][0, 0] == -(1.0 * 1.2) and res["stat_terms"][1, 0] == 1.0 * (1.0 - 0.2)
    free = ppo_grad_gaussian_host(**c, clip=float("inf"), ent_coef=0.0, per_sample=True)         # clip = inf never gates
    assert (free["terms"].abs().sum(dim=1) > 0.0).all() and (free["stat_terms"][:, 3] == 0.0).all()


def _blocks(pol, critic):
    """Column ranges of ``terms``: (W2 | b2 block, the critic's block, log_sigma)."""
    n_mid = pol.n_hidden or pol.n_in
    n_w1 = pol.n_hidden * (pol.n_in + 1)
    n_w2 = pol.n_out * (n_mid + 1)
    n_c = n_mid + 1 if critic else 0
    return n_w1, n_w2, n_c


def test_a_dead_column_carries_nothing():
    """sigma[1] == 0: dy[1] and dls[1] are exactly 0 on every sample, the other columns stay live."""
    c = make_case_gaussian(2, 5, 6, 5, 4, seed=13, sigma=(0.3, 0.0, 0.2, 0.05))
    res = ppo_grad_gaussian_host(**c, clip=float("inf"), ent_coef=0.01, per_sample=True)
    pol = c["policy"]
    n_w1, n_w2, n_c = _blocks(pol, True)
    t = res["terms"]
    W2t = t[:, n_w1:n_w1 + pol.n_out * pol.n_hidden].reshape(-1, pol.n_out, pol.n_hidden)
    b2t = t[:, n_w1 + pol.n_out * pol.n_hidden:n_w1 + n_w2]
    ls = t[:, -4:]
    assert (b2t[:, 1] == 0.0).all() and (W2t[:, 1] == 0.0).all() and (ls[:, 1] == 0.0).all()
    for o in (0, 2, 3):
        assert (b2t[:, o] != 0.0).all() and (ls[:, o] != 0.0).all()
    assert float(res["log_sigma"][1]) == 0.0 and float(res["W2"][1].abs().sum()) == 0.0 and float(res["W2"][0].abs().sum()) > 0.0
    assert (res["stat_terms"][:, 2] > -10.0).all() and float(res["stats"][2]) != 0.0         # (the entropy of three columns)


def test_a_grid_with_scale_zero_carries_only_the_value_term():
    scale = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0], dtype=F64)
    c = make_case_gaussian(2, 5, 6, 5, 4, seed=13, scale=scale)
    res = ppo_grad_gaussian_host(**c, clip=0.2, ent_coef=0.01, per_sample=True, ratio=True)
    n_w1, n_w2, n_c = _blocks(c["policy"], True)
    off = torch.tensor([False, True, False, True, False]).repeat(2)
    t = res["terms"]
    assert (t[off][:, n_w1:n_w1 + n_w2] == 0.0).all() and (t[off][:, -4:] == 0.0).all()     # no mean or log-sigma gradient at all
    assert (t[off][:, n_w1 + n_w2:n_w1 + n_w2 + n_c].abs().sum(dim=1) > 0.0).all()         # the critic's terms stay
    assert (res["stat_terms"][off][:, [0, 2, 3, 4]] == 0.0).all() and (res["stat_terms"][off][:, 1] > 0.0).all()
    t = ppo_grad_gaussian_host(**c, clip=float("inf"), ent_coef=0.01, per_sample=True)["terms"]      # (no gate: every live grid's terms show)
    assert (t[~off][:, n_w1:n_w1 + n_w2].abs().sum(dim=1) > 0.0).all() and (t[~off][:, -4:] != 0.0).all()
    assert (t[off][:, n_w1:n_w1 + n_w2] == 0.0).all() and (t[off][:, -4:] == 0.0).all()
    none = ppo_grad_gaussian_host(**{**c, "sampling": GaussianSampling(7, [0.0] * 4)}, clip=0.2, ent_coef=0.01)
    assert (none["W2"] == 0.0).all() and (none["b2"] == 0.0).all() and (none["log_sigma"] == 0.0).all() and none["w"].abs().sum() > 0.0
    assert none["stats"][[0, 2, 3, 4]].tolist() == [0.0] * 4


def test_mask_all_zero_gives_zeros():
    c = make_case_gaussian(2, 5, 6, 5, 4, seed=17)
    res = ppo_grad_gaussian_host(**c, mask=torch.zeros(2, 5, dtype=torch.uint8))
    assert all((res[n] == 0.0).all() for n in ("W1", "b1", "W2", "b2", "w", "b", "log_sigma", "stats"))
    assert res["stats"].shape == (5,) and res["log_sigma"].shape == (4,)


def test_ent_coef_enters_log_sigma_alone():
    c = make_case_gaussian(3, 40, 6, 5, 3, seed=19)
    a = ppo_grad_gaussian_host(**c, clip=0.2, ent_coef=0.0)
    b = ppo_grad_gaussian_host(**c, clip=0.2, ent_coef=0.01)
    for name in ("W1", "b1", "W2", "b2", "w", "b"):
        assert torch.equal(a[name], b[name]), name
    assert torch.allclose(b["log_sigma"][:3], a["log_sigma"][:3] - 0.01, rtol=0.0, atol=1e-15) and not torch.equal(a["log_sigma"], b["log_sigma"])
    assert float(a["log_sigma"][3]) == 0.0 and float(b["log_sigma"][3]) == 0.0               # (past n_out)


def ratio_bound(policy, gs, rows, raw, logp):
    """The derived per-sample bound on |rho - 1| for what a collection returns with un-updated parameters (include/mgx.h,
    mgx_policy_grad_gaussian), for ``rows`` [n, n_in], ``raw`` [n, A], ``logp`` [n] (float64, any device) and ``gs`` without a dead
    column among the grids asked: ``1.01 * B + 8 u``."""
    n, A_ = raw.shape
    y = policy.outputs(rows)
    B, Q = torch.zeros(n, dtype=F64, device=raw.device), torch.zeros(n, dtype=F64, device=raw.device)
    scale = gs.scale_on(raw.device, n) if gs.scale is not None and gs.scale.shape[0] == n else None
    for o in range(A_):
        s = torch.full((n,), gs.sigma[o], dtype=F64, device=raw.device) if scale is None else gs.sigma[o] * scale
        live = s > 0
        sd = torch.where(live, s, torch.ones_like(s))
        z = ((raw[:, o] - y[:, o]) / sd).abs()
        delta = U * (4.0 * z + 2.0 * raw[:, o].abs() / sd)
        B = torch.where(live, B + z * delta, B)
        Q = torch.where(live, Q + z * z, Q)
    B = B + 5.0 * U * Q + 2.0 * U * logp.abs()
    return 1.01 * B + 8.0 * U


@pytest.mark.parametrize("sigma", [[0.3, 0.1, 0.2, 0.05], [1e-3] * 4, [2.0] * 4])
def test_ratio_of_an_unupdated_policy_stays_inside_the_derived_bound(sigma):
    g = torch.Generator().manual_seed(23)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)     # noqa: E731
    n, n_in, nh, A_ = 4096, 10, 16, 4
    policy = MLPPolicy(rn(nh, n_in) * 0.5, rn(nh) * 0.1, rn(A_, nh) * 0.5, rn(A_) * 0.1, head="continuous")
    gs = GaussianSampling(29, sigma)
    rows, raws, logps = [], [], []
    for counter in range(4):
        obs = rn(n, n_in)
        u, logp, raw = policy.act(obs, gs, counter=counter, return_logp=True, return_raw=True)
        rows.append(obs), raws.append(raw), logps.append(logp)
    rows, raw, logp = torch.stack(rows), torch.stack(raws), torch.stack(logps)
    rho = ppo_grad_gaussian_host(policy, None, rows, raw, logp, torch.ones(4, n, dtype=F64), sampling=gs, ratio=True)["ratio"]
    bound = ratio_bound(policy, gs, rows.reshape(-1, n_in), raw.reshape(-1, A_), logp.reshape(-1)).reshape(4, n)
    frac = ((rho - 1.0).abs() / bound).max()
    print(f"sigma {sigma}: worst |rho - 1| / bound = {float(frac):.3f}, worst |rho - 1| = {float((rho - 1.0).abs().max()):.3e}")
    assert ((rho - 1.0).abs() <= bound).all()
    assert not (rho == 1.0).all()                                                           # (not exactly 1.0, as the header says)


def test_python_refusals():
    c = make_case_gaussian(2, 5, 6, 5, 4, seed=19)
    with pytest.raises(ValueError, match="GPU"):
        ppo_grad_gaussian(**c)                                                           # CPU tensors: as ppo_grad
    disc = MLPPolicy(c["policy"].W1, c["policy"].b1, c["policy"].W2, c["policy"].b2)
    with pytest.raises(ValueError, match="continuous head"):
        ppo_grad_gaussian_host(**{**c, "policy": disc, "critic": None, "returns": None})
    with pytest.raises(ValueError, match="ppo_grad_gaussian"):                           # ... and the discrete call names this one
        ppo_grad_host(c["policy"], None, c["rows"], torch.zeros(2, 5, dtype=torch.uint8), c["old_logp"], c["advantages"],
                      sampling=Sampling(7, 1.0))
    with pytest.raises(ValueError, match="population"):
        ppo_grad_gaussian_host(**{**c, "critic": None, "returns": None,
                                  "policy": MLPPolicy(torch.zeros(2, 5, 6, dtype=F64), torch.zeros(2, 5, dtype=F64),
                                                      torch.zeros(2, 4, 5, dtype=F64), torch.zeros(2, 4, dtype=F64), head="continuous")})
    with pytest.raises(ValueError, match="GaussianSampling"):
        ppo_grad_gaussian_host(**{**c, "sampling": Sampling(7, 1.0)})
    with pytest.raises(ValueError, match="raw_actions"):
        ppo_grad_gaussian_host(**{**c, "raw_actions": c["raw_actions"][:, :, :3].contiguous()})
    with pytest.raises(ValueError, match="raw_actions"):
        ppo_grad_gaussian_host(**{**c, "raw_actions": c["raw_actions"].float()})
    with pytest.raises(ValueError, match="clip"):
        ppo_grad_gaussian_host(**c, clip=-0.1)
    with pytest.raises(ValueError, match="returns"):
        ppo_grad_gaussian_host(**{**c, "returns": None})
