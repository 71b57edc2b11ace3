"""``ppo_grad_host`` (pymgrid_amd/policy.py), the host statement of the rule of ``mgx_policy_grad`` (include/mgx.h): the declaration
and its binding, the gradient against torch autograd of the same loss written with ``torch.softmax`` / ``torch.log``, and the gates
of the rule -- the clip, ``clip = inf``, the greedy head, the mask.  No GPU."""
import ctypes as C
import os

import pytest
import torch

from conftest import ROOT
from pymgrid_amd import _lib
from pymgrid_amd.policy import (MLPPolicy, Sampling, ValueHead, decision_rows, ppo_grad, ppo_grad_flat, ppo_grad_host)

# max_p |G_host - G_autograd| / (sum_s |g_s[p]| / M) over the cases of test_host_rule_against_autograd, measured on the CPU this
# was written on: 2.2e-15 (the two differ by libm's exp / log against the fixed E / L sequences and by the order of the sums).
# The bound is four times that.
AUTOGRAD_MEASURED = 2.2e-15
AUTOGRAD_BOUND = 4 * AUTOGRAD_MEASURED


def make_case(K, N, n_in, n_hidden, n_out, critic=True, seed=0, temperature=0.8, dtype=torch.float64):
    """Random normal data without ties: a policy, a critic, rows and what a collection would have returned for them."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)     # noqa: E731
    n_mid = n_hidden or n_in
    W1, b1 = (rn(n_hidden, n_in) * 0.5, rn(n_hidden) * 0.1) if n_hidden else (None, None)
    policy = MLPPolicy(W1, b1, rn(n_out, n_mid) * 0.5, rn(n_out) * 0.1)
    value = ValueHead(rn(n_mid) * 0.5, rn(1) * 0.1) if critic else None
    rows = rn(K, N, n_in).to(dtype)
    actions = torch.randint(0, n_out, (K, N), generator=g, dtype=torch.uint8)
    sampling = Sampling(7, temperature)
    # old probabilities round the current ones, so that both sides of the clip occur
    cur = ppo_grad_host(policy, None, rows, actions, torch.ones(K, N, dtype=torch.float64), rn(K, N), sampling=sampling, ratio=True)["ratio"]
    old = cur * torch.exp(0.3 * rn(K, N))
    return dict(policy=policy, critic=value, rows=rows, actions=actions, old_probs=old, advantages=rn(K, N),
                returns=rn(K, N) if critic else None, sampling=sampling)


def autograd_grads(c, clip, vf_coef, ent_coef, mask=None):
    """The same loss with torch.softmax / torch.log under autograd: (flat gradient in the order of ppo_grad_flat, stats)."""
    pol, cr = c["policy"], c["critic"]
    params = [t.clone().requires_grad_(True) for t in (pol.W1, pol.b1, pol.W2, pol.b2) if t is not None]
    W1, b1, W2, b2 = params if pol.n_hidden else [None, None] + params
    cparams = [t.clone().requires_grad_(True) for t in (cr.w, cr.b)] if cr is not None else []
    x = c["rows"].reshape(-1, pol.n_in).double()
    h = torch.relu(x @ W1[0].T + b1[0]) if pol.n_hidden else x
    y = h @ W2[0].T + b2[0]
    p = torch.softmax(y / c["sampling"].temperature, dim=1)
    logp = torch.log(p)
    a = c["actions"].reshape(-1).long()
    rho = p.gather(1, a[:, None])[:, 0] / c["old_probs"].reshape(-1)
    A = c["advantages"].reshape(-1)
    pl = -torch.minimum(rho * A, torch.clamp(rho, 1.0 - clip, 1.0 + clip) * A) if clip != float("inf") else -(rho * A)
    H = -(p * logp).sum(dim=1)
    vl = 0.5 * (h @ cparams[0][0] + cparams[1][0] - c["returns"].reshape(-1)) ** 2 if cr is not None else torch.zeros_like(pl)
    keep = mask.reshape(-1) != 0 if mask is not None else torch.ones_like(a, dtype=torch.bool)
    loss = pl[keep].mean() + vf_coef * vl[keep].mean() - ent_coef * H[keep].mean()
    loss.backward()
    flat = torch.cat([t.grad.reshape(-1) for t in params + cparams])
    return flat, torch.stack([pl[keep].mean(), vl[keep].mean(), H[keep].mean()]).detach()


def test_header_declares_the_call_and_the_binding_binds_it():
    with open(os.path.join(ROOT, "include", "mgx.h")) as fh:
        header = fh.read()
    for name in ("mgx_policy_grad", "mgx_policy_grad_workspace"):
        assert f"int {name}(" in header and name in _lib.SYMBOLS
    assert "struct mgx_policy_grad {" in header
    _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    assert L.mgx_policy_grad is not None and L.mgx_policy_grad_workspace is not None
    assert C.sizeof(_lib.PolicyGrad) == 8 + 6 * 8 + 3 * 8 + 9 * 8 + 8


@pytest.mark.parametrize("n_hidden,n_out,critic", [(16, 12, True), (5, 4, True), (0, 12, True), (16, 4, False)])
def test_host_rule_against_autograd(n_hidden, n_out, critic):
    c = make_case(3, 130, 10, n_hidden, n_out, critic=critic, seed=n_hidden + n_out)            # M = 390
    clip, vf, ent = 0.2, 0.5, 0.01
    res = ppo_grad_host(**c, clip=clip, vf_coef=vf, ent_coef=ent, per_sample=True)
    M = res["terms"].shape[0]
    assert M == 390 and 0.0 < float(res["stats"][3]) < 1.0                                  # (both sides of the gate occur)
    ref, ref_stats = autograd_grads(c, clip, vf, ent)
    scale = res["terms"].abs().sum(dim=0) / M
    err = float(((ppo_grad_flat(res) - ref).abs() / scale).max())
    print(f"n_hidden {n_hidden} n_out {n_out} critic {critic}: max_p |G_host - G_autograd| / (sum_s |g_s[p]| / M) = {err:.3e}")
    assert err <= AUTOGRAD_BOUND
    assert torch.allclose(res["stats"][:3], ref_stats, rtol=1e-13, atol=1e-15)


def test_host_rule_against_autograd_unclipped_and_masked():
    c = make_case(3, 130, 6, 16, 12, seed=3)
    mask = (torch.rand(3, 130, generator=torch.Generator().manual_seed(5)) < 0.6).to(torch.uint8)
    res = ppo_grad_host(**c, clip=float("inf"), vf_coef=0.5, ent_coef=0.01, mask=mask, per_sample=True)
    M = res["terms"].shape[0]
    assert M == int(mask.sum()) and float(res["stats"][3]) == 0.0
    ref, _ = autograd_grads(c, float("inf"), 0.5, 0.01, mask)
    scale = res["terms"].abs().sum(dim=0) / M
    err = float(((ppo_grad_flat(res) - ref).abs() / scale).max())
    print(f"clip = inf, masked: {err:.3e}")
    assert err <= AUTOGRAD_BOUND


def test_the_clip_gates_exactly():
    """A > 0 with rho > 1 + eps and A < 0 with rho < 1 - eps: exactly zero policy terms; the other two corners stay live."""
    c = make_case(1, 4, 6, 16, 4, critic=False, seed=11)
    cur = ppo_grad_host(**{**c, "old_probs": torch.ones(1, 4, dtype=torch.float64)}, ratio=True)["ratio"]
    c["old_probs"] = cur / torch.tensor([[1.5, 0.5, 1.5, 0.5]], dtype=torch.float64)       # rho = 1.5, 0.5, 1.5, 0.5
    c["advantages"] = torch.tensor([[1.0, -1.0, -1.0, 1.0]], dtype=torch.float64)
    res = ppo_grad_host(**c, clip=0.2, ent_coef=0.0, per_sample=True, ratio=True)
    assert torch.allclose(res["ratio"], torch.tensor([[1.5, 0.5, 1.5, 0.5]], dtype=torch.float64), rtol=1e-15)
    assert (res["terms"][:2] == 0.0).all() and (res["terms"][2:].abs().sum(dim=1) > 0.0).all()
    assert res["stat_terms"][:, 3].tolist() == [1.0, 1.0, 0.0, 0.0]
    assert res["stat_terms"][0, 0] == -(1.0 * 1.2) and res["stat_terms"][1, 0] == 1.0 * (1.0 - 0.2)
    free = ppo_grad_host(**c, clip=float("inf"), ent_coef=0.0, per_sample=True)              # clip = inf never gates
    assert (free["terms"].abs().sum(dim=1) > 0.0).all() and (free["stat_terms"][:, 3] == 0.0).all()


def test_greedy_rows_carry_only_the_value_term():
    c = make_case(2, 5, 6, 5, 4, seed=13)
    scale = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0], dtype=torch.float64)                    # tau = 0 on grids 1 and 3
    c["sampling"] = Sampling(7, 0.8, scale=scale)
    res = ppo_grad_host(**c, clip=0.2, ent_coef=0.01, per_sample=True, ratio=True)
    pol = c["policy"]
    n_w1, n_w2 = pol.n_hidden * (pol.n_in + 1), pol.n_out * (pol.n_hidden + 1)
    greedy = torch.tensor([False, True, False, True, False]).repeat(2)
    t = res["terms"]
    assert (t[greedy][:, n_w1:n_w1 + n_w2] == 0.0).all()                                    # no logit gradient at all
    assert (t[greedy][:, n_w1 + n_w2:].abs().sum(dim=1) > 0.0).all()                        # the critic's terms stay
    assert (res["stat_terms"][greedy][:, [0, 2, 3]] == 0.0).all() and (res["stat_terms"][greedy][:, 1] > 0.0).all()
    assert (t[~greedy][:, n_w1:n_w1 + n_w2].abs().sum(dim=1) > 0.0).all()
    assert torch.equal(res["ratio"].reshape(-1)[greedy], 1.0 / c["old_probs"].reshape(-1)[greedy])
    only_value = ppo_grad_host(**{**c, "sampling": Sampling(7, 0.0)}, clip=0.2, ent_coef=0.01)
    assert (only_value["W2"] == 0.0).all() and (only_value["b2"] == 0.0).all() and only_value["w"].abs().sum() > 0.0


@pytest.mark.parametrize("n_out", [12, 4])
def test_ratio_of_the_collecting_policy_is_exactly_one(n_out):
    """What the GPU end-to-end test states on the device, on the host: the gradient restates the forward of ``act`` operation by
    operation, so the probabilities ``act`` returned, fed back with the same parameters, give ``ratio == 1.0`` exactly -- on the
    grids of a temperature ladder and on the one whose ``scale`` of 0 makes it greedy."""
    N = 64
    c = make_case(1, N, 10, 16, n_out, critic=False, seed=23 + n_out)
    scale = torch.linspace(0.25, 2.0, N, dtype=torch.float64)
    scale[7] = 0.0
    sampling = Sampling(7, 0.8, scale=scale)
    obs = c["rows"][0]
    ids, prob = c["policy"].act(obs, sampling, 5, return_prob=True)
    assert prob[7] == 1.0 and 1 < len(set(ids.tolist())) and (prob < 1.0).sum() >= N - 2       # (a ladder that does sample)
    res = ppo_grad_host(c["policy"], None, obs.unsqueeze(0), ids.to(torch.uint8).unsqueeze(0), prob.unsqueeze(0), c["advantages"],
                        sampling=sampling, ratio=True)
    assert res["ratio"].shape == (1, N) and (res["ratio"] == 1.0).all()


def test_mask_all_zero_gives_zeros():
    c = make_case(2, 5, 6, 5, 4, seed=17)
    res = ppo_grad_host(**c, mask=torch.zeros(2, 5, dtype=torch.uint8))
    assert all((res[n] == 0.0).all() for n in ("W1", "b1", "W2", "b2", "w", "b", "stats"))


def test_decision_rows_and_checks():
    obs = torch.arange(24, dtype=torch.float64).reshape(3, 2, 4)
    before = -torch.ones(2, 4, dtype=torch.float64)
    rows = decision_rows(before, obs)
    assert torch.equal(rows[0], before) and torch.equal(rows[1:], obs[:-1]) and rows.is_contiguous()
    c = make_case(2, 5, 6, 5, 4, seed=19)
    with pytest.raises(ValueError, match="GPU"):
        ppo_grad(**c)                                                                    # CPU tensors: as gae
    with pytest.raises(ValueError, match="clip"):
        ppo_grad_host(**c, clip=-0.1)
    with pytest.raises(ValueError, match="returns"):
        ppo_grad_host(**{**c, "returns": None})
    with pytest.raises(ValueError, match="population"):
        ppo_grad_host(**{**c, "policy": MLPPolicy(torch.zeros(2, 5, 6, dtype=torch.float64), torch.zeros(2, 5, dtype=torch.float64),
                                                  torch.zeros(2, 4, 5, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.float64))})
