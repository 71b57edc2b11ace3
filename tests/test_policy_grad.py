"""``ppo_grad`` (mgx_policy_grad: policy_grad_kernel + policy_grad_finish_kernel) against ``ppo_grad_host``, the host statement of
the rule of include/mgx.h.  One live sample is exact (``==``): a product added to zeros.  Many samples are held to the any-order
summation bound against the exactly summed per-sample terms (math.fsum) -- the sum goes through the fp64 MFMA, whose inner order
and rounding are the hardware's -- and must be identical from run to run.  End to end: on the data of a sampling launch with a
critic, restarts inside, the ratio is exactly 1.0 and with ``returns = values`` the critic's gradient exactly 0.0.  WIDTH_CASES runs
both comparisons once per compiled form of the kernel: every row width 1 .. 12, with and without a critic."""
import ctypes as C
import math

import pytest
import torch

from test_policy_critic import _head
from test_policy_grad_host import make_case
from test_policy_rollout import _batch, _n_out
from test_policy_sample import _sampling, _spread_policy

F64, F32 = torch.float64, torch.float32
NAMES = ("W1", "b1", "W2", "b2", "w", "b")
U = 2.0 ** -53
ONE_SAMPLE_CASES = tuple((nh, n_in, n_out, critic) for critic in (True, False) for n_out in (12, 4) for nh, n_in in ((16, 10), (5, 7), (0, 12)))
MANY_SAMPLES_CASES = ((3, 16, 10, 12), (17, 16, 10, 12), (17, 40, 9, 4), (3, 0, 12, 12))
# (n_in, critic, n_hidden, n_out): every form policy_grad_kernel<D, CRITIC, softmax> is compiled in -- the row widths D = 1 .. 12 (the
# small ones are the rows of the small layouts), with and without a critic; hidden units and outputs rotate over the widths
WIDTH_CASES = tuple((D, critic, (16, 5, 0)[D % 3], (12, 4)[D % 2]) for D in range(1, 13) for critic in (True, False))


def _to(c, device):
    """The case of make_case with its tensors on ``device`` (the policy and the critic move themselves)."""
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in c.items()}


def _assert_equal(dev, host):
    for name in NAMES + ("stats",):
        if host[name] is None:
            assert dev[name] is None, name
        else:
            assert torch.equal(dev[name].cpu(), host[name]), (name, dev[name].cpu(), host[name])


def _assert_within_bound(dev, host):
    """|G_dev - G_exact| <= (M + 2) * 2^-53 * sum_s |g_s[p]| / M for every gradient entry and every statistic; G_exact the exact
    sum of the host's per-sample terms over M.  Returns the worst error as a fraction of its bound."""
    from pymgrid_amd import ppo_grad_flat
    worst = 0.0
    for got, terms in ((ppo_grad_flat(dev).cpu(), host["terms"]), (dev["stats"].cpu(), host["stat_terms"])):
        M = terms.shape[0]
        cols = terms.t().tolist()
        assert len(cols) == got.numel()
        for p, col in enumerate(cols):
            exact = math.fsum(col) / M
            bound = (M + 2) * U * math.fsum(abs(v) for v in col) / M
            err = abs(float(got[p]) - exact)
            assert err <= bound, (p, float(got[p]), exact, err, bound)
            worst = max(worst, err / bound if bound else 0.0)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("n_hidden,n_in,n_out,critic", ONE_SAMPLE_CASES)
def test_one_sample_is_exact(device, n_hidden, n_in, n_out, critic):
    from pymgrid_amd import ppo_grad, ppo_grad_host
    c = make_case(1, 1, n_in, n_hidden, n_out, critic=critic, seed=100 + n_hidden + n_out)
    cur = ppo_grad_host(**{**c, "old_probs": torch.ones(1, 1, dtype=F64)}, ratio=True)["ratio"]
    c["old_probs"] = cur / 1.03                                                            # rho ~ 1.03: inside the clip, terms live
    kw = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01, ratio=True)
    host = ppo_grad_host(**c, **kw)
    assert float(host["W2"].abs().sum()) > 0.0 and float(host["stats"][3]) == 0.0
    dev = ppo_grad(**_to(c, device), **kw)
    _assert_equal(dev, host)
    assert torch.equal(dev["ratio"].cpu(), host["ratio"])


@pytest.mark.gpu
@pytest.mark.parametrize("n_in,critic,n_hidden,n_out", WIDTH_CASES)
def test_every_row_width_one_sample_is_exact(device, n_in, critic, n_hidden, n_out):
    test_one_sample_is_exact(device, n_hidden, n_in, n_out, critic)


@pytest.mark.gpu
@pytest.mark.parametrize("n_in,critic,n_hidden,n_out", WIDTH_CASES)
def test_every_row_width_many_samples_within_the_summation_bound(device, n_in, critic, n_hidden, n_out):
    """K = 3, N = 130: three waves, the last with two live lanes."""
    test_many_samples_within_the_summation_bound(device, 3, n_hidden, n_in, n_out, critic)


@pytest.mark.gpu
@pytest.mark.parametrize("K,n_hidden,n_in,n_out", MANY_SAMPLES_CASES)
def test_many_samples_within_the_summation_bound(device, K, n_hidden, n_in, n_out, critic=True):
    """N = 130: three waves, the last with two live lanes; K = 17 crosses chunks of k, the last one partial."""
    from pymgrid_amd import ppo_grad, ppo_grad_host
    c = make_case(K, 130, n_in, n_hidden, n_out, critic=critic, seed=K + n_hidden)
    kw = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01)
    host = ppo_grad_host(**c, **kw, per_sample=True, ratio=True)
    assert host["terms"].shape[0] == K * 130 and 0.0 < float(host["stats"][3]) < 1.0
    cd = _to(c, device)
    dev = ppo_grad(**cd, **kw, ratio=True)
    worst = _assert_within_bound(dev, host)
    print(f"K {K} n_hidden {n_hidden}: worst |G_dev - G_exact| / bound = {worst:.3e}")
    assert torch.equal(dev["ratio"].cpu(), host["ratio"])                                  # (per sample: the host's operations)
    again = ppo_grad(**cd, **kw, ratio=True)
    for name in NAMES + ("stats", "ratio"):
        assert dev[name] is None and again[name] is None or torch.equal(again[name], dev[name]), name


@pytest.mark.gpu
def test_mask(device):
    from pymgrid_amd import ppo_grad, ppo_grad_host
    K, N = 3, 130
    c = make_case(K, N, 10, 16, 12, seed=31)
    mask = torch.rand(K, N, generator=torch.Generator().manual_seed(5)) < 0.6
    kw = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01)
    host = ppo_grad_host(**c, **kw, mask=mask, per_sample=True, ratio=True)
    M = int(mask.sum())
    assert host["terms"].shape[0] == M and 0 < M < K * N
    cd = _to(c, device)
    ratio = torch.full((K, N), -7.0, dtype=F64, device=device)
    dev = ppo_grad(**cd, **kw, mask=mask.to(device), ratio=True, out=dict(ratio=ratio))
    _assert_within_bound(dev, host)
    # M as counted: the clipped fraction is (1 / M) * an integer count, both exact
    assert float(dev["stats"][3]) == (1.0 / M) * float(host["stat_terms"][:, 3].sum())
    got = dev["ratio"].cpu()
    assert torch.equal(got[mask], host["ratio"][mask]) and (got[~mask] == -7.0).all()         # masked samples keep the caller's bytes
    bytes_ = ppo_grad(**cd, **kw, mask=mask.to(device).to(torch.uint8) * 3)                    # any non-zero byte is live
    for name in NAMES + ("stats",):
        assert torch.equal(bytes_[name], dev[name]), name
    none = ppo_grad(**cd, **kw, mask=torch.zeros(K, N, dtype=torch.uint8, device=device))      # M = 0 gives zeros
    assert all((none[n] == 0.0).all() for n in NAMES + ("stats",))


@pytest.mark.gpu
def test_float32_rows_are_widened(device):
    from pymgrid_amd import ppo_grad
    c = _to(make_case(3, 130, 10, 16, 12, seed=37, dtype=F32), device)
    assert c["rows"].dtype == F32
    kw = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01, ratio=True)
    narrow = ppo_grad(**c, **kw)
    wide = ppo_grad(**{**c, "rows": c["rows"].double()}, **kw)
    for name in NAMES + ("stats", "ratio"):
        assert torch.equal(narrow[name], wide[name]), name


@pytest.mark.gpu
@pytest.mark.parametrize("obs_dtype", [F64, F32])
def test_end_to_end_ratio_is_one(device, obs_dtype):
    """What the sampling launch with a critic returns, restarts inside the launch, fed back with the parameters that collected it."""
    from pymgrid_amd import decision_rows, gae, ppo_grad
    from pymgrid_amd.hetero import PerGridWindowEnv
    N, K = 130, 8
    pe = PerGridWindowEnv(_batch(device, "genset+battery+grid", "factorised", N), trajectory_length=5, discrete=True, auto_reset=True,
                          seed=23, obs_dtype=obs_dtype)
    torch.manual_seed(41)
    obs0 = pe.reset().clone()
    policy = _spread_policy(7, obs0, 16, _n_out(pe, True))
    head, sa = _head(9, policy), _sampling(seed=23, temperature=1.3)
    out = pe.rollout_policy(policy, K, sampling=sa, probs=True, critic=head, values=True, observations=True, actions=True, reward=True,
                            done=True)
    assert 0.0 < float(out["done"].double().mean()) < 1.0                                  # restarts fall inside the launch
    assert 0.0 < float((out["probs"] < 1.0).double().mean())
    adv = gae(out["reward"], out["done"], out["values"], out["last_value"], out["final_values"])["advantages"]
    rows = decision_rows(obs0, out["obs"])
    assert rows.dtype == obs_dtype and out["actions"].dtype == torch.uint8
    res = ppo_grad(policy, head, rows, out["actions"], out["probs"], adv, returns=out["values"], sampling=sa, ent_coef=0.01, ratio=True)
    assert (res["ratio"] == 1.0).all()
    assert float(res["stats"][1]) == 0.0 and (res["w"] == 0.0).all() and (res["b"] == 0.0).all()
    assert float(res["stats"][3]) == 0.0 and float(res["W2"].abs().sum()) > 0.0
    pe.env.close()


@pytest.mark.gpu
def test_refusals_of_the_c_abi(device):
    """Every refusal of mgx_policy_grad with its code; nothing is launched: the outputs keep the caller's bytes."""
    from pymgrid_amd import _lib
    lib = _lib.lib()
    K, N = 2, 5
    c = _to(make_case(K, N, 6, 5, 4, seed=41), device)
    nan = float("nan")
    outs = {n: torch.full((64,), nan, dtype=F64, device=device) for n in ("g_w1", "g_b1", "g_w2", "g_b2", "g_cw", "g_cb", "stats", "ratio_out")}
    ws = torch.zeros(1 << 16, dtype=F64, device=device)
    z = torch.zeros(4096, dtype=F64, device=device)
    idx = torch.zeros(N, dtype=torch.int32, device=device)
    INV, UNS = _lib.MGX_ERR_INVALID, _lib.MGX_ERR_UNSUPPORTED

    def call(pol_kw=None, pg_kw=None, critic=True, n=N, k=K, null_pg=False, crit_kw=None):
        pol, keep = c["policy"].c_struct(device, N)
        for key, v in (pol_kw or {}).items():
            setattr(pol, key, v)
        smp, keep_s = c["sampling"].c_struct(device, N)
        cr, keep_c = c["critic"].c_struct(device, N)
        for key, v in (crit_kw or {}).items():
            setattr(cr, key, v)
        pg = _lib.PolicyGrad()
        pg.struct_size = C.sizeof(_lib.PolicyGrad)
        pg.x, pg.action_id, pg.old_prob, pg.advantage = (c[q].data_ptr() for q in ("rows", "actions", "old_probs", "advantages"))
        pg.returns = c["returns"].data_ptr() if critic else None
        pg.clip_eps, pg.vf_coef, pg.ent_coef = 0.2, 0.5, 0.01
        for name, t in outs.items():
            setattr(pg, name, t.data_ptr() if critic or name not in ("g_cw", "g_cb") else None)
        pg.workspace, pg.workspace_bytes = ws.data_ptr(), ws.numel() * 8
        for key, v in (pg_kw or {}).items():
            setattr(pg, key, v)
        return lib.mgx_policy_grad(n, k, C.byref(pol), C.byref(cr) if critic else None, C.byref(smp), None if null_pg else C.byref(pg), None)

    need = C.c_int64()
    pol, keep = c["policy"].c_struct(device, N)
    assert lib.mgx_policy_grad_workspace(N, K, C.byref(pol), C.byref(need)) == _lib.MGX_OK and 0 < need.value <= ws.numel() * 8
    refused = [
        (INV, dict(null_pg=True)), (INV, dict(pg_kw=dict(struct_size=8))), (INV, dict(n=0)), (INV, dict(k=0)),
        (INV, dict(pol_kw=dict(n_out=13))), (INV, dict(pol_kw=dict(n_in=13))), (INV, dict(pol_kw=dict(n_in=0))),
        (INV, dict(pg_kw=dict(clip_eps=nan))), (INV, dict(pg_kw=dict(clip_eps=-0.1))), (INV, dict(pg_kw=dict(vf_coef=nan))),
        (INV, dict(pg_kw=dict(ent_coef=nan))), (INV, dict(critic=False, pg_kw=dict(g_cw=z.data_ptr()))),
        (INV, dict(critic=False, pg_kw=dict(g_cb=z.data_ptr()))), (INV, dict(critic=False, pg_kw=dict(returns=z.data_ptr()))),
        (INV, dict(pg_kw=dict(returns=None))), (INV, dict(pg_kw=dict(workspace_bytes=need.value - 8))),
        (INV, dict(pg_kw=dict(workspace=None))), (INV, dict(pg_kw=dict(x=None))), (INV, dict(crit_kw=dict(struct_size=4))),
        (INV, dict(pol_kw=dict(struct_size=4))),
        (UNS, dict(pol_kw=dict(n_policies=2))), (UNS, dict(pol_kw=dict(policy_index=idx.data_ptr()))),
        (UNS, dict(pol_kw=dict(n_hidden=_lib.POLICY_MAX_HIDDEN + 1))),
    ]
    for code, kw in refused:
        assert call(**kw) == code, (code, kw, lib.mgx_last_error())
        assert lib.mgx_last_error()
    torch.cuda.synchronize(device)
    assert all(bool(torch.isnan(t).all()) for t in outs.values())                          # nothing was launched
    for code, kw in ((INV, dict(n=0)), (INV, dict(k=0)), (INV, dict(n_out=13)), (UNS, dict(n_policies=2))):
        pol, keep = c["policy"].c_struct(device, N)
        for key, v in kw.items():
            if key not in ("n", "k"):
                setattr(pol, key, v)
        assert lib.mgx_policy_grad_workspace(kw.get("n", N), kw.get("k", K), C.byref(pol), C.byref(need)) == code
    assert lib.mgx_policy_grad_workspace(N, K, C.byref(pol), None) == INV
    assert call() == _lib.MGX_OK and call(critic=False) == _lib.MGX_OK                      # ... and the same structs untouched are taken
    torch.cuda.synchronize(device)
    assert not bool(torch.isnan(outs["stats"][:4]).any())
