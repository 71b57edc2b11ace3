"""``ppo_grad_gaussian`` (mgx_policy_grad_gaussian: policy_grad_kernel with the Gaussian head + policy_grad_finish_kernel) against
``ppo_grad_gaussian_host``, the host statement of the rule of include/mgx.h.  One live sample is exact (``==``): a product added to
zeros.  Many samples are held to the any-order summation bound against the exactly summed per-sample terms (math.fsum) and must be
identical from run to run.  End to end: on the data of a Gaussian launch with a critic, restarts inside, the ratio equals the host's
bit for bit and stays inside the derived bound, and with ``returns = values`` the critic's gradient is exactly 0.0.  WIDTH_CASES runs
the first two once per compiled form of the kernel: every row width 1 .. 12, with and without a critic."""
import ctypes as C

import pytest
import torch

from test_policy_gaussian import _head
from test_policy_grad import _assert_within_bound, _to
from test_policy_grad_gaussian_host import make_case_gaussian, ratio_bound
from test_policy_rollout import _batch, _policy

F64, F32 = torch.float64, torch.float32
NAMES = ("W1", "b1", "W2", "b2", "w", "b", "log_sigma")
KW = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01)


def _cpu(c):
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in c.items()}


ONE_SAMPLE_CASES = tuple((nh, n_in, A, critic) for critic in (True, False) for A in (4, 3, 1) for nh, n_in in ((16, 10), (5, 7), (0, 12)))
MANY_SAMPLES_CASES = ((3, 16, 10, 4, False), (17, 16, 10, 4, True), (17, 40, 9, 3, False), (3, 0, 12, 3, True), (17, 0, 12, 4, False))
# (n_in, critic, n_hidden, A): every form policy_grad_kernel<D, CRITIC, Gaussian> is compiled in -- the row widths D = 1 .. 12, with and
# without a critic; hidden units and the number of controls rotate over the widths (in this order of A every one-sample case is live
# on the host; with (4, 3, 2, 1) the sample of D = 4 leaves its five hidden units dead and W2's gradient zero)
WIDTH_CASES = tuple((D, critic, (16, 5, 0)[D % 3], (3, 4, 1, 2)[D % 4]) for D in range(1, 13) for critic in (True, False))


@pytest.mark.gpu
@pytest.mark.parametrize("n_in,critic,n_hidden,A", WIDTH_CASES)
def test_every_row_width_one_sample_is_exact(device, n_in, critic, n_hidden, A):
    test_one_sample_is_exact(device, n_hidden, n_in, A, critic)


@pytest.mark.gpu
@pytest.mark.parametrize("n_in,critic,n_hidden,A", WIDTH_CASES)
def test_every_row_width_many_samples_within_the_summation_bound(device, n_in, critic, n_hidden, A):
    """K = 3, N = 130: three waves, the last with two live lanes."""
    test_many_samples_within_the_summation_bound(device, 3, n_hidden, n_in, A, False, critic)


@pytest.mark.gpu
@pytest.mark.parametrize("n_hidden,n_in,A,critic", ONE_SAMPLE_CASES)
def test_one_sample_is_exact(device, n_hidden, n_in, A, critic):
    from pymgrid_amd import ppo_grad_gaussian, ppo_grad_gaussian_host
    c = make_case_gaussian(1, 1, n_in, n_hidden, A, critic=critic, seed=100 + n_hidden + A)
    # old_logp from the rule's own ratio: rho(old = 0) = E(logp), so old = log(rho0 / 1.03) puts rho near 1.03 -- inside the clip
    rho0 = ppo_grad_gaussian_host(**{**c, "old_logp": torch.zeros(1, 1, dtype=F64)}, ratio=True)["ratio"]
    c["old_logp"] = torch.log(rho0 / 1.03)
    host = ppo_grad_gaussian_host(**c, **KW, ratio=True)
    assert abs(float(host["ratio"]) - 1.03) < 1e-9 and float(host["W2"].abs().sum()) > 0.0 and float(host["stats"][3]) == 0.0
    assert (host["log_sigma"][:A] != 0.0).all() and (host["log_sigma"][A:] == 0.0).all()
    dev = ppo_grad_gaussian(**_to(c, device), **KW, ratio=True)
    for name in NAMES + ("stats", "ratio"):
        if host[name] is None:
            assert dev[name] is None, name
        else:
            assert torch.equal(dev[name].cpu(), host[name]), (name, dev[name].cpu(), host[name])


@pytest.mark.gpu
@pytest.mark.parametrize("K,n_hidden,n_in,A,dead", MANY_SAMPLES_CASES)
def test_many_samples_within_the_summation_bound(device, K, n_hidden, n_in, A, dead, critic=True):
    """N = 130: three waves, the last with two live lanes; K = 17 crosses chunks of k, the last one partial.  ``dead``: a column with
    sigma 0 and a scale ladder with zeros (grids without a live column)."""
    from pymgrid_amd import ppo_grad_gaussian, ppo_grad_gaussian_host
    N = 130
    sigma = (0.3, 0.0, 0.2, 0.05) if dead else (0.3, 0.1, 0.2, 0.05)
    scale = (torch.arange(N, dtype=F64) % 5) * 0.5 if dead else None                        # 0.0, 0.5, .. 2.0: every fifth grid is off
    c = make_case_gaussian(K, N, n_in, n_hidden, A, critic=critic, seed=K + n_hidden, sigma=sigma, scale=scale)
    host = ppo_grad_gaussian_host(**c, **KW, per_sample=True, ratio=True)
    assert host["terms"].shape[0] == K * N and 0.0 < float(host["stats"][3]) < 1.0
    if dead:
        assert float(host["log_sigma"][1]) == 0.0 and (host["stat_terms"][::5, 0] == 0.0).all()
    cd = _to(c, device)
    dev = ppo_grad_gaussian(**cd, **KW, ratio=True)
    worst = _assert_within_bound(dev, host)
    print(f"K {K} n_hidden {n_hidden} A {A} dead {dead}: worst |G_dev - G_exact| / bound = {worst:.3e}")
    assert torch.equal(dev["ratio"].cpu(), host["ratio"])                                  # (per sample: the host's operations)
    if dead:
        assert float(dev["log_sigma"][1]) == 0.0 and (dev["W2"][1] == 0.0).all()
    assert (dev["log_sigma"][A:] == 0.0).all()
    again = ppo_grad_gaussian(**cd, **KW, ratio=True)
    for name in NAMES + ("stats", "ratio"):
        assert dev[name] is None and again[name] is None or torch.equal(again[name], dev[name]), name


@pytest.mark.gpu
def test_mask(device):
    from pymgrid_amd import ppo_grad_gaussian, ppo_grad_gaussian_host
    K, N = 3, 130
    c = make_case_gaussian(K, N, 10, 16, 4, seed=31)
    mask = torch.rand(K, N, generator=torch.Generator().manual_seed(5)) < 0.6
    host = ppo_grad_gaussian_host(**c, **KW, mask=mask, per_sample=True, ratio=True)
    M = int(mask.sum())
    assert host["terms"].shape[0] == M and 0 < M < K * N
    cd = _to(c, device)
    ratio = torch.full((K, N), -7.0, dtype=F64, device=device)
    dev = ppo_grad_gaussian(**cd, **KW, mask=mask.to(device), ratio=True, out=dict(ratio=ratio))
    _assert_within_bound(dev, host)
    # M as counted: the clipped fraction is (1 / M) * an integer count, both exact
    assert float(dev["stats"][3]) == (1.0 / M) * float(host["stat_terms"][:, 3].sum())
    got = dev["ratio"].cpu()
    assert torch.equal(got[mask], host["ratio"][mask]) and (got[~mask] == -7.0).all()         # masked samples keep the caller's bytes
    bytes_ = ppo_grad_gaussian(**cd, **KW, mask=mask.to(device).to(torch.uint8) * 3)           # any non-zero byte is live
    for name in NAMES + ("stats",):
        assert torch.equal(bytes_[name], dev[name]), name
    none = ppo_grad_gaussian(**cd, **KW, mask=torch.zeros(K, N, dtype=torch.uint8, device=device))      # M = 0 gives zeros
    assert all((none[n] == 0.0).all() for n in NAMES + ("stats",))


@pytest.mark.gpu
def test_float32_rows_are_widened(device):
    from pymgrid_amd import ppo_grad_gaussian
    c = _to(make_case_gaussian(3, 130, 10, 16, 4, seed=37, dtype=F32), device)
    assert c["rows"].dtype == F32
    narrow = ppo_grad_gaussian(**c, **KW, ratio=True)
    wide = ppo_grad_gaussian(**{**c, "rows": c["rows"].double()}, **KW, ratio=True)
    for name in NAMES + ("stats", "ratio"):
        assert torch.equal(narrow[name], wide[name]), name


@pytest.mark.gpu
@pytest.mark.parametrize("obs_dtype", [F64, F32])
def test_end_to_end_on_a_gaussian_collection(device, obs_dtype):
    """What the Gaussian launch with a critic returns, restarts inside the launch, fed back with the parameters that collected it."""
    from pymgrid_amd import GaussianSampling, decision_rows, gae, ppo_grad_gaussian, ppo_grad_gaussian_host
    from pymgrid_amd.hetero import PerGridWindowEnv
    N, K = 130, 8
    pe = PerGridWindowEnv(_batch(device, "genset+battery+grid", "factorised", N), trajectory_length=5, discrete=False, auto_reset=True,
                          seed=23, obs_dtype=obs_dtype)
    torch.manual_seed(41)
    obs0 = pe.reset().clone()
    D, A = pe.env.engine.obs_dim, pe.env.engine.action_dim
    assert A == 4
    policy = _policy(7, D, 16, A, "continuous")
    head, gs = _head(9, policy), GaussianSampling(23, [0.3, 0.1, 0.2, 0.05])
    out = pe.step_k_policy(policy, K, sampling=gs, critic=head, values=True, observations=True, raw_actions=True, logp=True, reward=True,
                           done=True)
    assert 0.0 < float(out["done"].double().mean()) < 1.0                                  # restarts fall inside the launch
    adv = gae(out["reward"], out["done"], out["values"], out["last_value"], out["final_values"])["advantages"]
    rows = decision_rows(obs0, out["obs"])
    assert rows.dtype == obs_dtype and out["raw_actions"].shape == (K, N, A)
    args = (policy, head, rows, out["raw_actions"], out["logp"], adv)
    res = ppo_grad_gaussian(*args, returns=out["values"], sampling=gs, ent_coef=0.01, ratio=True)
    host = ppo_grad_gaussian_host(*(t.cpu() if torch.is_tensor(t) else t for t in args), returns=out["values"].cpu(), sampling=gs,
                                  ent_coef=0.01, ratio=True)
    rho = res["ratio"].cpu()
    assert torch.equal(rho, host["ratio"])
    bound = ratio_bound(policy, gs, rows.cpu().reshape(K * N, D), out["raw_actions"].cpu().reshape(K * N, A),
                        out["logp"].cpu().reshape(K * N)).reshape(K, N)
    print(f"worst |rho - 1| / bound = {float(((rho - 1.0).abs() / bound).max()):.3f}")
    assert ((rho - 1.0).abs() <= bound).all()
    assert float(res["stats"][1]) == 0.0 and (res["w"] == 0.0).all() and (res["b"] == 0.0).all()
    assert float(res["stats"][3]) == 0.0
    assert float(res["W2"].abs().sum()) > 0.0 and (res["log_sigma"] != 0.0).all()
    pe.env.close()


@pytest.mark.gpu
def test_refusals_of_the_c_abi(device):
    """Every refusal of mgx_policy_grad_gaussian with its code; nothing is launched: the outputs keep the caller's bytes.  A call
    through ``ppo_grad`` with the discrete head is what it was."""
    from pymgrid_amd import _lib, ppo_grad, ppo_grad_host
    from test_policy_grad_host import make_case
    lib = _lib.lib()
    K, N = 2, 5
    c = _to(make_case_gaussian(K, N, 6, 5, 4, seed=41), device)
    nan = float("nan")
    outs = {n: torch.full((64,), nan, dtype=F64, device=device)
            for n in ("g_w1", "g_b1", "g_w2", "g_b2", "g_cw", "g_cb", "g_log_sigma", "stats", "ratio_out")}
    ws = torch.zeros(1 << 16, dtype=F64, device=device)
    z = torch.zeros(4096, dtype=F64, device=device)
    idx = torch.zeros(N, dtype=torch.int32, device=device)
    INV, UNS = _lib.MGX_ERR_INVALID, _lib.MGX_ERR_UNSUPPORTED

    def call(pol_kw=None, pg_kw=None, critic=True, n=N, k=K, null_pg=False, crit_kw=None, gs_kw=None, sigma=None, null_gs=False):
        pol, keep = c["policy"].c_struct(device, N)
        for key, v in (pol_kw or {}).items():
            setattr(pol, key, v)
        smp, keep_s = c["sampling"].c_struct(device, N)
        for key, v in (gs_kw or {}).items():
            setattr(smp, key, v)
        if sigma is not None:
            smp.sigma[sigma[0]] = sigma[1]
        cr, keep_c = c["critic"].c_struct(device, N)
        for key, v in (crit_kw or {}).items():
            setattr(cr, key, v)
        pg = _lib.PolicyGradGaussian()
        pg.struct_size = C.sizeof(_lib.PolicyGradGaussian)
        pg.x, pg.raw_action, pg.old_logp, pg.advantage = (c[q].data_ptr() for q in ("rows", "raw_actions", "old_logp", "advantages"))
        pg.returns = c["returns"].data_ptr() if critic else None
        pg.clip_eps, pg.vf_coef, pg.ent_coef = 0.2, 0.5, 0.01
        for name, t in outs.items():
            setattr(pg, name, t.data_ptr() if critic or name not in ("g_cw", "g_cb") else None)
        pg.workspace, pg.workspace_bytes = ws.data_ptr(), ws.numel() * 8
        for key, v in (pg_kw or {}).items():
            setattr(pg, key, v)
        return lib.mgx_policy_grad_gaussian(n, k, C.byref(pol), C.byref(cr) if critic else None, None if null_gs else C.byref(smp),
                                            None if null_pg else C.byref(pg), None)

    need = C.c_int64()
    pol, keep = c["policy"].c_struct(device, N)
    assert lib.mgx_policy_grad_workspace(N, K, C.byref(pol), C.byref(need)) == _lib.MGX_OK and 0 < need.value <= ws.numel() * 8
    refused = [
        # everything mgx_policy_grad refuses
        (INV, dict(null_pg=True)), (INV, dict(pg_kw=dict(struct_size=8))), (INV, dict(n=0)), (INV, dict(k=0)),
        (INV, dict(pol_kw=dict(n_out=13))), (INV, dict(pol_kw=dict(n_in=13))), (INV, dict(pol_kw=dict(n_in=0))),
        (INV, dict(pg_kw=dict(clip_eps=nan))), (INV, dict(pg_kw=dict(clip_eps=-0.1))), (INV, dict(pg_kw=dict(vf_coef=nan))),
        (INV, dict(pg_kw=dict(ent_coef=nan))), (INV, dict(critic=False, pg_kw=dict(g_cw=z.data_ptr()))),
        (INV, dict(critic=False, pg_kw=dict(g_cb=z.data_ptr()))), (INV, dict(critic=False, pg_kw=dict(returns=z.data_ptr()))),
        (INV, dict(pg_kw=dict(returns=None))), (INV, dict(pg_kw=dict(workspace_bytes=need.value - 8))),
        (INV, dict(pg_kw=dict(workspace=None))), (INV, dict(pg_kw=dict(x=None))), (INV, dict(pg_kw=dict(advantage=None))),
        (INV, dict(pg_kw=dict(x_f32=2))), (INV, dict(crit_kw=dict(struct_size=4))), (INV, dict(crit_kw=dict(w=None))),
        (INV, dict(pol_kw=dict(struct_size=4))), (INV, dict(pol_kw=dict(w2=None))),
        (UNS, dict(pol_kw=dict(n_policies=2))), (UNS, dict(pol_kw=dict(policy_index=idx.data_ptr()))),
        (UNS, dict(pol_kw=dict(n_hidden=_lib.POLICY_MAX_HIDDEN + 1))),
        # the mgx_gaussian checks of the Gaussian launch
        (INV, dict(null_gs=True)), (INV, dict(gs_kw=dict(struct_size=8))), (INV, dict(sigma=(0, -0.1))), (INV, dict(sigma=(1, nan))),
        (INV, dict(sigma=(2, float("inf")))), (INV, dict(sigma=(3, 1e-310))),
        # ... and this call's own
        (INV, dict(pol_kw=dict(n_out=5))), (INV, dict(pol_kw=dict(n_out=0))), (INV, dict(pg_kw=dict(raw_action=None))),
        (INV, dict(pg_kw=dict(old_logp=None))),
    ]
    for code, kw in refused:
        assert call(**kw) == code, (code, kw, lib.mgx_last_error())
        assert lib.mgx_last_error()
    torch.cuda.synchronize(device)
    assert all(bool(torch.isnan(t).all()) for t in outs.values())                          # nothing was launched
    assert call() == _lib.MGX_OK and call(critic=False) == _lib.MGX_OK                      # ... and the same structs untouched are taken
    assert call(pg_kw=dict(g_log_sigma=None, stats=None, ratio_out=None)) == _lib.MGX_OK     # (every output may be NULL)
    torch.cuda.synchronize(device)
    assert not bool(torch.isnan(outs["stats"][:5]).any()) and not bool(torch.isnan(outs["g_log_sigma"][:4]).any())
    assert bool(torch.isnan(outs["stats"][5:]).all()) and bool(torch.isnan(outs["g_log_sigma"][4:]).all())
    # the discrete call beside it: one sample stays exact, stats stays [4]
    d = make_case(1, 1, 10, 16, 12, seed=128)
    host = ppo_grad_host(**d, clip=0.2, vf_coef=0.5, ent_coef=0.01)
    dev = ppo_grad(**_to(d, device), clip=0.2, vf_coef=0.5, ent_coef=0.01)
    assert dev["stats"].shape == (4,) and "log_sigma" not in dev
    for name in ("W1", "b1", "W2", "b2", "w", "b", "stats"):
        assert torch.equal(dev[name].cpu(), host[name]), name
