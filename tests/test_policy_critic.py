"""A critic beside the actor of the sampling launch (mgx_rollout_policy_critic_episodes, ``critic=`` / ``values=`` of
StepEngine.rollout_policy_episodes and PerGridWindowEnv.rollout_policy) and the advantages on the device (mgx_gae, ``pymgrid_amd.gae``):
the rules of ``mgx_critic`` and ``mgx_gae`` (include/mgx.h) on the host (``ValueHead.value``, ``gae_host``) against scalar Python
loops, and the kernels against those host statements bit for bit (torch.equal / _same_bits: both rules are fixed sequences of IEEE
operations on both sides, so there is no tolerance).  The forms of the kernels these cases leave out -- all ten layouts x the three row sources -- run in
tests/test_layout_matrix_policy.py, which also replays the launches on the CPU oracle."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from test_episode_rows import HostStats, _same_bits, _snapshot, _state_equal, _untouched
from test_policy_explore import DOCUMENTED as EXPLORE_DOCUMENTED
from test_policy_explore import _compare, _envs_equal, _forms_of
from test_policy_rollout import DOCUMENTED as GREEDY_DOCUMENTED
from test_policy_rollout import WANT, _batch, _c_policy, _n_out, _policy, _trace_end, _trace_launch, _trace_start
from test_policy_sample import CASES, LAUNCHES, LENGTH, N, T
from test_policy_sample import DOCUMENTED as SAMPLE_DOCUMENTED
from test_policy_sample import _envs, _nan_rows, _rows, _sampling, _spread_policy, _twin_steps

F64, F32 = torch.float64, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = ("values", "final_values", "last_value")
CORNERS = [(0.99, 0.95), (1.0, 1.0), (0.0, 0.0), (0.9, 0.0), (1.0, 0.0)]


def _head(seed, policy):
    """A ValueHead of random parameters on the trunk of ``policy``."""
    from pymgrid_amd import ValueHead
    rng = np.random.default_rng(seed)
    P, n_mid = policy.n_policies, policy.n_hidden or policy.n_in
    return ValueHead(rng.normal(0.0, 1.0, size=(P, n_mid)), rng.normal(0.0, 0.5, size=(P,)))


# ---- CPU: the rule of mgx_critic on the host ----------------------------------------------------------------------------------------
def _scalar_value(policy, head, obs):
    """V row by row in Python floats (IEEE doubles, one multiply and one add at a time), straight from the rule in include/mgx.h."""
    P = policy.n_policies
    out = []
    for n in range(obs.shape[0]):
        ps = 0 if policy.policy_index is None else int(policy.policy_index[n])
        ps = ps if 0 <= ps < P else 0
        v = [float(obs[n, j]) for j in range(obs.shape[1])]            # (a float32 value widens exactly)
        if policy.n_hidden:
            hid = []
            for u in range(policy.n_hidden):
                h = float(policy.b1[ps, u])
                for j in range(policy.n_in):
                    h = h + float(policy.W1[ps, u, j]) * v[j]
                hid.append(h if h > 0.0 else 0.0)
            v = hid
        V = float(head.b[ps])
        for j in range(len(v)):
            V = V + float(head.w[ps, j]) * v[j]
        out.append(V)
    return torch.tensor(out, dtype=F64)


@pytest.mark.parametrize("n_hidden", [0, 3])
@pytest.mark.parametrize("obs_dtype", [F64, F32])
def test_value_head_is_the_scalar_rule(n_hidden, obs_dtype):
    n, n_in, P = 5, 8, 2
    index = torch.tensor([-1, 0, 1, P, 1], dtype=torch.int32)
    policy = _policy(3, n_in, n_hidden, 6, "discrete", P=P, index=index)
    head = _head(4, policy)
    obs = _rows(n, n_in).to(obs_dtype)
    got = head.value(policy, obs)
    assert got.dtype == F64 and got.shape == (n,)
    assert torch.equal(got, _scalar_value(policy, head, obs))
    # the out-of-range indices take set 0, the others their own: the sets really differ
    zero = _head(4, policy)
    assert torch.equal(got[[0, 1, 3]], head.value(_policy(3, n_in, n_hidden, 6, "discrete", P=P), obs)[[0, 1, 3]])
    assert not torch.equal(got[[2, 4]], head.value(_policy(3, n_in, n_hidden, 6, "discrete", P=P), obs)[[2, 4]])
    assert zero.n_mid == (n_hidden or n_in) and zero.n_policies == P
    # one set, parameters without the population axis
    from pymgrid_amd import ValueHead
    one = _policy(5, n_in, n_hidden, 6, "discrete")
    h1 = ValueHead(head.w[0].numpy(), np.float64(head.b[0]))
    assert torch.equal(h1.value(one, obs), _scalar_value(one, h1, obs))


# ---- CPU: the rule of mgx_gae on the host -------------------------------------------------------------------------------------------
def _scalar_gae(reward, done, value, last_value, final_value, gamma, lam):
    K, n = reward.shape
    c = gamma * lam
    adv, ret = torch.empty(K, n, dtype=F64), torch.empty(K, n, dtype=F64)
    for i in range(n):
        nxt, carry = float(last_value[i]), 0.0
        for k in range(K - 1, -1, -1):
            d = bool(done[k, i] != 0)
            nv = (float(final_value[k, i]) if final_value is not None else 0.0) if d else nxt
            delta = (float(reward[k, i]) + gamma * nv) - float(value[k, i])
            A = delta if d else delta + c * carry
            adv[k, i], ret[k, i] = A, A + float(value[k, i])
            carry, nxt = A, float(value[k, i])
    return adv, ret


def _hand_made_done(K):
    """[K, 5] bool: no done; all; only k = 0; only k = K - 1; two in a row (as far as K allows)."""
    d = torch.zeros(K, 5, dtype=torch.bool)
    d[:, 1] = True
    d[0, 2] = True
    d[K - 1, 3] = True
    d[K // 2, 4] = True
    d[min(K // 2 + 1, K - 1), 4] = True
    return d


def _gae_inputs(K, n, seed, device="cpu", integers=False):
    """Seeded inputs: ``done`` drawn at rate 1 / 24, its first five columns (as many as n allows) the hand-made ones; ``final_value``
    holds NaN wherever ``done`` is not set -- the rule never reads it there."""
    g = torch.Generator().manual_seed(seed)
    draw = (lambda *s: torch.randint(-4, 5, s, generator=g).to(F64)) if integers else (lambda *s: torch.randn(*s, generator=g, dtype=F64))
    reward, value, last_value, fv = draw(K, n), draw(K, n), draw(n), draw(K, n)
    done = torch.rand(K, n, generator=g) < 1.0 / 24.0
    m = min(n, 5)
    done[:, :m] = _hand_made_done(K)[:, :m]
    fv = torch.where(done, fv, torch.full_like(fv, float("nan")))
    return tuple(t.to(device) for t in (reward, done, value, last_value, fv))


@pytest.mark.parametrize("gamma,lam", CORNERS)
@pytest.mark.parametrize("with_final", [True, False])
def test_gae_host_is_the_scalar_rule(gamma, lam, with_final):
    from pymgrid_amd.policy import gae_host
    reward, done, value, last_value, fv = _gae_inputs(5, 7, seed=1)
    assert bool(done[:, 0].sum() == 0) and bool(done[:, 1].all()) and done[:, 2].tolist() == [True, False, False, False, False]
    assert done[:, 3].tolist() == [False, False, False, False, True] and done[:, 4].tolist() == [False, False, True, True, False]
    fv = fv if with_final else None
    adv, ret = _scalar_gae(reward, done, value, last_value, fv, gamma, lam)
    for d in (done, done.to(torch.uint8)):
        got = gae_host(reward, d, value, last_value, final_value=fv, gamma=gamma, lam=lam)
        assert set(got) == {"advantages", "returns"}
        assert torch.equal(got["advantages"], adv) and torch.equal(got["returns"], ret)


def test_gae_host_exact_cases_on_small_integers():
    from pymgrid_amd.policy import gae_host
    K, n = 5, 7
    reward, done, value, last_value, fv = _gae_inputs(K, n, seed=2, integers=True)
    fv0 = torch.where(done, fv, torch.zeros_like(fv))
    # lam = 0: the one-step advantage A = r + gamma * nv - v (gamma = 0.5: exact on small integers)
    got = gae_host(reward, done, value, last_value, final_value=fv, gamma=0.5, lam=0.0)
    nxt = torch.cat([value[1:], last_value[None]])
    nv = torch.where(done, fv0, nxt)
    assert torch.equal(got["advantages"], reward + 0.5 * nv - value)
    assert torch.equal(got["returns"], reward + 0.5 * nv)
    # gamma = lam = 1 without a done: returns[k] = the rewards from k on + last_value
    none = torch.zeros_like(done)
    got = gae_host(reward, none, value, last_value, gamma=1.0, lam=1.0)
    assert torch.equal(got["returns"], reward.flip(0).cumsum(0).flip(0) + last_value)
    # final_value=None bootstraps 0.0 at done: a column that is done at every step
    got = gae_host(reward, done, value, last_value, final_value=None, gamma=1.0, lam=1.0)
    assert torch.equal(got["advantages"][:, 1], reward[:, 1] - value[:, 1]) and torch.equal(got["returns"][:, 1], reward[:, 1])
    # a NaN in advantage[k + 1] does not reach advantage[k] when done[k]
    bad = reward.clone()
    bad[3, 4] = float("nan")                                      # (column 4 is done at k = 2 and 3)
    got = gae_host(bad, done, value, last_value, final_value=fv, gamma=1.0, lam=1.0)
    assert bool(torch.isnan(got["advantages"][3, 4])) and not bool(torch.isnan(got["advantages"][:3, 4]).any())
    bad = reward.clone()
    bad[3, 0] = float("nan")                                      # (column 0 is never done: the NaN runs on)
    got = gae_host(bad, done, value, last_value, final_value=fv, gamma=1.0, lam=1.0)
    assert bool(torch.isnan(got["advantages"][:4, 0]).all()) and not bool(torch.isnan(got["advantages"][4, 0]))


# ---- CPU: validation, signatures, layout, the C entries -----------------------------------------------------------------------------
class _NoLaunch:
    """An engine stand-in for the checks StepEngine.rollout_policy_episodes makes before it touches a handle."""
    N, device = 4, torch.device("cpu")


def test_validation_errors():
    from pymgrid_amd import ValueHead, gae
    from pymgrid_amd.engine import StepEngine
    from pymgrid_amd.hetero import PerGridWindowEnv
    from pymgrid_amd.policy import gae_host
    for w, b in ((np.zeros(4, dtype=np.float32), np.float64(0)), (np.zeros(4), np.float32(0)), (np.zeros((2, 4)), np.zeros(3)),
                 (np.zeros((2, 2, 4)), np.zeros(2)), (np.zeros((1, 0)), np.zeros(1)), (np.zeros(4), np.zeros((1, 1))), (None, np.float64(0)),
                 (np.zeros(4), None)):
        with pytest.raises(ValueError):
            ValueHead(w, b)
    pol = _policy(7, 8, 3, 6, "discrete", P=2)
    good = _head(1, pol)
    st, keep = good.c_struct(torch.device("cpu"), 4)
    assert st.struct_size == C.sizeof(type(st)) == 8 + 2 * C.sizeof(C.c_void_p) and st.w == keep[0].data_ptr() and st.b == keep[1].data_ptr()
    assert good.lds_bytes(pol) == pol.lds_bytes + 2 * (1 + 3 + 0) * 8          # (1 + n_mid doubles per set; both sets stay even)
    for other in (_policy(7, 8, 4, 6, "discrete", P=2), _policy(7, 8, 3, 6, "discrete", P=1), _policy(7, 8, 0, 6, "discrete", P=2),
                  _policy(7, 8, 3, 4, "continuous", P=2)):
        with pytest.raises(ValueError):
            good.value(other, _rows(4, 8))
    with pytest.raises(ValueError):
        good.value(pol, _rows(4, 7))
    # critic= without sampling=, values= without critic=: refused before anything touches a handle
    with pytest.raises(ValueError, match=r"Sampling\(seed, temperature=0\)"):
        StepEngine.rollout_policy_episodes(_NoLaunch(), pol, None, 4, critic=good)
    with pytest.raises(ValueError, match=r"Sampling\(seed, temperature=0\)"):
        StepEngine._launch_policy_episodes(_NoLaunch(), "mgx_rollout_policy_episodes", pol, None, (), 4, {}, (), None, None, {}, False, False,
                                           critic=good)
    with pytest.raises(ValueError, match="critic="):
        StepEngine.rollout_policy_episodes(_NoLaunch(), pol, None, 4, sampling=_sampling(), values=True)
    with pytest.raises(ValueError, match="values names"):
        StepEngine.rollout_policy_episodes(_NoLaunch(), pol, None, 4, sampling=_sampling(), critic=good, values=("value",))
    for fn in (StepEngine.rollout_policy_episodes, PerGridWindowEnv.rollout_policy):
        par = inspect.signature(fn).parameters
        assert par["critic"].default is None and par["values"].default is False
    for fn in (StepEngine.step_k_policy_episodes, PerGridWindowEnv.step_k_policy):
        assert "critic" not in inspect.signature(fn).parameters
    par = inspect.signature(gae).parameters
    assert list(par) == ["reward", "done", "value", "last_value", "final_value", "gamma", "lam", "out"]
    assert (par["final_value"].default, par["gamma"].default, par["lam"].default, par["out"].default) == (None, 0.99, 0.95, None)
    # gae / gae_host: dtype, shape, contiguity, the range of gamma and lambda
    r, d, v, lv, fv = _gae_inputs(5, 7, seed=1)
    for fn in (gae, gae_host):
        for bad in (dict(reward=r.float()), dict(value=v.float()), dict(last_value=lv.float()), dict(final_value=fv.float()),
                    dict(done=d.to(torch.int32)), dict(done=d[:4]), dict(value=v[:, :6]), dict(last_value=lv[:6]), dict(final_value=fv[:4]),
                    dict(reward=r[0], done=d[0], value=v[0]), dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float("nan")), dict(lam=-0.1),
                    dict(lam=1.0001), dict(lam=float("nan"))):
            kw = dict(reward=r, done=d, value=v, last_value=lv, final_value=fv)
            kw.update(bad)
            with pytest.raises(ValueError):
                fn(**kw)
    with pytest.raises(ValueError, match="contiguous"):
        gae(r.t().contiguous().t(), d, v, lv)
    with pytest.raises(ValueError, match="contiguous"):
        gae(r, d, v.t().contiguous().t(), lv)
    with pytest.raises(ValueError, match="GPU"):
        gae(r, d, v, lv)                                          # (host tensors: gae_host is the rule anywhere)


def test_symbols_struct_and_header():
    from pymgrid_amd import ValueHead, _lib, gae, policy
    assert ValueHead is policy.ValueHead and gae is policy.gae
    _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "mgx.h")) as fh:
        header = fh.read()
    for name in ("mgx_rollout_policy_critic_episodes", "mgx_gae"):
        assert name in _lib.SYMBOLS and getattr(L, name) is not None and f"int {name}(" in header
    assert "mgx_policy_head_episodes.hip" in [u[0] for u in _lib.UNITS] and "mgx_gae.hip" in [u[0] for u in _lib.UNITS]
    assert SAMPLE_CRITIC in _lib.UNIT_HEADS["mgx_policy_head_episodes.hip"][1]
    assert all(any(src.endswith(f) for src in _lib.SOURCES) for f in ("mgx_policy_head_episodes.hip", "mgx_gae.hip"))
    assert _lib.lib().mgx_abi_minor() == 3 == _lib.ABI_MINOR and _lib.lib().mgx_abi_version() == 9
    # the three structs before it keep their sizes
    assert C.sizeof(_lib.Policy) == 24 + 5 * C.sizeof(C.c_void_p) and C.sizeof(_lib.Exploration) == 64 and C.sizeof(_lib.Sampling) == 32
    fields = re.search(r"typedef struct mgx_critic \{(.*?)\} mgx_critic;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert re.findall(r"([a-z_]+);", fields) == [n for n, _ in _lib.Critic._fields_] == ["struct_size", "reserved", "w", "b"]
    assert re.findall(r"(\w+) \*?[a-z_]+;", fields) == ["int32_t", "int32_t", "double", "double"]
    assert C.sizeof(_lib.Critic) == 8 + 2 * C.sizeof(C.c_void_p)
    assert _lib.Critic.w.offset == 8 and _lib.Critic.b.offset == 8 + C.sizeof(C.c_void_p)
    lib = _lib.lib()
    x, c = _lib.Sampling(), _lib.Critic()
    assert lib.mgx_rollout_policy_critic_episodes(None, None, C.byref(x), C.byref(c), None, 0, 4, None, None, None, None, None, None, None,
                                                  None, None, None, None, None) == _lib.MGX_ERR_INVALID
    assert b"mgx_rollout_policy_critic_episodes" in lib.mgx_last_error()
    assert lib.mgx_gae(4, 4, None, None, None, None, None, 0.99, 0.95, None, None, None) == _lib.MGX_ERR_INVALID
    assert b"mgx_gae" in lib.mgx_last_error()


SAMPLE_CRITIC = 3    # PolicyHead (csrc/mgx_policy.hpp)
DOCUMENTED = {   # (kernel, head): (forms, most AGPRs, most spilled SGPRs, least occupancy in waves per SIMD) -- the figures of DESIGN.md
    ("rollout_policy_head_episodes_kernel", SAMPLE_CRITIC): (30, 59, 65, 1),
}


def test_the_critic_kernel_uses_what_design_md_says():
    """The 30 forms of the sampling head with a critic (ten layouts x three row sources): no scratch memory, no vector register spilled, vgpr + agpr <= 512, LDS
    within the siblings' bound; AGPRs, spilled SGPRs and occupancy no worse than DESIGN.md's kernel table records them.  The greedy,
    exploring and sampling kernels keep exactly the figures their own tests record."""
    from pymgrid_amd import _lib
    _lib.build()
    usage = _lib.resource_usage()
    if usage is None:
        pytest.skip("libmgx.so was not built on this machine (no resource_usage.json beside the objects)")
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        design = fh.read()

    def forms_of(kernel):
        return _forms_of(usage, kernel)
    for kernel, (n_forms, agpr, sgpr_spill, occupancy) in DOCUMENTED.items():
        assert f"`{kernel[0]}<7,4,0,{kernel[1]}>`" in design
        forms = forms_of(kernel)
        assert len(forms) == n_forms, (kernel, sorted(forms))
        for name, u in forms.items():
            assert u["scratch"] == 0 and u["vgpr_spill"] == 0, (name, u)
            assert u["vgpr"] <= 256 and u["agpr"] <= agpr and u["vgpr"] + u["agpr"] <= 512, (name, u)
            assert u["sgpr_spill"] <= sgpr_spill and u["occupancy"] >= occupancy, (name, u)
            assert u["lds"] <= 24576 + 64, (name, u)
    for kernel, (n_forms, agpr, sgpr_spill, occupancy) in {**GREEDY_DOCUMENTED, **EXPLORE_DOCUMENTED, **SAMPLE_DOCUMENTED}.items():
        forms = forms_of(kernel)                                  # the siblings: exactly their recorded extremes
        assert len(forms) == n_forms, (kernel, sorted(forms))
        assert max(u["agpr"] for u in forms.values()) == agpr and max(u["sgpr_spill"] for u in forms.values()) == sgpr_spill, kernel
        assert min(u["occupancy"] for u in forms.values()) == occupancy, kernel
        assert all(u["scratch"] == 0 and u["vgpr_spill"] == 0 for u in forms.values()), kernel
    gae_forms = forms_of("gae_kernel")
    assert len(gae_forms) == 4 and all(u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["lds"] == 0 for u in gae_forms.values()), gae_forms


# ---- GPU: fused == stepped ---------------------------------------------------------------------------------------------------------
def _nan_out(K, n, D, dtype, device):
    """NaN-filled final_obs and final_values: what a launch does not write keeps these bits."""
    return dict(final_values=torch.full((K, n), float("nan"), dtype=F64, device=device), **_nan_rows(K, n, D, dtype, device))


def _value_refs(head, policy, before, ref):
    """What the three value outputs must hold, from the stepped twin's rows: ``before`` the row the first id was chosen on."""
    chosen_on = [before] + list(ref["obs"][:-1])
    values = torch.stack([head.value(policy, o) for o in chosen_on])
    finals = torch.stack([head.value(policy, o) for o in ref["final_obs"]])      # (NaN rows where not done: compared where done)
    return values, finals


def _fused_equals_stepped(device, arch, series, n_hidden, obs_dtype=F64, P=1, temperature=1.0, vacuous=True, n=N, length=LENGTH,
                          t=T, launches=LAUNCHES, trace=None):
    """The critic launch, in launches of 1, 7 and 64 steps on one env, == its stepped twin after every launch -- everything the
    sampling test compares, and the three value outputs against ``head.value`` on the twin's rows; a third env takes the same
    launches WITHOUT a critic and is left with the same bits; then one more single step.  ``vacuous``: the conditions on the test
    itself, from the stepped twin alone.  ``n``, ``length``, ``t``, ``launches``: another batch size, episode length, series
    length and other launches; ``trace``: a dict that receives what test_policy_rollout._trace_launch records."""
    from pymgrid_amd import _lib
    old = _lib.get_tunable("grid_major_copy")[0]
    if series == "gather":
        _lib.set_tunable("grid_major_copy", 0)
    try:
        fused, twin, plain = _envs(device, arch, series, obs_dtype, 3, n=n, length=length, t=t)
        assert torch.equal(fused.obs0, twin.obs0) and fused.obs0.dtype == obs_dtype
        D, n_out = fused.env.engine.obs_dim, _n_out(fused, True)
        index = None
        if P > 1:
            index = torch.randint(-1, P + 1, (n,), generator=torch.Generator().manual_seed(11)).to(torch.int32)
            assert int(index.min()) == -1 and int(index.max()) == P
        policy = _spread_policy(7, twin.obs0, n_hidden, n_out, P=P, index=index)
        head = _head(9, policy)
        sa = _sampling(seed=23, temperature=temperature)
        hs = HostStats(n, device)
        obs, seen = twin.obs0, []
        _trace_start(trace, fused, True)
        for K in launches:
            out = fused.rollout_policy(policy, K, sampling=sa, probs=True, critic=head, values=True, out=_nan_out(K, n, D, obs_dtype, device),
                                       **WANT)
            before = obs
            walked = [] if trace is not None else None
            ref, obs = _twin_steps(twin, policy, sa, obs, K, hs, seen, walked)
            _trace_launch(trace, walked, out, ref)
            got = {name: out.pop(name) for name in VALUES}
            _compare(out, ref, K)
            d = out["done"]
            assert bool(torch.isnan(out["final_obs"][~d]).all()) and not bool(torch.isnan(out["final_obs"][d]).any()), K
            values, finals = _value_refs(head, policy, before, ref)
            assert got["values"].dtype == F64 and got["values"].shape == (K, n) and got["last_value"].shape == (n,)
            assert torch.equal(got["values"], values), K
            assert torch.equal(got["final_values"][d], finals[d]), K
            assert bool(torch.isnan(got["final_values"][~d]).all()) and not bool(torch.isnan(got["final_values"][d]).any()), K
            assert torch.equal(got["last_value"], head.value(policy, out["obs"][-1])), K
            _envs_equal(fused, twin, K)
            hs.check(fused.episode_stats)
            # the critic changes nothing else: the sampling launch without one
            same = plain.rollout_policy(policy, K, sampling=sa, probs=True, out=_nan_rows(K, n, D, obs_dtype, device), **WANT)
            _compare(same, out, K)
            _envs_equal(plain, fused, K)
            for name in fused.episode_stats:
                assert torch.equal(plain.episode_stats[name], fused.episode_stats[name]), name
            if K == 64:
                assert int(ref["done"].sum()) >= 1                     # a grid restarts inside the 64-step launch
                if vacuous:        # at every restart the final row's value differs from the new episode's first row's for some grid
                    first = torch.stack([head.value(policy, o) for o in ref["obs"]])
                    for k in range(K):
                        if bool(d[k].any()):
                            assert bool((finals[k][d[k]] != first[k][d[k]]).any()), k
        _trace_end(trace, fused)
        if trace is not None:
            trace["greedy"] = torch.stack([g for _, g in seen])
        if vacuous:                                                    # the stepped twin ALONE says whether the test can pass vacuously
            taken, greedy = torch.stack([a for a, _ in seen]), torch.stack([g for _, g in seen])
            share = float((taken != greedy).double().mean())
            assert 0.2 <= share <= 0.8, share
        # the env stands where the twin stands: one more single step
        a = policy.act(obs, sa, counter=twin.env.current_step)
        (o1, r1, d1, _), (o2, r2, d2, _) = fused.step(a), twin.step(a)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
        _state_equal(fused.env, twin.env)
        for e in (fused, twin, plain):
            e.env.close()
    finally:
        _lib.set_tunable("grid_major_copy", old)


@pytest.mark.gpu
@pytest.mark.parametrize("arch,series,n_hidden,obs_dtype", CASES)
def test_fused_equals_stepped(arch, series, n_hidden, obs_dtype, device):
    _fused_equals_stepped(device, arch, series, n_hidden, obs_dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("n_hidden", [0, 16])
def test_a_population_has_a_critic_per_set(n_hidden, device):
    """P = 3 parameter sets with a policy_index (indices outside the population among them: set 0)."""
    _fused_equals_stepped(device, "genset+battery+grid", "factorised", n_hidden, P=3)


@pytest.mark.gpu
def test_each_value_output_is_independent(device):
    """With each of value_out / final_value_out / last_value_out NULL in turn the others keep their bits, and so does everything
    else; with none of them (``values=False``) the critic kernel runs and leaves what the sampling kernel leaves."""
    K = 64
    envs = _envs(device, "genset+battery+grid", "factorised", F64, 5, twin=None)
    D = envs[0].env.engine.obs_dim
    policy = _spread_policy(7, envs[0].obs0, 16, _n_out(envs[0], True))
    head, sa = _head(9, policy), _sampling(seed=23)
    full = envs[0].rollout_policy(policy, K, sampling=sa, probs=True, critic=head, values=True, out=_nan_out(K, N, D, F64, device), **WANT)
    assert bool(full["done"].any())
    for env, names in zip(envs[1:], [VALUES[1:], VALUES[:1] + VALUES[2:], VALUES[:2], ()]):
        out = env.rollout_policy(policy, K, sampling=sa, probs=True, critic=head, values=names or False,
                                 out={k: v for k, v in _nan_out(K, N, D, F64, device).items() if k == "final_obs" or k in names}, **WANT)
        assert set(out) == set(full) - (set(VALUES) - set(names))
        for name in out:
            assert _same_bits(out[name], full[name]) if out[name].is_floating_point() else torch.equal(out[name], full[name]), (names, name)
        _envs_equal(env, envs[0], K)
    zeroed = envs[1].rollout_policy(policy, 7, sampling=sa, critic=head, values=True, done=True)     # an allocated final_values: zeros
    assert torch.equal(zeroed["final_values"][~zeroed["done"]], torch.zeros_like(zeroed["final_values"][~zeroed["done"]]))
    with pytest.raises(ValueError, match=r"Sampling\(seed, temperature=0\)"):
        envs[1].rollout_policy(policy, 4, critic=head)
    with pytest.raises(ValueError, match="critic="):
        envs[1].rollout_policy(policy, 4, sampling=sa, values=True)
    for e in envs:
        e.env.close()


@pytest.mark.gpu
def test_temperature_zero_is_the_greedy_launch_with_values(device):
    K = 64
    plain, cold = _envs(device, "genset+battery+grid", "factorised", F64, 2, twin=None)
    D = plain.env.engine.obs_dim
    policy = _spread_policy(7, plain.obs0, 16, _n_out(plain, True))
    head = _head(9, policy)
    ref = plain.rollout_policy(policy, K, out=_nan_rows(K, N, D, F64, device), **WANT)
    out = cold.rollout_policy(policy, K, sampling=_sampling(seed=8, temperature=0.0), probs=True, critic=head, values=True,
                              out=_nan_out(K, N, D, F64, device), **WANT)
    assert torch.equal(out.pop("probs"), torch.ones(K, N, dtype=F64, device=device))
    got = {name: out.pop(name) for name in VALUES}
    _compare(out, ref, K)
    _envs_equal(cold, plain, K)
    d = ref["done"]
    values, finals = _value_refs(head, policy, plain.obs0, ref)
    assert torch.equal(got["values"], values) and torch.equal(got["final_values"][d], finals[d])
    assert torch.equal(got["last_value"], head.value(policy, ref["obs"][-1]))
    plain.env.close(); cold.env.close()


# ---- GPU: gae == gae_host ------------------------------------------------------------------------------------------------------------
def _gae_equals_host(reward, done, value, last_value, fv):
    """Every corner of (gamma, lam), with and without final_value, with and without returns, into allocated and given outputs."""
    from pymgrid_amd import gae
    from pymgrid_amd.policy import gae_host
    K, n = reward.shape
    for gamma, lam in CORNERS:
        for final_value in (fv, None):
            ref = gae_host(reward, done, value, last_value, final_value=final_value, gamma=gamma, lam=lam)
            got = gae(reward, done, value, last_value, final_value=final_value, gamma=gamma, lam=lam)
            assert set(got) == {"advantages", "returns"}
            assert _same_bits(got["advantages"], ref["advantages"]) and _same_bits(got["returns"], ref["returns"]), (K, n, gamma, lam)
            mine = torch.full((K, n), 7.0, dtype=F64, device=reward.device)
            only = gae(reward, done.view(torch.uint8), value, last_value, final_value=final_value, gamma=gamma, lam=lam,
                       out={"advantages": mine, "returns": None})
            assert set(only) == {"advantages"} and only["advantages"] is mine and _same_bits(mine, ref["advantages"]), (K, n, gamma, lam)


@pytest.mark.gpu
def test_gae_equals_gae_host_on_seeded_inputs(device):
    """N in {1, 64, 200} (one lane, a full wave, three waves and a last one of 8 lanes) x K in {1, 7, 64} (below the unrolled group,
    one short of it, eight of it).  The done share: at rate 1 / 24 a shape of at least 448 elements misses every done with
    probability below 1e-8, so it must lie strictly between 0 and 1 there, and over all shapes together."""
    total = hit = 0
    for n in (1, 64, 200):
        for K in (1, 7, 64):
            reward, done, value, last_value, fv = _gae_inputs(K, n, seed=100 * n + K, device=device)
            share = float(done[:, 5:].double().mean()) if n > 5 else None
            if share is not None and K * (n - 5) >= 448:
                assert 0.0 < share < 1.0, (K, n, share)
            total, hit = total + done.numel(), hit + int(done.sum())
            _gae_equals_host(reward, done, value, last_value, fv)
    assert 0 < hit < total


@pytest.mark.gpu
def test_gae_of_a_real_critic_launch(device):
    """The advantages of what a 64-step critic launch returns, final_values as the launch leaves them (NaN where no grid restarted)."""
    K = 64
    (pe,) = _envs(device, "genset+battery+grid", "factorised", F64, 1, twin=None)
    D = pe.env.engine.obs_dim
    policy = _spread_policy(7, pe.obs0, 16, _n_out(pe, True))
    out = pe.rollout_policy(policy, K, sampling=_sampling(seed=23), probs=True, critic=_head(9, policy), values=True, reward=True, done=True,
                            out=dict(final_values=torch.full((K, N), float("nan"), dtype=F64, device=device)))
    share = float(out["done"].double().mean())
    assert 0.0 < share < 1.0, share
    _gae_equals_host(out["reward"], out["done"], out["values"], out["last_value"], out["final_values"])
    pe.env.close()


# ---- GPU: the refusals of the C entry -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_of_the_c_abi(device):
    """The critic call refuses -- nothing launched: state, counter and the caller's buffers untouched -- a wrong struct_size, a NULL w,
    a NULL critic (MGX_ERR_INVALID), a critic that pushes the staged sets over MGX_POLICY_LDS_BYTES (MGX_ERR_UNSUPPORTED), and what the
    sampling call refuses: a NULL sampling, a forecast horizon."""
    from pymgrid_amd import DiscreteBatchedMicrogridEnv, _lib
    from pymgrid_amd.hetero import PerGridWindowEnv
    n, K = N, 5
    name = b"mgx_rollout_policy_critic_episodes"
    nan = float("nan")
    bufs = [torch.full((K, n), nan, dtype=F64, device=device) for _ in range(4)] + [torch.full((n,), nan, dtype=F64, device=device),
                                                                                   torch.full((K, n), 255, dtype=torch.uint8, device=device)]
    z = torch.zeros(64 * 64, dtype=F64, device=device)           # (zero critic parameters for any P, n_mid here)

    def critic(**kw):
        st = _lib.Critic()
        st.struct_size, st.w, st.b = C.sizeof(_lib.Critic), z.data_ptr(), z.data_ptr()
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    def call(env, pst, sst, cst, table=None):
        e = env.engine
        tptr, n_lists = e._table_ptr(env._table if table is None else table)
        return e._lib.mgx_rollout_policy_critic_episodes(e._h, C.byref(pst), None if sst is None else C.byref(sst),
                                                         None if cst is None else C.byref(cst), tptr, n_lists, K, bufs[0].data_ptr(), None, None,
                                                         None, bufs[5].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(),
                                                         bufs[4].data_ptr(), None, None, None)

    def refused(env, code, word, cst="good", sst="good", pst=None):
        e = env.engine
        if pst is None:
            pst, keep = _c_policy(device, min(e.obs_dim, 12), 16, len(env._table))
        sst = _sampling(seed=3).c_struct(device, n)[0] if sst == "good" else sst
        cst = critic() if cst == "good" else cst
        snap = _snapshot(env)
        rc = call(env, pst, sst, cst)
        msg = e._lib.mgx_last_error()
        assert rc == code and name in msg and word in msg, (rc, msg)
        torch.cuda.synchronize()
        _untouched(env, snap)
        assert all(bool(torch.isnan(b).all()) for b in bufs[:5]) and bool((bufs[5] == 255).all())
    pe = PerGridWindowEnv(_batch(device, "genset+battery+grid", "factorised", n, H=6, t=60), trajectory_length=9, discrete=True,
                          auto_reset=True, seed=2)
    pe.reset()
    refused(pe.env, _lib.MGX_ERR_UNSUPPORTED, b"horizon")                           # a handle with a forecast horizon
    pe.env.close()
    env = DiscreteBatchedMicrogridEnv(_batch(device, "genset+battery+grid", "factorised", n, t=60))
    env.reset()
    env.reset_windows(torch.zeros(n, dtype=torch.int32, device=device), None, max_length=20, rolling="inplace")
    e = env.engine
    n_out, D = len(env._table), e.obs_dim
    refused(env, _lib.MGX_ERR_INVALID, b"struct_size", critic(struct_size=C.sizeof(_lib.Critic) - 8))
    refused(env, _lib.MGX_ERR_INVALID, b"struct_size", critic(struct_size=0))
    refused(env, _lib.MGX_ERR_INVALID, b"NULL critic weights", critic(w=None))
    refused(env, _lib.MGX_ERR_INVALID, b"NULL critic weights", critic(b=None))
    refused(env, _lib.MGX_ERR_INVALID, b"NULL", cst=None)
    refused(env, _lib.MGX_ERR_INVALID, b"NULL", sst=None)
    # 64 hidden units, enough sets: over MGX_POLICY_LDS_BYTES
    m = (n_out + 3) // 4 * 4
    sets = lambda nh, P, extra: P * ((m + extra + nh * (D + 1 + extra + m) + 1) // 2 * 2) * 8     # noqa: E731  (extra = 1: a critic)
    P64 = _lib.POLICY_LDS_BYTES // sets(64, 1, 1) + 1
    refused(env, _lib.MGX_ERR_UNSUPPORTED, b"MGX_POLICY_LDS_BYTES", pst=_c_policy(device, D, 64, n_out, P=P64)[0])
    # ... and sets that fit WITHOUT a critic, so that the sampling call takes them, but not with one
    sharp = [(nh, P) for nh in range(64, 0, -1) for P in range(1, 40) if sets(nh, P, 0) <= _lib.POLICY_LDS_BYTES < sets(nh, P, 1)]
    assert sharp
    nh, P = sharp[0]
    pst, keep = _c_policy(device, D, nh, n_out, P=P)
    refused(env, _lib.MGX_ERR_UNSUPPORTED, b"MGX_POLICY_LDS_BYTES", pst=pst)
    sst = _sampling(seed=3).c_struct(device, n)[0]
    tptr, n_lists = e._table_ptr(env._table)
    t_before = e._lib.mgx_current_step(e._h)
    assert e._lib.mgx_rollout_policy_sample_episodes(e._h, C.byref(pst), C.byref(sst), tptr, n_lists, K, bufs[0].data_ptr(), None, None, None,
                                                     bufs[5].data_ptr(), bufs[1].data_ptr(), None, None, None) == _lib.MGX_OK, e._lib.mgx_last_error()
    torch.cuda.synchronize()
    assert e._lib.mgx_current_step(e._h) == t_before + K
    # ... and the critic call is taken once nothing stands in the way (zero parameters: V = 0 everywhere, every id weighs 1.0)
    for b in bufs[:5]:
        b.fill_(nan)
    pst, keep = _c_policy(device, D, 16, n_out)
    assert call(env, pst, sst, critic()) == _lib.MGX_OK, e._lib.mgx_last_error()
    torch.cuda.synchronize()
    assert e._lib.mgx_current_step(e._h) == t_before + 2 * K
    assert not bool(torch.isnan(bufs[0]).any()) and torch.equal(bufs[1], torch.full((K, n), 1.0 / n_out, dtype=F64, device=device))
    assert torch.equal(bufs[2], torch.zeros(K, n, dtype=F64, device=device)) and torch.equal(bufs[4], torch.zeros(n, dtype=F64, device=device))
    env.close()
