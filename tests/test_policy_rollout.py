"""Closed-loop policy roll-outs inside the fused per-grid-episode launches (mgx_rollout_policy_episodes /
mgx_step_k_policy_episodes, StepEngine.rollout_policy_episodes / step_k_policy_episodes, PerGridWindowEnv.rollout_policy /
step_k_policy): K steps in one launch == a twin stepped K times with ``policy.act(obs)`` on the observation its last step
returned -- rewards, done, traces, the actions taken, the rows, the rows before the restarts, the episode arrays, the state and
the statistics, bit for bit (torch.equal; MLPPolicy.act performs the kernel's IEEE operations in the kernel's order, so there is no
tolerance).  The forms of the kernels these cases leave out -- all ten layouts x the three row sources -- run in
tests/test_layout_matrix_policy.py, which also replays the launches on the CPU oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_episode_rows as rows_tests
from layouts import LAYOUTS, carve
from test_episode_rows import HostStats, _same_bits, _snapshot, _state_equal, _untouched

T = 200
LAUNCHES = (1, 7, 64, 130)          # K = 1, a K that is no multiple of a ring depth (4 / 8), a 64-step launch, one above 128
F64, F32 = torch.float64, torch.float32


def _batch(device, arch, series, n, H=0, t=T):
    """``arch``: an architecture generate() draws, or one of the ten layout flags (carved out of a genset+battery+grid batch)."""
    if isinstance(arch, int):
        return carve(rows_tests._batch(device, "genset+battery+grid", series, H, n=n, t=t), arch)
    return rows_tests._batch(device, arch, series, H, n=n, t=t)


def _policy(seed, n_in, n_hidden, n_out, head, P=1, tie=None, index=None):
    """Random parameters that spread the logits / controls over the rows of a batch: the weights of a unit sum to about zero over
    inputs in [0, 1], the continuous head's biases centre the controls inside [0, 1] so that both edges of the clip and its
    interior occur.  ``tie`` (an output): that output changes places with output 0 and output 1 then repeats output 0 (weights and
    bias), so the two tie at every input -- 1 is never taken, 0 wherever ``tie`` would have been."""
    rng = np.random.default_rng(seed)
    W1 = b1 = None
    if n_hidden:
        W1, b1 = rng.normal(0.0, 1.5, size=(P, n_hidden, n_in)), rng.normal(0.0, 0.5, size=(P, n_hidden))
    W2 = rng.normal(0.0, 1.5 if not n_hidden else 0.6, size=(P, n_out, n_hidden or n_in))
    b2 = rng.normal(0.5 if head == "continuous" else 0.0, 0.5, size=(P, n_out))
    if tie is not None:
        W2[:, [0, tie]], b2[:, [0, tie]] = W2[:, [tie, 0]], b2[:, [tie, 0]]
        W2[:, 1], b2[:, 1] = W2[:, 0], b2[:, 0]
    from pymgrid_amd import MLPPolicy
    return MLPPolicy(W1, b1, W2, b2, policy_index=index, head=head)


def _envs(device, discrete, arch, series, length, obs_dtype, n, count=2, seed=23, twin=1):
    """``count`` PerGridWindowEnv of the same batch, seed and first draw; number ``twin`` (the stepped one; None: none) reports the
    rows before the restarts."""
    from pymgrid_amd.hetero import PerGridWindowEnv
    kw = dict(trajectory_length=length, discrete=discrete, auto_reset=True, seed=seed, obs_dtype=obs_dtype)
    envs = [PerGridWindowEnv(_batch(device, arch, series, n), final_observation=(q == twin), **kw) for q in range(count)]
    for e in envs:
        torch.manual_seed(41)                   # the same first draw
        e.obs0 = e.reset()
    return envs


def _n_out(pe, discrete):
    return pe.env.action_space.n if discrete else pe.env.engine.action_dim


def _twin_steps(twin, policy, obs, K, hs, walked=None):
    """K times ``a = policy.act(obs); obs, r, done, info = twin.step(a)``: what the fused call offers, per step.  ``walked``: a list
    that receives every grid's series row before each step."""
    rows = {k: [] for k in ("reward", "done", "soc_trace", "status_trace", "actions", "obs", "final_obs")}
    cols = twin.env.batch.cols
    for _ in range(K):
        if walked is not None:
            walked.append(twin.env.current_steps.clone())
        a = policy.act(obs)
        obs, r, d, info = twin.step(a) if a.dtype == torch.int32 else twin.step(a, normalized=True)
        rows["actions"].append(a.to(torch.uint8) if a.dtype == torch.int32 else a.clone())
        rows["reward"].append(r.clone()); rows["done"].append(d.clone()); rows["obs"].append(obs.clone())
        fo = info["final_observation"]
        rows["final_obs"].append(torch.where(d[:, None], fo, torch.full_like(fo, float("nan"))))
        if "soc" in cols:
            rows["soc_trace"].append(cols["soc"].clone())
        if "gen_status" in cols:
            rows["status_trace"].append(cols["gen_status"].clone().view(torch.int32))
        hs.add(r, d)
    return {k: torch.stack(v) for k, v in rows.items() if v}, obs


def _launch(pe, policy, K, discrete, **kw):
    return (pe.rollout_policy if discrete else pe.step_k_policy)(policy, K, **kw)


WANT = dict(reward=True, done=True, soc_trace=True, status_trace=True, actions=True, observations=True, final_observations=True)


def _trace_start(trace, pe, discrete):
    """What an independent replay of a closed-loop launch starts from (``trace``: a dict, or None): the columns of the batch after
    the reset, on the host, and the priority-list table of a discrete env."""
    if trace is not None:
        trace["cols"] = pe.env.batch.numpy_columns()
        trace["table"] = pe.env._table if discrete else None


def _trace_launch(trace, walked, out, ref):
    """One launch: the series rows the twin walked, the actions the launch reports and its rewards; of the stepped twin ALONE (for
    the conditions on a test itself) the done flags and the actions taken."""
    if trace is not None:
        trace.setdefault("launches", []).append(dict(rows=torch.stack(walked), controls=out["actions"].contiguous(), reward=out["reward"],
                                                     done=ref["done"], taken=ref["actions"]))


def _trace_end(trace, pe):
    if trace is not None:
        cols = pe.env.batch.cols
        trace["state"] = {name: cols[name].clone() for name in ("charge", "soc", "gen_status") if name in cols}


def _fused_equals_stepped(device, discrete, arch, series, length, n_hidden, n, obs_dtype=F64, launches=LAUNCHES, tie=False,
                          closed=False, third=False, trace=None, seed=7):
    """The closed-loop launch, in launches of uneven size on one env, == its stepped twin after every launch; then the next single
    step.  ``closed``: the conditions on the test itself (restarts, the ids / controls really follow the observations).
    ``third``: a third env replays the returned actions through the open-loop rollout / step_k.  ``trace``: a dict that receives
    what an independent replay needs (_trace_start / _trace_launch / _trace_end); ``seed``: of the policy's parameters."""
    from pymgrid_amd import _lib
    old = _lib.get_tunable("grid_major_copy")[0]
    if series == "gather":
        _lib.set_tunable("grid_major_copy", 0)
    try:
        envs = _envs(device, discrete, arch, series, length, obs_dtype, n, count=3 if third else 2)
        fused, twin = envs[0], envs[1]
        assert torch.equal(fused.obs0, twin.obs0) and fused.obs0.dtype == obs_dtype
        D = fused.env.engine.obs_dim
        head = "discrete" if discrete else "continuous"
        policy = _policy(seed, D, n_hidden, _n_out(fused, discrete), head)
        _trace_start(trace, fused, discrete)
        if tie:                                                # the tie on the output the first observations favour: it really decides steps
            fav = int(torch.bincount(policy.act(twin.obs0).long(), minlength=policy.n_out).argmax())
            policy = _policy(seed, D, n_hidden, policy.n_out, head, tie=fav)
        hs = HostStats(n, device)
        obs = twin.obs0
        restarts, taken, moved = 0, [], False
        for K in launches:
            bufs = dict(final_obs=torch.full((K, n, D), float("nan"), dtype=obs_dtype, device=device))
            out = _launch(fused, policy, K, discrete, out=bufs, **WANT)
            walked = [] if trace is not None else None
            ref, obs = _twin_steps(twin, policy, obs, K, hs, walked)
            _trace_launch(trace, walked, out, ref)
            assert set(out) == set(ref), (sorted(out), sorted(ref))
            assert out["final_obs"] is bufs["final_obs"] and out["obs"].dtype == obs_dtype
            for name in out:
                if name != "final_obs":
                    assert out[name].shape == ref[name].shape and out[name].dtype == ref[name].dtype, (K, name)
                    assert torch.equal(out[name], ref[name]), (K, name)
            d = out["done"]
            assert _same_bits(out["final_obs"], ref["final_obs"]), K           # the rows before the restarts; NaN kept elsewhere
            assert bool(torch.isnan(out["final_obs"][~d]).all()) and not bool(torch.isnan(out["final_obs"][d]).any()), K
            assert torch.equal(fused.starts, twin.starts), K
            assert (fused.lengths is None) == (twin.lengths is None)
            if twin.lengths is not None:
                assert torch.equal(fused.lengths, twin.lengths), K
            assert torch.equal(fused.env.current_steps, twin.env.current_steps), K
            hs.check(fused.episode_stats)
            _state_equal(fused.env, twin.env)
            if third:                                                          # the open loop on the actions the closed loop took
                if discrete:
                    rep = envs[2].rollout(out["actions"], reward=True, done=True, soc_trace=True, status_trace=True, observations=True,
                                          final_observations=True, out=dict(final_obs=torch.full_like(bufs["final_obs"], float("nan"))))
                else:
                    rep = envs[2].step_k(out["actions"], normalized=True, reward=True, done=True, soc_trace=True, status_trace=True,
                                         observations=True, final_observations=True,
                                         out=dict(final_obs=torch.full_like(bufs["final_obs"], float("nan"))))
                assert set(rep) == set(out) - {"actions"}
                for name in rep:
                    assert _same_bits(rep[name], out[name]) if name == "final_obs" else torch.equal(rep[name], out[name]), (K, name)
                for name in fused.episode_stats:
                    assert torch.equal(envs[2].episode_stats[name], fused.episode_stats[name]), (K, name)
                _state_equal(envs[2].env, fused.env)
            # the stepped twin ALONE says whether the test can pass vacuously
            restarts += int(ref["done"].sum())
            taken.append(ref["actions"])
            if K > 1:
                moved |= bool((ref["actions"][1:] != ref["actions"][:-1]).any())
        assert int(fused.episode_stats["episodes"].sum()) == restarts
        _trace_end(trace, fused)
        if closed:
            assert restarts > n, restarts
            assert moved                                       # a grid's action changes between two steps of one launch
            if discrete:
                ids = torch.cat(taken).unique().tolist()
                assert len(ids) >= 3, ids
                if tie:
                    assert 1 not in ids and 0 in ids           # outputs 0 and 1 tie at every step: the lower index is taken
            else:
                u = torch.cat(taken)
                assert bool((u == 0).any()) and bool((u == 1).any()) and bool(((u > 0) & (u < 1)).any())
        # the env stands where the twin stands: the next single step returns the twin's row
        a = policy.act(obs)
        assert torch.equal(a, policy.act(out["obs"][-1]))
        kw = {} if discrete else dict(normalized=True)
        (o1, r1, d1, _), (o2, r2, d2, _) = fused.step(a, **kw), twin.step(a, **kw)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
        _state_equal(fused.env, twin.env)
        for e in envs:
            e.env.close()
    finally:
        _lib.set_tunable("grid_major_copy", old)


ARCHS = ["genset+battery+grid", "genset+battery", 5]           # 5: genset + grid, a layout without a battery
SERIES = ["factorised", "materialised", "gather"]
# (discrete, arch, series, n_hidden) crossed; the batch size (300: the last wave is partial and takes the lane-by-lane row path,
# 256: full waves, the tile path) and the episode length (9 / own lengths) rotate so that every arch and source sees both
CASES = [(disc, arch, series, nh, (300, 256)[(ai + si + hi) % 2], (9, None)[(ai + si + di) % 2])
         for di, disc in enumerate((True, False)) for ai, arch in enumerate(ARCHS) for si, series in enumerate(SERIES)
         for hi, nh in enumerate((0, 16))]


@pytest.mark.gpu
@pytest.mark.parametrize("discrete,arch,series,n_hidden,n,length", CASES)
def test_fused_equals_stepped(discrete, arch, series, n_hidden, n, length, device):
    closed = arch == "genset+battery+grid"                     # (the other tables hold too few lists for three ids beside a tie)
    _fused_equals_stepped(device, discrete, arch, series, length, n_hidden, n, closed=closed, tie=closed and discrete)


def test_the_cases_cover_both_sizes_and_lengths_everywhere():
    for key in (1, 2):                                         # per arch, per source
        seen = {}
        for c in CASES:
            seen.setdefault((c[0], c[key]), set()).add((c[4], c[5]))
        assert all({n for n, _ in v} == {300, 256} and {ln for _, ln in v} == {9, None} for v in seen.values()), seen


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [True, False])
@pytest.mark.parametrize("flags", LAYOUTS)
def test_all_ten_layouts(flags, discrete, device):
    li = LAYOUTS.index(flags)
    _fused_equals_stepped(device, discrete, flags, SERIES[li % 3], (9, None)[li % 2], (0, 16)[(li // 2) % 2], (300, 256)[li % 2],
                          launches=(7,))


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [True, False])
@pytest.mark.parametrize("n", [300, 256])
def test_float32_rows(n, discrete, device):
    """obs_dtype=float32: the policy reads the float rows the env returns, widened -- the twin is stepped from them."""
    _fused_equals_stepped(device, discrete, "genset+battery+grid", "factorised", 9, 16, n, obs_dtype=F32, closed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [True, False])
@pytest.mark.parametrize("series", ["factorised", "materialised"])
def test_the_open_loop_replays_the_actions_taken(series, discrete, device):
    _fused_equals_stepped(device, discrete, "genset+battery+grid", series, 9, 16, 300, launches=(7, 64), third=True)


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [True, False])
@pytest.mark.parametrize("n_hidden", [0, 16])
def test_a_population(n_hidden, discrete, device):
    """Three parameter sets and a random policy_index (indices outside the population among them: set 0) == three runs with one
    shared set each, selected per grid -- a grid's episodes depend on its own actions and its own draws alone."""
    from pymgrid_amd import MLPPolicy
    n, K, P = 300, 40, 3
    envs = _envs(device, discrete, "genset+battery+grid", "factorised", 9, F64, n, count=1 + P, twin=None)
    D = envs[0].env.engine.obs_dim
    head = "discrete" if discrete else "continuous"
    index = torch.randint(-1, P + 1, (n,), generator=torch.Generator().manual_seed(11)).to(torch.int32)
    pop = _policy(13, D, n_hidden, _n_out(envs[0], discrete), head, P=P, index=index)
    used = torch.where((index >= 0) & (index < P), index, torch.zeros_like(index)).to(device).long()
    assert used.unique().numel() == P and bool((index < 0).any()) and bool((index >= P).any())
    out = _launch(envs[0], pop, K, discrete, **WANT)
    singles = []
    for q in range(P):
        one = MLPPolicy(None if pop.W1 is None else pop.W1[q], None if pop.b1 is None else pop.b1[q], pop.W2[q], pop.b2[q], head=head)
        singles.append(_launch(envs[1 + q], one, K, discrete, **WANT))
    assert not torch.equal(singles[0]["actions"], singles[1]["actions"])          # the sets differ in what they do
    for name in out:
        picked = torch.stack([s[name] for s in singles])                            # [P, K, n, ...]
        sel = used.view(1, 1, n, *([1] * (picked.dim() - 3))).expand(1, *picked.shape[1:])
        assert torch.equal(out[name], picked.gather(0, sel)[0]), name
    for e in envs:
        e.env.close()


# ---- the kernels' resource figures (CPU: the compiler's remarks of the build) -----------------------------------------------------
DOCUMENTED = {   # kernel: (forms, most AGPRs, most spilled SGPRs, least occupancy in waves per SIMD) -- the figures of DESIGN.md
    "rollout_policy_episodes_kernel": (30, 50, 12, 1),
    "step_k_policy_episodes_kernel": (30, 0, 22, 2),
}


def test_the_policy_kernels_use_what_design_md_says():
    """Every form of the two kernels (ten layouts x three row sources): no scratch memory and no vector register spilled to it; the
    vector values the compiler moved into accumulation registers (AGPRs), the scalar registers it spilled to vector lanes and the
    occupancy no worse than DESIGN.md's kernel table records them -- the discrete forms DO overflow into AGPRs, the continuous ones
    do not."""
    from pymgrid_amd import _lib
    _lib.build()
    usage = _lib.resource_usage()
    if usage is None:
        pytest.skip("libmgx.so was not built on this machine (no resource_usage.json beside the objects)")
    for kernel, (n_forms, agpr, sgpr_spill, occupancy) in DOCUMENTED.items():
        forms = {name: u for name, u in usage.items() if name.split("<")[0].split("::")[-1] == kernel}
        assert len(forms) == n_forms, (kernel, sorted(forms))
        for name, u in forms.items():
            assert u["scratch"] == 0 and u["vgpr_spill"] == 0, (name, u)
            assert u["vgpr"] <= 256 and u["agpr"] <= agpr and u["vgpr"] + u["agpr"] <= 512, (name, u)
            assert u["sgpr_spill"] <= sgpr_spill and u["occupancy"] >= occupancy, (name, u)
            assert u["lds"] <= 24576 + 64, (name, u)              # the row strips (+ the list table); the parameter sets are dynamic


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _c_policy(device, n_in, n_hidden, n_out, P=1):
    """A mgx_policy of zero parameters straight for the C calls (+ what keeps its arrays alive)."""
    from pymgrid_amd import _lib
    z = lambda *shape: torch.zeros(*shape, dtype=F64, device=device)
    keep = [z(P, max(n_hidden, 1), n_in), z(P, max(n_hidden, 1)), z(P, max(n_out, 1), max(n_hidden or n_in, 1)), z(P, max(n_out, 1))]
    st = _lib.Policy()
    st.struct_size = C.sizeof(_lib.Policy)
    st.n_policies, st.n_in, st.n_hidden, st.n_out = P, n_in, n_hidden, n_out
    st.w1, st.b1, st.w2, st.b2 = (t.data_ptr() for t in keep)
    st.keep = keep                      # (the arrays live as long as the struct that points at them)
    return st, keep


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [True, False])
def test_refusals_of_the_c_abi(discrete, device):
    """Both calls refuse -- before anything is launched, with rows and without -- what the open-loop calls with rows refuse (a
    lock-step handle, several modules of a kind, a forecast horizon, state-only rows, a set final-observation buffer) with their
    codes, and of the policy: a wrong struct_size, n_in / n_out that do not fit the handle, NULL weights (MGX_ERR_INVALID), more
    hidden units or parameter bytes than the limits, float32 controls on the continuous call (MGX_ERR_UNSUPPORTED)."""
    from pymgrid_amd import BatchedMicrogridEnv, DiscreteBatchedMicrogridEnv, _lib
    from pymgrid_amd.engine import _ptr
    from pymgrid_amd.generator import generate, widen
    from pymgrid_amd.hetero import PerGridWindowEnv
    cls = DiscreteBatchedMicrogridEnv if discrete else BatchedMicrogridEnv
    n, K = 300, 5
    name = b"mgx_rollout_policy_episodes" if discrete else b"mgx_step_k_policy_episodes"
    starts = torch.zeros(n, dtype=torch.int32, device=device)

    def call(env, pst, rows=None, table=None):
        e = env.engine
        if discrete:
            tptr, n_lists = e._table_ptr(env._table if table is None else table)
            return e._lib.mgx_rollout_policy_episodes(e._h, C.byref(pst), tptr, n_lists, K, None, None, None, None, None, None, rows, None)
        return e._lib.mgx_step_k_policy_episodes(e._h, C.byref(pst), K, None, None, None, None, None, None, rows, None)

    def refused(env, code, word, pst=None, with_rows=(False, True), stats=None, table=None):
        e = env.engine
        if pst is None:
            n_out = (len(env._table) if table is None else len(table)) if discrete else e.action_dim
            pst, keep = _c_policy(device, min(e.obs_dim, 12), 16, n_out)
        for rows_on in with_rows:
            rows, buf = None, None
            if rows_on:
                buf = torch.full((K, n, e.obs_dim), float("nan"), dtype=e.obs_dtype, device=device)
                rows = _lib.EpisodeRows()
                rows.struct_size = C.sizeof(_lib.EpisodeRows)
                rows.obs = _ptr(buf)
                rows = C.byref(rows)
            snap = _snapshot(env, stats)
            rc = call(env, pst, rows, table)
            msg = e._lib.mgx_last_error()
            assert rc == code and name in msg and word in msg, (rc, msg)
            torch.cuda.synchronize()
            _untouched(env, snap, stats)
            assert buf is None or bool(torch.isnan(buf).all())
    # a forecast horizon: refused whether or not rows are asked for
    pe = PerGridWindowEnv(_batch(device, "genset+battery+grid", "factorised", n, H=6, t=60), trajectory_length=9, discrete=discrete,
                          auto_reset=True, seed=2)
    pe.reset()
    refused(pe.env, _lib.MGX_ERR_UNSUPPORTED, b"horizon")
    pe.env.close()
    env = cls(_batch(device, "genset+battery+grid", "factorised", n, t=60))
    e = env.engine
    stats = {nm: torch.full((n,), 3, dtype=dt, device=device) for nm, dt in e.EPISODE_STATS}
    env.reset()
    refused(env, _lib.MGX_ERR_INVALID, b"in-place episodes", stats=stats)            # a lock-step handle
    env.reset_windows(starts, None, max_length=9)                                   # gathered windows: no in-place episodes either
    refused(env, _lib.MGX_ERR_INVALID, b"in-place episodes", stats=stats)
    env.reset_windows(starts, None, max_length=9, rolling="inplace")
    _lib.check(e._lib.mgx_set_obs_mode(e._h, 1))                                    # state-only rows
    refused(env, _lib.MGX_ERR_UNSUPPORTED, b"state-only", stats=stats)
    _lib.check(e._lib.mgx_set_obs_mode(e._h, 0))
    e.set_final_obs(torch.zeros(n, e.obs_dim, dtype=F64, device=device))            # a set final-observation buffer
    refused(env, _lib.MGX_ERR_UNSUPPORTED, b"mgx_set_final_obs", stats=stats)
    e.set_final_obs(None)
    # the policy itself
    D = e.obs_dim
    n_out = len(env._table) if discrete else e.action_dim
    pst, keep = _c_policy(device, D, 16, n_out)
    pst.struct_size -= 8
    refused(env, _lib.MGX_ERR_INVALID, b"struct_size", pst, stats=stats)
    refused(env, _lib.MGX_ERR_INVALID, b"n_in", _c_policy(device, D - 1, 16, n_out)[0], stats=stats)
    refused(env, _lib.MGX_ERR_INVALID, b"n_out", _c_policy(device, D, 16, n_out + 1)[0], stats=stats)
    refused(env, _lib.MGX_ERR_INVALID, b"n_out", _c_policy(device, D, 0, n_out - 1)[0], stats=stats)
    pst, keep = _c_policy(device, D, 16, n_out)
    pst.w2 = None
    refused(env, _lib.MGX_ERR_INVALID, b"NULL", pst, stats=stats)
    pst, keep = _c_policy(device, D, 16, n_out)
    pst.b1 = None
    refused(env, _lib.MGX_ERR_INVALID, b"NULL", pst, stats=stats)
    refused(env, _lib.MGX_ERR_UNSUPPORTED, b"MGX_POLICY_MAX_HIDDEN", _c_policy(device, D, _lib.POLICY_MAX_HIDDEN + 1, n_out)[0], stats=stats)
    big = _c_policy(device, D, 16, n_out, P=400)[0]
    refused(env, _lib.MGX_ERR_UNSUPPORTED, b"MGX_POLICY_LDS_BYTES", big, stats=stats)
    assert re_bytes(e._lib.mgx_last_error()) > _lib.POLICY_LDS_BYTES                # the message names the size
    if not discrete:
        e.set_action_dtype(F32)
        refused(env, _lib.MGX_ERR_UNSUPPORTED, b"float32", stats=stats)
        e.set_action_dtype(F64)
    # ... and the handle is taken once nothing stands in the way, at the limits too
    for nh in (16, _lib.POLICY_MAX_HIDDEN):
        pst, keep = _c_policy(device, D, nh, n_out)
        t_before = e._lib.mgx_current_step(e._h)
        assert call(env, pst) == _lib.MGX_OK, e._lib.mgx_last_error()
        torch.cuda.synchronize()
        assert e._lib.mgx_current_step(e._h) == t_before + K
    env.close()
    # several modules of a kind
    wide = widen(generate(n, n_steps=60, seed=4, arch="genset+battery", device=device), n_battery=2)
    env = cls(wide)
    env.reset_windows(starts, None, max_length=9, rolling="inplace")
    refused(env, _lib.MGX_ERR_UNSUPPORTED, b"one module of every kind", table=np.zeros((1, 3, 2), dtype=np.int32))
    env.close()


def re_bytes(message):
    import re
    return int(re.search(rb"take (\d+) bytes", message).group(1))


@pytest.mark.gpu
@pytest.mark.parametrize("discrete", [True, False])
def test_refusals_of_the_python_surface(discrete, device):
    """PerGridWindowEnv.rollout_policy / step_k_policy: ValueError that says what stands in the way -- a horizon and
    observation_keys also WITHOUT observations (the policy reads whole rows), what rollout / step_k refuse, a policy of the wrong
    head or size -- and nothing launched; rollout / step_k keep their own refusals."""
    from pymgrid_amd.hetero import PerGridWindowEnv
    n, K = 300, 4
    head = "discrete" if discrete else "continuous"

    def batch(h=0, arch="genset+battery"):
        return _batch(device, arch, "factorised", n, H=h, t=60)

    def fitting(pe):
        return _policy(1, min(pe.env.engine.obs_dim, 12), 16, min(_n_out(pe, discrete), 12), head)
    cases = [("horizon", {}, batch(6)), ("observation_keys", dict(observation_keys=["load_current", "soc"]), batch()),
             ("final_observation", dict(final_observation=True), batch()), ("auto_reset=False", dict(auto_reset=False), batch()),
             ("several modules", {}, None)]
    for word, kw, b in cases:
        if b is None:
            from pymgrid_amd.generator import generate, widen
            b = widen(generate(n, n_steps=60, seed=4, arch="genset+battery", device=device), n_battery=2)
        pe = PerGridWindowEnv(b, **dict(dict(trajectory_length=9, discrete=discrete, auto_reset=True, seed=2), **kw))
        pe.reset()
        for rows in ({}, dict(observations=True), dict(final_observations=True)):
            snap = _snapshot(pe.env)
            with pytest.raises(ValueError, match=word):
                _launch(pe, fitting(pe), K, discrete, **rows)
            _untouched(pe.env, snap)
        if word in ("horizon", "observation_keys"):            # the open-loop call without rows is still offered there, word for word
            ctl = torch.zeros(K, n, dtype=torch.uint8, device=device) if discrete else \
                torch.zeros(K, n, pe.env.engine.action_dim, dtype=F64, device=device)
            assert (pe.rollout if discrete else pe.step_k)(ctl)["reward"].shape == (K, n)
            with pytest.raises(ValueError, match="writes no observations with " + word):
                (pe.rollout if discrete else pe.step_k)(ctl, observations=True)
        pe.env.close()
    # the wrong env for the call, and policies that do not fit
    pe = PerGridWindowEnv(batch(), trajectory_length=9, discrete=discrete, auto_reset=True, seed=2)
    with pytest.raises(ValueError, match="discrete="):
        (pe.step_k_policy if discrete else pe.rollout_policy)(fitting(pe), K)
    with pytest.raises(RuntimeError, match="before reset"):
        _launch(pe, fitting(pe), K, discrete)
    pe.reset()
    D, no = pe.env.engine.obs_dim, _n_out(pe, discrete)
    other = "continuous" if discrete else "discrete"
    bad = [("head", _policy(1, D, 16, min(no, 4), other)), ("columns", _policy(1, D - 1, 16, no, head)),
           ("outputs", _policy(1, D, 0, no - 1, head)),
           ("policy_index", _policy(1, D, 0, no, head, index=np.zeros(n - 1, dtype=np.int32)))]
    for word, pol in bad:
        snap = _snapshot(pe.env)
        with pytest.raises(ValueError, match=word):
            _launch(pe, pol, K, discrete)
        _untouched(pe.env, snap)
    assert pe.episode_stats is None                            # nothing was launched
    out = _launch(pe, fitting(pe), K, discrete, actions=True)
    assert set(out) == {"reward", "actions"} and out["actions"].shape == ((K, n) if discrete else (K, n, no))
    if not discrete:
        pe32 = PerGridWindowEnv(batch(), trajectory_length=9, discrete=False, auto_reset=True, seed=2, action_dtype=F32)
        pe32.reset()
        with pytest.raises(ValueError, match="float32"):
            pe32.step_k_policy(fitting(pe32), K)
        pe32.env.close()
    pe.env.close()
