"""step_k_hot_kernel (csrc/mgx_step_hot.hip): the kernel of its own that the lock-step reward + SoC launch of mgx_step_k takes on
factorised series without a GridModule.  It must compute, bit for bit, what step_k_kernel computes for the same launch (tunable
step_k_hot = 0) and what K single steps compute: reward, SoC trace and the state columns after the launch.  HOT_LAYOUTS x HOT_DTYPES
name the compiled forms: tests/test_layouts.py fails when the library holds one that is not among them."""
import pytest
import torch

U = 8                        # MGX_RING_HOT: the kernel's ring depth (a group of its main loop)
K_MAX = 128                  # STEP_HOT_MAX_K: the rows of one LDS image; K_MAX + 1 goes to step_k_kernel
KS = (1, U - 1, U, U + 1, 2 * U - 2, 2 * U - 1, 2 * U + 3, 64, K_MAX, K_MAX + 1)    # (2U - 1: the first K whose first group needs no guard)
T = 200
STATE = ("charge", "soc", "gen_status")
SENTINEL = -12345.678


def _batch(device, flags, N, seed=5, mixed_timers=False):
    """A factorised batch of layout `flags` (1 genset, 2 battery, 3 both): the genset + battery draw with the other module's columns
    dropped."""
    from pymgrid_amd import MicrogridBatch
    from pymgrid_amd.batch import BatchLayout
    from pymgrid_amd.generator import generate
    b = generate(N, n_steps=T, seed=seed, arch="genset+battery", device=device, mixed_timers=mixed_timers, series="factorised")
    if flags == 3:
        return b
    drop = ("bat_", "charge", "soc") if flags == 1 else ("gen_",)
    cols = {k: v for k, v in b.cols.items() if not k.startswith(drop)}
    return MicrogridBatch(BatchLayout(n_grids=N, n_steps=T, has_genset=flags == 1, has_battery=flags == 2, has_grid=False), cols)


@pytest.fixture
def hot():
    """Sets the step_k_hot tunable; puts the default back afterwards."""
    from pymgrid_amd import _lib
    yield lambda v: _lib.set_tunable("step_k_hot", v)
    _lib.set_tunable("step_k_hot", _lib.get_tunable("step_k_hot")[1])


class _Case:
    """One engine and its starting state; runs launches from that state."""

    def __init__(self, device, batch, action_dtype, shards=1):
        from pymgrid_amd import StepEngine
        self.batch, self.device, self.shards = batch, device, shards
        self.N, self.has_battery = batch.layout.n_grids, batch.layout.has_battery
        self.eng = StepEngine(batch, action_dtype=action_dtype)
        if shards > 1:
            self.eng.set_shards(shards)
        self.state0 = {k: batch.cols[k].clone() for k in STATE if k in batch.cols}

    def restore(self, t0):
        for k, v in self.state0.items():
            self.batch.cols[k].copy_(v)
        self.eng.reset(t0, want_obs=False)

    def state(self):
        return {k: self.batch.cols[k].clone() for k in self.state0}

    def launch(self, acts, normalized, t0, pad=2, ret_acc=None):
        """One mgx_step_k launch from the starting state at row t0 into sentinel-filled buffers with `pad` spare rows before and behind
        the [K, N] outputs: returns (reward, soc_trace or None, state after the launch) after checking that the spare rows kept the sentinel."""
        K, N = acts.shape[0], self.N
        self.restore(t0)
        bufs, out = {}, {}
        for name in ("reward",) + (("soc_trace",) if self.has_battery else ()):
            bufs[name] = torch.full(((K + 2 * pad) * N,), SENTINEL, dtype=torch.float64, device=self.device)
            out[name] = bufs[name][pad * N:(pad + K) * N].view(K, N)
        if self.shards > 1:
            self.eng.fork()
        self.eng.step_k(acts, normalized=normalized, reward=True, soc_trace=True, ret_acc=ret_acc, out=out)
        if self.shards > 1:
            self.eng.join()
        torch.cuda.synchronize(self.device)
        for name, b in bufs.items():
            assert bool((b[:pad * N] == SENTINEL).all()) and bool((b[(pad + K) * N:] == SENTINEL).all()), f"{name}: a write outside [K, N]"
        return out["reward"], out.get("soc_trace"), self.state()

    def single_steps(self, acts, normalized, t0, stops):
        """acts.shape[0] single steps from the starting state: (reward [K, N], SoC [K, N] or None, {K: state after K steps} for K in stops)."""
        self.restore(t0)
        rew, soc, states = [], [], {}
        for k in range(acts.shape[0]):
            if self.shards > 1:
                self.eng.fork()
            r = self.eng.step(acts[k], normalized=normalized, want_obs=False, want_done=False)[1]
            if self.shards > 1:
                self.eng.join()
            rew.append(r.clone())
            if self.has_battery:
                soc.append(self.batch.cols["soc"].clone())
            if k + 1 in stops:
                states[k + 1] = self.state()
        torch.cuda.synchronize(self.device)
        return torch.stack(rew), (torch.stack(soc) if self.has_battery else None), states

    def close(self):
        self.eng.close()


def _same(a, b, what):
    if a is None and b is None:
        return
    assert torch.equal(a, b), what


def _same_state(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (k, what)


def _actions(device, K, N, A, dtype, normalized, seed):
    g = torch.Generator(device=device); g.manual_seed(seed)
    a = torch.rand(K, N, A, dtype=torch.float64, device=device, generator=g)
    if not normalized:
        a = a * 70.0 - 10.0                       # raw requests, some outside every module's range
    return a.to(dtype).contiguous()


HOT_LAYOUTS, HOT_DTYPES = (1, 2, 3), (torch.float64, torch.float32)      # the forms step_k_hot_kernel<F, U, AT> is compiled in


@pytest.mark.gpu
@pytest.mark.parametrize("action_dtype", HOT_DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("flags", HOT_LAYOUTS)
def test_hot_kernel_equals_step_k_kernel_and_single_steps(flags, action_dtype, device, hot):
    """Layouts 1, 2, 3 x float64 / float32 controls x normalised or not; N = 1, 65, 300 (two workgroups of 192 grids: a wholly
    inactive wave that still meets the barriers, a partial wave), 301 in two shards; every K around the group size, the largest K
    the kernel takes and that + 1 (step_k_kernel's); t0 = 0 and 37."""
    A = 2 * (flags & 1) + (flags >> 1 & 1)
    for N, shards in ((1, 1), (65, 1), (300, 1), (301, 2)):
        case = _Case(device, _batch(device, flags, N, mixed_timers=(N == 65)), action_dtype, shards)
        for normalized, t0 in ((True, 0), (False, 37), (True, 37), (False, 0)):
            acts = _actions(device, max(KS), N, A, action_dtype, normalized, seed=N + t0)
            hot(1)                                # (single steps never take the fused kernels)
            ref_r, ref_s, ref_states = case.single_steps(acts, normalized, t0, KS)
            for K in KS:
                hot(1)
                r1, s1, st1 = case.launch(acts[:K], normalized, t0)
                hot(0)
                r0, s0, st0 = case.launch(acts[:K], normalized, t0)
                what = (flags, N, normalized, t0, K)
                _same(r1, r0, ("reward vs step_k_kernel", what)); _same(s1, s0, ("soc vs step_k_kernel", what))
                _same_state(st1, st0, ("vs step_k_kernel", what))
                _same(r1, ref_r[:K], ("reward vs single steps", what))
                _same(s1, None if ref_s is None else ref_s[:K], ("soc vs single steps", what))
                _same_state(st1, ref_states[K], ("vs single steps", what))
        case.close()


@pytest.mark.gpu
def test_both_loop_forms_in_one_launch(device, hot):
    """Gensets with start-up / wind-down times > 0 in some waves only: the first two waves are instantaneous (the form without
    the status machine), the others are not; ret_acc rides along."""
    N, K, t0 = 300, 2 * U + 3, 37
    b = _batch(device, 3, N, seed=9, mixed_timers=True)
    assert int((b.cols["gen_times"][128:] != 0).sum()) > 0
    b.cols["gen_times"][:128] = 0
    b.cols["gen_status"][:128] = 0x0101
    b.cols["gen_status"][:128:3] = 0
    case = _Case(device, b, torch.float64)
    acts = _actions(device, K, N, 3, torch.float64, True, seed=2)
    ref_r, ref_s, ref_states = case.single_steps(acts, True, t0, (K,))
    acc = {}
    for v in (1, 0):
        hot(v)
        acc[v] = torch.full((N,), 3.0, dtype=torch.float64, device=device)
        r, s, st = case.launch(acts, True, t0, ret_acc=acc[v])
        _same(r, ref_r, ("reward", v)); _same(s, ref_s, ("soc", v)); _same_state(st, ref_states[K], v)
    assert torch.equal(acc[1], acc[0])
    case.close()


@pytest.mark.gpu
@pytest.mark.parametrize("action_dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_special_values_in_the_controls(action_dtype, device, hot):
    """NaN, +-inf and -0.0 among the controls: the same bits from both kernels (NaN results included: compared as bit patterns)."""
    N, K = 300, U + 1
    case = _Case(device, _batch(device, 3, N, mixed_timers=True), action_dtype)
    for normalized in (True, False):
        acts = _actions(device, K, N, 3, action_dtype, normalized, seed=11)
        flat = acts.view(-1)
        for j, v in enumerate((float("nan"), float("inf"), float("-inf"), -0.0)):
            flat[j + 1::7 + j] = v
        res = {}
        for v in (1, 0):
            hot(v)
            r, s, st = case.launch(acts, normalized, 0)
            res[v] = (r.view(torch.int64), s.view(torch.int64), {k: (t.view(torch.int64) if t.dtype == torch.float64 else t) for k, t in st.items()})
        _same(res[1][0], res[0][0], ("reward", normalized)); _same(res[1][1], res[0][1], ("soc", normalized))
        _same_state(res[1][2], res[0][2], normalized)
    case.close()


@pytest.mark.gpu
def test_launch_cut_short_at_the_end_of_the_series(device, hot):
    """Device-resident counter, K = 64 from row T - 20: resolve_k drops the 44 steps past the series (and flags the overrun); the 20
    steps that run equal step_k_kernel's and 20 single steps, the rows of the dropped steps are not written."""
    from pymgrid_amd import MgxError
    N, K, left = 300, 64, 20
    t0 = T - left
    case = _Case(device, _batch(device, 3, N, mixed_timers=True), torch.float64)
    acts = _actions(device, K, N, 3, torch.float64, True, seed=4)
    ref_r, ref_s, ref_states = case.single_steps(acts[:left], True, t0, (left,))
    case.eng.use_device_counter(True)
    for v in (1, 0):
        hot(v)
        r, s, st = case.launch(acts, True, t0)
        _same(r[:left], ref_r, ("reward", v)); _same(s[:left], ref_s, ("soc", v)); _same_state(st, ref_states[left], v)
        assert bool((r[left:] == SENTINEL).all()) and bool((s[left:] == SENTINEL).all()), v
    with pytest.raises(MgxError):
        case.eng.use_device_counter(False)
    case.close()


def test_hot_kernel_resource_figures():
    """Every form of the new kernel: no scratch memory, no VGPR spills, no AGPRs, at least two waves per SIMD."""
    from pymgrid_amd import _lib
    usage = _lib.resource_usage()
    if not usage:
        pytest.skip("no resource_usage.json: the library was not built on this machine")
    forms = {k: v for k, v in usage.items() if "step_k_hot_kernel<" in k}
    assert len(forms) == 6, sorted(forms)             # layouts 1, 2, 3 x double / float controls
    for name, u in forms.items():
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["agpr"] == 0 and u["occupancy"] >= 2 and u["vgpr"] <= 256, (name, u)
