"""step_k_hot_kernel's control path (csrc/mgx_step_hot.hip): a wave loads the controls of a row as consecutive elements and hands every
lane its own grid's controls through a wave-private LDS tile, one step ahead.  The launch
must still compute, bit for bit, what step_k_kernel computes for it (tunable step_k_hot = 0) and what the CPU oracle computes: reward,
SoC trace, the state columns after the launch and ret_acc -- at the shapes where the new code can go wrong: partial waves, the 16-lane
fourth wave of a 208-grid workgroup, ragged last workgroups, a second workgroup, K around the ring depth / the peeled first group /
the guarded groups / the tail, both control types, every layout, shards, a control tensor that is a view, consecutive launches."""
import numpy as np
import pytest
import torch

from test_step_k_hot import STATE, _actions, _batch, _Case, _same, _same_state, hot    # noqa: F401  (hot: the tunable's fixture)

pytestmark = pytest.mark.gpu

NS = (1, 15, 16, 17, 63, 64, 65, 207, 208, 209, 224, 208 * 2 + 48)       # grids per shard
KS = (1, 2, 7, 8, 9, 15, 16, 17, 23, 64)
LAYOUTS = {1: "genset", 2: "battery", 3: "genset+battery"}


def _np_state(state):
    return {k: (v.cpu().numpy().view(np.uint32) if k == "gen_status" else v.cpu().numpy()).copy() for k, v in state.items()}


def _oracle_steps(oracle, case, acts, normalized, t0, stops):
    """The CPU oracle over acts.shape[0] steps from the case's starting state, one step per call: (reward [K, N], SoC [K, N] or None,
    {K: state after K steps} for K in stops).  Float32 controls enter widened, as the kernel widens them."""
    cols = case.batch.numpy_columns()
    st = _np_state(case.state0)
    a = acts.double().cpu().numpy()
    rew, soc, states = [], [], {}
    for k in range(a.shape[0]):
        rew.append(oracle.run_batch(cols, st, t0 + k, 1, a[k:k + 1], normalized=normalized)[0])
        if case.has_battery:
            soc.append(st["soc"].copy())
        if k + 1 in stops:
            states[k + 1] = {n: v.copy() for n, v in st.items()}
    return np.stack(rew), (np.stack(soc) if case.has_battery else None), states


def _ret(acc0, reward):
    """ret_acc after a launch: the kernel sums a grid's rewards in step order from 0.0 and adds the sum to what was there."""
    ret = np.zeros(reward.shape[1])
    for k in range(reward.shape[0]):
        ret = ret + reward[k]
    return acc0 + ret


def _check(case, oracle_rows, acts, normalized, t0, K, hot, what):
    """One launch of K steps by both kernels from the starting state: equal to each other and to the oracle's first K steps."""
    ref_r, ref_s, ref_states = oracle_rows
    res = {}
    for v in (1, 0):
        hot(v)
        acc = torch.full((case.N,), 3.0, dtype=torch.float64, device=case.device)
        r, s, st = case.launch(acts[:K], normalized, t0, ret_acc=acc)
        res[v] = (r.clone(), None if s is None else s.clone(), st, acc)
    r1, s1, st1, acc1 = res[1]
    r0, s0, st0, acc0 = res[0]
    _same(r1, r0, ("reward vs step_k_kernel", what)); _same(s1, s0, ("soc vs step_k_kernel", what))
    _same_state(st1, st0, ("vs step_k_kernel", what))
    assert torch.equal(acc1, acc0), ("ret_acc vs step_k_kernel", what)
    assert np.array_equal(r1.cpu().numpy(), ref_r[:K]), ("reward vs oracle", what)
    if s1 is not None:
        assert np.array_equal(s1.cpu().numpy(), ref_s[:K]), ("soc vs oracle", what)
    got = _np_state(st1)
    for name, v in ref_states[K].items():
        assert np.array_equal(got[name], v), (name, "vs oracle", what)
    assert np.array_equal(acc1.cpu().numpy(), _ret(np.full(case.N, 3.0), ref_r[:K])), ("ret_acc vs oracle", what)


@pytest.mark.parametrize("action_dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("flags", [1, 2, 3], ids=[LAYOUTS[f] for f in (1, 2, 3)])
def test_tile_path_every_wave_shape_and_k(flags, action_dtype, device, oracle, hot):
    """One shard of every size in NS x every K in KS (normalised controls for even N, raw ones for odd N; row 0 and row 37)."""
    A = 2 * (flags & 1) + (flags >> 1 & 1)
    for N in NS:
        normalized, t0 = N % 2 == 0, 37 * (N % 3 == 0)
        case = _Case(device, _batch(device, flags, N, seed=N, mixed_timers=(N in (65, 209))), action_dtype)
        acts = _actions(device, max(KS), N, A, action_dtype, normalized, seed=N + 1)
        rows = _oracle_steps(oracle, case, acts, normalized, t0, KS)
        for K in KS:
            _check(case, rows, acts, normalized, t0, K, hot, (flags, N, K))
        case.close()


@pytest.mark.parametrize("action_dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("flags", [1, 2, 3], ids=[LAYOUTS[f] for f in (1, 2, 3)])
def test_tile_path_two_shards_uneven_split(flags, action_dtype, device, oracle, hot):
    """Two shards on their own streams, split unevenly by the engine (the second shard starts at a multiple of 16 grids): a ragged
    last workgroup in each, a second workgroup in the larger ones."""
    A = 2 * (flags & 1) + (flags >> 1 & 1)
    for N in (33, 301, 2 * (208 * 2 + 48) + 17):
        case = _Case(device, _batch(device, flags, N, seed=N, mixed_timers=True), action_dtype, shards=2)
        acts = _actions(device, 23, N, A, action_dtype, True, seed=N)
        rows = _oracle_steps(oracle, case, acts, True, 5, (9, 23))
        for K in (9, 23):
            _check(case, rows, acts, True, 5, K, hot, (flags, N, K, "two shards"))
        case.close()


@pytest.mark.parametrize("action_dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("flags", [1, 2, 3], ids=[LAYOUTS[f] for f in (1, 2, 3)])
def test_tile_path_controls_are_a_view_one_row_into_a_buffer(flags, action_dtype, device, oracle, hot):
    """The controls start one row into a larger buffer whose other rows hold NaN: with odd N and float32 (or one or three float64
    controls) a row then starts off the 128-byte lines, and nothing outside rows [0, K) may reach a result."""
    A = 2 * (flags & 1) + (flags >> 1 & 1)
    for N, K in ((209, 17), (65, 8), (17, 64)):
        case = _Case(device, _batch(device, flags, N, seed=N + 3, mixed_timers=True), action_dtype)
        buf = torch.full((K + 2, N, A), float("nan"), dtype=action_dtype, device=device)
        buf[1:K + 1] = _actions(device, K, N, A, action_dtype, True, seed=N + K)
        acts = buf[1:K + 1]
        assert acts.data_ptr() == buf.data_ptr() + N * A * buf.element_size() and acts.is_contiguous()
        rows = _oracle_steps(oracle, case, acts, True, 0, (K,))
        _check(case, rows, acts, True, 0, K, hot, (flags, N, K, "view"))
        case.close()


@pytest.mark.parametrize("action_dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_tile_path_consecutive_launches_carry_the_state(action_dtype, device, oracle, hot):
    """Two launches on one handle without a reset in between (K = 9, then 17): the second starts from the state and the row the first
    left; both kernels and the oracle's 26 steps agree."""
    N, K1, K2, t0 = 209, 9, 17, 3
    case = _Case(device, _batch(device, 3, N, seed=21, mixed_timers=True), action_dtype)
    acts = _actions(device, K1 + K2, N, 3, action_dtype, True, seed=8)
    ref_r, ref_s, ref_states = _oracle_steps(oracle, case, acts, True, t0, (K1 + K2,))
    res = {}
    for v in (1, 0):
        hot(v)
        case.restore(t0)
        o1 = case.eng.step_k(acts[:K1], normalized=True, reward=True, soc_trace=True)
        o2 = case.eng.step_k(acts[K1:], normalized=True, reward=True, soc_trace=True)
        torch.cuda.synchronize(device)
        res[v] = (torch.cat([o1["reward"], o2["reward"]]), torch.cat([o1["soc_trace"], o2["soc_trace"]]), case.state())
        assert case.eng.current_step == t0 + K1 + K2
    _same(res[1][0], res[0][0], "reward vs step_k_kernel"); _same(res[1][1], res[0][1], "soc vs step_k_kernel")
    _same_state(res[1][2], res[0][2], "vs step_k_kernel")
    assert np.array_equal(res[1][0].cpu().numpy(), ref_r) and np.array_equal(res[1][1].cpu().numpy(), ref_s)
    got = _np_state(res[1][2])
    for name, v in ref_states[K1 + K2].items():
        assert np.array_equal(got[name], v), name
    case.close()
