"""The lock-step fused kernels (step_k_kernel / rollout_kernel) on ALL ten module layouts they are compiled for, in every
specialisation: materialised and factorised series, float64 and float32 controls, the HOT / lean / RICH forms of the loop, `done` as
bytes and as bits, gensets with and without timers (the GI form), more than one workgroup with a partial last wave, launches of
K = 1, 7 and 140 steps from counter values 0, 1 and 8 (below the ring depth 8 and above 4; past the 128-row LDS chunk and across
the outage words at rows 64 and 128), and shards.  Rewards and final state against the CPU oracle, traces / log / done against
single steps of a twin engine -- bit for bit.  The batches are carved out of one generated batch (tests/layouts.py)."""
import functools
import itertools

import numpy as np
import pytest
import torch

from layouts import F_BATTERY, F_GENSET, LAYOUTS, carve

pytestmark = pytest.mark.gpu

N, T, SEED = 600, 300, 9                # four workgroups of 192 grids, the last holds 24: a partial wave; shards: 512 + 88
LAUNCHES = (1, 7, 140)                  # consecutive launches on one engine: the counter starts at 0, 1, 8
K_SHARDS = 16
K_HOT, K_END = 9, 7                     # roll-out: a hot launch; both: the last 7 rows of the series, the last step ends the episode
SERIES = ("materialised", "factorised")
DTYPES = (torch.float64, torch.float32)
FORMS = ("hot", "lean", "rich")         # every step_k case runs all three on twin engines
STEP_K_CASES = tuple(itertools.product(LAYOUTS, SERIES, DTYPES))
ROLLOUT_CASES = tuple(itertools.product(LAYOUTS, SERIES, ("per_step", "fixed"), ("lean", "rich")))
STATE = ("charge", "soc", "gen_status")


@functools.lru_cache(maxsize=None)
def _full(device, series, mixed):
    from pymgrid_amd.generator import generate
    return generate(N, n_steps=T, seed=SEED, arch="genset+battery+grid", device=device, mixed_timers=mixed, series=series)


@functools.lru_cache(maxsize=None)
def _oracle_columns(device, flags, series, mixed):
    """Host columns of the carved batch (a factorised one materialised): the oracle's input, shared by the tests and left unchanged."""
    return carve(_full(device, series, mixed), flags).numpy_columns()


def _state(cols):
    return {k: cols[k].copy() for k in STATE if k in cols}


def _state_equals(batch, st, where):
    for name, want in st.items():
        got = batch.cols[name].cpu().numpy()
        assert np.array_equal(got.view(np.uint32) if name == "gen_status" else got, want), (where, name)


def _reference_ret(reward):
    """ret_acc of one launch: the kernel adds the K rewards in step order, then the sum to the accumulator."""
    ret = torch.zeros_like(reward[0])
    for k in range(reward.shape[0]):
        ret = ret + reward[k]
    return ret


@pytest.mark.parametrize("mixed", [True, False], ids=["timers", "instant"])
@pytest.mark.parametrize("flags,series,dtype", STEP_K_CASES)
def test_step_k_on_every_layout(flags, series, dtype, mixed, device, oracle):
    from pymgrid_amd import StepEngine
    hot, lean, rich, twin = (StepEngine(carve(_full(device, series, mixed), flags), action_dtype=dtype) for _ in range(4))
    L = hot.layout
    A = L.action_dim
    assert A == 2 * bool(flags & F_GENSET) + bool(flags & F_BATTERY) + bool(flags & 4) and hot.action_dim == A
    total = sum(LAUNCHES) + K_SHARDS
    gen = torch.Generator(device=device); gen.manual_seed(1000 * flags + 5)
    acts = torch.rand(total, N, A, dtype=torch.float64, device=device, generator=gen)     # (layout 0: [K, N, 0])
    acts[::7] = acts[::7].round()       # exact 0 / 1 controls: x == 0 routing, goal exactly 0 / 1
    acts = acts.to(dtype).contiguous()
    cols = _oracle_columns(device, flags, series, mixed)
    st = _state(cols)
    failed = np.zeros(N, dtype=np.uint8)
    # (float32 controls: the oracle takes them widened to float64, what the kernels do)
    ref = oracle.run_batch(cols, st, 0, total, acts.double().cpu().numpy(), normalized=True, nthreads=8, failed=failed)
    assert int(failed.sum()) == 0
    ref = torch.from_numpy(ref).to(device)
    ret_acc = torch.zeros(N, dtype=torch.float64, device=device)
    ret_ref = torch.zeros_like(ret_acc)
    t = 0
    for K in LAUNCHES:
        a = acts[t:t + K]
        assert hot.current_step == lean.current_step == rich.current_step == twin.current_step == t
        bits = K == 7
        lean.set_done_format(bits)
        out_hot = hot.step_k(a, reward=True, soc_trace=True)
        out_lean = lean.step_k(a, reward=True, done=True, soc_trace=True, ret_acc=ret_acc)
        out_rich = rich.step_k(a, reward=True, done=True, soc_trace=True, status_trace=True, log=True)
        single = {k: [] for k in ("reward", "done", "soc_trace", "status_trace", "log")}
        for k in range(K):
            _, r, d, lg = twin.step(a[k], want_obs=False, want_log=True)
            single["reward"].append(r.clone()); single["done"].append(d.clone()); single["log"].append(lg.clone())
            if L.has_battery:
                single["soc_trace"].append(twin.batch.cols["soc"].clone())
            if L.has_genset:
                single["status_trace"].append(twin.batch.cols["gen_status"].clone())
        single = {k: torch.stack(v) for k, v in single.items() if v}
        assert set(out_hot) == {"reward"} | ({"soc_trace"} if L.has_battery else set()), sorted(out_hot)
        assert set(out_lean) == set(out_hot) | {"done", "ret_acc"}, sorted(out_lean)
        assert set(out_rich) == set(single), (sorted(out_rich), sorted(single))
        if bits:
            assert out_lean["done"].shape == (K, (N + 15) // 16) and out_lean["done"].dtype == torch.int16
            out_lean["done"] = lean.unpack_done_bits(out_lean["done"]).to(torch.uint8)
        ret_ref = ret_ref + _reference_ret(out_lean["reward"])
        for form, out in (("hot", out_hot), ("lean", out_lean), ("rich", out_rich)):
            assert torch.equal(out["reward"], ref[t:t + K]), (form, K, "reward vs the oracle")
            for name, v in out.items():
                if name == "ret_acc":
                    assert torch.equal(v, ret_ref), (form, K, name)
                else:
                    assert v.shape == single[name].shape and torch.equal(v, single[name]), (form, K, name)
        for form, e in (("hot", hot), ("lean", lean), ("rich", rich)):
            for name in STATE:
                if name in e.batch.cols:
                    assert torch.equal(e.batch.cols[name], twin.batch.cols[name]), (form, K, name)
        t += K
    lean.set_done_format(False)
    # shards: two grid ranges (512 + 88) on streams of their own, between fork() and join()
    a = acts[t:t + K_SHARDS]
    for form, e in (("hot", hot), ("lean", lean), ("rich", rich)):
        e.set_shards(2)
        e.fork()
        out = e.step_k(a, reward=True, done=form != "hot", soc_trace=True, status_trace=form == "rich", log=form == "rich")
        e.join()
        assert torch.equal(out["reward"], ref[t:t + K_SHARDS]), (form, "shards")
        if "soc_trace" in out:
            assert torch.equal(out["soc_trace"][-1], e.batch.cols["soc"]), (form, "shards")
        if "done" in out:
            assert not bool(out["done"].any()), (form, "shards")                 # rows 148 .. 163 of 300
        assert e.current_step == total
        _state_equals(e.batch, st, (form, "final state vs the oracle"))
        e.set_shards(1)
    # the last K_END rows of the series (a reset keeps the module state): `done` is set in the last step, on every grid -- as
    # bits (600 = 37 words + 8 bits) and as bytes
    t_end = T - K_END
    a = acts[:K_END].contiguous()
    ref = oracle.run_batch(cols, st, t_end, K_END, a.double().cpu().numpy(), normalized=True, nthreads=8, failed=failed)
    assert int(failed.sum()) == 0
    twin.batch.load_state(rich.batch.state())
    for e in (hot, lean, rich, twin):
        e.reset(t_end, want_obs=False)
    single_done = torch.stack([twin.step(a[k], want_obs=False)[2].clone() for k in range(K_END)])
    assert bool(single_done[-1].all()) and not bool(single_done[:-1].any())
    lean.set_done_format(True)
    outs = dict(hot=hot.step_k(a, reward=True, soc_trace=True), lean=lean.step_k(a, reward=True, done=True, soc_trace=True),
                rich=rich.step_k(a, reward=True, done=True, soc_trace=True, status_trace=True, log=True))
    words = outs["lean"]["done"]
    assert words.shape == (K_END, (N + 15) // 16) and not bool(words[:-1].any())
    assert bool((words[-1, :-1] == -1).all()) and int(words[-1, -1]) == (1 << (N % 16)) - 1      # int16: sixteen set bits are -1
    outs["lean"]["done"] = lean.unpack_done_bits(words).to(torch.uint8)
    for form, e in (("hot", hot), ("lean", lean), ("rich", rich)):
        assert np.array_equal(outs[form]["reward"].cpu().numpy(), ref), (form, "end of the series")
        if form != "hot":
            assert torch.equal(outs[form]["done"], single_done), (form, "done at the end of the series")
        assert e.current_step == T
        _state_equals(e.batch, st, (form, "state at the end of the series vs the oracle"))
    for e in (hot, lean, rich, twin):
        e.close()


@pytest.mark.parametrize("mixed", [True, False], ids=["timers", "instant"])
@pytest.mark.parametrize("flags,series,ids_form,form", ROLLOUT_CASES)
def test_rollout_discrete_on_every_layout(flags, series, ids_form, form, mixed, device, oracle):
    from pymgrid_amd import StepEngine
    from pymgrid_amd.priority_list import get_priority_lists, table_array
    e = StepEngine(carve(_full(device, series, mixed), flags))
    L = e.layout
    lists = get_priority_lists(L.has_genset, L.has_battery, L.has_grid, False, L.grid_before_battery)
    assert len(lists) == {0: 1, 1: 2, 2: 1, 3: 4, 4: 1, 5: 4, 6: 2, 7: 12, 14: 2, 15: 12}[flags]
    table = table_array(lists)
    rich = form == "rich"
    gen = torch.Generator(device=device); gen.manual_seed(1000 * flags + 7)
    fixed = torch.randint(0, len(lists), (N,), device=device, generator=gen).to(torch.uint8)
    cols = _oracle_columns(device, flags, series, mixed)
    st = _state(cols)
    failed = np.zeros(N, dtype=np.uint8)
    reward_col = e.log_names.index("reward")
    t = 0
    for K in LAUNCHES + (K_SHARDS,):
        shards = t == sum(LAUNCHES)
        ids = torch.randint(0, len(lists), (K, N), device=device, generator=gen).to(torch.uint8) if ids_form == "per_step" else fixed
        assert e.current_step == t
        if shards:
            e.set_shards(2)
            e.fork()
        out = e.rollout_discrete(ids, table, K, reward=True, done=True, soc_trace=True, status_trace=rich, log=rich)
        if shards:
            e.join()
        ref = oracle.rollout_batch(cols, st, t, K, ids.cpu().numpy(), table, nthreads=8, failed=failed)
        assert int(failed.sum()) == 0, (K, int(failed.sum()))
        want = {"reward", "done"} | ({"soc_trace"} if L.has_battery else set()) \
            | ({"log"} if rich else set()) | ({"status_trace"} if rich and L.has_genset else set())
        assert set(out) == want, sorted(out)
        assert out["reward"].shape == (K, N) and np.array_equal(out["reward"].cpu().numpy(), ref), (K, "reward vs the oracle")
        _state_equals(e.batch, st, (K, "state vs the oracle"))
        assert not bool(out["done"].any())                                       # rows 0 .. 163 of 300
        if "soc_trace" in out:
            assert torch.equal(out["soc_trace"][-1], e.batch.cols["soc"]), K
        if "status_trace" in out:
            assert torch.equal(out["status_trace"][-1], e.batch.cols["gen_status"]), K
        if rich:
            assert out["log"].shape == (K, e.log_dim, N) and torch.equal(out["log"][:, reward_col], out["reward"]), K
        t += K
    e.set_shards(1)
    per_step = ids_form == "per_step"
    # HOT: reward + SoC only (no `done`, no trace, no log), whatever form the case's other launches take
    ids = torch.randint(0, len(lists), (K_HOT, N), device=device, generator=gen).to(torch.uint8) if per_step else fixed
    out = e.rollout_discrete(ids, table, K_HOT, reward=True, soc_trace=True)
    ref = oracle.rollout_batch(cols, st, t, K_HOT, ids.cpu().numpy(), table, nthreads=8, failed=failed)
    assert set(out) == {"reward"} | ({"soc_trace"} if L.has_battery else set())
    assert int(failed.sum()) == 0 and np.array_equal(out["reward"].cpu().numpy(), ref), "hot"
    _state_equals(e.batch, st, "hot")
    # the last K_END rows of the series (a reset keeps the module state): `done` in the last step, as bits
    e.reset(T - K_END, want_obs=False)
    e.set_done_format(True)
    ids = torch.randint(0, len(lists), (K_END, N), device=device, generator=gen).to(torch.uint8) if per_step else fixed
    out = e.rollout_discrete(ids, table, K_END, reward=True, done=True, soc_trace=True, status_trace=rich, log=rich)
    ref = oracle.rollout_batch(cols, st, T - K_END, K_END, ids.cpu().numpy(), table, nthreads=8, failed=failed)
    assert int(failed.sum()) == 0 and np.array_equal(out["reward"].cpu().numpy(), ref), "end of the series"
    _state_equals(e.batch, st, "end of the series")
    assert out["done"].shape == (K_END, (N + 15) // 16)
    done = e.unpack_done_bits(out["done"])
    assert bool(done[-1].all()) and not bool(done[:-1].any()) and e.current_step == T
    e.close()


# ---- the workgroup sizes 208 / 224 / 240 / 256 -----------------------------------------------------------------------------------
def grids_per_block(n, cus):
    """The host's rule (fused_grids_per_block): the multiple of 16 grids in [192, 256] that minimises what the busiest CU streams,
    ceil(workgroups / CUs) * grids per workgroup; the larger size on a tie."""
    best, best_cost = 256, -1
    for g in range(256, 191, -16):
        blocks = -(-n // g)
        cost = -(-blocks // cus) * g
        if best_cost < 0 or cost < best_cost:
            best, best_cost = g, cost
    return best


WORKGROUP_N = (50_001, 55_003, 59_001, 63_001)               # 208, 224, 240, 256 grids per workgroup on 256 CUs


def workgroup_cases(cus):
    """[(N, grids per workgroup)]: WORKGROUP_N where the device's CU count gives them four different sizes, else one N per size
    out of the rule itself (cus * g - 7 grids make exactly `cus` workgroups of g: larger workgroups cost more per CU, smaller ones
    need a second round -- whatever the CU count).  The size is the mirrored rule's: the launch shape is not visible from outside,
    so a host that picked another size would pass here as long as its kernels are right at that size."""
    cases = [(n, grids_per_block(n, cus)) for n in WORKGROUP_N]
    if len({g for _, g in cases}) != 4:
        cases = [(cus * g - 7, grids_per_block(cus * g - 7, cus)) for g in (208, 224, 240, 256)]
    return cases


@pytest.mark.parametrize("which", range(4))
def test_every_workgroup_size_of_the_fused_launch(which, device, oracle):
    """Layout 7, factorised series, the hot form and a launch with `done` as bits, K = 9 twice from row 6 of 24 (the second launch
    ends the episode), at grid counts for which the host picks 208, 224, 240 and 256 grids per workgroup (every N <= 49 152 runs
    with 192)."""
    from pymgrid_amd import StepEngine
    from pymgrid_amd.generator import generate
    cases = workgroup_cases(torch.cuda.get_device_properties(device).multi_processor_count)
    sizes = [g for _, g in cases]
    assert len(set(sizes)) == 4 and 192 not in sizes, cases
    n, size = cases[which]
    Tw, K, t0 = 24, 9, 6
    assert n % size and n % 64
    b = generate(n, n_steps=Tw, seed=SEED, arch="genset+battery+grid", device=device, mixed_timers=True, series="factorised")
    cols = b.numpy_columns()
    st = _state(cols)
    e = StepEngine(b)
    e.reset(t0, want_obs=False)
    gen = torch.Generator(device=device); gen.manual_seed(which)
    acts = torch.rand(2 * K, n, 4, dtype=torch.float64, device=device, generator=gen)
    failed = np.zeros(n, dtype=np.uint8)
    ref = oracle.run_batch(cols, st, t0, 2 * K, acts.cpu().numpy(), normalized=True, nthreads=8, failed=failed)
    assert int(failed.sum()) == 0
    out = e.step_k(acts[:K], reward=True, soc_trace=True)                        # hot
    assert np.array_equal(out["reward"].cpu().numpy(), ref[:K])
    e.set_done_format(True)
    out = e.step_k(acts[K:], reward=True, done=True, soc_trace=True)
    assert np.array_equal(out["reward"].cpu().numpy(), ref[K:])
    assert out["done"].shape == (K, (n + 15) // 16)
    done = e.unpack_done_bits(out["done"])
    want = (torch.arange(t0 + K, t0 + 2 * K, device=device) >= Tw - 1)[:, None].expand(K, n)
    assert torch.equal(done, want) and bool(done[-1].all()) and not bool(done[:-1].any())
    assert torch.equal(out["soc_trace"][-1], b.cols["soc"])
    _state_equals(b, st, (n, size))
    e.close()
