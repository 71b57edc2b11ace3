"""Microgrids with several gensets / batteries / grids (the reference's container takes any number of modules per name,
module_container.py:355-413): the CPU oracle against fixtures made by the real reference (tests/golden/multi.npz), and the
device's general kernels against both."""
import numpy as np
import pytest

from conftest import multi_cases
from layouts import random_multi_grid as _random_multi_grid


def test_multi_instance_oracle_vs_reference(oracle):
    """orc_mrun / orc_mobserve / orc_mpopulate_action == the reference on 7 module mixes (up to 4 gensets + 3 batteries +
    2 grids + 3 loads + 2 pvs: lists of >= 8 addends go through numpy's pairwise sum), normalised and raw controls: reward,
    done, every log column of every module instance, observations, expanded priority lists."""
    for ci, p, mt, z in multi_cases():
        names = [str(s) for s in z[f"c{ci}_log_names"]]
        for tag, normalized in (("n", True), ("r", False)):
            om = oracle.OracleMultiMicrogrid(p)
            assert np.array_equal(om.reset(), z[f"c{ci}_{tag}_obs0"]), (ci, tag)
            a = z[f"c{ci}_{tag}_actions"]
            for k in range(a.shape[0]):
                out = om.run(a[k], normalized)
                for n, v, r in zip(names, om.log_row(out, names), z[f"c{ci}_{tag}_log"][k]):
                    assert v is not None and v == r, (ci, tag, k, n, v, r)
                assert out.common.reward == z[f"c{ci}_{tag}_reward"][k] and out.common.done == z[f"c{ci}_{tag}_done"][k]
                assert np.array_equal(om.observe(), z[f"c{ci}_{tag}_obs"][k]), (ci, tag, k)
            for j in range(om.counts["battery"]):
                assert om.s.battery[j].charge == z[f"c{ci}_{tag}_charge"][-1, j]
                assert om.s.battery[j].soc == z[f"c{ci}_{tag}_soc"][-1, j]
            for j in range(om.counts["genset"]):
                st = om.s.genset[j]
                assert [st.gen_cur, st.gen_goal, st.gen_up, st.gen_down] == list(z[f"c{ci}_{tag}_status"][-1, j])
        if mt["n_lists"]:
            om = oracle.OracleMultiMicrogrid(p)
            table, ids = z[f"c{ci}_pl_table"], z[f"c{ci}_ids"]
            for k in range(len(ids)):
                ctrl = om.populate_action([tuple(int(x) for x in e) for e in table[ids[k]] if e[0] >= 0])
                assert np.array_equal(ctrl, z[f"c{ci}_control"][k]), (ci, k)
                assert om.run(ctrl, False).common.reward == z[f"c{ci}_dreward"][k], (ci, k)


def _unpack(word):
    w = int(word)
    return [w & 0xff, (w >> 8) & 0xff, (w >> 16) & 0xff, w >> 24]


def _check_log_row(names, dev_row, ref_names, ref_row, ctx):
    dev = dict(zip(names, dev_row))
    for n, r in zip(ref_names, ref_row):
        base, sfx = (n[:n.index("[")], n[n.index("["):]) if n.endswith("]") else (n, "")
        if base in ("gen_cur", "gen_goal", "gen_up", "gen_down"):
            v = _unpack(dev["genset_status" + sfx])[("gen_cur", "gen_goal", "gen_up", "gen_down").index(base)]
        else:
            v = dev[n]
        assert v == r, (*ctx, n, v, r)


@pytest.mark.gpu
def test_multi_instance_device_vs_reference(device):
    """The general kernels on the reference-made fixtures: two copies of every module mix in one batch; observations (reset
    and per step), reward, done, every log column of every module instance, final state -- all ==."""
    import torch
    from pymgrid_amd import BatchedMicrogridEnv, MicrogridBatch
    for ci, p, mt, z in multi_cases():
        ref_names = [str(s) for s in z[f"c{ci}_log_names"]]
        for tag, normalized in (("n", True), ("r", False)):
            env = BatchedMicrogridEnv(MicrogridBatch.from_grids([p, p], device=device), log=True)
            L = env.layout
            assert (L.n_genset, L.n_battery, L.n_grid) == (len(mt["genset"]), len(mt["battery"]), len(mt["grid"])) and L.multi
            assert np.array_equal(env.reset().cpu().numpy()[1], z[f"c{ci}_{tag}_obs0"]), (ci, tag)
            a = z[f"c{ci}_{tag}_actions"]
            names = env.engine.log_names
            assert names == L.log_names and len(names) == env.engine.log_dim
            for k in range(a.shape[0]):
                act = torch.as_tensor(np.stack([a[k], a[k]]), dtype=torch.float64, device=device)
                obs, reward, done, info = env.step(act, normalized=normalized)
                assert reward[0].item() == z[f"c{ci}_{tag}_reward"][k] == reward[1].item(), (ci, tag, k)
                assert int(done[1]) == z[f"c{ci}_{tag}_done"][k]
                assert np.array_equal(obs[0].cpu().numpy(), z[f"c{ci}_{tag}_obs"][k]), (ci, tag, k)
                _check_log_row(names, info["log"][:, 1].cpu().numpy(), ref_names, z[f"c{ci}_{tag}_log"][k], (ci, tag, k))
            if L.has_battery:
                assert np.array_equal(env.batch.cols["charge"].reshape(L.n_battery, 2)[:, 0].cpu().numpy(), z[f"c{ci}_{tag}_charge"][-1])
                assert np.array_equal(env.batch.cols["soc"].reshape(L.n_battery, 2)[:, 1].cpu().numpy(), z[f"c{ci}_{tag}_soc"][-1])
            if L.has_genset:
                st = env.batch.cols["gen_status"].reshape(L.n_genset, 2)[:, 0].cpu().numpy().view(np.uint32)
                assert [_unpack(w) for w in st] == z[f"c{ci}_{tag}_status"][-1].tolist()
            env.close()


@pytest.mark.gpu
def test_multi_instance_discrete_env_vs_reference(device):
    """DiscreteBatchedMicrogridEnv on microgrids with several gensets / batteries / grids: the priority lists over module
    instances are the reference's (same order, so the same action ids), the expanded controls and the rewards are ==; the
    N = 1 adaptor returns the reference's nested shapes."""
    import torch
    from pymgrid_amd import DiscreteBatchedMicrogridEnv, DiscreteMicrogridEnv, MicrogridBatch
    from pymgrid_amd.priority_list import lists_array
    for ci, p, mt, z in multi_cases():
        if not mt["n_lists"]:
            continue
        env = DiscreteBatchedMicrogridEnv(MicrogridBatch.from_grids([p, p, p], device=device))
        assert env.action_space.n == mt["n_lists"]
        assert np.array_equal(lists_array(env.actions_list), z[f"c{ci}_pl_table"]), ci
        env.reset()
        ids = z[f"c{ci}_ids"]
        for k in range(len(ids)):
            a = torch.full((3,), int(ids[k]), dtype=torch.int32, device=device)
            assert np.array_equal(env.get_action(a)[2].cpu().numpy(), z[f"c{ci}_control"][k]), (ci, k)
            _, reward, _, _ = env.step(a)
            assert reward[0].item() == z[f"c{ci}_dreward"][k] == reward[2].item(), (ci, k)
        env.close()
        one = DiscreteMicrogridEnv(p, device=device, flat_spaces=False)
        obs = one.reset()
        L = one.layout
        assert [len(obs.get(k, [])) for k in ("load", "pv", "genset", "battery", "grid")] == \
            [L.n_load, L.n_pv, L.n_genset, L.n_battery, L.n_grid]
        ctrl = one.get_action_dict(int(ids[0]))
        flat = np.concatenate([np.concatenate(ctrl["genset"]) if L.n_genset else np.zeros(0),
                               np.array(ctrl.get("battery", [])), np.array(ctrl.get("grid", []))])
        assert np.array_equal(flat, z[f"c{ci}_control"][0])
        obs, reward, done, info = one.step(int(ids[0]))
        assert reward == z[f"c{ci}_dreward"][0] and isinstance(done, bool)
        # RuleBasedControl: the reference's marginal-cost order of the module instances, and its rewards over the series
        from pymgrid_amd import RuleBasedControl
        renv = DiscreteBatchedMicrogridEnv(MicrogridBatch.from_grids([p, p], device=device))
        rbc = RuleBasedControl(renv)
        assert np.array_equal(np.array(rbc.priority_list[1]), z[f"c{ci}_rbc_list"]), (ci, rbc.priority_list[1])
        r = rbc.run()["reward"].cpu().numpy()
        assert np.array_equal(r[:, 0], z[f"c{ci}_rbc_reward"]) and np.array_equal(r[:, 1], r[:, 0]), ci
        renv.close()
        twin = DiscreteMicrogridEnv.from_microgrid(one)           # parameters and state of every instance carry over
        for name in ("charge", "soc", "gen_status"):
            if name in one.batch.cols:
                assert torch.equal(twin.batch.cols[name], one.batch.cols[name])
        twin.close(); one.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mix", [(2, 2, 2, 2, 1, 2, False), (3, 0, 1, 1, 1, 0, False), (0, 3, 2, 1, 2, 1, True),
                                 (8, 8, 8, 3, 3, 0, False), (1, 2, 1, 0, 1, 0, True)])
def test_multi_instance_batches_vs_oracle(mix, device, oracle):
    """Randomised batches (every grid its own parameters, genset timers, outages): continuous steps with normalised and raw
    controls, the violations mask of the dry run, discrete steps through the instance priority lists, the rule-based
    rollout -- log, observations, state against the multi-instance CPU oracle."""
    import torch
    from pymgrid_amd import BatchedMicrogridEnv, DiscreteBatchedMicrogridEnv, MicrogridBatch, RuleBasedControl
    n_gen, n_bat, n_grid, n_load, n_pv, H, grid_first = mix
    rs = np.random.RandomState(hash(mix) % 2 ** 31)
    T, N, K = 40, 70, 30
    grids = [_random_multi_grid(rs, T, n_gen, n_bat, n_grid, n_load, n_pv, H, grid_first) for _ in range(N)]
    env = BatchedMicrogridEnv(MicrogridBatch.from_grids(grids, device=device), log=True)
    oms = [oracle.OracleMultiMicrogrid(g) for g in grids]
    names = env.engine.log_names
    A = env.layout.action_dim
    obs0 = env.reset().cpu().numpy()
    for j, om in enumerate(oms):
        assert np.array_equal(obs0[j], om.reset()), j
    for k in range(K):
        normalized = k % 3 != 2
        a = rs.rand(N, A)
        if not normalized:
            a = (a * 2 - 0.7) * 60
            c = 0
            for q in range(n_gen):
                a[:, c] = np.clip(np.round(a[:, c] / 60), 0, 1); a[:, c + 1] = np.abs(a[:, c + 1]); c += 2
        if k % 5 == 0:
            a[:, :2 * n_gen:2] = np.round(a[:, :2 * n_gen:2])
        act = torch.as_tensor(a, dtype=torch.float64, device=device)
        mask = env.engine.check_step(act, normalized=normalized).cpu().numpy()
        obs, reward, done, info = env.step(act, normalized=normalized)
        log, obs = info["log"].cpu().numpy(), obs.cpu().numpy()
        assert np.array_equal(mask, log[names.index("violations")].astype(mask.dtype)), k
        for j, om in enumerate(oms):
            out = om.run(a[j], normalized)
            for c, (n, v) in enumerate(zip(names, om.log_row(out, names))):
                if v is not None:
                    assert log[c, j] == v, (k, j, n, log[c, j], v)
            assert reward[j].item() == out.common.reward and bool(done[j]) == bool(out.common.done)
            assert np.array_equal(obs[j], om.observe()), (k, j)
    env.close()
    if 2 * n_gen + n_bat + n_grid > 9:
        return
    # discrete steps + rule-based rollout on fresh copies
    denv = DiscreteBatchedMicrogridEnv(MicrogridBatch.from_grids(grids, device=device), remove_redundant_gensets=False)
    oms = [oracle.OracleMultiMicrogrid(g) for g in grids]
    denv.reset()
    for k in range(12):
        ids = rs.randint(0, denv.action_space.n, size=N)
        control = denv.get_action(ids).cpu().numpy()
        _, reward, _, _ = denv.step(ids)
        for j, om in enumerate(oms):
            if denv._instances:
                plist = denv.actions_list[ids[j]]
            else:
                plist = [(m, 0, a_) for m, a_ in denv.actions_list[ids[j]]]
            ctrl = om.populate_action(plist)
            assert np.array_equal(control[j], ctrl), (k, j)
            assert reward[j].item() == om.run(ctrl, False).common.reward, (k, j)
    denv.close()
    denv = DiscreteBatchedMicrogridEnv(MicrogridBatch.from_grids(grids, device=device), remove_redundant_gensets=False)
    rbc = RuleBasedControl(denv, remove_redundant_gensets=False)
    res = rbc.run()
    r = res["reward"].cpu().numpy()
    assert r.shape == (T, N)
    for j, g in enumerate(grids):
        om = oracle.OracleMultiMicrogrid(g)
        plist = rbc.priority_list[j] if rbc._instances else [(m, 0, a_) for m, a_ in rbc.priority_list[j]]
        for k in range(T):
            assert r[k, j] == om.run(om.populate_action(plist), False).common.reward, (j, k)
    denv.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mix", [(2, 2, 1, 1, 1, 0, False), (1, 1, 1, 3, 2, 0, False), (0, 3, 2, 1, 2, 1, True),
                                 (8, 8, 8, 8, 8, 0, False)])
def test_fused_launches_on_the_general_path(mix, device):
    """mgx_step_k and mgx_rollout_lists on layouts with several modules of a kind (a K-step loop around the general step)
    == K single steps / K discrete env steps: rewards, done, log rows, traces, final state; also split over two shards."""
    import torch
    from pymgrid_amd import BatchedMicrogridEnv, DiscreteBatchedMicrogridEnv, MicrogridBatch
    from pymgrid_amd.priority_list import lists_array
    n_gen, n_bat, n_grid, n_load, n_pv, H, grid_first = mix
    rs = np.random.RandomState(77 + sum(mix))
    T, N, K = 40, 600, 24
    grids = [_random_multi_grid(rs, T, n_gen, n_bat, n_grid, n_load, n_pv, H, grid_first) for _ in range(N)]
    make = lambda: MicrogridBatch.from_grids(grids, device=device)
    ref, fused, sharded = BatchedMicrogridEnv(make(), log=True), BatchedMicrogridEnv(make()), BatchedMicrogridEnv(make())
    A = ref.layout.action_dim
    acts = torch.rand(K, N, A, dtype=torch.float64, device=device)
    out = fused.engine.step_k(acts, reward=True, done=True, soc_trace=True, status_trace=True, log=True)
    sharded.engine.set_shards(2)
    out2 = sharded.engine.step_k(acts, reward=True, log=True)
    sharded.engine.join(); sharded.engine.set_shards(1)
    for k in range(K):
        _, reward, done, info = ref.step(acts[k])
        assert torch.equal(out["reward"][k], reward) and torch.equal(out2["reward"][k], reward), k
        assert torch.equal(out["done"][k].view(torch.bool), done)
        assert torch.equal(out["log"][k], info["log"]) and torch.equal(out2["log"][k], info["log"]), k
        if n_bat:
            assert torch.equal(out["soc_trace"][k], ref.batch.cols["soc"].reshape(n_bat, N)[0])
        if n_gen:
            assert torch.equal(out["status_trace"][k], ref.batch.cols["gen_status"].reshape(n_gen, N)[0])
    for name in ("charge", "soc", "gen_status"):
        if name in ref.batch.cols:
            assert torch.equal(fused.batch.cols[name], ref.batch.cols[name]) and torch.equal(sharded.batch.cols[name], ref.batch.cols[name])
    assert fused.engine.current_step == ref.engine.current_step == K
    for e in (ref, fused, sharded):
        e.close()
    if 2 * n_gen + n_bat + n_grid > 9:                     # the reference's list enumeration is factorial
        return
    # discrete: an id per step and grid through mgx_rollout_lists == the env's expand + step
    denv, roll = DiscreteBatchedMicrogridEnv(make(), remove_redundant_gensets=False), DiscreteBatchedMicrogridEnv(make(), remove_redundant_gensets=False)
    lists = denv._lists if denv._instances else torch.as_tensor(
        lists_array([tuple((m, 0, a) for m, a in pl) for pl in denv.actions_list]), device=device)
    ids = torch.randint(0, denv.action_space.n, (K, N), dtype=torch.int32, device=device)
    res = roll.engine.rollout_lists(ids, lists, K, reward=True, done=True)
    for k in range(K):
        _, reward, done, _ = denv.step(ids[k])
        assert torch.equal(res["reward"][k], reward), k
    for name in ("charge", "soc", "gen_status"):
        if name in denv.batch.cols:
            assert torch.equal(roll.batch.cols[name], denv.batch.cols[name])
    denv.close(); roll.close()


@pytest.mark.gpu
def test_reward_shapers_on_several_batteries_and_renewables_vs_reference(device):
    """BatteryDischargeShaper / PVCurtailmentShaper sum over the module instances (reward_shaping/base.py:10-16; the battery sum
    falls back to 0 as soon as one battery charged): shaped rewards of 40 discrete steps == the reference's."""
    import torch
    from pymgrid_amd import DiscreteBatchedMicrogridEnv, MicrogridBatch
    from pymgrid_amd.trajectory import BatteryDischargeShaper, PVCurtailmentShaper
    n = 0
    for ci, p, mt, z in multi_cases():
        if f"c{ci}_shape_bat" not in z:
            continue
        for tag, shaper in (("bat", BatteryDischargeShaper()), ("pv", PVCurtailmentShaper())):
            env = DiscreteBatchedMicrogridEnv(MicrogridBatch.from_grids([p, p], device=device), reward_shaping_func=shaper)
            env.reset()
            ids = z[f"c{ci}_shape_{tag}_ids"]
            for k in range(len(ids)):
                _, reward, _, _ = env.step(torch.full((2,), int(ids[k]), dtype=torch.int32, device=device))
                assert reward[0].item() == z[f"c{ci}_shape_{tag}"][k] == reward[1].item(), (ci, tag, k)
            env.close()
            n += 1
    assert n >= 8


@pytest.mark.gpu
def test_priority_lists_with_foreign_elements_are_skipped_not_dereferenced(device):
    """mgx_expand_lists reads its lists from device memory, where the host cannot validate them: an element naming a module
    the layout does not have (instance out of range, unknown kind) is skipped like padding."""
    import torch
    from pymgrid_amd import DiscreteBatchedMicrogridEnv, MicrogridBatch
    rs = np.random.RandomState(3)
    grids = [_random_multi_grid(rs, 30, 2, 2, 0, 1, 1, 0, False) for _ in range(50)]
    env = DiscreteBatchedMicrogridEnv(MicrogridBatch.from_grids(grids, device=device), remove_redundant_gensets=False)
    env.reset()
    good = env._lists[:1].clone()                                   # [1, L, 3]
    junk = torch.tensor([[[0, 7, 1], [5, 0, 0], [2, 0, 0], [1, 9, 0]]], dtype=torch.int32, device=device)   # nothing valid
    ids = torch.zeros(50, dtype=torch.int32, device=device)
    both = torch.cat([junk[:, :good.shape[1]] if junk.shape[1] >= good.shape[1] else
                      torch.cat([junk, -torch.ones(1, good.shape[1] - junk.shape[1], 3, dtype=torch.int32, device=device)], dim=1), good])
    assert torch.equal(env.engine.expand_lists(ids + 1, both.contiguous()), env.engine.expand_lists(ids, good.contiguous()))
    assert bool((env.engine.expand_lists(ids, both.contiguous()) == 0).all())          # the junk list deploys nothing
    env.close()


@pytest.mark.gpu
def test_general_path_long_run_vs_oracle(device, oracle):
    """3 000 consecutive steps (fused launches of 500) of grids with 2 gensets + 3 batteries + 2 grids + 2 loads + 2 pvs: every
    reward and the final state of every module instance == the oracle's (state carried through the cache across launches)."""
    import torch
    from pymgrid_amd import BatchedMicrogridEnv, MicrogridBatch
    rs = np.random.RandomState(11)
    T, N = 3000, 6
    grids = [_random_multi_grid(rs, T + 1, 2, 3, 2, 2, 2, 0, False) for j in range(N)]
    env = BatchedMicrogridEnv(MicrogridBatch.from_grids(grids, device=device), observations=False)
    A = env.layout.action_dim
    acts = torch.rand(T, N, A, dtype=torch.float64, device=device)
    rewards = torch.cat([env.engine.step_k(acts[k:k + 500], reward=True)["reward"] for k in range(0, T, 500)]).cpu().numpy()
    a = acts.cpu().numpy()
    for j, g in enumerate(grids):
        om = oracle.OracleMultiMicrogrid(g)
        for k in range(T):
            assert rewards[k, j] == om.run(a[k, j], True).common.reward, (j, k)
        ch = env.batch.cols["charge"].reshape(3, N)[:, j].cpu().numpy()
        st = env.batch.cols["gen_status"].reshape(2, N)[:, j].cpu().numpy().view(np.uint32)
        assert [om.s.battery[q].charge for q in range(3)] == list(ch)
        for q in range(2):
            s = om.s.genset[q]
            assert _unpack(st[q]) == [s.gen_cur, s.gen_goal, s.gen_up, s.gen_down]
    env.close()
