"""GPU parity: the HIP engine (through the C ABI in include/mgx.h) against
  (a) golden vectors produced by the real reference (tests/golden/*.npz), and
  (b) the CPU oracle on seeded inputs,
bit-exact (==) on every fp64 output: reward, SoC / charge, genset status, log columns, observations, expanded
controls.  (BASELINE.json asks for 1e-6 relative; the engine keeps the reference's operation order and disables
FMA contraction, so equality is the bar here.)"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import action_dim, actions_for, golden

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------
def _buckets(grids):
    from pymgrid_amd.scenario import bucket_by_layout
    return list(bucket_by_layout(grids).values())


def _batch(grids, device):
    from pymgrid_amd import MicrogridBatch
    return MicrogridBatch.from_grids(grids, device=device)


def _status4(word_tensor):
    from pymgrid_amd import unpack_status
    return unpack_status(word_tensor.cpu().numpy().view(np.uint32))


def _t(a, device, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=device)


# ------------------------------------------------------------------------------------------------------
def test_pymgrid25_full_year_vs_reference(pymgrid25, device):
    """BASELINE config 2: all 25 pymgrid25 scenarios batched (one SoA batch per module set), 8759 steps with the
    goldens' seeded random actions, fused launches of 512 steps: per-step reward, SoC and genset status must equal
    what the REFERENCE produced, for every step of the year."""
    from pymgrid_amd import StepEngine
    z = golden("pymgrid25_run.npz")
    for idx in _buckets(pymgrid25):
        grids = [pymgrid25[n] for n in idx]
        batch = _batch(grids, device)
        eng = StepEngine(batch)
        K = grids[0]["final_step"] - grids[0]["initial_step"]
        A = action_dim(grids[0])
        acts = np.stack([np.random.RandomState(int(z[f"s{n}_seed"])).rand(K, A) for n in idx], axis=1)   # [K, Nb, A]
        reward, soc, status, done = [], [], [], []
        for k0 in range(0, K, 512):
            out = eng.step_k(_t(acts[k0:k0 + 512], device), normalized=True, reward=True, done=True, soc_trace=True,
                             status_trace=True)
            reward.append(out["reward"]); soc.append(out["soc_trace"]); done.append(out["done"])
            if "status_trace" in out:
                status.append(out["status_trace"])
        reward, soc, done = torch.cat(reward).cpu().numpy(), torch.cat(soc).cpu().numpy(), torch.cat(done).cpu().numpy()
        assert eng.current_step == grids[0]["final_step"]
        for j, n in enumerate(idx):
            assert np.array_equal(reward[:, j], z[f"s{n}_reward"]), f"scenario {n}: reward"
            assert np.array_equal(soc[:, j], z[f"s{n}_soc"]), f"scenario {n}: soc"
            assert done[:-1, j].sum() == 0 and done[-1, j] == 1
        if status:
            st = _status4(torch.cat(status))
            for j, n in enumerate(idx):
                assert np.array_equal(st[:, j], z[f"s{n}_status"].astype(np.int32)), f"scenario {n}: genset status"
        eng.close()


def test_pymgrid25_log_columns_vs_reference(pymgrid25, device):
    """Single-step path with the log enabled: first 128 steps of every scenario, every log column the reference
    writes (balance log + per-module energies/rewards + pre-step SoC) equals the golden row."""
    from pymgrid_amd import StepEngine
    z = golden("pymgrid25_run.npz")
    names = [str(s) for s in z["log_names"]]
    for idx in _buckets(pymgrid25):
        grids = [pymgrid25[n] for n in idx]
        eng = StepEngine(_batch(grids, device))
        A = action_dim(grids[0])
        K = grids[0]["final_step"] - grids[0]["initial_step"]
        acts = np.stack([np.random.RandomState(int(z[f"s{n}_seed"])).rand(K, A)[:128] for n in idx], axis=1)
        for k in range(128):
            _, reward, done, log = eng.step(_t(acts[k], device), normalized=True, want_obs=False, want_log=True)
            log = log.cpu().numpy()
            for j, n in enumerate(idx):
                assert int(z[f"s{n}_log_idx"][k]) == k
                row = z[f"s{n}_log_sub"][k]
                dev = dict(zip(eng.log_names, log[:, j]))
                if "genset_status" in dev:
                    w = int(dev.pop("genset_status"))
                    dev.update(gen_cur=w & 0xff, gen_goal=(w >> 8) & 0xff, gen_up=(w >> 16) & 0xff, gen_down=w >> 24)
                for c, name in enumerate(names):
                    if not np.isnan(row[c]):
                        assert dev[name] == row[c], f"scenario {n} step {k} column {name}: {dev[name]!r} vs {row[c]!r}"
        eng.close()


def test_generated_grids_vs_reference(device):
    """48 generator-style grids built as real reference modules (genset timers 0..3, weak grids, normalised and
    raw / out-of-range / exact-zero controls, H = 0 and 24): every log column, state and observation."""
    from pymgrid_amd import StepEngine
    z = golden("generated.npz")
    names = [str(s) for s in z["log_names"]]
    meta = json.loads(str(z["meta"]))
    grids = []
    for i, m in enumerate(meta):
        p = dict(m)
        for k in ("load_ts", "pv_ts", "grid_ts"):
            if f"g{i}_{k}" in z.files:
                p[k] = z[f"g{i}_{k}"]
        grids.append(p)
    keyed = {}
    for i, p in enumerate(grids):
        from pymgrid_amd.scenario import architecture
        keyed.setdefault((architecture(p), p["horizon"], p["normalized"]), []).append(i)
    for (arch, horizon, normalized), idx in keyed.items():
        eng = StepEngine(_batch([grids[i] for i in idx], device))
        obs0 = eng.reset().cpu().numpy()
        for j, i in enumerate(idx):
            assert np.array_equal(obs0[j], z[f"g{i}_obs0"]), f"grid {i}: reset obs"
        K = z[f"g{idx[0]}_actions"].shape[0]
        acts = np.stack([z[f"g{i}_actions"] for i in idx], axis=1)
        for k in range(K):
            obs, reward, done, log = eng.step(_t(acts[k], device), normalized=normalized, want_obs=True, want_log=True)
            log, obs = log.cpu().numpy(), obs.cpu().numpy()
            charge = eng.batch.cols["charge"].cpu().numpy()
            for j, i in enumerate(idx):
                row = z[f"g{i}_log"][k]
                dev = dict(zip(eng.log_names, log[:, j]))
                if "genset_status" in dev:
                    w = int(dev.pop("genset_status"))
                    dev.update(gen_cur=w & 0xff, gen_goal=(w >> 8) & 0xff, gen_up=(w >> 16) & 0xff, gen_down=w >> 24)
                for c, name in enumerate(names):
                    if not np.isnan(row[c]):
                        assert dev[name] == row[c], f"grid {i} step {k} {name}: {dev[name]!r} vs {row[c]!r}"
                assert charge[j] == z[f"g{i}_charge"][k]
                if f"g{i}_obs" in z.files and k % 5 == 0:
                    assert np.array_equal(obs[j], z[f"g{i}_obs"][k // 5]), f"grid {i} step {k}: obs"
        eng.close()


def test_discrete_env_vs_reference(pymgrid25, device):
    """G3: DiscreteBatchedMicrogridEnv -- the priority-list table, the expanded (unnormalised) controls and the
    rewards of 400 random action ids per scenario equal DiscreteMicrogridEnv's."""
    from pymgrid_amd import DiscreteBatchedMicrogridEnv
    from pymgrid_amd.priority_list import table_array
    z = golden("discrete.npz")
    for idx in _buckets(pymgrid25):
        grids = [pymgrid25[n] for n in idx]
        env = DiscreteBatchedMicrogridEnv(_batch(grids, device), log=False, observations=True)
        for n in idx:
            assert np.array_equal(table_array(env.actions_list), z[f"s{n}_table"][:, :3])
            assert env.action_space.n == z[f"s{n}_table"].shape[0]
        ids = np.stack([z[f"s{n}_ids"] for n in idx], axis=1)          # [400, Nb]
        for k in range(ids.shape[0]):
            a = _t(ids[k], device, torch.int32)
            control = env.get_action(a).cpu().numpy()
            obs, reward, done, _ = env.step(a)
            reward = reward.cpu().numpy()
            soc = env.batch.cols["soc"].cpu().numpy()
            for j, n in enumerate(idx):
                assert np.array_equal(control[j], z[f"s{n}_control"][k]), f"scenario {n} step {k}: control"
                assert reward[j] == z[f"s{n}_reward"][k], f"scenario {n} step {k}: reward"
                assert soc[j] == z[f"s{n}_soc"][k]
        env.close()


def test_observations_vs_reference(pymgrid25, device):
    """reset + 40 post-step observations (H = 23; 4-component grid windows) and the end-of-series padding."""
    from pymgrid_amd import StepEngine
    z = golden("obs.npz")
    for idx in _buckets(pymgrid25):
        grids = [pymgrid25[n] for n in idx]
        eng = StepEngine(_batch(grids, device))
        obs0 = eng.reset().cpu().numpy()
        A = action_dim(grids[0])
        acts = np.stack([np.random.RandomState(3100 + n).rand(40, A) for n in idx], axis=1)
        for j, n in enumerate(idx):
            assert np.array_equal(obs0[j], z[f"head{n}_obs0"])
        for k in range(40):
            obs = eng.step(_t(acts[k], device))[0].cpu().numpy()
            for j, n in enumerate(idx):
                assert np.array_equal(obs[j], z[f"head{n}_obs"][k]), (n, k)
        eng.close()
    for n in (1, 0, 2):                                               # G5: run into the end of the series
        p = dict(pymgrid25[n]); p["initial_step"] = int(z[f"tail{n}_start"])
        eng = StepEngine(_batch([p], device))
        assert np.array_equal(eng.reset().cpu().numpy()[0], z[f"tail{n}_obs0"])
        K = p["final_step"] - p["initial_step"]
        acts = np.random.RandomState(3000 + n).rand(K, action_dim(p))
        for k in range(K):
            obs, reward, done, _ = eng.step(_t(acts[k:k + 1], device))
            assert reward.item() == z[f"tail{n}_reward"][k] and int(done.item()) == z[f"tail{n}_done"][k]
            assert np.array_equal(obs.cpu().numpy()[0], z[f"tail{n}_obs"][k]), k
        obs = eng.step(_t(np.full((1, action_dim(p)), 0.5), device))[0]
        assert np.array_equal(obs.cpu().numpy()[0], z[f"tail{n}_obs_extra"][0])
        from pymgrid_amd import MgxError
        with pytest.raises(MgxError) as e:                            # IndexError in the reference
            eng.step(_t(np.full((1, action_dim(p)), 0.5), device))
        assert e.value.code == 3
        eng.close()


def test_reset_keeps_dynamic_state(pymgrid25, device):
    from pymgrid_amd import StepEngine
    z = golden("obs.npz")
    p = pymgrid25[1]
    eng = StepEngine(_batch([p], device))
    acts = np.random.RandomState(3200).rand(30, action_dim(p))
    r1 = [eng.step(_t(acts[k:k + 1], device))[1].item() for k in range(15)]
    obs = eng.reset().cpu().numpy()[0]
    assert eng.current_step == 0
    assert np.array_equal(obs, z["reset_obs"])
    c = eng.batch.cols
    st = _status4(c["gen_status"])[0]
    assert np.array_equal(np.array([c["charge"].item(), c["soc"].item(), *st]), z["reset_state"])
    r2, soc2 = [], []
    for k in range(15, 30):
        r2.append(eng.step(_t(acts[k:k + 1], device))[1].item()); soc2.append(c["soc"].item())
    assert np.array_equal(r1, z["reset_reward1"]) and np.array_equal(r2, z["reset_reward2"])
    assert np.array_equal(soc2, z["reset_soc2"])
    eng.close()


# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["genset+battery", "battery+grid", "genset+battery+grid", "loadpv"])
def test_fused_equals_single_step_equals_oracle(arch, device, oracle):
    """Seeded generated batch: K fused steps == K single steps == CPU oracle, bit for bit (state + rewards)."""
    from pymgrid_amd import StepEngine
    from pymgrid_amd.generator import generate
    N, T, K = 5000, 80, 67            # ragged: N not a multiple of 256, K not a multiple of the pipeline depth
    gen = torch.Generator(device=device); gen.manual_seed(5)
    b1 = generate(N, n_steps=T, seed=9, arch=arch, device=device, mixed_timers=True)
    b2 = generate(N, n_steps=T, seed=9, arch=arch, device=device, mixed_timers=True)
    A = b1.layout.action_dim
    acts = torch.rand(K, N, A, dtype=torch.float64, device=device, generator=gen)
    acts[::7] = acts[::7].round()      # exact 0 / 1 controls: x == 0 routing, goal exactly 0/1
    cols = b1.numpy_columns()
    st = {k: cols[k].copy() for k in ("charge", "soc", "gen_status") if k in cols}
    e1, e2 = StepEngine(b1), StepEngine(b2)
    fused = e1.step_k(acts, reward=True, done=True, soc_trace=True, status_trace=True, log=True)
    single_r, single_log = [], []
    for k in range(K):
        _, r, d, lg = e2.step(acts[k], want_obs=False, want_log=True)
        single_r.append(r.clone()); single_log.append(lg.clone())
    single_r, single_log = torch.stack(single_r), torch.stack(single_log)
    assert torch.equal(fused["reward"], single_r)
    assert torch.equal(fused["log"], single_log)
    for k in ("charge", "soc", "gen_status"):
        if k in b1.cols:
            assert torch.equal(b1.cols[k], b2.cols[k])
    ref = oracle.run_batch(cols, st, 0, K, acts.cpu().numpy(), normalized=True, nthreads=8)
    assert np.array_equal(fused["reward"].cpu().numpy(), ref)
    for k in st:
        got = b1.cols[k].cpu().numpy()
        assert np.array_equal(got.view(np.uint32) if k == "gen_status" else got, st[k]), k
    if "soc_trace" in fused:
        assert torch.equal(fused["soc_trace"][-1], b1.cols["soc"])
    e1.close(); e2.close()


def test_full_size_batch_properties(device, oracle):
    """BASELINE config 3 size (N = 100 000 Template-4 grids): oracle equality on a fused chunk, energy balance,
    reward decomposition, metrics reduction."""
    from pymgrid_amd import StepEngine
    from pymgrid_amd.generator import generate
    N, T, K = 100_000, 72, 64
    b = generate(N, n_steps=T, seed=42, arch="genset+battery", device=device)
    cols = b.numpy_columns()
    st = {k: cols[k].copy() for k in ("charge", "soc", "gen_status")}
    eng = StepEngine(b)
    gen = torch.Generator(device=device); gen.manual_seed(7)
    acts = torch.rand(K, N, 3, dtype=torch.float64, device=device, generator=gen)
    ret = torch.zeros(N, dtype=torch.float64, device=device)
    out = eng.step_k(acts, reward=True, ret_acc=ret, log=True)
    ref = oracle.run_batch(cols, st, 0, K, acts.cpu().numpy(), normalized=True, nthreads=8)
    assert np.array_equal(out["reward"].cpu().numpy(), ref)
    assert np.array_equal(b.cols["charge"].cpu().numpy(), st["charge"])
    log = out["log"]
    ix = {n: j for j, n in enumerate(eng.log_names)}
    prov, absb = log[:, ix["overall_provided"]], log[:, ix["overall_absorbed"]]
    assert torch.allclose(prov, absb, rtol=1e-9, atol=1e-9)                  # microgrid.py:321-323
    total = log[:, ix["genset_reward"]] + log[:, ix["battery_reward"]] + log[:, ix["unbalanced_reward"]]
    assert torch.allclose(total, out["reward"], rtol=1e-12, atol=1e-9)
    assert torch.allclose(ret, out["reward"].sum(0), rtol=1e-12, atol=1e-6)
    soc = b.cols["soc"]
    assert (soc >= 0.2 - 1e-12).all() and (soc <= 1 + 1e-9).all()
    sums = eng.metrics(log[-1])
    assert torch.equal(sums, eng.metrics(log[-1]))                           # deterministic
    assert torch.allclose(sums, log[-1].sum(1), rtol=1e-11, atol=1e-5)
    eng.close()


def test_gym_adaptors_shapes(pymgrid25, device):
    """Reference tests/envs/test_discrete.py:12-95: flat obs shape, nested obs keys, action_space.n, float / bool
    return types, 10 random steps, reset."""
    from pymgrid_amd import DiscreteMicrogridEnv, MicrogridEnv
    for n in (0, 1, 2):
        p = pymgrid25[n]
        env = DiscreteMicrogridEnv(p, device=device)
        n_ctrl = (p.get("genset") is not None) + (p.get("battery") is not None) + (p.get("grid") is not None)
        n_expected = {1: 1, 2: 2 if p.get("genset") is None else 4, 3: 12}[n_ctrl]
        assert env.action_space.n == n_expected          # n_modules! * 2^n_gensets (test_discrete.py:73-80)
        obs = env.reset()
        assert obs.shape == env.observation_space.shape == (env.layout.obs_dim,)
        for _ in range(10):
            a = env.action_space.sample()
            ctrl = env.get_action_dict(a)
            assert set(ctrl) == {k for k in ("genset", "battery", "grid") if p.get(k) is not None}
            obs, reward, done, info = env.step(a)
            assert obs.shape == (env.layout.obs_dim,) and isinstance(reward, float) and isinstance(done, bool)
            assert env.last_log["reward"] == reward and set(info) == set(env._nested(obs)) and "provided_energy" in info["pv"][0]
        assert len(env.get_log_columns()["reward"]) == 10
        df = env.get_log()                                # Microgrid.get_log(as_frame=True) shape, indexed by step
        assert len(df) == 10 and df.columns.nlevels == 3 and list(df.index) == list(range(env.current_step - 10, env.current_step))
        assert np.array_equal(df[("balance", 0, "reward")].values, env.get_log_columns()["reward"][:, 0])
        assert ("battery", 0, "soc") in df.columns and ("unbalanced_energy", 0, "loss_load") in df.columns
        assert env.get_log(as_frame=False)[("balance", 0, "reward")][env.current_step - 1] == df[("balance", 0, "reward")].iloc[-1]
        env.reset(); assert env.current_step == 0 and len(env.get_log()) == 0 and env.get_log_columns() == {}
        with pytest.raises(ValueError):
            env.step(env.action_space.n)
        env.close()
        env = MicrogridEnv(p, device=device, flat_spaces=False)
        obs = env.reset()
        assert set(obs) == set(env.layout.obs_slices()) | {"unbalanced_energy"} and obs["unbalanced_energy"][0].shape == (0,)
        ctrl = {"battery": [0.5]}
        if p.get("genset") is not None: ctrl["genset"] = [np.array([1.0, 0.5])]
        if p.get("grid") is not None: ctrl["grid"] = [0.5]
        obs, reward, done, info = env.step(ctrl, normalized=True)
        assert isinstance(reward, float) and len(obs["load"][0]) == 24
        # Env.from_microgrid (envs/base/base.py:253-283): wrap a stepped microgrid -- parameters AND current state carry over
        # from_scenario(n) without a path: the packaged copy of the benchmark microgrids == the fixture
        packaged = DiscreteMicrogridEnv.from_scenario(n, device=device)
        assert packaged.action_space.n == n_expected and packaged.layout == env.layout
        for name in ("load_ts", "bat_max_capacity", "gen_running_max"):
            if name in env.batch.cols:
                assert torch.equal(packaged.batch.cols[name], env.batch.cols[name]), name
        packaged.close()
        # Microgrid.sample_action / get_empty_action / run (microgrid.py:227-381) on the continuous adaptor
        from pymgrid_amd import Microgrid
        mg = Microgrid(pymgrid25[n], device=device)
        ctrl = mg.sample_action()
        assert set(ctrl) == set(mg.get_empty_action()) == {k for k in ("genset", "battery", "grid") if pymgrid25[n].get(k) is not None}
        o2, r2, d2, i2 = mg.run(ctrl, normalized=True)
        assert isinstance(r2, float) and isinstance(d2, bool)
        # (run returns MicrogridStep's NESTED observation whatever flat_spaces says: microgrid.py:325; the flattening is env.step's)
        assert isinstance(o2, dict) and sum(len(a) for v in o2.values() for a in v) == mg.layout.obs_dim
        mg.close()
        twin = DiscreteMicrogridEnv.from_microgrid(env)
        for name in ("charge", "soc", "gen_status"):
            if name in env.batch.cols:
                assert torch.equal(twin.batch.cols[name], env.batch.cols[name]), name
        assert twin.action_space.n == n_expected and twin.current_step == 0
        twin.close(); env.close()


def test_error_paths(pymgrid25, device):
    from pymgrid_amd import BatchLayout, MgxError, MicrogridBatch, StepEngine
    p = pymgrid25[2]
    b = _batch([p], device)
    eng = StepEngine(b)
    with pytest.raises(ValueError):
        eng.step(torch.zeros(1, 2, dtype=torch.float64, device=device))          # wrong action width
    with pytest.raises(ValueError):
        eng.step(torch.zeros(1, 3, dtype=torch.float32, device=device))          # wrong dtype
    with pytest.raises(MgxError) as e:
        eng.step_k(torch.zeros(9000, 1, 3, dtype=torch.float64, device=device))  # leaves the series
    assert e.value.code == 3 and eng.current_step == 0
    with pytest.raises(MgxError):
        eng.reset(initial_step=8759)
    eng.close()
    z = golden("loadpv.npz")                                                       # 2 loads + 1 pv: general kernels
    multi = dict(load_ts=z["c1_load_ts"], pv_ts=z["c1_pv_ts"], final_step=100, horizon=0,
                 unbalanced=dict(loss_load_cost=10.0, overgeneration_cost=2.0))
    eng = StepEngine(_batch([multi], device))
    out = eng.step_k(torch.zeros(4, 1, 0, dtype=torch.float64, device=device))     # K-step loop of the general path
    assert out["reward"].shape == (4, 1) and eng.current_step == 4
    ring = eng.observe_windows(K=4)                                                # window prefetch of the general path (no state
    for k in range(4):                                                             # columns in this layout: block k IS the row of step t + k)
        assert torch.equal(ring[k], eng.observe())
        eng.step_k(torch.zeros(1, 1, 0, dtype=torch.float64, device=device))
    eng.close()
    with pytest.raises(ValueError):
        MicrogridBatch(BatchLayout(n_grids=1, n_steps=8760, has_genset=True, has_battery=True, n_load=2), b.cols)
    with pytest.raises(MgxError):
        StepEngine(_batch([p], "cpu"))                                           # no CPU path


@pytest.mark.parametrize("streams,prefetch", [(False, 0), (True, 0), (False, 8)])
def test_bucketed_fleet_of_mixed_layouts(streams, prefetch, pymgrid25, device):
    """BASELINE config 5 shape: the 25 scenarios (3 module sets) as ONE fleet; per-grid rewards / SoC of 200 steps
    equal the per-scenario goldens; buckets back to back, on separate streams, and with window prefetch."""
    from pymgrid_amd.hetero import BucketedFleet
    z = golden("pymgrid25_run.npz")
    fleet = BucketedFleet(pymgrid25, device=device, observations=True, streams=streams, obs_prefetch=prefetch)
    assert len(fleet.envs) == 3 and len(fleet) == 25
    obs = fleet.reset()
    assert [o.shape[1] for o in obs] == [env.layout.obs_dim for env in fleet.envs]
    K = 200
    acts = {n: np.random.RandomState(int(z[f"s{n}_seed"])).rand(8759, action_dim(p))[:K] for n, p in enumerate(pymgrid25)}
    for k in range(K):
        a = [_t(np.stack([acts[n][k] for n in idx]), device) for _, idx in fleet.buckets]
        obs, reward, done, _ = fleet.step(a)
        r = fleet.scatter(reward).cpu().numpy()
        soc = fleet.scatter([env.batch.cols["soc"] for env in fleet.envs]).cpu().numpy()
        for n in range(25):
            assert r[n] == z[f"s{n}_reward"][k] and soc[n] == z[f"s{n}_soc"][k], (n, k)
    fleet.close()


@pytest.mark.parametrize("arch", ["genset+battery", "genset+battery+grid"])
def test_randomized_differential_degenerate_parameters(arch, device, oracle):
    """Differential test over wild / degenerate parameters (zero-width action spaces, eta = 1, zero capacities and
    costs, min == max production, huge and tiny magnitudes, raw controls far outside the limits): 20 000 grids x 48
    steps, device == oracle bit for bit."""
    from pymgrid_amd import BatchLayout, MicrogridBatch, StepEngine, pack_status
    from pymgrid_amd.batch import pack_times
    rs = np.random.RandomState(int(os.environ.get("MGX_FUZZ_SEED", "99")))     # (soak runs: for s in ...; MGX_FUZZ_SEED=$s pytest -k degenerate)
    N, T, K = 20_000, 50, 48
    has_grid = "grid" in arch

    def pick(*choices):
        return rs.choice(np.array(choices, dtype=np.float64), size=N)
    scale = 10.0 ** rs.randint(-2, 7, size=N)
    cap = scale * pick(0.0, 1.0, 3.0, 100.0)
    cmin = cap * pick(0.0, 0.2, 0.5, 1.0)
    A = dict(
        load_ts=-np.abs(scale * rs.rand(T, N) * (rs.rand(T, N) > 0.1)),
        pv_ts=np.abs(scale * rs.rand(T, N) * (rs.rand(T, N) > 0.4)),
        loss_load_cost=pick(0.0, 10.0, 1e3), overgeneration_cost=pick(0.0, 1.0, 2.5),
        bat_min_capacity=cmin, bat_max_capacity=np.maximum(cap, 1e-300),
        bat_max_charge=cap * pick(0.0, 0.25, 1.0, 5.0), bat_max_discharge=cap * pick(0.0, 0.25, 1.0, 5.0),
        bat_efficiency=pick(1.0, 0.9, 0.5, 0.123), bat_cost_cycle=pick(0.0, 0.02, 7.0),
        gen_running_max=scale * pick(0.0, 1.0, 2.0),
        gen_cost=pick(0.0, 0.4, 3.0), gen_co2_per_unit=pick(0.0, 2.0), gen_cost_per_unit_co2=pick(0.0, 0.1),
    )
    A["gen_running_min"] = A["gen_running_max"] * pick(0.0, 0.05, 1.0)
    su, wd = rs.randint(0, 5, N), rs.randint(0, 5, N)
    on = rs.randint(0, 2, N)
    A["gen_times"] = pack_times(su, wd)
    A["gen_status"] = pack_status(on, on, np.where(on, 0, su), np.where(on, wd, 0))
    soc0 = np.clip(rs.rand(N), A["bat_min_capacity"] / A["bat_max_capacity"], 1.0)
    A["charge"] = np.maximum(soc0 * A["bat_max_capacity"], A["bat_min_capacity"])
    A["soc"] = A["charge"] / A["bat_max_capacity"]
    if has_grid:
        A["grid_max_import"] = scale * pick(0.0, 1.0, 4.0)
        A["grid_max_export"] = scale * pick(0.0, 1.0, 4.0)
        A["grid_cost_per_unit_co2"] = pick(0.0, 0.1)
        g = np.stack([rs.rand(T, N), rs.rand(T, N) * (rs.rand(T, N) > 0.5), rs.rand(T, N),
                      (rs.rand(T, N) > 0.2).astype(np.float64)], axis=1)
        A["grid_ts"] = g
    layout = BatchLayout(n_grids=N, n_steps=T, has_genset=True, has_battery=True, has_grid=has_grid)
    batch = MicrogridBatch.from_numpy(layout, A, device)
    cols = batch.numpy_columns()
    st = {k: cols[k].copy() for k in ("charge", "soc", "gen_status")}
    eng = StepEngine(batch)
    failed = np.zeros(N, dtype=np.uint8)        # grids on which the REFERENCE would raise (e.g. charge above
    for normalized in (True, False):            # max_capacity by a rounding when max_charge >= capacity / 2)
        a = rs.rand(K // 2, N, layout.action_dim)
        if not normalized:                                  # raw requests, up to 3x beyond any limit, both signs
            a[..., 1] = a[..., 1] * 3 * A["gen_running_max"]
            a[..., 2] = (a[..., 2] * 2 - 1) * 3 * np.maximum(A["bat_max_charge"], A["bat_max_discharge"])
            if has_grid:
                a[..., 3] = (a[..., 3] * 2 - 1) * 3 * np.maximum(A["grid_max_import"], A["grid_max_export"])
        a[::5] = np.round(a[::5])
        t0 = eng.current_step
        out = eng.step_k(_t(a, device), normalized=normalized, reward=True, soc_trace=True)
        ref = oracle.run_batch(cols, st, t0, K // 2, a, normalized=normalized, nthreads=8, failed=failed)
        ok = failed == 0
        got = out["reward"].cpu().numpy()
        assert np.array_equal(got[:, ok], ref[:, ok]), f"normalized={normalized}: {np.sum(got[:, ok] != ref[:, ok])} differ"
        for k in st:
            dev = batch.cols[k].cpu().numpy()
            dev = dev.view(np.uint32) if k == "gen_status" else dev
            assert np.array_equal(dev[ok], st[k][ok]), k
    assert failed.mean() < 0.02, failed.mean()
    eng.close()


def test_observation_keys_vs_reference(pymgrid25, device):
    """BaseMicrogridEnv(observation_keys=...) (reference tests/envs/test_discrete.py:82-95): the observation is the
    listed state keys in list order; unknown keys raise NameError."""
    from pymgrid_amd import DiscreteMicrogridEnv
    z = golden("obskeys.npz")
    for n in (1, 0, 2):
        keys = [str(k) for k in z[f"s{n}_keys"]]
        env = DiscreteMicrogridEnv(pymgrid25[n], device=device, observation_keys=keys)
        assert env.observation_space.shape == (len(keys),)
        assert np.array_equal(env.reset(), z[f"s{n}_obs0"])
        for k, a in enumerate(z[f"s{n}_ids"]):
            obs, _, _, _ = env.step(int(a))
            assert np.array_equal(obs, z[f"s{n}_obs"][k]), (n, k)
        env.close()
    with pytest.raises(NameError):
        DiscreteMicrogridEnv(pymgrid25[0], device=device, observation_keys=["current_status"])


@pytest.mark.parametrize("H", [1, 7, 8, 9, 26, 27, 28, 30, 31, 32, 33, 40, 55, 56, 63, 64, 70])
def test_observation_window_chunk_boundaries(H, device, oracle):
    """Forecast horizons around the window-round size (28 slots per round: 7 per lane x 4 horizon phases), ragged N
    (65 grids: a partly filled 16-grid tile), starts inside the series (fast path: SGPR-base
    loads) and steps that run into the end-of-series padding (general path): device observation == oracle."""
    from pymgrid_amd import StepEngine
    rs = np.random.RandomState(H)
    T, N = 90, 130
    grids = []
    for i in range(N):
        g = dict(load_ts=50 * rs.rand(T), pv_ts=40 * rs.rand(T) * (rs.rand(T) > 0.3), horizon=H, final_step=T,
                 initial_step=0, unbalanced=dict(loss_load_cost=10.0, overgeneration_cost=2.0),
                 battery=dict(min_capacity=20.0, max_capacity=100.0, max_charge=25.0, max_discharge=25.0,
                              efficiency=0.9, battery_cost_cycle=0.02, init_soc=0.5),
                 grid=dict(max_import=60.0, max_export=30.0, cost_per_unit_co2=0.1),
                 grid_ts=np.stack([0.1 + rs.rand(T), 0.5 * rs.rand(T), 0.3 * rs.rand(T),
                                   (rs.rand(T) > 0.2).astype(float)], axis=1))
        if i % 2:
            g["genset"] = None
        grids.append(g)
    for sub in ([g for g in grids if g.get("genset", 1) is None],):
        for g in sub:
            g.pop("genset")
        eng = StepEngine(_batch(sub, device))
        oms = [oracle.OracleMicrogrid(g) for g in sub[:12]]
        for start in (0, T - H - 3 if T - H - 3 > 0 else 0, T - 4):
            obs = eng.reset(initial_step=start).cpu().numpy()
            for j, om in enumerate(oms):
                assert np.array_equal(obs[j], om.reset(initial_step=start)), (H, start, j)
            a = rs.rand(len(sub), 2)
            for k in range(3):
                obs = eng.step(_t(a, device))[0].cpu().numpy()
                for j, om in enumerate(oms):
                    om.run(dict(battery=a[j, 0], grid=a[j, 1]), True)
                    assert np.array_equal(obs[j], om.observe()), (H, start, k, j)
        eng.close()


def test_small_and_ragged_shapes(device, oracle):
    """N around the wave / workgroup / balanced-workgroup sizes and K around the ring depth: fused steps, discrete
    rollout and single steps == oracle (empty tails, partially filled waves, K < ring depth)."""
    from pymgrid_amd import DiscreteBatchedMicrogridEnv
    from pymgrid_amd.generator import generate
    rs = np.random.RandomState(0)
    for N in (1, 2, 63, 64, 65, 207, 208, 209, 255, 256, 257, 1000):
        for K in (1, 2, 3, 4, 5, 9):
            env = DiscreteBatchedMicrogridEnv(generate(N, n_steps=K + 12, seed=N, device=device, mixed_timers=True),
                                              observations=False, remove_redundant_gensets=False)
            cols = env.batch.numpy_columns()
            st = {k: cols[k].copy() for k in ("charge", "soc", "gen_status")}
            a = rs.rand(K, N, 3)
            out = env.engine.step_k(_t(a, device), reward=True)
            ref = oracle.run_batch(cols, st, 0, K, a)
            assert np.array_equal(out["reward"].cpu().numpy(), ref), (N, K)
            ids = rs.randint(0, env.action_space.n, size=(K, N)).astype(np.uint8)
            t0 = env.engine.current_step
            out = env.engine.rollout_discrete(_t(ids, device, torch.uint8), env._table, K)
            ref = oracle.rollout_batch(cols, st, t0, K, ids, env._table)
            assert np.array_equal(out["reward"].cpu().numpy(), ref), (N, K)
            _, r, _, _ = env.step(_t(ids[0], device, torch.int32))
            ref = oracle.rollout_batch(cols, st, t0 + K, 1, ids[:1], env._table)
            assert np.array_equal(r.cpu().numpy(), ref[0]), (N, K)
            assert np.array_equal(env.batch.cols["charge"].cpu().numpy(), st["charge"])
            env.close()


def test_observation_extreme_magnitudes_and_unaligned_output(device, oracle):
    """Normalisation (v - lo) / spread at extreme magnitudes: series scaled by 2^k for k from deep in the subnormal
    range to near overflow, constant columns (spread 0 -> 1), and an output buffer that is only 8-byte aligned (scalar
    store path of the row writer): device observation == oracle, bit for bit."""
    from pymgrid_amd import StepEngine
    rs = np.random.RandomState(11)
    T, H = 64, 24
    grids = []
    for k in (-1060, -1030, -1022, -600, -523, -500, -499, -250, -52, -1, 0, 1, 53, 250, 499, 500, 523, 600, 900):
        for rep in range(3):
            scale = np.ldexp(1.0, k)
            load = (1.0 + rs.rand(T)) * scale * (50 if rep else 1)
            pv = rs.rand(T) * scale * (rs.rand(T) > 0.3)
            if rep == 2:
                pv = np.full(T, 3.0 * scale)                      # constant column: spread 0 -> 1
            grids.append(dict(load_ts=load, pv_ts=pv, horizon=H, final_step=T, initial_step=0,
                              unbalanced=dict(loss_load_cost=10.0, overgeneration_cost=2.0),
                              battery=dict(min_capacity=20.0, max_capacity=100.0, max_charge=25.0, max_discharge=25.0,
                                           efficiency=0.9, battery_cost_cycle=0.02, init_soc=0.5),
                              grid=dict(max_import=60.0, max_export=30.0, cost_per_unit_co2=0.1),
                              grid_ts=np.stack([(0.1 + rs.rand(T)) * np.ldexp(1.0, k // 2), 0.5 * rs.rand(T),
                                                rs.rand(T) * np.ldexp(1.0, -k // 3), (rs.rand(T) > 0.2).astype(float)], axis=1)))
    eng = StepEngine(_batch(grids, device))
    N, D = len(grids), eng.layout.obs_dim
    oms = [oracle.OracleMicrogrid(g) for g in grids]
    flat = torch.empty(N * D + 1, dtype=torch.float64, device=device)
    for out in (None, flat[1:].view(N, D)):
        for start in (0, 5, T - H - 5, T - 3):
            eng.reset(initial_step=start, want_obs=False)
            obs = eng.observe(out=out).cpu().numpy()
            for j, om in enumerate(oms):
                assert np.array_equal(obs[j], om.reset(initial_step=start)), (start, j)
    eng.close()


@pytest.mark.parametrize("arch,H,noise", [("genset+battery", 0, False), ("genset+battery+grid", 0, False),
                                          ("genset+battery", 24, False), ("genset+battery+grid", 24, True),
                                          ("battery+grid", 30, False), ("loadpv", 5, False)])
def test_float32_observations_are_the_rounded_float64_rows(arch, H, noise, device):
    """obs_dtype=float32 (mgx_set_obs_format): every observation entry point returns exactly the float64 row rounded
    to nearest float -- reset, observe, step, discrete step, through the inline (H = 0), window (H > 0, incl. forecast
    noise, end-of-series padding) and general multi-module kernels; ragged N, unaligned output buffer."""
    from pymgrid_amd import BatchedMicrogridEnv, DiscreteBatchedMicrogridEnv, StepEngine
    from pymgrid_amd.generator import generate
    N, T = 1003, 80

    def make():
        if arch == "loadpv":
            rs = np.random.RandomState(3)
            grids = [dict(load_ts=rs.rand(T, 2) * [20, 5], pv_ts=rs.rand(T, 3) * [10, 4, 1],
                          horizon=H, final_step=T, initial_step=0, unbalanced=dict(loss_load_cost=10.0, overgeneration_cost=2.0),
                          battery=dict(min_capacity=20.0, max_capacity=100.0, max_charge=25.0, max_discharge=25.0,
                                       efficiency=0.9, battery_cost_cycle=0.02, init_soc=0.5)) for _ in range(37)]
            return _batch(grids, device)
        b = generate(N, n_steps=T, seed=5, arch=arch, horizon=H, device=device)
        if noise:
            b.cols["load_noise_std"] = torch.full((N,), 3.0, dtype=torch.float64, device=device)
            b.cols["grid_noise_std"] = torch.full((N,), 0.05, dtype=torch.float64, device=device)
            b.forecast_noise = dict(seed=9, increase_uncertainty=True)
        return b
    e64, e32 = StepEngine(make()), StepEngine(make(), obs_dtype=torch.float32)
    n, D = e64.N, e64.obs_dim
    rs = np.random.RandomState(1)
    flat = torch.empty(n * D + 1, dtype=torch.float32, device=device)
    for start in (0, 3, T - 6):
        o64, o32 = e64.reset(initial_step=start), e32.reset(initial_step=start)
        assert o32.dtype == torch.float32 and torch.equal(o32, o64.to(torch.float32)), (start, "reset")
        assert torch.equal(e32.observe(out=flat[1:].view(n, D)), e64.observe().to(torch.float32)), (start, "observe")
        for k in range(4):
            a = _t(rs.rand(n, e64.action_dim), device)
            r64, r32 = e64.step(a), e32.step(a)
            assert torch.equal(r32[0], r64[0].to(torch.float32)), (start, k)
            assert torch.equal(r32[1], r64[1])                      # rewards stay float64
    with pytest.raises(ValueError):
        e32.observe(out=torch.empty(n, D, dtype=torch.float64, device=device))
    e64.close(); e32.close()
    if arch != "loadpv":
        d64 = DiscreteBatchedMicrogridEnv(make())
        d32 = DiscreteBatchedMicrogridEnv(make(), obs_dtype=torch.float32)
        assert torch.equal(d32.reset(), d64.reset().to(torch.float32))
        for k in range(3):
            ids = torch.from_numpy(rs.randint(0, d64.action_space.n, size=n).astype(np.int32)).to(device)
            assert torch.equal(d32.step(ids)[0], d64.step(ids)[0].to(torch.float32)), k
        d64.close(); d32.close()
        c32 = BatchedMicrogridEnv(make(), obs_dtype=torch.float32)
        assert c32.reset().dtype == torch.float32
        c32.close()


@pytest.mark.parametrize("arch,H,K,dtype", [("genset+battery", 24, 8, torch.float64), ("genset+battery+grid", 24, 8, torch.float64),
                                            ("genset+battery+grid", 23, 3, torch.float32), ("battery+grid", 5, 2, torch.float64),
                                            ("genset+battery+grid", 40, 30, torch.float64), ("genset+battery", 1, 64, torch.float32)])
def test_window_prefetch_equals_per_step_observations(arch, H, K, dtype, device):
    """obs_prefetch=K (mgx_observe_windows + state-only rows): the observation returned by every reset / step is
    identical to the per-step kernel's, across ring refills, into the end-of-series padding, ragged N, float32 rows;
    ring blocks ahead of the current step hold the right windows and zero state columns."""
    from pymgrid_amd import BatchedMicrogridEnv, DiscreteBatchedMicrogridEnv, StepEngine
    from pymgrid_amd.generator import generate
    N, T = 1003, 150
    rs = np.random.RandomState(K)

    def make():
        return generate(N, n_steps=T, seed=5, arch=arch, horizon=H, device=device, mixed_timers=True)
    ref, pre = BatchedMicrogridEnv(make(), obs_dtype=dtype), BatchedMicrogridEnv(make(), obs_dtype=dtype, obs_prefetch=K)
    assert pre.obs_prefetch == K
    for start, n_steps in ((0, 2 * K + 3), (T - H - 7, H + 6)):
        o_ref, o_pre = ref.reset(start), pre.reset(start)
        assert torch.equal(o_ref, o_pre), (start, "reset")
        for k in range(min(n_steps, T - start - 1)):
            a = _t(rs.rand(N, ref.layout.action_dim), device)
            s_ref, s_pre = ref.step(a), pre.step(a)
            assert torch.equal(s_ref[0], s_pre[0]), (start, k)
            assert torch.equal(s_ref[1], s_pre[1]) and torch.equal(s_ref[2], s_pre[2])
    ref.close(); pre.close()
    # the ring itself: block k = observation of step t + k, state columns zero for k > 0
    e = StepEngine(make(), obs_dtype=dtype)
    W, D = 1 + H, e.obs_dim
    n_state = 4 * e.layout.has_genset + 2 * e.layout.has_battery
    e.reset(initial_step=7, want_obs=False)
    ring = e.observe_windows(K)
    for k in range(K):
        if 7 + k >= T:
            break
        e.reset(initial_step=7 + k, want_obs=False)
        row = e.observe()
        if k:
            row[:, 2 * W:2 * W + n_state] = 0
        assert torch.equal(ring[k], row), k
    e.close()
    d_ref = DiscreteBatchedMicrogridEnv(make(), obs_dtype=dtype)
    d_pre = DiscreteBatchedMicrogridEnv(make(), obs_dtype=dtype, obs_prefetch=K)
    assert torch.equal(d_ref.reset(), d_pre.reset())
    for k in range(K + 2):
        ids = torch.from_numpy(rs.randint(0, d_ref.action_space.n, size=N).astype(np.int32)).to(device)
        assert torch.equal(d_ref.step(ids)[0], d_pre.step(ids)[0]), k
    d_ref.close(); d_pre.close()


@pytest.mark.parametrize("arch", ["genset+battery", "battery+grid", "genset+battery+grid"])
def test_float32_actions_equal_widened_float64_actions(arch, device):
    """action_dtype=float32 (mgx_set_action_format): single steps, fused K-step launches and the general multi-module
    kernel give bit-identical rewards / state / logs to the float64 path fed ``actions.double()``."""
    from pymgrid_amd import BatchedMicrogridEnv, StepEngine
    from pymgrid_amd.generator import generate
    N, T, K = 777, 64, 9
    g = torch.Generator(device=device); g.manual_seed(3)

    def make():
        return generate(N, n_steps=T, seed=8, arch=arch, device=device, mixed_timers=True)
    e64, e32 = StepEngine(make()), StepEngine(make(), action_dtype=torch.float32)
    A = e64.action_dim
    for k in range(5):
        a = torch.rand(N, A, dtype=torch.float32, device=device, generator=g)
        r64, r32 = e64.step(a.double(), want_log=True), e32.step(a, want_log=True)
        assert all(torch.equal(x, y) for x, y in zip(r64, r32)), k
    a = torch.rand(K, N, A, dtype=torch.float32, device=device, generator=g) * 1.2 - 0.1       # some out of range
    o64 = e64.step_k(a.double(), reward=True, soc_trace=True, status_trace=True, log=True)
    o32 = e32.step_k(a, reward=True, soc_trace=True, status_trace=True, log=True)
    assert o64.keys() == o32.keys() and all(torch.equal(o64[k], o32[k]) for k in o64)
    for name in ("charge", "soc", "gen_status"):
        if name in e64.batch.cols and e64.batch.cols[name] is not None:
            assert torch.equal(e64.batch.cols[name], e32.batch.cols[name]), name
    with pytest.raises(ValueError):
        e32.step(torch.rand(N, A, dtype=torch.float64, device=device))
    e64.close(); e32.close()
    env = BatchedMicrogridEnv(make(), action_dtype=torch.float32)
    env.reset()
    assert env.sample_action().dtype == torch.float32
    env.step(env.sample_action())
    env.step({"genset": [[1.0, 0.5]], "battery": [0.5], "grid": [0.5]})
    env.close()
    # general path: two loads, three renewables
    rs = np.random.RandomState(3)
    grids = [dict(load_ts=rs.rand(T, 2) * [20, 5], pv_ts=rs.rand(T, 3) * [10, 4, 1], horizon=2, final_step=T,
                  initial_step=0, unbalanced=dict(loss_load_cost=10.0, overgeneration_cost=2.0),
                  battery=dict(min_capacity=20.0, max_capacity=100.0, max_charge=25.0, max_discharge=25.0,
                               efficiency=0.9, battery_cost_cycle=0.02, init_soc=0.5)) for _ in range(37)]
    m64, m32 = StepEngine(_batch(grids, device)), StepEngine(_batch(grids, device), action_dtype=torch.float32)
    for k in range(4):
        a = torch.rand(37, 1, dtype=torch.float32, device=device, generator=g)
        assert all(torch.equal(x, y) for x, y in zip(m64.step(a.double())[:3], m32.step(a)[:3])), k
    m64.close(); m32.close()


@pytest.mark.parametrize("seed", [0, 1])
def test_random_fleet_every_module_set_vs_oracle(seed, device, oracle):
    """Device vs oracle over a random fleet that covers EVERY kernel specialisation: all 8 module sets (incl. genset-only,
    grid-only, genset+grid, battery-only, none), both battery / grid sweep orders, several load / renewable modules,
    horizons 0 / 3 / 24, lossy and degenerate batteries, genset timers and initial states, weak grids, raw and
    out-of-range requests.  Bucketed by layout, 25 steps each: reward, done, state, observation and every log column.
    A grid on which the oracle raises the reference's AssertionError (an over-full lossy battery) is left out from there on: at most
    10 % of the fleet, and of every module set at least one grid is compared to the end."""
    from pymgrid_amd import MicrogridBatch, StepEngine, unpack_status
    rs = np.random.RandomState(4242 + seed)
    T = 40
    grids = []
    for n in range(260):
        arch = n % 8                                          # bit 0 genset, bit 1 battery, bit 2 grid
        H = int(rs.choice([0, 0, 3, 24]))
        peak = 10 ** rs.uniform(0, 4)
        multi = rs.rand() < 0.15
        nl, npv = (int(rs.randint(1, 10)), int(rs.randint(0, 10))) if multi else (1, 1)
        p = dict(load_ts=peak * rs.rand(T, nl) * (rs.rand(T, nl) > 0.05), pv_ts=peak * rs.rand(T, npv) * (rs.rand(T, npv) > 0.4),
                 horizon=H, final_step=T, initial_step=0,
                 unbalanced=dict(loss_load_cost=float(rs.choice([10.0, 0.0, 3.3])), overgeneration_cost=float(rs.choice([1.0, 0.0]))))
        if not multi:
            p["load_ts"], p["pv_ts"] = p["load_ts"][:, 0], p["pv_ts"][:, 0]
        if arch & 1:
            rmax = peak * rs.uniform(0.3, 1.5)
            p["genset"] = dict(running_min_production=rmax * float(rs.choice([0.05, 0.3])), running_max_production=rmax,
                               genset_cost=rs.uniform(0, 1), co2_per_unit=float(rs.choice([0.0, 2.0])),
                               cost_per_unit_co2=float(rs.choice([0.0, 0.1])), start_up_time=int(rs.randint(0, 4)),
                               wind_down_time=int(rs.randint(0, 4)), init_start_up=bool(rs.randint(0, 2)),
                               allow_abortion=bool(rs.rand() < 0.7))
        if arch & 2:
            cap = peak * rs.uniform(0.5, 5)
            cmin = cap * float(rs.choice([0.0, 0.2, 0.5]))
            p["battery"] = dict(min_capacity=cmin, max_capacity=cap, max_charge=cap * rs.uniform(0.05, 1.2),
                                max_discharge=cap * rs.uniform(0.05, 1.2), efficiency=float(rs.choice([1.0, 0.9, 0.5])),
                                battery_cost_cycle=float(rs.choice([0.0, 0.02, 1.0])), init_soc=float(rs.uniform(cmin / cap, 1)))
        if arch & 4:
            p["grid"] = dict(max_import=peak * rs.uniform(0, 2), max_export=peak * float(rs.choice([0.0, rs.uniform(0, 2)])),
                             cost_per_unit_co2=float(rs.choice([0.0, 0.1])))
            p["grid_ts"] = np.stack([rs.rand(T) * float(rs.choice([0.0, 1.0, 30.0])), rs.rand(T), rs.rand(T) * 0.5,
                                     (rs.rand(T) > float(rs.choice([0.0, 0.3]))).astype(float)], axis=1)
        if (arch & 6) == 6 and rs.rand() < 0.5:
            p["controllable_order"] = ["grid", "battery"]
        grids.append(p)
    buckets = _buckets(grids)
    module_set = lambda g: (g.get("genset") is not None, g.get("battery") is not None, g.get("grid") is not None)   # noqa: E731
    assert len({module_set(g) for g in grids}) == 8
    left_out = []                                             # fleet indices of the grids the oracle gave up on
    for idx in buckets:
        sub = [grids[i] for i in idx]
        eng = StepEngine(MicrogridBatch.from_grids(sub, device=device))
        L = eng.layout
        oms = [oracle.OracleMicrogrid(g) for g in sub]
        obs = eng.reset().cpu().numpy()
        for j, om in enumerate(oms):
            assert np.array_equal(obs[j], om.reset()), (idx[j], "reset")
        normalized = bool(rs.randint(0, 3))
        for k in range(25):
            a = rs.rand(len(sub), L.action_dim) * 1.3 - 0.15
            c = 0
            if L.has_genset:
                a[:, 0] = rs.rand(len(sub)); a[:, 1] = np.maximum(a[:, 1], 0); c = 2
            if not normalized:
                for j, g in enumerate(sub):
                    cc = c
                    if L.has_genset:
                        a[j, 1] *= g["genset"]["running_max_production"]
                    if L.has_battery:
                        a[j, cc] = (a[j, cc] * 2 - 1) * g["battery"]["max_discharge"]; cc += 1
                    if L.has_grid:
                        a[j, cc] = (a[j, cc] * 2 - 1) * max(g["grid"]["max_import"], g["grid"]["max_export"])
            o, r, d, log = eng.step(_t(a, device), normalized=normalized, want_log=True)
            o, r, d, log = o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy(), log.cpu().numpy()
            for j, (om, g) in enumerate(zip(oms, sub)):
                if om is None:
                    continue
                try:
                    out = om.run(actions_for(g, a[j]), normalized)
                except AssertionError:                     # an over-full lossy battery: the reference gives up there,
                    oms[j] = None                          # the grid is skipped from here on
                    continue
                where = (idx[j], k)
                assert r[j] == out.reward and int(d[j]) == out.done, where
                assert np.array_equal(o[j], om.observe()), where
                dd = out.as_dict()
                for cidx, name in enumerate(eng.log_names):
                    if name in dd:
                        assert log[cidx, j] == dd[name], (where, name)
        if L.n_load == 1 and L.n_pv == 1 and L.action_dim:   # the fused kernels of this specialisation: K steps, ids
            from pymgrid_amd.priority_list import MODULE_NAMES, get_priority_lists, table_array
            K = 6
            a = rs.rand(K, len(sub), L.action_dim)
            out = eng.step_k(_t(a, device), normalized=True, reward=True)
            rk = out["reward"].cpu().numpy()
            lists = get_priority_lists(L.has_genset, L.has_battery, L.has_grid, False, L.grid_before_battery)
            ids = rs.randint(0, len(lists), size=(K, len(sub))).astype(np.uint8)
            out = eng.rollout_discrete(_t(ids, device, torch.uint8), table_array(lists), K, reward=True)
            rd = out["reward"].cpu().numpy()
            for j, (om, g) in enumerate(zip(oms, sub)):
                if om is None:
                    continue
                try:
                    for k in range(K):
                        assert rk[k, j] == om.run(actions_for(g, a[k, j]), True).reward, (idx[j], "step_k", k)
                    for k in range(K):
                        act = om.populate_action([(MODULE_NAMES[m], a_) for m, a_ in lists[ids[k, j]]])
                        assert rd[k, j] == om.run(act, normalized=False).reward, (idx[j], "rollout", k)
                except AssertionError as e:
                    if "absorbed_energy" not in str(e):
                        raise
                    oms[j] = None
        cols = eng.batch.cols
        for j, om in enumerate(oms):
            if om is None:
                continue
            if L.has_battery:
                assert cols["charge"][j].item() == om.s.charge and cols["soc"][j].item() == om.s.soc, idx[j]
            if L.has_genset:
                assert unpack_status(cols["gen_status"][j:j + 1].cpu().numpy().view(np.uint32))[0].tolist() == list(om.status), idx[j]
        left_out += [idx[j] for j, om in enumerate(oms) if om is None]
        eng.close()
    assert len(left_out) <= 0.10 * len(grids), (len(left_out), len(grids))
    left_out = set(left_out)
    compared = {module_set(g) for i, g in enumerate(grids) if i not in left_out}
    assert len(compared) == 8, sorted({module_set(g) for g in grids} - compared)


def test_stream_shards_equal_one_engine(device):
    """StreamShards (independent shards on their own HIP streams, joined once at the end) == the same grids in one engine:
    fused K-step launches and on-device rule-based rollouts, several rounds without joining in between."""
    from pymgrid_amd import MicrogridBatch, StepEngine
    from pymgrid_amd.generator import generate
    from pymgrid_amd.hetero import StreamShards
    from pymgrid_amd.priority_list import get_priority_lists, table_array
    N, T, K, S = 6000, 200, 16, 3
    whole = StepEngine(generate(N, n_steps=T, seed=12, arch="genset+battery+grid", device=device, mixed_timers=True))
    shards = StreamShards([generate(N, n_steps=T, seed=12, arch="genset+battery+grid", device=device, mixed_timers=True,
                                    rank=j, world=S) for j in range(S)])
    n = N // S
    g = torch.Generator(device=device); g.manual_seed(4)
    tab = table_array(get_priority_lists(True, True, True))
    rw, rs = [], []
    shards.fork()
    for rnd in range(4):
        a = torch.rand(K, N, 4, dtype=torch.float64, device=device, generator=g)
        parts = [a[:, j * n:(j + 1) * n].contiguous() for j in range(S)]
        torch.cuda.current_stream(device).synchronize()          # the slices were made on the caller's stream
        rw.append(whole.step_k(a, reward=True)["reward"])
        rs.append(shards.step_k(parts, reward=True))
    ids = torch.randint(0, len(tab), (N,), device=device, generator=g).to(torch.uint8)
    parts = [ids[j * n:(j + 1) * n].contiguous() for j in range(S)]
    torch.cuda.current_stream(device).synchronize()
    rw.append(whole.rollout_discrete(ids, tab, K, reward=True)["reward"])
    rs.append(shards.rollout_discrete(parts, [tab] * S, K, reward=True))
    shards.join()
    for x, ys in zip(rw, rs):
        assert torch.equal(x, torch.cat([y["reward"] for y in ys], dim=1))
    for name in ("charge", "soc", "gen_status"):
        assert torch.equal(whole.batch.cols[name], torch.cat([e.batch.cols[name] for e in shards.engines]))
    whole.close(); shards.close()


def test_genset_fsm_tables_on_device(device):
    """G4 on the device: every distinct GensetModule.update_status transition of the reference, with and without
    allow_abortion (genset_module.py:235-346), as ONE batch -- a grid per transition, preset status, one step."""
    from pymgrid_amd import MicrogridBatch, StepEngine, unpack_status
    z = golden("genset_fsm.npz")
    rows = [(r, True) for r in z["transitions"]] + [(r, False) for r in z["transitions_no_abortion"]]
    T = 4
    grids = [dict(load_ts=np.zeros(T), pv_ts=np.zeros(T), horizon=0, final_step=T, initial_step=0,
                  unbalanced=dict(loss_load_cost=10.0, overgeneration_cost=2.0),
                  genset=dict(running_min_production=10.0, running_max_production=100.0, genset_cost=1.0, co2_per_unit=0.0,
                              cost_per_unit_co2=0.0, start_up_time=int(r[1 - 1]), wind_down_time=int(r[1]), allow_abortion=allow,
                              status=[int(r[3]), int(r[4]), int(r[5]), int(r[6])])) for r, allow in rows]
    eng = StepEngine(MicrogridBatch.from_grids(grids, device=device))
    a = np.zeros((len(rows), 2))
    a[:, 0] = [float(r[2]) for r, _ in rows]
    eng.step(_t(a, device), want_obs=False)
    post = unpack_status(eng.batch.cols["gen_status"].cpu().numpy().view(np.uint32))
    for j, (r, allow) in enumerate(rows):
        assert post[j].tolist() == [int(v) for v in r[7:11]], (allow, r.tolist())
    eng.close()
