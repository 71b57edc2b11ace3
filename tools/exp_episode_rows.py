"""Timing of the fused roll-out over per-grid auto-reset episodes WITH observation rows (PerGridWindowEnv.rollout(observations=True,
final_observations=True), mgx_rollout_episodes_rows) against the only way to get those rows without it: the
PerGridWindowEnv(final_observation=True).step loop -- profiles/exp_episode_rows.txt.

100 000 generated genset+battery+grid grids, T = 8760, 168-step episodes, fixed rule-based ids, factorised and materialised series,
float64 and float32 rows.  One invocation builds one batch, measures the modes it is given on it and prints one JSON line per
(mode, K), so that a job can alternate source trees (--root names the tree whose pymgrid_amd is imported -- the yardstick is measured
on the parent commit's tree):

    step_rows     PerGridWindowEnv(discrete=True, auto_reset=True, final_observation=True).step(ids): obs + info["final_observation"]
                  + reward + done per step                                                          us per step (any tree)
    rollout_rows  PerGridWindowEnv.rollout(ids, K, reward, done, observations, final_observations)  us per step (trees that have it)
    rollout       the same launch without the rows (reward + done)                                  us per step (scale)

    python tools/exp_episode_rows.py --mode rollout_rows,rollout --series factorised --dtype float64 --K 64,512 [--root DIR] [--steps 2048] [--warmup 512]

bytes_per_env_step is the algorithmic HBM traffic of the launch per grid and step (the series values a step reads, reward 8 + done 1
written, + D x 8 or D x 4 for the row; final_obs adds D x itemsize / 168 on average); hbm_fraction prices it at 8 TB/s.
--launches N (rollout modes): run N launches and stop -- the form a counter pass (rocprofv3 --pmc FETCH_SIZE | WRITE_SIZE, each in
a run of its own) is taken of.
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, help="step_rows | rollout_rows | rollout, or several separated by commas")
    ap.add_argument("--series", choices=["factorised", "materialised"], default="factorised")
    ap.add_argument("--dtype", choices=["float64", "float32"], default="float64")
    ap.add_argument("--K", default="64", help="steps per launch (roll-out modes), or several separated by commas")
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=512)
    ap.add_argument("--grids", type=int, default=100_000)
    ap.add_argument("--T", type=int, default=8760)
    ap.add_argument("--length", type=int, default=168)
    ap.add_argument("--launches", type=int, default=0)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from pymgrid_amd import _lib
    from pymgrid_amd.generator import generate
    from pymgrid_amd.hetero import PerGridWindowEnv
    from pymgrid_amd.rbc import default_priority_ids
    _lib.build()
    dev = torch.device("cuda:0")
    dt = getattr(torch, a.dtype)
    batch = generate(a.grids, n_steps=a.T, seed=42, arch="genset+battery+grid", device=dev, series=a.series)   # (one batch for every mode)

    def timed(fn, n_calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_calls):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for mode in a.mode.split(","):
        if mode not in ("step_rows", "rollout_rows", "rollout"):
            raise SystemExit(f"unknown mode {mode!r}")
        torch.manual_seed(1)
        pe = PerGridWindowEnv(batch, trajectory_length=a.length, discrete=True, auto_reset=True, seed=7, obs_dtype=dt,
                              final_observation=mode == "step_rows")
        ids8 = torch.from_numpy(default_priority_ids(batch, pe.env.actions_list)).to(dev)
        pe.reset()
        D = pe.env.engine.obs_dim
        for K in ([0] if mode == "step_rows" else [int(k) for k in a.K.split(",")]):
            res = dict(mode=mode, series=a.series, dtype=a.dtype, K=K, grids=a.grids, obs_dim=D, kernels=_lib.source_hash())
            if mode == "step_rows":
                ids = ids8.to(torch.int32)
                timed(lambda: pe.step(ids), a.warmup)
                res["us_per_step"] = timed(lambda: pe.step(ids), a.steps) / a.steps * 1e6
            else:
                rows = mode == "rollout_rows"
                out = {"reward": torch.empty(K, a.grids, dtype=torch.float64, device=dev),
                       "done": torch.empty(K, a.grids, dtype=torch.uint8, device=dev)}
                kw = {}
                if rows:
                    out["obs"] = torch.empty(K, a.grids, D, dtype=dt, device=dev)
                    out["final_obs"] = torch.zeros(K, a.grids, D, dtype=dt, device=dev)
                    kw = dict(observations=True, final_observations=True)
                call = lambda: pe.rollout(ids8, K, reward=True, done=True, out=out, **kw)      # noqa: E731
                if a.launches:
                    timed(call, a.launches)
                    res["launches"] = a.launches
                else:
                    timed(call, max(1, a.warmup // K))
                    n = max(1, a.steps // K)
                    res["us_per_step"] = timed(call, n) / (n * K) * 1e6
                res["episodes_finished"] = int(pe.episode_stats["episodes"].sum())
                # series values read per step: factorised 3 base values + an outage word per 64 rows; materialised 6 values
                series = 3 * 8 + 8 / 64 if a.series == "factorised" else 6 * 8
                item = 8 if a.dtype == "float64" else 4
                res["bytes_per_env_step"] = series + 8 + 1 + (D * item * (1 + 1 / a.length) if rows else 0)
                if "us_per_step" in res:
                    res["hbm_fraction"] = res["bytes_per_env_step"] * a.grids / (res["us_per_step"] * 1e-6) / 8e12
                del out
            print(json.dumps(res), flush=True)
        pe.env.close()
        del pe


if __name__ == "__main__":
    main()
