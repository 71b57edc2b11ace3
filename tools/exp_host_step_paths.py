"""Host time per step of the Gym-step paths whose Python text lives in envs.py / hetero.py / engine.py, at a size where the GPU is never
the bound (1 000 grids per env or bucket, factorised series): time.perf_counter around `steps` steps after `warmup` -- what
tools/archive/exp_env_host_cost.py measured, with the unbound and the fleet paths added -- profiles/exp_host_step_paths.txt.

    a_env_bound        BatchedMicrogridEnv.step, bound (reuse_outputs=4)
    b_env_log          the same with log=True: unbound, the shared tail with log rows
    c_discrete_bound   DiscreteBatchedMicrogridEnv.step, bound
    c_discrete_log     the same with log=True
    d_pergrid_inline   PerGridWindowEnv(auto_reset=True).step at H = 0: the step kernel restarts the grids it finishes
    e_pergrid_ring     the same at H = 4 with rings: the restarted grids are patched into the ring behind the step
    f_pergrid_host     H = 0 with a torch generator: its draws restart the grids behind the step
    g_fleet_plans      BucketedFleet.step, per-step plans (reuse_outputs=0)
    g_fleet_fast       BucketedFleet.step, the fast path without binding (reuse_outputs=12, refill="chunks")
    g_fleet_bound      BucketedFleet.step, bound (reuse_outputs=12)
    h_pgfleet_h0       PerGridWindowFleet(auto_reset=True).step at H = 0
    h_pgfleet_h4       the same at H = 4

One invocation measures every path on one source tree (--root names the tree whose pymgrid_amd is imported: the yardstick is the
parent commit's tree, loading the same libmgx.so through MGX_LIB) and prints one JSON line per path; a job alternates the trees,
one process per tree and round:

    python tools/exp_host_step_paths.py [--root DIR] [--label parent|new] [--steps 10000] [--warmup 2000] [--only a_env_bound,...]
    python tools/exp_host_step_paths.py --table LINES.jsonl      (the table of all readings; a path is level when the new tree's
                                                                  median is no higher than the parent's highest reading)
"""
import argparse
import json
import os
import statistics
import sys
import time

N, T, LENGTH = 1000, 13_000, 168
ARCHS = ("genset+battery", "battery+grid", "genset+battery+grid")


def table(path):
    rows = {}
    for line in open(path):
        if line.startswith("{"):
            r = json.loads(line)
            rows.setdefault(r["path"], {}).setdefault(r["label"], []).append(r["us"])
    print(f"{'path':18s} {'parent readings':>26s} {'new readings':>20s}  parent max  new median  level")
    for name, by in rows.items():
        old, new = by.get("parent", []), by.get("new", [])
        if not old or not new:
            continue
        hi, med = max(old), statistics.median(new)
        print(f"{name:18s} {' '.join(f'{u:7.2f}' for u in old):>26s} {' '.join(f'{u:7.2f}' for u in new):>20s}  {hi:10.2f}  {med:10.2f}  "
              f"{'yes' if med <= hi else f'NO (+{med - hi:.2f} us)'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="new")
    ap.add_argument("--steps", type=int, default=10_000)
    ap.add_argument("--warmup", type=int, default=2_000)
    ap.add_argument("--only", default=None)
    ap.add_argument("--table", default=None)
    a = ap.parse_args()
    if a.table:
        return table(a.table)
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from pymgrid_amd import BatchedMicrogridEnv, DiscreteBatchedMicrogridEnv, _lib
    from pymgrid_amd.generator import generate
    from pymgrid_amd.hetero import BucketedFleet, PerGridWindowEnv, PerGridWindowFleet
    _lib.build()
    dev = torch.device("cuda:0")

    def batch(arch=ARCHS[2], H=0, seed=1):
        return generate(N, n_steps=T, seed=seed, arch=arch, horizon=H, device=dev, series="factorised")

    def batches(H):
        return [batch(arch, H, seed=1 + k) for k, arch in enumerate(ARCHS)]

    def gen():
        g = torch.Generator(device=dev)
        g.manual_seed(3)
        return g

    keep = dict(remove_redundant_gensets=False)
    pergrid = dict(trajectory_length=LENGTH, auto_reset=True, seed=5)
    paths = {
        "a_env_bound": lambda: BatchedMicrogridEnv(batch(), reuse_outputs=4),
        "b_env_log": lambda: BatchedMicrogridEnv(batch(), reuse_outputs=4, log=True),
        "c_discrete_bound": lambda: DiscreteBatchedMicrogridEnv(batch(), reuse_outputs=4, **keep),
        "c_discrete_log": lambda: DiscreteBatchedMicrogridEnv(batch(), reuse_outputs=4, log=True, **keep),
        "d_pergrid_inline": lambda: PerGridWindowEnv(batch(), **pergrid),
        "e_pergrid_ring": lambda: PerGridWindowEnv(batch(H=4), obs_prefetch=4, **pergrid),
        "f_pergrid_host": lambda: PerGridWindowEnv(batch(), generator=gen(), **pergrid),
        "g_fleet_plans": lambda: BucketedFleet.from_batches(batches(4), obs_prefetch=4),
        "g_fleet_fast": lambda: BucketedFleet.from_batches(batches(4), obs_prefetch=4, reuse_outputs=12, refill="chunks"),
        "g_fleet_bound": lambda: BucketedFleet.from_batches(batches(4), obs_prefetch=4, reuse_outputs=12),
        "h_pgfleet_h0": lambda: PerGridWindowFleet.from_batches(batches(0), **pergrid),
        "h_pgfleet_h4": lambda: PerGridWindowFleet.from_batches(batches(4), obs_prefetch=4, **pergrid),
    }
    for name in (a.only.split(",") if a.only else paths):
        torch.manual_seed(1)
        env = paths[name]()
        logs = getattr(env, "_keep_log", False)
        env.reset()
        act = env.sample_action()

        def run(n):
            for k in range(n):
                env.step(act)
                if logs and k % 500 == 499:          # (a log=True env keeps every step's rows until its next reset)
                    env._log_rows.clear()
                    env._shaped_rows.clear()
        run(a.warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(a.steps)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        print(json.dumps(dict(path=name, label=a.label, us=round(1e6 * (t1 - t0) / a.steps, 3), grids=N, steps=a.steps,
                              kernels=_lib.source_hash())), flush=True)
        (env.env if isinstance(env, PerGridWindowEnv) else env).close()
        del env


if __name__ == "__main__":
    main()
