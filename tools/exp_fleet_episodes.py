"""Per-grid auto-reset episodes on the config-5 fleet (PerGridWindowFleet): microseconds per fleet step for
  - the fused episode launch (fleet_step_kernel_v<true>: the in-place buckets of a fleet step in ONE launch),
  - the fleet_episodes tunable = 0 (the same mgx_fleet_step call, one step launch per in-place bucket beside it),
  - the per-bucket PerGridWindowEnv loop (one env.step per bucket from Python),
  - the lock-step BucketedFleet, for reference;
at H = 0 (rows per step) and H = 24 (observation rings), float64 and float32 rows.  99 999 generate_fleet grids (factorised series),
T = 8760, trajectory_length = 168 with device draws.

    python tools/exp_fleet_episodes.py [--grids 99999] [--steps 400] [--warmup 100] [--only H:dtype:mode]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/exp_fleet_episodes.py --steps 50 --warmup 10 --only 0:f64:fused
      (the kernel launches per step: the stats count over --steps + --warmup steps and the resets)

Prints one line per (H, dtype, mode): us per fleet step (device events over `steps` steps after `warmup`)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pymgrid_amd import _lib  # noqa: E402
from pymgrid_amd.generator import generate_fleet  # noqa: E402
from pymgrid_amd.hetero import BucketedFleet, PerGridWindowEnv, PerGridWindowFleet  # noqa: E402

MODES = ("fused", "beside", "loop", "lockstep")


def time_steps(step, actions, steps, warmup):
    for _ in range(warmup):
        step(actions)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        step(actions)
    t1.record()
    torch.cuda.synchronize()
    return 1e3 * t0.elapsed_time(t1) / steps


def run(batches, H, dtype, mode, steps, warmup):
    kw = dict(obs_dtype=dtype)
    _lib.set_tunable("fleet_episodes", 0 if mode == "beside" else 1)
    if mode == "lockstep":
        fleet = BucketedFleet.from_batches(batches, **kw)
        fleet.reset()
        step, close, actions = fleet.step, fleet.close, fleet.sample_action()
    elif mode == "loop":
        envs = [PerGridWindowEnv(b, trajectory_length=168, auto_reset=True, seed=5 + k, **kw) for k, b in enumerate(batches)]
        for pe in envs:
            pe.reset()

        def step(actions):
            for pe, a in zip(envs, actions):
                pe.step(a)

        def close():
            for pe in envs:
                pe.env.close()
        actions = [pe.sample_action() for pe in envs]
    else:
        fleet = PerGridWindowFleet.from_batches(batches, trajectory_length=168, auto_reset=True, seed=5, **kw)
        fleet.reset()
        step, close, actions = fleet.step, fleet.close, fleet.sample_action()
    us = time_steps(step, actions, steps, warmup)
    close()
    _lib.set_tunable("fleet_episodes", 1)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, default=99_999)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--only", default=None, help="H:dtype:mode, e.g. 0:f64:fused")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_fleet_episodes needs a GPU")
    cases = [(H, dt, m) for H in (0, 24) for dt in ("f64", "f32") for m in MODES]
    if args.only:
        h, dt, m = args.only.split(":")
        cases = [(int(h), dt, m)]
    parts = {}
    print(f"grids {args.grids}, T 8760, trajectory_length 168 (device draws), steps {args.steps} after {args.warmup}", flush=True)
    for H, dt, mode in cases:
        if H not in parts:
            parts.clear()
            parts[H] = [b for b, _ in generate_fleet(args.grids, n_steps=8760, seed=42, horizon=H, device="cuda",
                                                      series="factorised").values()]
            print(f"H = {H}: buckets " + ", ".join(str(b.layout.n_grids) for b in parts[H]), flush=True)
        us = run(parts[H], H, torch.float32 if dt == "f32" else torch.float64, mode, args.steps, args.warmup)
        print(f"H = {H:2d}  {dt}  {mode:8s}  {us:8.2f} us per fleet step", flush=True)


if __name__ == "__main__":
    main()
