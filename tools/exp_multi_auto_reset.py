"""Discrete auto-reset episodes on a layout with several modules of a kind (2 gensets + 2 batteries + 1 grid, N = 100 000, H = 0):
PerGridWindowEnv(discrete=True, auto_reset=True) -- in-place episodes, device draws -- with mgx_step_lists in one launch
(step_lists_small_kernel<F, true>, the restart in the kernel) against its two-launch form (multi_small_own = 0: expand_multi_kernel ->
control [N, A] -> step_multi_kernel<F, true>).  Times env.step (observation rows, done flags) and engine.step_lists alone (reward +
done, no rows); the modes alternate per repetition.  --reps 1 --warmup 0 --modes one --steps 100 --env-only: the loop to run under
`rocprofv3 --kernel-trace --stats` (one step_lists_small_kernel launch per step, no expand_multi_kernel)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pymgrid_amd import _lib  # noqa: E402
from pymgrid_amd.generator import generate, widen  # noqa: E402
from pymgrid_amd.hetero import PerGridWindowEnv  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--grids", type=int, default=100_000)
ap.add_argument("--rows", type=int, default=1200)
ap.add_argument("--length", type=int, default=24, help="trajectory_length of every episode")
ap.add_argument("--steps", type=int, default=1000)
ap.add_argument("--warmup", type=int, default=50)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--modes", default="one,two")
ap.add_argument("--env-only", action="store_true", help="time env.step only (the profiled loop)")
args = ap.parse_args()

dev = torch.device("cuda:0")
N = args.grids
torch.manual_seed(0)
envs = {}
for mode in args.modes.split(","):
    b = widen(generate(N, n_steps=args.rows, seed=5, arch="genset+battery+grid", horizon=0, device=dev, mixed_timers=True),
              n_genset=2, n_battery=2, n_grid=1)
    envs[mode] = PerGridWindowEnv(b, trajectory_length=args.length, discrete=True, auto_reset=True, seed=3, remove_redundant_gensets=False)
g = torch.Generator(device=dev); g.manual_seed(1)
n_ids = max(args.steps, args.warmup, 1)
ids = torch.randint(0, next(iter(envs.values())).action_space.n, (n_ids, N), dtype=torch.int32, device=dev, generator=g)
reward = torch.empty(N, dtype=torch.float64, device=dev)
done = torch.empty(N, dtype=torch.uint8, device=dev)


def timed(fn):
    for k in range(args.warmup):
        fn(ids[k])
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for k in range(args.steps):
        fn(ids[k])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / max(args.steps, 1) * 1e6


print(f"N = {N}, episodes of {args.length} steps, {args.steps} timed steps after {args.warmup}; multi_small_own: one = 1, two = 0")
for rep in range(args.reps):
    for mode, env in envs.items():
        _lib.set_tunable("multi_small_own", 1 if mode == "one" else 0)
        env.reset()
        e, lists = env.env.engine, env.env._lists
        us_env = timed(lambda a: env.step(a))
        if args.env_only:
            print(f"rep {rep} {mode} launch(es): env.step {us_env:.2f} us per env-step")
            continue
        # (two launches: the control buffer passed in, so that the call does not first try the one-launch form)
        out = dict(reward=reward, done=done, control=None if mode == "one" else e._empty(N, e.action_dim))
        us_eng = timed(lambda a: e.step_lists(a, lists, want_obs=False, out=out))
        print(f"rep {rep} {mode} launch(es): env.step {us_env:.2f} us, engine.step_lists (no rows) {us_eng:.2f} us per env-step")
_lib.set_tunable("multi_small_own", 1)
for env in envs.values():
    env.env.close()
