"""What exploration costs inside the closed-loop fused launches (PerGridWindowEnv.rollout_policy / step_k_policy with
``exploration=``, mgx_rollout_policy_explore_episodes / mgx_step_k_policy_explore_episodes) -- profiles/exp_policy_explore.txt.

100 000 generated grids of layout 7 (genset+battery+grid) and 3 (genset+battery), T = 8760, 168-step episodes, factorised series,
no forecast horizon, K = 64, 16 hidden units; the discrete and the continuous head.  Three legs per (layout, head), us per env-step:

    (g) greedy    rollout_policy / step_k_policy: the greedy kernels, which this feature leaves as they were
    (z) draws     the exploring kernels with epsilon = 0 / sigma = 0: every draw is made, no action changes -- the same
                  trajectories as (g), so (z) - (g) is the price of the Philox rounds and what surrounds them alone
    (x) explore   the exploring kernels with epsilon = 0.25 / sigma = 0.15

The legs run in the same process on envs of their own and ALTERNATE block by block (g, z, x, g, z, x, ...), so a drift of the box
falls on all three; every leg is warmed up first.  A block = `--launches` launches of K steps between two torch.cuda.synchronize();
the median block and the spread (min .. max) are reported, + the draws per step and the resource figures of the forms timed.

    python tools/exp_policy_explore.py [--out profiles/exp_policy_explore.txt] [--grids 100000] [--K 64] [--repeats 7] [--root DIR]
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--grids", type=int, default=100_000)
    ap.add_argument("--T", type=int, default=8760)
    ap.add_argument("--length", type=int, default=168)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--launches", type=int, default=24, help="launches per timed block")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    import torch
    from pymgrid_amd import Exploration, MLPPolicy, _lib
    from pymgrid_amd.generator import generate
    from pymgrid_amd.hetero import PerGridWindowEnv
    _lib.build()
    dev = torch.device("cuda:0")
    N, K = a.grids, a.K
    lines = [f"# tools/exp_policy_explore.py: {N} grids, T = {a.T}, {a.length}-step episodes, factorised, H = 0, K = {K}, "
             f"{a.hidden} hidden units; kernels {_lib.source_hash()}; {torch.cuda.get_device_name(0)}",
             f"# us per env-step: median of {a.repeats} blocks (min .. max); a block = {a.launches} launches of {K} steps; the legs "
             f"alternate block by block; reward is the only output"]

    def fmt(us):
        return f"{statistics.median(us):8.3f} ({min(us):.3f} .. {max(us):.3f})"

    results = []
    usage = _lib.resource_usage() or {}
    for arch, flags in (("genset+battery+grid", 7), ("genset+battery", 3)):
        for discrete in (True, False):
            head = "discrete" if discrete else "continuous"
            legs = {"g": None, "z": Exploration(7, epsilon=0.0, sigma=0.0), "x": Exploration(7, epsilon=0.25, sigma=0.15)}
            envs, calls = {}, {}
            for leg, ex in legs.items():
                pe = PerGridWindowEnv(generate(N, n_steps=a.T, seed=42, arch=arch, device=dev, series="factorised"),
                                      trajectory_length=a.length, discrete=discrete, auto_reset=True, seed=7)
                torch.manual_seed(41)                          # the same first draw of the episodes in every leg
                pe.reset()
                envs[leg] = pe
            pe = envs["g"]
            D = pe.env.engine.obs_dim
            n_out = pe.env.action_space.n if discrete else pe.env.engine.action_dim
            rng = np.random.default_rng(3)
            policy = MLPPolicy(rng.normal(0, 1.5, size=(a.hidden, D)), rng.normal(0, 0.5, size=a.hidden),
                               rng.normal(0, 0.6, size=(n_out, a.hidden)), rng.normal(0.0 if discrete else 0.5, 0.5, size=n_out),
                               head=head).to(dev)
            out = {leg: dict(reward=torch.empty(K, N, dtype=torch.float64, device=dev)) for leg in legs}
            for leg, ex in legs.items():
                fn = envs[leg].rollout_policy if discrete else envs[leg].step_k_policy
                calls[leg] = (lambda fn=fn, ex=ex, leg=leg: fn(policy, K, reward=True, out=out[leg], exploration=ex))
            for leg in legs:                                   # warm-up: every kernel form of the timed window
                for _ in range(4):
                    calls[leg]()
            torch.cuda.synchronize()
            assert torch.equal(out["g"]["reward"], out["z"]["reward"])          # (z) walks the trajectories of (g)
            us = {leg: [] for leg in legs}
            for _ in range(a.repeats):
                for leg in legs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.launches):
                        calls[leg]()
                    torch.cuda.synchronize()
                    us[leg].append((time.perf_counter() - t0) / (a.launches * K) * 1e6)
            assert torch.equal(out["g"]["reward"], out["z"]["reward"])
            med = {leg: statistics.median(v) for leg, v in us.items()}
            draws = 1 if discrete else n_out
            per_draw = (med["z"] - med["g"]) / draws / N * 1e6          # ps per draw, chip-wide: a step of N grids makes N * draws of them
            kernel = "rollout_policy" if discrete else "step_k_policy"
            lines += [f"layout {flags} ({arch}), {head} head  (n_in = {D}, n_out = {n_out}; {draws} draw{'s' if draws > 1 else ''} per grid and step)",
                      f"    (g) greedy                         {fmt(us['g'])}",
                      f"    (z) exploring, epsilon = sigma = 0 {fmt(us['z'])}",
                      f"    (x) exploring, 0.25 / 0.15         {fmt(us['x'])}",
                      f"    (z)/(g) = {med['z'] / med['g']:.3f}   (x)/(g) = {med['x'] / med['g']:.3f}   (z) - (g) = {med['z'] - med['g']:.3f} us per step "
                      f"= {per_draw:.1f} ps per draw (chip-wide)"]
            for name in (f"mgx::{kernel}_episodes_kernel<{flags}, {4 if flags & 4 else 8}, 0>",
                         f"mgx::{kernel}_head_episodes_kernel<{flags}, {4 if flags & 4 else 8}, 0, 1>"):      # (1: HEAD_EXPLORE)
                if name in usage:
                    lines.append(f"#   {name}: {json.dumps(usage[name], sort_keys=True)}")
            results.append(dict(layout=flags, head=head, n_out=int(n_out), draws=draws, **{k: round(v, 4) for k, v in med.items()}))
            for pe in envs.values():
                pe.env.close()
            del envs, calls, out
            torch.cuda.empty_cache()
    lines.append("# " + json.dumps(results))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
