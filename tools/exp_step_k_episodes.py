"""Timing of the fused continuous K-step over per-grid auto-reset episodes (PerGridWindowEnv.step_k, mgx_step_k_episodes) against
the single-step loop it replaces -- profiles/exp_step_k_episodes.txt.

100 000 generated genset+battery+grid grids, T = 8760, 168-step episodes, normalised controls out of a pre-drawn [K, N, A] tensor,
factorised and materialised series.  One invocation measures ONE mode and prints one JSON line, so that a job can alternate modes
(and source trees: --root names the tree whose pymgrid_amd is imported -- the baseline is measured on the parent commit's tree):

    step      PerGridWindowEnv(discrete=False, auto_reset=True, observations=False).step(actions[k])    us per step (any tree)
    step_k    PerGridWindowEnv.step_k(actions)                                                          us per step (trees that have it)
    lockstep  engine.step_k(actions) from row 0, every grid on the same row                             us per step (scale, any tree)

    python tools/exp_step_k_episodes.py --mode step_k --series factorised --K 64 [--root DIR] [--steps 2048] [--warmup 512]
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["step", "step_k", "lockstep"], required=True)
    ap.add_argument("--series", choices=["factorised", "materialised"], default="factorised")
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=512)
    ap.add_argument("--grids", type=int, default=100_000)
    ap.add_argument("--T", type=int, default=8760)
    ap.add_argument("--length", type=int, default=168)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from pymgrid_amd import _lib
    from pymgrid_amd.generator import generate
    from pymgrid_amd.hetero import PerGridWindowEnv
    from pymgrid_amd.envs import BatchedMicrogridEnv
    _lib.build()
    dev = torch.device("cuda:0")
    batch = generate(a.grids, n_steps=a.T, seed=42, arch="genset+battery+grid", device=dev, series=a.series)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    actions = torch.rand(a.K, a.grids, batch.layout.action_dim, dtype=torch.float64, device=dev, generator=g)
    torch.manual_seed(1)

    def timed(fn, n_calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_calls):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    res = dict(mode=a.mode, series=a.series, K=a.K, grids=a.grids, kernels=_lib.source_hash())
    if a.mode == "lockstep":
        env = BatchedMicrogridEnv(batch, observations=False)
        e = env.engine
        out = {"reward": torch.empty(a.K, a.grids, dtype=torch.float64, device=dev)}

        def call():
            if e.current_step + a.K > a.T:
                e.reset(0, want_obs=False)
            e.step_k(actions, reward=True, out=out)
        timed(call, max(1, a.warmup // a.K))
        n = max(1, a.steps // a.K)
        res["us_per_step"] = timed(call, n) / (n * a.K) * 1e6
    else:
        pe = PerGridWindowEnv(batch, trajectory_length=a.length, discrete=False, auto_reset=True, seed=7, observations=False)
        pe.reset()
        if a.mode == "step":
            rows = [actions[k] for k in range(a.K)]
            pos = [0]

            def one():
                pe.step(rows[pos[0] % a.K])
                pos[0] += 1
            timed(one, a.warmup)
            res["us_per_step"] = timed(one, a.steps) / a.steps * 1e6
        else:
            out = {"reward": torch.empty(a.K, a.grids, dtype=torch.float64, device=dev)}
            call = lambda: pe.step_k(actions, reward=True, out=out)      # noqa: E731
            timed(call, max(1, a.warmup // a.K))
            n = max(1, a.steps // a.K)
            res["us_per_step"] = timed(call, n) / (n * a.K) * 1e6
            res["episodes_finished"] = int(pe.episode_stats["episodes"].sum())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
