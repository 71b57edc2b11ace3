"""Timing of the closed-loop policy roll-outs inside the fused per-grid-episode launches (PerGridWindowEnv.rollout_policy /
step_k_policy, mgx_rollout_policy_episodes / mgx_step_k_policy_episodes) -- profiles/exp_policy_rollout.txt.

100 000 generated genset+battery+grid grids, T = 8760, 168-step episodes, factorised series, no forecast horizon, K = 64; the
discrete and the continuous head, n_hidden 0 and 16.  Three legs per (head, n_hidden), us per env-step each:

    (a) stepped   K times [the policy as torch operations on the device + pe.step]: the loop the launch replaces.  The policy here
                  is the FAST torch form (two matmuls, relu, argmax / clamp), not MLPPolicy.act's ordered loop -- what a user would
                  have written; its actions may differ from the kernel's in the last bit of a logit, its cost does not
    (b) floor     the open-loop rollout / step_k with observations=True on pre-drawn actions: the launch without a policy
    (c) fused     rollout_policy / step_k_policy, with observations=True and without

Every leg: warm-up calls, then `--repeats` timed blocks (torch.cuda.synchronize() around a block); the median block and the spread
(min .. max) are reported.  (a)/(c) and (c)/(b) from the medians, + the resource figures of the two kernels of this configuration.

    python tools/exp_policy_rollout.py [--out profiles/exp_policy_rollout.txt] [--grids 100000] [--K 64] [--repeats 5]
                                       [--series materialised] [--root DIR]      (--root: the tree whose pymgrid_amd is imported)
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
    ap.add_argument("--launches", type=int, default=8, help="fused launches per timed block")
    ap.add_argument("--stepped", type=int, default=128, help="single steps per timed block of leg (a)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--series", choices=["factorised", "materialised"], default="factorised")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    import torch
    from pymgrid_amd import MLPPolicy, _lib
    from pymgrid_amd.generator import generate
    from pymgrid_amd.hetero import PerGridWindowEnv
    _lib.build()
    dev = torch.device("cuda:0")
    N, K = a.grids, a.K
    lines = [f"# tools/exp_policy_rollout.py: {N} genset+battery+grid grids, T = {a.T}, {a.length}-step episodes, {a.series}, H = 0, "
             f"K = {K}; kernels {_lib.source_hash()}; {torch.cuda.get_device_name(0)}",
             f"# us per env-step: median of {a.repeats} blocks (min .. max); a block = {a.launches} launches of {K} steps, leg (a): "
             f"{a.stepped} single steps"]

    def blocks(fn, calls, steps_per_call, warm):
        for _ in range(warm):
            fn()
        us = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) / (calls * steps_per_call) * 1e6)
        return statistics.median(us), min(us), max(us)

    def fmt(r):
        return f"{r[0]:8.2f} ({r[1]:.2f} .. {r[2]:.2f})"

    results = []
    for discrete in (True, False):
        for n_hidden in (0, 16):
            head = "discrete" if discrete else "continuous"
            mk = lambda: PerGridWindowEnv(generate(N, n_steps=a.T, seed=42, arch="genset+battery+grid", device=dev, series=a.series),  # noqa: E731
                                          trajectory_length=a.length, discrete=discrete, auto_reset=True, seed=7)
            pe = mk()
            obs0 = pe.reset()
            D = pe.env.engine.obs_dim
            n_out = pe.env.action_space.n if discrete else pe.env.engine.action_dim
            rng = np.random.default_rng(3)
            W1 = rng.normal(0, 1.5, size=(n_hidden, D)) if n_hidden else None
            b1 = rng.normal(0, 0.5, size=n_hidden) if n_hidden else None
            W2 = rng.normal(0, 0.6 if n_hidden else 1.5, size=(n_out, n_hidden or D))
            b2 = rng.normal(0.0 if discrete else 0.5, 0.5, size=n_out)
            policy = MLPPolicy(W1, b1, W2, b2, head=head).to(dev)
            # (a) the stepped loop with the fast torch policy
            w1t = None if W1 is None else policy.W1[0].t().contiguous()
            w2t = policy.W2[0].t().contiguous()
            state = [obs0]

            def stepped():
                x = state[0]
                if w1t is not None:
                    x = torch.relu(torch.addmm(policy.b1[0], x, w1t))
                y = torch.addmm(policy.b2[0], x, w2t)
                act = y.argmax(dim=1).to(torch.int32) if discrete else y.clamp(0.0, 1.0)
                state[0] = pe.step(act)[0] if discrete else pe.step(act, normalized=True)[0]
            ra = blocks(stepped, a.stepped, 1, 64)
            pe.env.close()
            # (b) the open-loop launch with rows, on pre-drawn actions
            pe = mk()
            pe.reset()
            g = torch.Generator(device=dev)
            g.manual_seed(11)
            if discrete:
                ctl = torch.randint(0, n_out, (K, N), device=dev, generator=g).to(torch.uint8)
                outb = dict(reward=torch.empty(K, N, dtype=torch.float64, device=dev), obs=torch.empty(K, N, D, dtype=torch.float64, device=dev))
                floor = lambda: pe.rollout(ctl, reward=True, observations=True, out=outb)     # noqa: E731
            else:
                ctl = torch.rand(K, N, n_out, dtype=torch.float64, device=dev, generator=g)
                outb = dict(reward=torch.empty(K, N, dtype=torch.float64, device=dev), obs=torch.empty(K, N, D, dtype=torch.float64, device=dev))
                floor = lambda: pe.step_k(ctl, reward=True, observations=True, out=outb)      # noqa: E731
            rb = blocks(floor, a.launches, K, 4)
            pe.env.close()
            # (c) the closed-loop launch, with rows and without
            pe = mk()
            pe.reset()
            call = pe.rollout_policy if discrete else pe.step_k_policy
            rc_rows = blocks(lambda: call(policy, K, reward=True, observations=True, out=outb), a.launches, K, 4)
            outr = dict(reward=outb["reward"])
            rc = blocks(lambda: call(policy, K, reward=True, out=outr), a.launches, K, 4)
            restarts = int(pe.episode_stats["episodes"].sum())
            pe.env.close()
            results.append(dict(head=head, n_hidden=n_hidden, n_out=int(n_out), stepped=ra[0], floor=rb[0], fused_rows=rc_rows[0], fused=rc[0]))
            lines += [f"{head:10s} n_hidden = {n_hidden:2d}  (n_in = {D}, n_out = {n_out}; {restarts} episodes finished inside leg (c))",
                      f"    (a) stepped: torch policy + pe.step          {fmt(ra)}",
                      f"    (b) floor: open loop, observations=True       {fmt(rb)}",
                      f"    (c) fused policy, observations=True           {fmt(rc_rows)}",
                      f"    (c) fused policy, no observations             {fmt(rc)}",
                      f"    (a)/(c) = {ra[0] / rc_rows[0]:.2f} with observations, {ra[0] / rc[0]:.2f} without;  (c)/(b) = {rc_rows[0] / rb[0]:.2f}"]
    usage = _lib.resource_usage() or {}
    for name in ("mgx::rollout_policy_episodes_kernel<7, 4, 0>", "mgx::step_k_policy_episodes_kernel<7, 4, 0>"):
        if name in usage:
            lines.append(f"# {name}: {json.dumps(usage[name], sort_keys=True)}")
    lines.append("# " + json.dumps(results))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
