"""What softmax sampling costs inside the closed-loop fused discrete launch (PerGridWindowEnv.rollout_policy with ``sampling=``,
mgx_rollout_policy_sample_episodes) -- profiles/exp_policy_sample.txt.

100 000 generated grids of layout 7 (genset+battery+grid, 12 priority lists) and 3 (genset+battery, 4 lists), T = 8760, 168-step
episodes, factorised series, no forecast horizon, K = 64, 16 hidden units.  Four fused legs per layout, us per env-step (one step
of all grids):

    (g) greedy     rollout_policy: the greedy kernel
    (x) epsilon    rollout_policy with exploration=Exploration(epsilon=0.25): one Philox draw per grid and step
    (s) sampling   rollout_policy with sampling=Sampling(temperature=1.0), probs=True: up to n_out - 1 evaluations of the exp of
                   mgx_sampling, one Philox draw, one division and one more [K, N] stream per grid and step
    (c) cold       the sampling kernel at temperature 0: every lane takes the greedy id, the weights are still formed

and the loop the launch replaces:

    (t) stepped    K times ``ids = torch.multinomial(torch.softmax(policy(obs)), 1); obs, r, done, _ = pe.step(ids)``, the policy as
                   two torch matmuls

The fused legs run in the same process on envs of their own and ALTERNATE block by block (g, x, s, c, g, ...), so a drift of the box
falls on all; every leg is warmed up first.  A block = `--launches` launches of K steps between two torch.cuda.synchronize(); the
median block and the spread (min .. max) are reported, with the resource figures of the forms timed.  No threshold is applied: the
figures are the result.

    python tools/exp_policy_sample.py [--out profiles/exp_policy_sample.txt] [--grids 100000] [--K 64] [--repeats 7] [--root DIR]
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
    ap.add_argument("--stepped-blocks", type=int, default=3, help="blocks of K single steps of the stepped loop")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    import torch
    from pymgrid_amd import Exploration, MLPPolicy, Sampling, _lib
    from pymgrid_amd.generator import generate
    from pymgrid_amd.hetero import PerGridWindowEnv
    _lib.build()
    dev = torch.device("cuda:0")
    N, K = a.grids, a.K
    lines = [f"# tools/exp_policy_sample.py: {N} grids, T = {a.T}, {a.length}-step episodes, factorised, H = 0, K = {K}, "
             f"{a.hidden} hidden units; kernels {_lib.source_hash()}; {torch.cuda.get_device_name(0)}",
             f"# us per env-step: median of {a.repeats} blocks (min .. max); a block = {a.launches} launches of {K} steps; the fused legs "
             f"alternate block by block; reward is the only output, (s) and (c) also write probs; (t): {a.stepped_blocks} blocks of {K} single steps"]

    def fmt(us):
        return f"{statistics.median(us):8.3f} ({min(us):.3f} .. {max(us):.3f})"

    results = []
    usage = _lib.resource_usage() or {}
    for arch, flags in (("genset+battery+grid", 7), ("genset+battery", 3)):
        legs = {"g": {}, "x": dict(exploration=Exploration(7, epsilon=0.25)), "s": dict(sampling=Sampling(7, temperature=1.0), probs=True),
                "c": dict(sampling=Sampling(7, temperature=0.0), probs=True)}
        envs, calls = {}, {}
        for leg in list(legs) + ["t"]:
            pe = PerGridWindowEnv(generate(N, n_steps=a.T, seed=42, arch=arch, device=dev, series="factorised"),
                                  trajectory_length=a.length, discrete=True, auto_reset=True, seed=7)
            torch.manual_seed(41)                          # the same first draw of the episodes in every leg
            pe.obs0 = pe.reset()
            envs[leg] = pe
        pe = envs["g"]
        D, n_out = pe.env.engine.obs_dim, pe.env.action_space.n
        rng = np.random.default_rng(3)
        policy = MLPPolicy(rng.normal(0, 1.5, size=(a.hidden, D)), rng.normal(0, 0.5, size=a.hidden),
                           rng.normal(0, 0.6, size=(n_out, a.hidden)), rng.normal(0.0, 0.5, size=n_out), head="discrete").to(dev)
        out = {leg: dict(reward=torch.empty(K, N, dtype=torch.float64, device=dev), actions=torch.empty(K, N, dtype=torch.uint8, device=dev))
               for leg in legs}
        for leg in ("s", "c"):
            out[leg]["probs"] = torch.empty(K, N, dtype=torch.float64, device=dev)
        for leg, kw in legs.items():
            calls[leg] = (lambda fn=envs[leg].rollout_policy, kw=kw, leg=leg: fn(policy, K, reward=True, actions=True, out=out[leg], **kw))
        for leg in legs:                                   # warm-up: every kernel form of the timed window
            for _ in range(4):
                calls[leg]()
        torch.cuda.synchronize()
        assert torch.equal(out["g"]["reward"], out["c"]["reward"])          # (c) walks the trajectories of (g)
        us = {leg: [] for leg in legs}
        for _ in range(a.repeats):
            for leg in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.launches):
                    calls[leg]()
                torch.cuda.synchronize()
                us[leg].append((time.perf_counter() - t0) / (a.launches * K) * 1e6)
        assert torch.equal(out["g"]["reward"], out["c"]["reward"])
        off_greedy = float((out["s"]["actions"] != out["g"]["actions"]).double().mean())   # (other trajectories: a rough share only)
        mean_prob = float(out["s"]["probs"].mean())
        # the stepped loop
        pt = envs["t"]
        W1, b1, W2, b2 = policy.W1[0].T.contiguous(), policy.b1[0], policy.W2[0].T.contiguous(), policy.b2[0]
        obs = pt.obs0

        def stepped(obs):
            for _ in range(K):
                p = torch.softmax(torch.relu(obs @ W1 + b1) @ W2 + b2, dim=1)
                ids = torch.multinomial(p, 1)
                prob = p.gather(1, ids)                   # noqa: F841  (what an on-policy method keeps beside the id)
                obs, _, _, _ = pt.step(ids[:, 0].to(torch.int32))
            return obs
        obs = stepped(obs)                                 # warm-up
        us["t"] = []
        for _ in range(a.stepped_blocks):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            obs = stepped(obs)
            torch.cuda.synchronize()
            us["t"].append((time.perf_counter() - t0) / K * 1e6)
        med = {leg: statistics.median(v) for leg, v in us.items()}
        lines += [f"layout {flags} ({arch}), discrete head  (n_in = {D}, n_out = {n_out}); (s): mean probability of the id taken "
                  f"{mean_prob:.3f}, {off_greedy:.3f} of its ids differ from the greedy run's",
                  f"    (g) greedy                         {fmt(us['g'])}",
                  f"    (x) epsilon-greedy, 0.25           {fmt(us['x'])}",
                  f"    (s) sampling, temperature 1, probs {fmt(us['s'])}",
                  f"    (c) sampling kernel, temperature 0 {fmt(us['c'])}",
                  f"    (t) stepped multinomial + step     {fmt(us['t'])}",
                  f"    (s)/(g) = {med['s'] / med['g']:.3f}   (s)/(x) = {med['s'] / med['x']:.3f}   (s) - (g) = {med['s'] - med['g']:.3f} us per step   "
                  f"(t)/(s) = {med['t'] / med['s']:.1f}"]
        for kernel, head in (("rollout_policy", ""), ("rollout_policy_head", ", 1"), ("rollout_policy_head", ", 2")):   # (greedy, HEAD_EXPLORE, HEAD_SAMPLE)
            name = f"mgx::{kernel}_episodes_kernel<{flags}, {4 if flags & 4 else 8}, 0{head}>"
            if name in usage:
                lines.append(f"#   {name}: {json.dumps(usage[name], sort_keys=True)}")
        results.append(dict(layout=flags, n_out=int(n_out), **{k: round(v, 4) for k, v in med.items()}))
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
