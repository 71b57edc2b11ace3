"""What the Gaussian head costs inside the fused continuous K-step (PerGridWindowEnv.step_k_policy with ``sampling=GaussianSampling``,
mgx_step_k_policy_gaussian_episodes), without and with a critic -- profiles/exp_policy_gaussian.txt.

The workload of tools/exp_policy_explore.py: 100 000 generated grids of one layout (7: genset+battery+grid, four controls; 3:
genset+battery, three), T = 8760, 168-step episodes, factorised series, no forecast horizon, K = 64, 16 hidden units.  Legs, us
per env-step (one step of all grids):

    (g) greedy     step_k_policy: the greedy kernel, untouched
    (x) exploring  step_k_policy with exploration=Exploration(sigma=...): the exploring kernel, untouched -- the yardstick, the same
                   code as before the Gaussian head existed
    (n) gaussian   step_k_policy with sampling=GaussianSampling, logp=True, raw_actions=True
    (v) + critic   the same with critic=, values=True: the CRITIC form with its three value outputs
    (t) stepped    what a user does without it: per step a torch policy with torch.randn noise, its log-density and a torch
                   critic (matmuls), then env.step -- K single steps per block

(g), (x), (n), (v) and (t) run in the same process on envs of their own and ALTERNATE block by block, so a drift of the box falls on
all; every leg is warmed up first.  A block = `--launches` launches of K steps between two torch.cuda.synchronize() ((t): one
"launch" of K single steps); the median block and the spread (min .. max) are reported, with the resource figures of the forms
timed.  Every launch writes reward, done and the controls taken.  No threshold is applied: the figures are the result.  Not
isolated: the share of the head's cost that is the draw (Philox + log + quarter turn) against the two extra streams -- (n) always
writes both.

    python tools/exp_policy_gaussian.py [--out FILE] [--append] [--layout 7] [--grids 100000] [--K 64] [--repeats 7] [--root DIR]

One layout per process: run it once per layout, each run under a timeout of its own, the second with --append.
"""
import argparse
import json
import os
import statistics
import sys
import time

ARCH = {7: "genset+battery+grid", 3: "genset+battery"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--layout", type=int, default=7, choices=sorted(ARCH))
    ap.add_argument("--grids", type=int, default=100_000)
    ap.add_argument("--T", type=int, default=8760)
    ap.add_argument("--length", type=int, default=168)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--launches", type=int, default=12, help="launches per timed block")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    import torch
    from pymgrid_amd import Exploration, GaussianSampling, MLPPolicy, ValueHead, _lib
    from pymgrid_amd.generator import generate
    from pymgrid_amd.hetero import PerGridWindowEnv
    _lib.build()
    dev = torch.device("cuda:0")
    N, K, flags = a.grids, a.K, a.layout
    F64 = torch.float64
    lines = []
    if not a.append:
        lines += [f"# tools/exp_policy_gaussian.py: {N} grids, T = {a.T}, {a.length}-step episodes, factorised, H = 0, K = {K}, "
                  f"{a.hidden} hidden units; kernels {_lib.source_hash()}; {torch.cuda.get_device_name(0)}",
                  f"# us per env-step: median of {a.repeats} blocks (min .. max); a block = {a.launches} launches of {K} steps ((t): {K} single "
                  f"steps); the legs alternate block by block; every launch writes reward, done and the controls taken"]

    def fmt(us):
        return f"{statistics.median(us):9.3f} ({min(us):.3f} .. {max(us):.3f})"

    def timed(fn, reps, per):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (reps * per) * 1e6

    usage = _lib.resource_usage() or {}
    envs = {}
    for leg in ("g", "x", "n", "v", "t"):
        pe = PerGridWindowEnv(generate(N, n_steps=a.T, seed=42, arch=ARCH[flags], device=dev, series="factorised"),
                              trajectory_length=a.length, discrete=False, auto_reset=True, seed=7)
        torch.manual_seed(41)                              # the same first draw of the episodes in every leg
        pe.obs0 = pe.reset()
        envs[leg] = pe
    e = envs["g"].env.engine
    D, A = e.obs_dim, e.action_dim
    rng = np.random.default_rng(3)
    policy = MLPPolicy(rng.normal(0, 1.5, size=(a.hidden, D)), rng.normal(0, 0.5, size=a.hidden),
                       rng.normal(0, 0.6, size=(A, a.hidden)), rng.normal(0.5, 0.5, size=A), head="continuous").to(dev)
    head = ValueHead(torch.as_tensor(rng.normal(0, 1.0, size=a.hidden)).to(dev), torch.as_tensor(rng.normal(0, 0.5, size=1)).to(dev), head="continuous")
    sigma = [0.3, 0.1, 0.2, 0.05][:A]
    ex, gs = Exploration(7, sigma=sigma), GaussianSampling(7, sigma)
    base = lambda: dict(reward=torch.empty(K, N, dtype=F64, device=dev), done=torch.empty(K, N, dtype=torch.uint8, device=dev),   # noqa: E731
                        actions=torch.empty(K, N, A, dtype=F64, device=dev))
    out = {leg: base() for leg in ("g", "x", "n", "v")}
    for leg in ("n", "v"):
        out[leg].update(logp=torch.empty(K, N, dtype=F64, device=dev), raw_actions=torch.empty(K, N, A, dtype=F64, device=dev))
    out["v"].update(values=torch.empty(K, N, dtype=F64, device=dev), final_values=torch.zeros(K, N, dtype=F64, device=dev),
                    last_value=torch.empty(N, dtype=F64, device=dev))
    want = dict(reward=True, done=True, actions=True)
    res = {}

    def leg_g():
        res["g"] = envs["g"].step_k_policy(policy, K, out=out["g"], **want)

    def leg_x():
        res["x"] = envs["x"].step_k_policy(policy, K, exploration=ex, out=out["x"], **want)

    def leg_n():
        res["n"] = envs["n"].step_k_policy(policy, K, sampling=gs, logp=True, raw_actions=True, out=out["n"], **want)

    def leg_v():
        res["v"] = envs["v"].step_k_policy(policy, K, sampling=gs, logp=True, raw_actions=True, critic=head, values=True, out=out["v"], **want)

    W1, b1, W2, b2 = policy.W1[0].T.contiguous(), policy.b1[0], policy.W2[0].T.contiguous(), policy.b2[0]
    w, b = head.w[0], head.b[0]
    sg = torch.as_tensor(sigma, dtype=F64, device=dev)
    log_norm = float(torch.log(sg).sum()) + 0.5 * A * float(np.log(2 * np.pi))
    state = {"obs": envs["t"].obs0}

    def leg_t():                                           # K single steps: torch policy + randn + log-density + torch critic, env.step
        obs = state["obs"]
        for _ in range(K):
            h = torch.relu(obs @ W1 + b1)
            z = torch.randn(N, A, dtype=F64, device=dev)
            raw = (h @ W2 + b2) + sg * z
            res["t"] = (-0.5 * (z * z).sum(dim=1) - log_norm, h @ w + b)
            obs = envs["t"].step(raw.clamp(0.0, 1.0), normalized=True)[0]
        state["obs"] = obs

    for fn in (leg_g, leg_x, leg_n, leg_v):                # warm-up: every kernel of the timed window
        for _ in range(3):
            fn()
    leg_t()
    torch.cuda.synchronize()
    # (n) and (v) walk the same trajectories: the critic changes nothing
    for name in ("reward", "actions", "logp", "raw_actions"):
        assert torch.equal(res["n"][name], res["v"][name]), name
    us = {leg: [] for leg in ("g", "x", "n", "v", "t")}
    for _ in range(a.repeats):
        for leg, fn in (("g", leg_g), ("x", leg_x), ("n", leg_n), ("v", leg_v)):
            us[leg].append(timed(fn, a.launches, K))
        us["t"].append(timed(leg_t, 1, K))
    med = {leg: statistics.median(v) for leg, v in us.items()}
    clipped = float(((res["n"]["raw_actions"] != res["n"]["actions"])).double().mean())
    lines += [f"layout {flags} ({ARCH[flags]}), continuous head  (n_in = {D}, n_out = {A}); done share "
              f"{float(res['n']['done'].double().mean()):.4f}; share of controls the clip moved {clipped:.3f}",
              f"    (g) greedy launch                                  {fmt(us['g'])}",
              f"    (x) exploring launch (twelve-uniform noise)        {fmt(us['x'])}",
              f"    (n) Gaussian launch, logp + raw actions            {fmt(us['n'])}",
              f"    (v) Gaussian launch + critic, three value outputs  {fmt(us['v'])}",
              f"    (t) stepped: torch policy + randn + critic + step  {fmt(us['t'])}",
              f"    (n) - (x) = {med['n'] - med['x']:.3f} us per step   (n)/(x) = {med['n'] / med['x']:.3f}   (v) - (n) = {med['v'] - med['n']:.3f}   "
              f"(t)/(n) = {med['t'] / med['n']:.1f}   (t)/(v) = {med['t'] / med['v']:.1f}"]
    ring = 4 if flags & 4 else 8
    for name in (f"mgx::step_k_policy_episodes_kernel<{flags}, {ring}, 0>", f"mgx::step_k_policy_head_episodes_kernel<{flags}, {ring}, 0, 1>",
                 f"mgx::step_k_policy_head_episodes_kernel<{flags}, {ring}, 0, 4>",      # (1, 4, 5: HEAD_EXPLORE, HEAD_GAUSSIAN,
                 f"mgx::step_k_policy_head_episodes_kernel<{flags}, {ring}, 0, 5>"):     # HEAD_GAUSSIAN_CRITIC)
        if name in usage:
            lines.append(f"#   {name}: {json.dumps(usage[name], sort_keys=True)}")
    lines.append("# " + json.dumps(dict(layout=flags, n_out=int(A), **{k: round(v, 4) for k, v in med.items()})))
    for pe in envs.values():
        pe.env.close()
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
