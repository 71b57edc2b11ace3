"""What a critic beside the actor costs inside the sampling launch (PerGridWindowEnv.rollout_policy with ``critic=`` / ``values=``,
mgx_rollout_policy_critic_episodes) and what the advantage kernel (``pymgrid_amd.gae``, mgx_gae) reaches -- profiles/exp_policy_critic.txt.

The workload of tools/exp_policy_sample.py: 100 000 generated grids of layout 7 (genset+battery+grid, 12 priority lists) and 3
(genset+battery, 4 lists), T = 8760, 168-step episodes, factorised series, no forecast horizon, K = 64, 16 hidden units.  Legs per
layout, us per env-step (one step of all grids):

    (s) sampling   rollout_policy with sampling=, probs=True: the sampling kernel, untouched
    (v) critic     rollout_policy with sampling=, probs=True, critic=, values=True: the critic kernel with its three value outputs
    (a) today      what a user does without it: the sampling launch with observations=True, final_observations=True (a1), the
                   same critic evaluated in torch on obs and on the final rows of the episodes that ended (a2, two matmuls), and
                   the backward advantage loop in torch (a3, gae_host) -- timed together, and each part in blocks of its own
    (g) mgx_gae    pymgrid_amd.gae alone on the outputs of (v), against gae_host alone (a3), with the bytes the rule moves
                   (25 + 8 with final_value in, 16 out per element, + 8 N) and the share of the 8 TB/s HBM peak they make; the calls
                   go round several copies of the arrays, larger together than the 256 MiB Infinity Cache

(s), (v) and (a) run in the same process on envs of their own and ALTERNATE block by block, so a drift of the box falls on all;
every leg is warmed up first.  A block = `--launches` launches of K steps (with what follows them in (a)) between two
torch.cuda.synchronize(); the median block and the spread (min .. max) are reported, with the resource figures of the forms timed.
No threshold is applied: the figures are the result.

    python tools/exp_policy_critic.py [--out profiles/exp_policy_critic.txt] [--grids 100000] [--K 64] [--repeats 7] [--root DIR]
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
    ap.add_argument("--launches", type=int, default=12, help="launches per timed block")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--gae-calls", type=int, default=48, help="mgx_gae calls per timed block of leg (g)")
    ap.add_argument("--gae-sets", type=int, default=4, help="copies of the inputs and outputs leg (g) takes in turn")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    import torch
    from pymgrid_amd import MLPPolicy, Sampling, ValueHead, _lib, gae
    from pymgrid_amd.generator import generate
    from pymgrid_amd.hetero import PerGridWindowEnv
    from pymgrid_amd.policy import gae_host
    _lib.build()
    dev = torch.device("cuda:0")
    N, K = a.grids, a.K
    F64 = torch.float64
    lines = [f"# tools/exp_policy_critic.py: {N} grids, T = {a.T}, {a.length}-step episodes, factorised, H = 0, K = {K}, "
             f"{a.hidden} hidden units; kernels {_lib.source_hash()}; {torch.cuda.get_device_name(0)}",
             f"# us per env-step: median of {a.repeats} blocks (min .. max); a block = {a.launches} launches of {K} steps; (s), (v), (a) alternate "
             f"block by block; every launch writes reward, done, ids, probs; (g): us per call, {a.gae_calls} calls per block over {a.gae_sets} "
             f"sets of inputs and outputs taken in turn"]

    def fmt(us):
        return f"{statistics.median(us):9.3f} ({min(us):.3f} .. {max(us):.3f})"

    def timed(fn, reps, per):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (reps * per) * 1e6

    results = []
    usage = _lib.resource_usage() or {}
    for arch, flags in (("genset+battery+grid", 7), ("genset+battery", 3)):
        envs = {}
        for leg in ("s", "v", "a"):
            pe = PerGridWindowEnv(generate(N, n_steps=a.T, seed=42, arch=arch, device=dev, series="factorised"),
                                  trajectory_length=a.length, discrete=True, auto_reset=True, seed=7)
            torch.manual_seed(41)                          # the same first draw of the episodes in every leg
            pe.obs0 = pe.reset()
            envs[leg] = pe
        D, n_out = envs["s"].env.engine.obs_dim, envs["s"].env.action_space.n
        rng = np.random.default_rng(3)
        policy = MLPPolicy(rng.normal(0, 1.5, size=(a.hidden, D)), rng.normal(0, 0.5, size=a.hidden),
                           rng.normal(0, 0.6, size=(n_out, a.hidden)), rng.normal(0.0, 0.5, size=n_out), head="discrete").to(dev)
        head = ValueHead(torch.as_tensor(rng.normal(0, 1.0, size=a.hidden)).to(dev), torch.as_tensor(rng.normal(0, 0.5, size=1)).to(dev))
        sa = Sampling(7, temperature=1.0)
        base = lambda: dict(reward=torch.empty(K, N, dtype=F64, device=dev), done=torch.empty(K, N, dtype=torch.uint8, device=dev),   # noqa: E731
                            actions=torch.empty(K, N, dtype=torch.uint8, device=dev), probs=torch.empty(K, N, dtype=F64, device=dev))
        out = {leg: base() for leg in envs}
        out["v"].update(values=torch.empty(K, N, dtype=F64, device=dev), final_values=torch.zeros(K, N, dtype=F64, device=dev),
                        last_value=torch.empty(N, dtype=F64, device=dev))
        out["a"].update(obs=torch.empty(K, N, D, dtype=F64, device=dev), final_obs=torch.zeros(K, N, D, dtype=F64, device=dev))
        want = dict(reward=True, done=True, actions=True, sampling=sa, probs=True)
        res = {}

        def leg_s():
            res["s"] = envs["s"].rollout_policy(policy, K, out=out["s"], **want)

        def leg_v():
            res["v"] = envs["v"].rollout_policy(policy, K, critic=head, values=True, out=out["v"], **want)

        def collect():                                     # (a1)
            res["a"] = envs["a"].rollout_policy(policy, K, observations=True, final_observations=True, out=out["a"], **want)

        W1, b1, w, b = policy.W1[0].T.contiguous(), policy.b1[0], head.w[0], head.b[0]
        first = {"obs": envs["a"].obs0}

        def critic_torch(x):
            return torch.relu(x @ W1 + b1) @ w + b

        def evaluate():                                    # (a2): V of the rows the ids were chosen on, of the last row, of the final rows
            r = res["a"]
            v_obs = critic_torch(r["obs"].view(K * N, D)).view(K, N)
            values = torch.cat([critic_torch(first["obs"])[None], v_obs[:-1]])
            finals = torch.zeros(K, N, dtype=F64, device=dev)
            finals[r["done"]] = critic_torch(r["final_obs"][r["done"]])
            res["a_values"] = (values, finals, v_obs[-1])

        def advantages():                                  # (a3)
            r = res["a"]
            values, finals, last = res["a_values"]
            res["a_gae"] = gae_host(r["reward"], r["done"], values, last, final_value=finals)

        def leg_a():
            collect()
            evaluate()
            advantages()
            first["obs"] = res["a"]["obs"][-1].clone()

        for fn in (leg_s, leg_v, leg_a):                   # warm-up: every kernel of the timed window
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        # the three envs walk the same trajectories: the critic changes nothing, and torch's matmul agrees with the rule to rounding
        assert torch.equal(res["s"]["reward"], res["v"]["reward"]) and torch.equal(res["s"]["probs"], res["v"]["probs"])
        assert torch.equal(res["s"]["reward"], res["a"]["reward"])
        err = float((res["a_values"][0] - res["v"]["values"]).abs().max())
        us = {leg: [] for leg in ("s", "v", "a", "a1", "a2", "a3", "g")}
        for _ in range(a.repeats):
            for leg, fn in (("s", leg_s), ("v", leg_v), ("a", leg_a)):
                us[leg].append(timed(fn, a.launches, K))
        for _ in range(a.repeats):                         # the parts of (a), each alone (on the outputs of the last launch)
            us["a1"].append(timed(collect, a.launches, K))
            us["a2"].append(timed(evaluate, a.launches, K))
            us["a3"].append(timed(advantages, a.launches, K))
        # (g): the advantage kernel alone on the outputs of (v)
        r = res["v"]
        d8 = r["done"].view(torch.uint8)
        # (copies of the inputs and outputs taken in turn, a.gae_sets x 314 MB at the default sizes: a call must not find what the call
        # before it read in the 256 MiB Infinity Cache, or the rate is not one of HBM)
        sets = [dict(args=tuple(t.clone() for t in (r["reward"], d8, r["values"], r["last_value"])), fv=r["final_values"].clone(),
                     out=dict(advantages=torch.empty(K, N, dtype=F64, device=dev), returns=torch.empty(K, N, dtype=F64, device=dev)))
                for _ in range(a.gae_sets)]
        turn = [0]

        def run_gae():
            q = sets[turn[0] % len(sets)]
            turn[0] += 1
            gae(*q["args"], final_value=q["fv"], out=q["out"])
        for _ in sets:
            run_gae()
        g_out = sets[0]["out"]
        ref = gae_host(r["reward"], r["done"], r["values"], r["last_value"], final_value=r["final_values"])
        assert torch.equal(g_out["advantages"], ref["advantages"]) and torch.equal(g_out["returns"], ref["returns"])
        for _ in range(a.repeats):
            us["g"].append(timed(run_gae, a.gae_calls, 1))
        g_us = statistics.median(us["g"])
        moved = K * N * (25 + 8 + 16) + 8 * N
        med = {leg: statistics.median(v) for leg, v in us.items()}
        lines += [f"layout {flags} ({arch}), discrete head  (n_in = {D}, n_out = {n_out}); done share {float(r['done'].double().mean()):.4f}; "
                  f"torch's matmul critic differs from the rule by at most {err:.2e}",
                  f"    (s) sampling launch, probs                      {fmt(us['s'])}",
                  f"    (v) critic launch, probs + three value outputs  {fmt(us['v'])}",
                  f"    (a) today: rows + torch critic + torch loop     {fmt(us['a'])}",
                  f"        (a1) sampling launch with obs + final_obs   {fmt(us['a1'])}",
                  f"        (a2) torch critic on obs / final rows       {fmt(us['a2'])}",
                  f"        (a3) torch advantage loop (gae_host)        {fmt(us['a3'])}",
                  f"    (v) - (s) = {med['v'] - med['s']:.3f} us per step   (v)/(s) = {med['v'] / med['s']:.3f}   (v)/(a1) = {med['v'] / med['a1']:.3f}   "
                  f"(a1 + a2)/(v) = {(med['a1'] + med['a2']) / med['v']:.2f}   (a)/((v) + (g)/K) = {med['a'] / (med['v'] + g_us / K):.2f}",
                  f"    (g) mgx_gae, [{K}, {N}] with final_value and returns: {fmt(us['g'])} us per call = {g_us / K:.3f} us per env-step; "
                  f"{moved / 1e6:.1f} MB moved, {moved / g_us / 1e6:.3f} TB/s = {moved / g_us / 1e6 / 8.0:.3f} of the 8 TB/s peak; "
                  f"the torch loop (a3) takes {med['a3'] * K:.1f} us per call: {med['a3'] * K / g_us:.1f}x"]
        for head in (2, 3):                                       # (HEAD_SAMPLE, HEAD_SAMPLE_CRITIC)
            name = f"mgx::rollout_policy_head_episodes_kernel<{flags}, {4 if flags & 4 else 8}, 0, {head}>"
            if name in usage:
                lines.append(f"#   {name}: {json.dumps(usage[name], sort_keys=True)}")
        if flags == 7:
            lines += [f"#   {name}: {json.dumps(u, sort_keys=True)}" for name, u in sorted(usage.items()) if "gae_kernel" in name]
        results.append(dict(layout=flags, n_out=int(n_out), g_us_per_call=round(g_us, 3), g_tb_s=round(moved / g_us / 1e6, 4),
                            **{k: round(v, 4) for k, v in med.items() if k != "g"}))
        for pe in envs.values():
            pe.env.close()
        del envs, out, res, g_out, ref, r, sets
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
