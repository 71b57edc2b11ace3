"""What the PPO / A2C gradient on the device costs (``pymgrid_amd.ppo_grad``, mgx_policy_grad) against torch autograd of the same
loss on the same tensors -- profiles/exp_policy_grad.txt.

The shapes of tools/exp_policy_critic.py: 100 000 grids, K = 64 (6.4 M samples), 16 hidden units, a critic; rows of layout 7
(n_in = 12, 12 priority lists) and of layout 3 (n_in = 8, 4 lists).  The data is synthetic -- uniform rows, random ids, old
probabilities round the current ones so that both sides of the clip occur: the cost of the call does not depend on where the rows
came from.  Legs, us per call:

    (d) ppo_grad       the call: policy_grad_kernel + policy_grad_finish_kernel, workspace allocation included
    (t) autograd       the loss in torch, fp64 (two matmuls, relu, log_softmax, the clipped surrogate, the value loss, the entropy),
                       forward + backward, the parameters as leaves; the same rows, ids, probabilities, advantages, returns

with the bytes the rule moves per call (per sample 8 n_in of rows, 1 of id, 8 each of old probability, advantage and return; the
workspace is small beside them) and the share of the 8 TB/s HBM peak they make.  (d) and (t) ALTERNATE block by block and are
warmed up first; a block = ``--calls`` calls between two torch.cuda.synchronize(); the median block and the spread (min .. max) are
reported.  The calls go round ``--sets`` copies of the inputs, each larger than the 256 MiB Infinity Cache.  The greatest
difference between the two gradients is reported relative to the greatest entry.  No threshold is applied: the figures are the result.

    python tools/exp_policy_grad.py [--out profiles/exp_policy_grad.txt] [--grids 100000] [--K 64] [--repeats 7] [--root DIR]
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
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--calls", type=int, default=6, help="calls per timed block")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sets", type=int, default=2, help="copies of the inputs the calls take in turn")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from pymgrid_amd import MLPPolicy, Sampling, ValueHead, _lib, ppo_grad, ppo_grad_flat
    _lib.build()
    dev = torch.device("cuda:0")
    N, K, nh = a.grids, a.K, a.hidden
    F64 = torch.float64
    clip, vf, ent, tau = 0.2, 0.5, 0.01, 1.0
    lines = [f"# tools/exp_policy_grad.py: {N} grids, K = {K} ({N * K} samples), {nh} hidden units, a critic, clip {clip}, vf_coef {vf}, "
             f"ent_coef {ent}; kernels {_lib.source_hash()}; {torch.cuda.get_device_name(0)}",
             f"# us per call: median of {a.repeats} blocks (min .. max); a block = {a.calls} calls over {a.sets} sets of inputs taken in turn; "
             "(d) and (t) alternate block by block"]
    usage = _lib.resource_usage() or {}
    summary = []

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for q in range(a.calls):
            fn(q % a.sets)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.calls * 1e6

    for layout, n_in, n_out in ((7, 12, 12), (3, 8, 4)):
        g = torch.Generator(device=dev).manual_seed(layout)
        rn = lambda *s: torch.randn(*s, generator=g, dtype=F64, device=dev)     # noqa: E731
        W1, b1, W2, b2 = rn(nh, n_in) * 0.5, rn(nh) * 0.1, rn(n_out, nh) * 0.5, rn(n_out) * 0.1
        w, b = rn(nh) * 0.5, rn(1) * 0.1
        policy, head, sa = MLPPolicy(W1, b1, W2, b2), ValueHead(w, b), Sampling(7, tau)
        sets = []
        for _ in range(a.sets):
            rows = torch.rand(K, N, n_in, generator=g, dtype=F64, device=dev)
            ids = torch.randint(0, n_out, (K, N), generator=g, device=dev).to(torch.uint8)
            adv, ret = rn(K, N), rn(K, N)
            cur = ppo_grad(policy, None, rows, ids, torch.ones(K, N, dtype=F64, device=dev), adv, sampling=sa, ratio=True)["ratio"]
            sets.append((rows, ids, cur * torch.exp(0.3 * rn(K, N)), adv, ret))
        params = [t.clone().requires_grad_(True) for t in (W1, b1, W2, b2, w, b)]

        def device_leg(q):
            rows, ids, old, adv, ret = sets[q]
            return ppo_grad(policy, head, rows, ids, old, adv, returns=ret, sampling=sa, clip=clip, vf_coef=vf, ent_coef=ent)

        def autograd_leg(q):
            rows, ids, old, adv, ret = sets[q]
            for p in params:
                p.grad = None
            pW1, pb1, pW2, pb2, pw, pb = params
            x = rows.reshape(-1, n_in)
            h = torch.relu(torch.addmm(pb1, x, pW1.t()))
            logp = torch.log_softmax(torch.addmm(pb2, h, pW2.t()) / tau, dim=1)
            rho = torch.exp(logp.gather(1, ids.reshape(-1, 1).long())[:, 0]) / old.reshape(-1)
            A = adv.reshape(-1)
            pl = -torch.minimum(rho * A, torch.clamp(rho, 1.0 - clip, 1.0 + clip) * A)
            H = -(torch.exp(logp) * logp).sum(dim=1)
            vl = 0.5 * (torch.addmv(pb.expand(x.shape[0]), h, pw) - ret.reshape(-1)) ** 2
            (pl.mean() + vf * vl.mean() - ent * H.mean()).backward()
            return torch.cat([p.grad.reshape(-1) for p in params])

        got, ref = ppo_grad_flat(device_leg(0)), autograd_leg(0)
        diff = float((got - ref).abs().max() / ref.abs().max())
        for _ in range(2):
            timed(device_leg), timed(autograd_leg)
        d, t = [], []
        for _ in range(a.repeats):
            d.append(timed(device_leg))
            t.append(timed(autograd_leg))
        fmt = lambda v: f"{statistics.median(v):10.1f} ({min(v):.1f} .. {max(v):.1f})"     # noqa: E731
        md, mt = statistics.median(d), statistics.median(t)
        moved = N * K * (8 * n_in + 1 + 8 * 3)
        tbs = moved / md / 1e6
        lines += [f"layout {layout} rows  (n_in = {n_in}, n_out = {n_out}); the two gradients differ by at most {diff:.2e} of the greatest entry",
                  f"    (d) ppo_grad                         {fmt(d)}",
                  f"    (t) torch autograd, fp64             {fmt(t)}",
                  f"    (t)/(d) = {mt / md:.2f}   {moved / 1e6:.1f} MB moved per call, {tbs:.3f} TB/s = "
                  f"{tbs / 8.0:.3f} of the 8 TB/s peak"]
        for name in sorted(usage):
            if f"policy_grad_kernel<{n_in}, true, 0>" in name or "policy_grad_finish_kernel" in name:
                lines.append(f"#   {name}: {json.dumps(usage[name], sort_keys=True)}")
        summary.append(dict(layout=layout, n_in=n_in, n_out=n_out, d=round(md, 1), t=round(mt, 1), tb_s=round(tbs, 4),
                            diff=diff))
        del sets, params
        torch.cuda.empty_cache()
    lines.append("# " + json.dumps(summary))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
