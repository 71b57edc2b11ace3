"""What the PPO / A2C gradient of the Gaussian head costs on the device (``pymgrid_amd.ppo_grad_gaussian``, mgx_policy_grad_gaussian)
against torch autograd of the same loss on the same tensors, and against the discrete ``ppo_grad`` with four outputs at the same row
width in the same session -- profiles/exp_policy_grad_gaussian.txt.

The shapes of tools/exp_policy_grad.py: 100 000 grids, K = 64 (6.4 M samples), 16 hidden units; rows of layout 7 (n_in = 12, the
four controls) and of a three-control layout (n_in = 10: genset + grid), each with and without the critic.  The data is synthetic --
uniform rows, raw = y + s * z with z normal, old log-probabilities round the current ones so that both sides of the clip occur: the
cost of the call does not depend on where the rows came from.  Legs, us per call:

    (g) ppo_grad_gaussian  the call: policy_grad_kernel (Gaussian head) + policy_grad_finish_kernel, workspace allocation included
    (d) ppo_grad           the discrete call with FOUR outputs on the same rows, advantages and returns (random ids)
    (t) autograd           the loss in torch, fp64 (two matmuls, relu, the closed-form density and entropy, the clipped surrogate,
                           the value loss), forward + backward, the parameters and log sigma as leaves; the same tensors as (g)

with the bytes the rule moves per call (per sample 8 n_in of rows, 8 A of raw actions, 8 each of old log-probability, advantage and
return) and the share of the 8 TB/s HBM peak they make.  (g), (d) and (t) ALTERNATE block by block and are warmed up first; a block =
``--calls`` calls between two torch.cuda.synchronize(); the median block and the spread (min .. max) are reported.  The calls go
round ``--sets`` copies of the inputs, each larger than the 256 MiB Infinity Cache.  The greatest difference between the gradients of
(g) and (t) is reported relative to the greatest entry.  No threshold is applied: the figures are the result.

    python tools/exp_policy_grad_gaussian.py [--out profiles/exp_policy_grad_gaussian.txt] [--grids 100000] [--K 64] [--repeats 7]
"""
import argparse
import json
import math
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
    ap.add_argument("--autograd-repeats", type=int, default=3, help="timed blocks of the autograd leg (seconds each)")
    ap.add_argument("--sets", type=int, default=2, help="copies of the inputs the calls take in turn")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from pymgrid_amd import (GaussianSampling, MLPPolicy, Sampling, ValueHead, _lib, ppo_grad, ppo_grad_flat, ppo_grad_gaussian)
    _lib.build()
    dev = torch.device("cuda:0")
    N, K, nh = a.grids, a.K, a.hidden
    F64 = torch.float64
    clip, vf, ent = 0.2, 0.5, 0.01
    sigma = [0.3, 0.1, 0.2, 0.05]
    lines = [f"# tools/exp_policy_grad_gaussian.py: {N} grids, K = {K} ({N * K} samples), {nh} hidden units, clip {clip}, vf_coef {vf}, "
             f"ent_coef {ent}, sigma {sigma}; kernels {_lib.source_hash()}; {torch.cuda.get_device_name(0)}",
             f"# us per call: median of {a.repeats} blocks ({a.autograd_repeats} for (t)) (min .. max); a block = {a.calls} calls over "
             f"{a.sets} sets of inputs taken in turn; (g), (d) and (t) alternate block by block"]
    usage = _lib.resource_usage() or {}
    summary = []

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for q in range(a.calls):
            fn(q % a.sets)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.calls * 1e6

    for name, n_in, A in (("layout 7 rows, four controls", 12, 4), ("genset + grid rows, three controls", 10, 3)):
        for with_critic in (True, False):
            g = torch.Generator(device=dev).manual_seed(n_in + with_critic)
            rn = lambda *s: torch.randn(*s, generator=g, dtype=F64, device=dev)     # noqa: E731
            W1, b1, W2, b2 = rn(nh, n_in) * 0.5, rn(nh) * 0.1, rn(A, nh) * 0.5, rn(A) * 0.1
            w, b = rn(nh) * 0.5, rn(1) * 0.1
            policy = MLPPolicy(W1, b1, W2, b2, head="continuous")
            head = ValueHead(w, b, head="continuous") if with_critic else None
            gs = GaussianSampling(7, sigma[:A])
            W2d, b2d = rn(4, nh) * 0.5, rn(4) * 0.1                                   # the discrete twin: four outputs, the same trunk
            dpolicy, dhead, sa = MLPPolicy(W1, b1, W2d, b2d), (ValueHead(w, b) if with_critic else None), Sampling(7, 1.0)
            s = torch.tensor(sigma[:A], dtype=F64, device=dev)
            sets = []
            for _ in range(a.sets):
                rows = torch.rand(K, N, n_in, generator=g, dtype=F64, device=dev)
                y = policy.outputs(rows.reshape(K * N, n_in)).reshape(K, N, A)
                z = rn(K, N, A)
                raw = (y + s * z).contiguous()
                logp = (-0.5 * z * z - torch.log(s) - 0.5 * math.log(2 * math.pi)).sum(dim=2)
                adv, ret = rn(K, N), (rn(K, N) if with_critic else None)
                ids = torch.randint(0, 4, (K, N), generator=g, device=dev).to(torch.uint8)
                cur = ppo_grad(dpolicy, None, rows, ids, torch.ones(K, N, dtype=F64, device=dev), adv, sampling=sa, ratio=True)["ratio"]
                sets.append((rows, raw, logp + 0.3 * rn(K, N), adv, ret, ids, cur * torch.exp(0.3 * rn(K, N))))
                del y, z
            leaves = [W1, b1, W2, b2] + ([w, b] if with_critic else []) + [torch.log(s)]
            params = [t.clone().requires_grad_(True) for t in leaves]

            def gaussian_leg(q):
                rows, raw, old, adv, ret, _, _ = sets[q]
                return ppo_grad_gaussian(policy, head, rows, raw, old, adv, returns=ret, sampling=gs, clip=clip, vf_coef=vf, ent_coef=ent)

            def discrete_leg(q):
                rows, _, _, adv, ret, ids, oldp = sets[q]
                return ppo_grad(dpolicy, dhead, rows, ids, oldp, adv, returns=ret, sampling=sa, clip=clip, vf_coef=vf, ent_coef=ent)

            def autograd_leg(q):
                rows, raw, old, adv, ret, _, _ = sets[q]
                for p in params:
                    p.grad = None
                pW1, pb1, pW2, pb2 = params[:4]
                pls = params[-1]
                x = rows.reshape(-1, n_in)
                h = torch.relu(torch.addmm(pb1, x, pW1.t()))
                yy = torch.addmm(pb2, h, pW2.t())
                sg = torch.exp(pls)
                lp = (-0.5 * ((raw.reshape(-1, A) - yy) / sg) ** 2 - pls - 0.5 * math.log(2 * math.pi)).sum(dim=1)
                rho = torch.exp(lp - old.reshape(-1))
                Adv = adv.reshape(-1)
                pl = -torch.minimum(rho * Adv, torch.clamp(rho, 1.0 - clip, 1.0 + clip) * Adv)
                H = (pls + 0.5 + 0.5 * math.log(2 * math.pi)).sum()
                loss = pl.mean() - ent * H
                if with_critic:
                    pw, pb = params[4], params[5]
                    loss = loss + vf * (0.5 * (torch.addmv(pb.expand(x.shape[0]), h, pw) - ret.reshape(-1)) ** 2).mean()
                loss.backward()
                return torch.cat([p.grad.reshape(-1) for p in params])

            got, ref = ppo_grad_flat(gaussian_leg(0)), autograd_leg(0)
            diff = float((got[:ref.numel()] - ref).abs().max() / ref.abs().max())
            for _ in range(2):
                timed(gaussian_leg), timed(discrete_leg)
            timed(autograd_leg)
            gl, dl, tl = [], [], []
            for r in range(a.repeats):
                gl.append(timed(gaussian_leg))
                dl.append(timed(discrete_leg))
                if r < a.autograd_repeats:
                    tl.append(timed(autograd_leg))
            fmt = lambda v: f"{statistics.median(v):10.1f} ({min(v):.1f} .. {max(v):.1f})"     # noqa: E731
            mg, md, mt = statistics.median(gl), statistics.median(dl), statistics.median(tl)
            moved = N * K * (8 * n_in + 8 * A + 8 * (3 if with_critic else 2))
            tbs = moved / mg / 1e6
            lines += [f"{name} (n_in = {n_in}, A = {A}), {'a critic' if with_critic else 'no critic'}; the gradients of (g) and (t) differ "
                      f"by at most {diff:.2e} of the greatest entry",
                      f"    (g) ppo_grad_gaussian                {fmt(gl)}",
                      f"    (d) ppo_grad, four outputs           {fmt(dl)}",
                      f"    (t) torch autograd, fp64             {fmt(tl)}",
                      f"    (g)/(d) = {mg / md:.3f}   (t)/(g) = {mt / mg:.1f}   {moved / 1e6:.1f} MB moved per call, {tbs:.3f} TB/s = "
                      f"{tbs / 8.0:.3f} of the 8 TB/s peak"]
            crit = "true" if with_critic else "false"
            for kname in sorted(usage):
                if f"policy_grad_kernel<{n_in}, {crit}, " in kname:
                    lines.append(f"#   {kname}: {json.dumps(usage[kname], sort_keys=True)}")
            summary.append(dict(rows=name, n_in=n_in, A=A, critic=with_critic, g=round(mg, 1), d=round(md, 1), t=round(mt, 1),
                                g_over_d=round(mg / md, 3), tb_s=round(tbs, 4), diff=diff))
            del sets, params
            torch.cuda.empty_cache()
    for kname in sorted(usage):
        if "policy_grad_finish_kernel" in kname:
            lines.append(f"#   {kname}: {json.dumps(usage[kname], sort_keys=True)}")
    lines.append("# " + json.dumps(summary))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
