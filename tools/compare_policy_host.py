#!/usr/bin/env python
"""Compare the host statement of the policy rules (``pymgrid_amd.policy``: ``outputs``, ``act``, ``sample_weights``,
``ValueHead.value`` and the two ``*_host`` gradients) between two trees, bit for bit, on fixed seeded CPU inputs.

    python tools/compare_policy_host.py --record FILE [--root OLD_TREE]          # in (or pointed at) the tree to compare against
    python tools/compare_policy_host.py --check FILE [--out profiles/exp_policy_host_refactor.txt]

Every case calls the public functions only, so the same script runs in both trees.  ``--record`` stores every returned tensor;
``--check`` evaluates the cases again and compares each tensor with the stored one: dtype, shape, the positions of the NaNs, and
``torch.equal`` on the bits of everything else (so ``-0.0`` is not ``0.0``).  The cases: ``n_hidden`` in {0, 5, 16}; the discrete head
with ``n_out`` in {1, 4, 12} and the continuous one with 1, 3, 4 action columns; with and without a critic; a population whose
``policy_index`` has entries out of range (``outputs`` / ``act`` / ``sample_weights`` / ``value``); all five forms of ``act``; a ``scale``
ladder that contains 0; a sigma with a dead column; float32 rows; a mask, an all-zero mask, ``clip = inf``; a NaN and an inf among the
rows (a NaN in ``y``) and a NaN among the old densities.  Both gradients are taken with ``ratio=True, per_sample=True``, K * N = 201.
Prints one line per case, ``equal`` or the first differing entry; exits 1 if any differs."""
import argparse
import os
import sys

K, N = 3, 67
HIDDEN, DISCRETE_OUT, CONTINUOUS_OUT = (0, 5, 16), (1, 4, 12), (1, 3, 4)


def evaluate(root):
    """{case: {name: tensor or None}} of the tree at ``root``, in a fixed order."""
    sys.path.insert(0, os.path.abspath(root))
    import torch
    from pymgrid_amd.policy import (Exploration, GaussianSampling, MLPPolicy, Sampling, ValueHead, ppo_grad_gaussian_host,
                                    ppo_grad_host)
    F64 = torch.float64
    res = {}

    def named(prefix, value):
        if isinstance(value, dict):
            return {f"{prefix}.{k}": v for k, v in value.items()}
        if isinstance(value, tuple):
            return {f"{prefix}.{i}": v for i, v in enumerate(value)}
        return {prefix: value}

    for head, outs in (("discrete", DISCRETE_OUT), ("continuous", CONTINUOUS_OUT)):
        for nh in HIDDEN:
            for n_out in outs:
                n_in = 12 if n_out == 12 else 8
                g = torch.Generator().manual_seed(1000 * nh + 10 * n_out + (head == "continuous"))
                rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)     # noqa: E731
                n_mid = nh or n_in
                P = 3
                W1, b1 = (rn(P, nh, n_in) * 0.5, rn(P, nh) * 0.1) if nh else (None, None)
                W2, b2, w, b = rn(P, n_out, n_mid) * 0.5, rn(P, n_out) * 0.1, rn(P, n_mid) * 0.5, rn(P) * 0.1
                first = lambda t: None if t is None else t[0]     # noqa: E731
                one = MLPPolicy(first(W1), first(b1), W2[0], b2[0], head=head)
                index = (torch.arange(N, dtype=torch.int32) % (P + 2)) - 1            # -1 and P among them: set 0
                many = MLPPolicy(W1, b1, W2, b2, policy_index=index, head=head)
                critic, critics = ValueHead(w[0], b[0:1], head=head), ValueHead(w, b, head=head)
                scale = torch.rand(N, generator=g, dtype=F64) * 2.0
                scale[::9] = 0.0
                rows = torch.rand(K, N, n_in, generator=g, dtype=F64)
                rows_nan = rows.clone()
                rows_nan[1, 5, 2] = float("nan")
                rows_nan[2, 11, 0] = float("inf")
                rows32 = torch.rand(K, N, n_in, generator=g, dtype=F64).to(torch.float32)
                adv, ret = rn(K, N), rn(K, N)
                mask = torch.rand(K, N, generator=g) < 0.6
                sigma = [0.3, 0.0, 0.2, 0.1][:n_out] if n_out > 1 else 0.3              # (a dead column where there are several)
                for tag, pol, cr in (("one", one, critic), ("population", many, critics)):
                    c = {}
                    for rtag, obs in (("f64", rows[0]), ("nan", rows_nan[1]), ("inf", rows_nan[2]), ("f32", rows32[0])):
                        y = pol.outputs(obs)
                        c.update(named(f"{rtag}.outputs", y))
                        c.update(named(f"{rtag}.value", cr.value(pol, obs)))
                        c.update(named(f"{rtag}.act", pol.act(obs)))
                        if head == "discrete":
                            c.update(named(f"{rtag}.act_explore", pol.act(obs, Exploration(5, epsilon=0.4, scale=scale), 17)))
                            sa = Sampling(7, 0.8, scale=scale)
                            c.update(named(f"{rtag}.act_sample", pol.act(obs, sa, 17, return_prob=True)))
                            c.update(named(f"{rtag}.sample_weights", pol.sample_weights(y, sa)))
                            c.update(named(f"{rtag}.sample_weights_shared", pol.sample_weights(y, Sampling(7, 1.5))))
                        else:
                            c.update(named(f"{rtag}.act_explore", pol.act(obs, Exploration(5, sigma=sigma, scale=scale), 17)))
                            c.update(named(f"{rtag}.act_gaussian", pol.act(obs, GaussianSampling(7, sigma, scale=scale), 17,
                                                                           return_logp=True, return_raw=True)))
                            c.update(named(f"{rtag}.act_gaussian_shared", pol.act(obs, GaussianSampling(7, 0.25), 17, return_logp=True,
                                                                                  return_raw=True)))
                    res[f"{head} n_hidden={nh} n_out={n_out} {tag}: outputs, act, weights, value"] = c
                for ctag, cr in (("critic", critic), ("no critic", None)):
                    kw = dict(returns=ret if cr is not None else None, ratio=True, per_sample=True, ent_coef=0.01)
                    if head == "discrete":
                        sa = Sampling(7, 0.8, scale=scale)
                        ids = torch.randint(0, n_out, (K, N), generator=g).to(torch.uint8)
                        old = torch.rand(K, N, generator=g, dtype=F64) * 0.9 + 0.05
                        grad = lambda r, s=sa, o=old, **k: ppo_grad_host(one, cr, r, ids, o, adv, sampling=s, **{**kw, **k})     # noqa: E731
                        shared = Sampling(7, 1.5)
                    else:
                        sa = GaussianSampling(7, sigma, scale=scale)
                        raw = torch.rand(K, N, n_out, generator=g, dtype=F64) * 1.4 - 0.2
                        old = rn(K, N) * 0.5 - 1.0
                        grad = lambda r, s=sa, o=old, **k: ppo_grad_gaussian_host(one, cr, r, raw, o, adv, sampling=s, **{**kw, **k})     # noqa: E731
                        shared = GaussianSampling(7, 0.25)
                    old_nan = old.clone()
                    old_nan[0, 3] = float("nan")
                    c = {}
                    c.update(named("ladder", grad(rows)))
                    c.update(named("nan", grad(rows_nan, o=old_nan)))
                    c.update(named("nan_masked", grad(rows_nan, o=old_nan, mask=(rows_nan.sum(dim=2) + old_nan).isfinite())))
                    c.update(named("shared", grad(rows, s=shared)))
                    c.update(named("f32", grad(rows32)))
                    c.update(named("mask", grad(rows, mask=mask)))
                    c.update(named("mask_u8", grad(rows32, mask=mask.to(torch.uint8), ent_coef=0.0)))
                    c.update(named("mask_zero", grad(rows, mask=torch.zeros(K, N, dtype=torch.bool))))
                    c.update(named("clip_inf", grad(rows, clip=float("inf"))))
                    c.update(named("clip_0", grad(rows, clip=0.0, vf_coef=1.25)))
                    res[f"{head} n_hidden={nh} n_out={n_out} {ctag}: host gradient"] = c
    return res


def first_difference(name, old, new):
    """None where ``new`` is ``old`` bit for bit (NaNs: by position), else a line that names the first differing entry."""
    import torch
    if old is None or new is None:
        return None if old is None and new is None else f"{name}: {'None' if old is None else 'a tensor'} before, {'None' if new is None else 'a tensor'} now"
    if old.dtype != new.dtype or old.shape != new.shape:
        return f"{name}: {old.dtype} {list(old.shape)} before, {new.dtype} {list(new.shape)} now"
    a, b = old.reshape(-1), new.reshape(-1)
    if a.is_floating_point():
        na, nb = a != a, b != b
        bits = torch.int64 if a.dtype == torch.float64 else torch.int32
        zero = torch.zeros_like(a)
        bad = (na != nb) | (torch.where(na, zero, a).view(bits) != torch.where(nb, zero, b).view(bits))
    else:
        bad = a != b
    if not bool(bad.any()):
        return None
    at = int(bad.nonzero()[0])
    return f"{name}: {int(bad.sum())} of {a.numel()} entries differ, the first at flat index {at}: {a[at].item()!r} before, {b[at].item()!r} now"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    what = ap.add_mutually_exclusive_group(required=True)
    what.add_argument("--record", metavar="FILE")
    what.add_argument("--check", metavar="FILE")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree whose pymgrid_amd is evaluated")
    ap.add_argument("--out", default=None, help="--check: write the outcome here as well")
    a = ap.parse_args()
    got = evaluate(a.root)
    import torch
    if a.record:
        torch.save(got, a.record)
        print(f"recorded {len(got)} cases, {sum(len(c) for c in got.values())} tensors: {a.record}")
        return 0
    want = torch.load(a.check)
    lines = [f"# tools/compare_policy_host.py: {len(want)} cases, {sum(len(c) for c in want.values())} tensors, each against the tree "
             f"before the change; K * N = {K * N}; torch {torch.__version__}, CPU"]
    bad = 0
    for case in sorted(set(want) | set(got)):
        old, new = want.get(case), got.get(case)
        if old is None or new is None or list(old) != list(new):
            diffs = ["the case or its tensors' names differ"]
        else:
            diffs = [d for d in (first_difference(n, old[n], new[n]) for n in old) if d]
        nans = sum(int((t != t).sum()) for t in (new or {}).values() if t is not None and t.is_floating_point())
        lines.append(f"{case} ({len(new or ())} tensors, {nans} NaN entries): " + ("equal" if not diffs else f"{len(diffs)} tensors differ"))
        lines += ["    " + d for d in diffs[:3]]
        bad += bool(diffs)
    lines.append(f"# {len(want) - bad} of {len(want)} cases equal")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
