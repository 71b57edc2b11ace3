"""Timing of CEM planning on the device (PerGridWindowEnv.lookahead_gaussian / cem_refit: mgx_lookahead_gaussian_episodes /
mgx_cem_refit, CEMPlanner) -- profiles/exp_cem.txt.  One process, four parts:

  (a) the launch that draws its candidates in registers against the other route to the same kind of numbers: torch draws + clamp
      into a plan tensor [C, H, N, A], then the per-grid what-if launch (PerGridWindowEnv.lookahead) -- both parts of that route
      timed, and the peak device memory of either route.  hipEvent pairs around windows of repeated launches; 100 000 generated
      grids, factorised series, H = 24.
  (b) cem_refit against the torch route over that plan tensor (topk, gather, mean / std).
  (c) CEMPlanner(64 candidates, 8 elites, 3 iterations) per env-step.
  (d) control quality, once: the return of CEMPlanner and of ShootingMPC with as many uniformly drawn candidates per step, over one
      pass of the packaged pymgrid25 scenarios with continuous controls, per scenario.
  (p) a probe for a counter run: a few launches of (a)'s C = 64 form and nothing else.

    python tools/exp_cem.py [--out profiles/exp_cem.txt] [--grids 100000] [--parts abcd]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp_cem.txt"))
    ap.add_argument("--grids", type=int, default=100_000)
    ap.add_argument("--T", type=int, default=8760)
    ap.add_argument("--length", type=int, default=168)
    ap.add_argument("--H", type=int, default=24)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of launches per timed window")
    ap.add_argument("--parts", default="abcd")
    ap.add_argument("--quality-steps", type=int, default=0, help="steps of part (d); 0: the scenarios' whole series")
    a = ap.parse_args()
    import torch
    from pymgrid_amd import CEMPlanner, ShootingMPC, _lib
    from pymgrid_amd.generator import generate
    from pymgrid_amd.hetero import PerGridWindowEnv
    _lib.build()
    if not torch.cuda.is_available():
        raise SystemExit("exp_cem measures on the GPU: none is visible")
    dev = torch.device("cuda:0")
    N, H, F64 = a.grids, a.H, torch.float64
    lines = [f"exp_cem: {N} grids, T = {a.T}, episodes of {a.length}, H = {H}, kernels {_lib.source_hash()}, "
             f"{torch.cuda.get_device_name(0)}", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def event_ms(fn):
        """Median and minimum of five windows of repeated calls, hipEvent pairs around each window: ms per call."""
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        reps = int(min(400, max(5, a.window / max(time.perf_counter() - t0, 1e-6))))
        per = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            per.append(e0.elapsed_time(e1) / reps)
        per.sort()
        return per[2], per[0]

    def peak_gb(fn):
        """Peak device memory of one call above what is allocated before it, GB."""
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - before) / 1e9

    def env_of(arch):
        batch = generate(N, n_steps=a.T, seed=42, arch=arch, device=dev, series="factorised")
        pe = PerGridWindowEnv(batch, trajectory_length=a.length, discrete=False, auto_reset=True, seed=7, observations=False)
        pe.reset()
        A = pe.env.engine.action_dim
        mean = torch.full((H, N, A), 0.5, dtype=F64, device=dev)
        sigma = torch.full((H, N, A), 0.3, dtype=F64, device=dev)
        return pe, A, mean, sigma

    def torch_plans(mean, sigma, C):
        """The plan tensor the torch route needs before every launch: normal draws round the mean, clamped."""
        return torch.randn((C,) + tuple(mean.shape), dtype=F64, device=dev).mul_(sigma).add_(mean).clamp_(0.0, 1.0)

    if "p" in a.parts:
        pe, A, mean, sigma = env_of("genset+battery+grid")
        out = {"ret": torch.empty(64, N, dtype=F64, device=dev), "steps": torch.empty(N, dtype=torch.int32, device=dev)}
        for _ in range(3):
            pe.lookahead_gaussian(mean, sigma, 64, 1, pick=False, out=out)
        torch.cuda.synchronize()
        print(f"probe: 3 launches, C = 64, {N} grids, H = {H}; mean + sigma are {2 * mean.numel() * 8 / 1e6:.0f} MB")
        return

    if "a" in a.parts:
        say("(a) lookahead_gaussian against torch draws + clamp into [C, H, N, A], then the per-grid launch")
        say("    (ms per call: median of 5 windows [min], hipEvent pairs; peak: device memory of one call above the resident set, GB)")
        say(f"{'arch':22s}{'C':>4s}{'lookahead_gaussian':>22s}{'peak':>8s}{'torch draws':>20s}{'per-grid launch':>20s}{'route':>10s}{'peak':>8s}"
            f"{'ratio':>8s}")
        for arch in ("genset+battery+grid", "genset+battery"):
            pe, A, mean, sigma = env_of(arch)
            for C in (8, 64):
                out = {"ret": torch.empty(C, N, dtype=F64, device=dev), "steps": torch.empty(N, dtype=torch.int32, device=dev)}
                cem = event_ms(lambda: pe.lookahead_gaussian(mean, sigma, C, 1, pick=False, out=out))
                cem_peak = peak_gb(lambda: pe.lookahead_gaussian(mean, sigma, C, 1, pick=False, out=out))
                draw = event_ms(lambda: torch_plans(mean, sigma, C))
                plans = torch_plans(mean, sigma, C)
                launch = event_ms(lambda: pe.lookahead(plans, pick=False, out=out))
                del plans
                route_peak = peak_gb(lambda: pe.lookahead(torch_plans(mean, sigma, C), pick=False, out=out))
                route = draw[0] + launch[0]
                say(f"{arch:22s}{C:4d}{cem[0]:14.3f} [{cem[1]:6.3f}]{cem_peak:8.3f}{draw[0]:12.3f} [{draw[1]:6.3f}]{launch[0]:12.3f} [{launch[1]:6.3f}]"
                    f"{route:10.3f}{route_peak:8.3f}{cem[0] / route:8.3f}")
            pe.env.close()
            del pe, mean, sigma
            torch.cuda.empty_cache()
        usage = _lib.resource_usage() or {}
        forms = sorted((n, u) for n, u in usage.items() if "lookahead_gaussian_episodes_kernel" in n)
        if forms:
            say("    lookahead_gaussian_episodes_kernel<F, U, UA, SRC> (-Rpass-analysis=kernel-resource-usage): VGPRs, waves/SIMD, scratch bytes,")
            say("    scalar registers parked in vector lanes")
            for n, u in forms:
                say(f"        {n.split('::')[-1]:50s}{u.get('vgpr', 0):5d}{u.get('occupancy', 0):4d}{u.get('scratch', 0):4d}{u.get('sgpr_spill', 0):4d}")
        say()

    if "b" in a.parts:
        say("(b) cem_refit (elites + refit, regenerating the elites' controls) against torch over the plan tensor: topk, gather, mean / std")
        say(f"{'arch':22s}{'C':>4s}{'E':>4s}{'cem_refit':>20s}{'peak':>8s}{'torch route':>20s}{'peak':>8s}")
        for arch in ("genset+battery+grid", "genset+battery"):
            pe, A, mean, sigma = env_of(arch)
            for C, E in ((8, 2), (64, 8)):
                la = pe.lookahead_gaussian(mean, sigma, C, 1, pick=False)
                outs = {"mean": torch.empty_like(mean), "sigma": torch.empty_like(sigma), "elite": torch.empty(E, N, dtype=torch.int32, device=dev)}

                def refit():
                    pe.cem_refit(la["ret"], la["steps"], mean, sigma, 1, E, sigma_min=0.01, best_plan=False, out=outs)
                plans = torch_plans(mean, sigma, C)

                def torch_refit():
                    idx = la["ret"].topk(E, dim=0).indices
                    el = plans.gather(0, idx[:, None, :, None].expand(E, H, N, A))
                    return el.mean(dim=0), el.std(dim=0, unbiased=False).clamp_(min=0.01)
                t_dev, t_torch = event_ms(refit), event_ms(torch_refit)
                say(f"{arch:22s}{C:4d}{E:4d}{t_dev[0]:12.3f} [{t_dev[1]:6.3f}]{peak_gb(refit):8.3f}{t_torch[0]:12.3f} [{t_torch[1]:6.3f}]"
                    f"{peak_gb(torch_refit):8.3f}   (+ the plan tensor, {plans.numel() * 8 / 1e9:.3f} GB)")
                del plans
            pe.env.close()
            del pe, mean, sigma
            torch.cuda.empty_cache()
        say()

    if "c" in a.parts:
        say("(c) CEMPlanner(64 candidates, 8 elites, 3 iterations: 4 launches + 3 refits + 1 step), us per env-step")
        say("    (host clock around a synchronised window)")
        for arch in ("genset+battery+grid", "genset+battery"):
            pe, A, mean, sigma = env_of(arch)
            m = CEMPlanner(pe, H, n_candidates=64, n_elite=8, n_iters=3, seed=1)
            m.run(3, reward=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter(); m.run(10, reward=False); torch.cuda.synchronize()
            say(f"    {arch:24s}{(time.perf_counter() - t0) / 10 * 1e6:12.1f}")
            pe.env.close()
            del pe, mean, sigma, m
            torch.cuda.empty_cache()
        say()

    if "d" in a.parts:
        from pymgrid_amd import MicrogridBatch
        from pymgrid_amd.scenario import bucket_by_layout, load_npz_grids
        grids = load_npz_grids(os.path.join(ROOT, "pymgrid_amd", "data", "pymgrid25.npz"))
        say("(d) return over one pass of the packaged pymgrid25 scenarios, continuous controls, H = 24, per scenario: CEMPlanner(64, 8, 3:")
        say("    256 candidates a step) and ShootingMPC(n_random=256: as many, uniform in [0, 1]^A, shared by the grids).  Measured once.")
        say(f"{'scenario':>9s}{'layout':>24s}{'steps':>7s}{'ShootingMPC':>20s}{'CEMPlanner':>20s}{'CEM - shooting':>16s}")
        tot = [0.0, 0.0, 0]
        for idx in bucket_by_layout(grids).values():
            try:
                sub = [grids[n] for n in idx]
                steps = sub[0]["final_step"] - sub[0]["initial_step"]
                run = a.quality_steps or steps
                rets = []
                for who in ("shooting", "cem"):
                    batch = MicrogridBatch.from_grids(sub, device=dev)
                    if batch.layout.multi:
                        raise ValueError("several modules of a kind")
                    pe = PerGridWindowEnv(batch, trajectory_length=steps, discrete=False, auto_reset=True, seed=7, observations=False)
                    pe.reset()
                    m = ShootingMPC(pe, H, n_random=256, seed=1) if who == "shooting" else CEMPlanner(pe, H, 64, 8, 3, seed=1)
                    rets.append(m.run(run, reward=True)["reward"].sum(dim=0).cpu())
                    L = batch.layout
                    name = "+".join(k for k, has in (("genset", L.has_genset), ("battery", L.has_battery), ("grid", L.has_grid)) if has)
                    pe.env.close()
                for j, n in enumerate(idx):
                    say(f"{n:9d}{name:>24s}{run:7d}{float(rets[0][j]):20.1f}{float(rets[1][j]):20.1f}{float(rets[1][j] - rets[0][j]):16.1f}")
                    tot[0] += float(rets[0][j]); tot[1] += float(rets[1][j]); tot[2] += 1
            except Exception as exc:              # a layout the episode launches do not take: say so and go on
                say(f"    scenarios {list(idx)}: not run ({type(exc).__name__}: {exc})")
        if tot[2]:
            say(f"{'mean':>9s}{'':24s}{'':7s}{tot[0] / tot[2]:20.1f}{tot[1] / tot[2]:20.1f}{(tot[1] - tot[0]) / tot[2]:16.1f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
