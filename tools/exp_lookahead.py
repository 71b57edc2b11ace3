"""Timing of the what-if launches (PerGridWindowEnv.lookahead: mgx_lookahead_episodes / mgx_lookahead_step_k_episodes) and of
ShootingMPC -- profiles/exp_lookahead.txt.  One process, three parts:

  (a) the lookahead launch (shared and per-grid plans; discrete and continuous) against the only other way to the same numbers: C
      launches of rollout(K=H, reward=True) / step_k on C cloned envs -- timed here as C x one such launch, in the same process.
      hipEvent pairs around windows of repeated launches; 100 000 generated grids, factorised series, H = 24.
  (b) ShootingMPC.run per env-step beside RuleBasedControl.run_episodes per env-step.
  (c) control quality, once: the return of ShootingMPC(H = 24, constant plans + 32 random) and of RuleBasedControl over one pass of
      the packaged pymgrid25 scenarios (the layouts with one module of every kind), per scenario.

    python tools/exp_lookahead.py [--out profiles/exp_lookahead.txt] [--grids 100000] [--parts abc]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp_lookahead.txt"))
    ap.add_argument("--grids", type=int, default=100_000)
    ap.add_argument("--T", type=int, default=8760)
    ap.add_argument("--length", type=int, default=168)
    ap.add_argument("--H", type=int, default=24)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of launches per timed window")
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--quality-steps", type=int, default=0, help="steps of part (c); 0: the scenarios' whole series")
    a = ap.parse_args()
    import torch
    from pymgrid_amd import RuleBasedControl, ShootingMPC, _lib
    from pymgrid_amd.generator import generate
    from pymgrid_amd.hetero import PerGridWindowEnv
    _lib.build()
    if not torch.cuda.is_available():
        raise SystemExit("exp_lookahead measures on the GPU: none is visible")
    dev = torch.device("cuda:0")
    N, H = a.grids, a.H
    lines = [f"exp_lookahead: {N} grids, T = {a.T}, episodes of {a.length}, H = {H}, kernels {_lib.source_hash()}, "
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
        return per[2], per[0], reps

    def needed_bytes(batch, C, plan_bytes):
        """What the rule must move once: every grid's own columns and H series rows, the plans, ret [C, N]."""
        cols = sum(t.element_size() for t in batch.cols.values() if t is not None and t.dim() == 1 and t.shape[0] == N)
        row = 16 + (8 + 1 if batch.layout.has_grid else 0)         # factorised: load + pv (+ co2, an outage word per 64 rows)
        return N * (cols + H * row) + plan_bytes + C * N * 8

    if "a" in a.parts:
        say("(a) one lookahead launch against C roll-out launches (ms per launch: median of 5 windows [min]; hipEvent pairs)")
        say(f"{'arch':22s}{'kind':12s}{'plans':10s}{'C':>4s}{'lookahead':>20s}{'one rollout':>20s}{'C x rollout':>13s}{'ratio':>8s}"
            f"{'lane-steps/s':>14s}{'needed GB/s':>13s}")
        for arch in ("genset+battery+grid", "genset+battery"):
            for discrete in (True, False):
                batch = generate(N, n_steps=a.T, seed=42, arch=arch, device=dev, series="factorised")
                pe = PerGridWindowEnv(batch, trajectory_length=a.length, discrete=discrete, auto_reset=True, seed=7, observations=False)
                pe.reset()
                e = pe.env.engine
                A = e.action_dim
                g = torch.Generator(device=dev); g.manual_seed(5)
                n_lists = pe.env.action_space.n if discrete else 0
                out_r = {"reward": torch.empty(H, N, dtype=torch.float64, device=dev)}
                if discrete:
                    ids = torch.randint(0, n_lists, (H, N), device=dev, generator=g).to(torch.uint8)
                    base = event_ms(lambda: pe.rollout(ids, reward=True, out=out_r))
                else:
                    acts = torch.rand(H, N, A, device=dev, generator=g, dtype=torch.float64)
                    base = event_ms(lambda: pe.step_k(acts, reward=True, out=out_r))
                for C in sorted({n_lists or 8, 64}):
                    for per_grid in (False, True):
                        if discrete:
                            plans = torch.randint(0, n_lists, (C, H, N) if per_grid else (C, H), device=dev, generator=g).to(torch.uint8)
                        else:
                            plans = torch.rand((C, H, N, A) if per_grid else (C, H, A), device=dev, generator=g, dtype=torch.float64)
                        out = {"ret": torch.empty(C, N, dtype=torch.float64, device=dev), "steps": torch.empty(N, dtype=torch.int32, device=dev)}
                        med, low, reps = event_ms(lambda: pe.lookahead(plans, pick=False, out=out))
                        steps = float(out["steps"].double().mean())
                        gbs = needed_bytes(batch, C, plans.numel() * plans.element_size()) / (med * 1e-3) / 1e9
                        say(f"{arch:22s}{'discrete' if discrete else 'continuous':12s}{'per grid' if per_grid else 'shared':10s}{C:4d}"
                            f"{med:12.3f} [{low:6.3f}]{base[0]:12.3f} [{base[1]:6.3f}]{C * base[0]:13.3f}{med / (C * base[0]):8.3f}"
                            f"{C * N * steps / (med * 1e-3):14.3e}{gbs:13.1f}")
                        if C == 64 and not per_grid:      # ... and with the pick behind it (a second, small launch)
                            med_p, low_p, _ = event_ms(lambda: pe.lookahead(plans))
                            say(f"{'':22s}{'':12s}{'+ pick':10s}{C:4d}{med_p:12.3f} [{low_p:6.3f}]")
                        del plans
                pe.env.close()
                del batch, pe
                torch.cuda.empty_cache()
        say()

    if "b" in a.parts:
        say("(b) the receding-horizon loop, us per env-step (host clock around a synchronised window)")
        batch = generate(N, n_steps=a.T, seed=42, arch="genset+battery+grid", device=dev, series="factorised")
        pe = PerGridWindowEnv(batch, trajectory_length=a.length, discrete=True, auto_reset=True, seed=7, observations=False)
        pe.reset()
        for label, m in (("ShootingMPC(H=24, constant plans)", ShootingMPC(pe, H)),
                         ("ShootingMPC(H=24, constant + 32 random)", ShootingMPC(pe, H, n_random=32, seed=1))):
            m.run(20, reward=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter(); m.run(200, reward=False); torch.cuda.synchronize()
            say(f"    {label:44s}{(time.perf_counter() - t0) / 200 * 1e6:10.1f}")
        rbc = RuleBasedControl(pe)
        rbc.run_episodes(512, reset=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter(); rbc.run_episodes(4096, reset=False); torch.cuda.synchronize()
        say(f"    {'RuleBasedControl.run_episodes (chunk 512)':44s}{(time.perf_counter() - t0) / 4096 * 1e6:10.1f}")
        pe.env.close()
        del batch, pe
        torch.cuda.empty_cache()
        say()

    if "c" in a.parts:
        from pymgrid_amd import MicrogridBatch
        from pymgrid_amd.scenario import bucket_by_layout, load_npz_grids
        grids = load_npz_grids(os.path.join(ROOT, "pymgrid_amd", "data", "pymgrid25.npz"))
        say("(c) return over one pass of the packaged pymgrid25 scenarios (start 0, the whole series), per scenario")
        say(f"{'scenario':>9s}{'layout':>24s}{'steps':>7s}{'RuleBasedControl':>20s}{'ShootingMPC':>20s}{'MPC - RBC':>16s}")
        tot = [0.0, 0.0, 0]
        for idx in bucket_by_layout(grids).values():
            try:
                sub = [grids[n] for n in idx]
                steps = sub[0]["final_step"] - sub[0]["initial_step"]
                run = a.quality_steps or steps
                rets = []
                for who in ("rbc", "mpc"):
                    batch = MicrogridBatch.from_grids(sub, device=dev)
                    if batch.layout.multi:
                        raise ValueError("several modules of a kind")
                    pe = PerGridWindowEnv(batch, trajectory_length=steps, discrete=True, auto_reset=True, seed=7, observations=False)
                    pe.reset()
                    if who == "rbc":
                        r = RuleBasedControl(pe).run_episodes(run, reward=True, reset=False)["reward"]
                    else:
                        r = ShootingMPC(pe, H, n_random=32, seed=1).run(run, reward=True)["reward"]
                    rets.append(r.sum(dim=0).cpu())
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
