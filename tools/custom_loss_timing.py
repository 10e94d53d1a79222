"""Timings of the user-defined losses (ABI 12) on the headline shape (quadrotor, n_grid 50, fp32, 4096 bench seeds).

    python tools/custom_loss_timing.py [--out profiles/custom_loss_timing.json] [--reps 3] [--parent DIR]

(a) lfsd_sample_grid / lfsd_waypoint_vjp at K = 5 and K = 101 beside the same result composed from torch operations on the device
    (index, lerp, einsum), on the grids of one solved batch;
(b) a learner step with loss_fn = the squared waypoint loss beside the fused learner, with the share of aux_forward (want_grids makes
    the sweep write auxX_grid / auxU_grid);
(c) with --parent DIR (a built checkout of the parent commit): `python bench.py` there and here, alternated.
HIP events around every window, the variants of one comparison alternated, `--reps` windows each; the record keeps every window."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "custom_loss_timing.json"))
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50, help="kernel calls per window of (a)")
    ap.add_argument("--steps", type=int, default=10, help="learner steps per window of (b)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--bench-reps", type=int, default=3)
    args = ap.parse_args()
    import bench
    import lfsd_amd  # noqa: F401
    from lfsd_amd import CPDP, models
    assert torch.cuda.is_available(), "a timing needs the GPU"
    w = bench.WORKLOADS["quadrotor"]
    oc, env, d = models.quadrotor(n_grid=w["n_grid"])
    oc.setDevice("cuda:0", torch.float32)
    lib = oc.compile()
    B, N = args.batch, w["n_grid"]
    demos = bench.demo_set(argparse.Namespace(batch=B, config="quadrotor"), d, 0, "independent", w)

    def events(fn, count):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(count):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / count

    def alternate(variants, count):
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                ms[k].append(round(events(fn, count), 5))
        return dict(ms=ms, median_ms={k: round(float(np.median(v)), 5) for k, v in ms.items()})

    # ---- (a) the kernels beside torch compositions ----
    sol = oc.cocSolverBatch(demos["x0"], d["horizon"], demos["theta0"])
    aux = oc.auxSysSolverBatch(sol, want_grids=True)
    hz, X, aX, aU = sol["horizon"], sol["state_grid"], aux["auxX_grid"], aux["auxU_grid"]
    n, m, p = lib.n_state, lib.n_control, lib.n_auxvar
    rows_a = []

    def torch_lerp(grid, t):              # grid [B, N+1, C], t [B, K] -> [B, K, C]
        h = (hz / N)[:, None]
        k = torch.floor(t / h).clamp(0, N - 1)
        s = ((t - k * h) / h)[:, :, None]
        ia = k.long()[:, :, None].expand(-1, -1, grid.shape[2])
        ya = torch.gather(grid, 1, ia)
        return torch.lerp(ya, torch.gather(grid, 1, ia + 1), s)

    for K in (5, 101):
        t = (torch.linspace(0.02, 0.98, K, device="cuda:0")[None, :] * hz[:, None]).contiguous()
        rx = torch.randn((B, K, n), device="cuda:0")
        ru = torch.randn((B, K, m), device="cuda:0")
        aXf, aUf = aX.reshape(B, N + 1, p * n), aU.reshape(B, N + 1, p * m)
        out_s, out_x, out_g = torch.empty((B, K, n), device="cuda:0"), torch.empty((B, K, p * n), device="cuda:0"), torch.empty((B, p), device="cuda:0")

        def torch_vjp():
            return (torch.einsum("bki,bkqi->bq", rx, torch_lerp(aXf, t).reshape(B, K, p, n))
                    + torch.einsum("bkj,bkqj->bq", ru, torch_lerp(aUf, t).reshape(B, K, p, m)))
        assert torch.allclose(lib.sample_grid(X, hz, t), torch_lerp(X, t), rtol=1e-4, atol=1e-5)
        gk, gt = lib.waypoint_vjp(hz, t, rx, aX, ru, aU), torch_vjp()
        ok = torch.isfinite(gt).all(dim=1)
        assert torch.allclose(gk[ok], gt[ok], rtol=1e-3, atol=1e-3 * float(gt[ok].abs().max()))
        rec = dict(K=K,
                   sample_state=alternate(dict(kernel=lambda: lib.sample_grid(X, hz, t, out=out_s), torch=lambda: torch_lerp(X, t)), args.calls),
                   sample_auxX=alternate(dict(kernel=lambda: lib.sample_grid(aXf, hz, t, out=out_x), torch=lambda: torch_lerp(aXf, t)), args.calls),
                   waypoint_vjp=alternate(dict(kernel=lambda: lib.waypoint_vjp(hz, t, rx, aX, ru, aU, out=out_g), torch=torch_vjp), args.calls))
        print(json.dumps({k: (v if k == "K" else v["median_ms"]) for k, v in rec.items()}), flush=True)
        rows_a.append(rec)

    # ---- (b) a learner step: loss_fn = the squared waypoint loss beside the fused learner ----
    def learner(**kw):
        return CPDP.SparseDemoLearner(oc, demos["x0"], d["horizon"], d["taus"], d["waypoints"], d["interface"], demos["theta0"],
                                      method=w["method"], learning_rate=w["lr"], mu=0.9, **kw)
    fused = learner()
    idx, wps = list(d["interface"]), fused.wps
    cust = learner(loss_fn=lambda xt, ut: ((xt[:, :, idx] - wps) ** 2).sum((1, 2)), grad_scale=0.5)
    start = fused.theta.clone()

    def stepper(L):
        def run():
            L.step()
        return run

    def reset(L):
        L.theta.copy_(start)
        for t_ in (L.m, L.v, L.vhat):
            t_.zero_()
        L.iter_idx = 0
    steps = {}
    for _ in range(args.reps):
        for name, L in (("fused", fused), ("loss_fn", cust)):
            reset(L)
            for _ in range(args.warmup):
                L.step()
            torch.cuda.synchronize()
            steps.setdefault(name, []).append(round(events(stepper(L), args.steps), 4))

    def phase_ms(L):                      # one step bracketed with HIP events through the learner's hook
        reset(L)
        L.step()
        marks = []

        def hook(nm):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((nm, e))
        L.event_hook = hook
        L.step()
        torch.cuda.synchronize()
        L.event_hook = None
        return {a[0]: round(a[1].elapsed_time(b[1]), 4) for a, b in zip(marks[:-1], marks[1:])}
    rec_b = dict(step_ms=steps, step_ms_median={k: round(float(np.median(v)), 4) for k, v in steps.items()},
                 phases_ms=dict(fused=phase_ms(fused), loss_fn=phase_ms(cust)))
    print(json.dumps(rec_b), flush=True)

    # ---- (c) the default benchmark on the parent commit and on this tree, alternated ----
    rec_c = None
    if args.parent:
        runs = {"parent": [], "this": []}
        for _ in range(args.bench_reps):
            for name, cwd in (("parent", os.path.abspath(args.parent)), ("this", ROOT)):
                r = subprocess.run([sys.executable, "bench.py"], cwd=cwd, capture_output=True, text=True, timeout=600)
                assert r.returncode == 0, r.stderr[-2000:]
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
                res = json.loads(line)
                runs[name].append({k: res[k] for k in res if isinstance(res[k], (int, float)) and not isinstance(res[k], bool)})
                print(name, line[:300], flush=True)
        rec_c = runs
    out = dict(tool="tools/custom_loss_timing.py", workload="quadrotor n_grid 50 fp32, %d bench seeds" % B, device=torch.cuda.get_device_name(0),
               reps=args.reps, calls_per_window=args.calls, steps_per_window=args.steps, warmup=args.warmup,
               note="HIP events around each window; the variants of one comparison alternate; ms per call / per step",
               kernels=rows_a, learner=rec_b, bench=rec_c)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
