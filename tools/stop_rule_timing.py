"""Step time of the headline learner (quadrotor, n_grid 50, fp32, Nesterov, 4096 bench seeds) with the per-seed stop rule at fixed
active counts, next to a plain learner (no rule) on a batch of the same size.

    python tools/stop_rule_timing.py [--out profiles/stop_rule_timing.json] [--active 4096,3072,2048,1024,256] [--reps 3]
    python tools/stop_rule_timing.py --plain-only      # runs on a tree without the feature too (the parent's figure)

The rule's thresholds are set where no seed ever stops; the active set is then cut to the wanted size by retiring evenly spaced
seeds through lfsd_stop_compact itself (made-up losses), so every timed step takes the path of a learner whose set has shrunk:
gather, dense solve and sweeps, scatter, masked update, test, one 4-byte read.  Both variants of one size are timed alternately,
`--reps` times each, `--steps` steps per window between two synchronisations; the record keeps every window."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stop_rule_timing.json"))
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--active", default="4096,3072,2048,1024,256")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import bench
    import lfsd_amd  # noqa: F401
    from lfsd_amd import CPDP, models
    assert torch.cuda.is_available(), "a timing needs the GPU"
    w = bench.WORKLOADS["quadrotor"]
    oc, env, d = models.quadrotor(n_grid=w["n_grid"])
    oc.setDevice("cuda:0", torch.float32)
    B = args.batch
    demos = bench.demo_set(argparse.Namespace(batch=B, config="quadrotor"), d, 0, "independent", w)
    sync = torch.cuda.synchronize

    def learner(rows, **kw):
        return CPDP.SparseDemoLearner(oc, demos["x0"][rows], d["horizon"], d["taus"], d["waypoints"], d["interface"],
                                      demos["theta0"][rows], method=w["method"], learning_rate=w["lr"], mu=0.9, **kw)

    def window(L, theta0):
        # (every window walks the same iterations of the same seeds: parameters, optimizer state and counter start again)
        L.theta.copy_(theta0)
        for t in (L.m, L.v, L.vhat):
            t.zero_()
        L.iter_idx = 0
        for _ in range(args.warmup):
            L.step()
        sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            L.step()
        sync()
        return (time.perf_counter() - t0) / args.steps * 1e3

    rows_out = []
    for n in [int(v) for v in args.active.split(",")]:
        keep = np.unique(np.linspace(0, B - 1, n).round().astype(int))
        assert len(keep) == n
        variants = {"plain": learner(keep)}
        if not args.plain_only:
            L = learner(np.arange(B), stop_rule=dict(loss=-1.0, grad_norm=-1.0))
            L.step()
            if n < B:
                fake = torch.zeros(B, device="cuda:0") - 2.0          # below the loss threshold: these seeds stop ...
                fake[torch.as_tensor(keep, device="cuda:0")] = 1.0    # ... these go on
                L._apply_stop_rule(fake, torch.ones((B, L.theta.shape[1]), device="cuda:0"))
            assert L.n_active == n, (L.n_active, n)
            variants["stop_rule"] = L
        start = {k: v.theta.clone() for k, v in variants.items()}
        ms = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, v in variants.items():
                ms[k].append(window(v, start[k]))
        if "stop_rule" in variants:
            assert variants["stop_rule"].n_active == n             # nobody stopped during the windows
        rec = dict(batch=B, n_active=n, step_ms={k: [round(x, 4) for x in v] for k, v in ms.items()},
                   step_ms_median={k: round(float(np.median(v)), 4) for k, v in ms.items()})
        if "stop_rule" in ms:
            rec["overhead_ms"] = round(rec["step_ms_median"]["stop_rule"] - rec["step_ms_median"]["plain"], 4)
        print(json.dumps(rec), flush=True)
        rows_out.append(rec)
    out = dict(tool="tools/stop_rule_timing.py", label=args.label, workload="quadrotor n_grid 50 fp32 Nesterov lr 1e-2, bench seeds",
               steps_per_window=args.steps, warmup=args.warmup, reps=args.reps, device=torch.cuda.get_device_name(0),
               note="step_ms: wall clock between two device synchronisations / steps, host work and the rule's one 4-byte read per "
                    "step included; plain = a learner without a rule on a batch of n_active seeds (the same seeds)",
               rows=rows_out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
