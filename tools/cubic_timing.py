"""The auxiliary sweeps along the cubic interpolant (interplation_level=2) beside the linear ones on the headline shape (quadrotor,
n_grid 50, fp32, the benchmark's 4096 seeds): aux_riccati, aux_forward and the three curvature launches, HIP-event times.

    python tools/cubic_timing.py [--out profiles/cubic_interpolant_timing.json] [--reps 20] [--label ...]
    python tools/cubic_timing.py --level1-only      # runs on a tree without the feature too (the parent's figures)

Both levels are timed alternately on the same solved grids.  `--resources FILE` folds in the registers / scratch / LDS of the sweep
kernels from `tools/kernel_resources.py quadrotor --json FILE`; build times and the bench.py line are added to the record with
`--note key=value`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch


def kernel_resources(path):
    """The aux-sweep rows of a table written by `tools/kernel_resources.py quadrotor --json FILE` (no GPU needed for that one)."""
    if not path:
        return None
    return [r for r in json.load(open(path)) if "aux_" in r["name"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cubic_interpolant_timing.json"))
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--level1-only", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--resources", default="", help="JSON table of tools/kernel_resources.py quadrotor --json")
    ap.add_argument("--note", action="append", default=[], help="key=value pairs kept in the record")
    args = ap.parse_args()
    import bench
    import lfsd_amd  # noqa: F401
    from lfsd_amd import models
    assert torch.cuda.is_available(), "a timing needs the GPU"
    w = bench.WORKLOADS["quadrotor"]
    oc, env, d = models.quadrotor(n_grid=w["n_grid"])
    oc.setDevice("cuda:0", torch.float32)
    lib = oc.compile()
    B = args.batch
    demos = bench.demo_set(argparse.Namespace(batch=B, config="quadrotor"), d, 0, "independent", w)
    sol = oc.cocSolverBatch(demos["x0"], d["horizon"], demos["theta0"])
    levels = (1,) if args.level1_only else (1, 2)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    ms = {lv: dict(aux_riccati=[], aux_forward=[], curvature=[]) for lv in levels}
    Z = out = None
    for rep in range(args.warmup + args.reps):
        for lv in levels:
            marks = {}
            hook = lambda nm: marks.setdefault(nm, ev()).record()
            kw = {}
            t0, t1 = ev(), ev()
            if lv == 2:
                t0.record()
                kw = dict(interplation_level=2)
                curv = tuple(lib.grid_curvature(sol[k]) for k in ("state_grid", "control_grid", "costate_grid"))
                t1.record()
            aux = oc.auxSysSolverBatch(sol, d["taus"], d["waypoints"], d["interface"], Z_grid=Z, out=out, phase_hook=hook,
                                       validate=False, **kw)
            Z, out = aux["Z_grid"], {k: aux[k] for k in ("loss", "grad", "stats")}
            torch.cuda.synchronize()
            if rep >= args.warmup:
                ms[lv]["aux_riccati"].append(marks["riccati"].elapsed_time(marks["forward"]))
                ms[lv]["aux_forward"].append(marks["forward"].elapsed_time(marks["end"]))
                if lv == 2:
                    ms[lv]["curvature"].append(t0.elapsed_time(t1))
    # (with a phase hook the level-2 call fits the curvature grids before the "riccati" mark: they are timed on their own above)
    med = {"level%d" % lv: {k: round(float(np.median(v)), 4) for k, v in r.items() if v} for lv, r in ms.items()}
    rec = dict(tool="tools/cubic_timing.py", label=args.label, workload="quadrotor n_grid %d fp32, %d bench seeds" % (w["n_grid"], B),
               device=torch.cuda.get_device_name(0), reps=args.reps, ms_median=med,
               ms_min={"level%d" % lv: {k: round(float(np.min(v)), 4) for k, v in r.items() if v} for lv, r in ms.items()},
               units_mean={"riccati": float(aux["stats"][:, 0].float().mean()), "forward": float(aux["stats"][:, 2].float().mean())},
               kernels=kernel_resources(args.resources),
               notes=dict(kv.split("=", 1) for kv in args.note),
               note="HIP-event times of one launch each (curvature: the three lfsd_grid_curvature launches of a step together); "
                    "kernels: registers / scratch per lane / LDS per workgroup of the sweep kernels as the compiler reports them")
    print(json.dumps(rec, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
