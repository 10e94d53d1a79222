"""Cost of the hyper-parameter sweep on an MI355X -- a record, not a gate.
usage: python tools/hyper_sweep_timing.py [--batch 4096] [--steps 20] [--windows 3] [--out profiles/hyper_sweep_timing.json]

On `--batch` quadrotor seeds of the benchmark (n_grid 50, fp32), alternating windows of `--steps` steps, `--windows` windows per
variant, medians of the per-step time of a window (fresh learners per window: 5 warm-up steps, then the timed ones):
  scalar      the uniform Nesterov learner, scalar arguments (today's path)
  rows        the same values given as arrays: lfsd_lookahead_rows + lfsd_optimizer_step_rows
  trace       the scalar learner with trace=steps+5 (25): one lfsd_trace_append per step
  sweep       ONE learner of 8 configurations x batch/8 seeds
  one_by_one  EIGHT uniform learners of batch/8 seeds, one after the other (the sum of their windows)
The guard that the default path is what it was is bench.py on both trees; this tool times one tree."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models
import bench

ADAM = dict(beta_1=0.9, beta_2=0.999, epsilon=1e-8)
# test/opt_methods_comparison.py + three of the Adam rates of test/adam_learning_rate_comparison.py
CONFIGS = (dict(method="Vanilla", learning_rate=0.06), dict(method="Nesterov", learning_rate=0.01, mu=0.9),
           dict(method="Adam", learning_rate=0.22, **ADAM), dict(method="Nadam", learning_rate=0.10, **ADAM),
           dict(method="AMSGrad", learning_rate=0.06, **ADAM), dict(method="Adam", learning_rate=0.01, **ADAM),
           dict(method="Adam", learning_rate=0.02, **ADAM), dict(method="Adam", learning_rate=0.03, **ADAM))
DEFAULTS = dict(mu=0.9, beta_1=0.9, beta_2=0.999, epsilon=1e-8)


def window(learners, steps):
    """Seconds per step of `steps` steps of every learner in turn (one synchronisation at each end)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for L in learners:
        for _ in range(steps):
            L.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "hyper_sweep_timing.json"))
    a = ap.parse_args()
    w = bench.WORKLOADS["quadrotor"]
    oc, env, d = models.quadrotor(n_grid=w["n_grid"])
    oc.setDevice("cuda:0", torch.float32)
    B, C = a.batch, len(CONFIGS)
    S = B // C
    demos = bench.demo_set(argparse.Namespace(batch=B, config="quadrotor"), d, 0, "independent", w)
    x0, th0 = demos["x0"], demos["theta0"]
    warm = 5
    total = warm + a.steps                                            # steps a learner lives: trace=25 at the default --steps 20

    def make(rows, **kw):
        L = CPDP.SparseDemoLearner(oc, x0[rows], d["horizon"], d["taus"], d["waypoints"], d["interface"], th0[rows], **kw)
        L.count_unconverged = False
        return L
    everything = slice(0, B)
    nest = dict(method="Nesterov", learning_rate=w["lr"], mu=0.9)
    per_row = {k: [dict(DEFAULTS, **c)[k] for c in CONFIGS for _ in range(S)] for k in ("method", "learning_rate", "mu", "beta_1", "beta_2", "epsilon")}

    def sweep():      # every configuration's block on the same S seeds, as the eight uniform learners
        L = CPDP.SparseDemoLearner(oc, np.tile(x0[:S], (C, 1)), d["horizon"], d["taus"], d["waypoints"], d["interface"],
                                   np.tile(th0[:S], (C, 1)), **per_row)
        L.count_unconverged = False
        return [L]
    variants = {
        "scalar": lambda: [make(everything, **nest)],
        "rows": lambda: [make(everything, **dict(nest, learning_rate=np.full(B, w["lr"]), mu=np.full(B, 0.9)))],
        "trace": lambda: [make(everything, trace=total, **nest)],
        "one_by_one": lambda: [make(slice(0, S), **c) for c in CONFIGS],
        "sweep": sweep,
    }
    # Every window starts from FRESH learners -- 5 warm-up steps, then outer iterations 6 .. 5 + steps timed -- so that all windows
    # of a variant time the same outer iterations (a learner that kept learning across windows would be a different workload in
    # each); the variants alternate window by window.
    times = {k: [] for k in variants}
    for _ in range(a.windows):
        for k, fresh in variants.items():
            Ls = fresh()
            window(Ls, warm)
            times[k].append(window(Ls, a.steps))
            del Ls
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in times.items()}
    rec = dict(device=torch.cuda.get_device_name(0), batch=B, n_grid=w["n_grid"], dtype="f32", steps=a.steps, warmup_steps=warm, trace_capacity=total, windows=a.windows,
               configurations=C, seeds_per_configuration=S, ms_per_step={k: [1e3 * t for t in v] for k, v in times.items()},
               median_ms={k: 1e3 * v for k, v in med.items()}, spread=spread,
               rows_over_scalar=med["rows"] / med["scalar"], trace_over_scalar=med["trace"] / med["scalar"],
               one_by_one_over_sweep=med["one_by_one"] / med["sweep"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print(json.dumps(rec, sort_keys=True))


if __name__ == "__main__":
    main()
