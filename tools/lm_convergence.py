"""Outer iterations and step cost of the Levenberg-Marquardt update on an MI355X -- a record, not a gate.
usage: python tools/lm_convergence.py [--batch 4096] [--max-iter 100] [--steps 20] [--out profiles/lm_convergence.json]

Workloads: the benchmark's quadrotor (n_grid 50, fp32, `--batch` seeds of bench.demo_set) and the pendulum of
Examples/pendulum_groundtruth.py (n_grid 10, fp64, waypoints sampled at the true parameters, `--batch` seeds within +-30 % of them).
  iterations  outer iterations until the reference's stop test (`loss > 0.9 and |grad| > 0.05`, lib/QuadAlgorithm.py:242) fails, per
              seed (`stop_rule`), at most --max-iter: median, 90th percentile, share of seeds that never stopped -- for "LM" at its
              default values and at lm_lambda0 = 300 against "Nesterov" (lr 0.01, mu 0.9) and "Adam" (lr 0.22), the settings of
              test/opt_methods_comparison.py;
  phases      mean milliseconds per phase of a step from the learner's event_hook (HIP events), --steps steps after 5 warm-up steps,
              "LM" against "Vanilla" in the same run: what the sensitivity grids, lfsd_normal_matrix and lfsd_lm_step add."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models
import bench

METHODS = (("LM", dict(method="LM")), ("LM_lambda0_300", dict(method="LM", lm_lambda0=300.0)),
           ("Nesterov", dict(method="Nesterov", learning_rate=0.01, mu=0.9)),
           ("Adam", dict(method="Adam", learning_rate=0.22, beta_1=0.9, beta_2=0.999, epsilon=1e-8)))


def iterations(make, max_iter):
    out = {}
    for name, kw in METHODS:
        L = make(stop_rule=dict(loss=0.9, grad_norm=0.05), **kw)
        for _ in range(max_iter):
            if L.n_active == 0:
                break
            L.step()
        stop = L.stop_iter.cpu().numpy()
        took = np.where(stop == 0, max_iter, stop)
        out[name] = dict(median=float(np.median(took)), p90=float(np.percentile(took, 90)), never_stopped=float((stop == 0).mean()))
    return out


def phases(make, steps, warm=5):
    out = {}
    for name, kw in (("LM", dict(method="LM")), ("Vanilla", dict(method="Vanilla", learning_rate=1e-2))):
        L = make(**kw)
        L.count_unconverged = False
        for _ in range(warm):
            L.step()
        torch.cuda.synchronize()
        ev, cur = {}, {}

        def hook(nm):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            if cur.get("prev"):
                ev.setdefault(cur["prev"][0], []).append((cur["prev"][1], e))
            cur["prev"] = None if nm == "end" else (nm, e)
        L.event_hook = hook
        for _ in range(steps):
            L.step()
        torch.cuda.synchronize()
        ms = {k: float(np.mean([a.elapsed_time(b) for a, b in v])) for k, v in ev.items()}
        out[name] = dict(ms, total=float(sum(ms.values())))
    out["LM_over_Vanilla"] = out["LM"]["total"] / out["Vanilla"]["total"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "lm_convergence.json"))
    a = ap.parse_args()
    B = a.batch
    rec = dict(device=torch.cuda.get_device_name(0), batch=B, max_iter=a.max_iter, steps=a.steps)
    # quadrotor: the benchmark's workload
    w = bench.WORKLOADS["quadrotor"]
    oc, env, d = models.quadrotor(n_grid=w["n_grid"])
    oc.setDevice("cuda:0", torch.float32)
    demos = bench.demo_set(argparse.Namespace(batch=B, config="quadrotor"), d, 0, "independent", w)
    make = lambda **kw: CPDP.SparseDemoLearner(oc, demos["x0"], d["horizon"], d["taus"], d["waypoints"], d["interface"], demos["theta0"], **kw)
    rec["quadrotor"] = dict(n_grid=w["n_grid"], dtype="f32", iterations=iterations(make, a.max_iter), phases=phases(make, a.steps))
    # pendulum: Examples/pendulum_groundtruth.py
    oc, env, d = models.pendulum(n_grid=10)
    oc.setDevice("cuda:0", torch.float64)
    true = np.asarray(d["true_theta"], dtype=np.float64)
    taus = np.array([0.1, 0.3, 0.6, 0.7, 0.9]) * d["horizon"]
    sol = oc.cocSolverBatch(np.asarray([d["ini_state"]]), d["horizon"], true[None, :])
    wps = oc.sampleBatch(sol, taus)["state"][0][:, d["interface"]].double().cpu().numpy()
    seeds = true[None, :] * (1.0 + 0.3 * np.random.default_rng(7).uniform(-1, 1, (B, true.size)))
    x0 = np.tile(d["ini_state"], (B, 1))
    make = lambda **kw: CPDP.SparseDemoLearner(oc, x0, d["horizon"], taus, wps, d["interface"], seeds, **kw)
    rec["pendulum"] = dict(n_grid=10, dtype="f64", iterations=iterations(make, a.max_iter), phases=phases(make, a.steps))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print(json.dumps(rec, sort_keys=True))


if __name__ == "__main__":
    main()
