"""Guard, price and value of the learnable waypoint times on one MI355X -- a record, not a gate.
usage: python tools/free_times_study.py [--parent-tree DIR] [--batch 4096] [--steps 20] [--windows 3] [--seeds 256] [--iters 50]
                                        [--tau-lr 0.02] [--skip guard,price,value] [--out profiles/free_times.json]

(a) guard   `python bench.py --gpus 1 --steps 20 --warmup 5` as child processes, in this tree and in `--parent-tree` (a checkout of the
            parent commit built side by side), alternated, `--windows` runs per tree: medians of it/s and of aux_forward, the
            difference, and the run-to-run spread of the parent's own runs (as DESIGN.md section 10 did).  Without `--parent-tree` the
            part is recorded as pending.
(b) price   quadrotor, n_grid 50, `--batch` rows, fp32, the benchmark's Nesterov learner: step time with learn_taus=True against
            False and against learn_taus=True at tau_learning_rate 0 (every added launch, the times and so the workload unmoved: the
            price), fresh learners per window (5 warm-up steps, then `--steps` timed), windows alternated, medians; and the three added
            launches (lfsd_waypoint_time_grad, lfsd_optimizer_step on the times, lfsd_tau_project) alone, HIP events, 20 after 5.
(c) value   the quadrotor example with waypoints taken from its trajectory at a known theta* at the times tau*, the time stamps
            replaced by CPDP.chord_length_times (scaled to the horizon); theta learned for `--iters` Nesterov iterations from `--seeds`
            seeds with and without learn_taus (tau_learning_rate `--tau-lr`, tau_max_shift at its default): final loss,
            |theta - theta*| and max |tau - tau*| per variant, median and 90th percentile.  Reported as found; nothing is claimed
            about other values of tau_learning_rate or tau_max_shift."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models
import bench


def bench_once(tree):
    """One bench.py run in `tree` as a fresh child process; (it/s, aux_forward ms)."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree, capture_output=True,
                       text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("bench.py failed in %s: %s" % (tree, r.stderr[-2000:]))
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return float(rec["value"]), float(rec["config"]["kernel_ms"]["aux_forward"])


def guard(parent, runs):
    if parent is None:
        return dict(status="pending: no --parent-tree given")
    out = {"parent": [], "this": []}
    for _ in range(runs):
        for k, tree in (("parent", parent), ("this", ROOT)):
            out[k].append(bench_once(tree))
    med = {k: float(np.median([v[0] for v in vs])) for k, vs in out.items()}
    fwd = {k: float(np.median([v[1] for v in vs])) for k, vs in out.items()}
    spread = max(v[0] for v in out["parent"]) - min(v[0] for v in out["parent"])
    return dict(status="measured", runs=out, median_its=med, median_aux_forward_ms=fwd, difference_its=med["this"] - med["parent"],
                parent_spread_its=spread, inside_parent_spread=bool(abs(med["this"] - med["parent"]) <= spread))


def window(L, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        L.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def event_ms(fn, n=20, warm=5):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return dict(median_ms=float(np.median(t)), min_ms=t[0], max_ms=t[-1])


def price(batch, steps, windows, tau_lr):
    w = bench.WORKLOADS["quadrotor"]
    oc, env, d = models.quadrotor(n_grid=w["n_grid"])
    oc.setDevice("cuda:0", torch.float32)
    demos = bench.demo_set(argparse.Namespace(batch=batch, config="quadrotor"), d, 0, "independent", w)

    def make(**kw):
        L = CPDP.SparseDemoLearner(oc, demos["x0"], d["horizon"], d["taus"], d["waypoints"], d["interface"], demos["theta0"],
                                   method="Nesterov", learning_rate=w["lr"], mu=0.9, **kw)
        L.count_unconverged = False
        return L
    # (moving times change the gradient of theta and with it the path of the learner and the iterations of its solves: the variant
    #  at rate 0 makes every added launch and leaves the times, and so the workload, where they are -- that one is the price)
    variants = {"fixed": lambda: make(), "learn_taus_rate_0": lambda: make(learn_taus=True, tau_learning_rate=0.0),
                "learn_taus": lambda: make(learn_taus=True, tau_learning_rate=tau_lr)}
    times = {k: [] for k in variants}
    for _ in range(windows):                                       # fresh learners per window, variants alternated
        for k, fresh in variants.items():
            L = fresh()
            window(L, 5)
            times[k].append(window(L, steps))
            del L
    med = {k: float(np.median(v)) for k, v in times.items()}
    L = variants["learn_taus"]()
    L.step()
    lib, s = L.lib, L._tau
    idx = L.iface
    grad = lambda: lib.waypoint_time_grad(L._sol["state_grid"], L.hz, L.taus, L.wps, idx, out=L.tau_grad)
    opt = lambda: lib.optimizer_step("Nesterov", L.taus, L.tau_grad, 1, 0.0, 0.9, m=s["m"], v=s["v"], vhat=s["vhat"])      # (rate 0: the times stay)
    proj = lambda: lib.tau_project(s["start"], L.taus, L.hz, s["c"])
    s["start"].copy_(L.taus)
    launches = dict(waypoint_time_grad=event_ms(grad), optimizer_step_on_taus=event_ms(opt), tau_project=event_ms(proj))
    return dict(batch=batch, n_grid=w["n_grid"], dtype="f32", steps=steps, windows=windows, tau_learning_rate=tau_lr,
                ms_per_step={k: [1e3 * t for t in v] for k, v in times.items()}, median_ms={k: 1e3 * v for k, v in med.items()},
                added_ms=1e3 * (med["learn_taus_rate_0"] - med["fixed"]),
                fixed_spread_ms=1e3 * (max(times["fixed"]) - min(times["fixed"])), launches=launches)


def value(seeds, iters, tau_lr):
    oc, env, d = models.quadrotor()
    oc.setDevice("cuda:0", torch.float32)
    hz, iface = float(d["horizon"]), list(d["interface"])
    star = np.array(d["theta0"], dtype=np.float64)
    tau_star = np.array(d["taus"], dtype=np.float64)
    sol = oc.cocSolverBatch(np.asarray([d["ini_state"]]), hz, star[None, :])
    wps = oc.sampleBatch(sol, tau_star)["state"][0][:, iface].double().cpu().numpy()
    ends = oc.sampleBatch(sol, np.array([0.0, hz]))["state"][0][:, iface].double().cpu().numpy()
    stamps = CPDP.chord_length_times(np.concatenate([ends[:1], wps, ends[1:]]), 1.0)
    guess = stamps[1:-1] * (hz / stamps[-1])                       # the stamps on the learner's horizon
    rng = np.random.default_rng(7)
    theta0 = star[None, :] * (1.0 + 0.2 * rng.uniform(-1, 1, (seeds, star.size)))
    out = dict(seeds=seeds, iters=iters, tau_learning_rate=tau_lr, theta_star=star.tolist(), tau_star=tau_star.tolist(),
               chord_length_times=guess.tolist(), initial_max_tau_error=float(np.abs(guess - tau_star).max()))
    pct = lambda x: dict(median=float(np.nanmedian(x)), p90=float(np.nanpercentile(x, 90)), n_nan=int(np.isnan(x).sum()))
    for name, kw in (("fixed", {}), ("learn_taus", dict(learn_taus=True, tau_learning_rate=tau_lr))):
        L = CPDP.SparseDemoLearner(oc, np.tile(d["ini_state"], (seeds, 1)), hz, guess, wps, iface, theta0, method="Nesterov",
                                   learning_rate=d["lr"], mu=0.9, **kw)
        L.count_unconverged = False
        for _ in range(iters):
            L.step()
        loss = L.evaluate(L.theta)[0].double().cpu().numpy()
        th = L.theta.double().cpu().numpy()
        tau = L.taus.double().cpu().numpy()
        out[name] = dict(final_loss=pct(loss), theta_error=pct(np.linalg.norm(th - star[None, :], axis=1)),
                         max_tau_error=pct(np.abs(tau - tau_star[None, :]).max(axis=1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--seeds", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--tau-lr", type=float, default=0.02)
    ap.add_argument("--skip", default="")
    ap.add_argument("--out", default=os.path.join("profiles", "free_times.json"))
    a = ap.parse_args()
    skip = set(filter(None, a.skip.split(",")))
    rec = dict(device=torch.cuda.get_device_name(0))
    rec["guard"] = dict(status="skipped") if "guard" in skip else guard(a.parent_tree, a.windows)
    rec["price"] = dict(status="skipped") if "price" in skip else price(a.batch, a.steps, a.windows, a.tau_lr)
    rec["value"] = dict(status="skipped") if "value" in skip else value(a.seeds, a.iters, a.tau_lr)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print(json.dumps(rec, sort_keys=True))


if __name__ == "__main__":
    main()
