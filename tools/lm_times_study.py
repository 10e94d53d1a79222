"""Guard, price and value of the Levenberg-Marquardt step over parameters and waypoint times on one MI355X -- a
record, not a gate.
usage: python tools/lm_times_study.py [--parent-tree DIR] [--batch 4096] [--steps 20] [--windows 3] [--seeds 256] [--iters 50]
                                      [--tau-lr 0.02] [--skip guard,price,value] [--out profiles/lm_times.json]

(a) guard   as tools/free_times_study.py: `python bench.py --gpus 1 --steps 20 --warmup 5` in this tree and in `--parent-tree`, alternated;
            without `--parent-tree` the part is recorded as pending.
(b) price   quadrotor, n_grid 50, `--batch` rows, fp32: the LM step with lm_taus against without, fresh learners per window (5 warm-up
            steps, then `--steps` timed), windows alternated, medians; and lfsd_time_normal_blocks, lfsd_lm_step_times and lfsd_lm_step
            alone, HIP events, 20 after 5, on the state of a learner after one step.
(c) value   the quadrotor setting of tools/free_times_study.py (waypoints from the trajectory at theta* at the times tau*, the stamps
            replaced by chord-length times): joint LM, LM with the times fixed, Nesterov with learn_taus; outer iterations run, final
            loss, |theta - theta*| and max |tau - tau*| per variant, median and 90th percentile.  One setting, reported as found."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models
import bench
from free_times_study import event_ms, guard, window


def price(batch, steps, windows):
    w = bench.WORKLOADS["quadrotor"]
    oc, env, d = models.quadrotor(n_grid=w["n_grid"])
    oc.setDevice("cuda:0", torch.float32)
    demos = bench.demo_set(argparse.Namespace(batch=batch, config="quadrotor"), d, 0, "independent", w)

    def make(**kw):
        L = CPDP.SparseDemoLearner(oc, demos["x0"], d["horizon"], d["taus"], d["waypoints"], d["interface"], demos["theta0"],
                                   method="LM", **kw)
        L.count_unconverged = False
        return L
    variants = {"lm": lambda: make(), "lm_taus": lambda: make(lm_taus=True)}
    times = {k: [] for k in variants}
    for _ in range(windows):
        for k, fresh in variants.items():
            L = fresh()
            window(L, 5)
            times[k].append(window(L, steps))
            del L
    med = {k: float(np.median(v)) for k, v in times.items()}
    L = variants["lm_taus"]()
    L.step()
    lib, s, t = L.lib, L._lm, L._lmt
    loss, grad = L._aux["loss"].to(L.theta.dtype).contiguous(), L._aux["grad"].to(L.theta.dtype).contiguous()
    c = lambda x: x.clone()
    blocks = lambda: lib.time_normal_blocks(L._sol["state_grid"], L.hz, t["trial"], L._aux["auxX_grid"], L.iface)

    def step_times():      # (on copies of the state: every timed call starts from the same words)
        lib.lm_step_times(c(L.theta), c(s["loss"]), c(s["grad"]), c(s["H"]), c(s["lam"]), c(L.theta_trial), c(L.taus), c(t["trial"]),
                          c(t["gtau"]), c(t["C"]), c(t["d"]), c(t["ok"]), loss, grad, L._H_t, t["gtau_t"], t["C_t"], t["d_t"],
                          proj_lo=L.proj_lo)

    def step_plain():
        lib.lm_step(c(L.theta), c(s["loss"]), c(s["grad"]), c(s["H"]), c(s["lam"]), c(L.theta_trial), loss, grad, L._H_t, proj_lo=L.proj_lo)

    def copies():          # the clones alone: what the two figures above both contain
        for x in (L.theta, s["loss"], s["grad"], s["H"], s["lam"], L.theta_trial):
            c(x)
    launches = dict(time_normal_blocks=event_ms(blocks), lm_step_times_with_state_copies=event_ms(step_times),
                    lm_step_with_state_copies=event_ms(step_plain), state_copies_of_lm_step_alone=event_ms(copies))
    return dict(batch=batch, n_grid=w["n_grid"], dtype="f32", steps=steps, windows=windows,
                ms_per_step={k: [1e3 * x for x in v] for k, v in times.items()}, median_ms={k: 1e3 * v for k, v in med.items()},
                lm_spread_ms=1e3 * (max(times["lm"]) - min(times["lm"])), launches=launches,
                note="the two learners walk different paths (moving times change the solves' iteration counts): the step times are not a price")


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
    guess = stamps[1:-1] * (hz / stamps[-1])
    rng = np.random.default_rng(7)
    theta0 = star[None, :] * (1.0 + 0.2 * rng.uniform(-1, 1, (seeds, star.size)))
    out = dict(seeds=seeds, iters=iters, tau_learning_rate=tau_lr, theta_star=star.tolist(), tau_star=tau_star.tolist(),
               chord_length_times=guess.tolist(), initial_max_tau_error=float(np.abs(guess - tau_star).max()))
    pct = lambda x: dict(median=float(np.nanmedian(x)), p90=float(np.nanpercentile(x, 90)), n_nan=int(np.isnan(x).sum()))
    x0 = np.tile(d["ini_state"], (seeds, 1))
    variants = (("joint_lm", dict(method="LM", lm_taus=True)), ("lm_fixed_times", dict(method="LM")),
                ("nesterov_learn_taus", dict(method="Nesterov", learning_rate=d["lr"], mu=0.9, learn_taus=True, tau_learning_rate=tau_lr)))
    for name, kw in variants:
        L = CPDP.SparseDemoLearner(oc, x0, hz, guess, wps, iface, theta0, **kw)
        L.count_unconverged = False
        for _ in range(iters):
            L.step()
        if kw["method"] == "LM":                                   # the accepted point and its loss
            loss = L.lm_loss.double().cpu().numpy()
        else:
            loss = L.evaluate(L.theta)[0].double().cpu().numpy()
        th, tau = L.theta.double().cpu().numpy(), L.taus.double().cpu().numpy()
        out[name] = dict(outer_iterations=iters, final_loss=pct(loss), theta_error=pct(np.linalg.norm(th - star[None, :], axis=1)),
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
    ap.add_argument("--out", default=os.path.join("profiles", "lm_times.json"))
    a = ap.parse_args()
    skip = set(filter(None, a.skip.split(",")))
    rec = dict(device=torch.cuda.get_device_name(0))
    rec["guard"] = dict(status="skipped") if "guard" in skip else guard(a.parent_tree, a.windows)
    rec["price"] = dict(status="skipped") if "price" in skip else price(a.batch, a.steps, a.windows)
    rec["value"] = dict(status="skipped") if "value" in skip else value(a.seeds, a.iters, a.tau_lr)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print(json.dumps(rec, sort_keys=True))


if __name__ == "__main__":
    main()
