"""GPU tier of the user-defined losses (ABI 12): lfsd_sample_grid / lfsd_waypoint_vjp of the gfx950 libraries against torch fp64 on the
device at the shapes of tests/sample_cases.py (4099 trajectories included), COCSys.sampleBatch / sampleAuxBatch and the loss_fn learner
on the quadrotor library in fp32 and fp64, and four steps of a loss_fn learner on the benchmark's seeds.

The bounds are the derived ones of sample_cases, unchanged.  The same comparisons pass on the SIMT emulator (tests/test_sample_emu.py)."""
import argparse

import numpy as np
import pytest
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models
import cubic_cases as CC
import sample_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])


@pytest.fixture(scope="module")
def lib():
    return models.pendulum(n_grid=10)[0].compile()


@DTYPES
@pytest.mark.parametrize("n_grid", S.N_GRIDS)
def test_sample_grid_on_the_device(lib, n_grid, dtype):
    worst = 0.0
    for n_comp in S.N_COMPS:
        for batch in S.BATCHES_GPU:
            y64 = CC.grid_values(batch, n_grid, n_comp, seed=3)
            for n_times in S.N_TIMES:
                for cubic in (False, True):
                    for per_traj in (True, False):
                        for offset in (range(S.KINDS) if batch * n_times < S.KINDS else (0,)):
                            ratio, _ = S.run_sample(lib, DEV, dtype, n_grid, n_comp, n_times, batch, cubic, per_traj, offset, y64=y64)
                            assert ratio <= 1.0, (n_grid, n_comp, batch, n_times, cubic, per_traj, offset, ratio)
                            worst = max(worst, ratio)
    print("sample_grid %s n_grid %d on the device: worst error / bound %.3f" % (dtype, n_grid, worst))


@DTYPES
def test_nan_time_gives_a_nan_row_on_the_device(lib, dtype):
    for cubic in (False, True):
        _, (y, curv, hz, t, out) = S.run_sample(lib, DEV, dtype, 8, 13, 5, 67, cubic, True)
        t2 = t.clone()
        t2[40, 3] = float("nan")
        got = lib.sample_grid(y, hz, t2, curv=curv)
        assert bool(torch.isnan(got[40, 3]).all())
        got[40, 3] = out[40, 3]
        assert torch.equal(got, out)


@DTYPES
@pytest.mark.parametrize("dims", S.VJP_DIMS, ids=lambda d: "n%dm%dp%d" % d)
def test_waypoint_vjp_on_the_device(lib, dims, dtype):
    n, m, p = dims
    worst = 0.0
    for n_grid in S.VJP_N_GRIDS:
        for K in S.VJP_TIMES:
            for batch in S.BATCHES_GPU:
                for with_u in (True, False):
                    ratio = S.run_vjp(lib, DEV, dtype, batch, n_grid, n, m, p, K, with_u)
                    assert ratio <= 1.0, (dims, n_grid, K, batch, with_u, ratio)
                    worst = max(worst, ratio)
    print("waypoint_vjp %s (n, m, p) = %s on the device: worst error / bound %.3f" % (dtype, dims, worst))


# ---- the Python layer on the quadrotor library (n_grid 10, batch 64) ---------------------------------------------------------
def quad_batch(dtype, n_grid=10, B=64):
    oc, env, d = models.quadrotor(n_grid=n_grid)
    oc.setDevice(DEV, dtype)
    rng = np.random.default_rng(11)
    th = np.asarray(d["theta0"], dtype=np.float64)[None, :] * (1.0 + 0.1 * rng.standard_normal((B, len(d["theta0"]))))
    th[:, 0] = np.abs(th[:, 0]) + 0.2
    x0 = np.tile(np.asarray(d["ini_state"], dtype=np.float64), (B, 1))
    x0[:, :3] += 0.2 * rng.standard_normal((B, 3))
    return oc, d, th, x0


@DTYPES
def test_sample_batch_on_the_quadrotor(dtype):
    oc, d, th, x0 = quad_batch(dtype)
    lib = oc.compile()
    n, m, p = lib.n_state, lib.n_control, lib.n_auxvar
    sol = oc.cocSolverBatch(x0, d["horizon"], th)
    B, N, H = 64, 10, d["horizon"]
    times = np.concatenate(([0.0, H, 0.3 * H], np.asarray(d["taus"], dtype=np.float64), np.linspace(0, H, 101)))
    tt = torch.as_tensor(times).to(device=DEV, dtype=dtype)
    for level in (1, 2):
        s = oc.sampleBatch(sol, times, level)
        for key, gk in (("state", "state_grid"), ("control", "control_grid"), ("costate", "costate_grid")):
            curv = lib.grid_curvature(sol[gk]) if level == 2 else None
            ref = S.interp_reference(sol[gk], curv, sol["horizon"], tt)
            ratio = float(((s[key].double() - ref).abs() / (S.sampling_bound(sol[gk], curv, dtype) + 1e-300)).max())
            print("sampleBatch quadrotor %s level %d %s: worst error / bound %.3f" % (dtype, level, key, ratio))
            assert ratio <= 1.0 and tuple(s[key].shape) == (B, len(times), sol[gk].shape[2])
    aux = oc.auxSysSolverBatch(sol, want_grids=True)
    sa = oc.sampleAuxBatch(aux, sol["horizon"], times)
    for key, gk, e in (("dx", "auxX_grid", n), ("du", "auxU_grid", m)):
        flat = aux[gk].reshape(B, N + 1, p * e)
        ref = S.interp_reference(flat, None, sol["horizon"], tt).reshape(B, len(times), p, e)
        bound = S.sampling_bound(flat, None, dtype).reshape(B, 1, p, e) + 1e-300
        ok = torch.isfinite(ref).all(dim=3).all(dim=2).all(dim=1)              # (a row the sweeps skipped is NaN on both sides)
        ratio = float(((sa[key].double() - ref).abs() / bound)[ok].max())
        print("sampleAuxBatch quadrotor %s %s: worst error / bound %.3f (%d rows)" % (dtype, key, ratio, int(ok.sum())))
        assert ratio <= 1.0 and int(ok.sum()) >= B - 2
    with pytest.raises(ValueError):
        oc.sampleBatch(sol, [1.01 * H])


def fused_parity(oc, d, x0, th, dtype, level, what, **kw):
    """First evaluation of the loss_fn learner (squared waypoint loss, grad_scale 0.5) against the fused learner: both within the
    derived bounds of the fp64 evaluation on the learner's own grids, and within twice the bounds of each other."""
    idx = list(d["interface"])
    fused = CPDP.SparseDemoLearner(oc, x0, d["horizon"], d["taus"], d["waypoints"], d["interface"], th, interplation_level=level, **kw)
    cust = CPDP.SparseDemoLearner(oc, x0, d["horizon"], d["taus"], None, None, th, interplation_level=level,
                                  loss_fn=S.squared_waypoint_loss(idx, fused.wps), grad_scale=0.5, **kw)
    lf, gf = (t.double() for t in fused.evaluate(fused.theta))
    lc, gc = (t.double() for t in cust.evaluate(cust.theta))
    assert torch.equal(fused._sol["state_grid"], cust._sol["state_grid"])
    curv = cust._aux["curvature"][0] if level == 2 else None
    rl, rg, bl, bg = S.fused_reference(cust._sol["state_grid"], cust._aux["auxX_grid"], cust.hz, cust.taus, fused.wps, idx, curv)
    eps = S.eps_of(dtype)
    ok = torch.isfinite(rl) & torch.isfinite(rg).all(dim=1)
    assert int(ok.sum()) >= len(ok) - 2 and bool((torch.isfinite(lc) == ok).all()) and bool((torch.isfinite(lf) == ok).all())
    fl = lambda b: b * eps + 1e-300
    r = dict(loss_fn=((lc - rl).abs() / fl(bl))[ok].max(), fused=((lf - rl).abs() / fl(bl))[ok].max(),
             paths=((lc - lf).abs() / fl(2 * bl))[ok].max(), grad_loss_fn=((gc - rg).abs() / fl(bg))[ok].max(),
             grad_fused=((gf - rg).abs() / fl(bg))[ok].max(), grad_paths=((gc - gf).abs() / fl(2 * bg))[ok].max())
    r = {k: round(float(v), 3) for k, v in r.items()}
    print("fused parity %s %s level %d: error / bound %s" % (what, dtype, level, r))
    assert max(r.values()) <= 1.0, r
    return fused, cust


@DTYPES
@pytest.mark.parametrize("level", [1, 2])
def test_squared_loss_fn_is_the_fused_loss_on_the_quadrotor(dtype, level):
    oc, d, th, x0 = quad_batch(dtype)
    fused_parity(oc, d, x0, th, dtype, level, "quadrotor n_grid 10")


def test_loss_fn_learner_on_the_benchmark_seeds():
    """64 of the benchmark's seeds (quadrotor, n_grid 50, fp32, Nesterov as the benchmark runs it), four steps with the squared waypoint
    loss as a loss_fn: first-step parity with the fused learner within the fp32 bounds, finite losses and gradients, and a loss that
    falls from step 1 to step 4 for every seed whose solves ended converged."""
    import bench
    B = 64
    w = bench.WORKLOADS["quadrotor"]
    oc, env, d = models.quadrotor(n_grid=w["n_grid"])
    oc.setDevice(DEV, torch.float32)
    demos = bench.demo_set(argparse.Namespace(batch=B, config="quadrotor"), d, 0, "independent", w)
    fused, L = fused_parity(oc, d, demos["x0"], demos["theta0"], torch.float32, 1, "benchmark seeds n_grid 50", method=w["method"],
                            learning_rate=w["lr"], mu=0.9)
    losses, conv = [], torch.ones(B, dtype=torch.bool, device=DEV)
    for it in range(4):
        l, g = L.step()
        st = L._sol["status"]
        conv &= (st == 1) | (st == 2)
        losses.append(l.double().clone())
        assert bool(torch.isfinite(l[conv]).all()) and bool(torch.isfinite(g[conv]).all())
    print("loss_fn learner, 64 benchmark seeds: %d converged throughout, loss step 1 median %.4f -> step 4 median %.4f, largest ratio %.4f"
          % (int(conv.sum()), float(losses[0][conv].median()), float(losses[3][conv].median()), float((losses[3] / losses[0])[conv].max())))
    assert int(conv.sum()) >= B // 2
    assert bool((losses[3] < losses[0])[conv].all())
