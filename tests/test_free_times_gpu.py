"""GPU tier of the learnable waypoint times (ABI 17): lfsd_waypoint_time_grad and lfsd_tau_project of the gfx950 library at the shapes
of tests/tau_cases.py (a batch of one, 4099 rows with a partial last workgroup, one- and two-interval grids, both interpolants);
the central difference of the existing fused loss; the learner against the same launches made by hand, bit for bit (quadrotor fp32
with 36 rows).  The same cases pass on the SIMT emulator (tests/test_free_times_emu.py), which also covers the compiled-in interface:
no zoo model carries one, so no gfx950 library with one is built."""
import numpy as np
import pytest
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models
import lm_cases
import tau_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
SHAPES = pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "B%dK%d" % s)


@pytest.fixture(scope="module")
def lib():
    return models.quadrotor(n_grid=10)[0].compile()


@DTYPES
@SHAPES
def test_time_grad_linear_against_fp64_restatement_on_the_device(lib, shape, dtype):
    B, K = shape
    for n_grid in C.N_GRIDS:
        r = C.run_time_grad(lib, DEV, dtype, B, K, n_grid, cubic=False)
        print("time_grad linear B%d K%d n_grid %d: |dtau - ref| / bound %.3f" % (B, K, n_grid, r))
        assert r <= 1.0, (n_grid, r)


@DTYPES
@SHAPES
def test_time_grad_cubic_against_scipy_spline_derivative_on_the_device(lib, shape, dtype):
    B, K = shape
    for n_grid in C.N_GRIDS_CUBIC:
        r = C.run_time_grad(lib, DEV, dtype, B, K, n_grid, cubic=True)
        print("time_grad cubic B%d K%d n_grid %d: |dtau - ref| / bound %.3f" % (B, K, n_grid, r))
        assert r <= 1.0, (n_grid, r)


@DTYPES
def test_prior_term_alone_is_one_rounding_on_the_device(lib, dtype):
    C.run_prior_alone(lib, DEV, dtype)


@DTYPES
@SHAPES
@pytest.mark.parametrize("c", [0.1, 0.49])
def test_tau_project_is_its_numpy_restatement_on_the_device(lib, shape, dtype, c):
    C.run_tau_project(lib, DEV, dtype, shape[0], shape[1], c)


def test_central_difference_of_the_fused_loss_is_twice_dtau_on_the_device():
    """The quadrotor's fused loss (fp64, linear level) at tau +- h / 64 around mid-interval times: exactly quadratic inside an interval,
    so the only error is rounding, bounded as in tests/test_free_times_emu.py."""
    oc, env, d = models.quadrotor(n_grid=10)
    oc.setDevice(DEV, torch.float64)
    n_grid, hz, iface = 10, float(d["horizon"]), list(d["interface"])
    h = hz / n_grid
    mids = [1.5 * h, 4.5 * h, 8.5 * h]
    wps = torch.tensor([np.asarray(d["waypoints"])[:3].tolist()], dtype=torch.float64, device=DEV)
    sol = oc.cocSolverBatch(np.asarray([d["ini_state"]]), hz, np.asarray([d["theta0"]], dtype=np.float64))
    taus = torch.tensor([mids], dtype=torch.float64, device=DEV)
    idx = torch.tensor(iface, dtype=torch.int32, device=DEV)
    dtau = oc.compile().waypoint_time_grad(sol["state_grid"], sol["horizon"], taus, wps, idx).cpu().numpy()
    ref, bound = C.time_grad_reference(sol["horizon"], taus, sol["state_grid"], wps, n_grid, idx=tuple(iface))
    assert float((np.abs(dtau - ref) / bound).max()) <= 1.0
    X = sol["state_grid"].cpu().numpy()[0][:, iface]
    e, eps = h / 64, C.eps_of(torch.float64)
    for k, tk in enumerate(mids):
        lo, hi = taus.clone(), taus.clone()
        lo[:, k] -= e
        hi[:, k] += e
        Lm = float(oc.auxSysSolverBatch(sol, lo, wps, iface)["loss"][0])
        Lp = float(oc.auxSysSolverBatch(sol, hi, wps, iface)["loss"][0])
        kk = [int(np.floor(t / h)) for t in mids]
        M = np.array([np.abs(X[j]) + np.abs(X[j + 1]) for j in kk])
        r = np.array([np.abs(0.5 * (X[j] + X[j + 1]) - wps[0, i].cpu().numpy()) + np.abs(X[j + 1] - X[j]) / 64 for i, j in enumerate(kk)])
        dL = eps * (8 * (r * M).sum() + 3 * len(iface) * max(Lp, Lm))
        fd = (Lp - Lm) / (2 * e)
        tol = dL / e + 2 * bound[0, k]
        print("waypoint %d: |fd - 2 dtau| / bound %.3f" % (k, abs(fd - 2 * dtau[0, k]) / tol))
        assert abs(fd - 2 * dtau[0, k]) <= tol


def test_quadrotor_learner_is_its_launches_on_the_device():
    """36 rows, fp32, default mapping: Vanilla, Nesterov (the projected look-ahead) and Adam."""
    oc, env, d = models.quadrotor(n_grid=10)
    oc.setDevice(DEV, torch.float32)
    rows = 36
    seeds = lm_cases.compose_seeds(d["theta0"], rows)
    K = len(d["taus"])
    args = (np.tile(d["ini_state"], (rows, 1)), d["horizon"], d["taus"], d["waypoints"], d["interface"], seeds)
    x0, hz = oc._t(args[0]), oc._t(d["horizon"]).expand(rows).contiguous()
    taus = oc._t(d["taus"]).expand(rows, K).contiguous()
    wps = oc._t(d["waypoints"]).expand(rows, K, len(d["interface"])).contiguous()
    make = lambda **kw: CPDP.SparseDemoLearner(oc, *args, learn_taus=True, **kw)
    C.run_composition(make, oc, x0, hz, wps, list(d["interface"]), taus,
                      (("Vanilla", 1e-3, "Vanilla", 1e-3), ("Nesterov", 1e-4, "Nesterov", 1e-4), ("Adam", 1e-2, "Adam", 5e-3)))
