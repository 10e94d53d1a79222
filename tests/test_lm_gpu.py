"""GPU tier of the Levenberg-Marquardt outer update (ABI 14): lfsd_normal_matrix and lfsd_lm_step of the gfx950 library at the shapes
of tests/lm_cases.py (a batch of one, the 16-parameter limit, 4099 rows with a partial last workgroup, a one-interval grid); the LM
learner against the same launches made by hand, bit for bit (pendulum fp64, quadrotor fp32 with 36 rows); the ground-truth case; the
stop rule and the driver.  The same cases pass on the SIMT emulator (tests/test_lm_emu.py)."""
import numpy as np
import pytest
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models
import hyper_sweep_cases as H
import lm_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
SHAPES = pytest.mark.parametrize("shape", C.SHAPES_GPU, ids=lambda s: "B%dp%d" % s)


@pytest.fixture(scope="module")
def lib():
    return models.pendulum(n_grid=10)[0].compile()


@DTYPES
@SHAPES
def test_normal_matrix_against_fp64_restatement_on_the_device(lib, shape, dtype):
    B, p = shape
    for n_grid in C.N_GRIDS:
        for K in C.N_WAYPOINTS:
            rh, rg = C.run_normal_matrix(lib, DEV, dtype, B, p, n_grid, K)
            print("normal_matrix B%d p%d n_grid %d K %d: |H - ref| / bound %.3f, |J^T r - vjp| / bound %.3f" % (B, p, n_grid, K, rh, rg))
            assert rh <= 1.0 and rg <= 1.0, (n_grid, K, rh, rg)
            rs = C.run_normal_matrix_general(lib, DEV, dtype, B, p, n_grid, K)
            print("    sign-changing sensitivities: |H - ref| / bound %.3f" % rs)
            assert rs <= 1.0, (n_grid, K, rs)


@DTYPES
@SHAPES
def test_lm_step_walks_the_known_branches_on_the_device(lib, shape, dtype):
    B, p = shape
    for offset in (range(2 * C.KINDS) if B < 2 * C.KINDS else (0,)):
        worst = C.run_lm_step(lib, DEV, dtype, B, p, offset)
        assert worst <= 1.0, (offset, worst)
    print("lm_step B%d p%d: worst backward error / bound %.3f" % (B, p, worst))


def _learner_case(kind, dtype, rows, **data):
    oc, env, d = getattr(models, kind)(n_grid=10)
    oc.setDevice(DEV, dtype)
    d = dict(d, **data)
    seeds = C.compose_seeds(d["theta0"], rows)
    args = (np.tile(d["ini_state"], (rows, 1)), d["horizon"], d["taus"], d["waypoints"], d["interface"], seeds)

    def make(rows=slice(None), **kw):
        return CPDP.SparseDemoLearner(oc, args[0][rows], *args[1:5], args[5][rows], method="LM", **kw)
    return oc, args, make


PENDULUM = dict(taus=[0.2, 0.5, 0.8], waypoints=[[0.4], [1.5], [2.6]])


def test_pendulum_learner_is_its_launches_on_the_device():
    oc, args, make = _learner_case("pendulum", torch.float64, 8, **PENDULUM)
    C.run_composition(make, oc, args, C.COMPOSE_LAMBDA0["pendulum"])


def test_quadrotor_learner_is_its_launches_on_the_device():
    """36 rows (the first 12 are the CPU tier's), fp32, default mapping."""
    oc, args, make = _learner_case("quadrotor", torch.float32, 36)
    C.run_composition(make, oc, args, C.COMPOSE_LAMBDA0["quadrotor"])


def test_lm_learns_the_ground_truth_on_the_device():
    def make_oc():
        oc, env, d = models.pendulum(n_grid=10)
        oc.setDevice(DEV, torch.float64)
        return oc, d
    C.run_learns(make_oc)


def test_stop_rule_level_2_and_trace_on_the_device():
    oc, args, make = _learner_case("pendulum", torch.float64, 4, **PENDULUM)
    K = 4
    free = make(lm_lambda0=30.0, interplation_level=2)
    hist = []
    for _ in range(K):
        l, g = free.step()
        hist.append((l.clone(), g.clone(), free.theta.clone(), free.theta_trial.clone(), free.lm_lambda.clone(), free.lm_loss.clone()))
    first = hist[0][0]
    order = torch.argsort(first)
    rule = dict(loss=float(0.5 * (first[order[0]] + first[order[1]])), grad_norm=1e-12)      # the best seed stops after step 1
    L = make(stop_rule=rule, trace=K, lm_lambda0=30.0, interplation_level=2)
    for k in range(K):
        l, g = L.step()
        stop = L.stop_iter.cpu()
        for b in range(L.B):
            if not int(stop[b]) or int(stop[b]) == k + 1:
                for a, ref in zip((l, g, L.theta, L.theta_trial, L.lm_lambda, L.lm_loss), hist[k]):
                    assert H.same(a[b], ref[b]), (k, b)
    b0 = int(order[0])
    assert int(L.stop_iter[b0]) == 1 and L.n_active < L.B
    assert torch.equal(L.theta[b0], hist[0][2][b0]) and torch.equal(L.lm_lambda[b0], hist[0][4][b0])      # frozen since step 1
    assert torch.equal(L.theta_trace[b0, 1], L.theta[b0]) and bool(torch.isnan(L.theta_trace[b0, 2:]).all())
    on = L.stop_iter == 0
    assert torch.equal(L.theta_trace[on, K], L.theta[on])


def test_skip_unconverged_keeps_the_lm_state_of_a_frozen_row_on_the_device():
    oc, args, make = _learner_case("pendulum", torch.float64, 8, **PENDULUM)
    C.run_skip_unconverged(make, oc, args[0], args[1])


def test_level_2_and_trace_on_the_device():
    """Without a stop rule: the trace files the accepted theta; level 2 differs from level 1 from the second trial point on (these
    waypoint times are grid nodes, where the two interpolants of x agree: the first loss is the same, the sensitivities are not)."""
    oc, args, make = _learner_case("pendulum", torch.float64, 3, **PENDULUM)
    a, b = make(trace=6, lm_lambda0=30.0), make(interplation_level=2, warm_start=True, lm_lambda0=30.0)
    for k in range(6):
        la, _ = a.step()
        assert torch.equal(a.theta_trace[:, k + 1], a.theta) and torch.equal(a.loss_trace[:, k], la)
        if k < 2:
            lb, _ = b.step()
            assert bool(torch.isfinite(lb).all()) and (k == 0 or not bool((la == lb).any()))
    assert bool(b.lm_accepted.all()) and bool((a.theta_trace[:, 6] != a.theta_trace[:, 1]).any(dim=1).all())
    assert bool(torch.isfinite(a.grad_norm_trace).all())


def test_quadalgorithm_runs_lm_per_seed_on_the_device():
    new, ini, goal, demo = H.quad_driver(10, torch.float32, device=DEV)
    Q = new()
    Q.load_optimization_function(dict(method="LM", iter_num=4, lm_lambda0=300.0))
    seeds = np.array([1, 0.1, 0.1, 0.1, 0.1, 0.1, -1], dtype=float)[None, :] * np.array([[1.0], [1.3]])
    res = Q.run(ini, goal, demo, ObsList=[], initial_parameters=seeds, stop="per_seed")
    n = res["loss_trace"].shape[0]
    assert 1 <= n <= 4 and res["loss_trace"].shape == (n, 2) and res["parameter_trace"].shape == (n + 1, 2, 7)
    assert res["stop_iter"].shape == (2,) and np.isfinite(res["loss_trace"]).all()
