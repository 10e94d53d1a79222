"""GPU tier of the Levenberg-Marquardt step over parameters and waypoint times (ABI 18): lfsd_time_normal_blocks and lfsd_lm_step_times
of the gfx950 library at the shapes of tests/lm_times_cases.py (a batch of one, 130 rows across a workgroup boundary, 4099 rows with a
partial last workgroup, groups of several rows, the 16-parameter limit, a one-interval grid, both levels); the learner with lm_taus
against the same launches made by hand, bit for bit (quadrotor fp32, 36 rows, n_grid 10; grouped pendulum fp64).  The same cases pass
on the SIMT emulator (tests/test_lm_times_emu.py)."""
import numpy as np
import pytest
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models
import hyper_sweep_cases as H
import lm_cases as LC
import lm_times_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
SHAPES = pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "B%dp%dK%d" % s)
GROUPS = pytest.mark.parametrize("shape", C.GROUPS, ids=lambda s: "G%dD%dp%dK%d" % s)


@pytest.fixture(scope="module")
def lib():
    return models.pendulum(n_grid=10)[0].compile()


@pytest.fixture(scope="module")
def qlib():
    return models.quadrotor(n_grid=10)[0].compile()


@DTYPES
@SHAPES
def test_time_blocks_against_fp64_restatement_on_the_device(lib, shape, dtype):
    B, p, K = shape
    for n_grid in C.N_GRIDS:
        for cubic in ((False, True) if n_grid >= 3 else (False,)):
            r = C.run_time_blocks(lib, DEV, dtype, B, p, K, n_grid, cubic)
            print("time_blocks B%d p%d K%d n_grid %d level %d: worst fraction of the bound %.3f" % (B, p, K, n_grid, 2 if cubic else 1, r))
            assert r <= 1.0, (n_grid, cubic, r)


@DTYPES
@pytest.mark.parametrize("shape", C.SHAPES[:3], ids=lambda s: "B%dp%dK%d" % s)
def test_arrow_matrix_is_the_gram_matrix_of_the_augmented_jacobian_on_the_device(lib, qlib, shape, dtype):
    B, p, K = shape
    for n_grid, cubic in ((1, False), (10, False), (3, True), (10, True)):
        r = C.run_arrow_identity(lib, DEV, dtype, B, p, K, n_grid, cubic, tg_lib=qlib)
        print("arrow identity B%d p%d K%d n_grid %d level %d: worst fraction of the summed bounds %.3f" % (B, p, K, n_grid, 2 if cubic else 1, r))
        assert r <= 1.0, (n_grid, cubic, r)


@DTYPES
@SHAPES
def test_lm_step_times_walks_the_known_branches_on_the_device(lib, shape, dtype):
    B, p, K = shape
    for offset in (range(0, 3 * C.KINDS, 1) if B < 2 * C.KINDS else (0,)):
        worst, worst_np = C.run_lm_step_times(lib, DEV, dtype, B, 1, p, K, offset)
        assert worst_np <= 1.0 and worst <= 1.0, (offset, worst, worst_np)
    print("lm_step_times B%d p%d K%d: worst backward error / bound %.3f (numpy elimination in the dtype %.3f)" % (B, p, K, worst, worst_np))


@DTYPES
@GROUPS
def test_lm_step_times_grouped_on_the_device(lib, shape, dtype):
    G, D, p, K = shape
    for offset in (range(0, 3 * C.KINDS, 1) if G < 2 * C.KINDS else (0, 3)):
        worst, worst_np = C.run_lm_step_times(lib, DEV, dtype, G, D, p, K, offset)
        assert worst_np <= 1.0 and worst <= 1.0, (offset, worst, worst_np)
    print("lm_step_times G%d D%d p%d K%d: worst backward error / bound %.3f (numpy elimination in the dtype %.3f)" % (G, D, p, K, worst, worst_np))


QUAD_LAMBDA0 = LC.COMPOSE_LAMBDA0["quadrotor"]


def test_quadrotor_learner_is_its_launches_on_the_device():
    """36 rows, fp32, n_grid 10, default mapping: the learner against its launches, bit for bit over 6 steps, tau state included."""
    oc, env, d = models.quadrotor(n_grid=10)
    oc.setDevice(DEV, torch.float32)
    rows = 36
    seeds = LC.compose_seeds(d["theta0"], rows)
    x0 = np.tile(d["ini_state"], (rows, 1))

    def make(rows=slice(None), **kw):
        return CPDP.SparseDemoLearner(oc, x0[rows], d["horizon"], d["taus"], d["waypoints"], d["interface"], seeds[rows], method="LM",
                                      lm_taus=True, lm_lambda0=QUAD_LAMBDA0, **kw)
    K = len(d["taus"])
    hz = oc._t(d["horizon"]).expand(rows).contiguous()
    taus = oc._t(d["taus"]).expand(rows, K).contiguous()
    wps = oc._t(d["waypoints"]).expand(rows, K, -1).contiguous()
    hand = C.lmt_by_hand(oc, oc._t(x0), hz, taus, wps, d["interface"], seeds, 6, make().proj_lo, QUAD_LAMBDA0)
    C.run_composition(make, hand, steps=6, half=17)


def test_grouped_pendulum_learner_is_its_launches_on_the_device():
    oc, env, d = models.pendulum(n_grid=10)
    oc.setDevice(DEV, torch.float64)
    seeds = LC.compose_seeds(d["theta0"], 2)
    D, G = 3, 2
    taus_d = np.array([[0.2, 0.5, 0.8], [0.25, 0.5, 0.75], [0.1, 0.4, 0.9]])
    wps_d = np.array([[[0.4], [1.5], [2.6]], [[0.5], [1.4], [2.4]], [[0.2], [1.1], [2.8]]])
    x0_d = np.tile(d["ini_state"], (D, 1))

    def make(rows=slice(None), **kw):
        return CPDP.SparseDemoLearner(oc, x0_d, 1.0, taus_d, wps_d, [0], seeds[rows], method="LM", lm_taus=True, mode="grouped",
                                      demos_per_seed=D, lm_lambda0=C.GROUPED_LAMBDA0, skip_unconverged=False, **kw)
    hand = C.lmt_by_hand(oc, np.tile(x0_d, (G, 1)), oc._t(1.0).expand(G * D).contiguous(), np.tile(taus_d, (G, 1)), np.tile(wps_d, (G, 1, 1)),
                         [0], seeds, 6, make().proj_lo, C.GROUPED_LAMBDA0, D=D, skip=False)
    C.run_composition(make, hand, steps=6, half=1, D=D)


def test_level_2_weights_bounds_and_driver_on_the_device():
    oc, env, d = models.pendulum(n_grid=10)
    oc.setDevice(DEV, torch.float64)
    seeds = LC.compose_seeds(d["theta0"], 4)
    x0 = np.tile(d["ini_state"], (4, 1))
    taus, wps = [0.23, 0.52, 0.81], [[0.4], [1.5], [2.6]]
    w = torch.tensor([1.0, 0.5, 2.0], dtype=torch.float64, device=DEV).expand(4, 3).contiguous()
    bounds = ([0.15, 0.45, 0.7], [0.3, 0.6, 0.9])
    mk = lambda rows=slice(None), **kw: CPDP.SparseDemoLearner(oc, x0[rows], 1.0, taus, wps, [0], seeds[rows], method="LM", lm_taus=True,
                                                               lm_lambda0=1.0, interplation_level=2, waypoint_weights=w[rows],
                                                               tau_bounds=bounds, trace=3, **kw)
    bt = tuple(oc._t(x).expand(4, 3).contiguous() for x in bounds)
    hand = C.lmt_by_hand(oc, oc._t(x0), oc._t(1.0).expand(4).contiguous(), oc._t(taus).expand(4, 3).contiguous(),
                         oc._t(wps).expand(4, 3, 1).contiguous(), [0], seeds, 3, mk().proj_lo, 1.0, level=2, wts=w, bounds=bt)
    L, _ = C.run_composition(mk, hand, steps=3, bounds=bounds, need_reject=False, need_accept=False)
    assert torch.equal(L.theta_trace[:, 3], L.theta)
    new, ini, goal, demo = H.quad_driver(10, torch.float32, device=DEV)
    Q = new()
    Q.load_optimization_function(dict(method="LM", iter_num=3, lm_lambda0=300.0))
    res = Q.run(ini, goal, demo, ObsList=[], lm_taus=True)
    assert res["taus"].shape == (1, 3) and res["tau_trace"].shape[1:] == (1, 3) and np.all(np.diff(res["taus"][0]) > 0)
