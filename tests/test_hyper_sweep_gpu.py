"""GPU tier of the hyper-parameter sweeps in one batch (ABI 13): the three kernels of the gfx950 library against the scalar entry
points, bit for bit, at the shapes of tests/hyper_sweep_cases.py (4099 rows included); the 36-row quadrotor sweep in fp32 against nine
uniform learners, bit for bit; QuadAlgorithm.run_comparison against run(stop="per_seed").  The same comparisons pass on the SIMT
emulator (tests/test_hyper_sweep_emu.py)."""
import numpy as np
import pytest
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models
import hyper_sweep_cases as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
SHAPES = pytest.mark.parametrize("shape", H.SHAPES_GPU, ids=lambda s: "B%dp%d" % s)


@pytest.fixture(scope="module")
def lib():
    return models.pendulum(n_grid=10)[0].compile()


@DTYPES
@SHAPES
def test_rows_step_is_the_scalar_step_per_row_on_the_device(lib, shape, dtype):
    B, p = shape
    for iter_idx in H.ITERS:
        for masked in (False, True):
            for offset in (range(10) if B == 1 and not masked else (0,)):
                H.run_rows_against_scalars(lib, DEV, dtype, B, p, iter_idx, masked, offset)


@DTYPES
@SHAPES
def test_lookahead_rows_and_trace_append_on_the_device(lib, shape, dtype):
    for offset in (range(10) if shape[0] == 1 else (0,)):
        H.run_lookahead_rows(lib, DEV, dtype, *shape, offset=offset)
    for masked in (False, True):
        H.run_trace_append(lib, DEV, dtype, *shape, masked=masked)


def test_quadrotor_sweep_is_nine_uniform_learners_on_the_device():
    """Quadrotor, n_grid 10, fp32, the nine configurations x 4 seeds (36 rows), 6 steps, default mapping."""
    oc, env, d = models.quadrotor(n_grid=10)
    oc.setDevice(DEV, torch.float32)
    S, C = 4, len(H.NINE_CONFIGS)
    rng = np.random.default_rng(5)
    seeds = np.asarray(d["theta0"], dtype=np.float64)[None, :] * (1.0 + 0.1 * rng.uniform(-1, 1, (S, len(d["theta0"]))))
    args = (np.tile(d["ini_state"], (C * S, 1)), d["horizon"], d["taus"], d["waypoints"], d["interface"], np.tile(seeds, (C, 1)))
    make = lambda **kw: CPDP.SparseDemoLearner(oc, *args, **kw)
    sweep, got = H.sweep_against_uniform(make, H.NINE_CONFIGS, seeds=S, steps=6)
    assert sweep.theta.shape == (36, 7) and bool(torch.isfinite(sweep.loss_trace).all())
    # uniform values given as arrays: the rows path, and the scalar learner's bits
    cfg = H.METHOD_CONFIGS[3]
    a = make(**cfg)
    b = make(**dict(cfg, learning_rate=np.full(C * S, cfg["learning_rate"]), beta_2=[cfg["beta_2"]] * (C * S)))
    assert b._rows_path and not a._rows_path
    for (la, ga, ta), (lb, gb, tb) in zip(H.run_learner(a, 3), H.run_learner(b, 3)):
        assert torch.equal(la, lb) and torch.equal(ga, gb) and torch.equal(ta, tb)


def test_run_comparison_on_the_device():
    new, ini, goal, demo = H.quad_driver(10, torch.float32, device=DEV)
    H.run_comparison_case(new, ini, goal, demo, iter_num=4)
