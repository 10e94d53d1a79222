"""CPU tier of interpolation level 2 (cocSolver(..., interplation_level=2) handed to auxSysSolver, CPDP.py:388-390, 320-323): the
curvature-fit kernel and the level-2 instantiations of the two auxiliary sweeps through the SIMT emulator, against the fp64 recipe /
scipy's interp1d(kind='cubic') and the fp64 oracle integrating along the cubic interpolant (tests/cubic_cases.py)."""
import ctypes

import numpy as np
import pytest
import scipy.interpolate as sip
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models, runtime
from lfsd_amd.runtime import LfsdError
from conftest import build_emu_library
import cubic_cases as C


@pytest.fixture(scope="module")
def lib():
    return runtime.ModelLibrary(build_emu_library(models.pendulum(n_grid=8)[0]))


def _prepare(emu):
    def prepare(oc, dtype):
        emu(oc)
        oc.setDevice(dtype=dtype)
        return oc
    return prepare


# ---- 1. the curvature fit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_grid", C.N_GRIDS)
def test_recipe_is_scipys_cubic(n_grid):
    C.check_recipe_against_scipy(n_grid)
    # ... and the host restatement the interpolant probe of auxSysSolver uses is the same recipe
    y = C.grid_values(2, n_grid, 3)[0]
    assert np.abs(CPDP.notaknot_curvature(y) - C.curvature_recipe(y)).max() <= 1e-13 * np.abs(y).max()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n_grid", C.N_GRIDS)
def test_grid_curvature_matches_recipe(lib, n_grid, dtype):
    for n_comp in C.N_COMPS:
        for batch in C.BATCHES:
            C.run_curvature(lib, "cpu", dtype, n_grid, n_comp, batch)


def test_grid_curvature_refuses_bad_arguments(lib):
    L = lib.lib
    buf = (ctypes.c_double * 64)()
    d = ctypes.cast(buf, ctypes.c_void_p)
    d2 = ctypes.c_void_p(d.value + 256)
    assert L.lfsd_grid_curvature(1, 1, 2, 2, d, d2, None) == -1           # n_grid = 2: scipy's cubic needs four nodes
    for bad in ((7, 1, 3, 2, d, d2), (1, 0, 3, 2, d, d2), (1, 1, 3, 0, d, d2), (1, -1, 3, 2, d, d2), (1, 1, 3, 2, None, d2),
                (1, 1, 3, 2, d, None), (1, 1, 3, 2, d, d)):
        assert L.lfsd_grid_curvature(*bad, None) == -1, bad
    with pytest.raises(LfsdError):
        lib.grid_curvature(torch.zeros(2, 3, 2, dtype=torch.float64))
    # the cubic sweeps: all three curvature grids are required, n_grid >= 3 -- refused before any launch (host dummies)
    common = lambda n_grid, cx, cu, cl: [1, 1, n_grid, d, d, d, 0, d, d, d, cx, cu, cl, d]
    tail = [0, 0, None, None, None, d, d, None, None, 0, 1e-3, None, None, 0, None]
    assert L.lfsd_aux_solve_cubic(*common(8, None, d, d), *tail) == -1
    assert L.lfsd_aux_solve_cubic(*common(8, d, None, d), *tail) == -1
    assert L.lfsd_aux_forward_cubic(*common(8, d, d, None), *tail) == -1
    assert L.lfsd_aux_solve_cubic(*common(2, d, d, d), *tail) == -1
    assert L.lfsd_aux_riccati_cubic(*common(8, d, None, d), 0, 1e-3, None, None, 0, None) == -1
    assert L.lfsd_aux_riccati_cubic(*common(8, d, d, d), 0, 1e-3, None, None, 1 << 4, None) == -1      # a mask without the status array


# ---- 2. the sweeps against the cubic oracle ----------------------------------------------------------------------------
# (the emulator runs a lane group as fibers: the arm at 32 units and the quadrotor take minutes per dtype here, so their fp32
#  instantiations are left to the GPU tier, which runs all six combinations)
@pytest.mark.parametrize("kind,dtype", [("pendulum", torch.float64), ("pendulum", torch.float32), ("robotarm", torch.float64),
                                        ("quadrotor", torch.float64)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_sweeps_match_cubic_oracle(emu, kind, dtype):
    C.sweeps_vs_cubic_oracle(_prepare(emu), kind, dtype)


# ---- 3. API ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pend(emu):
    oc, env, d = models.pendulum(n_grid=8)
    emu(oc)
    oc.setDevice(dtype=torch.float64)
    c = C.SWEEP_CASES["pendulum"]
    th = np.asarray(c["thetas"], dtype=np.float64)
    sol = oc.cocSolverBatch(np.tile(d["ini_state"], (3, 1)), d["horizon"], th)
    return oc, d, c, th, sol


def test_skipped_rows_are_nan_at_level_2(pend):
    oc, d, c, th, sol = pend
    full = oc.auxSysSolverBatch(sol, c["taus"], c["wps"], d["interface"], want_grids=True, interplation_level=2)
    s2 = dict(sol)
    s2["status"] = torch.tensor([1, 4, 1], dtype=torch.int32)
    aux = oc.auxSysSolverBatch(s2, c["taus"], c["wps"], d["interface"], want_grids=True, interplation_level=2)
    for k in ("loss", "grad", "Z_grid", "auxX_grid", "auxU_grid"):
        assert bool(torch.isnan(aux[k][1]).all()), k
        assert torch.equal(aux[k][[0, 2]], full[k][[0, 2]]), k
    assert aux["stats"][1].tolist() == [0, 0, 0, 0]
    # ... and whatever statuses the caller names (a learner that freezes unconverged rows)
    s2["status"] = torch.tensor([3, 1, 2], dtype=torch.int32)
    aux = oc.auxSysSolverBatch(s2, c["taus"], c["wps"], d["interface"], skip_status=(3,), interplation_level=2)
    assert bool(torch.isnan(aux["loss"][0])) and bool(torch.isfinite(aux["loss"][1:]).all())


def test_aux_sys_solver_takes_the_cubic_interpolant_when_told_to(pend):
    oc, d, c, th, sol = pend
    n, m, p = 2, 1, 3
    N = c["n_grid"]
    try:
        tg, cubic = oc.cocSolver(d["ini_state"], d["horizon"], th[1], interplation_level=2)
        with pytest.raises(LfsdError, match="aux_interpolation"):      # the default refuses, and says which option changes that
            oc.auxSysSolver(tg, cubic, th[1])
        g = cubic(tg)
        user = sip.CubicSpline(tg, g, axis=0)
        with pytest.raises(LfsdError, match="aux_interpolation"):
            oc.auxSysSolver(tg, user, th[1])
        oc.setSolverOptions(aux_interpolation="as_given")
        a_tag = oc.auxSysSolver(tg, cubic, th[1])(tg)
        a_user = oc.auxSysSolver(tg, user, th[1])(tg)
        # the batched path's numbers
        batch = oc.auxSysSolverBatch(sol, want_grids=True, interplation_level=2)
        ref = np.concatenate((batch["auxX_grid"][1].numpy().transpose(0, 2, 1).reshape(N + 1, n * p),
                              batch["auxU_grid"][1].numpy().transpose(0, 2, 1).reshape(N + 1, m * p)), axis=1)
        assert np.allclose(a_tag, ref, rtol=1e-9, atol=1e-12)
        assert np.allclose(a_user, ref, rtol=1e-9, atol=1e-12)
        lin = oc.auxSysSolverBatch(sol, want_grids=True)
        assert not np.allclose(lin["auxX_grid"][1].numpy(), batch["auxX_grid"][1].numpy(), rtol=1e-3, atol=1e-6)
        # a linear interpolant is still differentiated along linearly
        a_lin = oc.auxSysSolver(tg, sip.interp1d(tg, g, axis=0), th[1])(tg)
        assert np.allclose(a_lin[:, :n * p], lin["auxX_grid"][1].numpy().transpose(0, 2, 1).reshape(N + 1, n * p), rtol=1e-9, atol=1e-12)
        # neither linear nor the not-a-knot spline: refused under either setting
        with pytest.raises(LfsdError):
            oc.auxSysSolver(tg, sip.CubicSpline(tg, g, axis=0, bc_type="clamped"), th[1])
        with pytest.raises(LfsdError):
            oc.setSolverOptions(aux_interpolation="cubic")
    finally:
        oc.setSolverOptions(aux_interpolation="linear")


def test_level_2_rows_do_not_depend_on_the_batch(pend):
    """The same row in batches of 1, 3 and 9: identical bits (curvature fit and both sweeps are per trajectory)."""
    oc, d, c, th, sol = pend
    keys = ("state_grid", "control_grid", "costate_grid", "horizon", "auxvar", "status")
    res = {}
    for B, at in ((1, 0), (3, 1), (9, 7)):
        idx = [(at + 1 + i) % 3 for i in range(B)]
        idx[at] = 1
        s = {k: sol[k][idx].contiguous() for k in keys}
        s["consts"] = sol["consts"]
        aux = oc.auxSysSolverBatch(s, c["taus"], c["wps"], d["interface"], want_grids=True, interplation_level=2)
        res[B] = {k: aux[k][at].clone() for k in ("loss", "grad", "Z_grid", "auxX_grid", "auxU_grid")}
        res[B]["curv"] = [t[at].clone() for t in aux["curvature"]]
    for B in (3, 9):
        for k in ("loss", "grad", "Z_grid", "auxX_grid", "auxU_grid"):
            assert torch.equal(res[B][k], res[1][k]), (B, k)
        for a, b in zip(res[B]["curv"], res[1]["curv"]):
            assert torch.equal(a, b), B


def test_level_1_is_the_old_entry_points_bit_for_bit(pend):
    """interp_level=1 (the default) of a library built from this tree == calling lfsd_aux_solve / lfsd_aux_riccati + lfsd_aux_forward
    directly with the ABI-10 argument lists."""
    oc, d, c, th, sol = pend
    lib = oc.compile()
    aux = oc.auxSysSolverBatch(sol, c["taus"], c["wps"], d["interface"], want_grids=True)
    assert aux["curvature"] is None
    B, N, n, m, p = 3, c["n_grid"], 2, 1, 3
    f64 = torch.float64
    tt = torch.tensor(c["taus"], dtype=f64).repeat(B, 1).contiguous()
    wp = torch.tensor(c["wps"], dtype=f64).repeat(B, 1, 1).contiguous()
    ii = torch.tensor(d["interface"], dtype=torch.int32)
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    for split in (False, True):
        Z = torch.empty((B, N + 1, n + p, n), dtype=f64)
        loss, grad = torch.zeros(B, dtype=f64), torch.zeros((B, p), dtype=f64)
        aX, aU = torch.empty((B, N + 1, p, n), dtype=f64), torch.empty((B, N + 1, p, m), dtype=f64)
        stats = torch.zeros((B, 4), dtype=torch.int32)
        common = (1, B, N, P(sol["horizon"]), P(sol["auxvar"]), P(sol["consts"]), 0, P(sol["state_grid"]), P(sol["control_grid"]),
                  P(sol["costate_grid"]), P(Z))
        tail = (tt.shape[1], 1, P(ii), P(tt), P(wp), P(loss), P(grad), P(aX), P(aU), oc.aux_substeps, oc.aux_rtol, P(stats),
                P(sol["status"]), 1 << 4, None)
        if split:
            assert lib.lib.lfsd_aux_riccati(*common, oc.aux_substeps, oc.aux_rtol, P(stats), P(sol["status"]), 1 << 4, None) == 0
            assert lib.lib.lfsd_aux_forward(*common, *tail) == 0
        else:
            assert lib.lib.lfsd_aux_solve(*common, *tail) == 0
        for k, t in (("loss", loss), ("grad", grad), ("Z_grid", Z), ("auxX_grid", aX), ("auxU_grid", aU), ("stats", stats)):
            assert torch.equal(aux[k], t), (split, k)
    # ... and the level-2 phases as separate launches are the one-call entry point
    one = oc.auxSysSolverBatch(sol, c["taus"], c["wps"], d["interface"], want_grids=True, interplation_level=2)
    two = oc.auxSysSolverBatch(sol, c["taus"], c["wps"], d["interface"], want_grids=True, interplation_level=2, phase_hook=lambda nm: None)
    for k in ("loss", "grad", "Z_grid", "auxX_grid", "auxU_grid", "stats"):
        assert torch.equal(one[k], two[k]), k
    with pytest.raises(LfsdError):
        oc.auxSysSolverBatch(sol, interplation_level=3)


def test_learner_runs_at_level_2(emu):
    """SparseDemoLearner(interplation_level=2): handed through to every step, with the stop rule's dense batch, warm starts, and in
    the shared-parameter mode; its losses are those of auxSysSolverBatch(..., interplation_level=2), not the linear ones."""
    oc, env, d = models.pendulum(n_grid=8)
    emu(oc)
    oc.setDevice(dtype=torch.float64)
    taus, wps = [0.1, 0.3, 0.6, 0.7, 0.9], [[0.4], [1.2], [2.1], [2.4], [2.9]]
    th0 = np.array([[1.0, 0.5, 1.5], [2.0, 1.0, 1.0], [0.7, 1.3, 0.6], [2.0, 1.0, 1.05]])
    x0 = np.tile(d["ini_state"], (4, 1))
    mk = lambda **kw: CPDP.SparseDemoLearner(oc, x0, d["horizon"], taus, wps, d["interface"], th0, learning_rate=1e-2, **kw)
    l1, _ = mk().step()
    lrn = mk(interplation_level=2)
    l2, g2 = lrn.step()
    sol = oc.cocSolverBatch(x0, d["horizon"], th0)
    ref = oc.auxSysSolverBatch(sol, taus, wps, d["interface"], interplation_level=2)
    assert torch.equal(l2, ref["loss"]) and torch.equal(g2, ref["grad"])
    assert bool(torch.isfinite(l2).all()) and not torch.allclose(l1, l2, rtol=1e-4)
    # stop rule (a threshold between the seeds' losses: the set shrinks after the first step) + warm start
    thr = float(l2.sort().values[1:3].mean())
    lrn = mk(interplation_level=2, stop_rule=dict(loss=thr, grad_norm=0.0), warm_start=True)
    la = lrn.step()[0].clone()               # (once seeds have stopped, step() returns the learner's own full-size buffers)
    assert torch.equal(la, l2) and 0 < lrn.n_active < 4
    lb, _ = lrn.step()
    act = lrn.active
    assert bool(torch.isfinite(lb).all()) and torch.equal(lb[~act], la[~act]) and not torch.equal(lb[act], la[act])
    free = mk(interplation_level=2, warm_start=True)
    free.step()
    lf, _ = free.step()
    assert torch.allclose(lb[act], lf[act], rtol=1e-7)      # (the dense batch restarts the same solves from the same controls)
    # shared mode: one theta, summed loss
    sh = CPDP.SparseDemoLearner(oc, x0, d["horizon"], taus, wps, d["interface"], th0[:1], mode="shared", interplation_level=2)
    ls, gs = sh.step()
    r0 = oc.auxSysSolverBatch(oc.cocSolverBatch(x0, d["horizon"], np.tile(th0[:1], (4, 1))), taus, wps, d["interface"], interplation_level=2)
    assert torch.allclose(ls, r0["loss"].sum().reshape(1), rtol=1e-12) and ls.shape == (1,) and gs.shape == (1, 3)
    with pytest.raises(LfsdError):
        mk(interplation_level=0)
