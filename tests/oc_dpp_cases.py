"""Shared cases of the register-exchange tests of the lean fp32 OC kernel (tests/test_oc_dpp_xchg_emu.py, tests/test_oc_dpp_xchg_gpu.py):
the product build (LFSD_OC_DPP_XCHG=1, csrc/cpdp_common.h: the per-stage hand-overs of OcSolver::backward_sc and costate_sweep_sc inside
a 16-lane group are row broadcasts in registers) against a build with -DLFSD_OC_DPP_XCHG=0 (the same values through LDS).  The switch
moves data and leaves every floating-point operation, its operands and its order alone: every output must be EQUAL, bit for bit.

All cases: fp32, mapping forced to lock-step (four trajectories per wavefront, one 16-lane group each), cold start unless said.
  grid20    quadrotor, n_grid 20, batch 8: rows 1 and 6 are copies of row 0 (another slot of the same wavefront, and another wavefront)
            and must also equal each other bit for bit -- what a group receives never depends on its partners
  grid24    quadrotor, n_grid 24, batch 4: the smallest even grid on which level 0 of the mesh continuation runs (kLeanTcMin = 12
            merged intervals; n_grid 20 merges to 10 and starts one level up)
  grid10    quadrotor, n_grid 10, batch 5: a ragged second wavefront -- three padded groups ride along and feed the broadcasts
  grid21    quadrotor, odd n_grid 21 (no level 0), batch 4, row 2 with an initial guess and all-zero rows beside it: the warm / cold
            mix of a learner that continues some solves
  maxiter3  quadrotor, n_grid 20, batch 4 at max_iter 3: rows 0, 1, 3 start from grid20's answers and finish at once, row 2 starts
            cold and is still running when the launch ends -- a finished partner beside an unfinished one
  rocket    rocket, n_grid 20, batch 4, Gauss-Newton / Hamiltonian iterations only (exact_after=-1, max_iter 8): the same template on
            13 live columns and 3 controls"""
import numpy as np
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import models

OFF_FLAGS = ("-DLFSD_OC_DPP_XCHG=0",)
OFF_TAG = "ocdpp0"
KEYS = ("state_grid", "control_grid", "costate_grid", "cost", "iters", "status")
CASES = ("grid20", "grid24", "grid10", "grid21", "maxiter3", "rocket")
# (kind, n_grid, batch)
SHAPES = dict(grid20=("quadrotor", 20, 8), grid24=("quadrotor", 24, 4), grid10=("quadrotor", 10, 5), grid21=("quadrotor", 21, 4),
              maxiter3=("quadrotor", 20, 4), rocket=("rocket", 20, 4))
MAXITER3_ROWS = (0, 2, 3, 4)      # rows of grid20 that maxiter3 solves again
MAXITER3_COLD = 2                 # ... its row that starts cold


def make_oc(case):
    kind, n_grid, _ = SHAPES[case]
    oc, _, d = models.ZOO[kind](n_grid=n_grid)
    oc.setSolverOptions(mapping="lockstep")
    if case == "maxiter3":
        oc.setSolverOptions(max_iter=3)
    if case == "rocket":
        oc.setSolverOptions(exact_after=-1, max_iter=8)
    return oc, d


def problem(case, d):
    """(ini_state [B][n], theta [B][p]) of a case, deterministic."""
    kind, n_grid, batch = SHAPES[case]
    if case == "maxiter3":
        x0, th = problem("grid20", d)
        return x0[list(MAXITER3_ROWS)], th[list(MAXITER3_ROWS)]
    rng = np.random.default_rng(100 + CASES.index(case))
    if kind == "rocket":
        th = np.asarray(d["theta0"], dtype=float)[None, :] * (1 + 0.2 * rng.uniform(0, 1, (batch, len(d["theta0"]))))
        x0 = np.tile(np.asarray(d["ini_state"], dtype=float), (batch, 1))
        x0[:, :3] += 0.5 * rng.standard_normal((batch, 3))
        return x0, th
    th = np.asarray(d["theta0"], dtype=float)[None, :] * (1 + 0.1 * rng.standard_normal((batch, len(d["theta0"]))))
    th[:, 0] = np.abs(th[:, 0]) + 0.2
    x0 = np.tile(np.asarray(d["ini_state"], dtype=float), (batch, 1))
    x0[:, :3] += 0.3 * rng.standard_normal((batch, 3))
    if case == "grid20":
        th[1], x0[1] = th[0], x0[0]
        th[6], x0[6] = th[0], x0[0]
    return x0, th


def u_init(case, device, grid20_sol=None):
    """The initial guess of a case (None: cold)."""
    kind, n_grid, batch = SHAPES[case]
    if case == "grid21":
        s = torch.linspace(0.0, 1.0, n_grid, dtype=torch.float64)[:, None]
        u = torch.zeros(batch, n_grid, 4, dtype=torch.float64)
        u[2] = 2.45 + 0.3 * torch.sin(3.0 * s + torch.arange(4, dtype=torch.float64)[None, :])
        return u.to(device=device, dtype=torch.float32).contiguous()
    if case == "maxiter3":
        u = grid20_sol["control_grid"][list(MAXITER3_ROWS), :n_grid].clone()
        u[MAXITER3_COLD] = 0
        return u.to(device).contiguous()
    return None


def solve(oc, d, case, device, grid20_sol=None):
    x0, th = problem(case, d)
    sol = oc.cocSolverBatch(x0, d["horizon"], th, u_init=u_init(case, device, grid20_sol))
    return sol


def assert_same(a, b, what):
    for k in KEYS:
        assert torch.equal(a[k], b[k]), "%s: %s differs between the register-exchange build and the LDS build" % (what, k)


def assert_case(case, a, b):
    """What a case asks of the pair of solutions beyond being equal."""
    assert_same(a, b, case)
    st = a["status"].tolist()
    if case in ("grid20", "grid24", "grid10", "grid21"):
        assert set(st) <= {1, 2}, (case, st)
        assert bool(torch.isfinite(a["costate_grid"]).all())
    if case == "grid20":
        for o in (a, b):
            for k in KEYS:
                assert torch.equal(o[k][0], o[k][1]) and torch.equal(o[k][0], o[k][6]), "grid20: copies of row 0 differ in " + k
    if case == "maxiter3":
        cold = MAXITER3_COLD
        assert st[cold] == 3 and a["iters"][cold].item() == 3, (st, a["iters"].tolist())
        assert all(st[r] in (1, 2) and a["iters"][r].item() < 3 for r in range(4) if r != cold), (st, a["iters"].tolist())
    if case == "rocket":
        assert bool(torch.isfinite(a["cost"]).all()) and max(a["iters"].tolist()) == 8, (st, a["iters"].tolist())
