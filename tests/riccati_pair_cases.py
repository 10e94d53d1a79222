"""Shared cases of the pair-staging tests (tests/test_riccati_pair_stage_emu.py, tests/test_riccati_pair_stage_gpu.py): the fp32
Riccati sweep of the quadrotor with LFSD_RIC_PAIR_STAGE=1 (the product: the nine coefficient nodes of two consecutive split units
staged in one pass) against a build with LFSD_RIC_PAIR_STAGE=0 (every unit stages its own five).  The switch changes where the
coefficients are evaluated, never their values: every output must be EQUAL, bit for bit.

The sweeps integrate along whatever grids they are given, so the inputs are written down here (smooth state / control / costate
grids around the hover flight of models.quadrotor, one parameter vector per row) instead of solved for: the same numbers on the
emulator and on the GPU, and no OC solve in the way.

Shapes: n_grid 6, batch 5 -- two trajectories per wavefront, so rows 0/2/4 run on the lower and rows 1/3 on the upper half of a
wave, and the third wavefront is ragged (its upper half repeats the last row and must store nothing)."""
import numpy as np
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import models

KIND, N_GRID, BATCH = "quadrotor", 6, 5
HORIZON = 0.25            # (short: the rtol run takes seconds on the emulator; the last interval is still stiff -- four units at substeps 1)
OFF_FLAGS = ("-DLFSD_RIC_PAIR_STAGE=0",)
OFF_TAG = "ricpair0"
SKIP_ROW = 3                 # (an odd trajectory slot: the upper half of the second wavefront leaves, the lower half sweeps on)
# (aux_substeps, aux_rtol): one unit per interval (five-node passes only), an even count (pairs only), an odd count (a pair and a
# tail unit; thirds are not dyadic, so units whose shared node is not ONE fraction fall back to single passes), and error control
FIXED = ((1, 0.0), (2, 0.0), (3, 0.0))
RTOL = 1e-4
# Split units of the Riccati sweep per row (stats[:, 0]) that these inputs produce on the CPU emulator, recorded with the one-unit
# build when the inputs were chosen: at aux_substeps=1, aux_rtol=0 (the stiffness rule alone: four units in the last interval, one in each
# of the other five) and at aux_substeps=1, aux_rtol=RTOL.  The emulator tests assert them as they are, so a change of the inputs or of
# the error control that removed the redone intervals could not pass on the strength of assert_redone's bound alone.
EMU_UNITS_FIXED1 = [9, 9, 9, 9, 9]
EMU_UNITS_RTOL = [72, 76, 72, 72, 96]      # (assert_redone's no-redo bound for these rows: 48)


def make_oc(n_grid=N_GRID):
    oc, _, d = models.quadrotor(n_grid=n_grid)
    return oc, d


def inputs(d, device, dtype=torch.float32, batch=BATCH, n_grid=N_GRID, horizon=HORIZON):
    """dict(horizon, auxvar, state_grid, control_grid, costate_grid, taus, waypoints, iface): deterministic, written in fp64 and
    rounded once."""
    rng = np.random.RandomState(20240917)
    s = np.linspace(0.0, 1.0, n_grid + 1)[None, :, None]
    x0 = np.asarray(d["ini_state"], dtype=np.float64)
    xN = np.array([3, 3, 1.5, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0], dtype=np.float64)
    amp = 0.2 + 0.1 * np.arange(batch)[:, None, None]
    ph = rng.uniform(0, 2 * np.pi, size=(batch, 1, 13))
    X = x0 + (xN - x0) * (3 * s ** 2 - 2 * s ** 3) + amp * np.sin(np.pi * s) * np.cos(2.0 * s + ph)
    X[:, :, 6:10] /= np.linalg.norm(X[:, :, 6:10], axis=2, keepdims=True)
    U = 2.45 + 0.8 * np.sin(3.0 * s + rng.uniform(0, 2 * np.pi, size=(batch, 1, 4))) * (1 + 0.2 * np.arange(batch)[:, None, None])
    L = (1.0 - 0.6 * s) * rng.uniform(-2.0, 2.0, size=(batch, 1, 13)) + 0.3 * np.sin(4.0 * s + ph)
    theta = np.asarray(d["theta0"], dtype=np.float64)[None, :] * (1.0 + 0.15 * np.arange(batch)[:, None])
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=device)
    return dict(horizon=t(np.full(batch, horizon)), auxvar=t(theta), state_grid=t(X), control_grid=t(U), costate_grid=t(L),
                taus=np.asarray(d["taus"]) * horizon, waypoints=d["waypoints"], iface=d["interface"])


def run(oc, inp, substeps, rtol, skip_row=None):
    """One auxSysSolverBatch along the given grids.  skip_row: that row carries status FAILED and is not differentiated."""
    B = inp["state_grid"].shape[0]
    status = torch.ones(B, dtype=torch.int32, device=inp["state_grid"].device)
    if skip_row is not None:
        status[skip_row] = 4
    sol = dict(horizon=inp["horizon"], auxvar=inp["auxvar"], consts=oc.consts_tensor(), state_grid=inp["state_grid"],
               control_grid=inp["control_grid"], costate_grid=inp["costate_grid"], status=status)
    oc.setSolverOptions(aux_substeps=substeps, aux_rtol=rtol)
    out = oc.auxSysSolverBatch(sol, inp["taus"], inp["waypoints"], inp["iface"], skip_status=(4,))
    return {k: out[k].clone() for k in ("Z_grid", "stats", "loss", "grad")}


def assert_same(a, b, what, skip_row=None):
    rows = [r for r in range(a["loss"].shape[0]) if r != skip_row]
    for k in ("Z_grid", "stats", "loss", "grad"):
        assert torch.equal(a[k][rows], b[k][rows]), "%s: %s differs between the pair-staging build and the one-unit build" % (what, k)
        assert k == "stats" or bool(torch.isfinite(a[k][rows]).all()), "%s: %s is not finite" % (what, k)
    if skip_row is not None:
        for o in (a, b):
            assert bool(torch.isnan(o["Z_grid"][skip_row]).all()) and bool(torch.isnan(o["loss"][skip_row])) \
                and bool(torch.isnan(o["grad"][skip_row]).all()), what + ": a skipped row returns NaN"
            assert o["stats"][skip_row].tolist() == [0, 0, 0, 0], what + ": a skipped row spends no units"


def assert_redone(fixed1, out, n_grid=N_GRID):
    """At least one row of the error-controlled run (aux_substeps=1) has redone an interval with doubled units -- seen from `stats`
    alone.  `fixed1`, the run at aux_substeps=1 and aux_rtol=0, has no error control and no carried-over unit count: interval k runs the
    u0_k units of the stiffness rule (the smallest power of two with dt x rate / u0_k <= 8), and a row's total U0 bounds the largest of
    them by U0 - (n_grid - 1).  At aux_rtol=1e-4 the cap is 8 / 10^(1/4) = 4.5, so the stiffness rule asks for at most 2 u0_k (the
    power of two above 1.78 x what it asked for; the two runs' P differ by the integration error, far inside the factor 2 / 1.78), and
    an interval otherwise starts from at most the units the interval before it ended with.  Without a rejected attempt no interval
    of a row therefore runs more than 2 (U0 - n_grid + 1) units: a row whose total is above n_grid times that has redone one."""
    u0 = fixed1["stats"][:, 0].tolist()
    u = out["stats"][:, 0].tolist()
    bound = [2 * n_grid * (v - (n_grid - 1)) for v in u0]
    assert any(a > b for a, b in zip(u, bound)), "no interval was redone at aux_rtol=%g: units %s, no-redo bounds %s" % (RTOL, u, bound)
    return u
