"""CPU tier of waypoint weights and ragged demonstrations (ABI 16): the weighted forward sweeps and lfsd_normal_matrix_weighted through the
SIMT emulator -- NULL and all-ones weights, zero weights, powers of two, bit for bit; general weights against an fp64 restatement and
against the oracle; the learner with ragged rows against learners on the compacted lists and against its launches made by hand; the
refusals; every LFSD_EINVAL case on host dummies (emulator and gfx950 library).  Cases and bounds: tests/weight_cases.py."""
import os
import subprocess

import numpy as np
import pytest
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models, runtime
from lfsd_amd.runtime import LfsdError
from conftest import TIGHT, build_emu_library, make_oracle, parity_record
import hyper_sweep_cases as H
import weight_cases as C

F64 = torch.float64


def prepare(oc, dtype):
    oc.use_library(build_emu_library(oc))
    oc.compile()
    oc.setDevice(dtype=dtype)


# ---- 1.-3. the kernels, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.KERNEL_CASES_EMU, ids=C.CASE_ID)
def test_null_ones_zero_and_power_of_two_weights_are_exact(case):
    C.run_kernel_case(prepare, "cpu", case)


# ---- 4. general weights against the fp64 restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.KERNEL_CASES_EMU, ids=C.CASE_ID)
def test_general_weights_against_fp64_restatement(case):
    """Worst fractions of the bounds seen on the emulator: loss 0.19, gradient 0.038, H 0.047 (bounds: tests/weight_cases.py; DESIGN.md
    section 16)."""
    fl, fg, fh = C.run_general_weights(prepare, "cpu", case)
    print("%s: |loss - ref| / bound %.3f, |grad - ref| / bound %.3f, |H - ref| / bound %s" % (C.CASE_ID(case), fl, fg, fh))
    assert fl <= 1.0 and fg <= 1.0 and (fh is None or fh <= 1.0), (fl, fg, fh)


# ---- 5. against the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pendulum", "quadrotor"])
def test_weighted_loss_is_the_weighted_sum_of_the_oracles_waypoints(kind):
    """Loss and gradient are linear in the per-waypoint terms: sum_k w_k x (the oracle's loss and gradient for waypoint k alone), at
    parity_cases' fp64 tolerance for the unweighted loss and gradient (1e-6, 1e-4)."""
    n_grid = 10
    oc, d, iface = C.make_model(kind, n_grid)
    prepare(oc, F64)
    oc.setSolverOptions(aux_substeps=16)
    th = np.asarray([1.0, 0.5, 1.5] if kind == "pendulum" else d["theta0"], dtype=np.float64)
    hz = float(d["horizon"])
    taus = np.array([0.1, 0.45, 0.8]) * hz
    wps = np.array([[0.4], [1.2], [2.4]]) if kind == "pendulum" else np.asarray(d["waypoints"], dtype=np.float64)[:3]
    w = np.array([0.3, 2.5, 0.0 if kind == "pendulum" else 1.7])
    sol = oc.cocSolverBatch(np.asarray(d["ini_state"], dtype=np.float64)[None, :], hz, th[None, :])
    aux = oc.auxSysSolverBatch(sol, taus, wps, iface, waypoint_weights=w)
    from oracle.cpdp_oracle import getloss_corrections
    o = make_oracle(kind, n_grid)
    tg, osol = o.cocSolver(np.asarray(d["ini_state"], dtype=np.float64), hz, th)
    oaux = o.auxSysSolver(tg, osol, th, **TIGHT)
    l_o, g_o = 0.0, 0.0
    for k in range(3):                                          # (one oracle solve; the loss of each waypoint alone)
        lk, gk = getloss_corrections(o, taus[k:k + 1], wps[k:k + 1], osol, oaux, iface)
        l_o, g_o = l_o + w[k] * lk, g_o + w[k] * np.asarray(gk, dtype=np.float64).reshape(-1)
    parity_record("weighted %s" % kind, "loss", abs(float(aux["loss"][0]) - l_o) / max(1.0, abs(l_o)), 1e-6)
    parity_record("weighted %s" % kind, "grad", float(np.abs(aux["grad"][0].double().numpy() - g_o).max() / max(np.abs(g_o).max(), 1e-300)), 1e-4)


# ---- 6. the learner ----------------------------------------------------------------------------------------------------------------
ROWS = 8


def _pendulum(rows=ROWS, n_grid=10):
    oc, args, lam0 = C.learner_problem(prepare, "pendulum", rows, F64, n_grid)

    def make(rows=None, k=None, **kw):
        sel = list(range(len(args[0]))) if rows is None else rows
        taus, wps = (args[2], args[3]) if k is None else (args[2][:k], args[3][:k])
        return CPDP.SparseDemoLearner(oc, args[0][sel], args[1], taus, wps, args[4], args[5][sel], **kw)
    return oc, args, lam0, make


@pytest.mark.parametrize("rule", C.RULES, ids=[r[0] for r in C.RULES])
def test_ragged_rows_walk_the_path_of_their_own_learners(rule):
    oc, args, lam0, make = _pendulum()
    C.run_ragged_independent(make, ROWS, rule, lam0)


def test_grouped_learner_with_padded_demonstrations_is_its_launches():
    oc, args, lam0, make = _pendulum(rows=2)
    G, D = 2, 3
    tl, wl = C.ragged_lists(args)
    taus, wps, wts = CPDP.pad_demonstrations(tl, wl)
    assert taus.shape == (D, C.K) and wps.shape == (D, C.K, 1) and np.isnan(taus[1, 3:]).all() and np.isnan(wps[2, 1:]).all()
    assert wts.tolist() == [[1] * 5, [1, 1, 1, 0, 0], [1, 0, 0, 0, 0]]
    x0 = np.tile(args[0][:1], (D, 1)) + np.array([[0.0, 0.0], [0.2, 0.0], [-0.1, 0.1]])
    gargs = (x0, args[1], taus, wps, args[4], args[5])
    L = CPDP.SparseDemoLearner(oc, *gargs, method="Vanilla", learning_rate=1e-2, mode="grouped", demos_per_seed=D, waypoint_weights=wts)
    assert L.B == G * D and tuple(L.wts.shape) == (G * D, C.K) and torch.equal(L.wts[:D], L.wts[D:])
    hand = C.grouped_by_hand(oc, gargs, G, D, wts, C.STEPS, L.proj_lo, 1e-2)
    th0 = L.theta.clone()
    for k in range(C.STEPS):
        loss, grad = L.step()
        th, lg, gg, n_ok = next(hand)
        assert torch.equal(L.theta, th) and torch.equal(loss, lg) and torch.equal(grad, gg) and torch.equal(L.n_ok, n_ok), k
    assert bool((L.theta != th0).any()) and bool(torch.isfinite(loss).all()) and int(L.n_ok.sum()) > 0
    # the same numbers through n_waypoints per demonstration on taus / waypoints padded with anything finite
    L2 = CPDP.SparseDemoLearner(oc, x0, args[1], np.nan_to_num(taus, nan=0.5), np.nan_to_num(wps, nan=7.0), args[4], args[5],
                                method="Vanilla", learning_rate=1e-2, mode="grouped", demos_per_seed=D, n_waypoints=[5, 3, 1])
    for k in range(C.STEPS):
        L2.step()
    assert torch.equal(L2.theta, L.theta)


def test_stop_rule_gathers_the_weights_with_the_rows():
    """6c: a row that stops; the survivors' traces equal the never-stopping run's up to each row's stop_iter."""
    oc, args, lam0, make = _pendulum()
    counts = [C.COUNTS[b % 3] for b in range(ROWS)]
    kw = dict(method="Vanilla", learning_rate=1e-2, n_waypoints=counts, trace=C.STEPS)
    free = make(**kw)
    for _ in range(C.STEPS):
        free.step()
    # thresholds between the rows' losses after two steps: some rows stop early, others go on
    l2 = free.loss_trace[:, 1]
    tol = float(l2.sort().values[ROWS // 2 - 1: ROWS // 2 + 1].mean())
    stop = make(stop_rule=dict(loss=tol, grad_norm=0.0), **kw)
    for _ in range(C.STEPS):
        stop.step()
    it = stop.stop_iter.tolist()
    first = min([i for i in it if i > 0] + [C.STEPS])
    assert first < C.STEPS and any(i == 0 or i > first for i in it), it      # a row stops, and others go on after it
    assert stop._dense is not None and "wts" in stop._dense
    for b in range(ROWS):
        n = it[b] if it[b] > 0 else C.STEPS
        assert torch.equal(stop.loss_trace[b, :n], free.loss_trace[b, :n]) and torch.equal(stop.theta_trace[b, :n + 1], free.theta_trace[b, :n + 1]), b
        assert bool(torch.isnan(stop.loss_trace[b, n:]).all())


def test_shared_mode_sums_the_weighted_rows():
    """6d: one step against the sum made by hand."""
    oc, args, lam0, make = _pendulum(rows=1)
    rows = 4
    x0 = np.tile(args[0][:1], (rows, 1)) + 0.1 * np.arange(rows)[:, None]
    counts = [5, 3, 1, 3]
    L = CPDP.SparseDemoLearner(oc, x0, args[1], args[2], args[3], args[4], args[5][:1], method="Vanilla", learning_rate=1e-2,
                               mode="shared", n_waypoints=counts)
    th0 = L.theta.clone()
    loss, grad = L.step()
    sol = oc.cocSolverBatch(x0, args[1], th0.expand(rows, -1).contiguous())
    aux = oc.auxSysSolverBatch(sol, args[2], args[3], args[4], waypoint_weights=L.wts, skip_status=(3, 4))
    assert L._ok is not None and bool(L._ok.all())
    assert torch.equal(loss, aux["loss"].sum().reshape(1)) and torch.equal(grad, aux["grad"].sum(dim=0, keepdim=True))
    th = th0.clone()
    z = torch.zeros_like(th)
    oc.compile().optimizer_step("Vanilla", th, grad, 0, 1e-2, m=z.clone(), v=z.clone(), vhat=z.clone(), proj_lo=L.proj_lo)
    assert torch.equal(L.theta, th) and bool((th != th0).any())


def test_level_2_takes_the_weights():
    """6e: one step of interplation_level=2 against the cubic weighted sweep called by hand, and against its compacted learner."""
    oc, args, lam0, make = _pendulum(rows=3)
    L = make(method="Vanilla", learning_rate=1e-2, n_waypoints=[5, 3, 1], interplation_level=2)
    th0 = L.theta.clone()
    loss, grad = L.step()
    sol = oc.cocSolverBatch(args[0], args[1], th0)
    aux = oc.auxSysSolverBatch(sol, args[2], args[3], args[4], waypoint_weights=L.wts, interplation_level=2)
    assert torch.equal(loss, aux["loss"]) and torch.equal(grad, aux["grad"])
    lin = oc.auxSysSolverBatch(sol, args[2], args[3], args[4], waypoint_weights=L.wts)
    assert not torch.equal(lin["loss"], aux["loss"])
    S = make(rows=[1], k=3, method="Vanilla", learning_rate=1e-2, interplation_level=2)
    l3, g3 = S.step()
    assert torch.equal(l3, loss[1:2]) and torch.equal(g3, grad[1:2]) and torch.equal(S.theta, L.theta[1:2])


def test_without_weights_the_learner_takes_the_launches_it_took(monkeypatch):
    """6f: no weights given -- the unweighted entry points, the call counts of today (as test_lm_emu's launch test)."""
    oc, args, lam0, make = _pendulum(rows=2)
    ml = oc.compile()
    calls = C.launch_spy(ml, monkeypatch)
    for name, kw in C.RULES:
        L = make(**kw)
        assert L.wts is None
        L.step(); L.step()
        want = {"aux_solve": 2, "normal_matrix": 2, "lm_step": 2} if name == "LM" else {"aux_solve": 2, "optimizer_step": 2}
        assert calls == want, (name, calls)
        calls.clear()
    L = make(method=["Adam", "Vanilla"], learning_rate=1e-2, stop_rule=dict(loss=0.0, grad_norm=0.0), interplation_level=2)
    L.step()
    assert calls == {"aux_solve": 1, "optimizer_step_rows": 1}
    calls.clear()
    # ... and with weights the same number of launches through the binding, the weighted entry points underneath
    monkeypatch.undo()
    seen = []
    fwd = ml.lib.lfsd_aux_forward_weighted
    monkeypatch.setattr(ml.lib, "lfsd_aux_forward_weighted", lambda *a: (seen.append("fwd"), fwd(*a))[1])
    nm = ml.lib.lfsd_normal_matrix_weighted
    monkeypatch.setattr(ml.lib, "lfsd_normal_matrix_weighted", lambda *a: (seen.append("H"), nm(*a))[1])
    L = make(method="LM", n_waypoints=[5, 3])
    L.step()
    assert seen == ["fwd", "H"]


# ---- 7. refusals and the ABI -------------------------------------------------------------------------------------------------------
def test_learner_and_helpers_refuse_what_they_cannot_mean():
    oc, args, lam0, make = _pendulum(rows=3)
    bad = [dict(waypoint_weights=[1.0] * 5, n_waypoints=3),                                 # both
           dict(waypoint_weights=[1.0] * 5, loss_fn=lambda x, u: x.sum((1, 2))),            # a user loss does its own weighting
           dict(n_waypoints=3, loss_fn=lambda x, u: x.sum((1, 2))),
           dict(waypoint_weights=[1.0, 1.0, -0.5, 1.0, 1.0]), dict(waypoint_weights=[1.0, float("nan"), 1.0, 1.0, 1.0]),
           dict(waypoint_weights=[1.0, float("inf"), 1.0, 1.0, 1.0]),
           dict(waypoint_weights=[1.0] * 4), dict(waypoint_weights=np.ones((2, 5))), dict(waypoint_weights=np.ones((3, 5, 1))),
           dict(waypoint_weights=np.ones((5, 3))),
           dict(n_waypoints=6), dict(n_waypoints=-1), dict(n_waypoints=[5, 3]), dict(n_waypoints=[5, 3, 6]), dict(n_waypoints=2.5),
           dict(n_waypoints=np.ones((3, 1), dtype=int))]
    for kw in bad:
        with pytest.raises(LfsdError):
            make(method="Vanilla", **kw)
    with pytest.raises(LfsdError):                                                          # [D, K] belongs to grouped mode
        CPDP.SparseDemoLearner(oc, args[0][:2], *args[1:5], args[5][:2], waypoint_weights=np.ones((1, 5)))
    # zero-weight entries are exempt from the range check, the others are not
    taus = np.array(args[2], dtype=np.float64)
    taus[3] = float("nan")
    taus[4] = 5.0 * args[1]
    L = make(method="Vanilla", n_waypoints=3, **{})
    L2 = CPDP.SparseDemoLearner(oc, args[0], args[1], taus, args[3], args[4], args[5], n_waypoints=3)
    l1, _ = L.step()
    l2, _ = L2.step()
    assert torch.equal(l1, l2)
    for kw in (dict(n_waypoints=4), dict(n_waypoints=5), dict(waypoint_weights=[1, 1, 1, 0, 1e-3]), {}):
        with pytest.raises(ValueError):
            CPDP.SparseDemoLearner(oc, args[0], args[1], taus, args[3], args[4], args[5], **kw)
    sol = oc.cocSolverBatch(args[0], args[1], args[5])
    with pytest.raises(LfsdError):
        oc.auxSysSolverBatch(sol, args[2], args[3], args[4], waypoint_weights=[1, 1, 1, 1, -1])
    with pytest.raises(LfsdError):
        oc.auxSysSolverBatch(sol, args[2], args[3], args[4], waypoint_weights=np.ones((3, 4)))
    with pytest.raises(LfsdError):
        oc.auxSysSolverBatch(sol, waypoint_weights=[1.0])
    for lists in (([], []), ([[0.1]], [[[1.0]], [[2.0]]]), ([[0.1, 0.2]], [[[1.0]]]), ([[0.1]], [[[1.0]]], [[1.0, 2.0]]), ([[0.1]], [[[1.0]]], [[-1.0]])):
        with pytest.raises(LfsdError):
            CPDP.pad_demonstrations(*lists)
    t, w, wt = CPDP.pad_demonstrations([[0.1, 0.2], [0.3]], [[[1.0, 2.0], [3.0, 4.0]], [[5.0, 6.0]]], [[0.5, 2.0], [3.0]])
    assert w.shape == (2, 2, 2) and wt.tolist() == [[0.5, 2.0], [3.0, 0.0]] and np.isnan(t[1, 1]) and t[1, 0] == 0.3


def test_the_driver_passes_the_weights_through():
    import inspect
    from lfsd_amd import QuadAlgorithm
    for fn in (QuadAlgorithm.QuadAlgorithm.run, QuadAlgorithm.QuadAlgorithm.run_comparison):
        assert inspect.signature(fn).parameters["waypoint_weights"].default is None


@pytest.mark.parametrize("which,kind", [("emulator", "pendulum"), ("emulator", "general"), ("hip", "pendulum")])
def test_entry_points_refuse_bad_arguments_before_any_launch(which, kind):
    """Host dummies stand in for the arrays: no launch is reached (the gfx950 library loads without a GPU, as in tests/test_capi.py).
    The gfx950 tier takes a library of the standard build; the model with a compiled-in interface is no part of it and is checked
    on the emulator build (the argument checks are the same host code)."""
    oc, d, iface = C.make_model(kind, 10)
    ml = runtime.ModelLibrary(build_emu_library(oc)) if which == "emulator" else oc.compile()
    C.weighted_einval(ml.lib, ml.n_state, ml.n_control, ml.n_auxvar, compiled_iface=iface is None)
    z = lambda *s: torch.zeros(s, dtype=F64)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    if which == "hip":                                          # no CPU fallback: host memory is refused by the binding
        with pytest.raises(LfsdError):
            ml.normal_matrix(z(2), z(2, 3), z(2, 4, 3, 2), i32(1), wp_weight=z(2, 3))
        return
    for bad in (lambda: ml.normal_matrix(z(2), z(2, 3), z(2, 4, 3, 2), i32(1), wp_weight=z(2, 2)),
                lambda: ml.normal_matrix(z(2), z(2, 3), z(2, 4, 3, 2), i32(1), wp_weight=z(2, 3).float()),
                lambda: ml.normal_matrix(z(2), z(2, 3), z(2, 4, 3, 2), i32(1), wp_weight=z(3, 2).T)):
        with pytest.raises(LfsdError):
            bad()


# ---- 8. AddressSanitizer + UBSan over the three entry points, in a stand-alone program --------------------------------------------
def test_weighted_entry_points_asan_ubsan_clean(tmp_path):
    """tests/emu/sanitize_weights_main.cpp (CPU SIMT-emulator build with its own main, as tests/test_groups_sanitize.py builds its
    program): NULL, all-zero and mixed weights with poisoned padding, both levels and precisions, exact-size heap buffers and guard
    words; run as a child process -- nothing is loaded into Python under a sanitizer."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    emu_dir = os.path.join(root, "tests", "emu")
    oc, _, _ = models.ZOO["pendulum"]()
    spec = oc.model_spec()
    runtime.write_header(spec)
    exe = str(tmp_path / "sanitize_weights")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-DLFSD_EMU",
           "-DLFSD_G=%d" % runtime.lanes_for(spec.n, spec.m, spec.p), "-I" + emu_dir, "-I" + runtime.CSRC_DIR,
           '-DLFSD_MODEL_HEADER="gen/%s.h"' % spec.hash(), os.path.join(emu_dir, "sanitize_weights_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, cwd=runtime.CSRC_DIR, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_stack_use_after_return=0:detect_leaks=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=1200)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.count("weights rc 0 wrong 0") == 2, r.stdout
