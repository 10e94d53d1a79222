"""CPU tier of the Levenberg-Marquardt step over parameters and waypoint times (ABI 18): lfsd_time_normal_blocks and lfsd_lm_step_times
through the SIMT emulator against fp64 restatements / known branches; every LFSD_EINVAL case on host dummies (emulator and gfx950
library); the learner with lm_taus against the same launches made by hand, bit for bit; its combinations and refusals; recovery of
known parameters and times against an fp64 numpy loop.  Cases and bounds: tests/lm_times_cases.py."""
import numpy as np
import pytest
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models, runtime
from lfsd_amd.runtime import LfsdError
from conftest import build_emu_library
import hyper_sweep_cases as H
import lm_cases as LC
import lm_times_cases as C

F64 = torch.float64
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, F64], ids=["fp32", "fp64"])
SHAPES = pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "B%dp%dK%d" % s)
GROUPS = pytest.mark.parametrize("shape", C.GROUPS, ids=lambda s: "G%dD%dp%dK%d" % s)


@pytest.fixture(scope="module")
def lib():
    return runtime.ModelLibrary(build_emu_library(models.pendulum(n_grid=10)[0]))


@pytest.fixture(scope="module")
def qlib():
    return runtime.ModelLibrary(build_emu_library(models.quadrotor(n_grid=10)[0]))


# ---- 1. kernels -----------------------------------------------------------------------------------------------------------------
@DTYPES
@SHAPES
def test_time_blocks_against_fp64_restatement(lib, shape, dtype):
    B, p, K = shape
    worst = 0.0
    for n_grid in C.N_GRIDS:
        for cubic in ((False, True) if n_grid >= 3 else (False,)):
            r = C.run_time_blocks(lib, "cpu", dtype, B, p, K, n_grid, cubic)
            print("time_blocks B%d p%d K%d n_grid %d level %d: worst fraction of the bound %.3f" % (B, p, K, n_grid, 2 if cubic else 1, r))
            assert r <= 1.0, (n_grid, cubic, r)
            worst = max(worst, r)
    print("time_blocks B%d p%d K%d: worst %.3f" % (B, p, K, worst))


@DTYPES
@pytest.mark.parametrize("shape", C.SHAPES[:3], ids=lambda s: "B%dp%dK%d" % s)
def test_arrow_matrix_is_the_gram_matrix_of_the_augmented_jacobian(lib, qlib, shape, dtype):
    B, p, K = shape
    for n_grid, cubic in ((1, False), (10, False), (3, True), (10, True)):
        r = C.run_arrow_identity(lib, "cpu", dtype, B, p, K, n_grid, cubic, tg_lib=qlib)
        print("arrow identity B%d p%d K%d n_grid %d level %d: worst fraction of the summed bounds %.3f" % (B, p, K, n_grid, 2 if cubic else 1, r))
        assert r <= 1.0, (n_grid, cubic, r)


@DTYPES
@SHAPES
def test_lm_step_times_walks_the_known_branches(lib, shape, dtype):
    B, p, K = shape
    for offset in (range(0, 3 * C.KINDS, 1) if B < 2 * C.KINDS else (0,)):
        worst, worst_np = C.run_lm_step_times(lib, "cpu", dtype, B, 1, p, K, offset)
        assert worst_np <= 1.0, ("the numpy elimination in the dtype", offset, worst_np)
        assert worst <= 1.0, (offset, worst)
    print("lm_step_times B%d p%d K%d: worst backward error / bound %.3f (numpy elimination in the dtype %.3f)" % (B, p, K, worst, worst_np))


@DTYPES
@GROUPS
def test_lm_step_times_grouped(lib, shape, dtype):
    G, D, p, K = shape
    for offset in (range(0, 3 * C.KINDS, 1) if G < 2 * C.KINDS else (0, 3)):
        worst, worst_np = C.run_lm_step_times(lib, "cpu", dtype, G, D, p, K, offset)
        assert worst_np <= 1.0, ("the numpy elimination in the dtype", offset, worst_np)
        assert worst <= 1.0, (offset, worst)
    print("lm_step_times G%d D%d p%d K%d: worst backward error / bound %.3f (numpy elimination in the dtype %.3f)" % (G, D, p, K, worst, worst_np))


@pytest.mark.parametrize("which", ["emulator", "hip"])
def test_entry_points_refuse_bad_arguments_before_any_launch(lib, which):
    ml = lib if which == "emulator" else models.pendulum(n_grid=10)[0].compile()
    C.time_blocks_einval(ml.lib)
    C.lm_step_times_einval(ml.lib)
    z = lambda *s: torch.zeros(s, dtype=F64)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    step = lambda **kw: ml.lm_step_times(z(2, 3), z(2), z(2, 3), z(2, 3, 3), z(2), z(2, 3), kw.pop("tau", z(4, 2)), z(4, 2), z(4, 2), z(4, 2, 3),
                                         z(4, 2), kw.pop("ok", i32(4)), z(2), z(2, 3), z(2, 3, 3), z(4, 2), z(4, 2, 3), z(4, 2),
                                         group_size=kw.pop("D", 2), **kw)
    if which == "hip":                                          # no CPU fallback: the HIP library refuses host memory
        with pytest.raises(LfsdError):
            ml.time_normal_blocks(z(2, 4, 2), z(2), z(2, 3), z(2, 4, 3, 2), i32(1))
        with pytest.raises(LfsdError):
            step()
        return
    for bad in (lambda: ml.time_normal_blocks(z(2, 4, 3), z(2), z(2, 3), z(2, 4, 3, 2), i32(1)),              # another n_state
                lambda: ml.time_normal_blocks(z(2, 4, 2), z(3), z(2, 3), z(2, 4, 3, 2), i32(1)),
                lambda: ml.time_normal_blocks(z(2, 4, 2), z(2), z(2, 3).float(), z(2, 4, 3, 2), i32(1)),
                lambda: ml.time_normal_blocks(z(2, 3, 2), z(2), z(2, 3), z(2, 3, 3, 2), i32(1), curv=z(2, 3, 2)),   # three nodes are no cubic
                lambda: ml.time_normal_blocks(z(2, 4, 2), z(2), z(2, 3), z(2, 4, 3, 2), i32(1), out=(z(2, 3, 3), z(2, 2))),
                lambda: step(D=3), lambda: step(D=0), lambda: step(ok=z(4)), lambda: step(tau=z(4, 3)), lambda: step(lambda_up=0.5)):
        with pytest.raises(LfsdError):
            bad()


# ---- 2. the learner ---------------------------------------------------------------------------------------------------------------
TAUS = [0.23, 0.52, 0.81]
WPS = [[0.4], [1.5], [2.6]]


def _pendulum(emu, rows=8):
    oc, env, d = models.pendulum(n_grid=10)
    emu(oc)
    oc.setDevice(dtype=F64)
    seeds = LC.compose_seeds(d["theta0"], rows)
    return oc, d, seeds


def _independent(emu, rows=8, **fixed):
    oc, d, seeds = _pendulum(emu, rows)
    x0 = np.tile(d["ini_state"], (rows, 1))

    def make(rows=slice(None), **kw):
        return CPDP.SparseDemoLearner(oc, x0[rows], 1.0, TAUS, WPS, [0], seeds[rows], method="LM", lm_taus=True, **dict(fixed, **kw))
    B = rows
    row = dict(x0=oc._t(x0), hz=oc._t(1.0).expand(B).contiguous(), taus=oc._t(TAUS).expand(B, 3).contiguous(),
               wps=oc._t(WPS).expand(B, 3, 1).contiguous())
    return oc, make, row, seeds


LAMBDA0 = 1.0      # (tests/lm_cases.py: COMPOSE_LAMBDA0 of the pendulum -- rejections and later acceptances within six steps)


def test_independent_learner_is_its_launches(emu):
    oc, make, row, seeds = _independent(emu, lm_lambda0=LAMBDA0)
    hand = C.lmt_by_hand(oc, row["x0"], row["hz"], row["taus"], row["wps"], [0], seeds, 6, make().proj_lo, LAMBDA0)
    C.run_composition(make, hand, steps=6, half=3)


def test_grouped_learner_is_its_launches(emu):
    oc, d, seeds = _pendulum(emu, rows=2)
    D = 3
    taus_d = np.array([[0.2, 0.5, 0.8], [0.25, 0.5, 0.75], [0.1, 0.4, 0.9]])
    wps_d = np.array([[[0.4], [1.5], [2.6]], [[0.5], [1.4], [2.4]], [[0.2], [1.1], [2.8]]])
    x0_d = np.tile(d["ini_state"], (D, 1))

    def make(rows=slice(None), skip=False, **kw):
        return CPDP.SparseDemoLearner(oc, x0_d, 1.0, taus_d, wps_d, [0], seeds[rows], method="LM", lm_taus=True, mode="grouped",
                                      demos_per_seed=D, lm_lambda0=C.GROUPED_LAMBDA0, skip_unconverged=skip, **kw)
    G = 2
    acc, lam = {}, {}
    for skip in (False, True):      # (tests/lm_times_cases.py, GROUPED_LAMBDA0: what each run rejects and accepts)
        hand = C.lmt_by_hand(oc, np.tile(x0_d, (G, 1)), oc._t(1.0).expand(G * D).contiguous(), np.tile(taus_d, (G, 1)),
                             np.tile(wps_d, (G, 1, 1)), [0], seeds, 6, make().proj_lo, C.GROUPED_LAMBDA0, D=D, skip=skip)
        L, hist = C.run_composition(lambda **kw: make(skip=skip, **kw), hand, steps=6, half=1, D=D)
        assert L.taus.shape == (6, 3) and L.theta.shape[0] == 2 and L.time_blocks[0].shape == (6, 3, 3)
        acc[skip] = torch.stack([h["accepted"] for h in hist])
        lam[skip] = torch.stack([h["lm_lambda"] for h in hist])
    a0 = acc[False][:, 0].tolist()
    assert False in a0[1:] and True in a0[a0.index(False, 1):]               # group 0 rejects, its lambda rises, and it accepts later
    assert bool((lam[False][1:, 0].max() > lam[False][0, 0]))
    assert bool((~acc[True][1:, 0]).all()) and bool(acc[True][1:, 1].all())      # frozen from step 2 beside an accepting group:
    assert bool((lam[True][1:, 0] == lam[True][0, 0]).all())                     # not a rejection, lambda stays


def test_combinations(emu):
    oc, make, row, seeds = _independent(emu, rows=4, lm_lambda0=LAMBDA0)
    # level 2 with weights and bounds, against the launches
    w = torch.tensor([1.0, 0.5, 2.0], dtype=F64).expand(4, 3).contiguous()
    bounds = ([0.15, 0.45, 0.7], [0.3, 0.6, 0.9])
    mk = lambda rows=slice(None), **kw: make(rows=rows, interplation_level=2, waypoint_weights=w[rows], tau_bounds=bounds, warm_start=False, **kw)
    bt = tuple(oc._t(x).expand(4, 3).contiguous() for x in bounds)
    hand = C.lmt_by_hand(oc, row["x0"], row["hz"], row["taus"], row["wps"], [0], seeds, 3, make().proj_lo, LAMBDA0, level=2, wts=w, bounds=bt)
    C.run_composition(mk, hand, steps=3, bounds=bounds, need_reject=False, need_accept=False)
    # ragged demonstrations against each demonstration learned alone, bit for bit
    K5, W5, counts = [0.15, 0.3, 0.5, 0.7, 0.85], [[0.3], [0.8], [1.5], [2.2], [2.6]], [5, 3, 1]
    tl, wl = [K5[:c] for c in counts], [W5[:c] for c in counts]
    tp, wpd, _ = CPDP.pad_demonstrations(tl, wl)
    x0 = row["x0"].numpy()
    kw = dict(method="LM", lm_taus=True, lm_lambda0=LAMBDA0)
    Lr = CPDP.SparseDemoLearner(oc, x0[:3], 1.0, tp, wpd, [0], seeds[:3], n_waypoints=counts, **kw)
    alone = [CPDP.SparseDemoLearner(oc, x0[i:i + 1], 1.0, tl[i], wl[i], [0], seeds[i:i + 1], **kw) for i in range(3)]
    for _ in range(3):
        Lr.step()
        for A in alone:
            A.step()
    for i, c in enumerate(counts):
        assert H.same(Lr.taus[i, :c], alone[i].taus[0]) and torch.equal(Lr.theta[i], alone[i].theta[0]), i
        assert H.same(Lr.tau_trial[i, :c], alone[i].tau_trial[0]) and torch.equal(Lr.theta_trial[i], alone[i].theta_trial[0]), i
        assert bool((Lr.tau_grad[i, c:] == 0).all()) and bool((Lr.time_blocks[1][i, c:] == 0).all())
    # skip_unconverged with one row forced to FAILED: its whole state, the times included, keeps every bit
    Lf = make(skip_unconverged=True, trace=4, lm_lambda0=30.0)      # (damped enough for the rows to stay where their sweeps converge)
    Lf.step()
    state = lambda L: [t.clone() for t in (L.theta, L.theta_trial, L.lm_lambda, L.lm_loss, L.taus, L.tau_trial) + L.time_blocks]
    before = state(Lf)
    mask = Lf.mask_unconverged

    def forced(status, loss, grad, stats=None):
        status = status.clone()
        status[1] = 4
        return mask(status, loss, grad, stats)
    Lf.mask_unconverged = forced
    l, _ = Lf.step()
    for a, b in zip(state(Lf), before):
        assert H.same(a[1], b[1])
    ok = Lf._ok
    assert not bool(ok[1]) and bool(ok.any()) and bool((Lf.lm_lambda[ok] != before[2][ok]).all())
    assert torch.equal(Lf.theta_trace[:, 2], Lf.theta) and H.same(Lf.loss_trace[:, 1], l)      # trace: the accepted theta, the returned loss


def test_refusals(emu):
    oc, make, row, seeds = _independent(emu, rows=2)
    x0 = row["x0"].numpy()
    args = (x0, 1.0, TAUS, WPS, [0], seeds)
    new = lambda *a, **kw: CPDP.SparseDemoLearner(oc, *(a or args), **dict(dict(method="LM", lm_taus=True), **kw))
    for kw, word in ((dict(method="Adam"), "method='LM'"), (dict(learn_taus=True, tau_learning_rate=1e-3), "learn_taus"),
                     (dict(tau_learning_rate=1e-3), "prior term is not part of this step's objective"),
                     (dict(tau_method="Adam"), "prior term is not part of this step's objective"),
                     (dict(tau_prior=0.5), "prior term is not part of this step's objective"),
                     (dict(loss_fn=H.squared_waypoint_loss([0], 0.0)), "sum of squares"),
                     (dict(stop_rule=dict(loss=0.9, grad_norm=0.05)), "stop_rule"), (dict(learning_rate=[0.1, 0.1]), "rows path"),
                     (dict(tau_max_shift=0.5), "tau_max_shift"), (dict(tau_bounds=([0.0, 0.0], [1.0, 1.0])), "tau_bounds")):
        with pytest.raises(LfsdError, match=word):
            new(**kw)
    with pytest.raises(LfsdError, match="independent"):
        new(x0, 1.0, TAUS, WPS, [0], seeds[:1], mode="shared")
    with pytest.raises(LfsdError, match="interface"):
        new(x0, 1.0, TAUS, WPS, None, seeds)
    for bad in ([0.5, 0.5, 0.8], [0.5, 0.2, 0.8]):
        with pytest.raises(LfsdError, match="taus"):
            new(x0, 1.0, bad, WPS, [0], seeds)
    # the older refusals still name what they named
    with pytest.raises(LfsdError, match="LM"):
        CPDP.SparseDemoLearner(oc, *args, method="LM", learn_taus=True, tau_learning_rate=1e-3)
    with pytest.raises(LfsdError, match="tau_method"):
        CPDP.SparseDemoLearner(oc, *args, method="Adam", learn_taus=True, tau_learning_rate=1e-3, tau_method="LM")
    # more than 16 parameters: no model of the zoo has them, so the learner cannot be built there; the binding's own check
    ml = oc.compile()
    with pytest.raises(LfsdError, match="16"):
        z = lambda *s: torch.zeros(s, dtype=F64)
        ml.lm_step_times(z(1, 17), z(1), z(1, 17), z(1, 17, 17), z(1), z(1, 17), z(1, 1), z(1, 1), z(1, 1), z(1, 1, 17), z(1, 1),
                         torch.zeros(1, dtype=torch.int32), z(1), z(1, 17), z(1, 17, 17), z(1, 1), z(1, 1, 17), z(1, 1))


def test_driver_returns_the_accepted_times(emu):
    oc_q = models.quadrotor(n_grid=6)[0]
    new, ini, goal, demo = H.quad_driver(6, torch.float32, library=build_emu_library(oc_q))
    Q = new()
    Q.load_optimization_function(dict(method="LM", iter_num=2, lm_lambda0=300.0))
    res = Q.run(ini, goal, demo, ObsList=[], lm_taus=True)
    assert res["taus"].shape == (1, 3) and res["tau_trace"].shape == (3, 1, 3) and np.all(np.diff(res["taus"][0]) > 0)
    assert Q.learner.tau_trial.shape == (1, 3) and Q.learner.method == "LM"


def test_without_lm_taus_the_learner_takes_the_launches_it_took(emu, monkeypatch):
    """The ORDERED list of every ModelLibrary call of two steps: an LM learner with lm_taus=False (and the arguments lm_taus reads)
    makes the list of a learner built without them, with outputs bit for bit; with lm_taus, that list with the two launches of the
    time terms behind normal_matrix, lm_step_times in the place of lm_step and tau_project behind it."""
    oc, d, seeds = _pendulum(emu, rows=2)
    args = (np.tile(d["ini_state"], (2, 1)), 1.0, TAUS, WPS, [0], seeds)
    ml = oc.compile()
    calls = []
    for name in dir(ml):
        fn = getattr(ml, name)
        if name.startswith("_") or not callable(fn) or isinstance(fn, type):
            continue

        def wrapped(*a, _fn=fn, _name=name, **kw):
            calls.append(_name)
            return _fn(*a, **kw)
        monkeypatch.setattr(ml, name, wrapped)

    def two_steps(L):
        per = []
        for _ in range(2):
            calls.clear()
            l, g = L.step()
            per.append((l.clone(), g.clone(), list(calls)))
        return per
    for kw in (dict(method="LM"), dict(method="Adam", learning_rate=1e-2)):
        base = two_steps(CPDP.SparseDemoLearner(oc, *args, **kw))
        L = CPDP.SparseDemoLearner(oc, *args, lm_taus=False, tau_max_shift=0.3, tau_bounds=([0.1, 0.4, 0.7], [0.3, 0.6, 0.9]), **kw)
        for (l, g, seq), (l0, g0, seq0) in zip(two_steps(L), base):
            assert seq == seq0 and torch.equal(l, l0) and torch.equal(g, g0)
            assert "time_normal_blocks" not in seq and "lm_step_times" not in seq and "tau_project" not in seq
        assert L.tau_trial is None and L.time_blocks is None and L.tau_grad is None
    ref = two_steps(CPDP.SparseDemoLearner(oc, *args, method="LM"))
    got = two_steps(CPDP.SparseDemoLearner(oc, *args, method="LM", lm_taus=True))
    for (_, _, seq), (_, _, seq0) in zip(got, ref):
        i, j = seq0.index("normal_matrix"), seq0.index("lm_step")
        expect = seq0[:i + 1] + ["waypoint_time_grad", "time_normal_blocks"] + seq0[i + 1:j] + ["lm_step_times", "tau_project"] + seq0[j + 1:]
        assert seq == expect, (seq, expect)


# ---- 3. recovery on data with a known answer ------------------------------------------------------------------------------------------
def test_recovery_follows_the_fp64_numpy_joint_lm(emu):
    """Conditions on the numpy loop alone first (tests/lm_times_cases.py says what start was chosen and why the grid has 40 intervals),
    row by row: within 12 steps the row's times come within a tenth of the largest initial shift and its accepted loss falls below 1e-6
    of its initial one, and every decision the row took up to there is clear by 100 x the parity tolerance.  Then the learner must
    follow each row's decisions, accepted losses and times over those steps within the pendulum's fp64 parity tolerance (1e-6,
    margin 1)."""
    oc, env, d = models.pendulum(n_grid=C.RECOVER_N_GRID)
    emu(oc)
    oc.setDevice(dtype=F64)
    hz, iface = float(d["horizon"]), list(C.RECOVER_IFACE)
    true = np.asarray(d["true_theta"], dtype=np.float64)
    star, start = C.recovery_start(hz)
    B, K = start.shape
    x0 = np.tile(d["ini_state"], (B, 1))
    sol = oc.cocSolverBatch(x0, hz, np.tile(true, (B, 1)))
    X = sol["state_grid"].numpy().copy()
    n_grid = X.shape[1] - 1
    h = hz / n_grid
    k = np.floor(star / h).astype(int)
    s = (star - k * h) / h
    wp = np.tile((X[0][k] + s[:, None] * (X[0][k + 1] - X[0][k]))[:, iface][None], (B, 1, 1))
    theta0 = true[None, :] * (1.0 + C.RECOVER_THETA_OFF * np.asarray(C.RECOVER_THETA_SIGNS, dtype=np.float64))
    L = CPDP.SparseDemoLearner(oc, x0, hz, start, wp, iface, theta0, method="LM", lm_taus=True, lm_lambda0=C.RECOVER_LAMBDA0,
                               tau_max_shift=C.RECOVER_C)

    def evaluate(th, tau):
        sol = oc.cocSolverBatch(x0, hz, th)
        aux = oc.auxSysSolverBatch(sol, tau, wp, iface, want_grids=True, validate=False)
        return sol["state_grid"].numpy().copy(), aux["auxX_grid"].numpy().copy()
    trace = C.numpy_joint_lm(evaluate, theta0, start, hz, wp, iface, C.RECOVER_STEPS, C.RECOVER_LAMBDA0, C.RECOVER_C, L.proj_lo.numpy())
    shift = np.abs(start - star).max()
    err = np.array([np.abs(t["taus"] - star).max(axis=1) for t in trace])           # [step, row]
    loss = np.array([t["lm_loss"] for t in trace])
    margin = np.array([t["margin"] for t in trace])
    steps = []
    for b in range(B):
        print("numpy loop, row %d: largest initial shift %.4f, max |tau - tau*| per step" % (b, shift), err[:, b])
        print("numpy loop, row %d: accepted loss / initial" % b, loss[:, b] / loss[0, b])
        print("numpy loop, row %d: decision margins per step" % b, margin[:, b])
        reached = [n for n in range(len(trace)) if err[n, b] < 0.1 * shift and loss[n, b] < 1e-6 * loss[0, b]]
        assert reached, "row %d of the numpy loop does not reach both conditions within %d steps" % (b, C.RECOVER_STEPS)
        steps.append(reached[0] + 1)
        least = float(margin[:steps[b], b].min())
        print("numpy loop, row %d: both conditions hold after %d steps; smallest decision margin up to there %.3e" % (b, steps[b], least))
        assert least > 100 * C.RECOVER_TOL, b
    worst_t = worst_l = 0.0
    for it in range(max(steps)):
        L.step()
        for b in range(B):
            if it >= steps[b]:                                   # past the row's last clear decision: losses at the rounding floor
                continue
            assert bool(L.lm_accepted[b]) == bool(trace[it]["accepted"][b]), (it, b)
            worst_t = max(worst_t, float(np.abs(L.taus[b].numpy() - trace[it]["taus"][b]).max()))
            worst_l = max(worst_l, abs(float(L.lm_loss[b]) - float(trace[it]["lm_loss"][b])))
            if it == steps[b] - 1:
                assert float(np.abs(L.taus[b].numpy() - star).max()) < 0.1 * shift and float(L.lm_loss[b]) < 1e-6 * loss[0, b], b
    print("learner against the numpy loop over %s steps: times %.3e, accepted losses %.3e (asserted < %.0e)" % (steps, worst_t, worst_l, C.RECOVER_TOL))
    assert worst_t < C.RECOVER_TOL and worst_l < C.RECOVER_TOL
