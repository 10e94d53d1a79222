"""CPU tier of the learnable waypoint times (ABI 17): lfsd_waypoint_time_grad and lfsd_tau_project through the SIMT emulator against fp64
restatements (numpy, scipy's not-a-knot spline) and against the existing fused loss by central differences; every LFSD_EINVAL case on
host dummies (emulator and gfx950 library); the learner with learn_taus against the same launches made by hand, bit for bit; the
launches of a learner without it, in order; exact decrease of a tau-only step; recovery of known times against an fp64 numpy loop;
grouped and shared mode by hand; combinations, refusals, the driver.  Cases and bounds:
tests/tau_cases.py."""
import numpy as np
import pytest
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models, runtime
from lfsd_amd.runtime import LfsdError
from conftest import build_emu_library
import hyper_sweep_cases as H
import tau_cases as C

F64 = torch.float64
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, F64], ids=["fp32", "fp64"])
SHAPES = pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "B%dK%d" % s)


@pytest.fixture(scope="module")
def lib():
    """The quadrotor's library: 13 states (the kernel takes the state dimension from its model)."""
    return runtime.ModelLibrary(build_emu_library(models.quadrotor(n_grid=10)[0]))


# ---- 1. kernels -----------------------------------------------------------------------------------------------------------------
@DTYPES
@SHAPES
def test_time_grad_linear_against_fp64_restatement(lib, shape, dtype):
    B, K = shape
    for n_grid in C.N_GRIDS:
        r = C.run_time_grad(lib, "cpu", dtype, B, K, n_grid, cubic=False)
        print("time_grad linear B%d K%d n_grid %d: |dtau - ref| / bound %.3f" % (B, K, n_grid, r))
        assert r <= 1.0, (n_grid, r)


@DTYPES
@SHAPES
def test_time_grad_cubic_against_scipy_spline_derivative(lib, shape, dtype):
    B, K = shape
    for n_grid in C.N_GRIDS_CUBIC:
        r = C.run_time_grad(lib, "cpu", dtype, B, K, n_grid, cubic=True)
        print("time_grad cubic B%d K%d n_grid %d: |dtau - ref| / bound %.3f" % (B, K, n_grid, r))
        assert r <= 1.0, (n_grid, r)


@DTYPES
def test_prior_term_alone_is_one_rounding(lib, dtype):
    C.run_prior_alone(lib, "cpu", dtype)


@DTYPES
def test_compiled_interface(dtype):
    """No zoo model carries a compiled-in interface: the pendulum observed through (sin q, q dq), as tests/weight_cases.py builds it."""
    import sympy as sp
    oc, env, d = models.pendulum(n_grid=10)
    X = list(oc.state)
    oc.setInterface([sp.sin(X[0]), X[0] * X[1]])
    ml = runtime.ModelLibrary(build_emu_library(oc))
    assert ml.n_interface == 2

    def g(x):
        y = np.stack([np.sin(x[..., 0]), x[..., 0] * x[..., 1]], -1)
        J = np.zeros(x.shape[:-1] + (2, 2))
        J[..., 0, 0], J[..., 1, 0], J[..., 1, 1] = np.cos(x[..., 0]), x[..., 1], x[..., 0]
        return y, J
    consts = torch.tensor(ml.const_defaults, dtype=dtype) if ml.n_const else None
    r = C.run_compiled_interface(ml, "cpu", dtype, g, consts=consts)
    print("time_grad compiled interface: |dtau - ref| / bound %.3f" % r)
    assert r <= 1.0
    with pytest.raises(LfsdError):                                  # the index path's library has none
        runtime.ModelLibrary(build_emu_library(models.pendulum(n_grid=10)[0])).waypoint_time_grad(
            torch.zeros(1, 4, 2, dtype=dtype), torch.ones(1, dtype=dtype), torch.zeros(1, 1, dtype=dtype), torch.zeros(1, 1, 1, dtype=dtype), None)


@DTYPES
@SHAPES
@pytest.mark.parametrize("c", [0.1, 0.49])
def test_tau_project_is_its_numpy_restatement(lib, shape, dtype, c):
    C.run_tau_project(lib, "cpu", dtype, shape[0], shape[1], c)


@pytest.mark.parametrize("which", ["emulator", "hip"])
def test_entry_points_refuse_bad_arguments_before_any_launch(which):
    """Host dummies stand in for the arrays: no launch is reached (the gfx950 library loads without a GPU, as in tests/test_capi.py)."""
    oc = models.pendulum(n_grid=10)[0]
    ml = runtime.ModelLibrary(build_emu_library(oc)) if which == "emulator" else oc.compile()
    C.time_grad_einval(ml.lib, ml.n_interface)
    C.tau_project_einval(ml.lib)
    z = lambda *s: torch.zeros(s, dtype=F64)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    if which == "hip":                                          # no CPU fallback: the HIP library refuses host memory
        with pytest.raises(LfsdError):
            ml.waypoint_time_grad(z(2, 4, 2), z(2), z(2, 3), z(2, 3, 1), i32(1))
        with pytest.raises(LfsdError):
            ml.tau_project(z(2, 3), z(2, 3), z(2), 0.25)
        return
    for bad in (lambda: ml.waypoint_time_grad(z(2, 4, 3), z(2), z(2, 3), z(2, 3, 1), i32(1)),              # three states: not this model
                lambda: ml.waypoint_time_grad(z(2, 4, 2), z(3), z(2, 3), z(2, 3, 1), i32(1)),
                lambda: ml.waypoint_time_grad(z(2, 4, 2), z(2), z(2, 3).float(), z(2, 3, 1), i32(1)),
                lambda: ml.waypoint_time_grad(z(2, 4, 2), z(2), z(2, 3), z(2, 3, 2), i32(1)),
                lambda: ml.waypoint_time_grad(z(2, 1, 2), z(2), z(2, 3), z(2, 3, 1), i32(1)),              # one node is no interval
                lambda: ml.waypoint_time_grad(z(2, 3, 2), z(2), z(2, 3), z(2, 3, 1), i32(1), curv=z(2, 3, 2)),
                lambda: ml.waypoint_time_grad(z(2, 4, 2), z(2), z(2, 3), z(2, 3, 1), torch.zeros(1, dtype=torch.int64)),
                lambda: ml.waypoint_time_grad(z(2, 4, 2), z(2), z(2, 3), z(2, 3, 1), i32(1), wp_weight=z(2, 2)),
                lambda: ml.waypoint_time_grad(z(2, 4, 2), z(2), z(2, 3), z(2, 3, 1), i32(1), out=z(2, 2)),
                lambda: ml.waypoint_time_grad(z(2, 4, 2), z(2), z(2, 3), z(2, 3, 1), i32(1), tau_prior=-1.0),
                lambda: ml.tau_project(z(2, 3), z(2, 2), z(2), 0.25),
                lambda: ml.tau_project(z(2, 3), z(2, 3), z(3), 0.25),
                lambda: ml.tau_project(z(2, 3), z(2, 3).float(), z(2), 0.25),
                lambda: ml.tau_project(z(2, 3), z(2, 3), z(2), 0.5),
                lambda: ml.tau_project(z(2, 3), z(2, 3), z(2), 0.25, row_active=z(2))):
        with pytest.raises(LfsdError):
            bad()
    t = z(2, 3)
    with pytest.raises(LfsdError):
        ml.tau_project(t, t, z(2), 0.25)


# ---- 2. against the existing device code, no formula shared -------------------------------------------------------------------------
def _pendulum(emu, rows=8, n_grid=10):
    oc, env, d = models.pendulum(n_grid=n_grid)
    emu(oc)
    oc.setDevice(dtype=F64)
    rng = np.random.default_rng(3)
    th0 = np.asarray(d["theta0"], dtype=np.float64)
    seeds = th0[None, :] * (1.0 + 0.3 * rng.uniform(-1, 1, (rows, th0.size)))
    return oc, d, seeds


def test_central_difference_of_the_fused_loss_is_twice_dtau(emu):
    """fp64, linear level, tau at mid-interval, eps_fd = h / 64: the fused loss of lfsd_aux_forward at tau +- eps_fd.  Inside an interval
    the loss is exactly quadratic in tau, so the central difference is exact up to rounding: each loss carries
    dL <= eps (8 sum |r| (|x_a| + |x_b|) + K C L) (four roundings of the interpolated value, the square and the sum), the difference
    quotient dL / eps_fd; dtau carries its own bound (tests/tau_cases.py)."""
    oc, d, seeds = _pendulum(emu, rows=3)
    lib = oc.compile()
    n_grid, hz = 10, float(d["horizon"])
    h = hz / n_grid
    taus = torch.tensor([[1.5 * h, 4.5 * h, 8.5 * h]] * 3, dtype=F64)
    wps = torch.tensor([[[0.4], [1.5], [2.6]]] * 3, dtype=F64)
    sol = oc.cocSolverBatch(np.tile(d["ini_state"], (3, 1)), hz, seeds)
    hz_t = sol["horizon"]
    idx = torch.tensor([0], dtype=torch.int32)
    dtau = lib.waypoint_time_grad(sol["state_grid"], hz_t, taus, wps, idx)
    ref, bound = C.time_grad_reference(hz_t, taus, sol["state_grid"], wps, n_grid, idx=(0,))
    assert float((np.abs(dtau.numpy() - ref) / bound).max()) <= 1.0
    e = h / 64
    eps = C.eps_of(F64)
    X = sol["state_grid"].numpy()
    for k in range(3):
        lo, hi = taus.clone(), taus.clone()
        lo[:, k] -= e
        hi[:, k] += e
        Lm = oc.auxSysSolverBatch(sol, lo, wps, [0])["loss"].clone().numpy()
        Lp = oc.auxSysSolverBatch(sol, hi, wps, [0])["loss"].clone().numpy()
        kk, s, _ = C.interval_of(hz_t, taus, n_grid)
        b = np.arange(3)[:, None]
        M = np.abs(X[b, kk][:, :, 0]) + np.abs(X[b, kk + 1][:, :, 0])
        r = np.abs(X[b, kk][:, :, 0] + s * (X[b, kk + 1][:, :, 0] - X[b, kk][:, :, 0]) - wps[:, :, 0].numpy()) + np.abs(X[b, kk + 1][:, :, 0] - X[b, kk][:, :, 0]) / 64
        dL = eps * (8 * (r * M).sum(1) + 3 * np.maximum(Lp, Lm))
        fd = (Lp - Lm) / (2 * e)
        tol = dL / e + 2 * bound[:, k]
        print("waypoint %d: |fd - 2 dtau| / bound" % k, np.abs(fd - 2 * dtau[:, k].numpy()) / tol)
        assert np.all(np.abs(fd - 2 * dtau[:, k].numpy()) <= tol)


# ---- 3. the learner ---------------------------------------------------------------------------------------------------------------
def _learner_args(emu, rows=8):
    oc, d, seeds = _pendulum(emu, rows)
    args = (np.tile(d["ini_state"], (rows, 1)), 1.0, [0.2, 0.5, 0.8], [[0.4], [1.5], [2.6]], [0], seeds)
    return oc, args


def test_learn_taus_false_takes_the_launches_it_took(emu, monkeypatch):
    """The ORDERED list of every ModelLibrary call of two steps (every public method is wrapped, nested calls included): without
    learn_taus it is the list of a learner built without the arguments, with outputs bit for bit; with it, that list plus the calls
    of the times at their places, and nothing else."""
    oc, args = _learner_args(emu, rows=2)
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

    def steps_of(L, outs=None):
        """The calls of each of two steps."""
        per = []
        for k in range(2):
            calls.clear()
            l, g = L.step()
            if outs is not None:
                assert torch.equal(l, outs[k][0]) and torch.equal(g, outs[k][1])
            else:
                per.append((l.clone(), g.clone()))
            per.append(list(calls))
        return per
    for method in ("Vanilla", "Nesterov", "Adam"):
        base = CPDP.SparseDemoLearner(oc, *args, method=method, learning_rate=1e-2)
        rec = steps_of(base)
        outs, want = rec[0::2], rec[1::2]
        for seq in want:
            assert "waypoint_time_grad" not in seq and "tau_project" not in seq and seq.count("optimizer_step") == 1
            assert seq.count("lookahead") == (1 if method == "Nesterov" else 0)
        L = CPDP.SparseDemoLearner(oc, *args, method=method, learning_rate=1e-2, learn_taus=False, tau_learning_rate=0.1,
                                   tau_max_shift=0.3, tau_prior=1.0)
        assert steps_of(L, outs) == want
        assert torch.equal(L.theta, base.theta) and torch.equal(L.taus, base.taus) and L.tau_grad is None and L.m_tau is None
        L = CPDP.SparseDemoLearner(oc, *args, method=method, learning_rate=1e-2, learn_taus=True, tau_learning_rate=1e-3)
        calls.clear()
        got = []
        for k in range(2):
            calls.clear()
            L.step()
            got.append(list(calls))
        for seq, ref in zip(got, want):
            i = ref.index("optimizer_step")
            expect = ref[:i] + ["waypoint_time_grad", "optimizer_step", "optimizer_step", "tau_project"] + ref[i + 1:]
            if method == "Nesterov":                         # the look-ahead times and their projection, right after theta's look-ahead
                j = expect.index("lookahead")
                expect = expect[:j + 1] + ["lookahead", "tau_project"] + expect[j + 1:]
            assert seq == expect, (method, seq, expect)


def test_pendulum_learner_is_its_launches(emu):
    oc, args = _learner_args(emu)
    x0, hz, taus, wps = oc._t(args[0]), oc._t(1.0).expand(8).contiguous(), oc._t(args[2]).expand(8, 3).contiguous(), \
        oc._t(args[3]).expand(8, 3, 1).contiguous()
    make = lambda **kw: CPDP.SparseDemoLearner(oc, *args, learn_taus=True, **kw)
    C.run_composition(make, oc, x0, hz, wps, [0], taus, (("Vanilla", 1e-2, "Vanilla", 2e-3), ("Nesterov", 1e-3, "Nesterov", 5e-4),
                                                         ("Adam", 1e-2, "Adam", 5e-3), ("Adam", 1e-2, "Vanilla", 2e-3)))
    # level 2 and a prior, weights
    w = torch.tensor([1.0, 0.5, 2.0], dtype=F64).expand(8, 3).contiguous()
    make2 = lambda **kw: CPDP.SparseDemoLearner(oc, *args, learn_taus=True, interplation_level=2, tau_prior=0.5, waypoint_weights=w, **kw)
    C.run_composition(make2, oc, x0, hz, wps, [0], taus, (("Vanilla", 1e-2, "Vanilla", 2e-3),), steps=3, level=2, prior=0.5, wts=w)


def test_tau_only_step_decreases_the_loss_by_the_quadratic_model(emu):
    """learning_rate = 0, Vanilla: the trajectory does not move, no waypoint leaves its interval (checked), so the loss after the step is
    the quadratic-in-tau model's value, to the rounding of two loss evaluations."""
    oc, args = _learner_args(emu, rows=4)
    args = args[:5] + (args[5][:4],)
    lr_tau = 1e-4
    L = CPDP.SparseDemoLearner(oc, *args, method="Vanilla", learning_rate=0.0, learn_taus=True, tau_learning_rate=lr_tau)
    l0, _ = L.step()
    l0, t0, t1, dtau = l0.clone().numpy(), L.tau0.numpy(), L.taus.numpy(), L.tau_grad.numpy()
    X = L._sol["state_grid"].numpy()
    h = 1.0 / 10
    k0, k1 = np.floor(t0 / h), np.floor(t1 / h)
    assert np.array_equal(k0, k1) and np.array_equal(t1, t0 - lr_tau * dtau) and np.abs(dtau).min() > 0
    l1 = L.evaluate(L.theta)[0].clone().numpy()
    b = np.arange(4)[:, None]
    k = k0.astype(int)
    xa, xb = X[b, k][:, :, [0]], X[b, k + 1][:, :, [0]]
    wp = np.asarray(args[3])[None]
    f0, g0, c0 = C.quadratic_in_tau(xa, xb - xa, h, ((t0 - k * h) / h)[:, :, None], wp, 1.0)
    dt = t1 - t0
    model = (f0 + g0 * dt + 0.5 * c0 * dt * dt).sum(1)
    assert np.allclose(g0, 2 * dtau, rtol=1e-9, atol=0)
    eps = C.eps_of(F64)
    tol = 64 * eps * (np.abs(xa) + np.abs(xb) + np.abs(wp)).max() ** 2 * 3      # every term of the loss: a few roundings of values of this size
    print("loss before", l0, "after", l1, "model", model, "|after - model|", np.abs(l1 - model), "tol", tol)
    assert np.all(np.abs(l1 - model) <= tol) and np.all(l1 < l0)


def test_modes_ragged_and_frozen_rows(emu):
    oc, args = _learner_args(emu, rows=6)
    kw = dict(method="Adam", learning_rate=1e-2, learn_taus=True, tau_learning_rate=2e-3)
    # the same seeds in a batch of another size: the same bits
    L = CPDP.SparseDemoLearner(oc, *args, **kw)
    Ls = CPDP.SparseDemoLearner(oc, args[0][:2], *args[1:5], args[5][:2], **kw)
    for _ in range(3):
        L.step(); Ls.step()
    assert torch.equal(L.taus[:2], Ls.taus) and torch.equal(L.m_tau[:2], Ls.m_tau) and torch.equal(L.theta[:2], Ls.theta)
    # grouped (G = 2, D = 3) and shared: rows own their times
    taus_d = np.array([[0.2, 0.5, 0.8], [0.25, 0.5, 0.75], [0.1, 0.4, 0.9]])
    Lg = CPDP.SparseDemoLearner(oc, args[0][:3], 1.0, taus_d, args[3], [0], args[5][:2], mode="grouped", demos_per_seed=3, **kw)
    for _ in range(2):
        lg, gg = Lg.step()
    assert Lg.taus.shape == (6, 3) and lg.shape == (2,) and not torch.equal(Lg.taus, Lg.tau0)
    assert not torch.equal(Lg.taus[:3], Lg.taus[3:])                 # (the two seeds' copies of a demonstration move apart)
    Lsh = CPDP.SparseDemoLearner(oc, args[0][:3], 1.0, taus_d, args[3], [0], args[5][0], mode="shared", skip_unconverged=False, **kw)
    Lsh.step()      # (skip_unconverged, on by default in this mode, freezes the times of a row with its gradient: checked last, below)
    assert Lsh.taus.shape == (3, 3) and Lsh.theta.shape[0] == 1 and not torch.equal(Lsh.taus, Lsh.tau0)
    # ragged demonstrations against each demonstration learned alone, bit for bit
    K5 = [0.15, 0.3, 0.5, 0.7, 0.85]
    W5 = [[0.3], [0.8], [1.5], [2.2], [2.6]]
    counts = [5, 3, 1]
    tl, wl = [K5[:c] for c in counts], [W5[:c] for c in counts]
    tp, wpd, _ = CPDP.pad_demonstrations(tl, wl)
    Lr = CPDP.SparseDemoLearner(oc, args[0][:3], 1.0, tp, wpd, [0], args[5][:3], n_waypoints=counts, **kw)
    alone = [CPDP.SparseDemoLearner(oc, args[0][i:i + 1], 1.0, tl[i], wl[i], [0], args[5][i:i + 1], **kw) for i in range(3)]
    for _ in range(3):
        Lr.step()
        for A in alone:
            A.step()
    for i, c in enumerate(counts):
        assert torch.equal(Lr.taus[i, :c], alone[i].taus[0]) and torch.equal(Lr.theta[i], alone[i].theta[0]), i
        assert torch.equal(Lr.m_tau[i, :c], alone[i].m_tau[0]) and bool((Lr.tau_grad[i, c:] == 0).all())
    # skip_unconverged with one row forced to FAILED: its times and moments keep every bit
    Lf = CPDP.SparseDemoLearner(oc, *args, skip_unconverged=True, **kw)
    Lf.step()
    before = C.learner_state(Lf)
    mask = Lf.mask_unconverged

    def forced(status, loss, grad, stats=None):
        status = status.clone()
        status[1] = 4
        return mask(status, loss, grad, stats)
    Lf.mask_unconverged = forced
    Lf.step()
    after = C.learner_state(Lf)
    for k in before:
        assert torch.equal(after[k][1], before[k][1]), k
    # (the error-controlled sweeps freeze some of these rows on their own: the rows the mask left in have moved)
    ok = Lf._ok
    assert not bool(ok[1]) and bool(ok.any())
    assert bool((after["taus"][ok] != before["taus"][ok]).any(dim=1).all()) and bool((after["m_tau"][ok] != before["m_tau"][ok]).any(dim=1).all())
    assert torch.equal(after["taus"][~ok], before["taus"][~ok]) and torch.equal(after["vhat_tau"][~ok], before["vhat_tau"][~ok])


def test_refusals(emu):
    oc, args = _learner_args(emu, rows=2)
    ok = dict(learn_taus=True, tau_learning_rate=1e-3)
    make = lambda *a, **kw: CPDP.SparseDemoLearner(oc, *(a or args), **dict(ok, **kw))
    for kw, word in ((dict(loss_fn=H.squared_waypoint_loss([0], 0.0)), "loss_fn"), (dict(method="LM"), "LM"),
                     (dict(stop_rule=dict(loss=0.9, grad_norm=0.05)), "stop_rule"), (dict(tau_learning_rate=None), "tau_learning_rate"),
                     (dict(tau_max_shift=0.5), "tau_max_shift"), (dict(tau_method="LM"), "tau_method"), (dict(tau_prior=-1.0), "tau_prior"),
                     (dict(tau_bounds=([0.0, 0.0], [1.0, 1.0])), "tau_bounds")):
        with pytest.raises(LfsdError, match=word):
            make(**kw)
    for bad in ([0.5, 0.5, 0.8], [0.5, 0.2, 0.8], [0.0, 0.5, 1.0][::-1]):
        with pytest.raises(LfsdError, match="taus"):
            make(args[0], args[1], bad, *args[3:])
    L = make(method=["Adam", "Vanilla"], tau_bounds=([0.1, 0.45, 0.7], [0.3, 0.55, 0.9]))
    assert L._tau["method"] == "Vanilla"
    L.step()
    assert bool((L.taus >= L._tau["lo"]).all()) and bool((L.taus <= L._tau["hi"]).all())


def test_driver_and_chord_length_times(emu):
    # the three-waypoint demonstration of tests/hyper_sweep_cases.py at QUAD_AVERAGE_SPEED = 1: each segment's chord length
    # rounded to 0.01, summed from 0 (by hand)
    pts = [[-2.0, -1.0, 0.6], [-1.0, -0.5, 0.9], [0.5, 0.2, 1.2], [1.8, 0.8, 1.4], [2.5, 1.0, 1.5]]
    seg = [round(float(np.sqrt(sum((a - b) ** 2 for a, b in zip(p, q)))), 2) for p, q in zip(pts[1:], pts[:-1])]
    assert seg == [1.16, 1.68, 1.45, 0.73]
    want = [0.0, 1.16, 1.16 + 1.68, 1.16 + 1.68 + 1.45, 1.16 + 1.68 + 1.45 + 0.73]
    got = CPDP.chord_length_times(pts, 1.0)
    assert got.tolist() == want
    assert CPDP.chord_length_times(pts, 2.0).tolist()[1] == 0.58
    with pytest.raises(LfsdError):
        CPDP.chord_length_times(pts[:1], 1.0)
    oc_q = models.quadrotor(n_grid=6)[0]
    new, ini, goal, demo = H.quad_driver(6, torch.float32, library=build_emu_library(oc_q))
    Q = new()
    Q.load_optimization_function(dict(method="Vanilla", learning_rate=1e-3, iter_num=2))
    res = Q.run(ini, goal, demo, ObsList=[], learn_taus=True, tau_learning_rate=1e-3)
    assert res["taus"].shape == (1, 3) and res["tau_trace"].shape == (3, 1, 3) and np.all(np.diff(res["taus"][0]) > 0)
    assert np.array_equal(res["tau_trace"][0][0], np.asarray(demo.time_list, dtype=res["taus"].dtype)) and not np.array_equal(res["tau_trace"][0], res["taus"])
    with pytest.raises(LfsdError, match="tau_learning_rate"):       # (the learner's refusal reaches the driver's caller)
        Q.run(ini, goal, demo, ObsList=[], learn_taus=True)


def test_recovery_of_known_times_follows_the_fp64_numpy_loop(emu):
    """Waypoints from the trajectory at theta* and tau*, a start shifted by +-0.3 of each gap, learning_rate = 0: first the numpy
    loop alone must bring max |tau - tau*| below a tenth of the initial shift (that is what tau_learning_rate and the step count were
    chosen for, tests/tau_cases.py), then the learner must follow its trace."""
    oc, env, d = models.pendulum(n_grid=10)
    emu(oc)
    oc.setDevice(dtype=F64)
    hz, iface = float(d["horizon"]), list(d["interface"])
    true = np.asarray(d["true_theta"], dtype=np.float64)
    star, start = C.recovery_start(hz)
    B, K = start.shape
    sol = oc.cocSolverBatch(np.tile(d["ini_state"], (B, 1)), hz, np.tile(true, (B, 1)))
    X = sol["state_grid"].numpy().copy()
    n_grid = X.shape[1] - 1
    h = hz / n_grid
    k = np.floor(star / h).astype(int)
    s = (star - k * h) / h
    wp = np.tile((X[0][k] + s[:, None] * (X[0][k + 1] - X[0][k]))[:, iface][None], (B, 1, 1))
    trace = C.numpy_tau_loop(X, hz, wp, start, C.RECOVER_LR, C.RECOVER_STEPS, C.RECOVER_C, tuple(iface))
    shift = np.abs(start - star).max()
    err = np.abs(trace - star).max(axis=(1, 2))
    print("numpy loop: initial shift %.4f, max |tau - tau*| after %d steps %.3e" % (shift, C.RECOVER_STEPS, err[-1]))
    assert err[-1] < 0.1 * shift and np.all(np.diff(trace, axis=2) > 0)
    L = CPDP.SparseDemoLearner(oc, np.tile(d["ini_state"], (B, 1)), hz, start, wp, iface, np.tile(true, (B, 1)), method="Vanilla",
                               learning_rate=0.0, learn_taus=True, tau_learning_rate=C.RECOVER_LR, tau_max_shift=C.RECOVER_C)
    worst, first = 0.0, None
    for it in range(C.RECOVER_STEPS):
        loss, _ = L.step()
        first = loss.clone() if first is None else first
        worst = max(worst, float(np.abs(L.taus.numpy() - trace[it + 1]).max()))
    print("learner against the numpy trace: max distance over %d steps %.3e (asserted < %.0e)" % (C.RECOVER_STEPS, worst, C.RECOVER_TOL))
    assert worst < C.RECOVER_TOL
    assert float(np.abs(L.taus.numpy() - star).max()) < 0.1 * shift and bool((loss < 1e-3 * first).all())
    assert torch.equal(L.theta, oc._t(np.tile(true, (B, 1))))


def _rows_ok(sol, aux):
    """The freeze mask of skip_unconverged, restated: converged or stalled, finite loss and gradient, no interval above tolerance."""
    st, loss, grad, stats = sol["status"], aux["loss"], aux["grad"], aux["stats"]
    return ((st == 1) | (st == 2)) & torch.isfinite(loss) & torch.isfinite(grad).all(dim=1) & ((stats[:, 1] + stats[:, 3]) == 0)


@pytest.mark.parametrize("mode", ["grouped", "shared"])
def test_grouped_and_shared_learners_are_their_launches(emu, mode):
    """G = 2 seeds x D = 3 demonstrations (grouped) and one theta for 3 demonstrations (shared), Vanilla, skip_unconverged at its
    default (on): theta, the per-row times and their moments against the launches made by hand, bit for bit -- the times of a row
    follow the ROW's freeze mask and its own demonstration, whatever its group does."""
    oc, args = _learner_args(emu, rows=6)
    lib = oc.compile()
    D, lr, tlr, c = 3, 1e-2, 2e-3, 0.25
    taus_d = np.array([[0.2, 0.5, 0.8], [0.25, 0.5, 0.75], [0.1, 0.4, 0.9]])
    wps_d = np.array([[[0.4], [1.5], [2.6]], [[0.5], [1.4], [2.4]], [[0.2], [1.1], [2.8]]])
    G = 2 if mode == "grouped" else 1
    B = G * D
    th0 = args[5][:G]
    kw = dict(mode=mode, method="Vanilla", learning_rate=lr, learn_taus=True, tau_learning_rate=tlr)
    if mode == "grouped":
        kw["demos_per_seed"] = D
    L = CPDP.SparseDemoLearner(oc, args[0][:D], 1.0, taus_d, wps_d, [0], th0 if mode == "grouped" else th0[0], **kw)
    theta = oc._t(th0).clone()
    x0, hz = oc._t(np.tile(args[0][:D], (G, 1))), oc._t(1.0).expand(B).contiguous()
    taus, wps = oc._t(np.tile(taus_d, (G, 1))).contiguous(), oc._t(np.tile(wps_d, (G, 1, 1))).contiguous()
    z = lambda t: torch.zeros_like(t)
    m, v, vh, mt, vt, vht = z(theta), z(theta), z(theta), z(taus), z(taus), z(taus)
    idx = torch.tensor([0], dtype=torch.int32)
    frozen_seen = any_ok = False
    for it in range(4):
        L.step()
        sol = oc.cocSolverBatch(x0, hz, theta.repeat_interleave(D, dim=0).contiguous())
        aux = oc.auxSysSolverBatch(sol, taus, wps, [0], validate=False, skip_status=(3, 4))
        ok = _rows_ok(sol, aux)
        oki = ok.to(torch.int32)
        frozen_seen, any_ok = frozen_seen or not bool(ok.all()), any_ok or bool(ok.any())
        dtau = lib.waypoint_time_grad(sol["state_grid"], hz, taus, wps, idx)
        grad = torch.where(ok.unsqueeze(1), aux["grad"], z(aux["grad"]))
        if mode == "grouped":
            _, gg, _, n_ok = lib.group_reduce(aux["loss"].contiguous(), grad.contiguous(), D, row_ok=oki)
            lib.optimizer_step("Vanilla", theta, gg, it, lr, m=m, v=v, vhat=vh, proj_lo=L.proj_lo, row_active=(n_ok > 0).to(torch.int32))
        else:
            lib.optimizer_step("Vanilla", theta, grad.sum(dim=0, keepdim=True).contiguous(), it, lr, m=m, v=v, vhat=vh, proj_lo=L.proj_lo)
        start = taus.clone()
        lib.optimizer_step("Vanilla", taus, dtau, it, tlr, m=mt, v=vt, vhat=vht, row_active=oki)
        lib.tau_project(start, taus, hz, c, row_active=oki)
        assert torch.equal(L.theta, theta) and torch.equal(L.taus, taus) and H.same(L.tau_grad, dtau), (mode, it)
        assert torch.equal(L.m_tau, mt) and torch.equal(L.v_tau, vt)
    assert torch.equal(L.taus, L.tau0) != any_ok      # (the error-controlled sweeps may freeze every row of so small a batch)
    print("%s: a row was frozen in some step: %s" % (mode, frozen_seen))
