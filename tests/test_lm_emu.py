"""CPU tier of the Levenberg-Marquardt outer update (ABI 14): lfsd_normal_matrix and lfsd_lm_step through the SIMT emulator against
an fp64 restatement / known branches; every LFSD_EINVAL case on host dummies (emulator and gfx950 library); the LM learner against
the same launches made by hand, bit for bit; its combinations and refusals.  Cases and bounds: tests/lm_cases.py."""
import numpy as np
import pytest
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models, runtime
from lfsd_amd.runtime import LfsdError
from conftest import build_emu_library
import hyper_sweep_cases as H
import lm_cases as C

F64 = torch.float64
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, F64], ids=["fp32", "fp64"])
SHAPES = pytest.mark.parametrize("shape", C.SHAPES_EMU, ids=lambda s: "B%dp%d" % s)


@pytest.fixture(scope="module")
def lib():
    return runtime.ModelLibrary(build_emu_library(models.pendulum(n_grid=10)[0]))


# ---- 1. kernels -----------------------------------------------------------------------------------------------------------------
@DTYPES
@SHAPES
def test_normal_matrix_against_fp64_restatement(lib, shape, dtype):
    B, p = shape
    for n_grid in C.N_GRIDS:
        for K in C.N_WAYPOINTS:
            rh, rg = C.run_normal_matrix(lib, "cpu", dtype, B, p, n_grid, K)
            print("normal_matrix B%d p%d n_grid %d K %d: |H - ref| / bound %.3f, |J^T r - vjp| / bound %.3f" % (B, p, n_grid, K, rh, rg))
            assert rh <= 1.0 and rg <= 1.0, (n_grid, K, rh, rg)
            rs = C.run_normal_matrix_general(lib, "cpu", dtype, B, p, n_grid, K)
            print("    sign-changing sensitivities: |H - ref| / bound %.3f" % rs)
            assert rs <= 1.0, (n_grid, K, rs)


@DTYPES
@SHAPES
def test_lm_step_walks_the_known_branches(lib, shape, dtype):
    B, p = shape
    for offset in (range(2 * C.KINDS) if B < 2 * C.KINDS else (0,)):      # a small batch: every kind and variant in turn
        worst = C.run_lm_step(lib, "cpu", dtype, B, p, offset)
        assert worst <= 1.0, (offset, worst)
    print("lm_step B%d p%d: worst backward error / bound %.3f" % (B, p, worst))


@pytest.mark.parametrize("which", ["emulator", "hip"])
def test_entry_points_refuse_bad_arguments_before_any_launch(lib, which):
    """Host dummies stand in for the arrays: no launch is reached (the gfx950 library loads without a GPU, as in tests/test_capi.py)."""
    ml = lib if which == "emulator" else models.pendulum(n_grid=10)[0].compile()
    C.normal_matrix_einval(ml.lib)
    C.lm_step_einval(ml.lib)
    z = lambda *s: torch.zeros(s, dtype=F64)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    if which == "hip":                                          # no CPU fallback: the HIP library refuses host memory
        with pytest.raises(LfsdError):
            ml.normal_matrix(z(2), z(2, 3), z(2, 4, 3, 2), i32(1))
        with pytest.raises(LfsdError):
            ml.lm_step(z(2, 3), z(2), z(2, 3), z(2, 3, 3), z(2), z(2, 3), z(2), z(2, 3), z(2, 3, 3))
        return
    # ... and the binding refuses what it can see
    for bad in (lambda: ml.normal_matrix(z(2), z(2, 3), z(2, 4, 3), i32(1)),                      # auxX_grid is [B, N+1, p, n]
                lambda: ml.normal_matrix(z(3), z(2, 3), z(2, 4, 3, 2), i32(1)),                   # horizon of another batch
                lambda: ml.normal_matrix(z(2), z(2, 3).float(), z(2, 4, 3, 2), i32(1)),           # taus in the grid's dtype
                lambda: ml.normal_matrix(z(2), z(2, 3), z(2, 4, 3, 2), torch.zeros(1, dtype=torch.int64)),
                lambda: ml.normal_matrix(z(2), z(2, 3), z(2, 1, 3, 2), i32(1)),                   # one node is no interval
                lambda: ml.normal_matrix(z(2), z(2, 3), z(2, 4, 3, 2), i32(1), out=z(2, 3, 2)),
                lambda: ml.lm_step(z(2, 17), z(2), z(2, 17), z(2, 17, 17), z(2), z(2, 17), z(2), z(2, 17), z(2, 17, 17)),
                lambda: ml.lm_step(z(2, 3), z(2), z(2, 3), z(2, 3, 2), z(2), z(2, 3), z(2), z(2, 3), z(2, 3, 3)),
                lambda: ml.lm_step(z(2, 3), z(2), z(2, 3), z(2, 3, 3), z(2), z(2, 3), z(2), z(2, 3), None),
                lambda: ml.lm_step(z(2, 3), z(2), z(2, 3), z(2, 3, 3), z(2).float(), z(2, 3), z(2), z(2, 3), z(2, 3, 3)),
                lambda: ml.lm_step(z(2, 3), z(2), z(2, 3), z(2, 3, 3), z(2), z(2, 3), z(2), z(2, 3), z(2, 3, 3), accepted=z(2))):
        with pytest.raises(LfsdError):
            bad()
    with pytest.raises(LfsdError):                              # the entry point's own refusal reaches the caller
        ml.lm_step(z(2, 3), z(2), z(2, 3), z(2, 3, 3), z(2), z(2, 3), z(2), z(2, 3), z(2, 3, 3), lambda_up=0.5)


# ---- 2. the learner ---------------------------------------------------------------------------------------------------------------
def _pendulum(emu, rows=8, n_grid=10):
    oc, env, d = models.pendulum(n_grid=n_grid)
    emu(oc)
    oc.setDevice(dtype=F64)
    seeds = C.compose_seeds(d["theta0"], rows)
    args = (np.tile(d["ini_state"], (rows, 1)), 1.0, [0.2, 0.5, 0.8], [[0.4], [1.5], [2.6]], [0], seeds)

    def make(rows=slice(None), **kw):
        return CPDP.SparseDemoLearner(oc, args[0][rows], *args[1:5], args[5][rows], method="LM", **kw)
    return oc, args, make


def test_pendulum_learner_is_its_launches(emu):
    oc, args, make = _pendulum(emu)
    C.run_composition(make, oc, args, C.COMPOSE_LAMBDA0["pendulum"])


def test_quadrotor_learner_is_its_launches(emu):
    oc, env, d = models.quadrotor(n_grid=10)
    emu(oc)
    oc.setDevice(dtype=torch.float32)
    rows = 12
    seeds = C.compose_seeds(d["theta0"], rows)
    args = (np.tile(d["ini_state"], (rows, 1)), d["horizon"], d["taus"], d["waypoints"], d["interface"], seeds)

    def make(rows=slice(None), **kw):
        return CPDP.SparseDemoLearner(oc, args[0][rows], *args[1:5], args[5][rows], method="LM", **kw)
    C.run_composition(make, oc, args, C.COMPOSE_LAMBDA0["quadrotor"])


def test_lm_learns_the_ground_truth(emu):
    """At N = 12 steps and, for the margin the case was chosen with, at N = 10 (figures observed: tests/lm_cases.py)."""
    def make_oc():
        oc, env, d = models.pendulum(n_grid=10)
        emu(oc)
        oc.setDevice(dtype=F64)
        return oc, d
    C.run_learns(make_oc, checkpoints=(C.LEARN_STEPS - 2, C.LEARN_STEPS))


def test_stop_rule_freezes_the_stopped_seed(emu):
    """A seed that meets the reference's test at once next to seeds that go on: its row is frozen, the survivors hold the bits of the
    learner without the rule up to their own stop."""
    oc, args, make = _pendulum(emu, rows=4)
    K = 4
    free = make(lm_lambda0=30.0)                              # (damped enough for the survivors to accept and move)
    hist = []
    for _ in range(K):
        l, g = free.step()
        hist.append((l.clone(), g.clone(), free.theta.clone(), free.theta_trial.clone(), free.lm_lambda.clone(), free.lm_loss.clone()))
    first = hist[0][0]
    order = torch.argsort(first)
    rule = dict(loss=float(0.5 * (first[order[0]] + first[order[1]])), grad_norm=1e-12)      # the best seed stops after step 1
    L = make(stop_rule=rule, trace=K, lm_lambda0=30.0)
    stopped_at = {}
    for k in range(K):
        if L.n_active == 0:
            break
        l, g = L.step()
        stop = L.stop_iter.clone()
        for b in range(L.B):
            s = int(stop[b])
            if s and b not in stopped_at:
                stopped_at[b] = (s, L.theta[b].clone(), L.theta_trial[b].clone(), L.lm_lambda[b].clone(), L.lm_loss[b].clone())
            if not s or s == k + 1:                       # still learning, or stopping in this step: the free learner's bits
                for a, ref in zip((l, g, L.theta, L.theta_trial, L.lm_lambda, L.lm_loss), hist[k]):
                    assert H.same(a[b], ref[b]), (k, b)
    assert int(order[0]) in stopped_at and stopped_at[int(order[0])][0] == 1 and len(stopped_at) < L.B + 1
    for b, (s, th, tr, lam, lo) in stopped_at.items():    # frozen from its stop on: every word of its LM state
        assert torch.equal(L.theta[b], th) and torch.equal(L.theta_trial[b], tr) and torch.equal(L.lm_lambda[b], lam)
        assert torch.equal(L.lm_loss[b], lo)
        assert torch.equal(L.theta_trace[b, s], th) and bool(torch.isnan(L.theta_trace[b, s + 1:]).all())
    assert L.n_active < L.B


def test_skip_unconverged_keeps_the_lm_state_of_a_frozen_row(emu):
    oc, args, make = _pendulum(emu, rows=8)
    C.run_skip_unconverged(make, oc, args[0], args[1])


def test_level_2_and_trace(emu):
    oc, args, make = _pendulum(emu, rows=3)
    a, b = make(trace=6, lm_lambda0=30.0), make(interplation_level=2, warm_start=True, lm_lambda0=30.0)
    for k in range(6):
        la, _ = a.step()
        assert torch.equal(a.theta_trace[:, k + 1], a.theta) and torch.equal(a.loss_trace[:, k], la)
        if k < 2:      # level 2 runs and differs: not in the first loss (these waypoint times are grid nodes, where the two
            lb, _ = b.step()      # interpolants of x agree) but in the sensitivities, so in the next trial point and its loss
            assert bool(torch.isfinite(lb).all()) and (k == 0 or not bool((la == lb).any()))
    assert bool(torch.isfinite(b.lm_loss).all()) and bool(b.lm_accepted.all())
    assert bool((a.theta_trace[:, 1] == torch.as_tensor(args[5][:3])).all())                    # step 1 accepts theta_0 itself
    assert bool((a.theta_trace[:, 6] != a.theta_trace[:, 1]).any(dim=1).all())                  # ... and the accepted point moves
    with pytest.raises(LfsdError):
        a.step()                                                                                 # beyond the capacity


def test_refusals(emu):
    oc, args, make = _pendulum(emu, rows=4)
    with pytest.raises(LfsdError, match="sum of squares"):
        make(loss_fn=lambda x, u: (x ** 2).sum((1, 2)))
    with pytest.raises(LfsdError, match="independent"):
        CPDP.SparseDemoLearner(oc, *args[:5], args[5][:1], method="LM", mode="shared")
    for kw in (dict(learning_rate=[0.1] * 4), dict(mu=np.full(4, 0.9)), dict(true_loss_print_flag=[False] * 4)):
        with pytest.raises(LfsdError, match="rows path"):
            make(**kw)
    with pytest.raises(LfsdError, match="rows path"):
        CPDP.SparseDemoLearner(oc, *args, method=["LM", "Adam", "LM", "Vanilla"])
    with pytest.raises(LfsdError, match="interface"):
        CPDP.SparseDemoLearner(oc, *args[:4], None, args[5], method="LM")
    for kw in (dict(lm_down=0.0), dict(lm_up=0.5), dict(lm_min=0.0), dict(lm_lambda0=1e9)):
        with pytest.raises(LfsdError):
            make(**kw)


def test_quadalgorithm_runs_lm_per_seed(emu):
    lib_path = build_emu_library(models.quadrotor(n_grid=10)[0])
    new, ini, goal, demo = H.quad_driver(10, F64, library=lib_path)
    Q = new()
    Q.load_optimization_function(dict(method="LM", iter_num=3, lm_lambda0=1e-2, lm_down=1.0 / 3.0, lm_up=2.0, lm_min=1e-8, lm_max=1e8))
    seeds = np.array([1, 0.1, 0.1, 0.1, 0.1, 0.1, -1], dtype=float)[None, :] * np.array([[1.0], [1.3]])
    res = Q.run(ini, goal, demo, ObsList=[], initial_parameters=seeds, stop="per_seed")
    n = res["loss_trace"].shape[0]
    assert 1 <= n <= 3 and res["loss_trace"].shape == (n, 2) and res["parameter_trace"].shape == (n + 1, 2, 7)
    assert res["stop_iter"].shape == (2,) and np.isfinite(res["loss_trace"]).all()
    assert Q.learner.method == "LM" and Q.learner.lm_lambda.shape == (2,)
    with pytest.raises(LfsdError, match="rows path"):
        new().run_comparison([dict(method="LM", iter_num=2), dict(method="Vanilla", learning_rate=0.06, iter_num=2)], ini, goal, demo)


def test_the_five_rules_take_the_launches_they_took(emu, monkeypatch):
    oc, args, make = _pendulum(emu, rows=2)
    ml = oc.compile()
    calls, grids = {}, []
    for name in ("normal_matrix", "lm_step", "optimizer_step"):
        def wrapped(*a, _fn=getattr(ml, name), _name=name, **kw):
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(*a, **kw)
        monkeypatch.setattr(ml, name, wrapped)
    aux_solve = ml.aux_solve

    def spy(*a, **kw):
        grids.append(bool(kw.get("want_grids", False)))
        return aux_solve(*a, **kw)
    monkeypatch.setattr(ml, "aux_solve", spy)
    L = CPDP.SparseDemoLearner(oc, *args, method="Vanilla", learning_rate=1e-2)
    L.step(); L.step()
    assert calls == {"optimizer_step": 2} and grids == [False, False]
    assert L.lm_lambda is None and L.normal_matrix is None and L._aux["auxX_grid"] is None
    calls.clear(); grids.clear()
    L = make()
    L.step(); L.step()
    assert calls == {"normal_matrix": 2, "lm_step": 2} and grids == [True, True]
