"""CPU tier of several demonstrations per seed (ABI 15): lfsd_group_reduce through the SIMT emulator against the sequential sum on the
CPU, bit for bit; every LFSD_EINVAL case on host dummies (emulator and gfx950 library) and the binding's own refusals; the grouped
learner against the same launches made by hand, against the independent learner (D = 1) and the shared one (G = 1); frozen rows and
groups; its combinations and refusals; the ground-truth case.  Cases and bounds: tests/group_cases.py."""
import numpy as np
import pytest
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models, runtime
from lfsd_amd.runtime import LfsdError
from conftest import build_emu_library
import hyper_sweep_cases as H
import sample_cases as S
import group_cases as C

F64 = torch.float64
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, F64], ids=["fp32", "fp64"])
SHAPES = pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "G%dD%dp%d" % s)


@pytest.fixture(scope="module")
def lib():
    return runtime.ModelLibrary(build_emu_library(models.pendulum(n_grid=10)[0]))


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------
@DTYPES
@SHAPES
@pytest.mark.parametrize("with_H", [False, True], ids=["noH", "H"])
@pytest.mark.parametrize("masked", [False, True], ids=["all", "mask"])
def test_group_reduce_is_the_sequential_sum(lib, shape, dtype, with_H, masked):
    C.run_group_reduce(lib, "cpu", dtype, *shape, with_H, masked)


@DTYPES
def test_a_nan_in_a_counted_row_propagates(lib, dtype):
    C.run_group_reduce_nan(lib, "cpu", dtype)


@pytest.mark.parametrize("which", ["emulator", "hip"])
def test_entry_point_refuses_bad_arguments_before_any_launch(lib, which):
    """Host dummies stand in for the arrays: no launch is reached (the gfx950 library loads without a GPU, as in tests/test_capi.py)."""
    ml = lib if which == "emulator" else models.pendulum(n_grid=10)[0].compile()
    C.group_reduce_einval(ml.lib, launches=which == "emulator")
    if which == "hip":                                          # no CPU fallback: the HIP library refuses host memory
        with pytest.raises(LfsdError):
            ml.group_reduce(torch.zeros(6, dtype=F64), torch.zeros((6, 2), dtype=F64), 3)
        return
    for bad in C.binding_refusals(ml):                          # ... and the binding refuses what it can see
        with pytest.raises(LfsdError):
            bad()


# ---- 2. the learner ---------------------------------------------------------------------------------------------------------------
def _pendulum(emu, G=3):
    oc, env, d = models.pendulum(n_grid=10)
    emu(oc)
    oc.setDevice(dtype=F64)
    oc.setSolverOptions(**C.FIXED_SUBSTEPS)
    args = C.pendulum_args(d, G, seed_rows=8)
    D = len(C.PENDULUM_DEMOS["horizon"])

    def make(groups=G, **kw):
        return CPDP.SparseDemoLearner(oc, *args[:5], args[5][:groups], mode="grouped", demos_per_seed=D, **kw)
    return oc, d, args, D, make


@pytest.mark.parametrize("rule", ["nesterov_true_loss", "LM"])
def test_pendulum_learner_is_its_launches(emu, rule):
    oc, d, args, D, make = _pendulum(emu)
    C.run_composition(make, oc, args, 3, D, "LM" if rule == "LM" else C.NESTEROV, lambda0=30.0)


@pytest.mark.parametrize("true_loss", [False, True], ids=["flag_off", "true_loss"])
def test_pendulum_learner_with_a_rule_per_group_is_its_launches(emu, true_loss):
    """true_loss: the scalar flag with a rule list -- the Nesterov group alone takes the second evaluation."""
    oc, d, args, D, make = _pendulum(emu, G=5)
    C.run_composition(make, oc, args, 5, D, C.rules_kwargs(5, true_loss))


def test_level_2_with_warm_start_is_its_launches(emu):
    oc, d, args, D, make = _pendulum(emu)
    C.run_composition(make, oc, args, 3, D, dict(method="Adam", learning_rate=0.05), steps=3, level=2, warm=True)


def test_quadrotor_learner_is_its_launches(emu):
    """G = D = 3 here (the emulator's run time); the -m gpu tier runs G = D = 6."""
    oc, env, d = models.quadrotor(n_grid=10)
    emu(oc)
    oc.setDevice(dtype=torch.float32)
    G = D = 3
    args = C.quadrotor_args(d, G, D)

    def make(groups=G, **kw):
        return CPDP.SparseDemoLearner(oc, *args[:5], args[5][:groups], mode="grouped", demos_per_seed=D, **kw)
    C.run_composition(make, oc, args, G, D, "LM", steps=2, lambda0=300.0)


@pytest.mark.parametrize("method", ["Adam", "LM", "Adam_level2_warm"])
def test_one_demonstration_per_seed_is_the_independent_learner(emu, method):
    oc, d, args, D, make = _pendulum(emu)
    x0, hz, taus, wps = C.tiled(oc, args, 1, D)                # three rows, one demonstration each
    kw = dict(method=method.split("_")[0], learning_rate=0.05, lm_lambda0=30.0)
    if method.endswith("warm"):
        kw.update(interplation_level=2, warm_start=True)
    C.run_one_demonstration_is_independent(
        lambda: CPDP.SparseDemoLearner(oc, x0, hz, taus, wps, [0], args[5][:3], mode="grouped", demos_per_seed=1, **kw),
        lambda: CPDP.SparseDemoLearner(oc, x0, hz, taus, wps, [0], args[5][:3], skip_unconverged=True, **kw))


def test_one_group_against_the_shared_learner(emu):
    oc, d, args, D, make = _pendulum(emu)
    lr = 0.05
    C.run_one_group_against_shared(lambda **kw: CPDP.SparseDemoLearner(oc, *C.tiled(oc, args, 1, D), [0], args[5][:1], method="Vanilla",
                                                                        learning_rate=lr, **kw), D, lr)


@pytest.mark.parametrize("method", ["Adam", "LM"])
def test_frozen_rows_and_groups(emu, method):
    oc, d, args, D, make = _pendulum(emu)
    L = make(method=method, learning_rate=0.05, lm_lambda0=30.0)      # (damped enough for every solve to converge)
    C.run_frozen(L, D, ("m", "v") if method == "Adam" else ("theta_trial", "lm_lambda", "lm_loss", "normal_matrix"))


def test_trace_level_2_and_warm_start(emu):
    oc, d, args, D, make = _pendulum(emu)
    a = make(method="Adam", learning_rate=0.05, trace=3)
    b = make(method="Adam", learning_rate=0.05, interplation_level=2, warm_start=True)
    assert a.loss_trace.shape == (3, 3) and a.grad_norm_trace.shape == (3, 3) and a.theta_trace.shape == (3, 4, 3)
    assert torch.equal(a.theta_trace[:, 0], a.theta)
    for k in range(3):
        la, ga = a.step()
        lb, gb = b.step()
        assert torch.equal(a.theta_trace[:, k + 1], a.theta) and torch.equal(a.loss_trace[:, k], la)
        assert torch.allclose(a.grad_norm_trace[:, k], torch.linalg.norm(ga, dim=1), rtol=1e-12)
        assert lb.shape == (3,) and bool(torch.isfinite(lb).all()) and bool((b.n_ok == D).all())
        assert not bool((ga == gb).all())                       # (level 2: other sensitivities)
    assert bool(torch.isnan(a.theta_trace).sum() == 0)
    with pytest.raises(LfsdError):
        a.step()                                                # beyond the capacity


def test_squared_loss_fn_is_the_fused_loss(emu):
    oc, d, args, D, make = _pendulum(emu)
    fused = make()
    cust = CPDP.SparseDemoLearner(oc, *args[:3], None, None, args[5][:3], mode="grouped", demos_per_seed=D,
                                  loss_fn=S.squared_waypoint_loss([0], fused.wps), grad_scale=0.5)
    lf, gf = fused.evaluate(fused.theta)
    lc, gc = cust.evaluate(cust.theta)
    assert lf.shape == lc.shape == (3,) and gc.shape == (3, 3) and cust.row_loss.shape == (9,)
    _, _, bl, bg = S.fused_reference(cust._sol["state_grid"], cust._aux["auxX_grid"], cust.hz, cust.taus, fused.wps, [0])
    eps = S.eps_of(F64)
    assert bool(((cust.row_loss - fused.row_loss).abs() <= 2 * bl * eps).all())
    assert bool(((cust.row_grad - fused.row_grad).abs() <= 2 * bg * eps).all())
    grp = lambda t: t.reshape((3, D) + tuple(t.shape[1:])).sum(dim=1)
    bound_l = grp(2 * bl * eps) + (D - 1) * eps * grp(fused.row_loss.abs())
    bound_g = grp(2 * bg * eps) + (D - 1) * eps * grp(fused.row_grad.abs())
    print("loss_fn against fused, group sums: error / bound", float(((lc - lf).abs() / bound_l).max()), float(((gc - gf).abs() / bound_g).max()))
    assert bool(((lc - lf).abs() <= bound_l).all()) and bool(((gc - gf).abs() <= bound_g).all())
    lc2, _ = cust.step()
    assert torch.equal(lc2, lc) and bool((cust.n_ok == D).all())


def test_refusals(emu, monkeypatch):
    oc, d, args, D, make = _pendulum(emu)
    with pytest.raises(LfsdError, match="stop_rule"):
        make(stop_rule=dict(loss=0.9, grad_norm=0.05))
    with pytest.raises(LfsdError, match="all-reduce"):
        make(process_group=object())
    with pytest.raises(LfsdError, match="scalar"):
        make(method="Nesterov", true_loss_print_flag=[True, False, True])
    with pytest.raises(LfsdError, match="whole number"):
        CPDP.SparseDemoLearner(oc, np.zeros((7, 2)), 1.0, [0.2, 0.5], [[0.4], [1.5]], [0], d["theta0"], mode="grouped", demos_per_seed=3)
    for mode in ("independent", "shared"):
        with pytest.raises(LfsdError, match="demos_per_seed"):
            CPDP.SparseDemoLearner(oc, *args[:5], d["theta0"], mode=mode, demos_per_seed=3)
    with pytest.raises(LfsdError, match="demos_per_seed"):
        CPDP.SparseDemoLearner(oc, *args[:5], args[5][:3], mode="grouped")
    with pytest.raises(LfsdError, match="theta0"):               # 9 rows are 3 groups: 2 parameter vectors are neither 1 nor 3
        CPDP.SparseDemoLearner(oc, np.zeros((9, 2)), 1.0, [0.2, 0.5], [[0.4], [1.5]], [0], args[5][:2], mode="grouped", demos_per_seed=3)
    with pytest.raises(LfsdError, match="ini_state"):            # 4 parameter vectors make 12 rows: 6 start states are neither 3 nor 12
        CPDP.SparseDemoLearner(oc, np.zeros((6, 2)), 1.0, [0.2, 0.5], [[0.4], [1.5]], [0], args[5][:4], mode="grouped", demos_per_seed=3)
    for kw in (dict(learning_rate=[0.1] * 9), dict(method=["Adam"] * 2), dict(mu=np.full(4, 0.9))):
        with pytest.raises(LfsdError, match="groups"):
            make(**kw)
    with pytest.raises(LfsdError, match="rows path"):
        make(method=["LM", "Adam", "LM"])
    with pytest.raises(LfsdError, match="sum of squares"):
        make(method="LM", loss_fn=lambda x, u: (x ** 2).sum((1, 2)))
    # evaluate() takes theta [G, p] or [1, p]: anything else would send the gather's index row // D past the end of theta
    L = make()
    th = L.theta.clone()
    for bad in (th[:2], th.repeat(3, 1), th[:, :2], th.float(), th[0], th.numpy()):
        with pytest.raises(LfsdError, match="grouped"):
            L.evaluate(bad)
    one = L.evaluate(th[:1])[0].clone()
    assert torch.equal(one, L.evaluate(th[:1].expand(3, -1).contiguous())[0]) and one.shape == (3,)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    with pytest.raises(LfsdError, match="all-reduce"):
        make()


def test_the_launches_of_each_mode(emu, monkeypatch):
    """The new launches belong to mode='grouped' alone; its hook gets the one new phase name."""
    oc, d, args, D, make = _pendulum(emu)
    ml = oc.compile()
    calls = {}
    for name in ("group_reduce", "gather_rows", "normal_matrix", "lm_step", "optimizer_step"):
        def wrapped(*a, _fn=getattr(ml, name), _name=name, **kw):
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(*a, **kw)
        monkeypatch.setattr(ml, name, wrapped)
    x0, hz, taus, wps = C.tiled(oc, args, 3, D)
    for mode, th in (("independent", args[5][:1]), ("shared", args[5][:1])):
        phases = []
        L = CPDP.SparseDemoLearner(oc, x0, hz, taus, wps, [0], th, mode=mode, method="Adam")
        L.event_hook = phases.append
        L.step()
        assert calls == {"optimizer_step": 1} and phases == ["oc_solve", "aux_riccati", "aux_forward", "update", "end"], (mode, calls, phases)
        calls.clear()
    phases = []
    L = make(method="LM")
    L.event_hook = phases.append
    L.step()
    assert calls == {"gather_rows": 1, "normal_matrix": 1, "group_reduce": 1, "lm_step": 1}
    assert phases == ["oc_solve", "aux_riccati", "aux_forward", "normal_matrix", "group_reduce", "update", "end"]


def test_grouped_lm_learns_the_ground_truth(emu):
    """At N = LEARN_STEPS and, for the margin the case was chosen with, at N - 2 (figures observed: tests/group_cases.py)."""
    def make_oc():
        oc, env, d = models.pendulum(n_grid=10)
        emu(oc)
        oc.setDevice(dtype=F64)
        return oc, d
    C.run_learns(make_oc, checkpoints=(C.LEARN_STEPS - 2, C.LEARN_STEPS))
