"""GPU tier of several demonstrations per seed (ABI 15): lfsd_group_reduce of the gfx950 library at the shapes of tests/group_cases.py
(one element, a group that straddles a workgroup, a partial last workgroup) against the sequential sum on the CPU, bit for bit; the
grouped learner against the same launches made by hand (pendulum fp64 G = D = 3, quadrotor fp32 G = D = 6), against the independent
learner (D = 1) and the shared one (G = 1); frozen rows and groups; the ground-truth case.  The same cases pass on the SIMT emulator
(tests/test_groups_emu.py)."""
import pytest
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models
from lfsd_amd.runtime import LfsdError
import sample_cases as S
import group_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, F64], ids=["fp32", "fp64"])
SHAPES = pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "G%dD%dp%d" % s)


@pytest.fixture(scope="module")
def lib():
    return models.pendulum(n_grid=10)[0].compile()


@DTYPES
@SHAPES
@pytest.mark.parametrize("with_H", [False, True], ids=["noH", "H"])
@pytest.mark.parametrize("masked", [False, True], ids=["all", "mask"])
def test_group_reduce_is_the_sequential_sum_on_the_device(lib, shape, dtype, with_H, masked):
    C.run_group_reduce(lib, DEV, dtype, *shape, with_H, masked)


@DTYPES
def test_a_nan_in_a_counted_row_propagates_on_the_device(lib, dtype):
    C.run_group_reduce_nan(lib, DEV, dtype)


def test_entry_point_refuses_bad_arguments_before_any_launch_on_the_device(lib):
    C.group_reduce_einval(lib.lib, launches=False)
    with pytest.raises(LfsdError):                              # no CPU fallback: host memory is refused by the binding
        lib.group_reduce(torch.zeros(6, dtype=F64), torch.zeros((6, 2), dtype=F64), 3)


def _pendulum(G=3):
    oc, env, d = models.pendulum(n_grid=10)
    oc.setDevice(DEV, F64)
    oc.setSolverOptions(**C.FIXED_SUBSTEPS)
    args = C.pendulum_args(d, G, seed_rows=8)
    D = len(C.PENDULUM_DEMOS["horizon"])

    def make(groups=G, **kw):
        return CPDP.SparseDemoLearner(oc, *args[:5], args[5][:groups], mode="grouped", demos_per_seed=D, **kw)
    return oc, d, args, D, make


@pytest.mark.parametrize("rule", ["nesterov_true_loss", "LM"])
def test_pendulum_learner_is_its_launches_on_the_device(rule):
    oc, d, args, D, make = _pendulum()
    C.run_composition(make, oc, args, 3, D, "LM" if rule == "LM" else C.NESTEROV, lambda0=30.0)


@pytest.mark.parametrize("true_loss", [False, True], ids=["flag_off", "true_loss"])
def test_pendulum_learner_with_a_rule_per_group_is_its_launches_on_the_device(true_loss):
    """true_loss: the scalar flag with a rule list -- the Nesterov group alone takes the second evaluation."""
    oc, d, args, D, make = _pendulum(G=5)
    C.run_composition(make, oc, args, 5, D, C.rules_kwargs(5, true_loss))


def test_level_2_with_warm_start_is_its_launches_on_the_device():
    oc, d, args, D, make = _pendulum()
    C.run_composition(make, oc, args, 3, D, dict(method="Adam", learning_rate=0.05), steps=3, level=2, warm=True)


@pytest.mark.parametrize("rule", ["rules", "LM"])
def test_quadrotor_learner_is_its_launches_on_the_device(rule):
    """G = D = 6: 36 rows, fp32, default mapping."""
    oc, env, d = models.quadrotor(n_grid=10)
    oc.setDevice(DEV, torch.float32)
    G = D = 6
    args = C.quadrotor_args(d, G, D)

    def make(groups=G, **kw):
        return CPDP.SparseDemoLearner(oc, *args[:5], args[5][:groups], mode="grouped", demos_per_seed=D, **kw)
    C.run_composition(make, oc, args, G, D, "LM" if rule == "LM" else C.rules_kwargs(G), steps=3, lambda0=300.0)


@pytest.mark.parametrize("method", ["Adam", "LM", "Adam_level2_warm"])
def test_one_demonstration_per_seed_is_the_independent_learner_on_the_device(method):
    oc, d, args, D, make = _pendulum()
    x0, hz, taus, wps = C.tiled(oc, args, 1, D)
    kw = dict(method=method.split("_")[0], learning_rate=0.05, lm_lambda0=30.0)
    if method.endswith("warm"):
        kw.update(interplation_level=2, warm_start=True)
    C.run_one_demonstration_is_independent(
        lambda: CPDP.SparseDemoLearner(oc, x0, hz, taus, wps, [0], args[5][:3], mode="grouped", demos_per_seed=1, **kw),
        lambda: CPDP.SparseDemoLearner(oc, x0, hz, taus, wps, [0], args[5][:3], skip_unconverged=True, **kw))


def test_one_group_against_the_shared_learner_on_the_device():
    oc, d, args, D, make = _pendulum()
    lr = 0.05
    C.run_one_group_against_shared(lambda **kw: CPDP.SparseDemoLearner(oc, *C.tiled(oc, args, 1, D), [0], args[5][:1], method="Vanilla",
                                                                        learning_rate=lr, **kw), D, lr)


@pytest.mark.parametrize("method", ["Adam", "LM"])
def test_frozen_rows_and_groups_on_the_device(method):
    oc, d, args, D, make = _pendulum()
    L = make(method=method, learning_rate=0.05, lm_lambda0=30.0)
    C.run_frozen(L, D, ("m", "v") if method == "Adam" else ("theta_trial", "lm_lambda", "lm_loss", "normal_matrix"))


def test_trace_level_2_warm_start_and_loss_fn_on_the_device():
    oc, d, args, D, make = _pendulum()
    a = make(method="Adam", learning_rate=0.05, trace=3)
    b = make(method="Adam", learning_rate=0.05, interplation_level=2, warm_start=True)
    for k in range(3):
        la, ga = a.step()
        lb, gb = b.step()
        assert torch.equal(a.theta_trace[:, k + 1], a.theta) and torch.equal(a.loss_trace[:, k], la)
        assert bool(torch.isfinite(lb).all()) and bool((b.n_ok == D).all()) and not bool((ga == gb).all())
    assert a.loss_trace.shape == (3, 3) and a.theta_trace.shape == (3, 4, 3) and int(torch.isnan(a.theta_trace).sum()) == 0
    fused = make()
    cust = CPDP.SparseDemoLearner(oc, *args[:3], None, None, args[5][:3], mode="grouped", demos_per_seed=D,
                                  loss_fn=S.squared_waypoint_loss([0], fused.wps), grad_scale=0.5)
    lf, gf = fused.evaluate(fused.theta)
    lc, gc = cust.evaluate(cust.theta)
    _, _, bl, bg = S.fused_reference(cust._sol["state_grid"], cust._aux["auxX_grid"], cust.hz, cust.taus, fused.wps, [0])
    eps = S.eps_of(F64)
    grp = lambda t: t.reshape((3, D) + tuple(t.shape[1:])).sum(dim=1)
    bound_l = grp(2 * bl * eps) + (D - 1) * eps * grp(fused.row_loss.abs())
    bound_g = grp(2 * bg * eps) + (D - 1) * eps * grp(fused.row_grad.abs())
    assert bool(((cust.row_loss - fused.row_loss).abs() <= 2 * bl * eps).all()) and bool(((cust.row_grad - fused.row_grad).abs() <= 2 * bg * eps).all())
    assert bool(((lc - lf).abs() <= bound_l).all()) and bool(((gc - gf).abs() <= bound_g).all())


def test_refusals_on_the_device():
    oc, d, args, D, make = _pendulum()
    for kw in (dict(stop_rule=dict(loss=0.9, grad_norm=0.05)), dict(process_group=object()),
               dict(method="Nesterov", true_loss_print_flag=[True, False, True]), dict(learning_rate=[0.1] * 9)):
        with pytest.raises(LfsdError):
            make(**kw)
    with pytest.raises(LfsdError):
        CPDP.SparseDemoLearner(oc, *args[:5], d["theta0"], mode="shared", demos_per_seed=3)
    L = make()
    for bad in (L.theta[:2], L.theta.repeat(3, 1), L.theta.float()):      # evaluate(): [G, p] or [1, p] only
        with pytest.raises(LfsdError):
            L.evaluate(bad)
    assert torch.equal(L.evaluate(L.theta[:1])[0], L.evaluate(L.theta[:1].expand(3, -1).contiguous())[0])


def test_grouped_lm_learns_the_ground_truth_on_the_device():
    def make_oc():
        oc, env, d = models.pendulum(n_grid=10)
        oc.setDevice(DEV, F64)
        return oc, d
    C.run_learns(make_oc)
