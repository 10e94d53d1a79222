"""CPU tier of the hyper-parameter sweeps in one batch (ABI 13): the three kernels through the SIMT emulator against the scalar entry
points, bit for bit; every LFSD_EINVAL case on host dummies; the sweep learner against uniform learners of the same batch, bit for
bit; QuadAlgorithm.run_comparison against run(stop="per_seed") configuration by configuration.  Cases: tests/hyper_sweep_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models, runtime
from lfsd_amd.runtime import LfsdError
from conftest import build_emu_library
import hyper_sweep_cases as H

F64 = torch.float64
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, F64], ids=["fp32", "fp64"])
SHAPES = pytest.mark.parametrize("shape", H.SHAPES_EMU, ids=lambda s: "B%dp%d" % s)


@pytest.fixture(scope="module")
def lib():
    return runtime.ModelLibrary(build_emu_library(models.pendulum(n_grid=10)[0]))


# ---- 1. kernels -----------------------------------------------------------------------------------------------------------------
@DTYPES
@SHAPES
def test_rows_step_is_the_scalar_step_per_row(lib, shape, dtype):
    B, p = shape
    for iter_idx in H.ITERS:
        for masked in (False, True):
            for offset in (range(10) if B == 1 and not masked else (0,)):      # a batch of one: every rule and both sets in turn
                H.run_rows_against_scalars(lib, "cpu", dtype, B, p, iter_idx, masked, offset)


@DTYPES
@SHAPES
def test_lookahead_rows_selects_on_the_method(lib, shape, dtype):
    for offset in (range(10) if shape[0] == 1 else (0,)):
        H.run_lookahead_rows(lib, "cpu", dtype, *shape, offset=offset)


@DTYPES
@SHAPES
def test_trace_append_files_one_iteration(lib, shape, dtype):
    for masked in (False, True):
        H.run_trace_append(lib, "cpu", dtype, *shape, masked=masked)


@pytest.mark.parametrize("which", ["emulator", "hip"])
def test_entry_points_refuse_bad_arguments_before_any_launch(lib, which):
    """Host dummies stand in for the arrays: no launch is reached (the gfx950 library loads without a GPU, as in tests/test_capi.py)."""
    ml = lib if which == "emulator" else models.pendulum(n_grid=10)[0].compile()
    L = ml.lib
    buf = (ctypes.c_double * 256)()
    d = ctypes.cast(buf, ctypes.c_void_p)
    at = lambda off: ctypes.c_void_p(d.value + off)
    step = lambda **kw: [kw.get("dtype", 1), kw.get("batch", 2), kw.get("n_param", 3), kw.get("iter_idx", 0), kw.get("method", d),
                         kw.get("hyper", d), kw.get("theta", d), kw.get("grad", d), kw.get("m", d), kw.get("v", d), kw.get("vhat", d),
                         None, None, None]
    for bad in (dict(dtype=7), dict(dtype=-1), dict(batch=0), dict(batch=-2), dict(n_param=0), dict(iter_idx=-1), dict(method=None),
                dict(hyper=None), dict(theta=None), dict(grad=None), dict(m=None), dict(v=None), dict(vhat=None)):
        assert L.lfsd_optimizer_step_rows(*step(**bad)) == -1, bad
    look = lambda **kw: [kw.get("dtype", 1), kw.get("batch", 2), kw.get("n_param", 3), kw.get("method", d), kw.get("hyper", d),
                         kw.get("theta", at(512)), kw.get("m", at(1024)), kw.get("out", at(1536)), None]
    for bad in (dict(dtype=7), dict(batch=0), dict(n_param=-1), dict(method=None), dict(hyper=None), dict(theta=None), dict(m=None),
                dict(out=None), dict(out=at(512)), dict(out=at(1024)), dict(out=at(512 + 40)), dict(out=at(1024 - 8))):
        assert L.lfsd_lookahead_rows(*look(**bad)) == -1, bad
    trace = lambda **kw: [kw.get("dtype", 1), kw.get("batch", 2), kw.get("n_param", 3), kw.get("iter_idx", 0), kw.get("capacity", 4),
                          kw.get("loss", d), kw.get("grad", d), kw.get("theta", d), None, kw.get("loss_trace", d),
                          kw.get("gnorm_trace", d), kw.get("theta_trace", d), None]
    for bad in (dict(dtype=7), dict(batch=0), dict(n_param=0), dict(capacity=0), dict(iter_idx=-1), dict(iter_idx=4), dict(iter_idx=9),
                dict(loss=None), dict(grad=None), dict(theta=None), dict(loss_trace=None, gnorm_trace=None, theta_trace=None)):
        assert L.lfsd_trace_append(*trace(**bad)) == -1, bad
    if which == "hip":
        return
    # ... and the binding refuses what it can see
    z = lambda *s: torch.zeros(s, dtype=F64)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    with pytest.raises(LfsdError):
        ml.optimizer_step_rows(i32(3), z(4, 5), z(4, 3), z(4, 3), 0, z(4, 3), z(4, 3), z(4, 3))           # method of another length
    with pytest.raises(LfsdError):
        ml.optimizer_step_rows(i32(4), z(4, 4), z(4, 3), z(4, 3), 0, z(4, 3), z(4, 3), z(4, 3))           # hyper is [B, 5]
    with pytest.raises(LfsdError):
        ml.optimizer_step_rows(i32(4), z(4, 5), z(4, 3), z(4, 3), 0, z(4, 3), z(4, 3), None)              # all state required
    with pytest.raises(LfsdError):
        ml.lookahead_rows(i32(4), z(4, 5).float(), z(4, 3), z(4, 3))                                      # hyper in theta's dtype
    with pytest.raises(LfsdError):
        ml.trace_append(0, z(4), z(4, 3), z(4, 3))                                                        # no trace at all
    with pytest.raises(LfsdError):
        ml.trace_append(2, z(4), z(4, 3), z(4, 3), loss_trace=z(4, 2))                                    # beyond the capacity
    with pytest.raises(LfsdError):
        ml.trace_append(0, z(4), z(4, 3), z(4, 3), loss_trace=z(4, 2), theta_trace=z(4, 2, 3))            # capacities disagree


def test_product_library_refuses_cpu_tensors():
    ml = models.pendulum(n_grid=10)[0].compile()
    z = lambda *s: torch.zeros(s, dtype=F64)
    i32 = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(LfsdError):
        ml.optimizer_step_rows(i32, z(4, 5), z(4, 3), z(4, 3), 0, z(4, 3), z(4, 3), z(4, 3))
    with pytest.raises(LfsdError):
        ml.lookahead_rows(i32, z(4, 5), z(4, 3), z(4, 3))
    with pytest.raises(LfsdError):
        ml.trace_append(0, z(4), z(4, 3), z(4, 3), loss_trace=z(4, 2))


# ---- 2. the learner ---------------------------------------------------------------------------------------------------------------
def _pendulum(emu, seeds, configs):
    """make(**learner kwargs) of len(configs) x seeds pendulum rows (n_grid 8, fp64): the same seeds under every configuration."""
    oc, env, d = models.pendulum(n_grid=8)
    emu(oc)
    oc.setDevice(dtype=F64)
    th = np.array([[1.0, 0.5, 1.5], [2.0, 1.0, 1.0], [1.4, 0.8, 1.0], [0.7, 1.3, 0.6]])[:seeds]
    B = len(configs) * seeds
    args = (np.tile(d["ini_state"], (B, 1)), 1.0, [0.2, 0.5, 0.8], [[0.4], [1.5], [2.6]], [0], np.tile(th, (len(configs), 1)))
    return oc, args, lambda **kw: CPDP.SparseDemoLearner(oc, *args, **kw)


def test_pendulum_sweep_is_nine_uniform_learners(emu):
    """18 rows: a partial wavefront of 8-lane groups."""
    oc, args, make = _pendulum(emu, 2, H.NINE_CONFIGS)
    sweep, _ = H.sweep_against_uniform(make, H.NINE_CONFIGS, seeds=2, steps=2)      # (steps cut for the CPU tier's time, not configurations)
    assert sweep._rows_path and sweep.theta.shape == (18, 3)


def test_quadrotor_sweep_is_five_uniform_learners(emu, monkeypatch):
    """The five method rows on the lock-step mapping of the 32-lane model."""
    monkeypatch.setattr(CPDP.COCSys, "mapping_override", "lockstep")
    oc, env, d = models.quadrotor(n_grid=10)
    emu(oc)
    oc.setDevice(dtype=F64)
    C = len(H.METHOD_CONFIGS)
    args = (np.tile(d["ini_state"], (C, 1)), d["horizon"], d["taus"], d["waypoints"], d["interface"], np.tile(d["theta0"], (C, 1)))
    make = lambda **kw: CPDP.SparseDemoLearner(oc, *args, **kw)
    H.sweep_against_uniform(make, H.METHOD_CONFIGS, seeds=1, steps=1)               # (steps cut for the CPU tier's time)


def test_scalar_arguments_take_todays_path(emu, monkeypatch):
    oc, args, make = _pendulum(emu, 2, H.METHOD_CONFIGS)
    ml = oc.compile()
    calls = {}

    def counting(name):
        fn = getattr(ml, name)

        def wrapped(*a, **kw):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **kw)
        monkeypatch.setattr(ml, name, wrapped)
    for name in ("optimizer_step_rows", "lookahead_rows", "trace_append", "optimizer_step", "lookahead"):
        counting(name)
    for cfg in H.METHOD_CONFIGS:
        calls.clear()
        a = make(**cfg)
        ra = H.run_learner(a, 2)
        assert not a._rows_path and a.loss_trace is None and a.theta_trace is None
        assert not {"optimizer_step_rows", "lookahead_rows", "trace_append"} & set(calls), calls
        assert calls["optimizer_step"] == 2 and calls.get("lookahead", 0) == (2 if cfg["method"] == "Nesterov" else 0)
        # uniform values given as arrays take the rows path and equal the scalar learner bit for bit
        calls.clear()
        B = a.B
        as_rows = dict(cfg, learning_rate=np.full(B, cfg["learning_rate"]))
        if "beta_1" in cfg:
            as_rows.update(beta_1=torch.full((B,), cfg["beta_1"], dtype=F64), epsilon=[cfg["epsilon"]] * B)
        b = make(**as_rows)
        rb = H.run_learner(b, 2)
        assert b._rows_path and calls["optimizer_step_rows"] == 2 and "optimizer_step" not in calls and "lookahead" not in calls
        assert calls.get("lookahead_rows", 0) == (2 if cfg["method"] == "Nesterov" else 0)      # skipped when no row is Nesterov
        for k in range(2):
            for x, y in zip(ra[k], rb[k]):
                assert torch.equal(x, y), (cfg, k)
    # a method list alone selects the rows path as well
    assert make(method=["Adam"] * a.B)._rows_path


def test_true_loss_flag_per_row(emu):
    """A flagged Nesterov row beside unflagged rows (Nesterov and others): the flagged learner's row; the others the unflagged one's."""
    oc, args, make = _pendulum(emu, 4, [dict()])
    nest = dict(method="Nesterov", learning_rate=0.01, mu=0.9)
    flagged = H.run_learner(make(true_loss_print_flag=True, **nest), 3)
    plain = H.run_learner(make(true_loss_print_flag=False, **nest), 3)
    adam = H.run_learner(make(method="Adam", learning_rate=0.22), 3)
    mixed = make(method=["Nesterov", "Nesterov", "Adam", "Nesterov"], learning_rate=[0.01, 0.01, 0.22, 0.01],
                 true_loss_print_flag=[True, False, True, True])      # (the flag of the Adam row acts on nothing)
    got = H.run_learner(mixed, 3)
    want = (flagged, plain, adam, flagged)
    for k in range(3):
        for r in range(4):
            for x, y in zip(got[k], want[r][k]):
                assert torch.equal(x[r], y[r]), (k, r)
    assert not torch.equal(flagged[0][0], plain[0][0])      # (the two evaluations do differ)


def test_sweep_with_stop_rule(emu):
    configs = H.NINE_CONFIGS
    S, K = 2, 3
    oc, args, make = _pendulum(emu, S, configs)
    B = len(configs) * S
    free = H.run_learner(make(**H.per_row_kwargs(configs, S)), K)
    # a loss threshold rows get below before the last step, and not all: the middle of the widest gap of the rule-free minima
    low = np.sort(torch.stack([f[0] for f in free[:K - 1]]).min(dim=0).values.numpy())
    i = 2 + int(np.argmax(low[3:-1] / low[2:-2]))
    rule = dict(loss=float(np.sqrt(low[i] * low[i + 1])), grad_norm=1e-12)
    assert low[i] < rule["loss"] < low[i + 1]
    sweep = make(trace=K, stop_rule=rule, **H.per_row_kwargs(configs, S))
    got = H.run_learner(sweep, K)
    stop = sweep.stop_iter.numpy()
    early = (stop > 0) & (stop < K)
    assert early.sum() >= 2 and not early.all(), stop
    for i, cfg in enumerate(configs):
        uni = make(trace=K, stop_rule=rule, **cfg)
        ref = H.run_learner(uni, K)
        rows = slice(i * S, (i + 1) * S)
        assert np.array_equal(stop[rows], uni.stop_iter.numpy()[rows]), cfg
        for k in range(K):
            for x, y in zip(got[k], ref[k]):
                assert H.same(x[rows], y[rows]), (cfg, k)
        for name in ("loss_trace", "grad_norm_trace", "theta_trace"):
            assert H.same(getattr(sweep, name)[rows], getattr(uni, name)[rows]), (cfg, name)
    # traces: filled up to stop_iter, NaN after it -- a seed is traced in the step in which it stops and never after
    for b in range(B):
        n = int(stop[b]) or K
        assert bool(torch.isfinite(sweep.loss_trace[b, :n]).all()) and bool(torch.isnan(sweep.loss_trace[b, n:]).all())
        assert bool(torch.isfinite(sweep.grad_norm_trace[b, :n]).all()) and bool(torch.isnan(sweep.grad_norm_trace[b, n:]).all())
        assert bool(torch.isfinite(sweep.theta_trace[b, :n + 1]).all()) and bool(torch.isnan(sweep.theta_trace[b, n + 1:]).all())
        assert torch.equal(sweep.theta_trace[b, n], sweep.theta[b])
        for k in range(n):
            assert sweep.loss_trace[b, k] == got[k][0][b]
    assert sweep.n_active == int((stop == 0).sum())


def test_sweep_with_loss_fn(emu):
    """The squared distance with grad_scale 0.5 is the fused loss: theta after 3 steps within 1e-8 relative (tests/test_sample_emu.py's
    bound for this pair: roundings of 1e-16 per step, not amplified by 1e8 in three steps)."""
    configs = H.METHOD_CONFIGS
    oc, args, make = _pendulum(emu, 2, configs)
    rows = H.per_row_kwargs(configs, 2)
    fused = make(**rows)
    cust = CPDP.SparseDemoLearner(oc, *args[:3], None, None, args[5], loss_fn=H.squared_waypoint_loss([0], fused.wps), grad_scale=0.5,
                                  trace=3, **rows)
    for _ in range(3):
        fused.step(); cust.step()
    rel = float(((cust.theta - fused.theta).abs() / fused.theta.abs().amax(dim=1, keepdim=True)).max())
    print("sweep with loss_fn: max relative theta difference after 3 steps %.3e" % rel)
    assert rel <= 1e-8
    assert not torch.equal(fused.theta, torch.as_tensor(args[5])) and bool(torch.isfinite(cust.loss_trace).all())


def test_sweep_with_warm_start_level_2_and_skip_unconverged(emu):
    """The rows path under the other options: still the uniform learners' rows."""
    oc, args, make = _pendulum(emu, 2, H.METHOD_CONFIGS)
    H.sweep_against_uniform(make, H.METHOD_CONFIGS, seeds=2, steps=2, distinct=False, warm_start=True, interplation_level=2,
                            skip_unconverged=True)


def test_second_evaluation_leaves_unflagged_rows_alone(emu):
    """A flagged Nesterov row makes the sweep evaluate the whole batch a second time.  Rows of other rules must not notice: with
    skip_unconverged and a stop rule, a row whose capped solve froze it in the first evaluation and that converges in the second
    has a ZEROED gradient, not a small one -- it must not stop; and its next solve continues the FIRST solve's controls, as in its
    uniform learner.  Every solve is capped at 10 iterations, of the 12 to 19 a cold pendulum solve takes: rows are frozen in the
    first step (asserted) and would converge in a second evaluation that continued them."""
    oc, args, make = _pendulum(emu, 2, H.METHOD_CONFIGS)
    oc.setSolverOptions(max_iter=10)
    try:
        kw = dict(skip_unconverged=True, stop_rule=dict(loss=1e-3, grad_norm=1e-3))
        probe = make(**H.per_row_kwargs(H.METHOD_CONFIGS, 2), **kw)
        probe.step()
        assert probe.n_unconverged > 0 and probe.n_active == probe.B          # frozen rows, and none of them stopped
        sweep, got = H.sweep_against_uniform(make, H.METHOD_CONFIGS, seeds=2, steps=5, distinct=False, **kw)
        assert not torch.equal(sweep.theta, torch.as_tensor(args[5]))           # (the solves did finish and the rows moved)
    finally:
        oc.setSolverOptions(max_iter=300)
    # warm starts: an unflagged row starts its next solve from its own first-evaluation controls
    H.sweep_against_uniform(make, H.METHOD_CONFIGS, seeds=2, steps=4, warm_start=True)


def test_method_of_another_type_is_the_reference_exception(emu):
    oc, args, make = _pendulum(emu, 1, [dict()])
    for bad in (None, 5, ["Adam", None], "SGD"):
        with pytest.raises(Exception, match="Wrong optimization method type!"):
            make(method=bad)


def test_refusals(emu):
    oc, args, make = _pendulum(emu, 2, H.METHOD_CONFIGS[:2])      # four rows
    for kw in (dict(learning_rate=[0.01] * 4), dict(method=["Adam"] * 4), dict(true_loss_print_flag=[True] * 4)):
        with pytest.raises(LfsdError):                             # per-row arguments in shared mode: there is one theta
            CPDP.SparseDemoLearner(oc, *args[:5], args[5][:1], mode="shared", **kw)
    for kw in (dict(learning_rate=[0.01] * 3), dict(method=["Adam"] * 5), dict(mu=np.full(2, 0.9)), dict(epsilon=torch.ones(7)),
               dict(true_loss_print_flag=[True])):
        with pytest.raises(LfsdError):
            make(**kw)
    with pytest.raises(Exception, match="Wrong optimization method type!"):
        make(method=["Adam", "Adam", "SGD", "Adam"])
    for bad in (0, -3, 2.5, True):
        with pytest.raises(LfsdError):
            make(trace=bad)
    L = make(trace=2, learning_rate=[0.01, 0.02, 0.03, 0.04])
    L.step(); L.step()
    theta = L.theta.clone()
    with pytest.raises(LfsdError):                                 # a step beyond the capacity
        L.step()
    assert torch.equal(L.theta, theta) and L.iter_idx == 2


def test_trace_in_shared_mode(emu):
    oc, args, make = _pendulum(emu, 3, [dict()])
    L = CPDP.SparseDemoLearner(oc, *args[:5], args[5][:1], mode="shared", learning_rate=1e-3, trace=2)
    assert L.loss_trace.shape == (1, 2) and L.theta_trace.shape == (1, 3, 3) and torch.equal(L.theta_trace[:, 0], L.theta)
    for k in range(2):
        l, g = L.step()
        assert torch.equal(L.loss_trace[:, k], l) and torch.equal(L.theta_trace[:, k + 1], L.theta)
        ref = float(torch.linalg.norm(g))
        assert abs(float(L.grad_norm_trace[0, k]) - ref) <= 5 * 2.3e-16 * ref


# ---- 3. the driver ----------------------------------------------------------------------------------------------------------------
def test_run_comparison_is_the_scripts_runs_in_one_batch(emu):
    lib_path = build_emu_library(models.quadrotor(n_grid=10)[0])
    new, ini, goal, demo = H.quad_driver(10, F64, library=lib_path)
    res = H.run_comparison_case(new, ini, goal, demo, iter_num=2)
    assert all(len(t) >= 1 for t in res["loss_trace_comparison"])
