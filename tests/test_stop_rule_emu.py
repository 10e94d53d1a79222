"""CPU tier of the per-seed stop rule (csrc/cpdp_rows.h, SparseDemoLearner(stop_rule=...), QuadAlgorithm.run(stop="per_seed")):
the kernels through the SIMT emulator against a numpy restatement, and the learner against the reference's own loop
(lib/QuadAlgorithm.py:239-257) run seed by seed around a batch-of-one learner WITHOUT a rule."""
import ctypes

import numpy as np
import pytest
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models, runtime
from conftest import build_emu_library
import stop_rule_cases as C


@pytest.fixture(scope="module")
def lib():
    oc = models.pendulum(n_grid=10)[0]
    return runtime.ModelLibrary(build_emu_library(oc))


# ---- 1. kernel exactness --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given", [False, True], ids=["null", "rows_in+eligible"])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n_rows", C.ROW_COUNTS)
def test_stop_compact_matches_numpy(lib, n_rows, dt, given):
    C.run_stop_compact(lib, "cpu", dt, n_rows, given)


@pytest.mark.parametrize("n_rows", C.ROW_COUNTS)
def test_row_copies_are_bit_exact(lib, n_rows):
    # rows of 4, 28 (a parameter vector), 48 (16-byte accesses) and 800 bytes (a 50 x 4 fp32 control grid); 8-byte words; and a
    # 16-byte-multiple row on a base address that is not one
    for row_words in (1, 7, 12) + ((200,) if n_rows <= 1025 else ()):
        C.run_row_copies(lib, "cpu", n_rows, row_words)
    C.run_row_copies(lib, "cpu", n_rows, 12, misalign=True)
    C.run_row_copies(lib, "cpu", n_rows, 7, word=torch.int64)
    C.run_row_copies(lib, "cpu", n_rows, 2, word=torch.int64)


def test_bad_arguments_are_refused_before_any_launch(lib):
    L = lib.lib
    buf = (ctypes.c_double * 64)()
    d = ctypes.cast(buf, ctypes.c_void_p)
    d2 = ctypes.c_void_p(d.value + 256)
    off2 = ctypes.c_void_p(d.value + 2)
    ok = lambda **kw: [kw.get("dtype", 0), kw.get("n_rows", 4), kw.get("n_param", 3), kw.get("loss", d), kw.get("grad", d),
                       kw.get("rows_in", None), None, kw.get("loss_tol", 0.9), kw.get("grad_tol", 0.05), kw.get("iter_idx", 0),
                       kw.get("rows_out", d), kw.get("pos_out", d), kw.get("n_out", d), kw.get("active", d),
                       kw.get("stop_iter", d), None]
    for bad in (dict(dtype=7), dict(n_rows=0), dict(n_rows=-3), dict(n_param=0), dict(iter_idx=-1), dict(loss=None),
                dict(grad=None), dict(rows_out=None), dict(pos_out=None), dict(n_out=None), dict(active=None),
                dict(stop_iter=None), dict(loss_tol=float("nan")), dict(grad_tol=float("nan")), dict(rows_in=d, rows_out=d)):
        assert L.lfsd_stop_compact(*ok(**bad)) == -1, bad
    for fn in (L.lfsd_gather_rows, L.lfsd_scatter_rows):
        assert fn(0, 16, d, d, d2, None) == -1 and fn(4, 0, d, d, d2, None) == -1 and fn(4, 6, d, d, d2, None) == -1
        assert fn(4, 16, None, d, d2, None) == -1 and fn(4, 16, d, None, d2, None) == -1 and fn(4, 16, d, d, None, None) == -1
        assert fn(4, 16, d, off2, d2, None) == -1 and fn(4, 16, d, d, off2, None) == -1
    # ... and the binding refuses what it can see
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    with pytest.raises(runtime.LfsdError):
        lib.stop_compact(torch.zeros(4), torch.zeros(4, 3), 0.9, 0.05, 0, i32(3), i32(4), i32(1), i32(4), i32(4))
    with pytest.raises(runtime.LfsdError):
        lib.gather_rows(i32(4), torch.zeros(8, 3), torch.zeros(2, 3), 4)


# ---- 2. the learner against the reference's loop ------------------------------------------------------------------------
def _workload(emu, kind):
    """(oc, per-seed learner arguments, theta0 [B,p], K, learning rate).  Seeds and K are picked so that the conditions the test
    asserts on the yardstick hold (measured with the loop below before the feature existed)."""
    if kind == "pendulum":
        oc, env, d = models.pendulum(n_grid=10)
        B, K, lr = 8, 5, 0.05
        rng = np.random.RandomState(3)
        theta0 = np.array(d["theta0"], dtype=float)[None, :] * (1 + 0.5 * rng.uniform(-1, 1, (B, 3)))
        taus = np.tile([0.2, 0.5, 0.8], (B, 1))
        wps = np.tile(np.array([[0.4], [1.5], [2.6]]), (B, 1, 1))
    else:
        oc, env, d = models.quadrotor(n_grid=6)
        B, K, lr = 4, 3, 0.05
        rng = np.random.RandomState(1)
        theta0 = np.array(d["theta0"], dtype=float)[None, :] * (1 + 0.2 * rng.uniform(-1, 1, (B, 7)))
        taus = np.tile(d["taus"], (B, 1))
        # every seed its own demonstration (the reference's waypoints pulled towards the start): losses two decades apart
        p0, w = np.array(d["ini_state"][:3]), np.array(d["waypoints"])
        wps = p0[None, None, :] + np.array([0.05, 0.1, 0.2, 1.0])[:, None, None] * (w[None] - p0[None, None, :])
    emu(oc)
    oc.setDevice(dtype=torch.float64)
    x0 = np.tile(d["ini_state"], (B, 1))

    def make(rows, **kw):
        rows = list(rows)
        return CPDP.SparseDemoLearner(oc, x0[rows], d["horizon"], taus[rows], wps[rows], d["interface"], theta0[rows],
                                      method="Vanilla", learning_rate=lr, **kw)
    return make, B, K


def _trace(L, K):
    out = []
    for _ in range(K):
        l, g = L.step()
        out.append((l.cpu().numpy().copy(), g.cpu().numpy().copy(), L.theta.cpu().numpy().copy()))
    return out


@pytest.mark.parametrize("kind", ["pendulum", "quadrotor"])
def test_learner_follows_the_reference_loop_seed_by_seed(emu, oc_mapping, kind):
    make, B, K = _workload(emu, kind)
    # thresholds from a never-stopping run of K iterations (no rule: the code as it was)
    free = _trace(make(range(B)), K)
    loss_all = np.array([f[0] for f in free]).T                                 # [B, K]
    norm_all = np.array([np.linalg.norm(f[1], axis=1) for f in free]).T
    loss_tol, grad_tol = C.widest_gap(loss_all), C.widest_gap(norm_all)
    # yardstick: the reference's loop around a batch of one, seed by seed
    ref = [C.reference_loop(lambda b=b: make([b]), K, loss_tol, grad_tol) for b in range(B)]
    ref_stop = np.array([r[0] for r in ref])
    # slot noise: the same seed in the batch of B and alone, same code (no rule).  Measured over all K iterations before the
    # feature existed, fp64 on the emulator: 0.0 for the pendulum and the quadrotor on both mappings -> bit identity is required.
    noise = 0.0
    for b, (s, l, g, th) in enumerate(ref):
        for k in range(len(l)):
            noise = max(noise, abs(free[k][0][b] - l[k]), np.abs(free[k][1][b] - g[k]).max(), np.abs(free[k][2][b] - th[k + 1]).max())
    assert noise == 0.0, noise
    # conditions on the yardstick alone
    assert ((ref_stop > 0) & (ref_stop < K)).sum() * 4 >= B, ref_stop          # a quarter stops before iteration K
    assert (ref_stop == 0).sum() * 4 >= B, ref_stop                            # a quarter still runs at K
    # no tested value next to a threshold: 100 x the slot noise (zero), and the rounding of a norm formed in another order
    tested_l = np.concatenate([r[1] for r in ref])
    tested_n = np.concatenate([np.linalg.norm(r[2], axis=1) for r in ref])
    margin = max(100 * noise, 1e-12)
    assert (np.abs(tested_l / loss_tol - 1) > margin).all() and (np.abs(tested_n / grad_tol - 1) > margin).all()

    L = make(range(B), stop_rule=dict(loss=loss_tol, grad_norm=grad_tol))
    theta_prev = L.theta.clone()
    for k in range(K):
        act_before = L.active.clone()
        l, g = L.step()
        assert l.shape == (B,) and g.shape[0] == B
        for b in range(B):
            s, rl, rg, rth = ref[b]
            kk = min(k, len(rl) - 1)                     # a stopped seed keeps its last values
            assert l[b].item() == rl[kk] and np.array_equal(g[b].numpy(), rg[kk]), (kind, b, k)
            assert np.array_equal(L.theta[b].numpy(), rth[kk + 1]), (kind, b, k)
            if not act_before[b]:
                assert torch.equal(L.theta[b], theta_prev[b])      # a stopped seed's theta never changes again
        theta_prev = L.theta.clone()
        assert L.n_active == int(L.active.sum())
    assert np.array_equal(L.stop_iter.numpy(), ref_stop), (L.stop_iter, ref_stop)
    assert np.array_equal(L.active.numpy(), ref_stop == 0)


# ---- 3. further learner cases ---------------------------------------------------------------------------------------------
def _pendulum_args(emu, B=3):
    oc, env, d = models.pendulum(n_grid=10)
    emu(oc)
    oc.setDevice(dtype=torch.float64)
    th = np.array([[1.0, 0.5, 1.5], [2.0, 1.0, 1.0], [1.4, 0.8, 1.0], [0.7, 1.3, 0.6]])[:B]
    return oc, (np.tile(d["ini_state"], (B, 1)), 1.0, [0.2, 0.5, 0.8], [[0.4], [1.5], [2.6]], [0], th)


@pytest.mark.parametrize("method", ["Vanilla", "Nesterov", "Adam"])
def test_no_rule_is_todays_path(emu, method):
    oc, args = _pendulum_args(emu)
    a = CPDP.SparseDemoLearner(oc, *args, method=method, learning_rate=2e-2)
    b = CPDP.SparseDemoLearner(oc, *args, method=method, learning_rate=2e-2, stop_rule=None)
    for _ in range(3):
        la, ga = a.step()
        lb, gb = b.step()
        assert torch.equal(la, lb) and torch.equal(ga, gb) and torch.equal(a.theta, b.theta)
    assert b.n_active == 3 and bool(b.active.all()) and int(b.stop_iter.sum()) == 0


def test_shared_mode_refuses_a_rule(emu):
    oc, args = _pendulum_args(emu)
    with pytest.raises(runtime.LfsdError):
        CPDP.SparseDemoLearner(oc, *args[:-1], args[-1][:1], mode="shared", stop_rule=dict(loss=0.9, grad_norm=0.05))
    with pytest.raises(runtime.LfsdError):
        CPDP.SparseDemoLearner(oc, *args, stop_rule=dict(loss=0.9))


@pytest.mark.parametrize("method", ["Nesterov", "AMSGrad"])
def test_rule_with_optimizer_state_matches_seeds_alone(emu, method):
    """Momentum / moment state of a stopped seed is frozen with it and the others' is untouched by the compaction."""
    oc, args = _pendulum_args(emu, B=4)
    kw = dict(method=method, learning_rate=5e-2)
    K = 5
    free = _trace(CPDP.SparseDemoLearner(oc, *args, **kw), K)
    last = np.sort(np.array([f[0] for f in free]).min(axis=0))      # a threshold two seeds get below within K iterations
    loss_tol = float(np.sqrt(last[1] * last[2]))
    rule = dict(loss=loss_tol, grad_norm=1e-6)
    L = CPDP.SparseDemoLearner(oc, *args, stop_rule=rule, **kw)
    got = _trace(L, K)
    assert 0 < L.n_active < 4
    for b in range(4):
        one = CPDP.SparseDemoLearner(oc, args[0][b:b + 1], *args[1:5], args[5][b:b + 1], **kw)
        s, rl, rg, rth = C.reference_loop(lambda: one, K, loss_tol, 1e-6)
        assert int(L.stop_iter[b]) == s
        for k in range(K):
            kk = min(k, len(rl) - 1)
            assert got[k][0][b] == rl[kk] and np.array_equal(got[k][2][b], rth[kk + 1]), (b, k)


def test_frozen_row_is_not_stopped_and_continues_its_own_controls(emu):
    """skip_unconverged: a row frozen in a step has a zeroed gradient -- that is not a small gradient, the row stays in the set
    (`eligible`); and when the set shrinks, its unfinished solve is continued from ITS controls at its new position."""
    oc, args = _pendulum_args(emu, B=4)
    oc.setSolverOptions(max_iter=3)                       # every solve stops at the limit for the first steps
    try:
        rule = dict(loss=1e-3, grad_norm=1e-3)
        L = CPDP.SparseDemoLearner(oc, *args, learning_rate=0.1, skip_unconverged=True, stop_rule=rule)
        ref = CPDP.SparseDemoLearner(oc, *args, learning_rate=0.1, skip_unconverged=True)
        l, g = L.step(); ref.step()
        assert (L._sol["status"] == 3).all() and (g == 0).all()
        assert L.n_active == 4 and int(L.stop_iter.sum()) == 0          # zero gradients, yet nobody stopped
        # rows 0 and 2 leave (white box: the kernel is handed made-up losses for them), rows 1 and 3 move to positions 0 and 1
        L2 = CPDP.SparseDemoLearner(oc, *args, learning_rate=0.1, skip_unconverged=True, stop_rule=rule)
        L2.step()
        assert L2.n_active == 4
        L2._ok = None
        L2._apply_stop_rule(torch.tensor([0.0, 9.0, 0.0, 9.0], dtype=torch.float64), torch.ones(4, 3, dtype=torch.float64))
        assert L2.n_active == 2 and L2.stop_iter.tolist() == [1, 0, 1, 0]
        for _ in range(14):
            L2.step(); ref.step()
            # rows 1 and 3 of the shrunk learner walk exactly the path of rows 1 and 3 of the full one: continued from their
            # own controls (a cold start, or another row's controls, gives other iterates under a 3-iteration limit)
            assert torch.equal(L2.theta[[1, 3]], ref.theta[[1, 3]])
            assert torch.equal(L2._sol_active["status"], ref._sol["status"][[1, 3]])
            assert torch.equal(L2._sol_active["control_grid"], ref._sol["control_grid"][[1, 3]])
        assert not torch.equal(ref.theta[[1, 3]], torch.as_tensor(args[5][[1, 3]]))      # (and they did move: the solves finished)
    finally:
        oc.setSolverOptions(max_iter=300)


def test_all_stopped_launches_nothing(emu):
    oc, args = _pendulum_args(emu)
    L = CPDP.SparseDemoLearner(oc, *args, learning_rate=1e-2, stop_rule=dict(loss=1e9, grad_norm=0.0))
    l0, g0 = L.step()                                      # every loss is below 1e9: all stop after their first update
    assert L.n_active == 0 and L.stop_iter.tolist() == [1, 1, 1] and not bool(L.active.any())
    theta = L.theta.clone()
    called = []
    L.event_hook = called.append
    l1, g1 = L.step()
    assert called == [] and L.iter_idx == 1
    assert torch.equal(l1, l0) and torch.equal(g1, g0) and torch.equal(L.theta, theta)


def test_quadalgorithm_per_seed(emu):
    from lfsd_amd.QuadAlgorithm import QuadAlgorithm, QuadPara, DemoSparse
    from lfsd_amd.JinEnv import QuadStates
    cfg = {"QUAD_AVERAGE_SPEED": 1.0, "LAB_SPACE_LIMIT": {"LIMIT_X": [-3.2, 3.2], "LIMIT_Y": [-1.6, 1.6], "LIMIT_Z": [0.0, 2.2]}}
    ini, goal = QuadStates(position=[-2.0, -1.0, 0.6]), QuadStates(position=[2.5, 1.0, 1.5])
    lib_path = build_emu_library(models.quadrotor(n_grid=6)[0])

    def run(demo, theta0, **kw):
        S = QuadAlgorithm(cfg, QuadPara([1.0, 1.0, 1.0], 1.0, 1.0, 0.02), 6, dtype=torch.float64)
        S.library = lib_path
        S.load_optimization_function({"learning_rate": 0.01, "iter_num": 3, "method": "Vanilla"})
        return S.run(ini, goal, demo, ObsList=[], initial_parameters=theta0, **kw)
    # a demonstration next to what the second seed flies anyway: that seed meets the reference's test (loss <= 0.9) at once
    base = np.array([1, 0.1, 0.1, 0.1, 0.1, 0.1, -1], dtype=float)
    seeds = np.stack([base * 1.6, base])
    probe = run(DemoSparse(waypoints=[[0, 0, 0.6]], time_list=[0.5], time_horizon=1.0), base)
    t = np.array([0.25, 0.5, 0.75])
    way = np.array([np.interp(t * 100, np.arange(101), probe["opt_state_traj"][:, i]) for i in range(3)]).T + 0.05
    demo = DemoSparse(waypoints=way.tolist(), time_list=t.tolist(), time_horizon=1.0)
    res = run(demo, seeds, stop="per_seed")
    assert "stop_iter" not in run(demo, seeds[1]) and res["stop_iter"].shape == (2,)
    alone = [run(demo, seeds[b:b + 1]) for b in range(2)]
    for b in range(2):
        n = alone[b]["loss_trace"].shape[0]                # the seed alone ran until ITS test failed (or iter_num)
        assert res["stop_iter"][b] == (n if n < 3 else res["stop_iter"][b])
        assert np.array_equal(res["loss_trace"][:n, b], alone[b]["loss_trace"][:, 0])
        assert np.array_equal(res["parameter_trace"][:n + 1, b], alone[b]["parameter_trace"][:, 0])
        assert (res["parameter_trace"][n:, b] == res["parameter_trace"][n, b]).all()      # last entry repeated
    assert res["stop_iter"][1] == 1 and res["stop_iter"][0] in (0, 3)
    assert res["loss_trace"].shape[0] == 3 and res["parameter_trace"].shape[:2] == (4, 2)
