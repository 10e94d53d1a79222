"""GPU tier of waypoint weights and ragged demonstrations (ABI 16): the weighted forward sweeps and lfsd_normal_matrix_weighted of the
gfx950 library at the cases of tests/weight_cases.py -- NULL and all-ones weights, zero weights, powers of two, bit for bit; general
weights against the fp64 restatement; the quadrotor fp32 learner (12 rows, n_grid 10) with ragged rows against learners on the compacted
lists, in grouped mode against its launches made by hand, with a stop rule, in shared mode and at interpolation level 2; the launches of
a learner without weights; the entry points' refusals.  The same cases pass on the SIMT emulator (tests/test_weights_emu.py)."""
import numpy as np
import pytest
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP
from lfsd_amd.runtime import LfsdError
import weight_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64


def prepare(oc, dtype):
    oc.setDevice(DEV, dtype)


@pytest.mark.parametrize("case", C.KERNEL_CASES, ids=C.CASE_ID)
def test_null_ones_zero_and_power_of_two_weights_are_exact_on_the_device(case):
    C.run_kernel_case(prepare, DEV, case)


@pytest.mark.parametrize("case", C.KERNEL_CASES, ids=C.CASE_ID)
def test_general_weights_against_fp64_restatement_on_the_device(case):
    fl, fg, fh = C.run_general_weights(prepare, DEV, case)
    print("%s: |loss - ref| / bound %.3f, |grad - ref| / bound %.3f, |H - ref| / bound %s" % (C.CASE_ID(case), fl, fg, fh))
    assert fl <= 1.0 and fg <= 1.0 and (fh is None or fh <= 1.0), (fl, fg, fh)


ROWS = 12


def _quadrotor(rows=ROWS):
    oc, args, lam0 = C.learner_problem(prepare, "quadrotor", rows, F32)

    def make(rows=None, k=None, **kw):
        sel = list(range(len(args[0]))) if rows is None else rows
        taus, wps = (args[2], args[3]) if k is None else (args[2][:k], args[3][:k])
        return CPDP.SparseDemoLearner(oc, args[0][sel], args[1], taus, wps, args[4], args[5][sel], **kw)
    return oc, args, lam0, make


@pytest.mark.parametrize("rule", C.RULES, ids=[r[0] for r in C.RULES])
def test_ragged_rows_walk_the_path_of_their_own_learners_on_the_device(rule):
    oc, args, lam0, make = _quadrotor()
    C.run_ragged_independent(make, ROWS, rule, lam0)


def test_grouped_learner_with_padded_demonstrations_is_its_launches_on_the_device():
    oc, args, lam0, make = _quadrotor(rows=2)
    G, D = 2, 3
    taus, wps, wts = CPDP.pad_demonstrations(*C.ragged_lists(args))
    x0 = np.tile(args[0][:1], (D, 1))
    x0[:, :3] += np.array([[0.0, 0.0, 0.0], [0.2, 0.0, -0.1], [-0.1, 0.1, 0.0]])
    gargs = (x0, args[1], taus, wps, args[4], args[5])
    L = CPDP.SparseDemoLearner(oc, *gargs, method="Vanilla", learning_rate=1e-2, mode="grouped", demos_per_seed=D, waypoint_weights=wts)
    hand = C.grouped_by_hand(oc, gargs, G, D, wts, C.STEPS, L.proj_lo, 1e-2)
    th0 = L.theta.clone()
    for k in range(C.STEPS):
        loss, grad = L.step()
        th, lg, gg, n_ok = next(hand)
        assert torch.equal(L.theta, th) and torch.equal(loss, lg) and torch.equal(grad, gg) and torch.equal(L.n_ok, n_ok), k
    assert bool((L.theta != th0).any()) and int(L.n_ok.sum()) > 0


def test_stop_rule_gathers_the_weights_with_the_rows_on_the_device():
    oc, args, lam0, make = _quadrotor()
    counts = [C.COUNTS[b % 3] for b in range(ROWS)]
    kw = dict(method="Vanilla", learning_rate=1e-2, n_waypoints=counts, trace=C.STEPS)
    free = make(**kw)
    for _ in range(C.STEPS):
        free.step()
    l2 = free.loss_trace[:, 1]
    tol = float(l2.sort().values[ROWS // 2 - 1: ROWS // 2 + 1].mean())
    stop = make(stop_rule=dict(loss=tol, grad_norm=0.0), **kw)
    for _ in range(C.STEPS):
        stop.step()
    it = stop.stop_iter.tolist()
    first = min([i for i in it if i > 0] + [C.STEPS])
    assert first < C.STEPS and any(i == 0 or i > first for i in it), it
    assert stop._dense is not None and "wts" in stop._dense
    for b in range(ROWS):
        n = it[b] if it[b] > 0 else C.STEPS
        assert torch.equal(stop.loss_trace[b, :n], free.loss_trace[b, :n]) and torch.equal(stop.theta_trace[b, :n + 1], free.theta_trace[b, :n + 1]), b


def test_shared_mode_and_level_2_take_the_weights_on_the_device():
    oc, args, lam0, make = _quadrotor(rows=4)
    counts = [5, 3, 1, 3]
    L = CPDP.SparseDemoLearner(oc, args[0], args[1], args[2], args[3], args[4], args[5][:1], method="Vanilla", learning_rate=1e-2,
                               mode="shared", n_waypoints=counts)
    th0 = L.theta.clone()
    loss, grad = L.step()
    sol = oc.cocSolverBatch(args[0], args[1], th0.expand(4, -1).contiguous())
    aux = oc.auxSysSolverBatch(sol, args[2], args[3], args[4], waypoint_weights=L.wts, skip_status=(3, 4))
    assert bool(L._ok.all())
    assert torch.equal(loss, aux["loss"].sum().reshape(1)) and torch.equal(grad, aux["grad"].sum(dim=0, keepdim=True))
    L2 = make(method="Vanilla", learning_rate=1e-2, n_waypoints=counts, interplation_level=2)
    th0 = L2.theta.clone()
    loss, grad = L2.step()
    sol = oc.cocSolverBatch(args[0], args[1], th0)
    aux = oc.auxSysSolverBatch(sol, args[2], args[3], args[4], waypoint_weights=L2.wts, interplation_level=2)
    assert torch.equal(loss, aux["loss"]) and torch.equal(grad, aux["grad"])
    S = make(rows=[1], k=3, method="Vanilla", learning_rate=1e-2, interplation_level=2)
    l3, g3 = S.step()
    assert torch.equal(l3, loss[1:2]) and torch.equal(g3, grad[1:2]) and torch.equal(S.theta, L2.theta[1:2])


def test_without_weights_the_learner_takes_the_launches_it_took_on_the_device(monkeypatch):
    oc, args, lam0, make = _quadrotor(rows=2)
    calls = C.launch_spy(oc.compile(), monkeypatch)
    for name, kw in C.RULES:
        L = make(**kw)
        L.step(); L.step()
        want = {"aux_solve": 2, "normal_matrix": 2, "lm_step": 2} if name == "LM" else {"aux_solve": 2, "optimizer_step": 2}
        assert calls == want, (name, calls)
        calls.clear()


def test_entry_points_refuse_bad_arguments_before_any_launch_on_the_device():
    oc, d, iface = C.make_model("pendulum", 10)
    ml = oc.compile()
    C.weighted_einval(ml.lib, ml.n_state, ml.n_control, ml.n_auxvar, compiled_iface=False)
    z = lambda *s: torch.zeros(s, dtype=F64)
    with pytest.raises(LfsdError):                              # no CPU fallback: host memory is refused by the binding
        ml.normal_matrix(z(2), z(2, 3), z(2, 4, 3, 2), torch.zeros(1, dtype=torch.int32), wp_weight=z(2, 3))
