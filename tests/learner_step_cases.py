"""What one SparseDemoLearner.step() does in terms of calls, shared by the CPU tier (tests/test_learner_steps_emu.py, the SIMT
emulator) and the -m gpu tier (tests/test_learner_steps_gpu.py).

The numeric tests compare the learner with launches made by hand; none states which calls a step makes.  Here every public method of
the ModelLibrary the learner holds is wrapped, so that each call is logged as one line: the method's name and, per argument, shape
and dtype of a tensor, ``None``, or the value of a scalar or string (dicts and tuples of those element by element; a callable as
``<fn>``).  Three steps of every configuration in CASES must give, step by step, the lines of EXPECTED and the event_hook names of
EXPECTED_HOOKS, and the solver's state grid, the sweeps' loss and the workspace must sit at the same addresses after steps 2 and 3
(the buffers are reused, nothing is allocated per step).  An extra launch, a lost ``out=`` or a reordered hook fails here while
every numeric test still passes.

The lines are written for the learner's float dtype ``F`` (fp64 on the emulator, fp32 on the device): a step makes the same calls in
either.  The workspace's size is a function of dtype and mapping and is logged as ``workspace``; a stop rule's thresholds come from
a run without the rule (as in tests/test_stop_rule_emu.py) and are logged as ``<loss_tol>`` / ``<grad_tol>``.

Shapes: B = 4 rows -- with a stop rule 4, then fewer, then 0 seeds are still learning; grouped mode has G = 2 groups of D = 2
demonstrations.  Pendulum n_grid = 10 (both tiers), quadrotor n_grid = 6 (32-lane groups, the other lock-step packing; device only)."""
import re

import numpy as np
import torch

from lfsd_amd import CPDP, models

STEPS = 3
B = 4
_DT = {torch.float32: "f32", torch.float64: "f64", torch.int32: "i32", torch.int64: "i64", torch.bool: "b"}


# ---- the log --------------------------------------------------------------------------------------------------------------------
def describe(x, name=None):
    if isinstance(x, np.generic):
        x = x.item()
    if isinstance(x, torch.Tensor):
        return "workspace" if name == "workspace" else "%s[%s]" % (_DT[x.dtype], ",".join(str(s) for s in x.shape))
    if isinstance(x, dict):
        return "{%s}" % ", ".join("%s: %s" % (k, describe(v, k)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return "(%s)" % ", ".join(describe(v) for v in x)
    if isinstance(x, torch.dtype):
        return _DT[x]
    if x is None or isinstance(x, (bool, int, float, str)):
        return repr(x)
    if callable(x):
        return "<fn>"
    raise TypeError("argument of a kind the log does not describe: %r" % (x,))


class Recorder:
    """Wraps the public methods of `lib` (on the instance: calls the library makes to itself are logged too) until close()."""

    def __init__(self, lib, dtype, symbols=()):
        self.lib, self.calls = lib, []
        self._float = re.compile(r"\b%s\b" % _DT[dtype])
        self._symbols = [(repr(float(v)), s) for v, s in symbols]
        self._names = [nm for nm in dir(type(lib)) if not nm.startswith("_") and callable(getattr(type(lib), nm))]
        for nm in self._names:
            setattr(lib, nm, self._wrap(nm, getattr(lib, nm)))

    def _wrap(self, nm, fn):
        def logged(*args, **kw):
            line = "%s(%s)" % (nm, ", ".join([describe(a) for a in args] + ["%s=%s" % (k, describe(v, k)) for k, v in kw.items()]))
            for value, symbol in self._symbols:
                line = line.replace(value, symbol)
            self.calls.append(self._float.sub("F", line))
            return fn(*args, **kw)
        return logged

    def close(self):
        for nm in self._names:
            delattr(self.lib, nm)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def make_model(kind, bind, device, dtype):
    """(oc, inputs): the model bound by `bind(oc)` (the emulator's library, or nothing on the device) and the B = 4 rows."""
    if kind == "pendulum":
        oc, env, d = models.pendulum(n_grid=10)
        theta0 = np.array([[1.0, 0.5, 1.5], [2.0, 1.0, 1.0], [1.4, 0.8, 1.0], [0.7, 1.3, 0.6]])
        taus = np.array([0.2, 0.5, 0.8])
        wps = np.tile(np.array([[0.4], [1.5], [2.6]]), (B, 1, 1))
        x0 = np.tile(d["ini_state"], (B, 1))
        x0[1::2, 0] += 0.3                                # (grouped mode: the second demonstration starts elsewhere)
    else:
        oc, env, d = models.quadrotor(n_grid=6)
        rng = np.random.RandomState(1)
        theta0 = np.array(d["theta0"], dtype=float)[None, :] * (1 + 0.2 * rng.uniform(-1, 1, (B, 7)))
        taus = np.array(d["taus"])
        # every row its own demonstration (the reference's waypoints pulled towards the start): losses two decades apart
        p0, w = np.array(d["ini_state"][:3]), np.array(d["waypoints"])
        wps = p0[None, None, :] + np.array([0.05, 0.1, 0.2, 1.0])[:, None, None] * (w[None] - p0[None, None, :])
        x0 = np.tile(d["ini_state"], (B, 1))
    bind(oc)
    oc.setDevice(device, dtype)
    return oc, dict(x0=x0, hz=d["horizon"], taus=taus, wps=wps, iface=d["interface"], theta0=theta0)


def _smooth_loss(x_tau, u_tau):
    return ((x_tau[:, :, :1] - 1.0) ** 2).sum((1, 2)) + 0.1 * (u_tau ** 2).sum((1, 2))


LR = dict(learning_rate=5e-2)
ROWS = dict(method=["Vanilla", "Nesterov", "Adam", "Vanilla"], true_loss_print_flag=[False, True, False, False], **LR)
GROUPED = dict(mode="grouped", demos_per_seed=2)
# name -> (learner arguments, stop rule: None, "shrinks" (thresholds from a run without the rule) or "all" (every seed stops at once))
CASES = {
    "vanilla": (dict(method="Vanilla", **LR), None),
    "nesterov_true_loss": (dict(method="Nesterov", true_loss_print_flag=True, **LR), None),
    "adam_warm": (dict(method="Adam", warm_start=True, **LR), None),
    "skip_unconverged_max_iter_3": (dict(method="Vanilla", skip_unconverged=True, **LR), None),
    "stop_rule": (dict(method="Vanilla", **LR), "shrinks"),
    "stop_rule_warm": (dict(method="Vanilla", warm_start=True, **LR), "shrinks"),
    "stop_rule_all_stop": (dict(method="Vanilla", **LR), "all"),
    "rows_flagged": (ROWS, None),
    "rows_flagged_stop_rule": (ROWS, "shrinks"),
    "shared_vanilla": (dict(mode="shared", method="Vanilla", **LR), None),
    "shared_nesterov_true_loss": (dict(mode="shared", method="Nesterov", true_loss_print_flag=True, **LR), None),
    "grouped_vanilla": (dict(GROUPED, method="Vanilla", **LR), None),
    "grouped_rules_flagged": (dict(GROUPED, method=["Nesterov", "Adam"], true_loss_print_flag=True, **LR), None),
    "grouped_lm": (dict(GROUPED, method="LM"), None),
    "lm": (dict(method="LM"), None),
    "lm_stop_rule": (dict(method="LM", lm_lambda0=30.0), "shrinks"),
    "learn_taus_nesterov": (dict(method="Vanilla", learn_taus=True, tau_method="Nesterov", tau_learning_rate=1e-3, **LR), None),
    "grouped_learn_taus_nesterov": (dict(GROUPED, method="Vanilla", learn_taus=True, tau_method="Nesterov", tau_learning_rate=1e-3,
                                         **LR), None),
    "lm_taus": (dict(method="LM", lm_taus=True), None),
    "loss_fn_level_2": (dict(method="Vanilla", loss_fn=_smooth_loss, interplation_level=2, **LR), None),
    "weights_trace": (dict(method="Vanilla", waypoint_weights=[1.0, 0.5, 2.0], trace=STEPS, **LR), None),
}


def make_learner(oc, inp, kw, **more):
    kw = dict(kw, **more)
    theta0 = inp["theta0"][:{"shared": 1, "grouped": 2}.get(kw.get("mode"), B)]
    wts = kw.pop("waypoint_weights", None)
    if wts is not None:                                   # (one weight per waypoint of the model, cycled)
        kw["waypoint_weights"] = [wts[k % len(wts)] for k in range(len(inp["taus"]))]
    return CPDP.SparseDemoLearner(oc, inp["x0"], inp["hz"], inp["taus"], inp["wps"], inp["iface"], theta0, **kw)


def shrinking_rule(oc, inp, kw):
    """A loss threshold two of the four seeds get below within the first two steps of a run without the rule (the geometric middle
    of the gap, as test_rule_with_optimizer_state_matches_seeds_alone picks it): the third step runs on a set that has shrunk."""
    free = make_learner(oc, inp, kw)
    lowest = np.sort(np.array([free.step()[0].double().cpu().numpy().copy() for _ in range(STEPS - 1)]).min(axis=0))
    assert 0 < lowest[1] < lowest[2], lowest
    return dict(loss=float(np.sqrt(lowest[1] * lowest[2])), grad_norm=1e-6)


def run_steps(oc, inp, name, on_step=None, steps=STEPS):
    """Three steps of case `name` with the library's calls logged.  Returns (calls per step, hook names per step, addresses of the
    reused buffers per step, n_active per step).  `on_step(L, k, loss, grad)`: called after each step (the bit-identity driver)."""
    kw, stop = CASES[name]
    max_iter = oc.max_iter
    if name == "skip_unconverged_max_iter_3":
        oc.setSolverOptions(max_iter=3)                   # every solve stops at the limit: status 3, continued at the next step
    rec = None
    try:
        rule = {None: None, "all": dict(loss=1e9, grad_norm=0.0)}[stop] if stop != "shrinks" else shrinking_rule(oc, inp, kw)
        L = make_learner(oc, inp, kw, **({} if rule is None else dict(stop_rule=rule)))
        symbols = () if stop != "shrinks" else ((rule["loss"], "<loss_tol>"), (rule["grad_norm"], "<grad_tol>"))
        rec = Recorder(L.lib, L.theta.dtype, symbols)
        hooks = []
        L.event_hook = hooks.append
        calls, names, where, active = [], [], [], []
        for k in range(steps):
            n_calls, n_hooks = len(rec.calls), len(hooks)
            loss, grad = L.step()
            calls.append(rec.calls[n_calls:])
            names.append(hooks[n_hooks:])
            ptr = lambda t: None if t is None else t.data_ptr()
            where.append((ptr(L._sol["state_grid"]), ptr(L._aux["loss"]), ptr(L._ws)))
            active.append(L.n_active)
            if on_step is not None:
                on_step(L, k, loss, grad)
        return calls, names, where, active
    finally:
        if rec is not None:
            rec.close()
        oc.setSolverOptions(max_iter=max_iter)


def run_case(kind, oc, inp, name):
    calls, names, where, active = run_steps(oc, inp, name)
    stop = CASES[name][1]
    if stop == "shrinks":                                 # the third step runs on 0 < n_active < B rows
        assert 0 < active[1] < B, active
    if stop == "all":
        assert active == [0, 0, 0]
    for k in range(STEPS):
        assert calls[k] == EXPECTED[kind][name][k], "step %d of %s:\n%s" % (k + 1, name, "\n".join(calls[k]))
        assert names[k] == EXPECTED_HOOKS[kind][name][k], (name, k + 1, names[k])
    assert where[1] == where[2] and where[1][0] is not None and where[1][2] is not None, where


# ---- the pinned lists (recorded from the learner before its step() was unified) --------------------------------------------
# (kind -> case -> per step, the lines of the log / the event_hook names)
EXPECTED_HOOKS = {
    'pendulum': {
        'vanilla': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
        ],
        'nesterov_true_loss': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
        ],
        'adam_warm': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
        ],
        'skip_unconverged_max_iter_3': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
        ],
        'stop_rule': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
        ],
        'stop_rule_warm': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
        ],
        'stop_rule_all_stop': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            [],
            [],
        ],
        'rows_flagged': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
        ],
        'rows_flagged_stop_rule': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
        ],
        'shared_vanilla': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
        ],
        'shared_nesterov_true_loss': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
        ],
        'grouped_vanilla': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce', 'update', 'end'],
        ],
        'grouped_rules_flagged': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce'],
        ],
        'grouped_lm': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'group_reduce', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'group_reduce', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'group_reduce', 'update', 'end'],
        ],
        'lm': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'update', 'end'],
        ],
        'lm_stop_rule': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'update', 'end'],
        ],
        'learn_taus_nesterov': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'tau_grad', 'update', 'tau_update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'tau_grad', 'update', 'tau_update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'tau_grad', 'update', 'tau_update', 'end'],
        ],
        'grouped_learn_taus_nesterov': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce', 'tau_grad', 'update', 'tau_update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce', 'tau_grad', 'update', 'tau_update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce', 'tau_grad', 'update', 'tau_update', 'end'],
        ],
        'lm_taus': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'tau_grad', 'time_blocks', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'tau_grad', 'time_blocks', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'tau_grad', 'time_blocks', 'update', 'end'],
        ],
        'loss_fn_level_2': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'loss_fn', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'loss_fn', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'loss_fn', 'update', 'end'],
        ],
        'weights_trace': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
        ],
    },
    'quadrotor': {
        'vanilla': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
        ],
        'nesterov_true_loss': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
        ],
        'adam_warm': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
        ],
        'skip_unconverged_max_iter_3': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
        ],
        'stop_rule': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
        ],
        'stop_rule_warm': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
        ],
        'stop_rule_all_stop': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            [],
            [],
        ],
        'rows_flagged': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
        ],
        'rows_flagged_stop_rule': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
        ],
        'shared_vanilla': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
        ],
        'shared_nesterov_true_loss': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward'],
        ],
        'grouped_vanilla': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce', 'update', 'end'],
        ],
        'grouped_rules_flagged': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce', 'update', 'end', 'oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce'],
        ],
        'grouped_lm': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'group_reduce', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'group_reduce', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'group_reduce', 'update', 'end'],
        ],
        'lm': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'update', 'end'],
        ],
        'lm_stop_rule': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'update', 'end'],
        ],
        'learn_taus_nesterov': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'tau_grad', 'update', 'tau_update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'tau_grad', 'update', 'tau_update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'tau_grad', 'update', 'tau_update', 'end'],
        ],
        'grouped_learn_taus_nesterov': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce', 'tau_grad', 'update', 'tau_update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce', 'tau_grad', 'update', 'tau_update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'group_reduce', 'tau_grad', 'update', 'tau_update', 'end'],
        ],
        'lm_taus': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'tau_grad', 'time_blocks', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'tau_grad', 'time_blocks', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'normal_matrix', 'tau_grad', 'time_blocks', 'update', 'end'],
        ],
        'loss_fn_level_2': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'loss_fn', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'loss_fn', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'loss_fn', 'update', 'end'],
        ],
        'weights_trace': [
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
            ['oc_solve', 'aux_riccati', 'aux_forward', 'update', 'end'],
        ],
    },
}

EXPECTED = {
    'pendulum': {
        'vanilla': [
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
            ],
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
            ],
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
            ],
        ],
        'nesterov_true_loss': [
            [
                'lookahead(F[4,3], F[4,3], 0.9)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Nesterov', F[4,3], F[4,3], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
            ],
            [
                'lookahead(F[4,3], F[4,3], 0.9)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Nesterov', F[4,3], F[4,3], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
            ],
            [
                'lookahead(F[4,3], F[4,3], 0.9)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Nesterov', F[4,3], F[4,3], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
            ],
        ],
        'adam_warm': [
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Adam', F[4,3], F[4,3], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
            ],
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Adam', F[4,3], F[4,3], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
            ],
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Adam', F[4,3], F[4,3], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
            ],
        ],
        'skip_unconverged_max_iter_3': [
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=3, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=i32[4])",
            ],
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=3, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=i32[4])",
            ],
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=3, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=i32[4])",
            ],
        ],
        'stop_rule': [
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
                'stop_compact(F[4], F[4,3], <loss_tol>, <grad_tol>, 0, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=None, eligible=None)',
            ],
            [
                'gather_rows(i32[4], F[4,3], F[4,3], 2)',
                'gather_rows(i32[4], F[4,2], F[4,2], 2)',
                'gather_rows(i32[4], F[4], F[4], 2)',
                'gather_rows(i32[4], F[4,3], F[4,3], 2)',
                'gather_rows(i32[4], F[4,3,1], F[4,3,1], 2)',
                "coc_solve(F[2,2], F[2], F[2,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[2,11,1], cost: F[2], costate_grid: F[2,11,2], iters: i32[2], state_grid: F[2,11,2], status: i32[2]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 2, 10, 16, 'auto', False)",
                'aux_solve(F[2], F[2,3], F[4], F[2,11,2], F[2,11,1], F[2,11,2], F[2,3], F[2,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[2,11,5,2], out={grad: F[2,3], loss: F[2], stats: i32[2,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[2], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,3], F[4,3], 2)',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=i32[4])",
                'stop_compact(F[2], F[2,3], <loss_tol>, <grad_tol>, 1, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=i32[2], eligible=None)',
            ],
            [
                'gather_rows(i32[4], F[4,3], F[4,3], 2)',
                "coc_solve(F[2,2], F[2], F[2,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[2,11,1], cost: F[2], costate_grid: F[2,11,2], iters: i32[2], state_grid: F[2,11,2], status: i32[2]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 2, 10, 16, 'auto', False)",
                'aux_solve(F[2], F[2,3], F[4], F[2,11,2], F[2,11,1], F[2,11,2], F[2,3], F[2,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[2,11,5,2], out={grad: F[2,3], loss: F[2], stats: i32[2,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[2], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,3], F[4,3], 2)',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=i32[4])",
                'stop_compact(F[2], F[2,3], <loss_tol>, <grad_tol>, 2, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=i32[2], eligible=None)',
            ],
        ],
        'stop_rule_warm': [
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
                'stop_compact(F[4], F[4,3], <loss_tol>, <grad_tol>, 0, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=None, eligible=None)',
                'gather_rows(i32[4], F[4,11,1], F[2,11,1], 2)',
                'gather_rows(i32[4], i32[4], i32[2], 2)',
            ],
            [
                'gather_rows(i32[4], F[4,3], F[4,3], 2)',
                'gather_rows(i32[4], F[4,2], F[4,2], 2)',
                'gather_rows(i32[4], F[4], F[4], 2)',
                'gather_rows(i32[4], F[4,3], F[4,3], 2)',
                'gather_rows(i32[4], F[4,3,1], F[4,3,1], 2)',
                "coc_solve(F[2,2], F[2], F[2,3], F[4], 10, 4, u_init=F[2,10,1], workspace=workspace, out={control_grid: F[2,11,1], cost: F[2], costate_grid: F[2,11,2], iters: i32[2], state_grid: F[2,11,2], status: i32[2]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 2, 10, 16, 'auto', False)",
                'aux_solve(F[2], F[2,3], F[4], F[2,11,2], F[2,11,1], F[2,11,2], F[2,3], F[2,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[2,11,5,2], out={grad: F[2,3], loss: F[2], stats: i32[2,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[2], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,3], F[4,3], 2)',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=i32[4])",
                'stop_compact(F[2], F[2,3], <loss_tol>, <grad_tol>, 1, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=i32[2], eligible=None)',
            ],
            [
                'gather_rows(i32[4], F[4,3], F[4,3], 2)',
                "coc_solve(F[2,2], F[2], F[2,3], F[4], 10, 4, u_init=F[2,10,1], workspace=workspace, out={control_grid: F[2,11,1], cost: F[2], costate_grid: F[2,11,2], iters: i32[2], state_grid: F[2,11,2], status: i32[2]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 2, 10, 16, 'auto', False)",
                'aux_solve(F[2], F[2,3], F[4], F[2,11,2], F[2,11,1], F[2,11,2], F[2,3], F[2,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[2,11,5,2], out={grad: F[2,3], loss: F[2], stats: i32[2,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[2], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,3], F[4,3], 2)',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=i32[4])",
                'stop_compact(F[2], F[2,3], <loss_tol>, <grad_tol>, 2, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=i32[2], eligible=None)',
            ],
        ],
        'stop_rule_all_stop': [
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
                'stop_compact(F[4], F[4,3], 1000000000.0, 0.0, 0, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=None, eligible=None)',
            ],
            [],
            [],
        ],
        'rows_flagged': [
            [
                'lookahead_rows(i32[4], F[4,5], F[4,3], F[4,3])',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'optimizer_step_rows(i32[4], F[4,5], F[4,3], F[4,3], 0, F[4,3], F[4,3], F[4,3], proj_lo=F[3], row_active=None)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
            ],
            [
                'lookahead_rows(i32[4], F[4,5], F[4,3], F[4,3])',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'optimizer_step_rows(i32[4], F[4,5], F[4,3], F[4,3], 1, F[4,3], F[4,3], F[4,3], proj_lo=F[3], row_active=None)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
            ],
            [
                'lookahead_rows(i32[4], F[4,5], F[4,3], F[4,3])',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'optimizer_step_rows(i32[4], F[4,5], F[4,3], F[4,3], 2, F[4,3], F[4,3], F[4,3], proj_lo=F[3], row_active=None)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
            ],
        ],
        'rows_flagged_stop_rule': [
            [
                'lookahead_rows(i32[4], F[4,5], F[4,3], F[4,3])',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'optimizer_step_rows(i32[4], F[4,5], F[4,3], F[4,3], 0, F[4,3], F[4,3], F[4,3], proj_lo=F[3], row_active=None)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'stop_compact(F[4], F[4,3], <loss_tol>, <grad_tol>, 0, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=None, eligible=None)',
            ],
            [
                'lookahead_rows(i32[4], F[4,5], F[4,3], F[4,3])',
                'gather_rows(i32[4], F[4,3], F[4,3], 2)',
                'gather_rows(i32[4], F[4,2], F[4,2], 2)',
                'gather_rows(i32[4], F[4], F[4], 2)',
                'gather_rows(i32[4], F[4,3], F[4,3], 2)',
                'gather_rows(i32[4], F[4,3,1], F[4,3,1], 2)',
                "coc_solve(F[2,2], F[2], F[2,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[2,11,1], cost: F[2], costate_grid: F[2,11,2], iters: i32[2], state_grid: F[2,11,2], status: i32[2]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 2, 10, 16, 'auto', False)",
                'aux_solve(F[2], F[2,3], F[4], F[2,11,2], F[2,11,1], F[2,11,2], F[2,3], F[2,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[2,11,5,2], out={grad: F[2,3], loss: F[2], stats: i32[2,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[2], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,3], F[4,3], 2)',
                'optimizer_step_rows(i32[4], F[4,5], F[4,3], F[4,3], 1, F[4,3], F[4,3], F[4,3], proj_lo=F[3], row_active=i32[4])',
                'gather_rows(i32[4], F[4,3], F[4,3], 2)',
                "coc_solve(F[2,2], F[2], F[2,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[2,11,1], cost: F[2], costate_grid: F[2,11,2], iters: i32[2], state_grid: F[2,11,2], status: i32[2]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 2, 10, 16, 'auto', False)",
                'aux_solve(F[2], F[2,3], F[4], F[2,11,2], F[2,11,1], F[2,11,2], F[2,3], F[2,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[2,11,5,2], out={grad: F[2,3], loss: F[2], stats: i32[2,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[2], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,3], F[4,3], 2)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,3], F[4,3], 2)',
                'stop_compact(F[2], F[2,3], <loss_tol>, <grad_tol>, 1, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=i32[2], eligible=None)',
            ],
            [
                'lookahead_rows(i32[4], F[4,5], F[4,3], F[4,3])',
                'gather_rows(i32[4], F[4,3], F[4,3], 2)',
                "coc_solve(F[2,2], F[2], F[2,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[2,11,1], cost: F[2], costate_grid: F[2,11,2], iters: i32[2], state_grid: F[2,11,2], status: i32[2]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 2, 10, 16, 'auto', False)",
                'aux_solve(F[2], F[2,3], F[4], F[2,11,2], F[2,11,1], F[2,11,2], F[2,3], F[2,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[2,11,5,2], out={grad: F[2,3], loss: F[2], stats: i32[2,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[2], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,3], F[4,3], 2)',
                'optimizer_step_rows(i32[4], F[4,5], F[4,3], F[4,3], 2, F[4,3], F[4,3], F[4,3], proj_lo=F[3], row_active=i32[4])',
                'gather_rows(i32[4], F[4,3], F[4,3], 2)',
                "coc_solve(F[2,2], F[2], F[2,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[2,11,1], cost: F[2], costate_grid: F[2,11,2], iters: i32[2], state_grid: F[2,11,2], status: i32[2]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 2, 10, 16, 'auto', False)",
                'aux_solve(F[2], F[2,3], F[4], F[2,11,2], F[2,11,1], F[2,11,2], F[2,3], F[2,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[2,11,5,2], out={grad: F[2,3], loss: F[2], stats: i32[2,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[2], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,3], F[4,3], 2)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,3], F[4,3], 2)',
                'stop_compact(F[2], F[2,3], <loss_tol>, <grad_tol>, 2, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=i32[2], eligible=None)',
            ],
        ],
        'shared_vanilla': [
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[1,3], F[1,3], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[1,3], v=F[1,3], vhat=F[1,3], proj_lo=F[3], row_active=None)",
            ],
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[1,3], F[1,3], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[1,3], v=F[1,3], vhat=F[1,3], proj_lo=F[3], row_active=None)",
            ],
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[1,3], F[1,3], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[1,3], v=F[1,3], vhat=F[1,3], proj_lo=F[3], row_active=None)",
            ],
        ],
        'shared_nesterov_true_loss': [
            [
                'lookahead(F[1,3], F[1,3], 0.9)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Nesterov', F[1,3], F[1,3], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[1,3], v=F[1,3], vhat=F[1,3], proj_lo=F[3], row_active=None)",
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
            ],
            [
                'lookahead(F[1,3], F[1,3], 0.9)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Nesterov', F[1,3], F[1,3], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[1,3], v=F[1,3], vhat=F[1,3], proj_lo=F[3], row_active=None)",
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
            ],
            [
                'lookahead(F[1,3], F[1,3], 0.9)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Nesterov', F[1,3], F[1,3], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[1,3], v=F[1,3], vhat=F[1,3], proj_lo=F[3], row_active=None)",
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
            ],
        ],
        'grouped_vanilla': [
            [
                'gather_rows(i32[4], F[2,3], F[4,3], 4)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,3], 2, H=None, row_ok=i32[4], out=(F[2], F[2,3], None, i32[2]))',
                "optimizer_step('Vanilla', F[2,3], F[2,3], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[2,3], v=F[2,3], vhat=F[2,3], proj_lo=F[3], row_active=i32[2])",
            ],
            [
                'gather_rows(i32[4], F[2,3], F[4,3], 4)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,3], 2, H=None, row_ok=i32[4], out=(F[2], F[2,3], None, i32[2]))',
                "optimizer_step('Vanilla', F[2,3], F[2,3], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[2,3], v=F[2,3], vhat=F[2,3], proj_lo=F[3], row_active=i32[2])",
            ],
            [
                'gather_rows(i32[4], F[2,3], F[4,3], 4)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,3], 2, H=None, row_ok=i32[4], out=(F[2], F[2,3], None, i32[2]))',
                "optimizer_step('Vanilla', F[2,3], F[2,3], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[2,3], v=F[2,3], vhat=F[2,3], proj_lo=F[3], row_active=i32[2])",
            ],
        ],
        'grouped_rules_flagged': [
            [
                'lookahead_rows(i32[2], F[2,5], F[2,3], F[2,3])',
                'gather_rows(i32[4], F[2,3], F[4,3], 4)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,3], 2, H=None, row_ok=i32[4], out=(F[2], F[2,3], None, i32[2]))',
                'optimizer_step_rows(i32[2], F[2,5], F[2,3], F[2,3], 0, F[2,3], F[2,3], F[2,3], proj_lo=F[3], row_active=i32[2])',
                'gather_rows(i32[4], F[2,3], F[4,3], 4)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,3], 2, H=None, row_ok=i32[4], out=(F[2], F[2,3], None, i32[2]))',
            ],
            [
                'lookahead_rows(i32[2], F[2,5], F[2,3], F[2,3])',
                'gather_rows(i32[4], F[2,3], F[4,3], 4)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,3], 2, H=None, row_ok=i32[4], out=(F[2], F[2,3], None, i32[2]))',
                'optimizer_step_rows(i32[2], F[2,5], F[2,3], F[2,3], 1, F[2,3], F[2,3], F[2,3], proj_lo=F[3], row_active=i32[2])',
                'gather_rows(i32[4], F[2,3], F[4,3], 4)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,3], 2, H=None, row_ok=i32[4], out=(F[2], F[2,3], None, i32[2]))',
            ],
            [
                'lookahead_rows(i32[2], F[2,5], F[2,3], F[2,3])',
                'gather_rows(i32[4], F[2,3], F[4,3], 4)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,3], 2, H=None, row_ok=i32[4], out=(F[2], F[2,3], None, i32[2]))',
                'optimizer_step_rows(i32[2], F[2,5], F[2,3], F[2,3], 2, F[2,3], F[2,3], F[2,3], proj_lo=F[3], row_active=i32[2])',
                'gather_rows(i32[4], F[2,3], F[4,3], 4)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,3], 2, H=None, row_ok=i32[4], out=(F[2], F[2,3], None, i32[2]))',
            ],
        ],
        'grouped_lm': [
            [
                'gather_rows(i32[4], F[2,3], F[4,3], 4)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=True, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,3], F[4,11,3,2], i32[1])',
                'group_reduce(F[4], F[4,3], 2, H=F[4,3,3], row_ok=i32[4], out=(F[2], F[2,3], F[2,3,3], i32[2]))',
                'lm_step(F[2,3], F[2], F[2,3], F[2,3,3], F[2], F[2,3], F[2], F[2,3], F[2,3,3], lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, proj_lo=F[3], row_active=i32[2], accepted=i32[2])',
            ],
            [
                'gather_rows(i32[4], F[2,3], F[4,3], 4)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=True, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,3], F[4,11,3,2], i32[1])',
                'group_reduce(F[4], F[4,3], 2, H=F[4,3,3], row_ok=i32[4], out=(F[2], F[2,3], F[2,3,3], i32[2]))',
                'lm_step(F[2,3], F[2], F[2,3], F[2,3,3], F[2], F[2,3], F[2], F[2,3], F[2,3,3], lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, proj_lo=F[3], row_active=i32[2], accepted=i32[2])',
            ],
            [
                'gather_rows(i32[4], F[2,3], F[4,3], 4)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=True, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,3], F[4,11,3,2], i32[1])',
                'group_reduce(F[4], F[4,3], 2, H=F[4,3,3], row_ok=i32[4], out=(F[2], F[2,3], F[2,3,3], i32[2]))',
                'lm_step(F[2,3], F[2], F[2,3], F[2,3,3], F[2], F[2,3], F[2], F[2,3], F[2,3,3], lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, proj_lo=F[3], row_active=i32[2], accepted=i32[2])',
            ],
        ],
        'lm': [
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=True, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,3], F[4,11,3,2], i32[1])',
                'lm_step(F[4,3], F[4], F[4,3], F[4,3,3], F[4], F[4,3], F[4], F[4,3], F[4,3,3], lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, proj_lo=F[3], row_active=None, accepted=i32[4])',
            ],
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=True, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,3], F[4,11,3,2], i32[1])',
                'lm_step(F[4,3], F[4], F[4,3], F[4,3,3], F[4], F[4,3], F[4], F[4,3], F[4,3,3], lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, proj_lo=F[3], row_active=None, accepted=i32[4])',
            ],
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=True, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,3], F[4,11,3,2], i32[1])',
                'lm_step(F[4,3], F[4], F[4,3], F[4,3,3], F[4], F[4,3], F[4], F[4,3], F[4,3,3], lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, proj_lo=F[3], row_active=None, accepted=i32[4])',
            ],
        ],
        'lm_stop_rule': [
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=True, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,3], F[4,11,3,2], i32[1])',
                'lm_step(F[4,3], F[4], F[4,3], F[4,3,3], F[4], F[4,3], F[4], F[4,3], F[4,3,3], lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, proj_lo=F[3], row_active=None, accepted=i32[4])',
                'stop_compact(F[4], F[4,3], <loss_tol>, <grad_tol>, 0, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=None, eligible=None)',
            ],
            [
                'gather_rows(i32[4], F[4,3], F[4,3], 2)',
                'gather_rows(i32[4], F[4,2], F[4,2], 2)',
                'gather_rows(i32[4], F[4], F[4], 2)',
                'gather_rows(i32[4], F[4,3], F[4,3], 2)',
                'gather_rows(i32[4], F[4,3,1], F[4,3,1], 2)',
                "coc_solve(F[2,2], F[2], F[2,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[2,11,1], cost: F[2], costate_grid: F[2,11,2], iters: i32[2], state_grid: F[2,11,2], status: i32[2]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 2, 10, 16, 'auto', False)",
                'aux_solve(F[2], F[2,3], F[4], F[2,11,2], F[2,11,1], F[2,11,2], F[2,3], F[2,3,1], i32[1], substeps=0, want_grids=True, Z_grid=F[2,11,5,2], out={grad: F[2,3], loss: F[2], stats: i32[2,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[2], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[2], F[2,3], F[2,11,3,2], i32[1])',
                'scatter_rows(i32[4], F[2,3,3], F[4,3,3], 2)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,3], F[4,3], 2)',
                'lm_step(F[4,3], F[4], F[4,3], F[4,3,3], F[4], F[4,3], F[4], F[4,3], F[4,3,3], lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, proj_lo=F[3], row_active=i32[4], accepted=i32[4])',
                'stop_compact(F[2], F[2,3], <loss_tol>, <grad_tol>, 1, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=i32[2], eligible=None)',
            ],
            [
                'gather_rows(i32[4], F[4,3], F[4,3], 2)',
                "coc_solve(F[2,2], F[2], F[2,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[2,11,1], cost: F[2], costate_grid: F[2,11,2], iters: i32[2], state_grid: F[2,11,2], status: i32[2]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 2, 10, 16, 'auto', False)",
                'aux_solve(F[2], F[2,3], F[4], F[2,11,2], F[2,11,1], F[2,11,2], F[2,3], F[2,3,1], i32[1], substeps=0, want_grids=True, Z_grid=F[2,11,5,2], out={grad: F[2,3], loss: F[2], stats: i32[2,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[2], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[2], F[2,3], F[2,11,3,2], i32[1])',
                'scatter_rows(i32[4], F[2,3,3], F[4,3,3], 2)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,3], F[4,3], 2)',
                'lm_step(F[4,3], F[4], F[4,3], F[4,3,3], F[4], F[4,3], F[4], F[4,3], F[4,3,3], lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, proj_lo=F[3], row_active=i32[4], accepted=i32[4])',
                'stop_compact(F[2], F[2,3], <loss_tol>, <grad_tol>, 2, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=i32[2], eligible=None)',
            ],
        ],
        'learn_taus_nesterov': [
            [
                'lookahead(F[4,3], F[4,3], 0.9)',
                'tau_project(F[4,3], F[4,3], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'waypoint_time_grad(F[4,11,2], F[4], F[4,3], F[4,3,1], i32[1], curv=None, consts=None, wp_weight=None, tau_ref=None, tau_prior=0.0, out=F[4,3])',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
                "optimizer_step('Nesterov', F[4,3], F[4,3], 0, 0.001, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=None, row_active=None)",
                'tau_project(F[4,3], F[4,3], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None, row_active=None)',
            ],
            [
                'lookahead(F[4,3], F[4,3], 0.9)',
                'tau_project(F[4,3], F[4,3], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'waypoint_time_grad(F[4,11,2], F[4], F[4,3], F[4,3,1], i32[1], curv=None, consts=None, wp_weight=None, tau_ref=None, tau_prior=0.0, out=F[4,3])',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
                "optimizer_step('Nesterov', F[4,3], F[4,3], 1, 0.001, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=None, row_active=None)",
                'tau_project(F[4,3], F[4,3], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None, row_active=None)',
            ],
            [
                'lookahead(F[4,3], F[4,3], 0.9)',
                'tau_project(F[4,3], F[4,3], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'waypoint_time_grad(F[4,11,2], F[4], F[4,3], F[4,3,1], i32[1], curv=None, consts=None, wp_weight=None, tau_ref=None, tau_prior=0.0, out=F[4,3])',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
                "optimizer_step('Nesterov', F[4,3], F[4,3], 2, 0.001, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=None, row_active=None)",
                'tau_project(F[4,3], F[4,3], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None, row_active=None)',
            ],
        ],
        'grouped_learn_taus_nesterov': [
            [
                'lookahead(F[4,3], F[4,3], 0.9)',
                'tau_project(F[4,3], F[4,3], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None)',
                'gather_rows(i32[4], F[2,3], F[4,3], 4)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,3], 2, H=None, row_ok=i32[4], out=(F[2], F[2,3], None, i32[2]))',
                'waypoint_time_grad(F[4,11,2], F[4], F[4,3], F[4,3,1], i32[1], curv=None, consts=None, wp_weight=None, tau_ref=None, tau_prior=0.0, out=F[4,3])',
                "optimizer_step('Vanilla', F[2,3], F[2,3], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[2,3], v=F[2,3], vhat=F[2,3], proj_lo=F[3], row_active=i32[2])",
                "optimizer_step('Nesterov', F[4,3], F[4,3], 0, 0.001, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=None, row_active=i32[4])",
                'tau_project(F[4,3], F[4,3], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None, row_active=i32[4])',
            ],
            [
                'lookahead(F[4,3], F[4,3], 0.9)',
                'tau_project(F[4,3], F[4,3], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None)',
                'gather_rows(i32[4], F[2,3], F[4,3], 4)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,3], 2, H=None, row_ok=i32[4], out=(F[2], F[2,3], None, i32[2]))',
                'waypoint_time_grad(F[4,11,2], F[4], F[4,3], F[4,3,1], i32[1], curv=None, consts=None, wp_weight=None, tau_ref=None, tau_prior=0.0, out=F[4,3])',
                "optimizer_step('Vanilla', F[2,3], F[2,3], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[2,3], v=F[2,3], vhat=F[2,3], proj_lo=F[3], row_active=i32[2])",
                "optimizer_step('Nesterov', F[4,3], F[4,3], 1, 0.001, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=None, row_active=i32[4])",
                'tau_project(F[4,3], F[4,3], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None, row_active=i32[4])',
            ],
            [
                'lookahead(F[4,3], F[4,3], 0.9)',
                'tau_project(F[4,3], F[4,3], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None)',
                'gather_rows(i32[4], F[2,3], F[4,3], 4)',
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=F[4,10,1], workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,3], 2, H=None, row_ok=i32[4], out=(F[2], F[2,3], None, i32[2]))',
                'waypoint_time_grad(F[4,11,2], F[4], F[4,3], F[4,3,1], i32[1], curv=None, consts=None, wp_weight=None, tau_ref=None, tau_prior=0.0, out=F[4,3])',
                "optimizer_step('Vanilla', F[2,3], F[2,3], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[2,3], v=F[2,3], vhat=F[2,3], proj_lo=F[3], row_active=i32[2])",
                "optimizer_step('Nesterov', F[4,3], F[4,3], 2, 0.001, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=None, row_active=i32[4])",
                'tau_project(F[4,3], F[4,3], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None, row_active=i32[4])',
            ],
        ],
        'lm_taus': [
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=True, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,3], F[4,11,3,2], i32[1])',
                'waypoint_time_grad(F[4,11,2], F[4], F[4,3], F[4,3,1], i32[1], curv=None, wp_weight=None)',
                'time_normal_blocks(F[4,11,2], F[4], F[4,3], F[4,11,3,2], i32[1], curv=None, wp_weight=None)',
                'lm_step_times(F[4,3], F[4], F[4,3], F[4,3,3], F[4], F[4,3], F[4,3], F[4,3], F[4,3], F[4,3,3], F[4,3], i32[4], F[4], F[4,3], F[4,3,3], F[4,3], F[4,3,3], F[4,3], group_size=1, lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, row_ok=None, wp_weight=None, proj_lo=F[3], group_active=None, accepted=i32[4])',
                'tau_project(F[4,3], F[4,3], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None, row_active=None)',
            ],
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=True, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,3], F[4,11,3,2], i32[1])',
                'waypoint_time_grad(F[4,11,2], F[4], F[4,3], F[4,3,1], i32[1], curv=None, wp_weight=None)',
                'time_normal_blocks(F[4,11,2], F[4], F[4,3], F[4,11,3,2], i32[1], curv=None, wp_weight=None)',
                'lm_step_times(F[4,3], F[4], F[4,3], F[4,3,3], F[4], F[4,3], F[4,3], F[4,3], F[4,3], F[4,3,3], F[4,3], i32[4], F[4], F[4,3], F[4,3,3], F[4,3], F[4,3,3], F[4,3], group_size=1, lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, row_ok=None, wp_weight=None, proj_lo=F[3], group_active=None, accepted=i32[4])',
                'tau_project(F[4,3], F[4,3], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None, row_active=None)',
            ],
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=True, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,3], F[4,11,3,2], i32[1])',
                'waypoint_time_grad(F[4,11,2], F[4], F[4,3], F[4,3,1], i32[1], curv=None, wp_weight=None)',
                'time_normal_blocks(F[4,11,2], F[4], F[4,3], F[4,11,3,2], i32[1], curv=None, wp_weight=None)',
                'lm_step_times(F[4,3], F[4], F[4,3], F[4,3,3], F[4], F[4,3], F[4,3], F[4,3], F[4,3], F[4,3,3], F[4,3], i32[4], F[4], F[4,3], F[4,3,3], F[4,3], F[4,3,3], F[4,3], group_size=1, lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, row_ok=None, wp_weight=None, proj_lo=F[3], group_active=None, accepted=i32[4])',
                'tau_project(F[4,3], F[4,3], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None, row_active=None)',
            ],
        ],
        'loss_fn_level_2': [
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], None, None, None, substeps=0, want_grids=True, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=2, auxX_grid=None, auxU_grid=None)',
                'grid_curvature(F[4,11,2])',
                'grid_curvature(F[4,11,1])',
                'grid_curvature(F[4,11,2])',
                'sample_grid(F[4,11,2], F[4], F[4,3], curv=F[4,11,2])',
                'sample_grid(F[4,11,1], F[4], F[4,3], curv=F[4,11,1])',
                'sample_grid(F[4,11,2], F[4], F[4,3], curv=F[4,11,2])',
                'waypoint_vjp(F[4], F[4,3], F[4,3,2], F[4,11,3,2], ru=F[4,3,1], auxU_grid=F[4,11,3,1])',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
            ],
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], None, None, None, substeps=0, want_grids=True, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=2, auxX_grid=None, auxU_grid=None)',
                'grid_curvature(F[4,11,2])',
                'grid_curvature(F[4,11,1])',
                'grid_curvature(F[4,11,2])',
                'sample_grid(F[4,11,2], F[4], F[4,3], curv=F[4,11,2])',
                'sample_grid(F[4,11,1], F[4], F[4,3], curv=F[4,11,1])',
                'sample_grid(F[4,11,2], F[4], F[4,3], curv=F[4,11,2])',
                'waypoint_vjp(F[4], F[4,3], F[4,3,2], F[4,11,3,2], ru=F[4,3,1], auxU_grid=F[4,11,3,1])',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
            ],
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], None, None, None, substeps=0, want_grids=True, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=2, auxX_grid=None, auxU_grid=None)',
                'grid_curvature(F[4,11,2])',
                'grid_curvature(F[4,11,1])',
                'grid_curvature(F[4,11,2])',
                'sample_grid(F[4,11,2], F[4], F[4,3], curv=F[4,11,2])',
                'sample_grid(F[4,11,1], F[4], F[4,3], curv=F[4,11,1])',
                'sample_grid(F[4,11,2], F[4], F[4,3], curv=F[4,11,2])',
                'waypoint_vjp(F[4], F[4,3], F[4,3,2], F[4,11,3,2], ru=F[4,3,1], auxU_grid=F[4,11,3,1])',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
            ],
        ],
        'weights_trace': [
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None, wp_weight=F[4,3])',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
                'trace_append(0, F[4], F[4,3], F[4,3], loss_trace=F[4,3], gnorm_trace=F[4,3], theta_trace=F[4,4,3], row_active=None)',
            ],
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None, wp_weight=F[4,3])',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
                'trace_append(1, F[4], F[4,3], F[4,3], loss_trace=F[4,3], gnorm_trace=F[4,3], theta_trace=F[4,4,3], row_active=None)',
            ],
            [
                "coc_solve(F[4,2], F[4], F[4,3], F[4], 10, 4, u_init=None, workspace=workspace, out={control_grid: F[4,11,1], cost: F[4], costate_grid: F[4,11,2], iters: i32[4], state_grid: F[4,11,2], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 10, 16, 'auto', False)",
                'aux_solve(F[4], F[4,3], F[4], F[4,11,2], F[4,11,1], F[4,11,2], F[4,3], F[4,3,1], i32[1], substeps=0, want_grids=False, Z_grid=F[4,11,5,2], out={grad: F[4,3], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None, wp_weight=F[4,3])',
                "optimizer_step('Vanilla', F[4,3], F[4,3], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,3], v=F[4,3], vhat=F[4,3], proj_lo=F[3], row_active=None)",
                'trace_append(2, F[4], F[4,3], F[4,3], loss_trace=F[4,3], gnorm_trace=F[4,3], theta_trace=F[4,4,3], row_active=None)',
            ],
        ],
    },
    'quadrotor': {
        'vanilla': [
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
            ],
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
            ],
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
            ],
        ],
        'nesterov_true_loss': [
            [
                'lookahead(F[4,7], F[4,7], 0.9)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Nesterov', F[4,7], F[4,7], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
            ],
            [
                'lookahead(F[4,7], F[4,7], 0.9)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Nesterov', F[4,7], F[4,7], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
            ],
            [
                'lookahead(F[4,7], F[4,7], 0.9)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Nesterov', F[4,7], F[4,7], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
            ],
        ],
        'adam_warm': [
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Adam', F[4,7], F[4,7], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
            ],
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Adam', F[4,7], F[4,7], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
            ],
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Adam', F[4,7], F[4,7], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
            ],
        ],
        'skip_unconverged_max_iter_3': [
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=3, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=i32[4])",
            ],
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=3, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=i32[4])",
            ],
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=3, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=i32[4])",
            ],
        ],
        'stop_rule': [
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
                'stop_compact(F[4], F[4,7], <loss_tol>, <grad_tol>, 0, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=None, eligible=None)',
            ],
            [
                'gather_rows(i32[4], F[4,7], F[4,7], 3)',
                'gather_rows(i32[4], F[4,13], F[4,13], 3)',
                'gather_rows(i32[4], F[4], F[4], 3)',
                'gather_rows(i32[4], F[4,5], F[4,5], 3)',
                'gather_rows(i32[4], F[4,5,3], F[4,5,3], 3)',
                "coc_solve(F[3,13], F[3], F[3,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[3,7,4], cost: F[3], costate_grid: F[3,7,13], iters: i32[3], state_grid: F[3,7,13], status: i32[3]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 3, 6, 16, 'auto', False)",
                'aux_solve(F[3], F[3,7], F[20], F[3,7,13], F[3,7,4], F[3,7,13], F[3,5], F[3,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[3,7,20,13], out={grad: F[3,7], loss: F[3], stats: i32[3,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[3], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'scatter_rows(i32[4], F[3], F[4], 3)',
                'scatter_rows(i32[4], F[3,7], F[4,7], 3)',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=i32[4])",
                'stop_compact(F[3], F[3,7], <loss_tol>, <grad_tol>, 1, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=i32[3], eligible=None)',
            ],
            [
                'gather_rows(i32[4], F[4,7], F[4,7], 2)',
                'gather_rows(i32[4], F[4,13], F[4,13], 2)',
                'gather_rows(i32[4], F[4], F[4], 2)',
                'gather_rows(i32[4], F[4,5], F[4,5], 2)',
                'gather_rows(i32[4], F[4,5,3], F[4,5,3], 2)',
                "coc_solve(F[2,13], F[2], F[2,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[2,7,4], cost: F[2], costate_grid: F[2,7,13], iters: i32[2], state_grid: F[2,7,13], status: i32[2]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 2, 6, 16, 'auto', False)",
                'aux_solve(F[2], F[2,7], F[20], F[2,7,13], F[2,7,4], F[2,7,13], F[2,5], F[2,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[2,7,20,13], out={grad: F[2,7], loss: F[2], stats: i32[2,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[2], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,7], F[4,7], 2)',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=i32[4])",
                'stop_compact(F[2], F[2,7], <loss_tol>, <grad_tol>, 2, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=i32[2], eligible=None)',
            ],
        ],
        'stop_rule_warm': [
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
                'stop_compact(F[4], F[4,7], <loss_tol>, <grad_tol>, 0, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=None, eligible=None)',
                'gather_rows(i32[4], F[4,7,4], F[3,7,4], 3)',
                'gather_rows(i32[4], i32[4], i32[3], 3)',
            ],
            [
                'gather_rows(i32[4], F[4,7], F[4,7], 3)',
                'gather_rows(i32[4], F[4,13], F[4,13], 3)',
                'gather_rows(i32[4], F[4], F[4], 3)',
                'gather_rows(i32[4], F[4,5], F[4,5], 3)',
                'gather_rows(i32[4], F[4,5,3], F[4,5,3], 3)',
                "coc_solve(F[3,13], F[3], F[3,7], F[20], 6, 4, u_init=F[3,6,4], workspace=workspace, out={control_grid: F[3,7,4], cost: F[3], costate_grid: F[3,7,13], iters: i32[3], state_grid: F[3,7,13], status: i32[3]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 3, 6, 16, 'auto', False)",
                'aux_solve(F[3], F[3,7], F[20], F[3,7,13], F[3,7,4], F[3,7,13], F[3,5], F[3,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[3,7,20,13], out={grad: F[3,7], loss: F[3], stats: i32[3,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[3], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'scatter_rows(i32[4], F[3], F[4], 3)',
                'scatter_rows(i32[4], F[3,7], F[4,7], 3)',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=i32[4])",
                'stop_compact(F[3], F[3,7], <loss_tol>, <grad_tol>, 1, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=i32[3], eligible=None)',
                'gather_rows(i32[4], F[3,7,4], F[2,7,4], 2)',
                'gather_rows(i32[4], i32[3], i32[2], 2)',
            ],
            [
                'gather_rows(i32[4], F[4,7], F[4,7], 2)',
                'gather_rows(i32[4], F[4,13], F[4,13], 2)',
                'gather_rows(i32[4], F[4], F[4], 2)',
                'gather_rows(i32[4], F[4,5], F[4,5], 2)',
                'gather_rows(i32[4], F[4,5,3], F[4,5,3], 2)',
                "coc_solve(F[2,13], F[2], F[2,7], F[20], 6, 4, u_init=F[2,6,4], workspace=workspace, out={control_grid: F[2,7,4], cost: F[2], costate_grid: F[2,7,13], iters: i32[2], state_grid: F[2,7,13], status: i32[2]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 2, 6, 16, 'auto', False)",
                'aux_solve(F[2], F[2,7], F[20], F[2,7,13], F[2,7,4], F[2,7,13], F[2,5], F[2,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[2,7,20,13], out={grad: F[2,7], loss: F[2], stats: i32[2,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[2], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,7], F[4,7], 2)',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=i32[4])",
                'stop_compact(F[2], F[2,7], <loss_tol>, <grad_tol>, 2, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=i32[2], eligible=None)',
            ],
        ],
        'stop_rule_all_stop': [
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
                'stop_compact(F[4], F[4,7], 1000000000.0, 0.0, 0, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=None, eligible=None)',
            ],
            [],
            [],
        ],
        'rows_flagged': [
            [
                'lookahead_rows(i32[4], F[4,5], F[4,7], F[4,7])',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'optimizer_step_rows(i32[4], F[4,5], F[4,7], F[4,7], 0, F[4,7], F[4,7], F[4,7], proj_lo=F[7], row_active=None)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
            ],
            [
                'lookahead_rows(i32[4], F[4,5], F[4,7], F[4,7])',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'optimizer_step_rows(i32[4], F[4,5], F[4,7], F[4,7], 1, F[4,7], F[4,7], F[4,7], proj_lo=F[7], row_active=None)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
            ],
            [
                'lookahead_rows(i32[4], F[4,5], F[4,7], F[4,7])',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'optimizer_step_rows(i32[4], F[4,5], F[4,7], F[4,7], 2, F[4,7], F[4,7], F[4,7], proj_lo=F[7], row_active=None)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
            ],
        ],
        'rows_flagged_stop_rule': [
            [
                'lookahead_rows(i32[4], F[4,5], F[4,7], F[4,7])',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'optimizer_step_rows(i32[4], F[4,5], F[4,7], F[4,7], 0, F[4,7], F[4,7], F[4,7], proj_lo=F[7], row_active=None)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'stop_compact(F[4], F[4,7], <loss_tol>, <grad_tol>, 0, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=None, eligible=None)',
            ],
            [
                'lookahead_rows(i32[4], F[4,5], F[4,7], F[4,7])',
                'gather_rows(i32[4], F[4,7], F[4,7], 2)',
                'gather_rows(i32[4], F[4,13], F[4,13], 2)',
                'gather_rows(i32[4], F[4], F[4], 2)',
                'gather_rows(i32[4], F[4,5], F[4,5], 2)',
                'gather_rows(i32[4], F[4,5,3], F[4,5,3], 2)',
                "coc_solve(F[2,13], F[2], F[2,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[2,7,4], cost: F[2], costate_grid: F[2,7,13], iters: i32[2], state_grid: F[2,7,13], status: i32[2]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 2, 6, 16, 'auto', False)",
                'aux_solve(F[2], F[2,7], F[20], F[2,7,13], F[2,7,4], F[2,7,13], F[2,5], F[2,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[2,7,20,13], out={grad: F[2,7], loss: F[2], stats: i32[2,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[2], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,7], F[4,7], 2)',
                'optimizer_step_rows(i32[4], F[4,5], F[4,7], F[4,7], 1, F[4,7], F[4,7], F[4,7], proj_lo=F[7], row_active=i32[4])',
                'gather_rows(i32[4], F[4,7], F[4,7], 2)',
                "coc_solve(F[2,13], F[2], F[2,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[2,7,4], cost: F[2], costate_grid: F[2,7,13], iters: i32[2], state_grid: F[2,7,13], status: i32[2]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 2, 6, 16, 'auto', False)",
                'aux_solve(F[2], F[2,7], F[20], F[2,7,13], F[2,7,4], F[2,7,13], F[2,5], F[2,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[2,7,20,13], out={grad: F[2,7], loss: F[2], stats: i32[2,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[2], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,7], F[4,7], 2)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,7], F[4,7], 2)',
                'stop_compact(F[2], F[2,7], <loss_tol>, <grad_tol>, 1, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=i32[2], eligible=None)',
            ],
            [
                'lookahead_rows(i32[4], F[4,5], F[4,7], F[4,7])',
                'gather_rows(i32[4], F[4,7], F[4,7], 2)',
                "coc_solve(F[2,13], F[2], F[2,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[2,7,4], cost: F[2], costate_grid: F[2,7,13], iters: i32[2], state_grid: F[2,7,13], status: i32[2]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 2, 6, 16, 'auto', False)",
                'aux_solve(F[2], F[2,7], F[20], F[2,7,13], F[2,7,4], F[2,7,13], F[2,5], F[2,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[2,7,20,13], out={grad: F[2,7], loss: F[2], stats: i32[2,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[2], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,7], F[4,7], 2)',
                'optimizer_step_rows(i32[4], F[4,5], F[4,7], F[4,7], 2, F[4,7], F[4,7], F[4,7], proj_lo=F[7], row_active=i32[4])',
                'gather_rows(i32[4], F[4,7], F[4,7], 2)',
                "coc_solve(F[2,13], F[2], F[2,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[2,7,4], cost: F[2], costate_grid: F[2,7,13], iters: i32[2], state_grid: F[2,7,13], status: i32[2]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 2, 6, 16, 'auto', False)",
                'aux_solve(F[2], F[2,7], F[20], F[2,7,13], F[2,7,4], F[2,7,13], F[2,5], F[2,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[2,7,20,13], out={grad: F[2,7], loss: F[2], stats: i32[2,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[2], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,7], F[4,7], 2)',
                'scatter_rows(i32[4], F[2], F[4], 2)',
                'scatter_rows(i32[4], F[2,7], F[4,7], 2)',
                'stop_compact(F[2], F[2,7], <loss_tol>, <grad_tol>, 2, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=i32[2], eligible=None)',
            ],
        ],
        'shared_vanilla': [
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[1,7], F[1,7], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[1,7], v=F[1,7], vhat=F[1,7], proj_lo=F[7], row_active=None)",
            ],
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[1,7], F[1,7], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[1,7], v=F[1,7], vhat=F[1,7], proj_lo=F[7], row_active=None)",
            ],
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Vanilla', F[1,7], F[1,7], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[1,7], v=F[1,7], vhat=F[1,7], proj_lo=F[7], row_active=None)",
            ],
        ],
        'shared_nesterov_true_loss': [
            [
                'lookahead(F[1,7], F[1,7], 0.9)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Nesterov', F[1,7], F[1,7], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[1,7], v=F[1,7], vhat=F[1,7], proj_lo=F[7], row_active=None)",
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
            ],
            [
                'lookahead(F[1,7], F[1,7], 0.9)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Nesterov', F[1,7], F[1,7], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[1,7], v=F[1,7], vhat=F[1,7], proj_lo=F[7], row_active=None)",
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
            ],
            [
                'lookahead(F[1,7], F[1,7], 0.9)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                "optimizer_step('Nesterov', F[1,7], F[1,7], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[1,7], v=F[1,7], vhat=F[1,7], proj_lo=F[7], row_active=None)",
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
            ],
        ],
        'grouped_vanilla': [
            [
                'gather_rows(i32[4], F[2,7], F[4,7], 4)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,7], 2, H=None, row_ok=i32[4], out=(F[2], F[2,7], None, i32[2]))',
                "optimizer_step('Vanilla', F[2,7], F[2,7], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[2,7], v=F[2,7], vhat=F[2,7], proj_lo=F[7], row_active=i32[2])",
            ],
            [
                'gather_rows(i32[4], F[2,7], F[4,7], 4)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,7], 2, H=None, row_ok=i32[4], out=(F[2], F[2,7], None, i32[2]))',
                "optimizer_step('Vanilla', F[2,7], F[2,7], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[2,7], v=F[2,7], vhat=F[2,7], proj_lo=F[7], row_active=i32[2])",
            ],
            [
                'gather_rows(i32[4], F[2,7], F[4,7], 4)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,7], 2, H=None, row_ok=i32[4], out=(F[2], F[2,7], None, i32[2]))',
                "optimizer_step('Vanilla', F[2,7], F[2,7], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[2,7], v=F[2,7], vhat=F[2,7], proj_lo=F[7], row_active=i32[2])",
            ],
        ],
        'grouped_rules_flagged': [
            [
                'lookahead_rows(i32[2], F[2,5], F[2,7], F[2,7])',
                'gather_rows(i32[4], F[2,7], F[4,7], 4)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,7], 2, H=None, row_ok=i32[4], out=(F[2], F[2,7], None, i32[2]))',
                'optimizer_step_rows(i32[2], F[2,5], F[2,7], F[2,7], 0, F[2,7], F[2,7], F[2,7], proj_lo=F[7], row_active=i32[2])',
                'gather_rows(i32[4], F[2,7], F[4,7], 4)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,7], 2, H=None, row_ok=i32[4], out=(F[2], F[2,7], None, i32[2]))',
            ],
            [
                'lookahead_rows(i32[2], F[2,5], F[2,7], F[2,7])',
                'gather_rows(i32[4], F[2,7], F[4,7], 4)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,7], 2, H=None, row_ok=i32[4], out=(F[2], F[2,7], None, i32[2]))',
                'optimizer_step_rows(i32[2], F[2,5], F[2,7], F[2,7], 1, F[2,7], F[2,7], F[2,7], proj_lo=F[7], row_active=i32[2])',
                'gather_rows(i32[4], F[2,7], F[4,7], 4)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,7], 2, H=None, row_ok=i32[4], out=(F[2], F[2,7], None, i32[2]))',
            ],
            [
                'lookahead_rows(i32[2], F[2,5], F[2,7], F[2,7])',
                'gather_rows(i32[4], F[2,7], F[4,7], 4)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,7], 2, H=None, row_ok=i32[4], out=(F[2], F[2,7], None, i32[2]))',
                'optimizer_step_rows(i32[2], F[2,5], F[2,7], F[2,7], 2, F[2,7], F[2,7], F[2,7], proj_lo=F[7], row_active=i32[2])',
                'gather_rows(i32[4], F[2,7], F[4,7], 4)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,7], 2, H=None, row_ok=i32[4], out=(F[2], F[2,7], None, i32[2]))',
            ],
        ],
        'grouped_lm': [
            [
                'gather_rows(i32[4], F[2,7], F[4,7], 4)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=True, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,5], F[4,7,7,13], i32[3])',
                'group_reduce(F[4], F[4,7], 2, H=F[4,7,7], row_ok=i32[4], out=(F[2], F[2,7], F[2,7,7], i32[2]))',
                'lm_step(F[2,7], F[2], F[2,7], F[2,7,7], F[2], F[2,7], F[2], F[2,7], F[2,7,7], lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, proj_lo=F[7], row_active=i32[2], accepted=i32[2])',
            ],
            [
                'gather_rows(i32[4], F[2,7], F[4,7], 4)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=True, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,5], F[4,7,7,13], i32[3])',
                'group_reduce(F[4], F[4,7], 2, H=F[4,7,7], row_ok=i32[4], out=(F[2], F[2,7], F[2,7,7], i32[2]))',
                'lm_step(F[2,7], F[2], F[2,7], F[2,7,7], F[2], F[2,7], F[2], F[2,7], F[2,7,7], lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, proj_lo=F[7], row_active=i32[2], accepted=i32[2])',
            ],
            [
                'gather_rows(i32[4], F[2,7], F[4,7], 4)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=True, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,5], F[4,7,7,13], i32[3])',
                'group_reduce(F[4], F[4,7], 2, H=F[4,7,7], row_ok=i32[4], out=(F[2], F[2,7], F[2,7,7], i32[2]))',
                'lm_step(F[2,7], F[2], F[2,7], F[2,7,7], F[2], F[2,7], F[2], F[2,7], F[2,7,7], lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, proj_lo=F[7], row_active=i32[2], accepted=i32[2])',
            ],
        ],
        'lm': [
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=True, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,5], F[4,7,7,13], i32[3])',
                'lm_step(F[4,7], F[4], F[4,7], F[4,7,7], F[4], F[4,7], F[4], F[4,7], F[4,7,7], lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, proj_lo=F[7], row_active=None, accepted=i32[4])',
            ],
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=True, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,5], F[4,7,7,13], i32[3])',
                'lm_step(F[4,7], F[4], F[4,7], F[4,7,7], F[4], F[4,7], F[4], F[4,7], F[4,7,7], lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, proj_lo=F[7], row_active=None, accepted=i32[4])',
            ],
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=True, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,5], F[4,7,7,13], i32[3])',
                'lm_step(F[4,7], F[4], F[4,7], F[4,7,7], F[4], F[4,7], F[4], F[4,7], F[4,7,7], lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, proj_lo=F[7], row_active=None, accepted=i32[4])',
            ],
        ],
        'lm_stop_rule': [
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=True, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,5], F[4,7,7,13], i32[3])',
                'lm_step(F[4,7], F[4], F[4,7], F[4,7,7], F[4], F[4,7], F[4], F[4,7], F[4,7,7], lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, proj_lo=F[7], row_active=None, accepted=i32[4])',
                'stop_compact(F[4], F[4,7], <loss_tol>, <grad_tol>, 0, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=None, eligible=None)',
            ],
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=True, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,5], F[4,7,7,13], i32[3])',
                'lm_step(F[4,7], F[4], F[4,7], F[4,7,7], F[4], F[4,7], F[4], F[4,7], F[4,7,7], lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, proj_lo=F[7], row_active=None, accepted=i32[4])',
                'stop_compact(F[4], F[4,7], <loss_tol>, <grad_tol>, 1, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=None, eligible=None)',
            ],
            [
                'gather_rows(i32[4], F[4,7], F[4,7], 1)',
                'gather_rows(i32[4], F[4,13], F[4,13], 1)',
                'gather_rows(i32[4], F[4], F[4], 1)',
                'gather_rows(i32[4], F[4,5], F[4,5], 1)',
                'gather_rows(i32[4], F[4,5,3], F[4,5,3], 1)',
                "coc_solve(F[1,13], F[1], F[1,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[1,7,4], cost: F[1], costate_grid: F[1,7,13], iters: i32[1], state_grid: F[1,7,13], status: i32[1]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 1, 6, 16, 'auto', False)",
                'aux_solve(F[1], F[1,7], F[20], F[1,7,13], F[1,7,4], F[1,7,13], F[1,5], F[1,5,3], i32[3], substeps=0, want_grids=True, Z_grid=F[1,7,20,13], out={grad: F[1,7], loss: F[1], stats: i32[1,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[1], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[1], F[1,5], F[1,7,7,13], i32[3])',
                'scatter_rows(i32[4], F[1,7,7], F[4,7,7], 1)',
                'scatter_rows(i32[4], F[1], F[4], 1)',
                'scatter_rows(i32[4], F[1,7], F[4,7], 1)',
                'lm_step(F[4,7], F[4], F[4,7], F[4,7,7], F[4], F[4,7], F[4], F[4,7], F[4,7,7], lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, proj_lo=F[7], row_active=i32[4], accepted=i32[4])',
                'stop_compact(F[1], F[1,7], <loss_tol>, <grad_tol>, 2, i32[4], i32[4], i32[1], i32[4], i32[4], rows_in=i32[1], eligible=None)',
            ],
        ],
        'learn_taus_nesterov': [
            [
                'lookahead(F[4,5], F[4,5], 0.9)',
                'tau_project(F[4,5], F[4,5], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'waypoint_time_grad(F[4,7,13], F[4], F[4,5], F[4,5,3], i32[3], curv=None, consts=None, wp_weight=None, tau_ref=None, tau_prior=0.0, out=F[4,5])',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
                "optimizer_step('Nesterov', F[4,5], F[4,5], 0, 0.001, 0.9, 0.9, 0.999, 1e-08, m=F[4,5], v=F[4,5], vhat=F[4,5], proj_lo=None, row_active=None)",
                'tau_project(F[4,5], F[4,5], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None, row_active=None)',
            ],
            [
                'lookahead(F[4,5], F[4,5], 0.9)',
                'tau_project(F[4,5], F[4,5], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'waypoint_time_grad(F[4,7,13], F[4], F[4,5], F[4,5,3], i32[3], curv=None, consts=None, wp_weight=None, tau_ref=None, tau_prior=0.0, out=F[4,5])',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
                "optimizer_step('Nesterov', F[4,5], F[4,5], 1, 0.001, 0.9, 0.9, 0.999, 1e-08, m=F[4,5], v=F[4,5], vhat=F[4,5], proj_lo=None, row_active=None)",
                'tau_project(F[4,5], F[4,5], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None, row_active=None)',
            ],
            [
                'lookahead(F[4,5], F[4,5], 0.9)',
                'tau_project(F[4,5], F[4,5], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'waypoint_time_grad(F[4,7,13], F[4], F[4,5], F[4,5,3], i32[3], curv=None, consts=None, wp_weight=None, tau_ref=None, tau_prior=0.0, out=F[4,5])',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
                "optimizer_step('Nesterov', F[4,5], F[4,5], 2, 0.001, 0.9, 0.9, 0.999, 1e-08, m=F[4,5], v=F[4,5], vhat=F[4,5], proj_lo=None, row_active=None)",
                'tau_project(F[4,5], F[4,5], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None, row_active=None)',
            ],
        ],
        'grouped_learn_taus_nesterov': [
            [
                'lookahead(F[4,5], F[4,5], 0.9)',
                'tau_project(F[4,5], F[4,5], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None)',
                'gather_rows(i32[4], F[2,7], F[4,7], 4)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,7], 2, H=None, row_ok=i32[4], out=(F[2], F[2,7], None, i32[2]))',
                'waypoint_time_grad(F[4,7,13], F[4], F[4,5], F[4,5,3], i32[3], curv=None, consts=None, wp_weight=None, tau_ref=None, tau_prior=0.0, out=F[4,5])',
                "optimizer_step('Vanilla', F[2,7], F[2,7], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[2,7], v=F[2,7], vhat=F[2,7], proj_lo=F[7], row_active=i32[2])",
                "optimizer_step('Nesterov', F[4,5], F[4,5], 0, 0.001, 0.9, 0.9, 0.999, 1e-08, m=F[4,5], v=F[4,5], vhat=F[4,5], proj_lo=None, row_active=i32[4])",
                'tau_project(F[4,5], F[4,5], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None, row_active=i32[4])',
            ],
            [
                'lookahead(F[4,5], F[4,5], 0.9)',
                'tau_project(F[4,5], F[4,5], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None)',
                'gather_rows(i32[4], F[2,7], F[4,7], 4)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,7], 2, H=None, row_ok=i32[4], out=(F[2], F[2,7], None, i32[2]))',
                'waypoint_time_grad(F[4,7,13], F[4], F[4,5], F[4,5,3], i32[3], curv=None, consts=None, wp_weight=None, tau_ref=None, tau_prior=0.0, out=F[4,5])',
                "optimizer_step('Vanilla', F[2,7], F[2,7], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[2,7], v=F[2,7], vhat=F[2,7], proj_lo=F[7], row_active=i32[2])",
                "optimizer_step('Nesterov', F[4,5], F[4,5], 1, 0.001, 0.9, 0.9, 0.999, 1e-08, m=F[4,5], v=F[4,5], vhat=F[4,5], proj_lo=None, row_active=i32[4])",
                'tau_project(F[4,5], F[4,5], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None, row_active=i32[4])',
            ],
            [
                'lookahead(F[4,5], F[4,5], 0.9)',
                'tau_project(F[4,5], F[4,5], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None)',
                'gather_rows(i32[4], F[2,7], F[4,7], 4)',
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=F[4,6,4], workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(3, 4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'group_reduce(F[4], F[4,7], 2, H=None, row_ok=i32[4], out=(F[2], F[2,7], None, i32[2]))',
                'waypoint_time_grad(F[4,7,13], F[4], F[4,5], F[4,5,3], i32[3], curv=None, consts=None, wp_weight=None, tau_ref=None, tau_prior=0.0, out=F[4,5])',
                "optimizer_step('Vanilla', F[2,7], F[2,7], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[2,7], v=F[2,7], vhat=F[2,7], proj_lo=F[7], row_active=i32[2])",
                "optimizer_step('Nesterov', F[4,5], F[4,5], 2, 0.001, 0.9, 0.9, 0.999, 1e-08, m=F[4,5], v=F[4,5], vhat=F[4,5], proj_lo=None, row_active=i32[4])",
                'tau_project(F[4,5], F[4,5], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None, row_active=i32[4])',
            ],
        ],
        'lm_taus': [
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=True, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,5], F[4,7,7,13], i32[3])',
                'waypoint_time_grad(F[4,7,13], F[4], F[4,5], F[4,5,3], i32[3], curv=None, wp_weight=None)',
                'time_normal_blocks(F[4,7,13], F[4], F[4,5], F[4,7,7,13], i32[3], curv=None, wp_weight=None)',
                'lm_step_times(F[4,7], F[4], F[4,7], F[4,7,7], F[4], F[4,7], F[4,5], F[4,5], F[4,5], F[4,5,7], F[4,5], i32[4], F[4], F[4,7], F[4,7,7], F[4,5], F[4,5,7], F[4,5], group_size=1, lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, row_ok=None, wp_weight=None, proj_lo=F[7], group_active=None, accepted=i32[4])',
                'tau_project(F[4,5], F[4,5], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None, row_active=None)',
            ],
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=True, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,5], F[4,7,7,13], i32[3])',
                'waypoint_time_grad(F[4,7,13], F[4], F[4,5], F[4,5,3], i32[3], curv=None, wp_weight=None)',
                'time_normal_blocks(F[4,7,13], F[4], F[4,5], F[4,7,7,13], i32[3], curv=None, wp_weight=None)',
                'lm_step_times(F[4,7], F[4], F[4,7], F[4,7,7], F[4], F[4,7], F[4,5], F[4,5], F[4,5], F[4,5,7], F[4,5], i32[4], F[4], F[4,7], F[4,7,7], F[4,5], F[4,5,7], F[4,5], group_size=1, lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, row_ok=None, wp_weight=None, proj_lo=F[7], group_active=None, accepted=i32[4])',
                'tau_project(F[4,5], F[4,5], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None, row_active=None)',
            ],
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=True, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None)',
                'normal_matrix(F[4], F[4,5], F[4,7,7,13], i32[3])',
                'waypoint_time_grad(F[4,7,13], F[4], F[4,5], F[4,5,3], i32[3], curv=None, wp_weight=None)',
                'time_normal_blocks(F[4,7,13], F[4], F[4,5], F[4,7,7,13], i32[3], curv=None, wp_weight=None)',
                'lm_step_times(F[4,7], F[4], F[4,7], F[4,7,7], F[4], F[4,7], F[4,5], F[4,5], F[4,5], F[4,5,7], F[4,5], i32[4], F[4], F[4,7], F[4,7,7], F[4,5], F[4,5,7], F[4,5], group_size=1, lambda_down=0.3333333333333333, lambda_up=2.0, lambda_min=1e-08, lambda_max=100000000.0, row_ok=None, wp_weight=None, proj_lo=F[7], group_active=None, accepted=i32[4])',
                'tau_project(F[4,5], F[4,5], F[4], 0.25, wp_weight=None, tau_lo=None, tau_hi=None, row_active=None)',
            ],
        ],
        'loss_fn_level_2': [
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], None, None, None, substeps=0, want_grids=True, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=2, auxX_grid=None, auxU_grid=None)',
                'grid_curvature(F[4,7,13])',
                'grid_curvature(F[4,7,4])',
                'grid_curvature(F[4,7,13])',
                'sample_grid(F[4,7,13], F[4], F[4,5], curv=F[4,7,13])',
                'sample_grid(F[4,7,4], F[4], F[4,5], curv=F[4,7,4])',
                'sample_grid(F[4,7,13], F[4], F[4,5], curv=F[4,7,13])',
                'waypoint_vjp(F[4], F[4,5], F[4,5,13], F[4,7,7,13], ru=F[4,5,4], auxU_grid=F[4,7,7,4])',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
            ],
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], None, None, None, substeps=0, want_grids=True, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=2, auxX_grid=None, auxU_grid=None)',
                'grid_curvature(F[4,7,13])',
                'grid_curvature(F[4,7,4])',
                'grid_curvature(F[4,7,13])',
                'sample_grid(F[4,7,13], F[4], F[4,5], curv=F[4,7,13])',
                'sample_grid(F[4,7,4], F[4], F[4,5], curv=F[4,7,4])',
                'sample_grid(F[4,7,13], F[4], F[4,5], curv=F[4,7,13])',
                'waypoint_vjp(F[4], F[4,5], F[4,5,13], F[4,7,7,13], ru=F[4,5,4], auxU_grid=F[4,7,7,4])',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
            ],
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], None, None, None, substeps=0, want_grids=True, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=2, auxX_grid=None, auxU_grid=None)',
                'grid_curvature(F[4,7,13])',
                'grid_curvature(F[4,7,4])',
                'grid_curvature(F[4,7,13])',
                'sample_grid(F[4,7,13], F[4], F[4,5], curv=F[4,7,13])',
                'sample_grid(F[4,7,4], F[4], F[4,5], curv=F[4,7,4])',
                'sample_grid(F[4,7,13], F[4], F[4,5], curv=F[4,7,13])',
                'waypoint_vjp(F[4], F[4,5], F[4,5,13], F[4,7,7,13], ru=F[4,5,4], auxU_grid=F[4,7,7,4])',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
            ],
        ],
        'weights_trace': [
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=None, out=None, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None, wp_weight=F[4,5])',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 0, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
                'trace_append(0, F[4], F[4,7], F[4,7], loss_trace=F[4,3], gnorm_trace=F[4,3], theta_trace=F[4,4,7], row_active=None)',
            ],
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None, wp_weight=F[4,5])',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 1, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
                'trace_append(1, F[4], F[4,7], F[4,7], loss_trace=F[4,3], gnorm_trace=F[4,3], theta_trace=F[4,4,7], row_active=None)',
            ],
            [
                "coc_solve(F[4,13], F[4], F[4,7], F[20], 6, 4, u_init=None, workspace=workspace, out={control_grid: F[4,7,4], cost: F[4], costate_grid: F[4,7,13], iters: i32[4], state_grid: F[4,7,13], status: i32[4]}, control_lb=None, control_ub=None, max_iter=300, tol=None, exact_after=16, mapping='auto')",
                "coc_workspace_bytes(F, 4, 6, 16, 'auto', False)",
                'aux_solve(F[4], F[4,7], F[20], F[4,7,13], F[4,7,4], F[4,7,13], F[4,5], F[4,5,3], i32[3], substeps=0, want_grids=False, Z_grid=F[4,7,20,13], out={grad: F[4,7], loss: F[4], stats: i32[4,4]}, phase_hook=<fn>, rtol=0.001, oc_status=i32[4], skip_status=(4), interp_level=1, auxX_grid=None, auxU_grid=None, wp_weight=F[4,5])',
                "optimizer_step('Vanilla', F[4,7], F[4,7], 2, 0.05, 0.9, 0.9, 0.999, 1e-08, m=F[4,7], v=F[4,7], vhat=F[4,7], proj_lo=F[7], row_active=None)",
                'trace_append(2, F[4], F[4,7], F[4,7], loss_trace=F[4,3], gnorm_trace=F[4,3], theta_trace=F[4,4,7], row_active=None)',
            ],
        ],
    },
}
