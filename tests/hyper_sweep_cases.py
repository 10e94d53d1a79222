"""Cases of the hyper-parameter sweeps in one batch (ABI 13: lfsd_optimizer_step_rows, lfsd_lookahead_rows, lfsd_trace_append; the
per-row arguments and `trace` of SparseDemoLearner; QuadAlgorithm.run_comparison), shared by the CPU tier (kernels through the SIMT
emulator, tests/test_hyper_sweep_emu.py) and the -m gpu tier (tests/test_hyper_sweep_gpu.py).

Yardsticks.  Kernel level: the scalar entry points (lfsd_optimizer_step, lfsd_lookahead) called once per (rule, hyper-parameter set)
on copies of the inputs -- a row of the rows call must hold their bits.  Learner level: a UNIFORM learner of the same batch, the same
seeds in the same slots, one per configuration -- a row's path does not depend on its partners (DESIGN.md sections 3.1 and 5), so a
row of the sweep must hold the bits of the row of the uniform learner with its configuration.  Identity, not a tolerance; the only
bound is the one of the gradient norm of lfsd_trace_append, (p + 2) eps relative: p roundings of the sum, one of the root."""
import numpy as np
import torch

SHAPES_EMU = ((1, 1), (5, 7), (67, 12), (4099, 7))      # 4099 x 7 leaves a partial last workgroup
SHAPES_GPU = ((1, 1), (67, 12), (4099, 7))
ITERS = (0, 1, 37)
GUARD, FILL = 8, 12345.0
# lr, mu, beta1, beta2, eps: the scripts' values (none is an fp32 number)
HYPER_SETS = ((0.06, 0.9, 0.9, 0.999, 1e-8), (0.22, 0.10, 0.999, 0.9, 0.01))
RULES = ("Vanilla", "Nesterov", "Adam", "Nadam", "AMSGrad")
BAD_CODE = 7

# test/opt_methods_comparison.py and test/adam_learning_rate_comparison.py
ADAM = dict(beta_1=0.9, beta_2=0.999, epsilon=1e-8)
METHOD_CONFIGS = (dict(method="Vanilla", learning_rate=0.06),
                  dict(method="Nesterov", learning_rate=0.01, mu=0.9, true_loss_print_flag=True),
                  dict(method="Adam", learning_rate=0.22, **ADAM),
                  dict(method="Nadam", learning_rate=0.10, **ADAM),
                  dict(method="AMSGrad", learning_rate=0.06, **ADAM))
ADAM_RATE_CONFIGS = tuple(dict(method="Adam", learning_rate=lr, **ADAM) for lr in (0.01, 0.02, 0.03, 0.04))
NINE_CONFIGS = METHOD_CONFIGS + ADAM_RATE_CONFIGS
DEFAULTS = dict(mu=0.9, beta_1=0.9, beta_2=0.999, epsilon=1e-8, true_loss_print_flag=False)


def same(a, b):
    """Equal, NaNs comparing as equal."""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def guarded(t):
    """A copy of `t` inside a guard band; returns (view, band)."""
    band = torch.full((t.numel() + 2 * GUARD,), FILL, dtype=t.dtype, device=t.device)
    view = band[GUARD:-GUARD].view(t.shape)
    view.copy_(t)
    return view, band


def band_intact(band):
    return bool((band[:GUARD] == FILL).all()) and bool((band[-GUARD:] == FILL).all())


def row_plan(B, offset=0):
    """(method code [B], set index [B]) cycling through the five rules and the two sets; rows `bad` (an unknown code) and `nan`
    (a NaN gradient) where the batch has room for them."""
    b = np.arange(B) + offset
    code, hset = (b % 5).astype(np.int32), ((b // 5) % 2).astype(np.int64)
    bad = 11 if B > 11 else None
    nan = 17 if B > 17 else None
    if bad is not None:
        code[bad] = BAD_CODE
    return code, hset, bad, nan


def opt_inputs(B, p, dtype, device, seed=0):
    g = torch.Generator().manual_seed(1000 * B + 10 * p + seed)
    r = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)
    to = lambda t: t.to(device=device, dtype=dtype).contiguous()
    theta, grad, m = r(B, p), r(B, p) * 10.0 ** (2 * torch.rand((B, 1), generator=g, dtype=torch.float64) - 1), 0.1 * r(B, p)
    v, vhat = r(B, p) ** 2, r(B, p) ** 2
    lo = torch.full((p,), -float("inf"), dtype=torch.float64)
    lo[::2] = 1e-8                                            # the examples' projection on every other parameter
    return to(theta), to(grad), to(m), to(v), to(vhat), to(lo)


def hyper_tensor(hset, dtype, device):
    """[B, 5], assembled in fp64 and cast once."""
    return torch.from_numpy(np.asarray(HYPER_SETS, dtype=np.float64)[hset]).to(device=device, dtype=dtype).contiguous()


def run_rows_against_scalars(lib, device, dtype, B, p, iter_idx, masked, offset=0):
    """lfsd_optimizer_step_rows against lfsd_optimizer_step per (rule, set), bit for bit; untouched rows and state keep their bits."""
    code, hset, bad, nan = row_plan(B, offset)
    theta0, grad, m0, v0, vhat0, lo = opt_inputs(B, p, dtype, device, seed=iter_idx)
    if nan is not None:
        grad[nan, p // 2] = float("nan")
    active = None
    act = np.ones(B, dtype=bool)
    if masked:
        act[::3] = False
        if nan is not None:
            act[nan] = True
        active = torch.from_numpy(act.astype(np.int32)).to(device)
    method = torch.from_numpy(code).to(device)
    hyper = hyper_tensor(hset, dtype, device)
    (th, bth), (m, bm), (v, bv), (vh, bvh) = guarded(theta0), guarded(m0), guarded(v0), guarded(vhat0)
    lib.optimizer_step_rows(method, hyper, th, grad, iter_idx, m, v, vh, proj_lo=lo, row_active=active)
    assert all(band_intact(b) for b in (bth, bm, bv, bvh)), (B, p, iter_idx, masked)
    init = (theta0, m0, v0, vhat0)
    got = (th, m, v, vh)
    finite_rows = np.ones(B, dtype=bool)
    if nan is not None:
        finite_rows[nan] = False
    checked = 0
    for rule in range(5):
        for k, hs in enumerate(HYPER_SETS):
            sel = (code == rule) & (hset == k)
            if not sel.any():
                continue
            ref = tuple(t.clone() for t in init)
            lib.optimizer_step(rule, ref[0], grad, iter_idx, hs[0], mu=hs[1], beta1=hs[2], beta2=hs[3], eps=hs[4], m=ref[1], v=ref[2],
                               vhat=ref[3], proj_lo=lo, row_active=active)
            idx = torch.from_numpy(np.nonzero(sel & finite_rows)[0]).to(device)
            for a, b in zip(got, ref):
                assert torch.equal(a[idx], b[idx]), (RULES[rule], k, B, p, iter_idx, masked)
            if nan is not None and sel[nan]:                  # a NaN gradient poisons its own row only: the scalar call's row,
                for a, b in zip(got, ref):                    # NaNs included (every other row is compared above)
                    assert same(a[nan], b[nan])
            # state the rule does not use keeps its bits
            unused = {0: (1, 2, 3), 1: (2, 3), 2: (3,), 3: (3,), 4: ()}[rule]
            all_idx = torch.from_numpy(np.nonzero(sel)[0]).to(device)
            for u in unused:
                assert torch.equal(got[u][all_idx], init[u][all_idx]), (RULES[rule], u)
            checked += int(sel.sum())
    assert checked == B - (bad is not None)
    # an unknown method code and a row_active == 0 row keep every bit
    frozen = ~act
    if bad is not None:
        frozen[bad] = True
    if frozen.any():
        idx = torch.from_numpy(np.nonzero(frozen)[0]).to(device)
        for a, b in zip(got, init):
            assert torch.equal(a[idx], b[idx])
    moved = act & (code != BAD_CODE) & finite_rows
    if moved.any():
        idx = torch.from_numpy(np.nonzero(moved)[0]).to(device)
        assert not torch.equal(th[idx], theta0[idx])         # (and the others did move)


def run_lookahead_rows(lib, device, dtype, B, p, offset=0):
    code, hset, bad, _ = row_plan(B, offset)
    theta, _, m, _, _, _ = opt_inputs(B, p, dtype, device, seed=5)
    other = np.nonzero(code != 1)[0]
    # m of a row that is not Nesterov is its first moment: NaN / Inf there must not reach out
    for k, r in enumerate(other):
        m[r, k % p] = (float("nan"), float("inf"), -float("inf"))[k % 3]
    method = torch.from_numpy(code).to(device)
    hyper = hyper_tensor(hset, dtype, device)
    out, band = guarded(torch.zeros_like(theta))
    res = lib.lookahead_rows(method, hyper, theta, m, out=out)
    assert res.data_ptr() == out.data_ptr() and band_intact(band)
    for k, hs in enumerate(HYPER_SETS):
        sel = np.nonzero((code == 1) & (hset == k))[0]
        if len(sel):
            ref = lib.lookahead(theta, m, hs[1])
            idx = torch.from_numpy(sel).to(device)
            assert torch.equal(out[idx], ref[idx]), (B, p, k)
            assert not torch.equal(out[idx], theta[idx])
    if len(other):
        idx = torch.from_numpy(other).to(device)
        assert torch.equal(out[idx], theta[idx]) and bool(torch.isfinite(out[idx]).all())


def run_trace_append(lib, device, dtype, B, p, masked, capacity=4):
    eps = float(torch.finfo(dtype).eps)
    nan_like = lambda *s: torch.full(s, float("nan"), dtype=dtype, device=device)
    (lt, blt), (gt, bgt), (tt, btt) = guarded(nan_like(B, capacity)), guarded(nan_like(B, capacity)), guarded(nan_like(B, capacity + 1, p))
    act = np.ones(B, dtype=bool)
    active = None
    if masked:
        act[::3] = False
        active = torch.from_numpy(act.astype(np.int32)).to(device)
    on = torch.from_numpy(act).to(device)
    filed = {}
    for it in (0, capacity - 1):
        theta, grad, _, _, _, _ = opt_inputs(B, p, dtype, device, seed=20 + it)
        loss = (grad ** 2).sum(dim=1).contiguous()
        lib.trace_append(it, loss, grad, theta, loss_trace=lt, gnorm_trace=gt, theta_trace=tt, row_active=active)
        filed[it] = (loss, grad, theta)
    assert band_intact(blt) and band_intact(bgt) and band_intact(btt)
    for it, (loss, grad, theta) in filed.items():
        assert torch.equal(lt[on, it], loss[on]) and torch.equal(tt[on, it + 1], theta[on])        # bit copies
        ref = torch.linalg.norm(grad.double(), dim=1)
        rel = ((gt[:, it].double() - ref).abs() / ref)[on]
        if act.any():
            assert float(rel.max()) <= (p + 2) * eps, (float(rel.max()), (p + 2) * eps)            # derived: p roundings + the root
    # every other trace word and every masked row still holds its NaN fill
    n_on = int(act.sum())
    assert int((~torch.isnan(lt)).sum()) == 2 * n_on and int((~torch.isnan(gt)).sum()) == 2 * n_on
    assert int((~torch.isnan(tt)).sum()) == 2 * n_on * p
    assert bool(torch.isnan(lt[:, 1:capacity - 1]).all()) and bool(torch.isnan(tt[:, 0]).all()) and bool(torch.isnan(tt[:, 2:capacity]).all())
    if masked:
        assert bool(torch.isnan(lt[~on]).all()) and bool(torch.isnan(gt[~on]).all()) and bool(torch.isnan(tt[~on]).all())
    # any one trace alone; the same bits as in the joint call
    g2, b2 = guarded(nan_like(B, capacity))
    loss, grad, theta = filed[0]
    lib.trace_append(0, loss, grad, theta, gnorm_trace=g2, row_active=active)
    assert band_intact(b2) and same(g2, torch.where(torch.arange(capacity, device=device)[None, :] == 0, gt, nan_like(B, capacity)))
    # a step beyond the capacity is refused by the entry point itself, before any launch
    L = lib.lib
    code = 0 if dtype == torch.float32 else 1
    p_ = lambda t: t.data_ptr()
    assert L.lfsd_trace_append(code, B, p, capacity, capacity, p_(loss), p_(grad), p_(theta), None, p_(lt), p_(gt), p_(tt), None) == -1
    assert L.lfsd_trace_append(code, B, p, -1, capacity, p_(loss), p_(grad), p_(theta), None, p_(lt), p_(gt), p_(tt), None) == -1


# ---- learner level ------------------------------------------------------------------------------------------------------------
def per_row_kwargs(configs, seeds):
    """The per-row arguments of a sweep learner: configuration-major, `seeds` rows per configuration."""
    full = [dict(DEFAULTS, **c) for c in configs]
    return {k: [c[k] for c in full for _ in range(seeds)] for k in full[0]}


def run_learner(L, steps):
    out = []
    for _ in range(steps):
        l, g = L.step()
        out.append((l.clone(), g.clone(), L.theta.clone()))
    return out


def sweep_against_uniform(make, configs, seeds, steps, distinct=True, **kw):
    """`make(**learner_kwargs)` builds a learner of len(configs) x seeds rows (configuration-major; the same seeds under every
    configuration).  The sweep learner against one uniform learner per configuration: per step loss, gradient and theta, and the
    three traces, row for row, identical.  Returns the sweep learner and its steps."""
    C = len(configs)
    sweep = make(trace=steps, **per_row_kwargs(configs, seeds), **kw)
    got = run_learner(sweep, steps)
    for i, cfg in enumerate(configs):
        uni = make(trace=steps, **cfg, **kw)
        assert not uni._rows_path
        ref = run_learner(uni, steps)
        rows = slice(i * seeds, (i + 1) * seeds)
        for k in range(steps):
            for a, b in zip(got[k], ref[k]):
                assert same(a[rows], b[rows]), (cfg, k)
        for name in ("loss_trace", "grad_norm_trace", "theta_trace"):
            assert same(getattr(sweep, name)[rows], getattr(uni, name)[rows]), (cfg, name)
        if "stop_rule" in kw:
            assert torch.equal(sweep.stop_iter[rows], uni.stop_iter[rows]), (cfg, sweep.stop_iter, uni.stop_iter)
        else:
            assert bool(torch.isfinite(uni.loss_trace[rows]).all())
    # after step 1, rows of different configurations hold different theta (same seed, another configuration)
    th1 = got[0][2].reshape(C, seeds, -1)
    for i in range(C if distinct else 0):      # (distinct=False: an option that may freeze a row for a step)
        for j in range(i + 1, C):
            assert bool((th1[i] != th1[j]).any(dim=1).all()), (configs[i], configs[j])
    assert same(sweep.theta_trace[:, steps], sweep.theta) and same(sweep.theta_trace[:, 1], got[0][2])
    return sweep, got


def squared_waypoint_loss(idx, wp):
    """The fused loss as a loss_fn (use with grad_scale=0.5: the reference's "no factor 2" convention)."""
    return lambda x_tau, u_tau: ((x_tau[:, :, idx] - wp) ** 2).sum((1, 2))


def quad_driver(n_grid, dtype, device=None, library=None):
    """A QuadAlgorithm on the workload of tests/test_stop_rule_emu.py::test_quadalgorithm_per_seed."""
    from lfsd_amd.QuadAlgorithm import QuadAlgorithm, QuadPara, DemoSparse
    from lfsd_amd.JinEnv import QuadStates
    cfg = {"QUAD_AVERAGE_SPEED": 1.0, "LAB_SPACE_LIMIT": {"LIMIT_X": [-3.2, 3.2], "LIMIT_Y": [-1.6, 1.6], "LIMIT_Z": [0.0, 2.2]}}
    ini, goal = QuadStates(position=[-2.0, -1.0, 0.6]), QuadStates(position=[2.5, 1.0, 1.5])
    demo = DemoSparse(waypoints=[[-1.0, -0.5, 0.9], [0.5, 0.2, 1.2], [1.8, 0.8, 1.4]], time_list=[0.25, 0.5, 0.75], time_horizon=1.0)

    def new():
        Q = QuadAlgorithm(cfg, QuadPara([1.0, 1.0, 1.0], 1.0, 1.0, 0.02), n_grid, device=device, dtype=dtype)
        Q.library = library
        return Q
    return new, ini, goal, demo


def run_comparison_case(new, ini, goal, demo, iter_num):
    """run_comparison on the five method configurations against load_optimization_function + run(stop="per_seed") one by one."""
    paras = [dict({k: v for k, v in c.items()}, iter_num=iter_num) for c in METHOD_CONFIGS]
    res = new().run_comparison(paras, ini, goal, demo)
    assert res["label_list"] == [c["method"] for c in METHOD_CONFIGS]
    assert len(res["loss_trace_comparison"]) == len(paras)
    for i, para in enumerate(paras):
        Q = new()
        Q.load_optimization_function(para)
        one = Q.run(ini, goal, demo, ObsList=[], stop="per_seed")
        ref = one["loss_trace"][:, 0]
        got = res["loss_trace_comparison"][i]
        assert got.shape == ref.shape and np.array_equal(got, ref), (para, got, ref)
        assert np.array_equal(res["parameter_trace"][i], one["parameter_trace"][:, 0]), para
        assert res["stop_iter"][i] == int(one["stop_iter"][0])
    # S = 2 seeds per configuration, one of which meets the reference's test (loss <= 0.9) at once: the demonstration lies next to
    # what the second seed flies anyway (as tests/test_stop_rule_emu.py::test_quadalgorithm_per_seed builds it)
    Q = new()
    Q.load_optimization_function(dict(paras[0], iter_num=1))
    base = np.array([1, 0.1, 0.1, 0.1, 0.1, 0.1, -1], dtype=float)
    probe = Q.run(ini, goal, type(demo)(waypoints=[[0, 0, 0.6]], time_list=[0.5], time_horizon=1.0), ObsList=[], initial_parameters=base)
    t = np.array([0.25, 0.5, 0.75])
    way = np.array([np.interp(t * 100, np.arange(101), probe["opt_state_traj"][:, i]) for i in range(3)]).T + 0.05
    near = type(demo)(waypoints=way.tolist(), time_list=t.tolist(), time_horizon=1.0)
    seeds = np.stack([base * 1.6, base])
    two = [paras[0], paras[1]]                                  # Vanilla and the flagged Nesterov
    res2 = new().run_comparison(two, ini, goal, near, initial_parameters=seeds)
    early = 0
    for i, para in enumerate(two):
        Q = new()
        Q.load_optimization_function(para)
        one = Q.run(ini, goal, near, ObsList=[], initial_parameters=seeds, stop="per_seed")
        assert res2["loss_trace_comparison"][i].shape == one["loss_trace"].shape == (one["loss_trace"].shape[0], 2)
        assert np.array_equal(res2["loss_trace_comparison"][i], one["loss_trace"]), para
        assert np.array_equal(res2["parameter_trace"][i], one["parameter_trace"]), para
        assert np.array_equal(res2["stop_iter"][i], one["stop_iter"]), para
        st = res2["stop_iter"][i]
        early += int(((st > 0) & (st < iter_num)).sum())
        took = np.where(st == 0, iter_num, st)
        assert res2["loss_trace_comparison"][i].shape[0] == took.max()
        for s_ in range(2):                                     # cut at the row's stop_iter: its last entry is repeated after it
            assert (res2["loss_trace_comparison"][i][took[s_] - 1:, s_] == res2["loss_trace_comparison"][i][took[s_] - 1, s_]).all()
    assert early >= 1 and iter_num >= 2                         # a row did stop before iter_num
    rates = [dict(c, iter_num=1) for c in ADAM_RATE_CONFIGS[:2]]
    assert new().run_comparison(rates, ini, goal, demo)["label_list"] == ["0.01", "0.02"]
    try:
        new().run_comparison([dict(paras[0]), dict(paras[1], iter_num=iter_num + 1)], ini, goal, demo)
    except ValueError:
        pass
    else:
        raise AssertionError("unequal iter_num must raise ValueError")
    return res
