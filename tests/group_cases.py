"""Cases of several demonstrations per seed (ABI 15: lfsd_group_reduce; SparseDemoLearner(mode="grouped", demos_per_seed=D)), shared by
the CPU tier (kernels through the SIMT emulator, tests/test_groups_emu.py) and the -m gpu tier (tests/test_groups_gpu.py).

Yardsticks and bounds.
  lfsd_group_reduce: exact.  torch.zeros plus the counted rows added one at a time, demonstrations ascending, in the kernel's dtype
    on the CPU -- IEEE additions and nothing else, so the kernel must give the same bits (torch.equal; NaN positions compared
    separately).  The inputs change sign and span eight decades: the test itself checks that the reverse order gives other bits.
  Learner: identity with the same launches made by hand (H.same); with D = 1 identity with the independent learner (torch.equal);
    G = 1 against mode='shared' after one Vanilla step: both sum D terms, each order is within (D - 1) u sum|g| of the exact sum
    (u = eps / 2), so the two differ by at most (D - 1) eps sum_d |g_dj|, times the learning rate on theta;
    loss_fn against the fused loss: per row sample_cases' bound (2 x its loss / gradient bound, as its "paths" comparison), on the
    group sums the sum of those plus (D - 1) eps sum_d |value_d| for the two reductions' own roundings;
    "it learns": conditions on a comparison made inside the test (below)."""
import ctypes

import numpy as np
import torch

import hyper_sweep_cases as H
import lm_cases as LMC

# (G, D, p): one element; a small odd one; 1 + 16 + 256 = 273 elements per group with H (a group straddles a workgroup); many groups;
# 1025 x 57 elements: a partial last workgroup
SHAPES = ((1, 1, 1), (2, 3, 7), (3, 2, 16), (67, 4, 12), (1025, 4, 7))
LM = LMC.LM


def eps_of(dtype):
    return float(torch.finfo(dtype).eps)


def same_bits(a, b):
    """torch.equal away from the NaNs, and the NaNs in the same places."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


# ---- lfsd_group_reduce ----------------------------------------------------------------------------------------------------------
def reduce_inputs(G, D, p, dtype, device, seed=0):
    """loss [B], grad [B, p], H [B, p, p] (bit-symmetric): signs at random, magnitudes 10^-4 .. 10^4."""
    g = torch.Generator().manual_seed(9176 * G + 131 * D + 17 * p + seed)
    B = G * D

    def val(*s):
        sign = torch.where(torch.rand(s, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)
        return sign * 10.0 ** (8.0 * torch.rand(s, generator=g, dtype=torch.float64) - 4.0) * (1.0 + torch.rand(s, generator=g, dtype=torch.float64))
    A = val(B, p, p)
    Hm = torch.tril(A) + torch.tril(A, -1).mT
    to = lambda t: t.to(device=device, dtype=dtype).contiguous()
    return to(val(B)), to(val(B, p)), to(Hm)


def reduce_mask(G, D, seed=0):
    """[B] int32: about a third of the rows left out; group G // 2 wholly; of group 0 (when it is not that group) the first row counts
    and, with D > 1, the last does not."""
    g = torch.Generator().manual_seed(77 * G + D + seed)
    ok = (torch.rand((G, D), generator=g) > 0.3).to(torch.int32)
    ok[G // 2] = 0
    if G > 1:
        ok[0, 0] = 1
        if D > 1:
            ok[0, D - 1] = 0
    return ok.reshape(-1).contiguous()


def reduce_reference(loss, grad, Hm, ok, D):
    """The sum rule on the CPU in the arrays' dtype: zeros, then one addition per counted row, demonstrations ascending."""
    outs = []
    B = loss.shape[0]
    G = B // D
    okc = None if ok is None else ok.cpu().reshape(G, D) != 0
    for t in (loss, grad, Hm):
        if t is None:
            outs.append(None)
            continue
        x = t.cpu().reshape((G, D) + tuple(t.shape[1:]))
        acc = torch.zeros((G,) + tuple(t.shape[1:]), dtype=t.dtype)
        for d in range(D):
            if okc is None:
                acc = acc + x[:, d]
            else:
                m = okc[:, d].reshape((G,) + (1,) * (t.dim() - 1))
                acc = torch.where(m, acc + x[:, d], acc)
        outs.append(acc)
    n_ok = torch.full((G,), D, dtype=torch.int32) if okc is None else okc.sum(dim=1).to(torch.int32)
    return outs[0], outs[1], outs[2], n_ok


def run_group_reduce(lib, device, dtype, G, D, p, with_H, masked):
    loss, grad, Hm = reduce_inputs(G, D, p, dtype, device)
    if not with_H:
        Hm = None
    ok = None
    if masked:
        ok = reduce_mask(G, D).to(device)
        out_rows = ok == 0                                      # NaN and inf in the rows left out, and only there
        fill = torch.tensor([float("nan"), float("inf"), -float("inf")], dtype=dtype, device=device)
        for t in (loss, grad) + (() if Hm is None else (Hm,)):
            flat = t.reshape(t.shape[0], -1)
            junk = fill[torch.arange(flat.shape[1], device=device) % 3][None, :].expand_as(flat)
            flat.copy_(torch.where(out_rows[:, None], junk, flat))
    new = lambda *s: torch.full(s, 777.0, dtype=dtype, device=device)
    (lg, b1), (gg, b2), (ng, b4) = H.guarded(new(G)), H.guarded(new(G, p)), H.guarded(torch.full((G,), 99, dtype=torch.int32, device=device))
    Hg, b3 = H.guarded(new(G, p, p)) if with_H else (None, None)
    res = lib.group_reduce(loss, grad, D, H=Hm, row_ok=ok, out=(lg, gg, Hg, ng))
    assert res[0].data_ptr() == lg.data_ptr() and res[3].data_ptr() == ng.data_ptr()
    assert all(H.band_intact(b) for b in (b1, b2, b4) + ((b3,) if with_H else ()))
    rl, rg, rH, rn = reduce_reference(loss, grad, Hm, ok, D)
    assert torch.equal(ng.cpu(), rn), (ng, rn)
    assert same_bits(lg.cpu(), rl) and same_bits(gg.cpu(), rg)
    assert bool(torch.isfinite(lg).all()) and bool(torch.isfinite(gg).all())      # nothing of a masked row got in
    if with_H:
        assert same_bits(Hg.cpu(), rH) and torch.equal(Hg, Hg.mT) and bool(torch.isfinite(Hg).all())
    if masked:
        gone = (rn == 0).to(device)
        assert bool(gone[G // 2]) and bool((lg[gone] == 0).all()) and bool((gg[gone] == 0).all())
        assert not with_H or bool((Hg[gone] == 0).all())
    elif D >= 3 and G * p >= 14:       # the inputs tell summation orders apart: descending d gives other bits somewhere
        rev = lambda t: t.reshape((G, D) + tuple(t.shape[1:])).flip(1).reshape(t.shape)
        _, rg2, _, _ = reduce_reference(rev(loss), rev(grad), None, None, D)
        assert not torch.equal(rg2, rg)
    # the outputs without out=, and the first G' < G groups alone: the same bits
    fresh = lib.group_reduce(loss, grad, D, H=Hm, row_ok=ok)
    assert same_bits(fresh[0], lg) and same_bits(fresh[1], gg) and torch.equal(fresh[3], ng) and (fresh[2] is None) == (not with_H)
    if G > 1:
        Gs = max(1, G // 2 + 1)
        cut = lambda t: None if t is None else t[:Gs * D].contiguous()
        part = lib.group_reduce(cut(loss), cut(grad), D, H=cut(Hm), row_ok=cut(ok))
        assert same_bits(part[0], lg[:Gs]) and same_bits(part[1], gg[:Gs]) and torch.equal(part[3], ng[:Gs])
        assert not with_H or same_bits(part[2], Hg[:Gs])


def run_group_reduce_nan(lib, device, dtype, G=5, D=3, p=4):
    """A NaN in a row that counts reaches its group's element and no other."""
    loss, grad, Hm = reduce_inputs(G, D, p, dtype, device, seed=3)
    ok = torch.ones(G * D, dtype=torch.int32, device=device)
    ok[2 * D] = 0                                              # (group 2 leaves its first row out, and counts the NaN row)
    grad[2 * D + 1, 1] = float("nan")
    loss[3 * D + 2] = float("nan")
    Hm[0 * D + 1, 2, 3] = Hm[0 * D + 1, 3, 2] = float("nan")
    lg, gg, Hg, ng = lib.group_reduce(loss, grad, D, H=Hm, row_ok=ok)
    rl, rg, rH, rn = reduce_reference(loss, grad, Hm, ok, D)
    assert same_bits(lg.cpu(), rl) and same_bits(gg.cpu(), rg) and same_bits(Hg.cpu(), rH) and torch.equal(ng.cpu(), rn)
    assert bool(torch.isnan(gg[2, 1])) and int(torch.isnan(gg).sum()) == 1
    assert bool(torch.isnan(lg[3])) and int(torch.isnan(lg).sum()) == 1
    assert bool(torch.isnan(Hg[0, 2, 3])) and bool(torch.isnan(Hg[0, 3, 2])) and int(torch.isnan(Hg).sum()) == 2


def group_reduce_einval(L, launches):
    """Every LFSD_EINVAL case of lfsd_group_reduce on host dummies (no launch is reached).  `launches`: the library runs on host
    memory (the emulator), so the base case itself can be called and must return 0."""
    buf = (ctypes.c_double * 256)()
    d = ctypes.cast(buf, ctypes.c_void_p).value
    at = lambda off: ctypes.c_void_p(d + off)
    # G = 2, D = 3, p = 2 in fp64: loss 48 B, grad 96 B, H 192 B, row_ok 24 B; loss_g 16 B, grad_g 32 B, H_g 64 B, n_ok 8 B
    base = dict(dtype=1, G=2, D=3, p=2, loss=at(0), grad=at(64), H=at(192), ok=at(448), loss_g=at(512), grad_g=at(576), H_g=at(640),
                n_ok=at(768))
    names = ("loss", "grad", "H", "ok", "loss_g", "grad_g", "H_g", "n_ok")
    call = lambda **kw: (lambda a: L.lfsd_group_reduce(a["dtype"], a["G"], a["D"], a["p"], *[a[nm] for nm in names], None))(dict(base, **kw))
    if launches:
        assert call() == 0 and call(H=None, H_g=None) == 0 and call(ok=None) == 0
    far = lambda k: ctypes.c_void_p(k << 40)
    bads = [dict(dtype=7), dict(dtype=-1), dict(G=0), dict(G=-1), dict(D=0), dict(D=-2), dict(p=0), dict(p=-1),
            dict(loss=None), dict(grad=None), dict(loss_g=None), dict(grad_g=None), dict(n_ok=None),
            dict(H=None), dict(H_g=None),                                      # exactly one of the two
            dict(loss_g=at(0)), dict(loss_g=at(40)), dict(loss_g=at(64 + 88)), dict(loss_g=at(448 + 16)),
            dict(grad_g=at(32)), dict(grad_g=at(192 - 8)), dict(H_g=at(192 + 184)), dict(H_g=at(0)), dict(n_ok=at(448 + 20)),
            dict(n_ok=at(192)), dict(n_ok=at(44)),
            # more than 2^31-1 workgroups, and an n_param whose square times n_groups leaves 62 bits (addresses far apart: nothing
            # overlaps, nothing is dereferenced)
            dict(G=2 ** 31 - 1, D=1, p=46340, loss=far(1), grad=far(2), H=far(8), ok=None, loss_g=far(3), grad_g=far(4), H_g=far(24),
                 n_ok=far(5)),
            dict(G=1, D=1, p=46341, loss=far(1), grad=far(2), H=far(8), ok=None, loss_g=far(3), grad_g=far(4), H_g=far(24), n_ok=far(5))]
    for bad in bads:
        assert call(**bad) == -1, bad


def binding_refusals(ml):
    """What ModelLibrary.group_reduce refuses by looking: a list of thunks that must raise LfsdError (CPU tensors: the emulator's)."""
    z = lambda *s: torch.zeros(s, dtype=torch.float64)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    return (lambda: ml.group_reduce(z(6), z(6, 2), 4),                                       # B % D
            lambda: ml.group_reduce(z(6), z(6, 2), 0),
            lambda: ml.group_reduce(z(6), z(6, 2), 1.5),
            lambda: ml.group_reduce(z(5), z(6, 2), 3),                                       # loss of another batch
            lambda: ml.group_reduce(z(6).float(), z(6, 2), 3),
            lambda: ml.group_reduce(z(6), z(6, 2).half(), 3),
            lambda: ml.group_reduce(z(6), z(6), 3),                                          # grad is [B, p]
            lambda: ml.group_reduce(z(6), z(6, 2), 3, H=z(6, 2, 3)),
            lambda: ml.group_reduce(z(6), z(6, 2), 3, row_ok=torch.zeros(6, dtype=torch.int64)),
            lambda: ml.group_reduce(z(6), z(6, 2), 3, row_ok=torch.zeros(6, dtype=torch.bool)),
            lambda: ml.group_reduce(z(6), z(6, 2), 3, row_ok=i32(2)),
            lambda: ml.group_reduce(z(6), z(6, 2), 3, out=(z(2), z(2, 2), z(2, 2, 2), i32(2))),      # H_g without H
            lambda: ml.group_reduce(z(6), z(6, 2), 3, H=z(6, 2, 2), out=(z(2), z(2, 2), None, i32(2))),
            lambda: ml.group_reduce(z(6), z(6, 2), 3, out=(z(3), z(2, 2), None, i32(2))),
            lambda: ml.group_reduce(z(6), z(6, 2), 3, out=(z(2), z(2, 2), None, z(2))),
            lambda: ml.group_reduce(z(6), z(6, 2), 3, out=(z(2), z(2, 2), None)))


# ---- the learner ----------------------------------------------------------------------------------------------------------------
# Three demonstrations of the pendulum: another start state, horizon and waypoint set each (the waypoint times are the same
# fractions of each horizon).  Far from any trajectory of the model, as lm_cases' waypoints are.
PENDULUM_DEMOS = dict(ini_state=[[0.0, 0.0], [0.3, 0.0], [-0.2, 0.1]], horizon=[1.0, 0.9, 1.1],
                      taus=[[0.2, 0.5, 0.8], [0.18, 0.45, 0.72], [0.22, 0.55, 0.88]],
                      waypoints=[[[0.4], [1.5], [2.6]], [[0.5], [1.3], [2.2]], [[0.2], [1.0], [2.0]]])
COMPOSE_STEPS = 4
# The pendulum's sweeps, error-controlled at the default tolerance, flag an interval accepted above it for about a third of these rows
# (mask_unconverged then leaves the row out: seen on the emulator, erratic from step to step).  The learner cases fix the sub-stepping,
# as smoke() does, so that a row is left out only where a case means it to be.  The LM cases take lm_lambda0 = 30: at 1 the nearly
# undamped steps leave whole groups without a converged demonstration from step 2 on, and frozen state would be compared with itself.
FIXED_SUBSTEPS = dict(aux_rtol=0.0, aux_substeps=8)
SEED_SCALE = 0.2
NESTEROV = dict(method="Nesterov", learning_rate=0.01, mu=0.9, true_loss_print_flag=True)
FIVE_RULES = H.METHOD_CONFIGS                      # Vanilla, Nesterov (flag: refused per group, dropped below), Adam, Nadam, AMSGrad


def pendulum_args(d, G, seed_rows=None):
    """(ini_state [D, n], horizon [D], taus [D, K], waypoints [D, K, 1], interface, theta0 [G, p]) -- per demonstration: the learner tiles."""
    P = PENDULUM_DEMOS
    th0 = np.asarray(d["theta0"], dtype=np.float64)      # (lm_cases' seeds, at SEED_SCALE: most rows pass the sweeps' tolerance flag)
    seeds = (th0[None, :] * (1.0 + SEED_SCALE * np.random.default_rng(LMC.COMPOSE_SEED).uniform(-1, 1, (seed_rows or G, th0.size))))[:G]
    return (np.asarray(P["ini_state"]), np.asarray(P["horizon"]), np.asarray(P["taus"]), np.asarray(P["waypoints"]), [0], seeds)


def quadrotor_args(d, G, D):
    """D demonstrations of the quadrotor: the start position and the waypoints moved by up to 0.2 m per demonstration."""
    rng = np.random.default_rng(11)
    x0 = np.tile(np.asarray(d["ini_state"], dtype=np.float64), (D, 1))
    x0[:, :3] += 0.2 * rng.uniform(-1, 1, (D, 3))
    wps = np.asarray(d["waypoints"], dtype=np.float64)[None] + 0.2 * rng.uniform(-1, 1, (D,) + np.asarray(d["waypoints"]).shape)
    seeds = np.asarray(d["theta0"], dtype=np.float64)[None, :] * (1.0 + 0.2 * np.random.default_rng(5).uniform(-1, 1, (G, len(d["theta0"]))))
    return (x0, d["horizon"], np.asarray(d["taus"]), wps, d["interface"], seeds)


def rules_kwargs(G, true_loss=False):
    """A per-group list of the five rules (cycled over G groups).  `true_loss`: the scalar flag -- the Nesterov groups then take
    their loss and gradient from a second evaluation at theta."""
    cfgs = [dict(H.DEFAULTS, **FIVE_RULES[g % 5]) for g in range(G)]
    kw = {k: [c[k] for c in cfgs] for k in ("method", "learning_rate", "mu", "beta_1", "beta_2", "epsilon")}
    return dict(kw, true_loss_print_flag=True) if true_loss else kw


def tiled(oc, args, G, D):
    """The [B]-row tensors of per-demonstration `args`, as the learner builds them."""
    x0, hz, taus, wps = (oc._t(a) for a in args[:4])
    B = G * D
    x0 = x0.repeat(G, 1) if x0.shape[0] == D else x0
    hz = hz.expand(B).contiguous() if hz.dim() == 0 else (hz.repeat(G) if hz.shape[0] == D else hz)
    taus = taus.unsqueeze(0).expand(B, -1).contiguous() if taus.dim() == 1 else (taus.repeat(G, 1) if taus.shape[0] == D else taus)
    wps = wps.unsqueeze(0).expand(B, -1, -1).contiguous() if wps.dim() == 2 else (wps.repeat(G, 1, 1) if wps.shape[0] == D else wps)
    return x0.contiguous(), hz.contiguous(), taus.contiguous(), wps.contiguous()


def grouped_by_hand(oc, args, G, D, steps, proj_lo, rule, lambda0=1e-2, level=1, warm=False):
    """The grouped iteration from its launches: evaluation point on G rows, lfsd_gather_rows, cocSolverBatch, auxSysSolverBatch (rows the
    solve left unconverged skipped), the mask of skip_unconverged (the default of the mode), lib.normal_matrix, lib.group_reduce, the
    update on G rows.  `rule`: dict(method=...) of a uniform rule, a dict of per-group lists, or "LM".  Yields per step a dict of the
    state after the update and of the (loss, grad) step() returns.  `level` / `warm`: interplation_level and warm_start."""
    lib = oc.compile()
    x0, hz, taus, wps = tiled(oc, args, G, D)
    iface = args[4]
    th = oc._t(args[5]).contiguous().clone()
    p, dev, dt = th.shape[1], th.device, th.dtype
    B = G * D
    idx = torch.as_tensor(list(iface), dtype=torch.int32, device=dev)
    gidx = (torch.arange(B, dtype=torch.int32, device=dev) // D).contiguous()
    lm = rule == "LM"
    z = lambda: torch.zeros_like(th)
    m, v, vhat = z(), z(), z()
    if lm:
        trial = th.clone()
        loss_acc = torch.full((G,), float("inf"), dtype=dt, device=dev)
        g_acc, H_acc = z(), torch.zeros((G, p, p), dtype=dt, device=dev)
        lam = torch.full((G,), lambda0, dtype=dt, device=dev)
    else:
        rows = not isinstance(rule["method"], str)
        if rows:
            codes = torch.from_numpy(np.array([H.RULES.index(mth) for mth in rule["method"]], dtype=np.int32)).to(dev)
            hyper = torch.from_numpy(np.stack([np.asarray(rule[k], dtype=np.float64) for k in
                                               ("learning_rate", "mu", "beta_1", "beta_2", "epsilon")], axis=1)).to(device=dev, dtype=dt).contiguous()
        else:
            hp = dict(H.DEFAULTS, **rule)
    prev = [None]

    def evaluate(point):
        rows_th = lib.gather_rows(gidx, point.contiguous(), torch.empty((B, p), dtype=dt, device=dev), B)
        u_init = None
        if prev[0] is not None:      # (skip_unconverged: a solve at the iteration limit is continued, every other one cold-starts)
            cont = (prev[0]["status"] == 3).reshape(-1, 1, 1)
            pu = prev[0]["control_grid"][:, :-1]
            u_init = pu.contiguous() if warm else torch.where(cont & torch.isfinite(pu), pu, torch.zeros_like(pu)).contiguous()
        sol = oc.cocSolverBatch(x0, hz, rows_th, consts=oc.consts_tensor(), u_init=u_init)
        prev[0] = sol
        aux = oc.auxSysSolverBatch(sol, taus, wps, iface, want_grids=lm, validate=False, skip_status=(3, 4), interplation_level=level)
        loss, grad = aux["loss"].to(dt), aux["grad"].to(dt)
        st = sol["status"]
        ok = ((st == 1) | (st == 2)) & torch.isfinite(loss) & torch.isfinite(grad).all(dim=1)
        if aux.get("stats") is not None:
            ok = ok & ((aux["stats"][:, 1] + aux["stats"][:, 3]) == 0)
        grad = torch.where(ok.unsqueeze(1), grad, torch.zeros_like(grad))
        Hm = None
        if lm:
            aX = aux["auxX_grid"]
            Hm = lib.normal_matrix(hz.to(aX.dtype).contiguous(), taus.to(aX.dtype).contiguous(), aX, idx).to(dt).contiguous()
        lg, gg, Hg, n_ok = lib.group_reduce(loss.contiguous(), grad.contiguous(), D, H=Hm, row_ok=ok.to(torch.int32))
        return lg, gg, Hg, n_ok, loss, grad

    for it in range(steps):
        if lm:
            point = trial
        elif rows:
            point = lib.lookahead_rows(codes, hyper, th, m) if "Nesterov" in rule["method"] else th
        else:
            point = lib.lookahead(th, m, hp["mu"]) if hp["method"] == "Nesterov" else th
        lg, gg, Hg, n_ok, rl, rg = evaluate(point)
        active = (n_ok > 0).to(torch.int32)
        if lm:
            lib.lm_step(th, loss_acc, g_acc, H_acc, lam, trial, lg, gg, Hg, proj_lo=proj_lo, row_active=active, **LM)
        elif rows:
            lib.optimizer_step_rows(codes, hyper, th, gg, it, m, v, vhat, proj_lo=proj_lo, row_active=active)
            flag = codes == H.RULES.index("Nesterov")
            if rule.get("true_loss_print_flag") and bool(flag.any()):
                # the flagged groups take the second evaluation; every other group (and its rows' start state) stays the first's
                first = (prev[0]["control_grid"].clone(), prev[0]["status"].clone())
                l1, g1, n1 = lg.clone(), gg.clone(), n_ok.clone()
                l2, g2, _, n2, rl, rg = evaluate(th)
                fB = flag.repeat_interleave(D)
                for t, t1 in zip((prev[0]["control_grid"], prev[0]["status"]), first):
                    t.copy_(torch.where(fB.reshape((-1,) + (1,) * (t.dim() - 1)), t, t1))
                lg, gg, n_ok = torch.where(flag, l2, l1), torch.where(flag.unsqueeze(1), g2, g1), torch.where(flag, n2, n1)
        else:
            lib.optimizer_step(hp["method"], th, gg, it, hp["learning_rate"], hp["mu"], hp["beta_1"], hp["beta_2"], hp["epsilon"],
                               m=m, v=v, vhat=vhat, proj_lo=proj_lo, row_active=active)
            if hp["method"] == "Nesterov" and hp["true_loss_print_flag"]:
                lg, gg, Hg, n_ok, rl, rg = evaluate(th)
        out = dict(theta=th.clone(), m=m.clone(), v=v.clone(), vhat=vhat.clone(), loss=lg.clone(), grad=gg.clone(), n_ok=n_ok.clone(),
                   row_loss=rl.clone(), row_grad=rg.clone())
        if lm:
            out.update(theta_trial=trial.clone(), lm_lambda=lam.clone(), lm_loss=loss_acc.clone(), normal_matrix=H_acc.clone())
        yield out


STATE = ("theta", "m", "v", "vhat", "theta_trial", "lm_lambda", "lm_loss", "normal_matrix", "n_ok", "row_loss", "row_grad")


def run_composition(make, oc, args, G, D, rule, steps=COMPOSE_STEPS, lambda0=1e-2, level=1, warm=False):
    """`make(groups=G', **kw)` builds the grouped learner of the first G' groups of `args`.  The learner against its launches made by
    hand, bit for bit, for `steps` steps; then the first groups alone in a learner of fewer groups: the same bits."""
    kw = dict(method="LM", lm_lambda0=lambda0) if rule == "LM" else dict(rule)
    if level != 1 or warm:
        kw.update(interplation_level=level, warm_start=warm)
    L = make(groups=G, **kw)
    assert (L.n_groups, L.demos_per_seed, L.B) == (G, D, G * D) and L.skip_unconverged
    hand = grouped_by_hand(oc, args, G, D, steps, L.proj_lo, rule, lambda0=lambda0, level=level, warm=warm)
    hist = []
    for k in range(steps):
        loss, grad = L.step()
        ref = next(hand)
        assert loss.shape == (G,) and grad.shape == (G, L.theta.shape[1])
        assert H.same(loss, ref["loss"]) and H.same(grad, ref["grad"]), k
        for nm in STATE:
            if nm in ref:
                assert H.same(getattr(L, nm), ref[nm]), (k, nm)
        hist.append(dict(ref))
    assert bool(torch.isfinite(hist[-1]["loss"]).all()) and bool((hist[-1]["theta"] != hist[0]["theta"]).any())
    print("rows counted per group and step:", [h["n_ok"].tolist() for h in hist])
    assert bool((hist[0]["n_ok"] == D).all())
    if rule == "LM":
        assert torch.equal(L.normal_matrix, L.normal_matrix.mT) and L.normal_matrix.shape == (G, L.theta.shape[1], L.theta.shape[1])
    if G > 1:
        Gs = max(1, G // 2 + (G > 2))
        cut = lambda v: v[:Gs] if isinstance(v, list) else v
        Ls = make(groups=Gs, **{k: cut(v) for k, v in kw.items()})
        for k in range(steps):
            loss, grad = Ls.step()
            assert H.same(loss, hist[k]["loss"][:Gs]) and H.same(grad, hist[k]["grad"][:Gs]), k
            for nm in STATE:
                if nm in hist[k] and not nm.startswith("row_"):
                    assert H.same(getattr(Ls, nm), hist[k][nm][:Gs]), (k, nm)
            assert H.same(Ls.row_loss, hist[k]["row_loss"][:Gs * D])
    return L, hist


def run_one_demonstration_is_independent(make_grouped, make_independent, steps=4):
    """D = 1: the grouped learner is the independent learner with the same skip_unconverged, word for word."""
    a, b = make_grouped(), make_independent()
    for k in range(steps):
        (la, ga), (lb, gb) = a.step(), b.step()
        on = a.n_ok > 0      # (a group without a counted row returns zeros, the independent learner the row's own values)
        assert torch.equal(la[on], lb[on]) and torch.equal(ga[on], gb[on]) and torch.equal(a.theta, b.theta), k
        assert torch.equal(on, b._ok)
        for nm in ("m", "v", "vhat", "theta_trial", "lm_lambda", "lm_loss", "normal_matrix"):
            if getattr(b, nm, None) is not None:
                assert torch.equal(getattr(a, nm), getattr(b, nm)), (k, nm)
    assert bool((a.n_ok == 1).all()) and a.n_groups == a.B == b.B and not torch.equal(a.theta, make_grouped().theta)


def run_one_group_against_shared(make, D, lr):
    """G = 1 against mode='shared' after one Vanilla step: |dtheta_j| <= lr (D - 1) eps sum_d |g_dj| (module docstring)."""
    g, s = make(mode="grouped", demos_per_seed=D), make(mode="shared")
    th0 = g.theta.clone()
    lg, gg = g.step()
    ls, gs = s.step()
    eps = eps_of(g.theta.dtype)
    rows = g.row_grad.double().abs().sum(dim=0)
    bound = lr * (D - 1) * eps * rows
    diff = (g.theta.double() - s.theta.double()).abs()[0]
    print("G = 1 against shared: |dtheta|", diff.cpu().numpy(), "bound", bound.cpu().numpy())
    assert bool((diff <= bound).all()), (diff, bound)
    assert g.theta.shape == s.theta.shape == (1, th0.shape[1]) and bool((g.theta != th0).any())
    assert bool(((gg.double() - gs.double()).abs()[0] <= (D - 1) * eps * rows).all())


def run_frozen(L, D, extra_state):
    """One row of group 0 and every row of group 1 made not ok inside mask_unconverged, after the learner has moved: group 0 sums the
    other rows, group 1 keeps every word of theta and of `extra_state` (names of optimizer / LM state)."""
    L.step()
    L.step()
    G = L.n_groups
    orig = L.mask_unconverged
    bad = torch.zeros(L.B, dtype=torch.bool, device=L.theta.device)
    bad[1] = True
    bad[D:2 * D] = True

    def wrapped(status, loss, grad, stats=None):
        loss, grad = orig(status, loss, grad, stats=stats)
        L._ok = L._ok & ~bad
        nan = torch.full_like(loss, float("nan"))
        return torch.where(bad, nan, loss), torch.where(bad.unsqueeze(1), nan.unsqueeze(1), grad)      # what is left out may be NaN
    L.mask_unconverged = wrapped
    names = ("theta",) + tuple(extra_state)
    before = {nm: getattr(L, nm).clone() for nm in names}
    loss, grad = L.step()
    want = [D - 1, 0] + [D] * (G - 2)
    assert L.n_ok.tolist() == want and L.n_unconverged == D + 1
    rl, rg = L.row_loss, L.row_grad
    keep = [d for d in range(D) if d != 1]
    acc_l, acc_g = torch.zeros_like(rl[0]), torch.zeros_like(rg[0])
    for d in keep:
        acc_l, acc_g = acc_l + rl[d], acc_g + rg[d]
    assert torch.equal(loss[0], acc_l) and torch.equal(grad[0], acc_g) and bool(torch.isfinite(grad[0]).all())
    assert float(loss[1]) == 0.0 and not bool(grad[1].any())
    for nm in names:
        assert torch.equal(getattr(L, nm)[1], before[nm][1]), nm
    for g in [0] + list(range(2, G)):                                                       # (the others went on)
        assert any(not torch.equal(getattr(L, nm)[g], before[nm][g]) for nm in names), g
    L.mask_unconverged = orig
    L.step()
    assert L.n_ok.tolist() == [D] * G and L.n_unconverged == 0
    assert any(not torch.equal(getattr(L, nm)[1], before[nm][1]) for nm in names)           # ... and group 1 is updated again


# "It learns": lm_cases.run_learns' setting (Examples/pendulum_groundtruth.py: waypoints sampled from the solve at the true theta, zero
# residual; its 8 seeds perturbed by +-30 %, numpy default_rng(LMC.LEARN_SEED); fp64, n_grid 10, default LM values, the example's
# learning rate 1e-2 for the Vanilla learner) with D = 3 start states, every group learning from the three demonstrations.  N =
# LEARN_STEPS was fixed on the emulator by that file's rule, a margin of two steps: the conditions also hold at N - 2 (the CPU tier
# checks both).  Observed on the emulator, group loss / initial group loss per seed:
#   LM accepted, N = 12:  4.5e-08 1.6e-04 9.4e-04 2.7e-07 1.2e-04 2.4e-06 7.6e-07 2.1e-02      (N = 10: 1.3e-07 1.7e-04 9.4e-04 7.8e-07 3.5e-04 7.1e-06
#                                                                                              2.2e-06 2.1e-02: 7 of 8 below 1e-3 at either N)
#   Vanilla,     N = 12:  0.080 0.103 0.237 0.019 0.081 0.014 0.014 0.031                      (N = 10: 0.126 0.171 0.378 0.034 0.109 0.026 0.025 0.050)
# (skip_unconverged is on in this mode: the sweeps' tolerance flag leaves some demonstrations out of some steps, group 8 stalls at 2e-2.)
LEARN_STARTS = ((0.0, 0.0), (0.4, 0.0), (-0.3, 0.2))
LEARN_STEPS = 12


def run_learns(make_oc, checkpoints=(LEARN_STEPS,)):
    from lfsd_amd import CPDP
    oc, d = make_oc()
    D = len(LEARN_STARTS)
    true = np.asarray(d["true_theta"], dtype=np.float64)
    taus = np.array([0.1, 0.3, 0.6, 0.7, 0.9]) * d["horizon"]
    x0 = np.asarray(LEARN_STARTS, dtype=np.float64)
    sol = oc.cocSolverBatch(x0, d["horizon"], np.tile(true, (D, 1)))
    wps = oc.sampleBatch(sol, taus)["state"][:, :, d["interface"]].double().cpu().numpy()      # [D, K, 1]
    rng = np.random.default_rng(LMC.LEARN_SEED)
    seeds = true[None, :] * (1.0 + 0.3 * rng.uniform(-1, 1, (8, true.size)))
    args = (x0, d["horizon"], taus, wps, d["interface"], seeds)
    lm = CPDP.SparseDemoLearner(oc, *args, method="LM", mode="grouped", demos_per_seed=D)
    va = CPDP.SparseDemoLearner(oc, *args, method="Vanilla", learning_rate=d["lr"], mode="grouped", demos_per_seed=D)
    assert lm.n_groups == 8 and lm.B == 24
    first = None
    for k in range(max(checkpoints)):
        l, _ = lm.step()
        va.step()
        first = l.clone() if first is None else first
        if k + 1 in checkpoints:
            # the accepted group loss after N steps against the Vanilla learner's group loss at ITS theta after N steps
            lv = va.evaluate(va.theta)[0].clone()
            rel = lm.lm_loss / first
            print("N = %d: LM accepted loss / initial loss" % (k + 1), rel.cpu().numpy())
            print("N = %d: Vanilla loss / initial loss    " % (k + 1), (lv / first).cpu().numpy())
            assert bool((lm.lm_loss <= lv).all()), (k + 1, lm.lm_loss, lv)
            assert int((rel < 1e-3).sum()) >= 4, (k + 1, rel)
