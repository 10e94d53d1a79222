"""Cases of waypoint weights and ragged demonstrations in the fused loss (ABI 16: lfsd_aux_forward_weighted, lfsd_aux_forward_cubic_weighted,
lfsd_normal_matrix_weighted; SparseDemoLearner(waypoint_weights=..., n_waypoints=...)), shared by the CPU tier (kernels through the SIMT
emulator, tests/test_weights_emu.py) and the -m gpu tier (tests/test_weights_gpu.py).

Yardsticks and bounds (eps of the kernel's dtype).
  NULL and ones, zero weights, powers of two: exact (torch.equal).  A weight enters through the scaled residual rs = w r (and H through
    (w x1) x2), one IEEE multiplication that is exact for w = 1 and commutes with every later rounding for w = 2^j; a zero weight skips
    the waypoint before anything of it is read, so the sums are those of the compacted list, added in the same order.
  General weights against an fp64 numpy restatement from the state grid (and, at level 2, the curvature grid) and auxX_grid that the
    SAME call returned -- the interval rule and the extended-precision fraction of lm_cases.interpolant_reference:
      loss      within (K n_iface + 3) eps sum_k w_k |r_k|^2
      gradient  within (K n_iface + n_grid + 6) eps sum_k w_k sum_c |r_kc| (|X_k| + |X_k+1|)      (node values of the waypoint's interval)
      H         within (K n_iface + n_grid + 6) eps sum_k w_k sum_c M M,  M = |X_k| + |X_k+1|      (lm_cases' bound, each term with its w_k)
    The targets are set from the solved trajectory, wp = -y / 2 - sign(y): every residual is at least as large as the value it is
    formed from (|r| = 1.5 |y| + 1), so the roundings of the interpolant are roundings of r and the loss bound is one in |r|^2.
  Oracle (emulator tier): sum_k w_k x (the oracle's loss and gradient for waypoint k alone) at parity_cases' tolerance for the model's
    unweighted loss and gradient in fp64 (loss 1e-6 relative to max(1, loss), gradient 1e-4 of its largest component).
  Learner: identity (torch.equal) with learners built on the compacted waypoint lists, and with the same launches made by hand."""
import contextlib
import ctypes

import numpy as np
import torch

import hyper_sweep_cases as H
import lm_cases as LMC

K = 5
N_GRIDS = (4, 10)
BATCHES = (1, 5, 67)                   # a partial wavefront, a partial lane group
POWERS = (-3, -1, 1, 4)
SKIP_ROW = 2                           # (of batches that have one) forced to a skipped status
F32, F64 = torch.float32, torch.float64
# (model, n_grid, B, dtype, interpolation level): the pendulum (8-lane groups) at every size, precision and level; the quadrotor (fp32:
# 16-lane forward groups, the index interface) and the pendulum seen through a compiled-in interface at the sizes that differ in kind
KERNEL_CASES = [("pendulum", N, B, dt, lvl) for N in N_GRIDS for B in BATCHES for dt in (F32, F64) for lvl in (1, 2)] + \
    [("quadrotor", 4, 5, F32, 1), ("quadrotor", 10, 67, F32, 1), ("quadrotor", 10, 5, F32, 2), ("quadrotor", 4, 1, F64, 1),
     ("quadrotor", 10, 5, F64, 2),
     ("general", 10, 5, F64, 1), ("general", 4, 67, F32, 1), ("general", 10, 1, F32, 2), ("general", 4, 5, F64, 2)]
# the emulator runs every lane as a fiber, and the CPU suite runs for every later change: its tier takes a subset in which every model
# still meets both precisions and both levels, every batch size and both grid sizes (the device tier runs all of KERNEL_CASES)
KERNEL_CASES_EMU = [("pendulum", 4, 1, F32, 1), ("pendulum", 10, 1, F64, 2), ("pendulum", 4, 5, F32, 2), ("pendulum", 4, 5, F64, 1),
                    ("pendulum", 10, 5, F32, 1), ("pendulum", 10, 5, F64, 2), ("pendulum", 4, 67, F32, 1), ("pendulum", 10, 67, F64, 2),
                    ("quadrotor", 4, 5, F32, 1), ("quadrotor", 10, 5, F32, 2), ("quadrotor", 4, 1, F64, 1),
                    ("general", 10, 5, F64, 1), ("general", 10, 1, F32, 2), ("general", 4, 5, F64, 2)]
assert set(KERNEL_CASES_EMU) <= set(KERNEL_CASES)
CASE_ID = lambda c: "%s-N%d-B%d-%s-L%d" % (c[0], c[1], c[2], "fp32" if c[3] == F32 else "fp64", c[4])
PAIRS = [(i, j) for i in range(K) for j in range(i + 1, K)]      # the two slots a row drops: ten choices, by row


def eps_of(dtype):
    return float(torch.finfo(dtype).eps)


def make_model(kind, n_grid):
    """(oc, d, interface_idx or None).  "general": parity_cases' general-interface pendulum, (sin q, q dq) compiled into the library."""
    import sympy as sp
    from lfsd_amd import models
    oc, env, d = models.ZOO["pendulum" if kind == "general" else kind](n_grid=n_grid)
    if kind == "general":
        X = list(oc.state)
        oc.setInterface([sp.sin(X[0]), X[0] * X[1]])
        return oc, d, None
    return oc, d, list(d["interface"])


_SOLVED = {}


def solved(prepare, kind, n_grid, B, dtype):
    """The OC solve of B seeds (theta0 perturbed by +-10 %, horizons by +-10 %), computed once and shared; row SKIP_ROW's status is set
    to FAILED afterwards (B > SKIP_ROW): the sweeps then skip it.  Returns (oc, d, iface, sol)."""
    key = (prepare, kind, n_grid, B, dtype)
    if key not in _SOLVED:
        oc, d, iface = make_model(kind, n_grid)
        prepare(oc, dtype)
        oc.setSolverOptions(aux_rtol=0.0, aux_substeps=4)
        rng = np.random.default_rng(1000 * n_grid + B)
        th0 = np.asarray([1.0, 0.5, 1.5] if kind != "quadrotor" else d["theta0"], dtype=np.float64)
        th = th0[None, :] * (1.0 + 0.1 * rng.uniform(-1, 1, (B, th0.size)))
        hz = float(d["horizon"]) * (1.0 + 0.1 * rng.uniform(-1, 1, B))
        sol = oc.cocSolverBatch(np.tile(np.asarray(d["ini_state"], dtype=np.float64), (B, 1)), hz, th)
        assert set(sol["status"].tolist()) <= {1, 2}, sol["status"]
        if B > SKIP_ROW:
            sol["status"][SKIP_ROW] = 4
        _SOLVED[key] = (oc, d, iface, sol)
    return _SOLVED[key]


def waypoint_times(hz, n_grid, dtype):
    """[B, K] in the dtype: 0, the horizon, a node as the kernel forms it, a point inside an interval, a second one in that interval --
    node and interval move with the row."""
    B = hz.shape[0]
    h = hz / n_grid
    b = torch.arange(B, device=hz.device)
    node = (1 + b % max(1, n_grid - 1)).to(dtype)
    cell = (b % n_grid).to(dtype)
    fa = (0.15 + 0.05 * (b % 7).to(dtype))
    t = torch.stack([torch.zeros_like(hz), hz, (node * h).minimum(hz), (cell + fa) * h, (cell + fa + 0.3) * h], dim=1)
    return t.to(dtype).contiguous()


def interface_values(kind, x):
    """y = g(x) and dg/dx [.., n_iface, n] in numpy for the three models' interfaces (x [.., n])."""
    n = x.shape[-1]
    if kind == "general":
        y = np.stack([np.sin(x[..., 0]), x[..., 0] * x[..., 1]], axis=-1)
        J = np.zeros(x.shape[:-1] + (2, n))
        J[..., 0, 0] = np.cos(x[..., 0])
        J[..., 1, 0], J[..., 1, 1] = x[..., 1], x[..., 0]
        return y, J
    idx = [0] if kind == "pendulum" else list(range(3))
    J = np.zeros(x.shape[:-1] + (len(idx), n))
    for c, i in enumerate(idx):
        J[..., c, i] = 1.0
    return x[..., idx], J


def interval_fraction(hz, taus, n_grid):
    """(k [B, K] int, s [B, K] fp64): h the dtype's quotient, the interval in fp64, the fraction in extended precision (lm_cases)."""
    hz_host = hz.cpu().numpy()
    h = (hz_host / hz_host.dtype.type(n_grid)).astype(np.float64)[:, None]
    t = taus.double().cpu().numpy()
    k = np.clip(np.floor(t / h), 0, n_grid - 1)
    s = ((t.astype(np.longdouble) - k.astype(np.longdouble) * h.astype(np.longdouble)) / h.astype(np.longdouble)).astype(np.float64)
    return k.astype(np.int64), s


def state_at(sol, curv, hz, taus, n_grid):
    """x(tau) [B, K, n] in fp64 on the interpolant of the level (curv: the state curvature grid, or None)."""
    k, s = interval_fraction(hz, taus, n_grid)
    X = sol["state_grid"].double().cpu().numpy()
    b = np.arange(X.shape[0])[:, None]
    s3 = s[:, :, None]
    x = X[b, k] + s3 * (X[b, k + 1] - X[b, k])
    if curv is not None:
        Cv = curv.double().cpu().numpy()
        x = x + ((1 - s3) ** 3 - (1 - s3)) * Cv[b, k] + (s3 ** 3 - s3) * Cv[b, k + 1]
    return x


def targets_far_from(kind, sol, hz, taus, n_grid, dtype, device):
    """wp = -y / 2 - sign(y) on the linear interpolant: |r| >= |y| + 1 whatever the level (module docstring)."""
    y, _ = interface_values(kind, state_at(sol, None, hz, taus, n_grid))
    wp = -0.5 * y - np.where(y < 0, -1.0, 1.0)
    return torch.from_numpy(wp).to(device=device, dtype=dtype).contiguous()


@contextlib.contextmanager
def null_weights(ml, marker):
    """Inside: the binding hands NULL where it would hand `marker`'s address -- the weighted entry points with wp_weight == NULL."""
    orig = ml._p
    ml._p = lambda t: None if t is marker else orig(t)
    try:
        yield
    finally:
        del ml._p


def aux_call(oc, sol, taus, wps, iface, level, weights=None, guard=True):
    """One evaluation with both sensitivity grids, loss / gradient / stats inside guard bands.  Returns the binding's dict."""
    B = sol["state_grid"].shape[0]
    lib, dev = oc.compile(), sol["state_grid"].device
    dt = sol["state_grid"].dtype
    p = lib.n_auxvar
    (loss, b1), (grad, b2) = H.guarded(torch.full((B,), 777.0, dtype=dt, device=dev)), H.guarded(torch.full((B, p), 777.0, dtype=dt, device=dev))
    stats, b3 = H.guarded(torch.full((B, 4), 99, dtype=torch.int32, device=dev))
    kw = {} if weights is None else dict(waypoint_weights=weights)
    out = oc.auxSysSolverBatch(sol, taus, wps, iface, want_grids=True, out=dict(loss=loss, grad=grad, stats=stats), validate=False,
                               skip_status=(4,), interplation_level=level, **kw)
    assert out["loss"].data_ptr() == loss.data_ptr() and all(H.band_intact(b) for b in (b1, b2, b3))
    return out


OUTPUTS = ("loss", "grad", "auxX_grid", "auxU_grid", "stats")


def same_outputs(a, b, rows=None):
    for nm in OUTPUTS:
        x, y = (a[nm], b[nm]) if rows is None else (a[nm][rows], b[nm][rows])
        if not H.same(x, y):
            return nm
    return None


def skipped_rows_are_nan(out, B):
    if B <= SKIP_ROW:
        return True
    r = SKIP_ROW
    ok = bool(torch.isnan(out["loss"][r])) and bool(torch.isnan(out["grad"][r]).all()) and bool(torch.isnan(out["auxX_grid"][r]).all())
    keep = torch.ones(B, dtype=torch.bool, device=out["loss"].device)
    keep[r] = False
    return ok and bool(torch.isfinite(out["loss"][keep]).all()) and bool(torch.isfinite(out["grad"][keep]).all()) and \
        bool(torch.isfinite(out["auxX_grid"][keep]).all())


def normal(oc, out, hz, taus, iface, weights=None):
    """lfsd_normal_matrix[_weighted] of an evaluation's auxX_grid into a guarded H (index interfaces only)."""
    lib = oc.compile()
    aX = out["auxX_grid"]
    B, _, p, _ = aX.shape
    Hm, band = H.guarded(torch.full((B, p, p), 777.0, dtype=aX.dtype, device=aX.device))
    idx = torch.as_tensor(list(iface), dtype=torch.int32, device=aX.device)
    kw = {} if weights is None else dict(wp_weight=weights)
    lib.normal_matrix(hz, taus, aX, idx, out=Hm, **kw)
    assert H.band_intact(band)
    return Hm


def drop_plan(B, device):
    """(keep [B, 3] slots kept, ascending; drop [B, 2]) -- row b drops the pair PAIRS[b % 10]."""
    drop = torch.tensor([PAIRS[b % len(PAIRS)] for b in range(B)], device=device)
    keep = torch.tensor([[k for k in range(K) if k not in PAIRS[b % len(PAIRS)]] for b in range(B)], device=device)
    return keep, drop


def run_kernel_case(prepare, device, case):
    """Tests 1-3 of the issue on one case; returns nothing, asserts."""
    kind, n_grid, B, dtype, level = case
    oc, d, iface, sol = solved(prepare, kind, n_grid, B, dtype)
    lib = oc.compile()
    hz = sol["horizon"]
    taus = waypoint_times(hz, n_grid, dtype)
    wps = targets_far_from(kind, sol, hz, taus, n_grid, dtype, device)
    ones = torch.ones((B, K), dtype=dtype, device=device)
    # 1. NULL and ones
    ref = aux_call(oc, sol, taus, wps, iface, level)
    assert skipped_rows_are_nan(ref, B)
    w1 = aux_call(oc, sol, taus, wps, iface, level, weights=ones)
    assert same_outputs(ref, w1) is None, same_outputs(ref, w1)
    marker = torch.ones((B, K), dtype=dtype, device=device)
    with null_weights(lib, marker):
        w0 = aux_call(oc, sol, taus, wps, iface, level, weights=marker)
    assert same_outputs(ref, w0) is None, same_outputs(ref, w0)
    assert bool((ref["loss"][torch.isfinite(ref["loss"])] > 0).all())
    if iface is not None:
        H0 = normal(oc, ref, hz, taus, iface)
        assert H.same(H0, H0.mT) and H.same(normal(oc, ref, hz, taus, iface, ones), H0)
        with null_weights(lib, marker):
            assert H.same(normal(oc, ref, hz, taus, iface, marker), H0)
    # 2. zero weights are absent waypoints, bit for bit
    keep, drop = drop_plan(B, device)
    wz = torch.zeros((B, K), dtype=dtype, device=device).scatter_(1, keep, 1.0)
    rows = torch.arange(B, device=device)[:, None]
    tz, pz = taus.clone(), wps.clone()
    tz[rows[:, 0], drop[:, 0]], tz[rows[:, 0], drop[:, 1]] = float("nan"), 1e30
    pz[rows[:, 0], drop[:, 0]], pz[rows[:, 0], drop[:, 1]] = 1e30, float("nan")
    t3, p3 = taus[rows, keep].contiguous(), wps[rows, keep].contiguous()
    short = aux_call(oc, sol, t3, p3, iface, level)
    ragged = aux_call(oc, sol, tz, pz, iface, level, weights=wz)
    assert same_outputs(short, ragged) is None, same_outputs(short, ragged)
    assert skipped_rows_are_nan(ragged, B)
    none = aux_call(oc, sol, tz, pz, iface, level, weights=torch.zeros_like(wz))
    live = torch.isfinite(ref["loss"])
    assert bool((none["loss"][live] == 0).all()) and bool((none["grad"][live] == 0).all()) and H.same(none["auxX_grid"], ref["auxX_grid"])
    assert skipped_rows_are_nan(dict(none, auxX_grid=ref["auxX_grid"]), B)
    if iface is not None:
        Hs = normal(oc, short, hz, t3, iface)
        assert H.same(normal(oc, ragged, hz, tz, iface, wz), Hs) and H.same(Hs, Hs.mT)
        Hz = normal(oc, ref, hz, tz, iface, torch.zeros_like(wz))
        assert bool((Hz[live] == 0).all())
    # 3. exact scaling: K = 1 and a weight of 2^j
    t1, p1 = taus[:, 3:4].contiguous(), wps[:, 3:4].contiguous()
    one = aux_call(oc, sol, t1, p1, iface, level)
    H1 = normal(oc, one, hz, t1, iface) if iface is not None else None
    for j in POWERS:
        f = 2.0 ** j
        sc = aux_call(oc, sol, t1, p1, iface, level, weights=torch.full((B, 1), f, dtype=dtype, device=device))
        assert H.same(sc["loss"], one["loss"] * f) and H.same(sc["grad"], one["grad"] * f), j
        if iface is not None:
            assert H.same(normal(oc, one, hz, t1, iface, torch.full((B, 1), f, dtype=dtype, device=device)), H1 * f), j


def general_weights(B, dtype, device, seed=0):
    """[B, K] weights over four decades, none a power of two, one exact zero per row from B = 5 up."""
    g = torch.Generator().manual_seed(4241 * B + seed)
    w = 10.0 ** (4.0 * torch.rand((B, K), generator=g, dtype=torch.float64) - 2.0)
    if B >= 5:
        w[torch.arange(B), torch.arange(B) % K] = 0.0
    return w.to(device=device, dtype=dtype).contiguous()


def run_general_weights(prepare, device, case):
    """Test 4: returns the worst fraction of each bound (loss, grad, H or None); asserts nothing but the set-up."""
    kind, n_grid, B, dtype, level = case
    oc, d, iface, sol = solved(prepare, kind, n_grid, B, dtype)
    hz = sol["horizon"]
    taus = waypoint_times(hz, n_grid, dtype)
    wps = targets_far_from(kind, sol, hz, taus, n_grid, dtype, device)
    w = general_weights(B, dtype, device)
    out = aux_call(oc, sol, taus, wps, iface, level, weights=w)
    live = torch.isfinite(out["loss"]).cpu().numpy()
    eps = eps_of(dtype)
    curv = out["curvature"][0] if level == 2 else None
    y, J = interface_values(kind, state_at(sol, curv, hz, taus, n_grid))                # [B, K, c], [B, K, c, n]
    r = y - wps.double().cpu().numpy()
    w64 = w.double().cpu().numpy()
    ni = r.shape[-1]
    k, s = interval_fraction(hz, taus, n_grid)
    aX = out["auxX_grid"].double().cpu().numpy()                                        # [B, N+1, p, n]
    b = np.arange(B)[:, None]
    xa, xb = aX[b, k], aX[b, k + 1]                                                     # [B, K, p, n]
    Xt = xa + s[:, :, None, None] * (xb - xa)
    M = np.abs(xa) + np.abs(xb)
    loss_ref = np.einsum("bk,bkc->b", w64, r * r)
    loss_bound = (K * ni + 3) * eps * loss_ref
    rJ = np.einsum("bkc,bkcn->bkn", r, J)                                               # r^T dg/dx
    grad_ref = np.einsum("bk,bkn,bkqn->bq", w64, rJ, Xt)
    grad_bound = (K * ni + n_grid + 6) * eps * np.einsum("bk,bkc,bkcn,bkqn->bq", w64, np.abs(r), np.abs(J), M)
    got_l, got_g = out["loss"].double().cpu().numpy(), out["grad"].double().cpu().numpy()
    fl = float((np.abs(got_l - loss_ref)[live] / loss_bound[live]).max())
    fg = float((np.abs(got_g - grad_ref)[live] / grad_bound[live]).max())
    fh = None
    if iface is not None:
        Hm = normal(oc, out, hz, taus, iface, w).double().cpu().numpy()
        assert np.array_equal(Hm[live], np.swapaxes(Hm, 1, 2)[live])
        Xi, Mi = Xt[..., list(iface)], M[..., list(iface)]
        H_ref = np.einsum("bk,bkqc,bkrc->bqr", w64, Xi, Xi)
        H_bound = (K * ni + n_grid + 6) * eps * np.einsum("bk,bkqc,bkrc->bqr", w64, Mi, Mi)
        fh = float((np.abs(Hm - H_ref)[live] / np.maximum(H_bound[live], 1e-300)).max())
    return fl, fg, fh


# ---- entry points: LFSD_EINVAL on host dummies ------------------------------------------------------------------------------------
def weighted_einval(L, n_state, n_control, n_auxvar, compiled_iface):
    """Every LFSD_EINVAL case of the three weighted entry points on host dummies (no launch is reached): those of their siblings, with
    and without a weight array, and H overlapping the weights."""
    buf = (ctypes.c_double * 4096)()
    d = ctypes.cast(buf, ctypes.c_void_p).value
    at = lambda off: ctypes.c_void_p(d + off)
    cd = ctypes.c_double
    names = ("hz", "th", "cs", "X", "U", "Lm", "c1", "c2", "c3", "Z", "idx", "taus", "wps", "w", "loss", "grad")
    base = dict(dtype=1, batch=2, n_grid=3, per=0, nw=2, ni=1, substeps=0, rtol=1e-3, mask=0, st=None,
                **{nm: at(1024 * (i % 4)) for i, nm in enumerate(names)})

    def fwd(cubic, **kw):
        a = dict(base, **kw)
        head = (a["dtype"], a["batch"], a["n_grid"], a["hz"], a["th"], a["cs"], a["per"], a["X"], a["U"], a["Lm"])
        curv = (a["c1"], a["c2"], a["c3"]) if cubic else ()
        tail = (a["Z"], a["nw"], a["ni"], a["idx"], a["taus"], a["wps"], a["w"], a["loss"], a["grad"], None, None, a["substeps"],
                cd(a["rtol"]), None, a["st"], a["mask"], None)
        return (L.lfsd_aux_forward_cubic_weighted if cubic else L.lfsd_aux_forward_weighted)(*head, *curv, *tail)
    bads = [dict(dtype=7), dict(dtype=-1), dict(batch=0), dict(batch=-2), dict(n_grid=0), dict(nw=-1), dict(ni=-1), dict(ni=0), dict(substeps=-1),
            dict(rtol=-1.0), dict(rtol=float("nan")), dict(hz=None), dict(th=None), dict(X=None), dict(U=None), dict(Lm=None), dict(Z=None),
            dict(loss=None), dict(grad=None), dict(taus=None), dict(wps=None), dict(mask=-1), dict(mask=16)]
    if not compiled_iface:
        bads.append(dict(idx=None))
    for cubic in (False, True):
        for bad in bads:
            for w in (base["w"], None):
                assert fwd(cubic, **dict(dict(w=w), **bad)) == -1, (cubic, bad, w)
    for bad in (dict(c1=None), dict(c2=None), dict(c3=None), dict(n_grid=2)):
        assert fwd(True, **bad) == -1, bad
    # lfsd_normal_matrix_weighted: lm_cases' layout, the weights (32 B) at 192
    nb = dict(dtype=1, batch=2, n_grid=3, n_state=2, n_param=2, K=2, ni=1, idx=at(0), hz=at(64), taus=at(128), w=at(192), aX=at(256), H=at(1024))
    call = lambda **kw: (lambda a: L.lfsd_normal_matrix_weighted(a["dtype"], a["batch"], a["n_grid"], a["n_state"], a["n_param"], a["K"], a["ni"],
                                                                 a["idx"], a["hz"], a["taus"], a["w"], a["aX"], a["H"], None))(dict(nb, **kw))
    bads = [dict(dtype=7), dict(dtype=-1), dict(batch=0), dict(batch=-3), dict(n_grid=0), dict(n_state=0), dict(n_param=0), dict(K=0),
            dict(ni=0), dict(idx=None), dict(hz=None), dict(taus=None), dict(aX=None), dict(H=None),
            dict(H=at(0)), dict(H=at(64 + 8)), dict(H=at(128 - 8)), dict(H=at(128 + 24)), dict(H=at(256 + 248)), dict(H=at(256 - 56)),
            dict(batch=2 ** 31 - 1, n_grid=1, n_state=1, n_param=17, K=1, idx=ctypes.c_void_p(1 << 36), hz=ctypes.c_void_p(1 << 40),
                 taus=ctypes.c_void_p(1 << 41), w=ctypes.c_void_p(1 << 42), aX=ctypes.c_void_p(1 << 44), H=ctypes.c_void_p((1 << 44) + (1 << 43)))]
    for bad in bads:
        for w in ((nb["w"], None) if "w" not in bad else (bad["w"],)):
            assert call(**dict(dict(w=w), **bad)) == -1, (bad, w)
    assert call(H=at(192 + 24)) == -1 and call(H=at(192 - 56)) == -1                       # H overlapping the weights


# ---- the learner ----------------------------------------------------------------------------------------------------------------
COUNTS = (5, 3, 1)
STEPS = 6
RULES = (("Vanilla", dict(method="Vanilla", learning_rate=1e-2)), ("Nesterov", dict(method="Nesterov", learning_rate=1e-2, mu=0.9)),
         ("LM", dict(method="LM")))


def learner_problem(prepare, kind, rows, dtype, n_grid=10):
    """(oc, args, lambda0): `rows` seeds of lm_cases' composition cases with K = 5 waypoints (times and targets spread over the horizon;
    the targets far from the trajectories, as lm_cases' are).  Fixed sub-stepping, as group_cases: a row is frozen only where a case
    means it to be."""
    oc, d, iface = make_model(kind, n_grid)
    prepare(oc, dtype)
    oc.setSolverOptions(aux_rtol=0.0, aux_substeps=8)
    seeds = LMC.compose_seeds(d["theta0"], rows)
    hz = float(d["horizon"])
    if kind == "pendulum":
        taus, wps = np.array([0.15, 0.35, 0.5, 0.7, 0.9]) * hz, np.array([[0.3], [0.9], [1.5], [2.1], [2.7]])
    else:                                  # (lm_cases' quadrotor case: the model's own five waypoints, for which its lambda0 was chosen)
        taus, wps = np.asarray(d["taus"], dtype=np.float64), np.asarray(d["waypoints"], dtype=np.float64)
    args = (np.tile(np.asarray(d["ini_state"], dtype=np.float64), (rows, 1)), hz, taus, wps, iface, seeds)
    return oc, args, LMC.COMPOSE_LAMBDA0[kind]


def state_of(L):
    out = dict(theta=L.theta.clone())
    if L.lm_lambda is not None:
        out.update(trial=L.theta_trial.clone(), lam=L.lm_lambda.clone(), lm_loss=L.lm_loss.clone(), Hm=L.normal_matrix.clone())
    return out


def run_ragged_independent(make, rows, rule, lambda0):
    """6a: rows with n_waypoints = 5, 3, 1 (cycling) inside one K = 5 learner against three learners built with K = 5, 3, 1 on the same
    seeds: theta, loss and gradient traces, bit for bit.  `make(rows=index list, k=waypoints kept or None, **kw)`."""
    name, kw = rule
    kw = dict(kw, **(dict(lm_lambda0=lambda0) if name == "LM" else {}))
    counts = [COUNTS[b % 3] for b in range(rows)]
    L = make(rows=list(range(rows)), n_waypoints=counts, trace=STEPS, **kw)
    assert L.wts is not None and L.wts.sum(dim=1).tolist() == [float(c) for c in counts]
    hist = []
    for _ in range(STEPS):
        loss, grad = L.step()
        hist.append((loss.clone(), grad.clone(), state_of(L)))
    moved = False
    for c in COUNTS:
        sel = [b for b in range(rows) if counts[b] == c]
        S = make(rows=sel, k=c, trace=STEPS, **kw)
        assert S.wts is None and S.taus.shape[1] == c
        for k in range(STEPS):
            loss, grad = S.step()
            # (H.same: torch.equal away from the NaNs and the NaNs in the same places -- an LM step may throw a row far out)
            assert H.same(loss, hist[k][0][sel]) and H.same(grad, hist[k][1][sel]), (c, k)
            for nm, v in state_of(S).items():
                assert H.same(v, hist[k][2][nm][sel]), (c, k, nm)
        assert H.same(S.loss_trace, L.loss_trace[sel]) and H.same(S.theta_trace, L.theta_trace[sel]) and \
            H.same(S.grad_norm_trace, L.grad_norm_trace[sel])
        moved = moved or bool((S.theta_trace[:, -1] != S.theta_trace[:, 0]).any())
    assert moved and bool(torch.isfinite(L.loss_trace[:, 0]).all())
    if name == "LM":
        acc = torch.stack([h[2]["lm_loss"] for h in hist])
        assert bool((acc[1:] < acc[:-1]).any()) and bool((torch.stack([h[2]["lam"] for h in hist])[1:] > hist[0][2]["lam"]).any()), \
            "steps are accepted and rejected"
    return L


def grouped_by_hand(oc, args, G, D, wts, steps, proj_lo, lr):
    """6b, a Vanilla rule: expand, solve, weighted sweeps, lfsd_group_reduce, update -- the launches of the grouped learner."""
    import group_cases as GC
    lib = oc.compile()
    x0, hz, taus, wps = GC.tiled(oc, args, G, D)
    th = oc._t(args[5]).contiguous().clone()
    B, p, dev, dt = G * D, th.shape[1], th.device, th.dtype
    w = oc._t(wts).repeat(G, 1).contiguous()
    gidx = (torch.arange(B, dtype=torch.int32, device=dev) // D).contiguous()
    z = lambda: torch.zeros_like(th)
    m, v, vhat = z(), z(), z()
    prev = None
    for it in range(steps):
        rows_th = lib.gather_rows(gidx, th.contiguous(), torch.empty((B, p), dtype=dt, device=dev), B)
        u_init = None
        if prev is not None:
            cont = (prev["status"] == 3).reshape(-1, 1, 1)
            pu = prev["control_grid"][:, :-1]
            u_init = torch.where(cont & torch.isfinite(pu), pu, torch.zeros_like(pu)).contiguous()
        sol = prev = oc.cocSolverBatch(x0, hz, rows_th, consts=oc.consts_tensor(), u_init=u_init)
        aux = oc.auxSysSolverBatch(sol, taus, wps, args[4], validate=False, skip_status=(3, 4), waypoint_weights=w)
        loss, grad = aux["loss"].to(dt), aux["grad"].to(dt)
        st = sol["status"]
        ok = ((st == 1) | (st == 2)) & torch.isfinite(loss) & torch.isfinite(grad).all(dim=1) & ((aux["stats"][:, 1] + aux["stats"][:, 3]) == 0)
        grad = torch.where(ok.unsqueeze(1), grad, torch.zeros_like(grad))
        lg, gg, _, n_ok = lib.group_reduce(loss.contiguous(), grad.contiguous(), D, row_ok=ok.to(torch.int32))
        lib.optimizer_step("Vanilla", th, gg, it, lr, 0.9, 0.9, 0.999, 1e-8, m=m, v=v, vhat=vhat, proj_lo=proj_lo,
                           row_active=(n_ok > 0).to(torch.int32))
        yield th.clone(), lg.clone(), gg.clone(), n_ok.clone()


def ragged_lists(args):
    """Demonstrations of 5, 3 and 1 waypoints as Python lists (the first, the middle three, the last of `args`' five)."""
    taus, wps = np.asarray(args[2]), np.asarray(args[3])
    return [taus.tolist(), taus[1:4].tolist(), taus[4:].tolist()], [wps.tolist(), wps[1:4].tolist(), wps[4:].tolist()]


def launch_spy(ml, monkeypatch):
    """Counts the binding's calls and makes the three weighted entry points raise: a learner without weights must not reach them."""
    calls = {}
    for name in ("normal_matrix", "lm_step", "optimizer_step", "optimizer_step_rows", "aux_solve", "group_reduce"):
        def wrapped(*a, _fn=getattr(ml, name), _name=name, **kw):
            assert kw.get("wp_weight") is None, _name
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(*a, **kw)
        monkeypatch.setattr(ml, name, wrapped)

    def refuse(*a):
        raise AssertionError("a weighted entry point was called")
    for sym in ("lfsd_aux_forward_weighted", "lfsd_aux_forward_cubic_weighted", "lfsd_normal_matrix_weighted"):
        monkeypatch.setattr(ml.lib, sym, refuse)
    return calls
