"""Cases of the Levenberg-Marquardt step over parameters and waypoint times (ABI 18: lfsd_time_normal_blocks, lfsd_lm_step_times;
SparseDemoLearner(method="LM", lm_taus=True)), shared by the CPU tier (kernels through the SIMT emulator, tests/test_lm_times_emu.py)
and the -m gpu tier (tests/test_lm_times_gpu.py).

Yardsticks and bounds (eps of the kernel's dtype, N = n_grid, C = n_iface, Y = max |node value| of the state grid of the row).
  lfsd_time_normal_blocks: an fp64 numpy restatement on the kernel's own rounded arrays.  The interval is formed as the kernel forms it
    (h = horizon / N and k = floor(tau / h) in the arrays' type: the slope jumps at a node), the fraction in extended precision
    (tests/tau_cases.py: interval_of).  At level 2 the slope is the derivative of scipy's not-a-knot CubicSpline of the state grid.
    Per interface component c the kernel multiplies a slope t with an interpolant x of the sensitivity grid:
      the slope carries ds (tests/tau_cases.py, section 17):  linear 2 eps |d| / h with d = x_b - x_a of the STATE grid; cubic
        (2 |d| + 400 Y + 12 Y (6 (N / 2 + 2) + 6)) eps / h;
      the interpolant carries dx = (N / 2 + 2.5) eps M, M = |X_a| + |X_b| of the SENSITIVITY grid (tests/lm_cases.py, section 14: the
        bound in the node values, valid for sensitivities of any sign);
      the product of the two perturbed factors is off by ds |x| + |t| dx + ds dx; forming (w t), the product and the sum of C terms add
      one rounding per operation: (C + 3) eps sum |w t| |x| covers the weight's product, the product, the C - 1 additions and the
      rounding of the result with one to spare.
        |C_kq - ref| <= sum_c w (ds |x| + |t| dx + ds dx) + (C + 3) eps sum_c |w t| |x|
        |d_k  - ref| <= sum_c w (2 |t| ds + ds ds)       + (C + 3) eps sum_c w t t                    (x replaced by t itself)
  The arrow identity: the matrix [[H, C^T], [C, diag d]] assembled from lfsd_normal_matrix and the two outputs against J_aug^T W J_aug of
    the restatement (J_aug: the columns of theta, then one column per waypoint holding t_k in that waypoint's rows), block by block
    within the bounds above and (K C + N + 6) eps sum M M of tests/lm_cases.py for H; [grad; gtau] = J_aug^T W r with lfsd_waypoint_vjp
    (bound (K C + N + 6) eps sum M |w r|) and lfsd_waypoint_time_grad (the bound of tests/tau_cases.py).
  lfsd_lm_step_times: copies and untouched words bit for bit; lambda the value the same multiplications give in the dtype; with all-zero
    C and d the bits of lfsd_lm_step; the solve by the backward error of the FULL damped arrow system
      A = [[H + lambda (diag H + floor I), C^T], [C, diag D]],  |A z + g|_inf <= 8 n eps (|A|_inf |z|_inf + |g|_inf),  n = p + D K
    (section 14's bound with the full dimension; z is read exactly from a run with theta = 0, no projection).  The same elimination
    written in numpy in the dtype is held to the same bound first (run_lm_step_times asserts it before it looks at the kernel).
  Learner: identity with the same launches made by hand; recovery against a numpy loop (below)."""
import ctypes

import numpy as np
import torch

import hyper_sweep_cases as H
import lm_cases as LC
import tau_cases as TC

SHAPES = ((1, 1, 1), (67, 12, 5), (130, 7, 5), (4099, 7, 5))      # (B, p, K); 130 crosses a 64-lane workgroup with a partial last one
GROUPS = ((1, 3, 7, 4), (33, 3, 7, 4), (65, 2, 16, 1))            # (G, D, p, K)
N_GRIDS = (1, 3, 10)
N_STATE = LC.N_STATE
IFACE = LC.IFACE
LM = LC.LM
KINDS = LC.KINDS

eps_of = LC.eps_of


# ---- lfsd_time_normal_blocks ---------------------------------------------------------------------------------------------------------
def block_inputs(B, p, n_grid, K, dtype, device, seed=0):
    """(hz, taus, state grid X, sensitivity grid aX, targets wp, idx): tau at 0, at the horizon, on nodes and inside intervals
    (tests/lm_cases.py: normal_inputs, sign-changing sensitivities), scattered interface indices."""
    hz, taus, aX, r, idx = LC.normal_inputs(B, p, n_grid, K, dtype, device, seed=seed + 2, general=True)
    g = torch.Generator().manual_seed(31 * B + 7 * p + n_grid + K + seed)
    X = torch.randn((B, n_grid + 1, N_STATE), generator=g, dtype=torch.float64).to(device=device, dtype=dtype).contiguous()
    wp = torch.randn((B, K, len(IFACE)), generator=g, dtype=torch.float64).to(device=device, dtype=dtype).contiguous()
    return hz, taus, X, aX, wp, idx


def blocks_reference(hz, taus, X, aX, n_grid, w=None, cubic=False):
    """fp64: J [B, K, p, C], t [B, K, C], x(tau) [B, K, C], C_ref [B, K, p], d_ref [B, K] and their bounds (module docstring), M of J."""
    eps = eps_of(X.dtype)
    k, s, h = TC.interval_of(hz, taus, n_grid)
    with np.errstate(invalid="ignore"):
        s = np.where(np.isfinite(s), s, 0.0)
    X64, A64 = X.double().cpu().numpy(), aX.double().cpu().numpy()[:, :, :, list(IFACE)]
    Y = np.abs(X64).max(axis=(1, 2))[:, None, None]
    b = np.arange(X64.shape[0])[:, None]
    xa, xb = X64[b, k][:, :, list(IFACE)], X64[b, k + 1][:, :, list(IFACE)]
    d = xb - xa
    s3, h3 = s[:, :, None], h[:, :, None]
    N, C = n_grid, len(IFACE)
    if not cubic:
        xv, t = xa + s3 * d, d / h3
        ds = 2 * eps * np.abs(d) / h3
    else:
        from scipy.interpolate import CubicSpline
        cs = CubicSpline(np.arange(N + 1, dtype=np.float64), X64, axis=1, bc_type="not-a-knot")
        c, dc = cs.c, cs.derivative().c
        ci = lambda a, m: a[m][k, b][:, :, list(IFACE)]
        xv = ((ci(c, 0) * s3 + ci(c, 1)) * s3 + ci(c, 2)) * s3 + ci(c, 3)
        t = ((ci(dc, 0) * s3 + ci(dc, 1)) * s3 + ci(dc, 2)) / h3
        ds = (2 * np.abs(d) + 400 * Y + 12 * Y * (6 * (N / 2 + 2) + 6)) * eps / h3
    Ja, Jb = A64[b, k], A64[b, k + 1]                                    # [B, K, p, C]
    J = Ja + s[:, :, None, None] * (Jb - Ja)
    M = np.abs(Ja) + np.abs(Jb)
    dx = (N / 2 + 2.5) * eps * M
    wk = np.ones(taus.shape) if w is None else w.double().cpu().numpy()
    w3, w4 = wk[:, :, None], wk[:, :, None, None]
    t4, ds4 = t[:, :, None, :], ds[:, :, None, :]
    Cref = (w4 * t4 * J).sum(-1)
    Cb = (w4 * (ds4 * np.abs(J) + np.abs(t4) * dx + ds4 * dx)).sum(-1) + (C + 3) * eps * (w4 * np.abs(t4) * np.abs(J)).sum(-1)
    dref = (w3 * t * t).sum(-1)
    db = (w3 * (2 * np.abs(t) * ds + ds * ds)).sum(-1) + (C + 3) * eps * (w3 * t * t).sum(-1)
    return dict(J=J, t=t, x=xv, C=Cref, Cb=Cb, d=dref, db=db, M=M, w=wk)


def _ratio(got, ref, bound):
    err = np.abs(got.double().cpu().numpy() - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(q.max())


def run_time_blocks(lib, device, dtype, B, p, K, n_grid, cubic):
    """Worst fraction of the bound over C and d of one shape; asserts the exact properties on the way."""
    hz, taus, X, aX, wp, idx = block_inputs(B, p, n_grid, K, dtype, device)
    curv = lib.grid_curvature(X) if cubic else None
    call = lambda **kw: lib.time_normal_blocks(kw.pop("X", X), kw.pop("hz", hz), kw.pop("taus", taus), kw.pop("aX", aX),
                                               kw.pop("idx", idx), curv=kw.pop("curv", curv), **kw)
    oC, bandC = H.guarded(torch.zeros((B, K, p), dtype=dtype, device=device))
    od, bandd = H.guarded(torch.zeros((B, K), dtype=dtype, device=device))
    rC, rd = call(out=(oC, od))
    assert rC.data_ptr() == oC.data_ptr() and rd.data_ptr() == od.data_ptr() and H.band_intact(bandC) and H.band_intact(bandd)
    assert bool(torch.isfinite(oC).all()) and bool(torch.isfinite(od).all()) and bool((od >= 0).all())
    ref = blocks_reference(hz, taus, X, aX, n_grid, cubic=cubic)
    worst = max(_ratio(oC, ref["C"], ref["Cb"]), _ratio(od, ref["d"], ref["db"]))
    # weights: all ones give the bits of none; powers of two scale exactly; against the restatement
    ones = torch.ones_like(taus)
    C1, d1 = call(wp_weight=ones)
    assert torch.equal(C1, oC) and torch.equal(d1, od)
    pw = torch.tensor([1.0, 0.25, 4.0], dtype=dtype, device=device)[torch.arange(B * K, device=device).reshape(B, K) % 3].contiguous()
    Cw, dw = call(wp_weight=pw)
    assert torch.equal(Cw, oC * pw[:, :, None]) and torch.equal(dw, od * pw)
    wr = (0.5 + torch.rand((B, K), generator=torch.Generator().manual_seed(B + K), dtype=torch.float64)).to(device=device, dtype=dtype).contiguous()
    Cr, dr = call(wp_weight=wr)
    refw = blocks_reference(hz, taus, X, aX, n_grid, w=wr, cubic=cubic)
    worst = max(worst, _ratio(Cr, refw["C"], refw["Cb"]), _ratio(dr, refw["d"], refw["db"]))
    # a zero-weight waypoint with a NaN tau: +0.0, and nothing of it is read; the others keep their bits
    gone = (torch.arange(B * K, device=device).reshape(B, K) % 3) == 1
    w0, t0 = ones.clone(), taus.clone()
    w0[gone], t0[gone] = 0.0, float("nan")
    C0, d0 = call(taus=t0, wp_weight=w0)
    assert not bool(torch.isnan(C0).any()) and not bool(torch.isnan(d0).any())
    assert torch.equal(C0[~gone], oC[~gone]) and torch.equal(d0[~gone], od[~gone])
    assert bool((C0[gone] == 0).all()) and bool((d0[gone] == 0).all())
    assert not bool(torch.signbit(C0[gone]).any()) and not bool(torch.signbit(d0[gone]).any())
    # a NaN row (state and sensitivity grids) poisons its own row and no other
    at = B // 2
    X2, aX2 = X.clone(), aX.clone()
    X2[at], aX2[at] = float("nan"), float("nan")
    C2, d2 = call(X=X2, aX=aX2, curv=lib.grid_curvature(X2) if cubic else None)
    keep = torch.ones(B, dtype=torch.bool, device=device)
    keep[at] = False
    assert bool(torch.isnan(C2[at]).all()) and bool(torch.isnan(d2[at]).all()) and torch.equal(C2[keep], oC[keep]) and torch.equal(d2[keep], od[keep])
    # permuting the rows permutes the bits; a row alone gives its bits
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(B + p)).to(device)
    pc = lambda t: None if t is None else t[perm].contiguous()
    Cp, dp = call(X=pc(X), hz=pc(hz), taus=pc(taus), aX=pc(aX), curv=pc(curv))
    assert torch.equal(Cp, oC[perm]) and torch.equal(dp, od[perm])
    one = lambda t: None if t is None else t[at:at + 1].contiguous()
    Co, do = call(X=one(X), hz=one(hz), taus=one(taus), aX=one(aX), curv=one(curv))
    assert torch.equal(Co[0], oC[at]) and torch.equal(do[0], od[at])
    # an interface index outside [0, n_state): found on the device, nothing is written
    for bad in ((1, N_STATE, 11), (-1, 6, 11)):
        o2, b2 = H.guarded(torch.full((B, K, p), 777.0, dtype=dtype, device=device))
        o3, b3 = H.guarded(torch.full((B, K), 777.0, dtype=dtype, device=device))
        call(idx=torch.tensor(bad, dtype=torch.int32, device=device), out=(o2, o3))
        assert H.band_intact(b2) and H.band_intact(b3) and bool((o2 == 777.0).all()) and bool((o3 == 777.0).all()), bad
    return worst


def run_arrow_identity(lib, device, dtype, B, p, K, n_grid, cubic, tg_lib=None):
    """[[H, C^T], [C, diag d]] = J_aug^T W J_aug and [grad; gtau] = J_aug^T W r, block by block within the summed bounds; returns the
    worst fraction.  `tg_lib`: a library of a model with N_STATE states (lfsd_waypoint_time_grad is the one call here that lives in the
    model library)."""
    eps, ni = eps_of(dtype), len(IFACE)
    hz, taus, X, aX, wp, idx = block_inputs(B, p, n_grid, K, dtype, device, seed=5)
    curv = lib.grid_curvature(X) if cubic else None
    w = torch.tensor([1.0, 0.5, 2.0], dtype=dtype, device=device)[torch.arange(B * K, device=device).reshape(B, K) % 3].contiguous()
    Cd, dd = lib.time_normal_blocks(X, hz, taus, aX, idx, curv=curv, wp_weight=w)
    Hd = lib.normal_matrix(hz, taus, aX, idx, wp_weight=w)
    ref = blocks_reference(hz, taus, X, aX, n_grid, w=w, cubic=cubic)
    J, t, wk, M = ref["J"], ref["t"], ref["w"], ref["M"]
    # J_aug of a row: K C residual rows, p + K columns
    Ja = np.zeros((B, K, ni, p + K))
    Ja[:, :, :, :p] = np.transpose(J, (0, 1, 3, 2))
    for k in range(K):
        Ja[:, k, :, p + k] = t[:, k]
    A = np.einsum("bkcu,bk,bkcv->buv", Ja, wk, Ja)
    worst = _ratio(Hd, A[:, :p, :p], (K * ni + n_grid + 6) * eps * np.einsum("bkqc,bk,bkrc->bqr", M, wk, M))
    worst = max(worst, _ratio(Cd, A[:, p:, :p], ref["Cb"]), _ratio(dd, np.einsum("bkk->bk", A[:, p:, p:]), ref["db"]))
    off = A[:, p:, p:] - np.einsum("bk,kj->bkj", np.einsum("bkk->bk", A[:, p:, p:]), np.eye(K))
    assert not off.any()                                   # the time block IS diagonal: a time enters its own waypoint only
    # right-hand side: r = x(tau) - wp of the restatement, rounded to the dtype, handed to the device as the residual
    r = torch.from_numpy(ref["x"]).to(device) - wp.double()
    r_dev = r.to(dtype)
    rx = torch.zeros((B, K, N_STATE), dtype=dtype, device=device)
    rx[:, :, list(IFACE)] = (w[:, :, None] * r_dev)        # (powers of two: exact)
    g = lib.waypoint_vjp(hz, taus, rx, aX)
    r64 = (w[:, :, None] * r_dev).double().cpu().numpy()
    rhs = np.einsum("bkcu,bkc->bu", Ja, r64)
    worst = max(worst, _ratio(g, rhs[:, :p], (K * ni + n_grid + 6) * eps * np.einsum("bkqc,bkc->bq", M, np.abs(r64))))
    gt = (tg_lib or lib).waypoint_time_grad(X, hz, taus, wp, idx, curv=curv, wp_weight=w)
    gref, gb = TC.time_grad_reference(hz, taus, X, wp, n_grid, w=w, cubic=cubic)
    assert np.allclose(gref, np.einsum("bkcu,bkc->bu", Ja, wk[:, :, None] * r.cpu().numpy())[:, p:], rtol=1e-9, atol=1e-12)
    return max(worst, _ratio(gt, gref, gb))


def time_blocks_einval(L):
    """Every LFSD_EINVAL case of lfsd_time_normal_blocks on host dummies (no launch is reached)."""
    buf = (ctypes.c_double * 4096)()
    base_addr = ctypes.cast(buf, ctypes.c_void_p).value
    at = lambda off: ctypes.c_void_p(base_addr + off)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.lfsd_time_normal_blocks.argtypes = [ci] * 7 + [vp] * 10
    # B = 2, n_grid = 3, n = 2, p = 2, K = 2, n_iface = 1, fp64: idx 4 B, hz 16 B, taus / w 32 B, X / curv 128 B, aX 256 B, C 64 B, d 32 B
    base = dict(dtype=1, batch=2, n_grid=3, n=2, p=2, K=2, ni=1, idx=at(0), hz=at(64), taus=at(128), w=None, X=at(512), curv=None,
                aX=at(1024), C=at(2048), d=at(3072))
    call = lambda **kw: (lambda a: L.lfsd_time_normal_blocks(a["dtype"], a["batch"], a["n_grid"], a["n"], a["p"], a["K"], a["ni"], a["idx"],
                                                             a["hz"], a["taus"], a["w"], a["X"], a["curv"], a["aX"], a["C"], a["d"],
                                                             None))(dict(base, **kw))
    far = lambda i: vp(1 << (36 + i))
    bads = [dict(dtype=7), dict(dtype=-1), dict(batch=0), dict(batch=-3), dict(n_grid=0), dict(n=0), dict(p=0), dict(K=0), dict(ni=0),
            dict(idx=None), dict(hz=None), dict(taus=None), dict(X=None), dict(aX=None), dict(C=None), dict(d=None),
            dict(curv=at(768), n_grid=2),                                                  # the cubic interpolant needs four nodes
            dict(C=at(0)), dict(C=at(64 + 8)), dict(C=at(128 - 8)), dict(C=at(512 + 120)), dict(C=at(1024 + 248)), dict(C=at(3072 - 8)),
            dict(d=at(128 + 24)), dict(d=at(512 - 8)), dict(d=at(1024)), dict(d=at(2048 + 56)), dict(w=at(2048)), dict(curv=at(3072 - 120)),
            # more than 2^31-1 workgroups (addresses far apart: nothing overlaps, nothing is dereferenced)
            dict(batch=2 ** 31 - 1, n_grid=1, n=1, p=16, K=64, idx=far(0), hz=far(4), taus=far(8), X=far(12), aX=far(16), C=far(20), d=far(24))]
    for bad in bads:
        assert call(**bad) == -1, bad


# ---- lfsd_lm_step_times ------------------------------------------------------------------------------------------------------------
# Group g has the row kind of tests/lm_cases.py (kind (g + offset) % 10, the `big` variant every other decade); its D rows and their K
# waypoints carry a Jacobian of their own: per waypoint J_k [C x p], t_k [C], H += sum w J^T J, c_k = w J^T t, d_k = w t^T t, so the arrow
# matrix stays a Gram matrix.  Kinds 6-9 are statements about H alone (zero / indefinite / zero row / diagonal): their rows carry zero
# blocks at both points.  On top, cycling with the group index:
#   extra 1  a waypoint with d = 0 (and c = 0) at both points            extra 2  a row with ok_acc = 0 (and row_ok = 0) inside the group
#   extra 3  no counted row at all (ok_acc = row_ok = 0 for every row)   extra 4  a NaN in C_t of a counted row: rejected
#   extra 5  a NaN in C_t of an uncounted row: ignored                   extra 0  nothing
def lmt_state(G, D, p, K, dtype, device, offset=0, seed=0, zero_blocks=False):
    st, kind, big = LC.lm_state(G, p, dtype, device, offset, seed)
    B = G * D
    rng = np.random.default_rng(977 * G + 31 * D + 7 * p + K + seed)
    ni = 3
    extra = (np.arange(G) + offset) % 6
    plain = ~np.isin(kind, (6, 7, 8, 9))
    w = np.where(rng.random((B, K)) < 0.2, 0.0, rng.choice([1.0, 0.5, 2.0], (B, K)))
    w[::2, 0] = 1.0
    out = {}
    Hadd = {}
    ok_acc, row_ok = np.ones(B, dtype=np.int32), np.ones(B, dtype=np.int32)
    for which in ("acc", "t"):
        J = rng.standard_normal((B, K, ni, p)) * 10.0 ** (2.0 * rng.random((B, 1, 1, p)) - 1.0)
        t = rng.standard_normal((B, K, ni)) * 10.0 ** (2.0 * rng.random((B, K, 1)) - 1.0)
        for g in range(G):
            rows = slice(g * D, (g + 1) * D)
            if not plain[g] or zero_blocks:
                J[rows], t[rows] = 0.0, 0.0
            if extra[g] == 1:
                t[g * D, K - 1] = 0.0
        out["C_" + which] = np.einsum("bk,bkcq,bkc->bkq", w, J, t)
        out["d_" + which] = np.einsum("bk,bkc,bkc->bk", w, t, t)
        out["gtau_" + which] = rng.standard_normal((B, K)) * (out["d_" + which] > 0)
        Hadd[which] = np.einsum("bk,bkcq,bkcr->bqr", w, J, J)
    for g in range(G):
        if extra[g] in (2, 5) and D > 1:
            ok_acc[g * D + 1] = row_ok[g * D + 1] = 0
        if extra[g] == 3:
            ok_acc[g * D:(g + 1) * D] = row_ok[g * D:(g + 1) * D] = 0
    for which, oks in (("acc", ok_acc), ("t", row_ok)):                # H of a group: its counted rows' Gram matrices on top
        add = (Hadd[which] * oks[:, None, None]).reshape(G, D, p, p).sum(1)
        key = "H_acc" if which == "acc" else "H_t"
        base = st[key].double().cpu().numpy()
        first = kind == 0 if which == "acc" else np.zeros(G, dtype=bool)
        st[key] = torch.from_numpy(np.where(first[:, None, None], base, base + add)).to(device=device, dtype=dtype).contiguous()
    nan_reject = np.zeros(G, dtype=bool)
    for g in range(G):
        if extra[g] == 4 and plain[g] and not zero_blocks:      # (a NaN is no zero block: the sibling would accept)
            out["C_t"][g * D + D - 1, 0, p - 1] = np.nan
            w[g * D + D - 1, 0] = 1.0
            nan_reject[g] = True
        if extra[g] == 5 and D > 1:
            out["C_t"][g * D + 1, :, :] = np.nan
            out["gtau_t"][g * D + 1, 0] = np.inf
    for g in np.nonzero(kind == 0)[0]:                                 # nothing accepted yet: the accepted blocks are still zero
        rows = slice(g * D, (g + 1) * D)
        out["C_acc"][rows], out["d_acc"][rows], out["gtau_acc"][rows], ok_acc[rows] = 0.0, 0.0, 0.0, 0
    hz = 1.0 + rng.random(B)
    tau = np.sort(rng.random((B, K)), axis=1) * hz[:, None]
    trial = np.sort(rng.random((B, K)), axis=1) * hz[:, None]
    tau[w == 0], trial[w == 0] = np.nan, np.nan                        # (NaN padding of the waypoints that do not exist)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype).contiguous()
    st.update({k: to(v) for k, v in out.items()})
    st.update(tau=to(tau), tau_trial=to(trial), w=to(w), ok_acc=torch.from_numpy(ok_acc).to(device), row_ok=torch.from_numpy(row_ok).to(device))
    return st, kind, big, extra, nan_reject


STATE = ("theta", "loss_acc", "grad_acc", "H_acc", "lam", "trial", "tau", "tau_trial", "gtau_acc", "C_acc", "d_acc", "ok_acc")


def lmt_call(lib, st, D, proj_lo=None, use_active=True, use_w=True):
    """lfsd_lm_step_times on guarded copies of the state; returns the state after the call (+ accepted)."""
    v, bands = {}, []
    for nm in STATE:
        v[nm], band = H.guarded(st[nm])
        bands.append(band)
    acc, band = H.guarded(torch.full((st["lam"].shape[0],), 99, dtype=torch.int32, device=st["lam"].device))
    bands.append(band)
    lib.lm_step_times(v["theta"], v["loss_acc"], v["grad_acc"], v["H_acc"], v["lam"], v["trial"], v["tau"], v["tau_trial"], v["gtau_acc"],
                      v["C_acc"], v["d_acc"], v["ok_acc"], st["loss_t"], st["grad_t"], st["H_t"], st["gtau_t"], st["C_t"], st["d_t"],
                      group_size=D, row_ok=st["row_ok"], wp_weight=st["w"] if use_w else None, proj_lo=proj_lo,
                      group_active=st["active"] if use_active else None, accepted=acc, **LM)
    assert all(H.band_intact(b) for b in bands)
    return dict(v, accepted=acc)


def numpy_elimination(Hm, gv, C, d, gt, lam, dtype):
    """The kernel's elimination in numpy, in the dtype: (dtheta [p], dtau [m]) of the damped arrow system with the rows C [m, p],
    d, gt [m] that enter (D_k > 0 for all of them)."""
    T = np.float32 if dtype == torch.float32 else np.float64
    Hm, gv, C, d, gt, lam = (np.asarray(x, dtype=T) for x in (Hm, gv, C, d, gt, lam))
    p = Hm.shape[0]
    hmax = np.diag(Hm).max()
    ft = T(1e-8) * (d.max() if d.size else T(0))
    Dk = d + lam * (d + ft)
    S = Hm + lam * (np.diag(np.diag(Hm)) + T(1e-8) * hmax * np.eye(p, dtype=T))
    b = -gv
    for k in range(C.shape[0]):
        u = C[k] / Dk[k]
        S = S - np.outer(u, C[k])
        b = b + u * gt[k]
    Lc = np.linalg.cholesky(S)
    dth = np.linalg.solve(Lc.T, np.linalg.solve(Lc, b)).astype(T)
    return dth, (-(gt + C @ dth) / Dk).astype(T)


def arrow_backward_error(Hm, gv, C, d, gt, lam, dth, dtau, n_full, eps):
    """|A z + g|_inf / (8 n eps (|A|_inf |z|_inf + |g|_inf)) of the full damped arrow system in fp64."""
    p, m = Hm.shape[0], C.shape[0]
    hmax = float(np.diag(Hm).max())
    ft = 1e-8 * (float(d.max()) if m else 0.0)
    A = np.zeros((p + m, p + m))
    A[:p, :p] = Hm + lam * (np.diag(np.diag(Hm)) + 1e-8 * hmax * np.eye(p))
    A[p:, :p], A[:p, p:] = C, C.T
    A[p:, p:] = np.diag(d + lam * (d + ft))
    z, g = np.concatenate([dth, dtau]).astype(np.float64), np.concatenate([gv, gt])
    resid = np.abs(A @ z + g).max()
    return resid / (8 * n_full * eps * (np.abs(A).sum(axis=1).max() * np.abs(z).max() + np.abs(g).max()))


def run_lm_step_times(lib, device, dtype, G, D, p, K, offset=0):
    """Returns (worst backward error / bound of the kernel, of the numpy elimination in the dtype); asserts everything else."""
    eps = eps_of(dtype)
    st, kind, big, extra, nan_reject = lmt_state(G, D, p, K, dtype, device, offset)
    n_full = p + D * K
    # 1. all-zero blocks: theta, theta_trial, lambda, accepted are the bits of lfsd_lm_step on the same inputs
    plo = torch.full((p,), -float("inf"), dtype=torch.float64)
    plo[0] = 0.25
    plo = plo.to(device=device, dtype=dtype)
    sz, _, _, _, _ = lmt_state(G, D, p, K, dtype, device, offset, zero_blocks=True)
    Z = lmt_call(lib, sz, D, proj_lo=plo)
    O = LC.lm_call(lib, sz, proj_lo=plo)
    for nm in ("theta", "trial", "lam", "accepted", "loss_acc", "grad_acc", "H_acc"):
        assert H.same(Z[nm], O[nm]), ("bits of lfsd_lm_step", nm)
    # 2. run A: theta = theta_trial = 0, no projection -- theta_trial comes out as dtheta, tau_trial - tau as dtau
    zero_t = lambda t: torch.where(torch.isnan(t), t, torch.zeros_like(t))        # (the NaN padding of absent waypoints stays)
    stA = dict(st, theta=torch.zeros_like(st["theta"]), trial=torch.zeros_like(st["trial"]), tau=zero_t(st["tau"]),
               tau_trial=zero_t(st["tau_trial"]))
    A = lmt_call(lib, stA, D)
    cast = lambda x: torch.tensor(x, dtype=torch.float64).to(dtype)
    down, up, lo, hi = (cast(LM[k]) for k in ("lambda_down", "lambda_up", "lambda_min", "lambda_max"))
    want_accept = np.isin(kind, (0, 1, 8, 9)) & ~nan_reject
    cpu = lambda d_, nm: d_[nm].cpu()
    a_all, s_all = {nm: cpu(A, nm) for nm in STATE + ("accepted",)}, {nm: cpu(stA, nm) for nm in STATE}
    t_all = {nm: stA[nm].cpu() for nm in ("loss_t", "grad_t", "H_t", "gtau_t", "C_t", "d_t", "row_ok", "w")}
    worst = worst_np = 0.0
    for g in range(G):
        k, rows = kind[g], slice(g * D, (g + 1) * D)
        grp = lambda d_, nm: d_[nm][rows] if nm in ("tau", "tau_trial", "gtau_acc", "C_acc", "d_acc", "ok_acc") else d_[nm][g]
        if k == 5:                                      # not active: every word of the state, accepted = 0
            assert all(H.same(grp(a_all, nm), grp(s_all, nm)) for nm in STATE) and int(a_all["accepted"][g]) == 0
            continue
        acc = bool(want_accept[g])
        assert int(a_all["accepted"][g]) == int(acc), (g, k, extra[g])
        lam0 = s_all["lam"][g]
        lam1 = torch.maximum(lam0 * down, lo) if acc else torch.minimum(lam0 * up, hi)
        ok_t = t_all["row_ok"][rows] != 0
        if acc:                                         # the copies, word for word
            assert torch.equal(a_all["loss_acc"][g], t_all["loss_t"][g]) and torch.equal(a_all["grad_acc"][g], t_all["grad_t"][g])
            assert torch.equal(a_all["H_acc"][g], t_all["H_t"][g]) and torch.equal(a_all["theta"][g], s_all["trial"][g])
            assert H.same(a_all["tau"][rows], s_all["tau_trial"][rows]) and torch.equal(a_all["ok_acc"][rows], t_all["row_ok"][rows])
            for nm in ("gtau", "C", "d"):
                assert H.same(a_all[nm + "_acc"][rows][ok_t], t_all[nm + "_t"][rows][ok_t]), (g, nm)
                assert H.same(a_all[nm + "_acc"][rows][~ok_t], s_all[nm + "_acc"][rows][~ok_t]), (g, nm)
        else:
            for nm in ("theta", "loss_acc", "grad_acc", "H_acc", "tau", "gtau_acc", "C_acc", "d_acc", "ok_acc"):
                assert H.same(grp(a_all, nm), grp(s_all, nm)), (g, k, nm)
        if k == 7 and p > 1:                            # (zero blocks: the retries of lfsd_lm_step, compared bit for bit above in run Z)
            lam1 = a_all["lam"][g]
        assert torch.equal(a_all["lam"][g], lam1), (g, k, float(a_all["lam"][g]), float(lam1))
        Hm, gv = a_all["H_acc"][g].double().numpy(), a_all["grad_acc"][g].double().numpy()
        hmax = float(np.diag(Hm).max())
        moves = np.isfinite(float(a_all["loss_acc"][g])) and hmax > 0
        dth = a_all["trial"][g].double().numpy()
        tau_a, trial_a = a_all["tau"][rows].numpy(), a_all["tau_trial"][rows].numpy()
        stays = (not moves) or (k == 7 and p > 1 and bool(big[g]))
        if stays:
            assert not dth.any() and np.array_equal(trial_a.view(np.uint8), tau_a.view(np.uint8)), (g, k)
            continue
        lam64 = float(a_all["lam"][g])
        Ca, da, ga_ = (a_all[nm][rows].double().numpy() for nm in ("C_acc", "d_acc", "gtau_acc"))
        okr = a_all["ok_acc"][rows].numpy() != 0
        ex = t_all["w"][rows].numpy() != 0
        enter = okr[:, None] & ex
        ft = 1e-8 * (da[enter].max() if enter.any() else 0.0)
        with np.errstate(invalid="ignore"):
            moving = enter & (da + lam64 * (da + ft) > 0)
        # everything that does not enter keeps its time, bit for bit
        assert np.array_equal(trial_a[~moving].view(np.uint8), tau_a[~moving].view(np.uint8)), (g, k)
        dtau = trial_a[moving].astype(np.float64)             # (tau = 0 in this run: tau_trial is dtau itself, exactly)
        assert not tau_a[moving].any()
        Cm, dm, gm = Ca[moving], da[moving], ga_[moving]
        assert np.isfinite(dth).all() and dth.any()
        dth_np, dtau_np = numpy_elimination(Hm, gv, Cm, dm, gm, a_all["lam"][g].numpy(), dtype)
        worst_np = max(worst_np, arrow_backward_error(Hm, gv, Cm, dm, gm, lam64, dth_np, dtau_np, n_full, eps))
        worst = max(worst, arrow_backward_error(Hm, gv, Cm, dm, gm, lam64, dth, dtau, n_full, eps))
    # 3. run B: random theta and a projection on component 0: max(theta + dtheta, proj_lo) with run A's dtheta; tau_trial as in run A
    Bres = lmt_call(lib, st, D, proj_lo=plo)
    on = torch.from_numpy(kind != 5).to(device)
    for nm in ("lam", "accepted", "H_acc", "grad_acc", "loss_acc", "gtau_acc", "C_acc", "d_acc", "ok_acc"):
        assert H.same(Bres[nm], A[nm]), nm
    # tau_trial = tau + dtau with run A's dtau, bit for bit (one addition in the dtype)
    on_rows = on.repeat_interleave(D)
    assert H.same(Bres["tau_trial"][on_rows], (Bres["tau"] + A["tau_trial"])[on_rows])
    assert H.same(Bres["tau_trial"][~on_rows], st["tau_trial"][~on_rows]) and H.same(Bres["tau"][~on_rows], st["tau"][~on_rows])
    expect = torch.maximum(Bres["theta"] + A["trial"], plo[None, :])
    assert torch.equal(Bres["trial"][on], expect[on]) and torch.equal(Bres["trial"][~on], st["trial"][~on])
    # 4. permuting the groups permutes the bits; a group alone gives its bits
    perm = torch.randperm(G, generator=torch.Generator().manual_seed(3 * G + p)).to(device)
    rperm = (perm[:, None] * D + torch.arange(D, device=device)[None, :]).reshape(-1)
    per_row = ("tau", "tau_trial", "gtau_acc", "C_acc", "d_acc", "ok_acc", "gtau_t", "C_t", "d_t", "row_ok", "w")
    P = lmt_call(lib, {nm: (t[rperm] if nm in per_row else t[perm]).contiguous() for nm, t in st.items()}, D, proj_lo=plo)
    for nm in STATE + ("accepted",):
        assert H.same(P[nm], Bres[nm][rperm if nm in per_row else perm]), nm
    at = G // 2
    one = lmt_call(lib, {nm: (t[at * D:(at + 1) * D] if nm in per_row else t[at:at + 1]).contiguous() for nm, t in st.items()}, D, proj_lo=plo)
    for nm in STATE + ("accepted",):
        assert H.same(one[nm], Bres[nm][at * D:(at + 1) * D] if nm in per_row else Bres[nm][at:at + 1]), nm
    return worst, worst_np


def lm_step_times_einval(L):
    """Every LFSD_EINVAL case of lfsd_lm_step_times on host dummies (no launch is reached)."""
    buf = (ctypes.c_double * 64)()
    d = ctypes.cast(buf, ctypes.c_void_p)
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.lfsd_lm_step_times.argtypes = [ci] * 5 + [cd] * 4 + [vp] * 24
    names = ("theta", "loss_acc", "grad_acc", "H_acc", "lam", "trial", "tau", "tau_trial", "gtau_acc", "C_acc", "d_acc", "ok_acc",
             "loss_t", "grad_t", "H_t", "gtau_t", "C_t", "d_t")
    base = dict(dtype=1, G=2, D=2, p=3, K=2, down=1.0 / 3.0, up=2.0, lo=1e-8, hi=1e8, **{nm: d for nm in names})
    call = lambda **kw: (lambda a: L.lfsd_lm_step_times(a["dtype"], a["G"], a["D"], a["p"], a["K"], a["down"], a["up"], a["lo"], a["hi"],
                                                        *[a[nm] for nm in names], None, None, None, None, None, None))(dict(base, **kw))
    nan = float("nan")
    bads = [dict(dtype=7), dict(dtype=-1), dict(G=0), dict(G=-1), dict(D=0), dict(D=-2), dict(K=0), dict(K=-1), dict(p=0), dict(p=-2), dict(p=17),
            dict(down=0.0), dict(down=-0.5), dict(down=1.5), dict(down=nan), dict(up=0.5), dict(up=nan), dict(lo=0.0), dict(lo=-1.0),
            dict(lo=nan), dict(lo=1e9), dict(hi=nan), dict(hi=1e-9), dict(dtype=0, lo=1e-50), dict(dtype=0, hi=1e39)] + [{nm: None} for nm in names]
    for bad in bads:
        assert call(**bad) == -1, bad


# ---- the learner -----------------------------------------------------------------------------------------------------------------
# The grouped learner (pendulum, fp64, n_grid 10, G = 2 seeds of lm_cases.compose_seeds, D = 3 demonstrations) starts at lambda0 = 3.
# Tried 0.01 / 0.1 / 0.3 / 1 / 3 / 10 / 30 over six steps: up to 0.1 both groups reject every proposal after the first evaluation, at 30
# both accept every one.  At 3 group 0 rejects in steps 2-4 (lambda raised per group, the trial times of its three rows back at the
# accepted ones, tau_project after a rejected group) and accepts in steps 5 and 6, while group 1 accepts throughout.  The second run,
# with skip_unconverged, is no further rejection test: there the solves of all three rows of group 0 fail at the first trial point and
# stay frozen, so the group is inactive from step 2 on (not accepted, lambda untouched, its times kept through group_active and the
# per-row row_active of tau_project) beside the accepting group 1.
GROUPED_LAMBDA0 = 3.0


def rows_ok(sol, aux):
    """The freeze mask of skip_unconverged, restated (tests/test_free_times_emu.py)."""
    st, loss, grad, stats = sol["status"], aux["loss"], aux["grad"], aux["stats"]
    return ((st == 1) | (st == 2)) & torch.isfinite(loss) & torch.isfinite(grad).all(dim=1) & ((stats[:, 1] + stats[:, 3]) == 0)


def lmt_by_hand(oc, x0, hz, taus, wps, iface, theta0, steps, proj_lo, lambda0, D=1, c=0.25, level=1, wts=None, bounds=None, skip=None):
    """The joint LM iteration from its launches.  x0 / hz / taus / wps / wts per ROW (B = G * D), theta0 [G, p].  Yields per step the
    state after the update and the (loss, grad) step() returns."""
    lib = oc.compile()
    th = oc._t(theta0).contiguous().clone()
    G, p = th.shape
    dev, dt = th.device, th.dtype
    skip = (D > 1) if skip is None else skip
    x0, hz, tau, wps = oc._t(x0), oc._t(hz).contiguous(), oc._t(taus).contiguous().clone(), oc._t(wps).contiguous()
    B, K = tau.shape
    trial, tau_trial = th.clone(), tau.clone()
    loss_acc = torch.full((G,), float("inf"), dtype=dt, device=dev)
    g_acc, H_acc = torch.zeros_like(th), torch.zeros((G, p, p), dtype=dt, device=dev)
    lam = torch.full((G,), lambda0, dtype=dt, device=dev)
    z = lambda *s: torch.zeros(s, dtype=dt, device=dev)
    gtau, Ca, da, oka = z(B, K), z(B, K, p), z(B, K), torch.zeros(B, dtype=torch.int32, device=dev)
    accepted = torch.zeros(G, dtype=torch.int32, device=dev)
    idx = torch.as_tensor(list(iface), dtype=torch.int32, device=dev)
    lo, hi = (None, None) if bounds is None else bounds
    wkw = {} if wts is None else dict(waypoint_weights=wts)
    prev = None
    for _ in range(steps):
        th_rows = trial if D == 1 else trial.repeat_interleave(D, dim=0).contiguous()
        u_init = None
        if skip and prev is not None:      # (a solve at the iteration limit is continued, every other one cold-starts: the learner's rule)
            pu = prev["control_grid"][:, :-1]
            u_init = torch.where((prev["status"] == 3).reshape(-1, 1, 1) & torch.isfinite(pu), pu, torch.zeros_like(pu)).contiguous()
        sol = oc.cocSolverBatch(x0, hz, th_rows, consts=oc.consts_tensor(), u_init=u_init)
        prev = dict(control_grid=sol["control_grid"].clone(), status=sol["status"].clone())
        aux = oc.auxSysSolverBatch(sol, tau_trial, wps, iface, want_grids=True, validate=False, interplation_level=level,
                                   skip_status=(3, 4) if skip else None, **wkw)
        aX = aux["auxX_grid"]
        ad = aX.dtype
        cv = lambda t: None if t is None else t.to(ad).contiguous()
        curv = aux["curvature"][0] if level == 2 else None
        Hm = lib.normal_matrix(cv(hz), cv(tau_trial), aX, idx, **({} if wts is None else dict(wp_weight=cv(wts)))).to(dt)
        gt = lib.waypoint_time_grad(cv(sol["state_grid"]), cv(hz), cv(tau_trial), cv(wps), idx, curv=curv, wp_weight=cv(wts)).to(dt)
        Ct, dt_ = lib.time_normal_blocks(cv(sol["state_grid"]), cv(hz), cv(tau_trial), aX, idx, curv=curv, wp_weight=cv(wts))
        Ct, dt_ = Ct.to(dt), dt_.to(dt)
        loss, grad = aux["loss"].to(dt).clone(), aux["grad"].to(dt).clone()
        row_ok = active = None
        if skip:
            ok = rows_ok(sol, aux)
            row_ok = ok.to(torch.int32)
            grad = torch.where(ok.unsqueeze(1), grad, torch.zeros_like(grad))
            active = row_ok
        if D > 1:
            loss, grad, Hm, n_ok = lib.group_reduce(loss.contiguous(), grad.contiguous(), D, H=Hm.contiguous(), row_ok=row_ok)
            active = None if row_ok is None else (n_ok > 0).to(torch.int32)
        lib.lm_step_times(th, loss_acc, g_acc, H_acc, lam, trial, tau, tau_trial, gtau, Ca, da, oka, loss.contiguous(), grad.contiguous(),
                          Hm, gt.contiguous(), Ct.contiguous(), dt_.contiguous(), group_size=D, row_ok=row_ok, wp_weight=wts, proj_lo=proj_lo,
                          group_active=active, accepted=accepted, **LM)
        rows = active if active is None or D == 1 else active.repeat_interleave(D).contiguous()
        lib.tau_project(tau, tau_trial, hz, c, wp_weight=wts, tau_lo=lo, tau_hi=hi, row_active=rows)
        yield dict(theta=th.clone(), theta_trial=trial.clone(), lm_lambda=lam.clone(), lm_loss=loss_acc.clone(), taus=tau.clone(),
                   tau_trial=tau_trial.clone(), tau_grad=gt.clone(), C=Ca.clone(), d=da.clone(), loss=loss.clone(), grad=grad.clone(),
                   accepted=accepted.clone() != 0)


def learner_view(L, loss, grad):
    C, d = L.time_blocks
    return dict(theta=L.theta, theta_trial=L.theta_trial, lm_lambda=L.lm_lambda, lm_loss=L.lm_loss, taus=L.taus, tau_trial=L.tau_trial,
                tau_grad=L.tau_grad, C=C, d=d, loss=loss, grad=grad, accepted=L.lm_accepted)


def ordered_inside(taus, hz, wts=None, bounds=None):
    t = taus.double().cpu().numpy()
    w = None if wts is None else wts.cpu().numpy()
    for b in range(t.shape[0]):
        row = t[b] if w is None else t[b][w[b] != 0]
        if row.size and not (np.all(np.isfinite(row)) and np.all(np.diff(row) > 0) and row[0] >= 0 and row[-1] <= float(hz[b])):
            return False
    if bounds is not None:
        lo, hi = (np.broadcast_to(np.asarray(x, dtype=np.float64), t.shape) for x in bounds)
        ex = np.ones(t.shape, dtype=bool) if w is None else w != 0
        return bool(np.all(t[ex] >= lo[ex]) and np.all(t[ex] <= hi[ex]))
    return True


def run_composition(make, hand, steps=6, half=None, D=1, bounds=None, need_reject=True, need_accept=True):
    """The learner against the launches made by hand, bit for bit over `steps` steps, tau state included; lm_loss never increases; an
    acceptance after the first step and a rejection; times ordered and inside the bounds; the same seeds in a batch of another size."""
    L = make()
    hist, acc = [], []
    for k in range(steps):
        loss, grad = L.step()
        want = next(hand)
        got = learner_view(L, loss, grad)
        for nm in want:
            assert H.same(got[nm], want[nm]), (k, nm)
        hist.append({nm: t.clone() for nm, t in got.items()})
        acc.append(L.lm_accepted.clone())
        assert ordered_inside(L.taus, L.hz, L.wts, bounds) and ordered_inside(L.tau_trial, L.hz, L.wts, bounds), k
    lm_loss = torch.stack([h["lm_loss"] for h in hist])
    assert bool((lm_loss[1:] <= lm_loss[:-1]).all()) and bool(torch.isfinite(lm_loss[-1]).all())
    acc = torch.stack(acc)
    assert not need_accept or bool(acc[1:].any()), acc
    assert not need_reject or bool((~acc[1:]).any()), acc
    assert not need_accept or not torch.equal(L.taus, L.tau0)                # the accepted times have moved
    assert not torch.equal(L.tau_trial, L.tau0)
    if half is not None:                                                     # the same seeds in a batch of another size: the same bits
        Ls = make(rows=slice(0, half))
        for k in range(steps):
            loss, grad = Ls.step()
            got = learner_view(Ls, loss, grad)
            for nm in got:
                per_row = nm in ("taus", "tau_trial", "tau_grad", "C", "d")
                assert H.same(got[nm], hist[k][nm][:half * D if per_row else half]), (k, nm)
    return L, hist


# ---- recovery on data with a known answer -------------------------------------------------------------------------------------------
# Pendulum, fp64, the setting of tests/tau_cases.py: waypoints from the trajectory at theta* at known times tau*, but on a grid of
# RECOVER_N_GRID = 40 intervals, not 10.  The Gauss-Newton step takes dy/dtheta from auxX_grid, the sensitivity of the continuous
# problem sampled on the grid, which is the derivative of the solved state grid only up to the discretisation: against central
# differences of the solver (step 1e-6) it is off by 0.23 / 0.35 / 0.16 per parameter at n_grid 10 (entries of size 0.7 / 1.6 / 1.5),
# by 0.03 / 0.07 / 0.10 at 40 and 0.01 / 0.01 / 0.02 at 100, while the joint Jacobian's smallest singular value is 0.03 .. 0.05 against
# 5 for the largest.  With a Jacobian a quarter off the step converges linearly at best: at n_grid 10 the fp64 loop below contracts the
# loss by 0.3 .. 0.8 per accepted step near the solution and rejects every second proposal (4.7e-6 of the initial loss after 12 steps
# from theta off by 10 %, no better from 30 % or 50 % or shifts of 0.15 / 0.3 / 0.45 of the gap, lambda0 1e-2 or 1e-4), so a decision
# with a margin of 1e-4 cannot be followed by a loss below 1e-6 of an initial loss below 10.  At 40 intervals the loop accepts every
# step and contracts the loss a thousand-fold in its last ones.
# A row learns p = 3 parameters and K times from its own waypoints, and every waypoint brings one unknown of its own: with the angle alone
# (one residual per waypoint) the joint problem has more unknowns than residuals whatever K is -- the loss then goes to zero at times
# that are NOT tau* (seen with K = 3: the loop ends 0.032 from tau* at a loss of 1e-28).  So both state components are observed,
# interface (0, 1), at K = 5 waypoints: 10 residuals for 8 unknowns.
# Chosen start: theta = theta* (1 + 0.3 s) with s = (+1, -1, +1) for row 0 and (-1, +1, -1) for row 1, every time shifted by
# RECOVER_SHIFT = 0.15 of its gap to the neighbour on the side of the sign pattern below, lambda0 = 1e-2 (the learner's default), the
# default tau_max_shift 0.25.  The loop is fp64 numpy: the state grid and the sensitivity grid of each trial point come from the solver
# and the sweeps (as tests/tau_cases.py takes its state grid from the solver); residuals, Jacobian, slope, the dense (p + K) damped
# solve and the projection are formed here, no kernel of the step is called.  The conditions are counted row by row, since each row
# is a problem of its own: a row runs until both of its conditions hold (at most RECOVER_STEPS = 12 steps; here 4 and 5), the
# decisions it took up to there must each be clear by 100 x the parity tolerance (smallest margins 1.45e-4 and 1.14e-4), and the
# learner is compared with the row over those steps.  (Later decisions compare losses that fall to the rounding floor: their margin
# goes to zero with the loss in any implementation.)
RECOVER_TAU_STAR = (0.25, 0.35, 0.55, 0.65, 0.85)      # nodes of the 40-interval grid: the interpolant's kinks
RECOVER_IFACE = (0, 1)
RECOVER_THETA_SIGNS = ((+1, -1, +1), (-1, +1, -1))
RECOVER_SIGNS = ((+1, -1, +1, -1, +1), (-1, +1, -1, +1, -1))
RECOVER_N_GRID = 40
RECOVER_THETA_OFF, RECOVER_SHIFT, RECOVER_STEPS, RECOVER_C, RECOVER_LAMBDA0 = 0.3, 0.15, 12, 0.25, 1e-2
RECOVER_TOL = TC.RECOVER_TOL


def recovery_start(horizon):
    star = np.array(RECOVER_TAU_STAR, dtype=np.float64) * horizon
    edges = np.concatenate([[0.0], star, [horizon]])
    rows = [[star[k] + RECOVER_SHIFT * (edges[k + 2] - star[k] if s > 0 else -(star[k] - edges[k])) for k, s in enumerate(signs)]
            for signs in RECOVER_SIGNS]
    return star, np.array(rows)


def numpy_joint_lm(evaluate, theta0, tau0, hz, wp, idx, steps, lambda0, c, proj_lo):
    """Levenberg-Marquardt over (theta, tau) in fp64 numpy, row by row.  `evaluate(theta [B, p], tau [B, K]) -> (X [B, N+1, n],
    aX [B, N+1, p, n])`: the solved state grid and its sensitivity grid.  Returns a list per step of dict(theta, taus, lm_loss,
    accepted, margin = |loss_t - loss_acc|)."""
    B, p = theta0.shape
    K = tau0.shape[1]
    th, tau = theta0.copy(), tau0.copy()
    th_t, tau_t = th.copy(), tau.copy()
    lam = np.full(B, lambda0)
    loss_acc = np.full(B, np.inf)
    acc_state = [None] * B
    out = []
    for _ in range(steps):
        X, aX = evaluate(th_t, tau_t)
        n_grid = X.shape[1] - 1
        h = hz / n_grid
        accepted, margin = np.zeros(B, dtype=bool), np.zeros(B)
        for b in range(B):
            k = np.clip(np.floor(tau_t[b] / h), 0, n_grid - 1).astype(int)
            s = (tau_t[b] - k * h) / h
            xa, xb = X[b][k][:, idx], X[b][k + 1][:, idx]                                  # [K, C]
            r = xa + s[:, None] * (xb - xa) - wp[b]
            t = (xb - xa) / h
            Ja, Jb = aX[b][k][:, :, idx], aX[b][k + 1][:, :, idx]                          # [K, p, C]
            J = Ja + s[:, None, None] * (Jb - Ja)
            loss = float((r * r).sum())
            margin[b] = abs(loss - loss_acc[b])
            if loss < loss_acc[b]:
                accepted[b] = True
                th[b], tau[b], loss_acc[b] = th_t[b], tau_t[b], loss
                acc_state[b] = (np.einsum("kqc,kc->q", J, r), (r * t).sum(1), np.einsum("kqc,krc->qr", J, J), np.einsum("kqc,kc->kq", J, t),
                                (t * t).sum(1))
                lam[b] = max(lam[b] / 3.0, 1e-8)
            else:
                lam[b] = min(lam[b] * 2.0, 1e8)
            g, gt, Hm, Cm, dm = acc_state[b]
            A = np.zeros((p + K, p + K))
            A[:p, :p] = Hm + lam[b] * (np.diag(np.diag(Hm)) + 1e-8 * np.diag(Hm).max() * np.eye(p))
            A[p:, :p], A[:p, p:] = Cm, Cm.T
            A[p:, p:] = np.diag(dm + lam[b] * (dm + 1e-8 * dm.max()))
            zsol = np.linalg.solve(A, -np.concatenate([g, gt]))
            th_t[b] = np.maximum(th[b] + zsol[:p], proj_lo)
            prop = (tau[b] + zsol[p:])[None, :]
            tau_t[b] = TC.project_reference(tau[b][None, :].copy(), prop, np.array([hz]), c)[0]
        out.append(dict(theta=th.copy(), taus=tau.copy(), lm_loss=loss_acc.copy(), accepted=accepted, margin=margin))
    return out
