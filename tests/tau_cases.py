"""Cases of the learnable waypoint times (ABI 17: lfsd_waypoint_time_grad, lfsd_tau_project; SparseDemoLearner(learn_taus=True)), shared by
the CPU tier (kernels through the SIMT emulator, tests/test_free_times_emu.py) and the -m gpu tier (tests/test_free_times_gpu.py).

Yardsticks and bounds (eps of the kernel's dtype, N = n_grid, C = n_iface, Y = max |node value| of the trajectory).
  lfsd_waypoint_time_grad, linear level: an fp64 numpy restatement on the kernel's own rounded arrays.  The interval is formed as the
    kernel forms it (h = horizon / N and k = floor(tau / h) in the arrays' type: the slope jumps at a node, so the interval must be the
    kernel's), the fraction in extended precision.  Per component q, with d = x_b - x_a, M = |x_a| + |x_b|:
      the fraction carries (N / 2 + 2) eps (k h and the difference, as tests/lm_cases.py counts it), the interpolated value
      dx = ((N / 2 + 4) |d| + M) eps, the slope d / h two roundings, ds = 2 eps |d| / h, the product and the sum C + 4 more:
      |dtau - ref| <= sum_q [ w dx |slope| + |w r| ds + (C + 4) eps |w r| |slope| ] (+ 3 eps (|prior term| + sum |terms|) with a prior).
    The middle and last terms are the "small multiple of eps times sum |w r| |x_b - x_a| / h"; the first is the conditioning of the
    residual itself, which does not vanish with r.
  cubic level: scipy.interpolate.CubicSpline(bc_type="not-a-knot") and its .derivative() of the same grid in fp64.  The curvature
    grid comes from lfsd_grid_curvature in the dtype: its right-hand sides carry 7 Y eps, the (1, 4, 1) system has an inverse of norm
    1/2 and the elimination adds a few eps of |c| <= 2 Y, the end rows c_0 = 2 c_1 - c_2 triple it: |dc| <= 100 Y eps, |c| <= 6 Y.
    With |w_a|, |w_b| <= 0.385, |w_a'|, |w_b'| <= 2 and their own derivatives in s at most 2 and 6:
      dx += (77 Y + 12 Y (3 (N / 2 + 2) + 4)) eps,    ds += (400 Y + 12 Y (6 (N / 2 + 2) + 6)) eps / h.
  lfsd_tau_project: a numpy restatement in the dtype, bit for bit (the kernel forms its bounds without fused multiply-adds).
  Learner: identity with the same launches made by hand; conditions on comparisons made inside the tests."""
import ctypes

import numpy as np
import torch

import hyper_sweep_cases as H

SHAPES = ((1, 1), (67, 5), (4099, 5))       # 4099 x 5 leaves a partial last workgroup
N_GRIDS = (1, 2, 10)
N_GRIDS_CUBIC = (3, 10)                     # the cubic interpolant needs four nodes
N_STATE = 13
IFACE = (1, 6, 11)                          # three scattered state components


def eps_of(dtype):
    return float(torch.finfo(dtype).eps)


def grad_inputs(B, K, n_grid, dtype, device, seed=0):
    g = torch.Generator().manual_seed(7919 * B + 131 * K + 17 * n_grid + seed)
    u = lambda *s: torch.rand(s, generator=g, dtype=torch.float64)
    X = torch.randn((B, n_grid + 1, N_STATE), generator=g, dtype=torch.float64)
    hz = (0.5 + 2.5 * u(B)).to(device=device, dtype=dtype).contiguous()
    h = hz / n_grid
    slot = (torch.arange(B * K).reshape(B, K) % 5).to(device)      # 0, the horizon, a node as the kernel forms it, two interior
    node = torch.randint(0, n_grid + 1, (B, K), generator=g).to(device)
    inner = (u(B, K).to(device) * hz[:, None].double()).to(dtype)
    t = torch.where(slot == 0, torch.zeros_like(inner), inner)
    t = torch.where(slot == 1, hz[:, None].expand(B, K), t)
    t = torch.where(slot == 2, (node.to(dtype) * h[:, None]).minimum(hz[:, None]), t)
    wp = torch.randn((B, K, len(IFACE)), generator=g, dtype=torch.float64)
    to = lambda a: a.to(device=device, dtype=dtype).contiguous()
    return hz, t.contiguous(), to(X), to(wp), torch.tensor(IFACE, dtype=torch.int32, device=device)


def interval_of(hz, taus, n_grid):
    """(k [B, K] int64, s [B, K] fp64, h [B, 1] fp64): the interval in the arrays' type, as the kernel forms it; the fraction in
    extended precision."""
    hz_host = hz.cpu().numpy()
    h = hz_host / hz_host.dtype.type(n_grid)
    t = taus.cpu().numpy()
    with np.errstate(invalid="ignore"):
        q = np.floor(t / h[:, None])
    k = np.where(q >= 1, np.where(q < n_grid - 1, q, n_grid - 1), 0).astype(np.int64)
    L = np.longdouble
    s = ((t.astype(L) - k.astype(L) * h.astype(L)[:, None]) / h.astype(L)[:, None]).astype(np.float64)
    return k, s, h.astype(np.float64)[:, None]


def time_grad_reference(hz, taus, X, wp, n_grid, w=None, cubic=False, tau_ref=None, prior=0.0, idx=IFACE):
    """(dtau_ref [B, K], bound [B, K]) in fp64 (module docstring)."""
    eps = eps_of(X.dtype)
    k, s, h = interval_of(hz, taus, n_grid)
    X64 = X.double().cpu().numpy()
    Y = np.abs(X64).max(axis=(1, 2))[:, None, None]
    b = np.arange(X64.shape[0])[:, None]
    xa, xb = X64[b, k][:, :, list(idx)], X64[b, k + 1][:, :, list(idx)]      # [B, K, C]
    d, M = xb - xa, np.abs(xa) + np.abs(xb)
    s3, h3 = s[:, :, None], h[:, :, None]
    N, C = n_grid, len(idx)
    if not cubic:
        x, slope = xa + s3 * d, d / h3
        dx = ((N / 2 + 4) * np.abs(d) + M) * eps
        ds = 2 * eps * np.abs(d) / h3
    else:
        from scipy.interpolate import CubicSpline
        cs = CubicSpline(np.arange(N + 1, dtype=np.float64), X64, axis=1, bc_type="not-a-knot")      # knots at u = t / h
        c, dc = cs.c, cs.derivative().c                                                              # [4 | 3, N, B, n]
        ci = lambda a, m: a[m][k, b][:, :, list(idx)]
        x = ((ci(c, 0) * s3 + ci(c, 1)) * s3 + ci(c, 2)) * s3 + ci(c, 3)
        slope = ((ci(dc, 0) * s3 + ci(dc, 1)) * s3 + ci(dc, 2)) / h3
        dx = ((N / 2 + 4) * np.abs(d) + M + 77 * Y + 12 * Y * (3 * (N / 2 + 2) + 4)) * eps
        ds = (2 * np.abs(d) + 400 * Y + 12 * Y * (6 * (N / 2 + 2) + 6)) * eps / h3
    r = x - wp.double().cpu().numpy()
    wk = np.ones(taus.shape) if w is None else w.double().cpu().numpy()
    wr = wk[:, :, None] * r
    ref = (wr * slope).sum(-1)
    bound = (wk[:, :, None] * dx * np.abs(slope) + np.abs(wr) * ds + (C + 4) * eps * np.abs(wr * slope)).sum(-1)
    if tau_ref is not None and prior != 0.0:
        pt = prior * (taus.double().cpu().numpy() - tau_ref.double().cpu().numpy())
        bound = bound + 3 * eps * (np.abs(pt) + np.abs(wr * slope).sum(-1))
        ref = ref + pt
    return ref, bound


def run_time_grad(lib, device, dtype, B, K, n_grid, cubic):
    """Worst |dtau - ref| / bound of one shape; asserts the exact properties on the way."""
    hz, taus, X, wp, idx = grad_inputs(B, K, n_grid, dtype, device)
    curv = lib.grid_curvature(X) if cubic else None
    call = lambda **kw: lib.waypoint_time_grad(kw.pop("X", X), kw.pop("hz", hz), kw.pop("taus", taus), kw.pop("wp", wp),
                                               kw.pop("idx", idx), curv=kw.pop("curv", curv), **kw)
    out, band = H.guarded(torch.zeros((B, K), dtype=dtype, device=device))
    res = call(out=out)
    assert res.data_ptr() == out.data_ptr() and H.band_intact(band) and bool(torch.isfinite(out).all())
    ref, bound = time_grad_reference(hz, taus, X, wp, n_grid, cubic=cubic)
    ratio = float((np.abs(out.double().cpu().numpy() - ref) / bound).max())
    # with a prior
    tau_ref = (taus.double() + 0.1 * torch.randn(taus.shape, generator=torch.Generator().manual_seed(B), dtype=torch.float64).to(device)).to(dtype)
    got = call(tau_ref=tau_ref, tau_prior=0.75)
    ref_p, bound_p = time_grad_reference(hz, taus, X, wp, n_grid, cubic=cubic, tau_ref=tau_ref, prior=0.75)
    ratio = max(ratio, float((np.abs(got.double().cpu().numpy() - ref_p) / bound_p).max()))
    assert torch.equal(call(tau_ref=tau_ref, tau_prior=0.0), out) and torch.equal(call(tau_ref=None, tau_prior=0.75), out)
    # weights: all ones give the bits of none; powers of two scale exactly; weight 0 with NaN tau / target / tau_ref gives +0.0
    ones = torch.ones_like(taus)
    assert torch.equal(call(wp_weight=ones), out)
    pw = torch.tensor([1.0, 0.25, 4.0], dtype=dtype, device=device)[torch.arange(B * K, device=device).reshape(B, K) % 3]
    assert torch.equal(call(wp_weight=pw.contiguous()), out * pw)
    w0 = ones.clone()
    gone = (torch.arange(B * K, device=device).reshape(B, K) % 3) == 1
    w0[gone] = 0.0
    nan = float("nan")
    t0, wp0, tr0 = taus.clone(), wp.clone(), tau_ref.clone()
    t0[gone], tr0[gone] = nan, nan
    wp0[gone] = nan
    got0 = call(taus=t0, wp=wp0, wp_weight=w0, tau_ref=tr0, tau_prior=0.75)
    assert not bool(torch.isnan(got0).any())
    assert torch.equal(got0[~gone], got[~gone])
    assert bool((got0[gone] == 0).all()) and not bool(torch.signbit(got0[gone]).any())
    # a NaN state row poisons its own row and no other
    at = B // 2
    X2 = X.clone()
    X2[at] = nan
    got2 = call(X=X2, curv=lib.grid_curvature(X2) if cubic else None)
    keep = torch.ones(B, dtype=torch.bool, device=device)
    keep[at] = False
    assert bool(torch.isnan(got2[at]).all()) and torch.equal(got2[keep], out[keep])
    # permuting the rows permutes the bits; a row alone gives its bits
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(B + K)).to(device)
    pc = lambda t: None if t is None else t[perm].contiguous()
    assert torch.equal(call(X=pc(X), hz=pc(hz), taus=pc(taus), wp=pc(wp), curv=pc(curv)), out[perm])
    one = lambda t: None if t is None else t[at:at + 1].contiguous()
    assert torch.equal(call(X=one(X), hz=one(hz), taus=one(taus), wp=one(wp), curv=one(curv))[0], out[at])
    # an interface index outside [0, n_state): found on the device, nothing is written
    for bad in ((1, N_STATE, 11), (-1, 6, 11)):
        out2, band2 = H.guarded(torch.full((B, K), 777.0, dtype=dtype, device=device))
        call(idx=torch.tensor(bad, dtype=torch.int32, device=device), out=out2)
        assert H.band_intact(band2) and bool((out2 == 777.0).all()), bad
    return ratio


def run_prior_alone(lib, device, dtype, n_grid=8):
    """r = 0 exactly (times on nodes of a grid whose step is a power of two, targets the node values): dtau is the prior term, one
    rounding (tau - tau_ref is exact by construction)."""
    B, K = 5, 4
    g = torch.Generator().manual_seed(11)
    X = torch.randn((B, n_grid + 1, N_STATE), generator=g, dtype=torch.float64).to(device=device, dtype=dtype)
    hz = torch.full((B,), n_grid * 0.125, dtype=dtype, device=device)
    k = torch.tensor([[0, 2, 5, 7]] * B, device=device)
    taus = (k * 0.125).to(dtype).contiguous()
    wp = X[torch.arange(B, device=device)[:, None], k][:, :, list(IFACE)].contiguous()
    tau_ref = (taus - 0.015625 * torch.arange(1, K + 1, device=device)).to(dtype).contiguous()
    idx = torch.tensor(IFACE, dtype=torch.int32, device=device)
    got = lib.waypoint_time_grad(X, hz, taus, wp, idx, tau_ref=tau_ref, tau_prior=0.3)
    exact = float(torch.tensor(0.3, dtype=dtype)) * (taus.double() - tau_ref.double())
    assert bool(((got.double() - exact).abs() <= 0.5 * eps_of(dtype) * exact.abs()).all())


def run_compiled_interface(lib, device, dtype, iface_fn, B=67, K=5, n_grid=10, consts=None):
    """A library with a compiled-in interface y = g(x): dtau against r^T (dg/dx) xdot formed in fp64 by `iface_fn(x) -> (y, J)`."""
    n = lib.n_state
    g = torch.Generator().manual_seed(5)
    X = (0.5 * torch.randn((B, n_grid + 1, n), generator=g, dtype=torch.float64)).to(device=device, dtype=dtype).contiguous()
    hz = (0.5 + torch.rand(B, generator=g, dtype=torch.float64)).to(device=device, dtype=dtype)
    taus = (torch.rand((B, K), generator=g, dtype=torch.float64).to(device) * hz[:, None].double()).to(dtype).contiguous()
    wp = torch.randn((B, K, lib.n_interface), generator=g, dtype=torch.float64).to(device=device, dtype=dtype).contiguous()
    got = lib.waypoint_time_grad(X, hz, taus, wp, None, consts=consts)
    k, s, h = interval_of(hz, taus, n_grid)
    X64 = X.double().cpu().numpy()
    b = np.arange(B)[:, None]
    xa, xb = X64[b, k], X64[b, k + 1]
    x, slope = xa + s[:, :, None] * (xb - xa), (xb - xa) / h[:, :, None]
    y, J = iface_fn(x)                                                        # [B, K, q], [B, K, q, n]
    r = y - wp.double().cpu().numpy()
    ref = np.einsum("bkq,bkqi,bki->bk", r, J, slope)
    # the index path's count with the generated code's few dozen operations on values of order one: 64 eps of the terms' magnitude
    bound = 64 * (n_grid / 2 + 4) * eps_of(dtype) * np.einsum("bkq,bkqi,bki->bk", np.abs(r) + 1, np.abs(J), np.abs(slope) + 1)
    return float((np.abs(got.double().cpu().numpy() - ref) / bound).max())


# ---- lfsd_tau_project ----------------------------------------------------------------------------------------------------------
def project_reference(ref, io, hz, c, w=None, lo=None, hi=None, active=None):
    """The projection in numpy, in the arrays' type, operation for operation."""
    T = ref.dtype.type
    out = io.copy()
    B, K = ref.shape
    c = T(c)
    exists = np.ones((B, K), dtype=bool) if w is None else (w != 0)
    act = np.ones(B, dtype=bool) if active is None else (active != 0)
    prev = np.zeros(B, dtype=ref.dtype)
    with np.errstate(invalid="ignore"):
        for k in range(K):
            nxt, found = hz.copy(), np.zeros(B, dtype=bool)
            for j in range(k + 1, K):
                take = ~found & exists[:, j]
                nxt = np.where(take, ref[:, j], nxt)
                found |= take
            rk = ref[:, k]
            wlo, whi = rk - c * (rk - prev), rk + c * (nxt - rk)
            v = io[:, k].copy()
            if lo is not None:
                v = np.where(v > lo[:, k], v, lo[:, k])
            if hi is not None:
                v = np.where(v < hi[:, k], v, hi[:, k])
            v = np.where(v < wlo, wlo, np.where(v > whi, whi, v))
            v = np.where(np.isfinite(io[:, k]), v, rk)
            do = exists[:, k] & act
            out[:, k] = np.where(do, v, io[:, k])
            prev = np.where(exists[:, k], rk, prev)
    return out


def project_inputs(B, K, dtype, ragged=True, seed=0):
    """Ordered reference times, ragged rows (zero weights in the middle and at the end, NaN padded), proposals that overshoot both
    ways, swap neighbours or are not finite, bounds, inactive rows.  numpy arrays in the dtype."""
    rng = np.random.default_rng(1000 * B + K + seed)
    nd = torch.empty(0, dtype=dtype).numpy().dtype
    hz = (0.5 + 2.5 * rng.random(B)).astype(nd)
    ref = (np.sort(rng.random((B, K)), axis=1) * 0.98 + 0.01) * hz[:, None].astype(np.float64)
    ref = ref.astype(nd)
    ref[:, 1:] = np.maximum(ref[:, 1:], np.nextafter(ref[:, :-1], nd.type(np.inf)))      # (strictly increasing after the cast)
    kind = rng.integers(0, 6, (B, K))
    io = ref.astype(np.float64) + 0.02 * hz[:, None] * rng.standard_normal((B, K))         # a small move
    io = np.where(kind == 1, ref + 10.0 * hz[:, None], io)                                 # overshoot up
    io = np.where(kind == 2, ref - 10.0 * hz[:, None], io)                                 # overshoot down
    io = np.where(kind == 3, np.roll(ref, 1, axis=1), io)                                  # a neighbour's time: a swap
    io = np.where(kind == 4, rng.choice([np.nan, np.inf, -np.inf], (B, K)), io)
    io = io.astype(nd)
    w = np.ones((B, K), dtype=nd)
    if K >= 3 and ragged:
        w[rng.random((B, K)) < 0.25] = 0.0                                                 # in the middle and at the end
        w[::7, K - 1] = 0.0
    ref[w == 0] = np.nan
    io[w == 0] = np.nan
    lo = (ref - 0.05 * hz[:, None] * rng.random((B, K))).astype(nd)
    hi = (ref + 0.05 * hz[:, None] * rng.random((B, K))).astype(nd)
    active = (rng.random(B) < 0.8).astype(np.int32)
    return hz, ref, io, w, lo, hi, active


def run_tau_project(lib, device, dtype, B, K, c):
    dev = lambda a: None if a is None else torch.from_numpy(a).to(device).contiguous()
    for use_w, use_b, use_a in ((False, False, False), (True, False, False), (True, True, True)):
        hz, r_, i_, w, lo, hi, active = project_inputs(B, K, dtype, ragged=use_w)      # (without weights: no NaN padding)
        kw = dict(w=w if use_w else None, lo=lo if use_b else None, hi=hi if use_b else None, active=active if use_a else None)
        want = project_reference(r_, i_, hz, c, **kw)
        buf, band = H.guarded(dev(i_))
        got = lib.tau_project(dev(r_), buf, dev(hz), c, wp_weight=dev(kw["w"]), tau_lo=dev(kw["lo"]), tau_hi=dev(kw["hi"]),
                              row_active=dev(kw["active"]))
        assert H.band_intact(band)
        g = got.cpu().numpy()
        assert np.array_equal(g.view(np.uint8), want.view(np.uint8)), (use_w, use_b, use_a)      # bit for bit, NaN padding included
        ex = np.ones((B, K), dtype=bool) if not use_w else (w != 0)
        act = np.ones(B, dtype=bool) if not use_a else (active != 0)
        assert np.array_equal(g[~(ex & act[:, None])].view(np.uint8), i_[~(ex & act[:, None])].view(np.uint8))
        for b in np.nonzero(act)[0]:                     # strictly ordered, inside (0, horizon), non-finite proposals keep the time
            row = g[b][ex[b]]
            assert np.all(np.isfinite(row)) and np.all(np.diff(row) > 0) and (row.size == 0 or (row[0] >= 0 and row[-1] <= hz[b])), (b, row)
            bad = ex[b] & ~np.isfinite(i_[b])
            assert np.array_equal(g[b][bad], r_[b][bad])
        # invariant under a permutation of the rows
        perm = np.random.default_rng(B).permutation(B)
        pk = {k: (None if v is None else v[perm]) for k, v in kw.items()}
        gp = lib.tau_project(dev(r_[perm]), dev(i_[perm]), dev(hz[perm]), c, wp_weight=dev(pk["w"]), tau_lo=dev(pk["lo"]),
                             tau_hi=dev(pk["hi"]), row_active=dev(pk["active"]))
        assert np.array_equal(gp.cpu().numpy().view(np.uint8), g[perm].view(np.uint8))


# ---- LFSD_EINVAL on host dummies ---------------------------------------------------------------------------------------------------
def time_grad_einval(L, n_iface_compiled):
    buf = (ctypes.c_double * 4096)()
    d = ctypes.cast(buf, ctypes.c_void_p).value
    at = lambda off: ctypes.c_void_p(d + off)
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.lfsd_waypoint_time_grad.argtypes = [ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, cd, vp, vp]
    base = dict(dtype=1, batch=2, n_grid=3, K=2, ni=1, X=at(0), curv=None, hz=at(8192), consts=None, cpt=0, taus=at(8192 + 64),
                wp=at(8192 + 128), idx=at(8192 + 256), w=None, tref=None, prior=0.0, out=at(16384))
    call = lambda **kw: (lambda a: L.lfsd_waypoint_time_grad(a["dtype"], a["batch"], a["n_grid"], a["K"], a["ni"], a["X"], a["curv"],
                                                             a["hz"], a["consts"], a["cpt"], a["taus"], a["wp"], a["idx"], a["w"],
                                                             a["tref"], a["prior"], a["out"], None))(dict(base, **kw))
    bads = [dict(dtype=7), dict(dtype=-1), dict(batch=0), dict(batch=-3), dict(n_grid=0), dict(n_grid=-1), dict(K=0), dict(K=-2),
            dict(ni=0), dict(ni=-1), dict(X=None), dict(hz=None), dict(taus=None), dict(wp=None), dict(out=None),
            dict(curv=at(4096), n_grid=2),                                         # the cubic interpolant needs four nodes
            dict(prior=-1.0), dict(prior=float("nan")), dict(prior=float("inf")), dict(prior=1e300, dtype=0),
            dict(out=at(8192 + 64)), dict(out=at(0)), dict(out=at(8192)), dict(out=at(8192 + 128 + 8)),
            dict(batch=2 ** 31 - 1, K=2 ** 10, X=vp(1 << 50), hz=vp(1 << 40), taus=vp(1 << 44), wp=vp(1 << 46), idx=vp(1 << 36),
                 out=vp(1 << 48))]                                                 # more than 2^31-1 workgroups
    # the compiled-in interface: absent, or of another size
    bads.append(dict(idx=None, ni=n_iface_compiled + 1))
    if n_iface_compiled == 0:
        bads.append(dict(idx=None, ni=1))
    for bad in bads:
        assert call(**bad) == -1, bad


def tau_project_einval(L):
    buf = (ctypes.c_double * 1024)()
    d = ctypes.cast(buf, ctypes.c_void_p).value
    at = lambda off: ctypes.c_void_p(d + off)
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.lfsd_tau_project.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, vp, cd, vp, vp]
    base = dict(dtype=1, batch=2, K=3, ref=at(0), io=at(256), hz=at(512), w=None, lo=None, hi=None, c=0.25, act=None)
    call = lambda **kw: (lambda a: L.lfsd_tau_project(a["dtype"], a["batch"], a["K"], a["ref"], a["io"], a["hz"], a["w"], a["lo"], a["hi"],
                                                      a["c"], a["act"], None))(dict(base, **kw))
    bads = [dict(dtype=5), dict(batch=0), dict(batch=-1), dict(K=0), dict(K=-1), dict(ref=None), dict(io=None), dict(hz=None),
            dict(c=0.0), dict(c=0.5), dict(c=-0.1), dict(c=0.7), dict(c=float("nan")), dict(c=1e-60, dtype=0),
            dict(c=0.49999999999, dtype=0),                                        # 0.5 after the cast to float
            dict(io=at(0)), dict(io=at(40)), dict(io=at(512 - 40)), dict(w=at(256 + 8)), dict(lo=at(256)), dict(hi=at(256 + 40)),
            dict(act=at(256 + 44))]
    for bad in bads:
        assert call(**bad) == -1, bad


# ---- the learner -------------------------------------------------------------------------------------------------------------------
def learner_state(L):
    c = lambda t: t.detach().clone()
    return dict(theta=c(L.theta), m=c(L.m), v=c(L.v), vhat=c(L.vhat), taus=c(L.taus), m_tau=c(L.m_tau), v_tau=c(L.v_tau),
                vhat_tau=c(L.vhat_tau))


def hand_step(oc, S, it, x0, hz, wps, iface, tau0, method, lr, tau_method, tau_lr, mu=0.9, b1=0.9, b2=0.999, eps=1e-8, c=0.25,
              level=1, wts=None, prior=0.0, proj_lo=None):
    """One learner step as a sequence of ModelLibrary calls on the state `S` (learner_state); returns (loss, grad, dtau)."""
    lib = oc.compile()
    th_e = lib.lookahead(S["theta"], S["m"], mu) if method == "Nesterov" else S["theta"]
    tau_e = S["taus"]
    if tau_method == "Nesterov":
        tau_e = lib.tau_project(S["taus"], lib.lookahead(S["taus"], S["m_tau"], mu), hz, c, wp_weight=wts)
    sol = oc.cocSolverBatch(x0, hz, th_e)
    aux = oc.auxSysSolverBatch(sol, tau_e, wps, iface, validate=False, interplation_level=level,
                               **({} if wts is None else dict(waypoint_weights=wts)))
    loss, grad = aux["loss"].clone(), aux["grad"].clone()
    curv = aux["curvature"][0] if level == 2 else None
    idx = torch.as_tensor(list(iface), dtype=torch.int32, device=hz.device)
    dtau = lib.waypoint_time_grad(sol["state_grid"], hz, tau_e.contiguous(), wps, idx, curv=curv, wp_weight=wts,
                                  tau_ref=tau0 if prior > 0 else None, tau_prior=prior)
    lib.optimizer_step(method, S["theta"], grad, it, lr, mu, b1, b2, eps, m=S["m"], v=S["v"], vhat=S["vhat"], proj_lo=proj_lo)
    start = S["taus"].clone()
    lib.optimizer_step(tau_method, S["taus"], dtau, it, tau_lr, mu, b1, b2, eps, m=S["m_tau"], v=S["v_tau"], vhat=S["vhat_tau"])
    lib.tau_project(start, S["taus"], hz, c, wp_weight=wts)
    return loss, grad, dtau


def run_composition(make, oc, x0, hz, wps, iface, tau0, rules, steps=6, **kw):
    """The learner against its launches made by hand, bit for bit over `steps` steps, the moments of the times included.
    `make(method, tau_method)` builds the learner; `rules`: (method, lr, tau_method, tau_lr) tuples."""
    for method, lr, tau_method, tau_lr in rules:
        L = make(method=method, learning_rate=lr, tau_method=tau_method, tau_learning_rate=tau_lr)
        S = learner_state(L)
        moved = False
        for it in range(steps):
            loss, grad = L.step()
            loss, grad = loss.clone(), grad.clone()
            hl, hg, hd = hand_step(oc, S, it, x0, hz, wps, iface, tau0, method, lr, tau_method, tau_lr, proj_lo=L.proj_lo, **kw)
            assert H.same(loss, hl) and H.same(grad, hg) and H.same(L.tau_grad, hd), (method, tau_method, it)
            for k, v in learner_state(L).items():
                assert H.same(v, S[k]), (method, tau_method, it, k)
            moved = moved or not torch.equal(L.taus, L.tau0)
        assert moved and torch.equal(L.tau0, tau0), (method, tau_method)


def quadratic_in_tau(ya, d, h, s, wp, w):
    """Inside an interval of the linear interpolant the loss of one waypoint is w |ya + s d - wp|^2 with s = (tau - k h) / h: exactly
    quadratic in tau.  Returns (loss, dloss/dtau, d2loss/dtau2) in fp64."""
    r = ya + s * d - wp
    return w * (r * r).sum(-1), 2 * w * (r * d).sum(-1) / h, 2 * w * (d * d).sum(-1) / (h * h)


# ---- recovery on data with a known answer ------------------------------------------------------------------------------------------
# Waypoints taken from the trajectory of the model at theta* at known times tau*; the learner starts at theta* (learning_rate = 0: the
# trajectory does not move) with every time shifted by +-0.3 of its gap to the neighbour on that side.  The reference is the loop
# below: fp64 numpy, no kernel of the project (time_grad_reference's formula, a Vanilla step, project_reference).  The loss of a
# waypoint is w |x(tau) - x(tau*)|^2, (half) its curvature in tau is the squared slope of the observed component, about 5 to 12 /s^2
# where the pendulum swings (tau* in [0.35, 0.85] of the horizon): tau_learning_rate = 0.08 contracts the error by 0.05 to 0.6 per
# step, 40 steps bring it far below a tenth of the shift (the restatement's own figure is asserted before the learner is looked at).
RECOVER_TAU_STAR = (0.37, 0.58, 0.83)
RECOVER_SIGNS = ((+1, -1, +1), (-1, +1, -1))
RECOVER_LR, RECOVER_STEPS, RECOVER_SHIFT, RECOVER_C = 0.08, 40, 0.3, 0.25
# the fp64 parity tolerance the project asserts for the pendulum's loss (tests/parity_cases.py: 1e-6); margin 1 (DESIGN.md section 17
# has the measured distance)
RECOVER_TOL = 1e-6


def recovery_start(horizon):
    star = np.array(RECOVER_TAU_STAR, dtype=np.float64) * horizon
    edges = np.concatenate([[0.0], star, [horizon]])
    rows = []
    for signs in RECOVER_SIGNS:
        rows.append([star[k] + RECOVER_SHIFT * (edges[k + 2] - star[k] if s > 0 else -(star[k] - edges[k])) for k, s in enumerate(signs)])
    return star, np.array(rows)


def numpy_tau_loop(X, horizon, wp, tau_start, lr, steps, c, idx):
    """Vanilla descent on the times in fp64 numpy: X [B, N+1, n] the state grid, wp [B, K, C]; returns the trace [steps+1, B, K]."""
    B, K = tau_start.shape
    n_grid = X.shape[1] - 1
    hz = torch.full((B,), float(horizon), dtype=torch.float64)
    Xt, wpt = torch.from_numpy(X), torch.from_numpy(wp)
    tau = tau_start.copy()
    trace = [tau.copy()]
    for _ in range(steps):
        g, _ = time_grad_reference(hz, torch.from_numpy(tau), Xt, wpt, n_grid, idx=idx)
        tau = project_reference(tau, tau - lr * g, hz.numpy(), c)
        trace.append(tau.copy())
    return np.array(trace)
