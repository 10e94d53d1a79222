"""Cases of the Levenberg-Marquardt outer update (ABI 14: lfsd_normal_matrix, lfsd_lm_step; SparseDemoLearner(method="LM")), shared by
the CPU tier (kernels through the SIMT emulator, tests/test_lm_emu.py) and the -m gpu tier (tests/test_lm_gpu.py).

Yardsticks and bounds (eps of the kernel's dtype).
  lfsd_normal_matrix: an fp64 numpy restatement on the kernel's own rounded arrays.  The interval rule forms h = horizon / n_grid in the
    arrays' type; the restatement takes that h and forms the interval in fp64 and the fraction in extended precision (the kernel
    forms the fraction as the sampling kernels do, s = (tau - k h) / h in the arrays' type: up to (k / 2 + 1) eps on s, which the
    +-20 % data below turns into at most a quarter of that on X).  |H - H_ref| <= (K n_iface + 3) eps sum|X||X| elementwise: one rounding per
    product and per addition plus the three of the interpolation.  The sensitivities keep their sign and vary by +-20 % along the
    grid (per-component signs and per-parameter scales over three decades are free), so that |X(tau)| is no smaller than the
    increments s (X_k+1 - X_k) whose roundings the "+3" stands for: the bound is then a rigorous one for these inputs, in units of
    the interpolant's own magnitude as the issue states it.  J^T r against lfsd_waypoint_vjp: the same count with |X||r|.
    General data -- sensitivities that change sign along the grid and inside intervals, where X(tau) cancels -- get a second case
    with a bound in the node values: with M = |X_k| + |X_k+1| >= |X(tau)|, |X_k+1 - X_k|, the interpolant carries at most
    (n_grid / 2 + 2.5) eps M (the fraction's (k / 2 + 1) eps times the increment, 1.5 eps of its own roundings), a product twice that
    plus one, the sum K n_iface - 1 more:  |H - H_ref| <= (K n_iface + n_grid + 6) eps sum M M.
  lfsd_lm_step: copies and untouched rows bit for bit; lambda the value the same multiplications give in the dtype; the solve by its
    backward error |A delta + g|_inf <= 8 p eps (|A|_inf |delta|_inf + |g|_inf) with A rebuilt in fp64 from the row's final lambda (the
    Cholesky bound (3p + 1) eps for the factorisation and the two substitutions, a factor of about 2 because A is formed in the dtype).
    delta is read exactly from a run with theta = 0 and no projection (theta_trial = 0 + delta); a second run with random theta and a
    projection must give max(theta + delta, proj_lo) with that delta, bit for bit.
  Learner: identity with the same launches made by hand; conditions on a comparison made inside the test ("it learns")."""
import ctypes

import numpy as np
import torch

import hyper_sweep_cases as H

SHAPES_EMU = ((1, 1), (5, 7), (67, 12), (300, 16), (4099, 7))
SHAPES_GPU = ((1, 1), (67, 12), (300, 16), (4099, 7))
N_GRIDS = (1, 10)
N_WAYPOINTS = (1, 5)
N_STATE = 13
IFACE = (1, 6, 11)                     # three scattered state components
KINDS = 10                             # row kinds of the lm_step cases, below
LM = dict(lambda_down=1.0 / 3.0, lambda_up=2.0, lambda_min=1e-8, lambda_max=1e8)

# Learner cases.  The seeds of the composition cases are theta0 * (1 + COMPOSE_SCALE * u), u uniform in [-1, 1] from numpy's
# default_rng(COMPOSE_SEED).  Every row accepts its first evaluation by construction, so "a row accepts" alone would say nothing: the
# test asks for an acceptance AFTER the first step and for a rejection.  Seed 3 and the initial dampings below were chosen on the
# emulator for that.  These waypoints are far from any trajectory of the model (losses of 2 to 28) and some parameters are barely
# identified, so the nearly undamped step of the default lambda0 = 1e-2 is rejected five times in a row by most rows (pendulum: one
# acceptance in step 6; quadrotor: none in 6 steps).  Pendulum, lambda0 = 1: rows reject in steps 2-4 and accept in steps 5 and 6.
# Quadrotor, lambda0 = 300: all 12 rows accept in step 2, 5 accept and 7 reject in step 3.
COMPOSE_SEED, COMPOSE_SCALE, COMPOSE_STEPS = 3, 0.5, 6
COMPOSE_LAMBDA0 = dict(pendulum=1.0, quadrotor=300.0)


def eps_of(dtype):
    return float(torch.finfo(dtype).eps)


# ---- lfsd_normal_matrix ---------------------------------------------------------------------------------------------------------
def normal_inputs(B, p, n_grid, K, dtype, device, seed=0, general=False):
    g = torch.Generator().manual_seed(7919 * B + 131 * p + 17 * n_grid + K + seed)
    u = lambda *s: torch.rand(s, generator=g, dtype=torch.float64)
    n = N_STATE
    sign = torch.where(u(B, 1, p, n) < 0.5, -1.0, 1.0)
    scale = 10.0 ** (3.0 * u(B, 1, p, 1) - 1.5)
    aX = sign * scale * (0.8 + 0.4 * u(B, n_grid + 1, p, n))
    if general:                                                           # sign changes along the grid and inside intervals
        aX = scale * torch.randn((B, n_grid + 1, p, n), generator=g, dtype=torch.float64)
    hz = (0.5 + 2.5 * u(B)).to(device=device, dtype=dtype).contiguous()
    h = hz / n_grid                                                       # (in the dtype, as the kernel forms it)
    slot = (torch.arange(B * K).reshape(B, K)) % 5                        # 0, the horizon, a node as the kernel forms it, two interior
    node = torch.randint(0, n_grid + 1, (B, K), generator=g).to(device)
    inner = (u(B, K).to(device) * hz[:, None].double()).to(dtype)
    slot = slot.to(device)
    t = torch.where(slot == 0, torch.zeros_like(inner), inner)
    t = torch.where(slot == 1, hz[:, None].expand(B, K), t)
    t = torch.where(slot == 2, (node.to(dtype) * h[:, None]).minimum(hz[:, None]), t)
    r = torch.randn((B, K, len(IFACE)), generator=g, dtype=torch.float64)
    to = lambda a: a.to(device=device, dtype=dtype).contiguous()
    return hz, t.contiguous(), to(aX), to(r), torch.tensor(IFACE, dtype=torch.int32, device=device)


def interpolant_reference(hz, taus, aX, n_grid):
    """X(tau_k)[q][idx_c] in fp64 numpy, [B, K, p, n_iface], and M = |X_k| + |X_k+1| of its interval.  h is the dtype's quotient (the interval rule's: numpy's IEEE division
    of the host copies); the fraction is formed in extended precision, so that the fp64 case measures the kernel's roundings and not
    those of the restatement's own k h (up to n_grid / 2 eps); everything else is fp64."""
    hz_host = hz.cpu().numpy()
    h = (hz_host / hz_host.dtype.type(n_grid)).astype(np.float64)[:, None]
    t = taus.double().cpu().numpy()
    k = np.clip(np.floor(t / h), 0, n_grid - 1)
    s = ((t.astype(np.longdouble) - k.astype(np.longdouble) * h.astype(np.longdouble)) / h.astype(np.longdouble)).astype(np.float64)
    s = s[:, :, None, None]
    k = k.astype(np.int64)
    X = aX.double().cpu().numpy()[:, :, :, list(IFACE)]                   # [B, N+1, p, c]
    b = np.arange(X.shape[0])[:, None]
    xa, xb = X[b, k], X[b, k + 1]                                         # [B, K, p, c]
    return xa + s * (xb - xa), np.abs(xa) + np.abs(xb)


def run_normal_matrix_general(lib, device, dtype, B, p, n_grid, K):
    """Sign-changing sensitivities against the bound in the node values (module docstring); returns worst error / bound."""
    hz, taus, aX, r, idx = normal_inputs(B, p, n_grid, K, dtype, device, seed=1, general=True)
    out = lib.normal_matrix(hz, taus, aX, idx)
    assert bool(torch.isfinite(out).all()) and torch.equal(out, out.mT)
    X, M = interpolant_reference(hz, taus, aX, n_grid)
    assert B * p < 8 or ((X[..., 0] < 0).any() and (X[..., 0] > 0).any())
    bound = (K * len(IFACE) + n_grid + 6) * eps_of(dtype) * np.einsum("bkqc,bkrc->bqr", M, M)
    return float((np.abs(out.double().cpu().numpy() - np.einsum("bkqc,bkrc->bqr", X, X)) / bound).max())


def run_normal_matrix(lib, device, dtype, B, p, n_grid, K):
    """Returns (worst |H - H_ref| / bound, worst |J^T r - vjp| / bound); asserts everything else."""
    eps, ni = eps_of(dtype), len(IFACE)
    hz, taus, aX, r, idx = normal_inputs(B, p, n_grid, K, dtype, device)
    out, band = H.guarded(torch.zeros((B, p, p), dtype=dtype, device=device))
    res = lib.normal_matrix(hz, taus, aX, idx, out=out)
    assert res.data_ptr() == out.data_ptr() and H.band_intact(band)
    assert bool(torch.isfinite(out).all()) and torch.equal(out, out.mT)
    X, _ = interpolant_reference(hz, taus, aX, n_grid)
    ref = np.einsum("bkqc,bkrc->bqr", X, X)
    bound = (K * ni + 3) * eps * np.einsum("bkqc,bkrc->bqr", np.abs(X), np.abs(X))
    ratio_h = float((np.abs(out.double().cpu().numpy() - ref) / bound).max())
    # J^T r with the same J is lfsd_waypoint_vjp of r scattered on the interface components
    rx = torch.zeros((B, K, N_STATE), dtype=dtype, device=device)
    rx[:, :, list(IFACE)] = r
    g = lib.waypoint_vjp(hz, taus, rx, aX)
    r64 = r.double().cpu().numpy()
    gref = np.einsum("bkqc,bkc->bq", X, r64)
    gbound = (K * ni + 3) * eps * np.einsum("bkqc,bkc->bq", np.abs(X), np.abs(r64))
    ratio_g = float((np.abs(g.double().cpu().numpy() - gref) / gbound).max())
    # a NaN row of auxX_grid (a row the sweeps skipped) poisons its own H and no other
    at = B // 2
    aX2 = aX.clone()
    aX2[at] = float("nan")
    got2 = lib.normal_matrix(hz, taus, aX2, idx)
    keep = torch.ones(B, dtype=torch.bool, device=device)
    keep[at] = False
    assert bool(torch.isnan(got2[at]).all()) and torch.equal(got2[keep], out[keep])
    # permuting the rows of the batch permutes the bits; a row alone gives its bits
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(B + p)).to(device)
    assert torch.equal(lib.normal_matrix(hz[perm].contiguous(), taus[perm].contiguous(), aX[perm].contiguous(), idx), out[perm])
    one = lib.normal_matrix(hz[at:at + 1].contiguous(), taus[at:at + 1].contiguous(), aX[at:at + 1].contiguous(), idx)
    assert torch.equal(one[0], out[at])
    # an interface index outside [0, n_state): found on the device, nothing is written
    for bad in ((1, N_STATE, 11), (-1, 6, 11)):
        out2, band2 = H.guarded(torch.full((B, p, p), 777.0, dtype=dtype, device=device))
        lib.normal_matrix(hz, taus, aX, torch.tensor(bad, dtype=torch.int32, device=device), out=out2)
        assert H.band_intact(band2) and bool((out2 == 777.0).all()), bad
    return ratio_h, ratio_g


def normal_matrix_einval(L):
    """Every LFSD_EINVAL case of lfsd_normal_matrix on host dummies (no launch is reached)."""
    buf = (ctypes.c_double * 1024)()
    d = ctypes.cast(buf, ctypes.c_void_p).value
    at = lambda off: ctypes.c_void_p(d + off)
    # B = 2, n_grid = 3, n = 2, p = 2, K = 2, n_iface = 1 in fp64: idx 4 B, horizon 16 B, taus 32 B, auxX 256 B, H 64 B
    base = dict(dtype=1, batch=2, n_grid=3, n_state=2, n_param=2, K=2, ni=1, idx=at(0), hz=at(64), taus=at(128), aX=at(256), H=at(1024))
    call = lambda **kw: (lambda a: L.lfsd_normal_matrix(a["dtype"], a["batch"], a["n_grid"], a["n_state"], a["n_param"], a["K"], a["ni"],
                                                        a["idx"], a["hz"], a["taus"], a["aX"], a["H"], None))(dict(base, **kw))
    bads = [dict(dtype=7), dict(dtype=-1), dict(batch=0), dict(batch=-3), dict(n_grid=0), dict(n_state=0), dict(n_param=0), dict(K=0),
            dict(ni=0), dict(idx=None), dict(hz=None), dict(taus=None), dict(aX=None), dict(H=None),
            dict(H=at(0)), dict(H=at(64 + 8)), dict(H=at(128 - 8)), dict(H=at(128 + 24)), dict(H=at(256 + 248)), dict(H=at(256 - 56)),
            # more than 2^31-1 workgroups: 2^31-1 rows of 17 x 17 (addresses far apart: nothing overlaps, nothing is dereferenced)
            dict(batch=2 ** 31 - 1, n_grid=1, n_state=1, n_param=17, K=1, idx=ctypes.c_void_p(1 << 36), hz=ctypes.c_void_p(1 << 40),
                 taus=ctypes.c_void_p(1 << 41), aX=ctypes.c_void_p(1 << 44), H=ctypes.c_void_p((1 << 44) + (1 << 43)))]
    for bad in bads:
        assert call(**bad) == -1, bad


# ---- lfsd_lm_step -----------------------------------------------------------------------------------------------------------------
# Row kinds (row b has kind (b + offset) % 10; `big` = ((b + offset) // 10) % 2 selects a variant):
#   0 first evaluation (loss_acc = +inf, nothing accepted)   1 accept   2 reject, larger loss   3 reject, NaN loss
#   4 reject, a NaN in H_t beside a finite smaller loss   5 row_active = 0 (would accept)   6 all-zero H_acc (rejecting: cannot move)
#   7 indefinite H_acc = I - (1 + nu) (e0 e1^T + e1 e0^T) with a constant diagonal, so that A = H_acc + lambda (1 + 1e-8) I is positive
#     definite iff lambda (1 + 1e-8) > nu: nu = 0.5 needs 4 factors lambda_up from 0.04 (big = 0), nu = 1000 exhausts the 8 retries
#     (big = 1: the row stays where it is); p = 1 has no indefinite matrix with a positive diagonal: a plain rejection there
#   8 accept an H_t with a zero row / column (a parameter without sensitivity)   9 accept a diagonal H_t whose step binds proj_lo[0]
def lm_state(B, p, dtype, device, offset=0, seed=0):
    g = torch.Generator().manual_seed(104729 * B + 211 * p + seed)
    rn = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)
    ru = lambda *s: torch.rand(s, generator=g, dtype=torch.float64)
    kind = (np.arange(B) + offset) % KINDS
    big = ((np.arange(B) + offset) // KINDS) % 2
    spd = lambda: (lambda J: J.transpose(1, 2) @ J)(rn(B, p + 2, p) * 10.0 ** (2.0 * ru(B, 1, p) - 1.0))
    H_acc, H_t = spd(), spd()
    g_acc, g_t = rn(B, p), rn(B, p)
    loss_acc = 1.0 + ru(B)
    loss_t = torch.where(torch.from_numpy(np.isin(kind, (2, 6, 7))), 2.0 * loss_acc, 0.5 * loss_acc)
    lam = 10.0 ** (4.0 * ru(B) - 3.0)
    theta, trial = 1.0 + ru(B, p), 1.0 + ru(B, p)
    active = np.ones(B, dtype=np.int32)
    for b in range(B):
        k = kind[b]
        if k == 0:
            loss_acc[b], H_acc[b], g_acc[b] = float("inf"), 0.0, 0.0
        elif k == 3:
            loss_t[b] = float("nan")
        elif k == 4:
            H_t[b, p - 1, 0] = H_t[b, 0, p - 1] = float("nan")
        elif k == 5:
            active[b] = 0
        elif k == 6:
            H_acc[b] = 0.0
        elif k == 7 and p > 1:
            nu = 1000.0 if big[b] else 0.5
            H_acc[b] = torch.eye(p, dtype=torch.float64)
            H_acc[b, 0, 1] = H_acc[b, 1, 0] = -(1.0 + nu)
            lam[b] = 0.02
        elif k == 8:
            j0 = b % p
            H_t[b, j0, :] = 0.0
            H_t[b, :, j0] = 0.0
            g_t[b, j0] = 0.0
            if p == 1:                                   # (all of H_t is then zero: max_j H[j][j] = 0, the row cannot move)
                pass
        elif k == 9:
            H_t[b] = torch.diag(0.5 + ru(p))
            g_t[b, 0] = 5.0
            trial[b, 0] = 0.25 + 1e-3
            lam[b] = 1e-2
    to = lambda a: a.to(device=device, dtype=dtype).contiguous()
    st = dict(theta=to(theta), loss_acc=to(loss_acc), grad_acc=to(g_acc), H_acc=to(H_acc), lam=to(lam), trial=to(trial),
              loss_t=to(loss_t), grad_t=to(g_t), H_t=to(H_t), active=torch.from_numpy(active).to(device))
    return st, kind, big


def lm_call(lib, st, proj_lo=None, use_active=True):
    """lfsd_lm_step on guarded copies of the state; returns the state after the call (+ accepted)."""
    names = ("theta", "loss_acc", "grad_acc", "H_acc", "lam", "trial")
    views, bands = {}, []
    for nm in names:
        views[nm], band = H.guarded(st[nm])
        bands.append(band)
    acc, band = H.guarded(torch.full((st["lam"].shape[0],), 99, dtype=torch.int32, device=st["lam"].device))
    bands.append(band)
    lib.lm_step(views["theta"], views["loss_acc"], views["grad_acc"], views["H_acc"], views["lam"], views["trial"], st["loss_t"],
                st["grad_t"], st["H_t"], proj_lo=proj_lo, row_active=st["active"] if use_active else None, accepted=acc, **LM)
    assert all(H.band_intact(b) for b in bands)
    return dict(views, accepted=acc)


def run_lm_step(lib, device, dtype, B, p, offset=0):
    """Returns the worst backward error / bound of the rows that solved; asserts everything else."""
    eps = eps_of(dtype)
    st, kind, big = lm_state(B, p, dtype, device, offset)
    # run A: theta = theta_trial = 0, no projection -- theta_trial comes out as delta itself
    stA = dict(st, theta=torch.zeros_like(st["theta"]), trial=torch.zeros_like(st["trial"]))
    A = lm_call(lib, stA)
    cast = lambda x: torch.tensor(x, dtype=torch.float64).to(dtype)      # the entry point's cast of its double arguments
    down, up, lo, hi = (cast(LM[k]) for k in ("lambda_down", "lambda_up", "lambda_min", "lambda_max"))
    want_accept = np.isin(kind, (0, 1, 8, 9))
    worst = 0.0
    for b in range(B):
        k, row = kind[b], (lambda d: {nm: d[nm][b].cpu() for nm in ("theta", "loss_acc", "grad_acc", "H_acc", "lam", "trial")})
        a, s = row(A), row(stA)
        if k == 5:                                      # not active: every word of the state, accepted = 0
            assert all(H.same(a[nm], s[nm]) for nm in a) and int(A["accepted"][b]) == 0
            continue
        acc = bool(want_accept[b])
        assert int(A["accepted"][b]) == int(acc), (b, k)
        lam1 = torch.maximum(s["lam"] * down, lo) if acc else torch.minimum(s["lam"] * up, hi)
        if acc:                                         # the copies, word for word
            assert torch.equal(a["loss_acc"], st["loss_t"][b].cpu()) and torch.equal(a["grad_acc"], st["grad_t"][b].cpu())
            assert torch.equal(a["H_acc"], st["H_t"][b].cpu()) and torch.equal(a["theta"], s["trial"])
        else:
            assert all(H.same(a[nm], s[nm]) for nm in ("theta", "loss_acc", "grad_acc", "H_acc")), (b, k)
        Hm, gv = a["H_acc"].double().numpy(), a["grad_acc"].double().numpy()
        hmax = float(np.diag(Hm).max())
        moves = np.isfinite(float(a["loss_acc"])) and hmax > 0
        retries, stays = 0, not moves
        if k == 7 and p > 1:                            # the number of lambda_up factors until A is positive definite, in the dtype
            nu, lam_r = (1000.0 if big[b] else 0.5), lam1
            while not float(lam_r) * (1 + 1e-8) > nu * (1 + 1e-3) and retries < 8:
                assert float(lam_r) * (1 + 1e-8) < nu * (1 - 1e-3)       # (clear of the rounding of the factorisation)
                lam_r = torch.minimum(lam_r * up, hi)
                retries += 1
            stays = not float(lam_r) * (1 + 1e-8) > nu
            assert retries == (8 if big[b] else 4) and stays == bool(big[b])
            lam1 = lam_r
        assert torch.equal(a["lam"], lam1), (b, k, float(a["lam"]), float(lam1))
        delta = a["trial"].double().numpy()
        if stays:                                       # theta_trial <- theta (= 0 in this run)
            assert k in (0, 6, 7, 8) and not delta.any(), (b, k)
            continue
        lam64 = float(a["lam"])
        Am = Hm + lam64 * (np.diag(np.diag(Hm)) + 1e-8 * hmax * np.eye(p))
        resid = np.abs(Am @ delta + gv).max()
        bound = 8 * p * eps * (np.abs(Am).sum(axis=1).max() * np.abs(delta).max() + np.abs(gv).max())
        assert np.isfinite(delta).all() and delta.any()
        worst = max(worst, resid / bound)
    # run B: random theta, a projection on component 0: max(theta + delta, proj_lo) with run A's delta, bit for bit
    plo = torch.full((p,), -float("inf"), dtype=torch.float64)
    plo[0] = 0.25
    plo = plo.to(device=device, dtype=dtype)
    Bres = lm_call(lib, st, proj_lo=plo)
    on = torch.from_numpy(kind != 5).to(device)
    assert torch.equal(Bres["lam"], A["lam"]) and torch.equal(Bres["accepted"], A["accepted"]) and H.same(Bres["H_acc"], A["H_acc"])
    assert H.same(Bres["grad_acc"], A["grad_acc"]) and H.same(Bres["loss_acc"], A["loss_acc"])
    acc_rows = torch.from_numpy(want_accept & (kind != 5)).to(device)
    assert torch.equal(Bres["theta"][acc_rows], st["trial"][acc_rows]) and torch.equal(Bres["theta"][~acc_rows], st["theta"][~acc_rows])
    expect = torch.maximum(Bres["theta"] + A["trial"], plo[None, :])
    assert torch.equal(Bres["trial"][on], expect[on]) and torch.equal(Bres["trial"][~on], st["trial"][~on])
    assert bool((Bres["trial"][on][:, 0] >= plo[0]).all())
    for b in np.nonzero(kind == 9)[0]:                  # the projection binds: delta[0] < -1e-3 by construction
        assert float(A["trial"][b, 0]) < -1e-3 and float(Bres["trial"][b, 0]) == float(plo[0]), b
    # row_active = NULL: the row of kind 5 accepts like any other
    if (kind == 5).any():
        C = lm_call(lib, st, proj_lo=plo, use_active=False)
        b5 = torch.from_numpy(kind == 5).to(device)
        assert bool((C["accepted"][b5] == 1).all()) and torch.equal(C["theta"][b5], st["trial"][b5])
        assert torch.equal(C["trial"][on], Bres["trial"][on])
    # permuting the rows permutes the bits
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3 * B + p)).to(device)
    P = lm_call(lib, {nm: t[perm].contiguous() for nm, t in st.items()}, proj_lo=plo)
    for nm in ("theta", "loss_acc", "grad_acc", "H_acc", "lam", "trial", "accepted"):
        assert H.same(P[nm], Bres[nm][perm]), nm
    return worst


def lm_step_einval(L):
    """Every LFSD_EINVAL case of lfsd_lm_step on host dummies (no launch is reached)."""
    buf = (ctypes.c_double * 64)()
    d = ctypes.cast(buf, ctypes.c_void_p)
    cd = ctypes.c_double
    names = ("theta", "loss_acc", "grad_acc", "H_acc", "lam", "trial", "loss_t", "grad_t", "H_t")
    base = dict(dtype=1, batch=2, p=3, down=1.0 / 3.0, up=2.0, lo=1e-8, hi=1e8, **{nm: d for nm in names})
    call = lambda **kw: (lambda a: L.lfsd_lm_step(a["dtype"], a["batch"], a["p"], cd(a["down"]), cd(a["up"]), cd(a["lo"]), cd(a["hi"]),
                                                  *[a[nm] for nm in names], None, None, None, None))(dict(base, **kw))
    nan = float("nan")
    bads = [dict(dtype=7), dict(dtype=-1), dict(batch=0), dict(batch=-1), dict(p=0), dict(p=-2), dict(p=17), dict(down=0.0), dict(down=-0.5),
            dict(down=1.5), dict(down=nan), dict(up=0.5), dict(up=nan), dict(lo=0.0), dict(lo=-1.0), dict(lo=nan), dict(lo=1e9),
            dict(hi=nan), dict(hi=1e-9),
            dict(dtype=0, lo=1e-50), dict(dtype=0, hi=1e39)] + [{nm: None} for nm in names]      # 0 / inf once cast to fp32
    for bad in bads:
        assert call(**bad) == -1, bad


# ---- the learner ----------------------------------------------------------------------------------------------------------------
def compose_seeds(theta0, rows):
    rng = np.random.default_rng(COMPOSE_SEED)
    th0 = np.asarray(theta0, dtype=np.float64)
    return th0[None, :] * (1.0 + COMPOSE_SCALE * rng.uniform(-1, 1, (rows, th0.size)))


def lm_by_hand(oc, x0, hz, taus, wps, iface, theta0, steps, proj_lo, lambda0=1e-2):
    """The LM iteration from its launches: cocSolverBatch, auxSysSolverBatch(want_grids=True, waypoints), lib.normal_matrix,
    lib.lm_step.  Yields per step (theta, theta_trial, lambda, loss_acc, loss, grad) after the update."""
    lib = oc.compile()
    th = oc._t(theta0).contiguous().clone()
    B, p = th.shape
    dev, dt = th.device, th.dtype
    trial = th.clone()
    loss_acc = torch.full((B,), float("inf"), dtype=dt, device=dev)
    g_acc, H_acc = torch.zeros_like(th), torch.zeros((B, p, p), dtype=dt, device=dev)
    lam = torch.full((B,), lambda0, dtype=dt, device=dev)
    x0, hz_t = oc._t(x0), oc._t(hz)
    hz_t = hz_t.expand(B).contiguous() if hz_t.dim() == 0 else hz_t
    tt = oc._t(taus)
    tt = tt.unsqueeze(0).expand(B, -1).contiguous() if tt.dim() == 1 else tt
    wp = oc._t(wps)
    wp = wp.unsqueeze(0).expand(B, -1, -1).contiguous() if wp.dim() == 2 else wp
    idx = torch.as_tensor(list(iface), dtype=torch.int32, device=dev)
    for _ in range(steps):
        sol = oc.cocSolverBatch(x0, hz_t, trial, consts=oc.consts_tensor())
        aux = oc.auxSysSolverBatch(sol, tt, wp, iface, want_grids=True, validate=False)
        aX = aux["auxX_grid"]
        Hm = lib.normal_matrix(hz_t.to(aX.dtype).contiguous(), tt.to(aX.dtype).contiguous(), aX, idx).to(dt)
        loss, grad = aux["loss"].to(dt).clone(), aux["grad"].to(dt).clone()
        lib.lm_step(th, loss_acc, g_acc, H_acc, lam, trial, loss, grad, Hm, proj_lo=proj_lo, **LM)
        yield th.clone(), trial.clone(), lam.clone(), loss_acc.clone(), loss, grad


def run_composition(make, oc, args, lambda0, steps=COMPOSE_STEPS):
    """`make(rows=slice, **kw)` builds a learner of the rows `rows` of `args`; args = (x0 [B, n], hz, taus, wps, iface, theta0 [B, p])."""
    L = make(lm_lambda0=lambda0)
    x0, hz, taus, wps, iface, th0 = args
    hand = lm_by_hand(oc, x0, hz, taus, wps, iface, th0, steps, L.proj_lo, lambda0=lambda0)
    hist, accepted = [], []
    for k in range(steps):
        loss, grad = L.step()
        th, trial, lam, lacc, l2, g2 = next(hand)
        for a, b, nm in ((L.theta, th, "theta"), (L.theta_trial, trial, "theta_trial"), (L.lm_lambda, lam, "lambda"),
                         (L.lm_loss, lacc, "lm_loss"), (loss, l2, "loss"), (grad, g2, "grad")):
            assert H.same(a, b), (k, nm)
        hist.append((L.theta.clone(), L.theta_trial.clone(), L.lm_lambda.clone(), L.lm_loss.clone(), loss.clone(), grad.clone()))
        accepted.append(L.lm_accepted.clone())
        assert L.lm_accepted.dtype == torch.bool and L.normal_matrix.shape == (L.B, th0.shape[1], th0.shape[1])
    lm_loss = torch.stack([h[3] for h in hist])                            # [steps, B]: never increases
    assert bool((lm_loss[1:] <= lm_loss[:-1]).all()) and bool(torch.isfinite(lm_loss[-1]).all())
    acc = torch.stack(accepted)
    assert bool(acc[0].all())                                              # the first finite evaluation is accepted
    assert bool(acc[1:].any()) and bool((~acc[1:]).any()), acc             # a later acceptance and a rejection somewhere
    assert torch.equal(L.normal_matrix, L.normal_matrix.mT)
    # the same seeds in a batch of another size: the same bits
    half = max(1, L.B // 2 - 1)
    Ls = make(rows=slice(0, half), lm_lambda0=lambda0)
    for k in range(steps):
        loss, grad = Ls.step()
        for a, b in zip((Ls.theta, Ls.theta_trial, Ls.lm_lambda, Ls.lm_loss, loss, grad), hist[k]):
            assert H.same(a, b[:half]), k
    return L, hist


def run_skip_unconverged(make, oc, x0, hz):
    """ONE part of the rows forced to status 3 after the learner has moved: that row keeps every word of its LM state beside rows that
    go on, and evaluates the same trial point again.  The iteration cap that splits the batch is found by solving the learner's
    next trial points by hand under falling caps (nothing of the learner is touched by that)."""
    L = make(skip_unconverged=True, lm_lambda0=300.0)         # (damped enough for every row to accept and move twice)
    for _ in range(2):
        L.step()
    assert bool(L.lm_accepted.any()) and not torch.equal(L.theta, L.theta_trial)          # (the rows have moved)
    hz_t = oc._t(hz)
    hz_t = hz_t.expand(L.B).contiguous() if hz_t.dim() == 0 else hz_t
    try:
        frozen = None
        for cap in range(int(L._sol["iters"].max()), 1, -1):
            oc.setSolverOptions(max_iter=cap)
            st = oc.cocSolverBatch(oc._t(x0), hz_t, L.theta_trial.clone(), consts=oc.consts_tensor())["status"]
            if 0 < int((st == 3).sum()) < L.B and bool(((st == 1) | (st == 2))[st != 3].all()):
                frozen = st == 3
                break
        assert frozen is not None, "no iteration cap splits the batch"
        before = tuple(t.clone() for t in (L.theta, L.theta_trial, L.lm_lambda, L.lm_loss, L.normal_matrix))
        L.step()                                                                          # under that cap
        # (the learner also freezes a converged row whose sweeps accepted an interval above their tolerance: frozen is ITS mask)
        assert torch.equal(L._sol["status"] == 3, frozen)
        frozen = ~L._ok
        assert bool(frozen[L._sol["status"] == 3].all()) and bool((~frozen).any()) and L.n_unconverged == int(frozen.sum())
        for a, b in zip((L.theta, L.theta_trial, L.lm_lambda, L.lm_loss, L.normal_matrix), before):
            assert torch.equal(a[frozen], b[frozen])
        assert not bool(L.lm_accepted[frozen].any()) and bool((L.lm_lambda[~frozen] != before[2][~frozen]).all())
    finally:
        oc.setSolverOptions(max_iter=300)
    assert torch.equal(L._eval_point()[frozen], before[1][frozen])                        # the frozen rows evaluate the SAME trial point
    L.step()
    assert bool((L._sol["status"][frozen] != 3).all())                                    # (their solves were continued)
    again = frozen & L._ok
    assert bool(again.any()) and bool((L.lm_lambda[again] != before[2][again]).all())     # ... and are updated again
    return frozen


# "It learns": Examples/pendulum_groundtruth.py -- waypoints sampled from the solve at the true theta (zero residual), 8 seeds
# perturbed by +-30 % (numpy default_rng(LEARN_SEED)), fp64, n_grid 10, default LM values, the example's learning rate 1e-2 for the
# Vanilla learner.  N = LEARN_STEPS = 12 was fixed on the emulator with a margin of two steps: the conditions also hold at N = 10
# (the CPU tier checks both).  Observed on the emulator, loss / initial loss per seed:
#   LM accepted, N = 12:  3.0e-09 7.4e-06 1.3e-05 7.9e-07 1.7e-04 2.6e-06 8.7e-07 2.4e-06      (N = 10: 8.4e-09 ... 4.6e-04, all < 1e-3)
#   Vanilla,     N = 12:  0.46 0.47 0.46 0.24 0.37 0.22 0.19 0.27                              (N = 10: 0.53 0.54 0.52 0.30 0.44 0.28 0.24 0.33)
LEARN_SEED, LEARN_STEPS = 1, 12


def run_learns(make_oc, checkpoints=(LEARN_STEPS,)):
    from lfsd_amd import CPDP
    oc, d = make_oc()
    true = np.asarray(d["true_theta"], dtype=np.float64)
    taus = np.array([0.1, 0.3, 0.6, 0.7, 0.9]) * d["horizon"]
    sol = oc.cocSolverBatch(np.asarray([d["ini_state"]]), d["horizon"], true[None, :])
    wps = oc.sampleBatch(sol, taus)["state"][0][:, d["interface"]].double().cpu().numpy()
    rng = np.random.default_rng(LEARN_SEED)
    seeds = true[None, :] * (1.0 + 0.3 * rng.uniform(-1, 1, (8, true.size)))
    args = (np.tile(d["ini_state"], (8, 1)), d["horizon"], taus, wps, d["interface"], seeds)
    lm = CPDP.SparseDemoLearner(oc, *args, method="LM")
    va = CPDP.SparseDemoLearner(oc, *args, method="Vanilla", learning_rate=d["lr"])
    first = None
    for k in range(max(checkpoints)):
        l, _ = lm.step()
        va.step()
        first = l.clone() if first is None else first
        if k + 1 in checkpoints:
            # the accepted loss after N steps against the Vanilla learner's loss at ITS theta after N steps (one more evaluation)
            lv = va.evaluate(va.theta)[0].clone()
            rel = lm.lm_loss / first
            print("N = %d: LM accepted loss / initial loss" % (k + 1), rel.cpu().numpy())
            print("N = %d: Vanilla loss / initial loss    " % (k + 1), (lv / first).cpu().numpy())
            assert bool((lm.lm_loss <= lv).all()), (k + 1, lm.lm_loss, lv)
            assert int((rel < 1e-3).sum()) >= 4, (k + 1, rel)
