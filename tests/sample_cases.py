"""Cases of the sampling kernels (csrc/cpdp_sample.h: lfsd_sample_grid, lfsd_waypoint_vjp) and of the user-written losses built on
them, shared by the CPU tier (kernels through the SIMT emulator, tests/test_sample_emu.py) and the -m gpu tier
(tests/test_sample_gpu.py): shapes, inputs, fp64 references and the bounds.

References.  The interpolation formula of include/lfsd_cpdp.h restated in fp64 (torch, on the device the kernel ran on; the interval is
found in fp64 from the kernel's own inputs cast up), itself cross-checked against scipy's interp1d -- linear, and kind='cubic' at the five
interior fractions of every interval as cubic_cases.check_recipe_against_scipy does.

Bounds (derived, eps of the kernel's dtype).
  Sampling, per (trajectory, component):  4 (n_grid + 3) eps (max_k |y_k| + 2 max_k |c_k|), the c term only with a curvature grid.
    h = horizon / N, k h, the subtraction and the division put at most (N + 1.5) eps on s (t <= N h, so the absolute error of
    t - k h is up to N eps h); the linear part moves by |y_k+1 - y_k| <= 2 max|y| per unit of s, plus three roundings of its own;
    the cubic weights have |w'| <= 2 and |w| < 0.39 each.  A factor 2 covers the fp64 reference's own rounding in the fp64 case.
    An interval index that rounds across a node is harmless: both interpolants are continuous there.
  Vjp, per (trajectory, parameter):  sum_{k,e} |r_ke| 4 (N + 3) eps max_nodes |A_qe|  +  (K (n + m) + 2) eps sum_{k,e} |r_ke A_qe(tau_k)|:
    the sampling bound carried through the dot product plus the forward error of a dot product of K (n + m) terms."""
import numpy as np
import scipy.interpolate as sip
import torch

import cubic_cases as CC

N_GRIDS = (3, 8, 50)
N_COMPS = (1, 13, 91)               # 13: a state grid of the quadrotor; 91 = 7 x 13: its auxX_grid
N_TIMES = (1, 5, 101)               # 5: the waypoints of the examples; 101: opt_sol(linspace(0, T, 101)), lib/QuadAlgorithm.py:309
BATCHES_EMU = (1, 67)
BATCHES_GPU = (1, 67, 4099)         # 4099: a ragged last workgroup, rows that straddle wavefronts
VJP_DIMS = ((2, 1, 3), (13, 4, 7), (13, 3, 12))      # (n, m, p): pendulum, quadrotor, rocket-like
VJP_TIMES = (1, 5, 17)
VJP_N_GRIDS = (3, 50)
KINDS = 6                           # time kinds below


def eps_of(dtype):
    return float(torch.finfo(dtype).eps)


def make_times(hz, n_grid, n_times, per_traj, seed=0, offset=0):
    """Sampling times in the dtype of ``hz`` [B]: [B, K] or -- shared by the batch, built on the SHORTEST horizon so that they lie in
    every trajectory's range -- [K].  Slot (b K + j + offset) mod 6 decides the kind: 0, exactly the horizon, an exact node k h (as
    the kernel forms it), the next float below a node, two interior points."""
    dt, dev = hz.dtype, hz.device
    B = hz.shape[0]
    g = torch.Generator().manual_seed(10007 * n_grid + 101 * n_times + B + seed)
    base = hz if per_traj else hz.min().reshape(1)
    R = base.shape[0]
    h = base / n_grid                                                   # (rounded in dt, as the kernel does)
    slot = (torch.arange(R * n_times).reshape(R, n_times) + offset) % KINDS
    node = torch.randint(1, n_grid + 1, (R, n_times), generator=g).to(dev)
    frac = torch.rand((R, n_times), generator=g, dtype=torch.float64).to(dev)
    slot = slot.to(dev)
    at_node = (node.to(dt) * h[:, None]).clamp(max=base[:, None])
    below = torch.nextafter(at_node, torch.zeros_like(at_node))
    inner = (frac * base[:, None].double()).to(dt)
    t = torch.where(slot == 0, torch.zeros_like(inner), inner)
    t = torch.where(slot == 1, base[:, None].expand(R, n_times), t)
    t = torch.where(slot == 2, at_node, t)
    t = torch.where(slot == 3, below, t)
    t = t.clamp(min=0).minimum(base[:, None])
    return (t if per_traj else t[0]).contiguous()


def make_horizons(batch, dtype, device, seed=0):
    g = torch.Generator().manual_seed(77 + batch + seed)
    return (0.5 + 2.5 * torch.rand((batch,), generator=g, dtype=torch.float64)).to(device=device, dtype=dtype).contiguous()


def interp_reference(grid, curv, hz, times):
    """fp64 restatement on the inputs' own device: grid / curv [B, N+1, C], hz [B], times [B, K] or [K] -> [B, K, C]."""
    y, t, H = grid.double(), times.double(), hz.double()
    B, N1, C = y.shape
    N = N1 - 1
    if t.dim() == 1:
        t = t.unsqueeze(0).expand(B, -1)
    h = (H / N)[:, None]
    k = torch.floor(t / h).clamp(0, N - 1)
    s = (t - k * h) / h
    k = k.long()
    ia = k[:, :, None].expand(-1, -1, C)
    ya, yb = torch.gather(y, 1, ia), torch.gather(y, 1, ia + 1)
    s = s[:, :, None]
    out = ya + s * (yb - ya)
    if curv is not None:
        c = curv.double()
        out = out + ((1 - s) ** 3 - (1 - s)) * torch.gather(c, 1, ia) + (s ** 3 - s) * torch.gather(c, 1, ia + 1)
    return out


def sampling_bound(grid, curv, dtype):
    """[B, 1, C]"""
    N = grid.shape[1] - 1
    mag = grid.double().abs().amax(dim=1, keepdim=True)
    if curv is not None:
        mag = mag + 2.0 * curv.double().abs().amax(dim=1, keepdim=True)
    return 4.0 * (N + 3) * eps_of(dtype) * mag


def check_reference_against_scipy(n_grid, n_comp=3, batch=2):
    """interp_reference (fp64) is scipy's interp1d: linear everywhere, kind='cubic' at the interior fractions of every interval."""
    y = CC.grid_values(batch, n_grid, n_comp)
    c = CC.curvature_recipe(y)
    H = np.array([1.7, 0.9])[:batch]
    for b in range(batch):
        tg = np.linspace(0.0, H[b], n_grid + 1)
        t = np.concatenate([tg[k] + np.asarray(CC.FRACTIONS) * (tg[1] - tg[0]) for k in range(n_grid)])
        T = lambda a: torch.as_tensor(a)
        for kind, cc in (("linear", None), ("cubic", c)):
            ref = sip.interp1d(tg, y[b], axis=0, kind=kind)(t)
            got = interp_reference(T(y[b:b + 1]), None if cc is None else T(cc[b:b + 1]), T(H[b:b + 1]), T(t)[None])[0].numpy()
            assert np.abs(got - ref).max() <= 1e-12 * np.abs(y[b]).max(), (kind, n_grid, b)


def run_sample(lib, device, dtype, n_grid, n_comp, n_times, batch, cubic, per_traj, offset=0, y64=None):
    """lfsd_sample_grid against the fp64 restatement; returns the worst error / bound.  y64: the grid values, if the caller keeps
    them for several cases of one shape."""
    y64 = CC.grid_values(batch, n_grid, n_comp, seed=3) if y64 is None else y64
    y = torch.as_tensor(y64).to(device=device, dtype=dtype).contiguous()
    hz = make_horizons(batch, dtype, device)
    t = make_times(hz, n_grid, n_times, per_traj, offset=offset)
    curv = lib.grid_curvature(y) if cubic else None
    guard = torch.full((batch * n_times * n_comp + 16,), 12345.0, dtype=dtype, device=device)      # the output sits inside a guard band
    out = guard[8:-8].view(batch, n_times, n_comp)
    res = lib.sample_grid(y, hz, t, curv=curv, out=out)
    assert res.data_ptr() == out.data_ptr()
    assert bool((guard[:8] == 12345.0).all()) and bool((guard[-8:] == 12345.0).all())
    assert bool(torch.isfinite(out).all())
    ref = interp_reference(y, curv, hz, t)
    ratio = float(((out.double() - ref).abs() / sampling_bound(y, curv, dtype)).max())
    return ratio, (y, curv, hz, t, out)


# ---- the vjp ------------------------------------------------------------------------------------------------------------
def vjp_inputs(batch, n_grid, n, m, p, K, dtype, device, seed=0):
    g = torch.Generator().manual_seed(31 * batch + 7 * n_grid + n + 3 * K + seed)
    mk = lambda *shape: torch.randn(shape, generator=g, dtype=torch.float64)
    scale = 10.0 ** (3.0 * torch.rand((batch, 1, p, 1), generator=g, dtype=torch.float64) - 1.5)      # parameters of mixed sensitivity
    aX = (scale * mk(batch, n_grid + 1, p, n)).cumsum(dim=1) / (n_grid + 1) ** 0.5
    aU = scale * mk(batch, n_grid + 1, p, m)
    rx, ru = mk(batch, K, n), 0.3 * mk(batch, K, m)
    hz = make_horizons(batch, dtype, device, seed=seed)
    taus = make_times(hz, n_grid, K, True, seed=seed)
    to = lambda a: a.to(device=device, dtype=dtype).contiguous()
    return hz, taus, to(rx), to(ru), to(aX), to(aU)


def vjp_reference(hz, taus, rx, ru, aX, aU):
    """(grad [B, p], bound [B, p] / eps) in fp64 from the kernel's own arrays."""
    B, N1, p, n = aX.shape
    N, K = N1 - 1, taus.shape[1]
    m = aU.shape[3] if aU is not None else 0
    A = aX.double() if aU is None else torch.cat((aX.double(), aU.double()), dim=3)           # [B, N+1, p, n+m]
    r = rx.double() if ru is None else torch.cat((rx.double(), ru.double()), dim=2)           # [B, K, n+m]
    E = A.shape[3]
    At = interp_reference(A.reshape(B, N1, p * E), None, hz, taus).reshape(B, K, p, E)
    terms = r[:, :, None, :] * At                                                              # [B, K, p, E]
    grad = terms.sum(dim=(1, 3))
    Amax = A.abs().amax(dim=1)                                                                 # [B, p, E]
    bound = 4.0 * (N + 3) * (r.abs().sum(dim=1)[:, None, :] * Amax).sum(dim=2) + (K * (n + m) + 2) * terms.abs().sum(dim=(1, 3))
    return grad, bound


def run_vjp(lib, device, dtype, batch, n_grid, n, m, p, K, with_u):
    """lfsd_waypoint_vjp against the fp64 chain rule; a row in batches of 1, 3 and `batch`; a NaN residual row.  Returns the worst
    error / bound."""
    hz, taus, rx, ru, aX, aU = vjp_inputs(batch, n_grid, n, m, p, K, dtype, device)
    if not with_u:
        ru = aU = None
    guard = torch.full((batch * p + 16,), 12345.0, dtype=dtype, device=device)
    out = guard[8:-8].view(batch, p)
    lib.waypoint_vjp(hz, taus, rx, aX, ru=ru, auxU_grid=aU, out=out)
    assert bool((guard[:8] == 12345.0).all()) and bool((guard[-8:] == 12345.0).all())
    ref, bound = vjp_reference(hz, taus, rx, ru, aX, aU)
    ratio = float(((out.double() - ref).abs() / (bound * eps_of(dtype))).max())
    # the same row in batches of 1 and 3 (at another position): identical bits
    at = batch // 2
    sub = lambda t, idx: None if t is None else t[idx].contiguous()
    one = lib.waypoint_vjp(*(sub(t, [at]) for t in (hz, taus, rx, aX)), ru=sub(ru, [at]), auxU_grid=sub(aU, [at]))
    idx3 = [(at + 1) % batch, (at + 2) % batch, at]
    three = lib.waypoint_vjp(*(sub(t, idx3) for t in (hz, taus, rx, aX)), ru=sub(ru, idx3), auxU_grid=sub(aU, idx3))
    assert torch.equal(one[0], out[at]) and torch.equal(three[2], out[at]), (batch, n_grid, n, m, p, K)
    # a NaN residual poisons its own trajectory only
    rx2 = rx.clone()
    rx2[at, K // 2, n - 1] = float("nan")
    got2 = lib.waypoint_vjp(hz, taus, rx2, aX, ru=ru, auxU_grid=aU)
    assert bool(torch.isnan(got2[at]).all())
    keep = torch.ones(batch, dtype=torch.bool, device=device)
    keep[at] = False
    assert torch.equal(got2[keep], out[keep])
    return ratio


# ---- losses -----------------------------------------------------------------------------------------------------------------
def squared_waypoint_loss(idx, wp):
    """The fused loss as a loss_fn (use with grad_scale=0.5: the reference's "no factor 2" convention)."""
    return lambda x_tau, u_tau: ((x_tau[:, :, idx] - wp) ** 2).sum((1, 2))


def fused_reference(sol_X, aX, hz, taus, wps, idx, curv=None):
    """fp64 evaluation of the fused loss / gradient on the learner's own grids: loss [B], grad [B, p], and the bounds / eps
    (loss: the sampling bound through the squares + the sum's forward error; gradient: the vjp bound with the residual's own
    sampling error carried along)."""
    B, N1, n = sol_X.shape
    N, K, p = N1 - 1, taus.shape[1], aX.shape[2]
    x = interp_reference(sol_X, curv, hz, taus)[:, :, idx]                                         # [B, K, q]
    r = x - wps.double()
    loss = (r ** 2).sum(dim=(1, 2))
    rx = torch.zeros((B, K, n), dtype=torch.float64, device=sol_X.device)
    rx[:, :, idx] = r
    grad, gb = vjp_reference(hz, taus, rx, None, aX, None)
    mag = sol_X.double().abs().amax(dim=1)
    if curv is not None:
        mag = mag + 2.0 * curv.double().abs().amax(dim=1)
    dx = (4.0 * (N + 3) * mag[:, idx])[:, None, :] + r.abs()                                       # sampling + the subtraction, per eps
    loss_b = (2.0 * r.abs() * dx).sum(dim=(1, 2)) + (K * len(idx) + 2) * loss
    Amax = aX.double().abs().amax(dim=1)[:, :, idx]                                                # [B, p, q]
    grad_b = gb + (dx.sum(dim=1)[:, None, :] * Amax).sum(dim=2)
    return loss, grad, loss_b, grad_b
