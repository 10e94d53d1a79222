"""CPU tier of the user-defined losses (ABI 12): lfsd_sample_grid / lfsd_waypoint_vjp through the SIMT emulator against fp64
references and scipy's interp1d, and the Python layer on them -- COCSys.sampleBatch / sampleAuxBatch, SparseDemoLearner(loss_fn=...),
QuadAlgorithm.run(sample_all=True) -- in fp64 (tests/sample_cases.py: shapes, references, bounds)."""
import ctypes

import numpy as np
import pytest
import scipy.interpolate as sip
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models, runtime
from lfsd_amd.runtime import LfsdError
from conftest import build_emu_library
import cubic_cases as CC
import sample_cases as S

F64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    return runtime.ModelLibrary(build_emu_library(models.pendulum(n_grid=8)[0]))


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_grid", S.N_GRIDS)
def test_reference_is_scipys_interp1d(n_grid):
    S.check_reference_against_scipy(n_grid)


@pytest.mark.parametrize("dtype", [torch.float32, F64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n_grid", S.N_GRIDS)
def test_sample_grid_matches_reference(lib, n_grid, dtype):
    worst = 0.0
    for n_comp in S.N_COMPS:
        for batch in S.BATCHES_EMU:
            y64 = CC.grid_values(batch, n_grid, n_comp, seed=3)
            for n_times in S.N_TIMES:
                for cubic in (False, True):
                    for per_traj in (True, False):
                        for offset in (range(S.KINDS) if batch * n_times < S.KINDS else (0,)):
                            ratio, _ = S.run_sample(lib, "cpu", dtype, n_grid, n_comp, n_times, batch, cubic, per_traj, offset, y64=y64)
                            assert ratio <= 1.0, (n_grid, n_comp, batch, n_times, cubic, per_traj, offset, ratio)
                            worst = max(worst, ratio)
    print("sample_grid %s n_grid %d: worst error / bound %.3f" % (dtype, n_grid, worst))


@pytest.mark.parametrize("n_grid", S.N_GRIDS)
def test_sample_grid_is_scipys_interp1d(lib, n_grid):
    """fp64, straight against scipy: the linear interpolant at the special times, the cubic one (curvature fitted by
    lfsd_grid_curvature: its bound of cubic_cases.run_curvature, 64 eps max|y|, weighted by |wa| + |wb| < 1, is added) at the five
    interior fractions of every interval."""
    B, C = 5, 13
    y = torch.as_tensor(CC.grid_values(B, n_grid, C, seed=3)).contiguous()
    hz = S.make_horizons(B, F64, "cpu")
    t = S.make_times(hz, n_grid, 101, True)
    got = lib.sample_grid(y, hz, t)
    bound = S.sampling_bound(y, None, F64)
    curv = lib.grid_curvature(y)
    fr = torch.cat([(k + torch.tensor(CC.FRACTIONS, dtype=F64)) / n_grid for k in range(n_grid)])
    tc = (hz[:, None] * fr[None, :]).contiguous()
    gotc = lib.sample_grid(y, hz, tc, curv=curv)
    boundc = S.sampling_bound(y, curv, F64) + 64.0 * S.eps_of(F64) * y.abs().amax(dim=1, keepdim=True)
    worst = 0.0
    for b in range(B):
        tg = np.linspace(0.0, float(hz[b]), n_grid + 1)
        tg[-1] = float(hz[b])
        ref = sip.interp1d(tg, y[b].numpy(), axis=0)(t[b].numpy())
        refc = sip.interp1d(tg, y[b].numpy(), axis=0, kind="cubic")(tc[b].numpy())
        r1 = float((np.abs(got[b].numpy() - ref) / bound[b].numpy()).max())
        r2 = float((np.abs(gotc[b].numpy() - refc) / boundc[b].numpy()).max())
        assert r1 <= 1.0 and r2 <= 1.0, (n_grid, b, r1, r2)
        worst = max(worst, r1, r2)
    print("sample_grid fp64 n_grid %d against scipy: worst error / bound %.3f" % (n_grid, worst))


def test_nan_time_gives_a_nan_row(lib):
    for dtype in (torch.float32, F64):
        for cubic in (False, True):
            ratio, (y, curv, hz, t, out) = S.run_sample(lib, "cpu", dtype, 8, 13, 5, 4, cubic, True)
            t2 = t.clone()
            t2[2, 3] = float("nan")
            got = lib.sample_grid(y, hz, t2, curv=curv)
            assert bool(torch.isnan(got[2, 3]).all())
            got[2, 3] = out[2, 3]
            assert torch.equal(got, out)


@pytest.mark.parametrize("dtype", [torch.float32, F64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("dims", S.VJP_DIMS, ids=lambda d: "n%dm%dp%d" % d)
def test_waypoint_vjp_matches_chain_rule(lib, dims, dtype):
    n, m, p = dims
    worst = 0.0
    for n_grid in S.VJP_N_GRIDS:
        for K in S.VJP_TIMES:
            for batch in S.BATCHES_EMU:
                for with_u in (True, False):
                    ratio = S.run_vjp(lib, "cpu", dtype, batch, n_grid, n, m, p, K, with_u)
                    assert ratio <= 1.0, (dims, n_grid, K, batch, with_u, ratio)
                    worst = max(worst, ratio)
    print("waypoint_vjp %s (n, m, p) = %s: worst error / bound %.3f" % (dtype, dims, worst))


def test_entry_points_refuse_bad_arguments(lib):
    """Every LFSD_EINVAL case of include/lfsd_cpdp.h, on host dummies: refused before any launch."""
    L = lib.lib
    buf = (ctypes.c_double * 4096)()
    base = ctypes.cast(buf, ctypes.c_void_p).value
    P = lambda i: ctypes.c_void_p(base + 4096 * i)
    g, c, h, t, o = P(0), P(1), P(2), P(3), P(4)
    ok = dict(dtype=1, batch=1, n_grid=3, n_comp=2, n_times=2, per=1, grid=g, curv=c, hz=h, times=t, out=o)
    call = lambda **kw: L.lfsd_sample_grid(*[dict(ok, **kw)[k] for k in ("dtype", "batch", "n_grid", "n_comp", "n_times", "per", "grid",
                                                                          "curv", "hz", "times", "out")], None)
    buf[3 * 512] = 0.5; buf[3 * 512 + 1] = 0.5; buf[2 * 512] = 1.0          # (a valid call does run on these host arrays: emulator)
    assert call() == 0 and call(curv=None, n_grid=1) == 0
    for bad in (dict(grid=None), dict(hz=None), dict(times=None), dict(out=None), dict(batch=0), dict(batch=-3), dict(n_comp=0),
                dict(n_times=0), dict(n_grid=0), dict(n_grid=2), dict(curv=None, n_grid=0), dict(out=g), dict(out=c), dict(out=h),
                dict(out=t), dict(out=ctypes.c_void_p(base + 8)), dict(dtype=2), dict(dtype=-1), dict(per=2),
                dict(batch=2 ** 31 - 1, n_times=2 ** 20, n_comp=2 ** 20)):
        assert call(**bad) == -1, bad
    hz, ta, rx, ru, aX, aU, gr = (P(i) for i in range(7))
    okv = dict(dtype=1, batch=1, n_grid=3, n=2, m=1, p=3, K=2, hz=hz, taus=ta, rx=rx, ru=ru, aX=aX, aU=aU, grad=gr)
    callv = lambda **kw: L.lfsd_waypoint_vjp(*[dict(okv, **kw)[k] for k in ("dtype", "batch", "n_grid", "n", "m", "p", "K", "hz", "taus",
                                                                            "rx", "ru", "aX", "aU", "grad")], None)
    buf[0] = 1.0
    assert callv() == 0 and callv(ru=None, aU=None) == 0
    for bad in (dict(hz=None), dict(taus=None), dict(rx=None), dict(aX=None), dict(grad=None), dict(ru=None), dict(aU=None),
                dict(batch=0), dict(n_grid=0), dict(n=0), dict(m=0), dict(p=0), dict(K=0), dict(K=-1), dict(grad=hz), dict(grad=ta),
                dict(grad=rx), dict(grad=ru), dict(grad=aX), dict(grad=aU), dict(dtype=5),
                dict(batch=2 ** 31 - 1, p=2 ** 20)):
        assert callv(**bad) == -1, bad
    # the Python binding: shapes, dtypes, the pair ru / auxU_grid
    y, hzt = torch.zeros(2, 4, 3, dtype=F64), torch.ones(2, dtype=F64)
    with pytest.raises(LfsdError):
        lib.sample_grid(y, hzt, torch.zeros(3, 5, dtype=F64))
    with pytest.raises(LfsdError):
        lib.sample_grid(y[:, :3].contiguous(), hzt, torch.zeros(5, dtype=F64), curv=y[:, :3].contiguous())
    with pytest.raises(LfsdError):
        lib.sample_grid(y, hzt.float(), torch.zeros(5, dtype=F64))
    with pytest.raises(LfsdError):
        lib.waypoint_vjp(hzt, torch.zeros(2, 5, dtype=F64), torch.zeros(2, 5, 2, dtype=F64), torch.zeros(2, 4, 3, 2, dtype=F64),
                         ru=torch.zeros(2, 5, 1, dtype=F64))


def test_product_library_refuses_cpu_tensors():
    lib = models.pendulum()[0].compile()
    y, hz = torch.zeros(2, 4, 3), torch.ones(2)
    with pytest.raises(LfsdError):
        lib.sample_grid(y, hz, torch.zeros(5))
    with pytest.raises(LfsdError):
        lib.waypoint_vjp(hz, torch.zeros(2, 5), torch.zeros(2, 5, 2), torch.zeros(2, 4, 3, 2))


# ---- 2. the Python layer (fp64; pendulum n_grid 8, quadrotor n_grid 10; batch 3) ----------------------------------------------
_CASES = {}


def case(emu, kind):
    if kind not in _CASES:
        c = CC.SWEEP_CASES[kind]
        oc, env, d = models.ZOO[kind](n_grid=c["n_grid"])
        emu(oc)
        oc.setDevice(dtype=F64)
        th = np.asarray(c["thetas"], dtype=np.float64)
        x0 = np.tile(d["ini_state"], (3, 1))
        sol = oc.cocSolverBatch(x0, d["horizon"], th)
        assert set(sol["status"].tolist()) <= {1, 2}
        _CASES[kind] = (oc, d, c, th, x0, sol)
    return _CASES[kind]


@pytest.mark.parametrize("kind", ["pendulum", "quadrotor"])
def test_sample_batch_is_the_interpolant_of_each_row(emu, kind):
    oc, d, c, th, x0, sol = case(emu, kind)
    N, H = c["n_grid"], d["horizon"]
    tg = np.linspace(0, H, N + 1)
    times = np.concatenate(([0.0, H, tg[3], np.nextafter(tg[3], 0.0)], np.asarray(c["taus"], dtype=np.float64), np.linspace(0, H, 17)))
    grids = torch.cat([sol[k] for k in ("state_grid", "control_grid", "costate_grid")], dim=2)
    for level in (1, 2):
        s = oc.sampleBatch(sol, times, level)
        got = torch.cat([s[k] for k in ("state", "control", "costate")], dim=2)
        assert tuple(got.shape) == (3, len(times), grids.shape[2])
        curv = oc.compile().grid_curvature(grids.contiguous()) if level == 2 else None
        bound = S.sampling_bound(grids, curv, F64)
        if level == 2:
            bound = bound + 64.0 * S.eps_of(F64) * grids.abs().amax(dim=1, keepdim=True)      # (the curvature fit: cubic_cases.run_curvature)
        for b in range(3):
            ref = oc.interpolation(tg, grids[b].numpy(), level)(times)
            ratio = float((np.abs(got[b].numpy() - ref) / bound[b].numpy()).max())
            print("sampleBatch %s level %d row %d: worst error / bound %.3f" % (kind, level, b, ratio))
            assert ratio <= 1.0
    # per-trajectory times, and curvature grids handed in with the solution
    tt = torch.as_tensor(np.stack([times, times[::-1], 0.5 * times])).contiguous()
    s2 = oc.sampleBatch(dict(sol, curvature=tuple(oc.compile().grid_curvature(sol[k]) for k in ("state_grid", "control_grid", "costate_grid"))), tt, 2)
    shared = oc.sampleBatch(sol, times, 2)
    assert torch.equal(s2["state"][0], shared["state"][0]) and torch.equal(s2["costate"][1].flip(0), shared["costate"][1])
    # range validation: scipy's ValueError, unless switched off
    for bad in ([-1e-3, 0.5 * H], [0.5 * H, H * (1 + 1e-6)]):
        with pytest.raises(ValueError):
            oc.sampleBatch(sol, bad)
        assert bool(torch.isfinite(oc.sampleBatch(sol, bad, validate=False)["state"]).all())
    with pytest.raises(LfsdError):
        oc.sampleBatch(sol, times, 3)


@pytest.mark.parametrize("kind", ["pendulum", "quadrotor"])
def test_sample_aux_batch_is_auxsys_sol_of_each_row(emu, kind):
    oc, d, c, th, x0, sol = case(emu, kind)
    lib = oc.compile()
    n, m, p = lib.n_state, lib.n_control, lib.n_auxvar
    N, H = c["n_grid"], d["horizon"]
    tg = np.linspace(0, H, N + 1)
    times = np.concatenate(([0.0, H, tg[2]], np.asarray(c["taus"], dtype=np.float64), np.linspace(0, H, 7)))
    aux = oc.auxSysSolverBatch(sol, want_grids=True)
    s = oc.sampleAuxBatch(aux, sol["horizon"], times)
    assert tuple(s["dx"].shape) == (3, len(times), p, n) and tuple(s["du"].shape) == (3, len(times), p, m)
    bx = S.sampling_bound(aux["auxX_grid"].reshape(3, N + 1, p * n), None, F64).reshape(3, 1, p, n)
    bu = S.sampling_bound(aux["auxU_grid"].reshape(3, N + 1, p * m), None, F64).reshape(3, 1, p, m)
    for b in range(3):
        grids = np.concatenate([sol[k][b].numpy() for k in ("state_grid", "control_grid", "costate_grid")], axis=1)
        auxsys_sol = oc.auxSysSolver(tg, oc.interpolation(tg, grids), th[b])
        ref = auxsys_sol(times)                                       # [K, n p + m p], dx/dtheta as [n][p] row-major (CPDP.py:381)
        # The one-trajectory call runs the sweeps again on a batch of one: its grid values are this row's up to the sweeps' own
        # row-against-batch-of-one parity (a few ulp on the quadrotor), and two linear interpolants are no further apart than their
        # nodes.  That nodal difference -- of existing code, taken from the grids the one-trajectory call kept -- is added per component.
        dX = (oc.last_aux["auxX_grid"][0] - aux["auxX_grid"][b]).abs().amax(dim=0, keepdim=True).numpy()
        dU = (oc.last_aux["auxU_grid"][0] - aux["auxU_grid"][b]).abs().amax(dim=0, keepdim=True).numpy()
        assert dX.max() <= 1e-12 * float(aux["auxX_grid"][b].abs().max())
        ex = np.abs(s["dx"][b].numpy().transpose(0, 2, 1).reshape(len(times), n * p) - ref[:, :n * p])
        eu = np.abs(s["du"][b].numpy().transpose(0, 2, 1).reshape(len(times), m * p) - ref[:, n * p:])
        rx = float((ex / (bx[b].numpy() + dX).transpose(0, 2, 1).reshape(1, n * p)).max())
        ru = float((eu / (bu[b].numpy() + dU).transpose(0, 2, 1).reshape(1, m * p)).max())
        # ... and with the transposition of CPDP.py:381 applied to this row's own grids, the sampling bound alone
        own = oc.interpolation(tg, np.concatenate((aux["auxX_grid"][b].numpy().transpose(0, 2, 1).reshape(N + 1, n * p),
                                                   aux["auxU_grid"][b].numpy().transpose(0, 2, 1).reshape(N + 1, m * p)), axis=1))(times)
        ox = np.abs(s["dx"][b].numpy().transpose(0, 2, 1).reshape(len(times), n * p) - own[:, :n * p])
        ou = np.abs(s["du"][b].numpy().transpose(0, 2, 1).reshape(len(times), m * p) - own[:, n * p:])
        floor = lambda v: v + 1e-300
        assert float((ox / floor(bx[b].numpy().transpose(0, 2, 1).reshape(1, n * p))).max()) <= 1.0
        assert float((ou / floor(bu[b].numpy().transpose(0, 2, 1).reshape(1, m * p))).max()) <= 1.0
        print("sampleAuxBatch %s row %d: worst error / bound dx %.3f du %.3f" % (kind, b, rx, ru))
        assert rx <= 1.0 and ru <= 1.0
    with pytest.raises(ValueError):
        oc.sampleAuxBatch(aux, sol["horizon"], [1.5 * H])
    oc.sampleAuxBatch(aux, sol["horizon"], [1.5 * H], validate=False)
    with pytest.raises(LfsdError):
        oc.sampleAuxBatch(oc.auxSysSolverBatch(sol), sol["horizon"], times)


def _learners(oc, d, c, th, x0, level=1, **kw):
    fused = CPDP.SparseDemoLearner(oc, x0, d["horizon"], c["taus"], c["wps"], d["interface"], th, interplation_level=level, **kw)
    idx = list(d["interface"])
    cust = CPDP.SparseDemoLearner(oc, x0, d["horizon"], c["taus"], None, None, th, interplation_level=level,
                                  loss_fn=S.squared_waypoint_loss(idx, fused.wps), grad_scale=0.5, **kw)
    return fused, cust, idx


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("kind", ["pendulum", "quadrotor"])
def test_squared_loss_fn_is_the_fused_loss(emu, kind, level):
    oc, d, c, th, x0, sol = case(emu, kind)
    fused, cust, idx = _learners(oc, d, c, th, x0, level)
    lf, gf = fused.evaluate(fused.theta)
    lc, gc = cust.evaluate(cust.theta)
    assert torch.equal(fused._sol["state_grid"], cust._sol["state_grid"])
    curv = cust._aux["curvature"][0] if level == 2 else None
    rl, rg, bl, bg = S.fused_reference(cust._sol["state_grid"], cust._aux["auxX_grid"], cust.hz, cust.taus, fused.wps, idx, curv)
    eps = S.eps_of(F64)
    floor = lambda b: b * eps + 1e-300
    ratios = dict(loss_fn=float(((lc - rl).abs() / floor(bl)).max()), fused=float(((lf - rl).abs() / floor(bl)).max()),
                  paths=float(((lc - lf).abs() / floor(2 * bl)).max()), grad_loss_fn=float(((gc - rg).abs() / floor(bg)).max()),
                  grad_fused=float(((gf - rg).abs() / floor(bg)).max()), grad_paths=float(((gc - gf).abs() / floor(2 * bg)).max()))
    print("fused parity %s level %d: error / bound %s" % (kind, level, {k: round(v, 3) for k, v in ratios.items()}))
    assert max(ratios.values()) <= 1.0, ratios


def test_loss_fn_learner_follows_the_fused_learner(emu):
    """Five Nesterov steps in fp64: theta of the loss_fn learner stays within 1e-8 relative of the fused learner's (the traces differ by
    roundings of 1e-16 per step; five steps do not amplify them by 1e8)."""
    oc, d, c, th, x0, sol = case(emu, "pendulum")
    fused, cust, idx = _learners(oc, d, c, th, x0, method="Nesterov", learning_rate=1e-2)
    for it in range(5):
        lf, _ = fused.step()
        lc, _ = cust.step()
        rel = float(((cust.theta - fused.theta).abs() / fused.theta.abs().amax(dim=1, keepdim=True)).max())
        print("step %d: max relative theta difference %.3e, loss difference %.3e" % (it + 1, rel, float((lc - lf).abs().max())))
        assert rel <= 1e-8
    assert not torch.equal(fused.theta, torch.as_tensor(th))
    # warm starts and the true-loss flag go through the same evaluate()
    a = CPDP.SparseDemoLearner(oc, x0, d["horizon"], c["taus"], None, None, th, method="Nesterov", warm_start=True,
                               true_loss_print_flag=True, loss_fn=S.squared_waypoint_loss(idx, fused.wps), grad_scale=0.5)
    b = CPDP.SparseDemoLearner(oc, x0, d["horizon"], c["taus"], c["wps"], d["interface"], th, method="Nesterov", warm_start=True,
                               true_loss_print_flag=True)
    for it in range(2):
        la, lb = a.step()[0], b.step()[0]
    assert torch.allclose(la, lb, rtol=1e-9) and torch.allclose(a.theta, b.theta, rtol=1e-8)


def test_a_loss_the_fused_path_cannot_express(emu):
    """Ragged demonstrations as masks, a Huber distance and a control term: the gradient is the numpy chain rule on the product's own
    sensitivity grids, within the vjp bound; a masked-out waypoint's target does not matter."""
    oc, d, c, th, x0, sol = case(emu, "pendulum")
    taus = [0.1, 0.3, 0.6, 0.7, 0.9]
    wps = torch.tensor([[0.4], [1.2], [2.1], [2.4], [2.9]], dtype=F64)
    W = torch.tensor([[1, 1, 1, 1, 1], [0, 0, 1, 0, 0], [1, 0, 1, 1, 0]], dtype=F64)       # all / a single waypoint / some
    lam = 0.05
    state = {}

    def make(targets, delta):
        def loss_fn(x_tau, u_tau):
            r = x_tau[:, :, 0] - targets[None, :, 0]
            hub = torch.where(r.abs() <= delta, 0.5 * r * r, delta * (r.abs() - 0.5 * delta))
            state["x"], state["u"] = x_tau.detach(), u_tau.detach()
            return (W * hub).sum(dim=1) + lam * (u_tau ** 2).sum(dim=(1, 2))
        return loss_fn
    probe = CPDP.SparseDemoLearner(oc, x0, d["horizon"], taus, None, None, th, loss_fn=make(wps, 1e9))
    probe.evaluate(probe.theta)
    r0 = (state["x"][:, :, 0] - wps[None, :, 0]).abs()
    delta = float(r0[W > 0].median())
    assert bool((r0[W > 0] < delta).any()) and bool((r0[W > 0] > delta).any())        # both branches of the Huber loss
    L = CPDP.SparseDemoLearner(oc, x0, d["horizon"], taus, None, None, th, loss_fn=make(wps, delta))
    loss, grad = L.evaluate(L.theta)
    x, u = state["x"].numpy(), state["u"].numpy()
    r = x[:, :, 0] - wps.numpy()[None, :, 0]
    hub = np.where(np.abs(r) <= delta, 0.5 * r * r, delta * (np.abs(r) - 0.5 * delta))
    assert np.allclose(loss.numpy(), (W.numpy() * hub).sum(1) + lam * (u ** 2).sum((1, 2)), rtol=1e-13)
    rx = np.zeros_like(x)
    rx[:, :, 0] = W.numpy() * np.clip(r, -delta, delta)
    ru = 2.0 * lam * u
    ref, bound = S.vjp_reference(L.hz, L.taus, torch.as_tensor(rx), torch.as_tensor(ru), L._aux["auxX_grid"], L._aux["auxU_grid"])
    ratio = float(((grad - ref).abs() / (bound * S.eps_of(F64))).max())
    print("custom loss: gradient against the numpy chain rule, worst error / bound %.3f" % ratio)
    assert ratio <= 1.0 and bool((grad.abs().amax(dim=1) > 0).all())
    # ... and against dx/dtheta(tau), du/dtheta(tau) sampled and contracted on the host
    sa = oc.sampleAuxBatch(L._aux, L.hz, L.taus)
    host = np.einsum("bki,bkqi->bq", rx, sa["dx"].numpy()) + np.einsum("bkj,bkqj->bq", ru, sa["du"].numpy())
    assert float((np.abs(grad.numpy() - host) / (2 * bound.numpy() * S.eps_of(F64))).max()) <= 1.0
    # a masked-out waypoint: another target, the same loss and gradient, bit for bit
    wps2 = wps.clone()
    wps2[0, 0] += 3.0            # masked in rows 1; used in rows 0 and 2
    wps2[4, 0] -= 2.0            # masked in rows 1 and 2
    L2 = CPDP.SparseDemoLearner(oc, x0, d["horizon"], taus, None, None, th, loss_fn=make(wps2, delta))
    loss2, grad2 = L2.evaluate(L2.theta)
    assert torch.equal(loss2[1], loss[1]) and torch.equal(grad2[1], grad[1])
    assert not torch.equal(loss2[0], loss[0]) and not torch.equal(grad2[2], grad[2])
    # a loss without a control term: no ru, the control grids are not read
    L3 = CPDP.SparseDemoLearner(oc, x0, d["horizon"], taus, None, None, th, loss_fn=lambda xt, ut: (W * (xt[:, :, 0] - wps[None, :, 0]) ** 2).sum(1))
    l3, g3 = L3.evaluate(L3.theta)
    r3 = np.zeros_like(x)
    r3[:, :, 0] = 2.0 * W.numpy() * r
    ref3, b3 = S.vjp_reference(L3.hz, L3.taus, torch.as_tensor(r3), None, L3._aux["auxX_grid"], None)
    assert float(((g3 - ref3).abs() / (b3 * S.eps_of(F64))).max()) <= 1.0
    with pytest.raises(LfsdError):
        bad = CPDP.SparseDemoLearner(oc, x0, d["horizon"], taus, None, None, th, loss_fn=lambda xt, ut: xt.sum())
        bad.evaluate(bad.theta)


def test_loss_fn_in_shared_mode_and_with_skipped_rows(emu, monkeypatch):
    oc, d, c, th, x0, sol = case(emu, "pendulum")
    wp = torch.tensor(c["wps"], dtype=F64)
    fn = S.squared_waypoint_loss(list(d["interface"]), wp[None])
    mk = lambda **kw: CPDP.SparseDemoLearner(oc, x0, d["horizon"], c["taus"], None, None, kw.pop("theta", th), loss_fn=fn, grad_scale=0.5, **kw)
    # shared mode sums over the batch
    sh = mk(theta=th[:1], mode="shared")
    ls, gs = sh.step()
    ind = mk(theta=np.tile(th[:1], (3, 1)))
    li, gi = ind.evaluate(ind.theta)
    assert ls.shape == (1,) and gs.shape == (1, 3)
    assert torch.allclose(ls, li.sum().reshape(1), rtol=1e-13) and torch.allclose(gs, gi.sum(dim=0, keepdim=True), rtol=1e-12)
    assert sh.n_unconverged == 0
    # a row forced to FAILED: skipped by the sweeps (NaN grids -> NaN loss and gradient), masked by skip_unconverged
    real = oc.cocSolverBatch

    def failing(*a, **kw):
        s = real(*a, **kw)
        s["status"][1] = 4
        return s
    monkeypatch.setattr(oc, "cocSolverBatch", failing)
    raw = mk(skip_unconverged=False)
    lr_, gr_ = raw.evaluate(raw.theta)
    assert bool(torch.isnan(lr_[1])) and bool(torch.isnan(gr_[1]).all()) and bool(torch.isfinite(lr_[[0, 2]]).all())
    assert bool(torch.isfinite(gr_[[0, 2]]).all())
    sk = mk(skip_unconverged=True)
    theta0 = sk.theta.clone()
    l, g = sk.step()
    assert sk._ok.tolist() == [True, False, True] and sk.n_unconverged == 1
    assert bool((g[1] == 0).all()) and torch.equal(sk.theta[1], theta0[1]) and not torch.equal(sk.theta[0], theta0[0])
    sh2 = mk(theta=th[:1], mode="shared")
    l2, g2 = sh2.step()
    assert bool(torch.isfinite(l2).all()) and bool(torch.isfinite(g2).all()) and sh2.n_unconverged == 1
    assert torch.allclose(l2, (li[0] + li[2]).reshape(1), rtol=1e-13)
    monkeypatch.undo()
    with pytest.raises(LfsdError, match="stop_rule"):
        mk(stop_rule=dict(loss=0.9, grad_norm=0.05))
    with pytest.raises(LfsdError):
        CPDP.SparseDemoLearner(oc, x0, d["horizon"], c["taus"], None, None, th, loss_fn=3)


def test_default_learner_launches_what_it_did(emu):
    """loss_fn=None: the fused path, result for result (the same buffers, no sensitivity grids, no sampling)."""
    oc, d, c, th, x0, sol = case(emu, "pendulum")
    L = CPDP.SparseDemoLearner(oc, x0, d["horizon"], c["taus"], c["wps"], d["interface"], th)
    called = []
    L.event_hook = called.append
    l, g = L.step()
    assert called == ["oc_solve", "aux_riccati", "aux_forward", "update", "end"]
    assert L._aux["auxX_grid"] is None and L.loss_fn is None
    ref = oc.auxSysSolverBatch(oc.cocSolverBatch(x0, d["horizon"], th), c["taus"], c["wps"], d["interface"])
    assert torch.equal(l, ref["loss"]) and torch.equal(g, ref["grad"])


def test_quadalgorithm_samples_all_seeds(emu):
    from lfsd_amd.QuadAlgorithm import QuadAlgorithm, QuadPara, DemoSparse
    from lfsd_amd.JinEnv import QuadStates
    cfg = {"QUAD_AVERAGE_SPEED": 1.0, "LAB_SPACE_LIMIT": {"LIMIT_X": [-3.2, 3.2], "LIMIT_Y": [-1.6, 1.6], "LIMIT_Z": [0.0, 2.2]}}
    ini, goal = QuadStates(position=[-2.0, -1.0, 0.6]), QuadStates(position=[2.5, 1.0, 1.5])
    lib_path = build_emu_library(models.quadrotor(n_grid=6)[0])
    demo = DemoSparse(waypoints=[[-1.0, -0.5, 0.9], [0.5, 0.2, 1.2], [1.8, 0.8, 1.4]], time_list=[0.25, 0.5, 0.75], time_horizon=1.0)
    base = np.array([1, 0.1, 0.1, 0.1, 0.1, 0.1, -1], dtype=float)

    def run(**kw):
        Q = QuadAlgorithm(cfg, QuadPara([1.0, 1.0, 1.0], 1.0, 1.0, 0.02), 6, dtype=F64)
        Q.library = lib_path
        Q.load_optimization_function({"learning_rate": 0.01, "iter_num": 1, "method": "Vanilla"})
        return Q, Q.run(ini, goal, demo, ObsList=[], initial_parameters=np.stack([base, base * 1.3]), **kw)
    Q, res = run(sample_all=True)
    assert res["opt_state_traj_all"].shape == (2, 101, 13) and res["opt_control_traj_all"].shape == (2, 101, 4)
    # row 0 is the reference's own key: the same grids (a batch row equals a batch of one on the emulator in fp64), sampled by the
    # kernel instead of scipy -- the sampling bound
    sol = Q.oc.last_solution
    for key, gk in (("opt_state_traj", "state_grid"), ("opt_control_traj", "control_grid")):
        bound = S.sampling_bound(sol[gk], None, F64)[0].numpy()
        ratio = float((np.abs(res[key + "_all"][0] - res[key]) / bound).max())
        print("sample_all %s: row 0 against the one-trajectory result, worst error / bound %.3f" % (key, ratio))
        assert ratio <= 1.0
    assert np.abs(res["opt_state_traj_all"][1] - res["opt_state_traj_all"][0]).max() > 1e-3
    _, plain = run()
    assert "opt_state_traj_all" not in plain and "opt_control_traj_all" not in plain
    assert np.array_equal(plain["opt_state_traj"], res["opt_state_traj"]) and np.array_equal(plain["parameter_trace"], res["parameter_trace"])
