"""GPU tier of interpolation level 2: the curvature-fit kernel on the device against torch fp64, the level-2 sweeps of the gfx950
libraries against the fp64 oracle integrating along the cubic interpolant (tests/cubic_cases.py), and the batched learner.

The bounds are the level-1 bounds of parity_cases, unchanged.  The same comparisons pass on the SIMT emulator (tests/test_cubic_emu.py;
fp32 there: pendulum)."""
import numpy as np
import pytest
import torch

import lfsd_amd  # noqa: F401
from lfsd_amd import CPDP, models
import cubic_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return models.pendulum(n_grid=10)[0].compile()


def prepare(oc, dtype):
    oc.setDevice("cuda:0", dtype)
    return oc


def torch_curvature(y):
    """The recipe of cubic_cases.curvature_recipe in torch fp64 operations on the device, [B, N+1, C]."""
    y = y.double()
    N = y.shape[1] - 1
    d = y[:, :-2] - 2.0 * y[:, 1:-1] + y[:, 2:]                # d[:, k-1] = d_k
    c = torch.zeros_like(y)
    c[:, 1], c[:, N - 1] = d[:, 0] / 6.0, d[:, N - 2] / 6.0
    if N >= 4:
        K = N - 3                                              # unknowns c_2 .. c_N-2
        A = 4.0 * torch.eye(K, dtype=y.dtype, device=y.device)
        if K > 1:
            i = torch.arange(K - 1, device=y.device)
            A[i, i + 1] = 1.0
            A[i + 1, i] = 1.0
        rhs = d[:, 1:N - 2].clone()
        rhs[:, 0] -= c[:, 1]
        rhs[:, -1] -= c[:, N - 1]
        c[:, 2:N - 1] = torch.linalg.solve(A, rhs)
    c[:, 0] = 2.0 * c[:, 1] - c[:, 2]
    c[:, N] = 2.0 * c[:, N - 1] - c[:, N - 2]
    return c


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n_grid", C.N_GRIDS)
def test_grid_curvature_on_the_device(lib, n_grid, dtype):
    for n_comp in C.N_COMPS:
        for batch in C.BATCHES:
            got, ref = C.run_curvature(lib, "cuda:0", dtype, n_grid, n_comp, batch)
    # the last shape once more against torch fp64 on the device (the same bound)
    y = torch.as_tensor(C.grid_values(batch, n_grid, n_comp)).to(device="cuda:0", dtype=dtype)
    want = torch_curvature(y)
    bound = 64.0 * torch.finfo(dtype).eps * y.double().abs().amax(dim=1, keepdim=True)
    assert bool(((lib.grid_curvature(y).double() - want).abs() <= bound).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_grid_curvature_large_batch(lib, dtype):
    """4099 trajectories x n_grid 50 x 30 components: 480 workgroups, the last one ragged, rows that straddle wavefronts."""
    B, N, Cc = 4099, 50, 30
    t = torch.linspace(0, 1, N + 1, dtype=torch.float64, device="cuda:0")[None, :, None]
    g = torch.Generator(device="cuda:0").manual_seed(5)
    amp = 10.0 ** (4.0 * torch.rand((B, 1, Cc), dtype=torch.float64, device="cuda:0", generator=g) - 2.0)
    y = amp * (torch.sin(3.0 * t + 6.0 * torch.rand((B, 1, Cc), dtype=torch.float64, device="cuda:0", generator=g))
               + 0.05 * torch.randn((B, N + 1, Cc), dtype=torch.float64, device="cuda:0", generator=g))
    y = y.to(dtype).contiguous()
    got = lib.grid_curvature(y)
    want = torch_curvature(y)
    bound = 64.0 * torch.finfo(dtype).eps * y.double().abs().amax(dim=1, keepdim=True)
    err = (got.double() - want).abs()
    print("grid_curvature 4099 x 50 x 30 %s: worst error / bound %.3f" % (dtype, float((err / bound).max())))
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind", ["pendulum", "robotarm", "quadrotor"])
def test_sweeps_match_cubic_oracle(kind, dtype):
    C.sweeps_vs_cubic_oracle(prepare, kind, dtype)


def waypoint_loss_fp64(X, tg, taus, wps, iface, kind):
    """sum_k |x(tau_k)[iface] - w_k|^2 per trajectory along scipy's interpolant of the state grids X [B, N+1, n], fp64; also the
    residuals [B, K, len(iface)]."""
    import scipy.interpolate as sip
    x = sip.interp1d(tg, X, axis=1, kind=kind)(np.asarray(taus, dtype=np.float64))[:, :, list(iface)]
    r = x - np.asarray(wps, dtype=np.float64)[None]
    return (r ** 2).sum(axis=(1, 2)), r


def test_learner_at_level_2_on_quadrotor_seeds():
    """Four steps of SparseDemoLearner(interplation_level=2) on 64 quadrotor seeds (fp32, the benchmark's update rule): finite
    losses, and not the level-1 learner's.

    "Not the level-1 learner's" is checked in two ways.  (a) The first step of both learners solves the same problem at the same
    parameters, so the two losses differ by the interpolant of x(tau) alone, and that difference has an independent reference:
    scipy's linear and not-a-knot interpolants of the learner's own state grids, in fp64.  The product's loss at either level, and
    hence the difference of the two, must meet that reference within the rounding bound of an fp32 evaluation: per component
    |dx| <= 64 eps max|x| (the curvature bound of tests/cubic_cases.run_curvature weighted by |(1-s)^3 - (1-s)| + |s^3 - s| <= 0.77,
    the rest for the linear part), carried through the squares, plus 16 eps of the loss for the sum of its 15 terms.  The check
    has teeth only where the reference difference stands above that bound; it has to for at least half of the seeds.  (b) Over the
    four steps every seed's losses differ from the level-1 run's in at least one bit (the kernels have no atomics, a run repeats
    bit for bit, so a differing bit is a differing computation).

    No lower bound is set on how far a seed's two losses are apart: the loss is a sum of squares, the cubic correction enters it
    with either sign, and over 64 seeds the difference passes through zero.  scipy's own two interpolants of these seeds' first
    grids, in fp64, are 1.4e-5 to 2.5e-4 of the loss apart, median 5.1e-5 (63 of 64 above twice the rounding bound; the kernels
    on the SIMT emulator meet the reference within 0.035 of the bound); at the fourth step an MI355X gave 5.6e-5 to 4e-3, median
    2.2e-3."""
    oc, env, d = models.quadrotor(n_grid=25)
    oc.setDevice("cuda:0", torch.float32)
    rng = np.random.default_rng(3)
    B = 64
    th0 = np.asarray(d["theta0"], dtype=np.float64)[None, :] * (1.0 + 0.1 * rng.standard_normal((B, len(d["theta0"]))))
    th0[:, 0] = np.abs(th0[:, 0]) + 0.2
    x0 = np.tile(np.asarray(d["ini_state"], dtype=np.float64), (B, 1))
    x0[:, :3] += 0.2 * rng.standard_normal((B, 3))
    losses, grids = {}, {}
    for level in (1, 2):
        L = CPDP.SparseDemoLearner(oc, x0, d["horizon"], d["taus"], d["waypoints"], d["interface"], th0, method="Nesterov",
                                   learning_rate=1e-2, interplation_level=level)
        steps = []
        for it in range(4):
            steps.append(L.step()[0].double().cpu())           # (a copy: the learner reuses its loss buffer)
            if it == 0:
                grids[level] = L._sol["state_grid"].double().cpu().numpy()
                taus, wps = L.taus[0].double().cpu().numpy(), L.wps[0].double().cpu().numpy()      # as the kernels read them
        losses[level] = torch.stack(steps)
    assert bool(torch.isfinite(losses[2]).all()) and bool(torch.isfinite(losses[1]).all())
    assert np.array_equal(grids[1], grids[2])                  # the first solve does not depend on the level
    # (a) the first step against scipy's interpolants of the same grids
    X = grids[1]
    tg = np.linspace(0.0, d["horizon"], X.shape[1])
    eps = float(torch.finfo(torch.float32).eps)
    dx = 64.0 * eps * np.abs(X[:, :, list(d["interface"])]).max(axis=1)[:, None, :]        # [B, 1, 3]
    ref, bound = {}, {}
    for level, kind in ((1, "linear"), (2, "cubic")):
        ref[level], r = waypoint_loss_fp64(X, tg, taus, wps, d["interface"], kind)
        bound[level] = (2.0 * np.abs(r) * dx + dx ** 2).sum(axis=(1, 2)) + 16.0 * eps * ref[level]
        err = np.abs(losses[level][0].numpy() - ref[level])
        print("learner level %d, first step: worst |loss - fp64 reference| / bound %.3f" % (level, float((err / bound[level]).max())))
        assert (err <= bound[level]).all(), (level, float((err / bound[level]).max()))
    diff_ref = ref[2] - ref[1]
    diff_got = (losses[2][0] - losses[1][0]).numpy()
    resolved = np.abs(diff_ref) > 2.0 * (bound[1] + bound[2])
    print("learner level 2 - level 1, first step: reference difference / loss min %.2e median %.2e max %.2e; %d of %d seeds above "
          "twice the rounding bound; worst |got - reference| / bound %.3f"
          % (float(np.abs(diff_ref / ref[1]).min()), float(np.median(np.abs(diff_ref / ref[1]))), float(np.abs(diff_ref / ref[1]).max()),
             int(resolved.sum()), B, float((np.abs(diff_got - diff_ref) / (bound[1] + bound[2])).max())))
    print("learner, first step: |reference difference| / (twice the rounding bound) min %.2f median %.2f"
          % (float((np.abs(diff_ref) / (2.0 * (bound[1] + bound[2]))).min()), float(np.median(np.abs(diff_ref) / (2.0 * (bound[1] + bound[2]))))))
    assert 2 * int(resolved.sum()) >= B
    assert (np.abs(diff_got - diff_ref) <= bound[1] + bound[2]).all()
    assert (np.sign(diff_got[resolved]) == np.sign(diff_ref[resolved])).all()
    # (b) every seed: not the level-1 run
    rel = ((losses[2] - losses[1]).abs() / losses[1].abs()).max(dim=0).values
    print("learner level 2 vs 1 over four steps: largest relative loss difference per seed, min %.2e median %.2e"
          % (float(rel.min()), float(rel.median())))
    assert bool((losses[2] != losses[1]).any(dim=0).all())
