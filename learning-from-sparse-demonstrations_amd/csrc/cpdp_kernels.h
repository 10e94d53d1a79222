// Batched Continuous-PDP kernels for gfx950 (MI355X).
//
// One *lane group* of G lanes (G | 64, one 64-lane wavefront per workgroup) owns
// one trajectory.  Matrices of the per-trajectory recursions are held
// "column per lane": lane j keeps column j of the n x (n+m) shooting
// sensitivity, of V_xx, of the Riccati pair Z = [P W], of the auxiliary state
// X = dx/dtheta.  Quantities every column needs (the current state, costate,
// gains, packed Jacobian/Hessian entries) are group-uniform and are exchanged
// through LDS.  Per-trajectory records in HBM are trajectory-major, so each
// wavefront streams its own contiguous record.
//
// What each kernel replaces in the reference (CPDP/CPDP.py):
//   oc_solve_kernel       COCSys.cocSolver            CPDP.py:92-198  (IPOPT NLP solve ->
//                         batched DDP on the identical RK4 multiple-shooting discretisation;
//                         returns state/control/costate grids, costate == lam_g)
//   aux_riccati_kernel    COCSys.auxSysSolver part 1  CPDP.py:316-338 (Riccati sweep for P, W)
//   aux_forward_kernel    COCSys.auxSysSolver part 2  CPDP.py:340-381 (dx/dtheta forward sweep)
//                         + getloss_*corrections      lib/QuadAlgorithm.py:616-673
//   optimizer_kernel      Vanilla/Nesterov/Adam/Nadam/AMSGrad updates  lib/QuadAlgorithm.py:454-578
//   stop_compact_kernel   the loop's stop test, per seed                lib/QuadAlgorithm.py:239-257
//   grid_curvature_kernel COCSys.interpolation(x, y, 2)                 CPDP.py:388-390 (curvature grids of the cubic
//                         interpolant; aux_*_cubic_kernel are the two sweeps along it)
//   grid_sample_kernel    calling opt_sol(t) / auxsys_sol(t)                   CPDP.py:386-390 (the interpolants at arbitrary times)
//   waypoint_vjp_kernel   `diff_loss += r @ auxsys_sol(tau)` of a user's loss   Examples/*.py getloss_corrections
//   normal_matrix_kernel, lm_step_kernel   no counterpart: a Levenberg-Marquardt outer update from J^T J of the waypoint residuals
//   group_reduce_kernel   no counterpart: loss, gradient and J^T J of several demonstrations summed per seed, in a fixed order
//   waypoint_time_grad_kernel, tau_project_kernel   no counterpart: dLoss/dtau of the waypoint loss and the ordered update of the
//                         times, which the reference invents and then treats as exact (lib/InputWaypoints.py:212-228)
//   time_blocks_kernel, lm_step_times_kernel   no counterpart: the coupling and time blocks of the Gauss-Newton matrix in (theta, tau)
//                         and the Levenberg-Marquardt step with the times eliminated per waypoint
//
// The same source builds for the GPU with hipcc and, with -DLFSD_EMU, for the CPU
// SIMT emulator in tests/emu (test infrastructure; never used by the product path).
//
// Sources: cpdp_common.h (switches, primitives, dense helpers), cpdp_oc.h (OC solve), cpdp_aux.h (auxiliary
// system sweeps + loss), cpdp_opt.h (update rules), cpdp_rows.h (per-seed stop rule, row compaction / gather / scatter),
// cpdp_spline.h (curvature fit of the cubic interpolant), cpdp_sample.h (sampling the interpolants, chain rule of a user's loss),
// cpdp_lm.h (Gauss-Newton matrix of the waypoint loss, Levenberg-Marquardt step), cpdp_groups.h (per-group sums of several
// demonstrations per seed), cpdp_times.h (learnable waypoint times), cpdp_lm_times.h (Levenberg-Marquardt over parameters and times).
#pragma once
#include "cpdp_common.h"
#include "cpdp_oc.h"
#include "cpdp_spline.h"
#include "cpdp_sample.h"
#include "cpdp_aux.h"
#include "cpdp_opt.h"
#include "cpdp_rows.h"
#include "cpdp_lm.h"
#include "cpdp_groups.h"
#include "cpdp_times.h"
#include "cpdp_lm_times.h"
