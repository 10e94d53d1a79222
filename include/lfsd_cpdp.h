/* lfsd_cpdp.h — C ABI of the MI355X-native batched Continuous-PDP solver.
 *
 * One shared library is built per optimal-control model (dimensions and the
 * model's derivative code are compiled in); every library exports exactly the
 * symbols below.  All array arguments are DEVICE pointers (hipMalloc'd memory,
 * e.g. torch tensors' data_ptr()), row-major, batch-major; `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  dtype: 0 = float32,
 * 1 = float64 (the arithmetic type of every array in the call).
 * Every function returns 0 on success, a negative LFSD_E* code on bad
 * arguments, or a positive hipError_t if a launch failed.
 *
 * Reference interface each entry point replaces (wanxinjin/Learning-from-
 * Sparse-Demonstrations @ v1):
 *   lfsd_coc_solve        CPDP/CPDP.py:92-198   COCSys.cocSolver (and :486-594 time-varying)
 *   lfsd_aux_solve        CPDP/CPDP.py:301-381  COCSys.auxSysSolver (and :706-786)   [= lfsd_aux_riccati + lfsd_aux_forward]
 *                         + lib/QuadAlgorithm.py:616-673 getloss_pos_corrections / getloss_corrections
 *                           (Examples/*.py getloss_corrections)
 *   lfsd_optimizer_step   lib/QuadAlgorithm.py:454-578 Vanilla/Nesterov/Adam/Nadam/AMSGrad
 *   lfsd_lookahead        lib/QuadAlgorithm.py:478 (Nesterov look-ahead point)
 *   lfsd_stop_compact     lib/QuadAlgorithm.py:239-257 (the learning loop's stop test, per seed; ABI 10)
 *   lfsd_gather_rows / lfsd_scatter_rows   the dense batch of the seeds still learning (ABI 10)
 *   lfsd_grid_curvature   CPDP/CPDP.py:388-390  COCSys.interpolation(x, y, 2): the cubic interpolant of a grid (ABI 11)
 *   lfsd_aux_*_cubic      CPDP/CPDP.py:301-381  auxSysSolver handed that interpolant (interplation_level=2; ABI 11)
 *   lfsd_sample_grid      CPDP/CPDP.py:386-390  calling opt_sol(t) / auxsys_sol(t): Examples/rocket_groundtruth.py:75-84
 *                         true_opt_sol(taus), lib/QuadAlgorithm.py:306-317 opt_sol(linspace(0, T, 101)) (ABI 12)
 *   lfsd_waypoint_vjp     the `diff_loss += r @ auxsys_sol(tau)` of a user-written loss: Examples/pendulum_timewarping.py:72-86,
 *                         Examples/rocket_groundtruth.py:45-70, lib/QuadAlgorithm.py:616-673 (ABI 12)
 *   lfsd_optimizer_step_rows / lfsd_lookahead_rows   the same update rules with the rule and its hyper-parameters PER ROW: the runs
 *                         of test/opt_methods_comparison.py and test/*_learning_rate_comparison.py as one batch (ABI 13)
 *   lfsd_trace_append     loss_trace / parameter_trace of lib/QuadAlgorithm.py:244-252, kept on the device (ABI 13)
 *   lfsd_normal_matrix / lfsd_lm_step   no counterpart: a second-order outer update for the sum-of-squares loss of
 *                         lib/QuadAlgorithm.py:616-639, where the reference has the five first-order rules (ABI 14)
 *   lfsd_group_reduce     no counterpart: the reference learns from one demonstration per run (lib/QuadAlgorithm.py:239-257); loss,
 *                         gradient and J^T J of several demonstrations per seed, summed per seed in a fixed order (ABI 15)
 *   lfsd_aux_forward_weighted / lfsd_aux_forward_cubic_weighted / lfsd_normal_matrix_weighted   a weight per waypoint in the loss of
 *                         lib/QuadAlgorithm.py:616-639 (the reference weighs every waypoint equally); with zero weights, demonstrations
 *                         of different lengths in one batch, as Examples/quad_example_human_input.py collects them (ABI 16)
 *   lfsd_waypoint_time_grad / lfsd_tau_project   no counterpart: the reference invents the waypoint times (lib/InputWaypoints.py:212-228,
 *                         generate_time: chord length over an average speed) and then treats them as exact in the loss of
 *                         lib/QuadAlgorithm.py:616-673; the derivative of that loss in the times, and their ordered update (ABI 17)
 *   lfsd_time_normal_blocks / lfsd_lm_step_times   no counterpart: the Gauss-Newton matrix of the loss of lib/QuadAlgorithm.py:616-639
 *                         in parameters AND waypoint times is an arrow (a time enters one waypoint's residuals only); its border and
 *                         diagonal, and the Levenberg-Marquardt step with the times eliminated per waypoint (ABI 18)
 */
#ifndef LFSD_CPDP_H
#define LFSD_CPDP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LFSD_ABI_VERSION 18
#define LFSD_F32 0
#define LFSD_F64 1
#define LFSD_EINVAL (-1)   /* bad argument (null pointer, non-positive size, unknown enum) */
#define LFSD_ENOSPC (-2)   /* workspace too small */

/* status[] values written by lfsd_coc_solve */
#define LFSD_ST_CONVERGED 1   /* max |dJ/du| < tol * (1 + |J|)                         */
#define LFSD_ST_STALLED   2   /* converged to working precision: no step improves J beyond rounding, or the Newton
                                 decrement is below the resolution of J with the gradient at its rounding floor */
#define LFSD_ST_MAXITER   3
#define LFSD_ST_FAILED    4   /* non-finite cost / regularisation exhausted            */

/* mapping of the optimal-control solve onto the machine (lfsd_coc_solve) */
#define LFSD_MAP_AUTO     0   /* by batch size / model / exact_after */
#define LFSD_MAP_LOCKSTEP 1   /* several trajectories per wavefront, shooting intervals in sequence */
#define LFSD_MAP_WIDE     2   /* one trajectory per wavefront, intervals / step lengths in parallel */

/* optimizer methods (lib/QuadAlgorithm.py:164-188) */
#define LFSD_OPT_VANILLA  0
#define LFSD_OPT_NESTEROV 1
#define LFSD_OPT_ADAM     2
#define LFSD_OPT_NADAM    3
#define LFSD_OPT_AMSGRAD  4
#define LFSD_OPT_LM       5   /* Levenberg-Marquardt (ABI 14): not a code of lfsd_optimizer_step*, its update is lfsd_lm_step */

typedef struct lfsd_model_info {
  int abi_version;
  int n_state, n_control, n_auxvar, n_const;   /* n_const may be 0 */
  int time_varying;                            /* 1: COCSys_TimeVarying semantics */
  int lanes_per_trajectory;                    /* lane-group width G the kernels were built with */
  int is_emulator;                             /* 1 only for the CPU SIMT-emulator test build */
  const char* name;
  const char* hash;
} lfsd_model_info;

int lfsd_get_model_info(lfsd_model_info* out);
/* outputs of the interface function y = g(x) compiled into this library (ABI 9), 0 if the model was generated without one.  The
 * reference's interface functions are arbitrary CasADi expressions of the state (lib/QuadAlgorithm.py:616-639, Examples/*.py:
 * `Function('interface', [oc.state], [...])` and its `jacobian`); every example selects state components, which `iface_idx` covers
 * without a recompilation; a model generated with `setInterface(expr)` carries g and (dg/dx)^T r as generated code. */
int lfsd_interface_dim(void);
/* default value of runtime constant i (the number the reference would have baked into the CasADi graph) */
double lfsd_const_default(int i);

/* bytes of device scratch lfsd_coc_solve needs for `batch` trajectories when called with the same exact_after / mapping
 * and with (bounded != 0) or without control bounds: the two mappings of the solve lay their scratch out differently, and an
 * fp64 solve that is seeded by an fp32 one (see lfsd_coc_solve) stages the fp32 problem behind its own scratch */
size_t lfsd_coc_workspace_bytes(int dtype, int batch, int n_grid, int exact_after, int mapping, int bounded);

/* Solve `batch` independent optimal-control problems (the NLP of CPDP.py:110-175:
 * n_grid shooting intervals, steps_per_grid RK4 steps each, piecewise-constant control).
 *   ini_state [B][n_state]   horizon [B]   auxvar [B][n_auxvar]
 *   consts    [B][n_const] (const_per_traj=1) or [n_const] (const_per_traj=0); may be NULL if n_const==0
 *   u_init    [B][n_grid][n_control] initial guess, or NULL for zeros
 * outputs (CPDP.py:186-196):
 *   state_grid [B][n_grid+1][n_state], control_grid [B][n_grid+1][n_control] (last row repeated),
 *   costate_grid [B][n_grid+1][n_state] (== IPOPT lam_g), cost [B], iters [B], status [B]
 * solver: Gauss-Newton steps first, then Newton steps; `exact_after` = iteration from which the exact
 *   Lagrangian Hessian of the RK4 stages (what IPOPT gets from CasADi) is forced: 16 is the default policy,
 *   0 = exact from the first iteration, <0 = never (Gauss-Newton / Hamiltonian model only).
 *   steps_per_grid <= 8.
 *   control_lb / control_ub [n_control] (shared by the batch) or NULL: finite control bounds, the reference's
 *   setControlVariable(control, control_lb, control_ub) -> lbw / ubw of the NLP (CPDP.py:33-46, 150-153).  Both or
 *   neither; entries beyond +-1e19 mean "unbounded in that direction".  Solved by a control-limited backward sweep
 *   (box QP per stage, zero feedback gain on clamped components, clamped roll-out); the initial guess is the midpoint of
 *   finite bounds as in the reference.
 *   state_lb / state_ub [n_state] (shared by the batch), state_mult [B][n_grid][2][n_state], state_rho > 0, or all NULL:
 *   finite STATE bounds, the reference's setStateVariable(state, state_lb, state_ub) -> lbw / ubw of the shooting nodes
 *   X_1..X_N (CPDP.py:20-31, 140-147).  One call solves ONE augmented-Lagrangian subproblem: the nodes' terms
 *   [max(0, lu + rho (x - ub))^2 - lu^2 + max(0, ll + rho (lb - x))^2 - ll^2] / (2 rho) with the multipliers lu = state_mult
 *   [b][k-1][0][:], ll = [b][k-1][1][:] of node k are added to the cost; the caller updates the multipliers
 *   (lu <- max(0, lu + rho (x_k - ub)), ll likewise) and the penalty between calls until the nodes are feasible -- the outer
 *   loop is host code (COCSys.cocSolverBatch).  The returned costates include the bound multipliers, as IPOPT's lam_g
 *   do.  With state bounds the control-bound arrays must be given too (entries of +-1e20 where there is none).
 *   mapping: LFSD_MAP_AUTO, or force one of the two mappings of the same algorithm (same KKT points either way).
 *   dtype LFSD_F64, lock-step mapping, 32-lane models (quadrotor class), no bounds, exact_after != 0: the problem is solved in
 *   fp32 first -- from u_init as well when one is given: an all-zero row of u_init is a cold start, so a caller that hands zeros
 *   for every row it does not continue gets every row seeded -- and the fp64 kernel starts from those controls (a trajectory
 *   the fp32 solve failed on starts from its own row of u_init, or cold).  Every output and every convergence test is the fp64
 *   kernel's; iters[] counts both solves (so it may exceed max_iter, which bounds each of them); lfsd_coc_workspace_bytes
 *   includes the staging area.  LFSD_F64_SEED=0 in the environment switches the seeding off; a workspace without room for the
 *   staging area (sized while the switch was off) makes the call solve unseeded rather than fail.
 *   Wide mapping, dtype LFSD_F32, no bounds, exact_after >= 0, models whose interval-parallel phases take several rounds of one
 *   wavefront (more than 8 columns of [A B]: quadrotor, rocket): a trajectory may get a workgroup of FOUR wavefronts -- from the start
 *   when batch <= the number of CUs, else in a SECOND launch on the same stream that takes over the trajectories still running once
 *   all but one-per-CU are finished (their solver state is parked in the workspace; a device counter decides, the host reads nothing
 *   in between; lfsd_coc_workspace_bytes includes the counters and the hand-over list).  The reference solves every seed on its own
 *   (Examples/robotarm_random.py:60-73): a trajectory's outputs do not depend on the scheme or on the moment of the hand-over, bit
 *   for bit.  Environment (test hooks): LFSD_WIDE_WAVES=1 never more than one wavefront per trajectory, =4 four from the start at any
 *   batch; LFSD_WIDE_CAPACITY=<n> in place of the CU count; LFSD_WIDE_SUSPEND_IT=<k> hand over at iteration k.   */
int lfsd_coc_solve(int dtype, int batch, int n_grid, int steps_per_grid,
                   const void* ini_state, const void* horizon, const void* auxvar,
                   const void* consts, int const_per_traj, const void* u_init,
                   const void* control_lb, const void* control_ub,
                   const void* state_lb, const void* state_ub, const void* state_mult, double state_rho,
                   void* state_grid, void* control_grid, void* costate_grid,
                   void* cost, int* iters, int* status,
                   int max_iter, double tol, int exact_after, int mapping,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Differentiate the maximum principle along the solved trajectories and evaluate the
 * sparse-demonstration loss and its gradient.
 *   Z_grid  [B][n_grid+1][n_state+n_auxvar][n_state]  out: Riccati pair [P W], column-major
 *           (P_k, W_k of CPDP.py:329-338)
 *   iface_idx [n_iface] int32: state components exposed by the interface function; NULL (ABI 9): the interface function
 *           compiled into the library, n_iface = lfsd_interface_dim() (waypoints [B][n_waypoints][n_iface] as before)
 *   taus [B][n_waypoints], waypoints [B][n_waypoints][n_iface]
 *   loss [B], grad [B][n_auxvar]:  loss = sum_k |y(tau_k)-wp_k|^2, grad = sum_k (y-wp)^T dy/dx dx/dtheta
 *           (no factor 2, exactly as lib/QuadAlgorithm.py:630-637)
 *   auxX_grid [B][n_grid+1][n_auxvar][n_state], auxU_grid [B][n_grid+1][n_auxvar][n_control]:
 *           optional (NULL to skip) grids of dx/dtheta and du/dtheta (CPDP.py:352-381), column-major
 *   substeps: minimum coarse split-steps ("units") per grid interval (a 2x finer sweep is run alongside and
 *           Richardson-extrapolated; stiff intervals are refined further); 0 selects the default (1 with rtol > 0, else 4).
 *   rtol:   > 0: error-controlled sub-stepping -- an interval is redone with twice the units while the Richardson estimate
 *           |fine - coarse| / 3 of a block of columns exceeds rtol x that block's magnitude (the reference integrates the
 *           same ODEs with scipy's solve_ivp at its default rtol 1e-3, CPDP.py:335, 368, which is the host side's default here too:
 *           measured gradient error 1e-5..1e-4 of the exact ODE solution against the reference integrator's 2.6e-3).
 *           0: fixed `substeps`.  With oc_status given, a row whose solve did NOT end converged / at working precision (its grids
 *           are not a KKT point) stops refining once it has spent 24 x n_grid x substeps split units in a sweep (64 x until round 5); reported in `stats`.
 *   stats   [B][4] int32 or NULL: per trajectory, {split units executed by the Riccati sweep (rejected attempts included),
 *           intervals of it that were accepted ABOVE rtol because refinement stopped gaining (next to a conjugate point) or hit
 *           its cap, the same two numbers of the forward sweep}.  A non-zero second or fourth entry marks a loss / gradient
 *           whose error estimate exceeds the tolerance asked for.
 *   oc_status [B] int32 or NULL, skip_status_mask (ABI 8): the status[] lfsd_coc_solve wrote for these trajectories and a
 *           bit mask over its values (bit s set = skip rows with status s, e.g. 1 << LFSD_ST_FAILED).  A skipped row costs
 *           nothing: neither sweep runs for it, its loss, gradient and its Z_grid / auxX_grid / auxU_grid rows are NaN
 *           (never what the caller's buffers held before), its stats 0.  Without it a solve that FAILED (non-finite grids) or ran out of iterations on a problem
 *           without a minimiser still goes through the error-controlled sweeps, refines to the cap and holds its launch
 *           many times longer than the well-posed batch needs.  NULL (or mask 0): every row is differentiated, as the
 *           reference does.                                                                   */
int lfsd_aux_solve(int dtype, int batch, int n_grid,
                   const void* horizon, const void* auxvar, const void* consts, int const_per_traj,
                   const void* state_grid, const void* control_grid, const void* costate_grid,
                   void* Z_grid,
                   int n_waypoints, int n_iface, const int* iface_idx,
                   const void* taus, const void* waypoints,
                   void* loss, void* grad, void* auxX_grid, void* auxU_grid,
                   int substeps, double rtol, int* stats,
                   const int* oc_status, int skip_status_mask, void* stream);

/* The two phases of lfsd_aux_solve as separate launches (same arguments; lfsd_aux_solve == riccati then forward):
 *   lfsd_aux_riccati  CPDP/CPDP.py:316-338  backward Riccati sweep, fills Z_grid
 *   lfsd_aux_forward  CPDP/CPDP.py:340-381  forward sensitivity sweep from Z_grid + loss/gradient          */
int lfsd_aux_riccati(int dtype, int batch, int n_grid,
                     const void* horizon, const void* auxvar, const void* consts, int const_per_traj,
                     const void* state_grid, const void* control_grid, const void* costate_grid,
                     void* Z_grid, int substeps, double rtol, int* stats,
                     const int* oc_status, int skip_status_mask, void* stream);
int lfsd_aux_forward(int dtype, int batch, int n_grid,
                     const void* horizon, const void* auxvar, const void* consts, int const_per_traj,
                     const void* state_grid, const void* control_grid, const void* costate_grid,
                     const void* Z_grid,
                     int n_waypoints, int n_iface, const int* iface_idx,
                     const void* taus, const void* waypoints,
                     void* loss, void* grad, void* auxX_grid, void* auxU_grid,
                     int substeps, double rtol, int* stats,
                     const int* oc_status, int skip_status_mask, void* stream);

/* ABI 11 -- interpolation level 2.  The reference's cocSolver(..., interplation_level=2) returns scipy's interp1d(kind='cubic') of
 * the solved grids -- the not-a-knot cubic spline -- and its auxSysSolver integrates the Riccati and sensitivity ODEs along whatever
 * interpolant it is handed (CPDP.py:320-323, 347, 388-390).  On the uniform time grid the spline is carried as one CURVATURE grid per
 * solution grid, c_k = h^2 y''(t_k) / 6: on interval k at fraction s
 *     y(s) = y_k + s (y_k+1 - y_k) + ((1-s)^3 - (1-s)) c_k + (s^3 - s) c_k+1 .
 * lfsd_grid_curvature fits it for every component of a grid:
 *   grid, curv [B][n_grid+1][n_comp] of arithmetic type `dtype` (distinct arrays); n_grid >= 3 (four nodes, as scipy asks),
 *   batch > 0, n_comp > 0, else LFSD_EINVAL.  Any model library serves any grid (nothing of the model enters). */
int lfsd_grid_curvature(int dtype, int batch, int n_grid, int n_comp, const void* grid, void* curv, void* stream);

/* lfsd_aux_solve / lfsd_aux_riccati / lfsd_aux_forward along that cubic interpolant: the arguments of their namesakes plus
 *   state_curv [B][n_grid+1][n_state], control_curv [B][n_grid+1][n_control], costate_curv [B][n_grid+1][n_state]
 * (lfsd_grid_curvature of the three grids; all three required, n_grid >= 3).  The nominal (x, u, lambda)(t) inside the sweeps and
 * x(tau) of the loss follow the spline.  What the reference keeps linear stays linear: [P W] between its grid values inside the
 * forward sweep, dx/dtheta(tau) in the gradient, and the returned auxX_grid / auxU_grid are grid values as before
 * (CPDP.py:338, 381: interpolation() at its default level). */
int lfsd_aux_solve_cubic(int dtype, int batch, int n_grid,
                         const void* horizon, const void* auxvar, const void* consts, int const_per_traj,
                         const void* state_grid, const void* control_grid, const void* costate_grid,
                         const void* state_curv, const void* control_curv, const void* costate_curv,
                         void* Z_grid,
                         int n_waypoints, int n_iface, const int* iface_idx,
                         const void* taus, const void* waypoints,
                         void* loss, void* grad, void* auxX_grid, void* auxU_grid,
                         int substeps, double rtol, int* stats,
                         const int* oc_status, int skip_status_mask, void* stream);
int lfsd_aux_riccati_cubic(int dtype, int batch, int n_grid,
                           const void* horizon, const void* auxvar, const void* consts, int const_per_traj,
                           const void* state_grid, const void* control_grid, const void* costate_grid,
                           const void* state_curv, const void* control_curv, const void* costate_curv,
                           void* Z_grid, int substeps, double rtol, int* stats,
                           const int* oc_status, int skip_status_mask, void* stream);
int lfsd_aux_forward_cubic(int dtype, int batch, int n_grid,
                           const void* horizon, const void* auxvar, const void* consts, int const_per_traj,
                           const void* state_grid, const void* control_grid, const void* costate_grid,
                           const void* state_curv, const void* control_curv, const void* costate_curv,
                           const void* Z_grid,
                           int n_waypoints, int n_iface, const int* iface_idx,
                           const void* taus, const void* waypoints,
                           void* loss, void* grad, void* auxX_grid, void* auxU_grid,
                           int substeps, double rtol, int* stats,
                           const int* oc_status, int skip_status_mask, void* stream);

/* ABI 12 -- user-defined losses.  Every example of the reference ends in a loss the user writes from two callables, opt_sol(t) ->
 * [x, u, lambda] of cocSolver and auxsys_sol(t) -> [dx/dtheta, du/dtheta] of auxSysSolver (Examples/pendulum_timewarping.py:72-86,
 * Examples/rocket_groundtruth.py:45-70, lib/QuadAlgorithm.py:616-673), and samples trajectories with the same callables
 * (rocket_groundtruth.py:75-84, QuadAlgorithm.py:306-317).  lfsd_sample_grid is the batched call of such an interpolant:
 *   grid [B][n_grid+1][n_comp]; curv: NULL -- the linear interpolant (CPDP.py:386) -- or the curvature grid lfsd_grid_curvature
 *   fitted to `grid` -- the not-a-knot cubic (CPDP.py:388-390; then n_grid >= 3); horizon [B];
 *   times [B][n_times] (times_per_traj = 1) or [n_times] shared by the batch (0);   out [B][n_times][n_comp].
 * Interval and fraction as in the fused waypoint loss of lfsd_aux_solve: h = horizon / n_grid, k = clamp(floor(t / h), 0, n_grid-1),
 * s = (t - k h) / h, y = y_k + s (y_k+1 - y_k) [+ ((1-s)^3 - (1-s)) c_k + (s^3 - s) c_k+1].  t = horizon is interval n_grid-1 at
 * s = 1; a t outside [0, horizon] extrapolates its end interval (scipy raises ValueError: that check is the caller's); a NaN time
 * gives a NaN row.  n_comp = n_state serves a state grid, n_comp = n_auxvar * n_state an auxX_grid.  Nothing of the model enters.
 * LFSD_EINVAL: a NULL grid / horizon / times / out, batch / n_comp / n_times <= 0, n_grid < 1 (< 3 with curv), times_per_traj
 * not 0 / 1, `out` overlapping an input, an unknown dtype, more than 2^31-1 workgroups. */
int lfsd_sample_grid(int dtype, int batch, int n_grid, int n_comp, int n_times, int times_per_traj,
                     const void* grid, const void* curv, const void* horizon, const void* times, void* out, void* stream);

/* The chain rule of a loss L(x(tau_1..K), u(tau_1..K)) through auxsys_sol, without materialising auxsys_sol(tau):
 *   grad[b][q] = sum_k ( sum_i rx[b][k][i] X(tau_k)[q][i]  +  sum_j ru[b][k][j] U(tau_k)[q][j] )
 *   rx [B][K][n_state] = dL/dx(tau_k), ru [B][K][n_control] = dL/du(tau_k) (the caller's: autograd of a torch function, say);
 *   X, U: the LINEAR interpolants of auxX_grid [B][n_grid+1][n_param][n_state], auxU_grid [B][n_grid+1][n_param][n_control] as
 *   lfsd_aux_solve returns them (auxsys_sol is linear at either interpolation level, CPDP.py:381); interval rule as above;
 *   horizon [B], taus [B][K], grad [B][n_param].  ru and auxU_grid: both or neither (a loss without a control term).
 * Summed in a fixed order (k ascending, states then controls, components ascending), no atomics: a row's gradient is the same
 * bits in any batch.  With rx = x(tau) - waypoint on the interface components this is the gradient lfsd_aux_solve fuses (its
 * "no factor 2" convention, lib/QuadAlgorithm.py:630-637, is HALF the derivative of the squared distance).
 * LFSD_EINVAL: a NULL required pointer, a non-positive size, n_grid < 1, exactly one of ru / auxU_grid, `grad` overlapping an
 * input, an unknown dtype, more than 2^31-1 workgroups. */
int lfsd_waypoint_vjp(int dtype, int batch, int n_grid, int n_state, int n_control, int n_param, int n_waypoints,
                      const void* horizon, const void* taus, const void* rx, const void* ru,
                      const void* auxX_grid, const void* auxU_grid, void* grad, void* stream);

/* theta <- update(theta, grad) for every trajectory; m/v/vhat are optimizer state [B][n_param]
 * (m: Nesterov velocity or first moment; v: second moment; vhat: AMSGrad max; unused ones may be NULL).
 * proj_lo [n_param] or NULL: theta <- max(theta, proj_lo) after the step (the examples' projection
 * current_parameter[0] = fmax(current_parameter[0], 1e-8)).  iter_idx counts from 0.
 * row_active [B] int32 or NULL: rows with 0 are frozen for this step -- theta and m/v/vhat stay untouched (a
 * learner that skips trajectories whose solve did not converge; the reference has no such case, pass NULL).  */
int lfsd_optimizer_step(int dtype, int method, int batch, int n_param, int iter_idx,
                        double lr, double mu, double beta1, double beta2, double eps,
                        void* theta, const void* grad, void* m, void* v, void* vhat,
                        const void* proj_lo, const int* row_active, void* stream);

/* out = theta + mu * v   (Nesterov look-ahead, [B][n_param]) */
int lfsd_lookahead(int dtype, long long n, double mu, const void* theta, const void* v, void* out, void* stream);

/* ABI 13 -- hyper-parameter sweeps in one batch.  The reference's comparison scripts (test/opt_methods_comparison.py: five update
 * rules at five learning rates; test/{vanilla,nesterov,adam,nadam,amsgrad}_learning_rate_comparison.py: one rule at four rates)
 * run QuadAlgorithm.run once per configuration.  Here every ROW of a batch carries its own rule and hyper-parameters:
 *   method [B] int32 (LFSD_OPT_*), hyper [B][5] of arithmetic type `dtype`: lr, mu, beta1, beta2, eps of the row.
 * lfsd_optimizer_step_rows is lfsd_optimizer_step with those read per row, expression for expression: a row's theta / m / v / vhat
 * come out as the bits lfsd_optimizer_step gives when called with that row's rule and values (its double arguments cast to
 * `dtype` are the entries of `hyper`).  proj_lo, row_active, iter_idx as there.  A row whose method code is not one of the five is
 * left untouched, and so is the state its rule does not use (m, v, vhat for Vanilla; v, vhat for Nesterov; vhat for Adam / Nadam).
 * m, v and vhat are all required: the batch may mix rules.
 * LFSD_EINVAL: a NULL method / hyper / theta / grad / m / v / vhat, batch or n_param <= 0, iter_idx < 0, an unknown dtype. */
int lfsd_optimizer_step_rows(int dtype, int batch, int n_param, int iter_idx, const int* method, const void* hyper,
                             void* theta, const void* grad, void* m, void* v, void* vhat,
                             const void* proj_lo, const int* row_active, void* stream);

/* The evaluation point of such a batch: out[b] = theta[b] + hyper[b][1] * m[b] for a Nesterov row (lib/QuadAlgorithm.py:478), and
 * out[b] = theta[b], bit for bit, for every other row -- selected on the method, not multiplied by zero: m of an Adam row is its
 * first moment and may be Inf or NaN.  theta, m, out [B][n_param]; out must not overlap theta or m.
 * LFSD_EINVAL: a NULL pointer, batch or n_param <= 0, an unknown dtype, `out` overlapping theta or m. */
int lfsd_lookahead_rows(int dtype, int batch, int n_param, const int* method, const void* hyper,
                        const void* theta, const void* m, void* out, void* stream);

/* Traces on the device (the reference appends loss and parameters to host lists every iteration, lib/QuadAlgorithm.py:244-252).
 * For every row with row_active == NULL or row_active[b] != 0:
 *   loss_trace  [B][capacity]              [b][iter_idx]       = loss[b]
 *   gnorm_trace [B][capacity]              [b][iter_idx]       = ||grad[b]||_2   (summed in `dtype`, components ascending, by one
 *                                                                thread, no atomics: the same bits in any batch)
 *   theta_trace [B][capacity+1][n_param]   [b][iter_idx+1][:]  = theta[b][:]     (slot 0 is theta_0: the caller's)
 * Any of the three traces may be NULL, not all.  No other word of the traces is written.  loss [B], grad, theta [B][n_param].
 * LFSD_EINVAL: a NULL loss / grad / theta, all three traces NULL, batch / n_param / capacity <= 0, iter_idx < 0 or >= capacity,
 * an unknown dtype. */
int lfsd_trace_append(int dtype, int batch, int n_param, int iter_idx, int capacity,
                      const void* loss, const void* grad, const void* theta, const int* row_active,
                      void* loss_trace, void* gnorm_trace, void* theta_trace, void* stream);

/* ABI 14 -- a Levenberg-Marquardt outer update.  The default loss is a sum of squares, loss = sum_k |y(tau_k) - wp_k|^2, and the forward
 * sweep returns dx/dtheta on the grid (auxX_grid): its linear interpolant at the waypoint times, restricted to the interface components,
 * is the Jacobian J of the residuals; the fused gradient is J^T r ("no factor 2").  lfsd_normal_matrix forms the Gauss-Newton matrix
 *   H[b][q1][q2] = sum_k sum_c X(tau_k)[q1][idx_c] X(tau_k)[q2][idx_c]            (= J^T J;  H [B][n_param][n_param])
 * with X the LINEAR interpolant of auxX_grid [B][n_grid+1][n_param][n_state] (the dx/dtheta(tau) of the fused gradient and of
 * lfsd_waypoint_vjp at either interpolation level), interval and fraction as in lfsd_sample_grid; horizon [B], taus [B][n_waypoints],
 * iface_idx [n_iface] int32 (state components; the interface compiled into a library is not served).  Summed k ascending, then c
 * ascending, by one thread per element of the lower triangle, which stores the element and its mirror image: both triangles hold the
 * same bits; no atomics, a row's H is the same bits in any batch.  A NaN row of auxX_grid (a row the sweeps skipped) gives a NaN row
 * of H and touches no other.  Small eigenvalues of H are directions of theta the waypoints do not pin down.
 * LFSD_EINVAL: a NULL pointer, a non-positive size, n_grid < 1, H overlapping an input, an unknown dtype, more than 2^31-1 workgroups.
 * iface_idx is a device array and the call reads nothing back: its range is checked ON THE DEVICE -- with an entry outside
 * [0, n_state) the call returns 0 and writes no word of H. */
int lfsd_normal_matrix(int dtype, int batch, int n_grid, int n_state, int n_param, int n_waypoints, int n_iface,
                       const int* iface_idx, const void* horizon, const void* taus, const void* auxX_grid, void* H, void* stream);

/* The accept / reject state machine of Levenberg-Marquardt and the damped solve, for every row, in one launch and without a host read.
 * State per row (in/out):  theta [B][p] the last accepted point;  loss_acc [B], grad_acc [B][p], H_acc [B][p][p] loss, gradient and H
 * there (loss_acc = +inf: nothing accepted yet);  lambda [B] the damping;  theta_trial [B][p]: on input the point that was just
 * evaluated, on output the next point to evaluate.  Inputs: loss_t [B], grad_t [B][p], H_t [B][p][p] the evaluation at theta_trial;
 * proj_lo [p] or NULL;  row_active [B] int32 or NULL (a row with 0 keeps every word of its state);  lambda_down / lambda_up /
 * lambda_min / lambda_max, cast to `dtype`.  accepted [B] int32 or NULL: 1 where the row accepted in this call, else 0 (also for a
 * row that is not active).  For every active row:
 *   1. accept iff loss_t < loss_acc and loss_t, grad_t, H_t are all finite:  theta <- theta_trial, (loss, grad, H)_acc <- (loss, grad,
 *      H)_t, lambda <- max(lambda * lambda_down, lambda_min);  otherwise lambda <- min(lambda * lambda_up, lambda_max);
 *   2. loss_acc still +inf, or max_j H_acc[j][j] not positive:  theta_trial <- theta (the row cannot move);  else
 *   3. A = H_acc + lambda (diag(H_acc) + 1e-8 max_j H_acc[j][j] I)  (Marquardt's scaling with a floor: a parameter without
 *      sensitivity cannot make A singular),
 *   4. Cholesky without pivoting, A delta = -grad_acc;
 *   5. a pivot that is not positive or not finite:  lambda <- min(lambda * lambda_up, lambda_max) and the factorisation again, at most
 *      8 such retries in one call (lambda is raised once per retry); if the last one fails too, theta_trial <- theta;
 *   6. else theta_trial <- max(theta + delta, proj_lo) componentwise.
 * One row per lane, fixed operation order, no atomics: a row's outputs are the same bits in any batch.
 * The nine state / input arrays must be distinct and must not overlap (not checked).
 * LFSD_EINVAL: a NULL required pointer, batch <= 0, n_param <= 0 or > 16, lambda_down outside (0, 1], lambda_up < 1, lambda_min <= 0
 * or > lambda_max, a NaN among the four, any of these AFTER the cast to `dtype` (a lambda_min that is 0 as a float, a lambda_max that
 * is inf), an unknown dtype. */
int lfsd_lm_step(int dtype, int batch, int n_param, double lambda_down, double lambda_up, double lambda_min, double lambda_max,
                 void* theta, void* loss_acc, void* grad_acc, void* H_acc, void* lambda, void* theta_trial,
                 const void* loss_t, const void* grad_t, const void* H_t, const void* proj_lo, const int* row_active,
                 int* accepted, void* stream);

/* ABI 15 -- several demonstrations per seed.  A batch of B = n_groups * group_size rows holds the demonstrations of one seed (one
 * parameter vector) next to each other: row g * group_size + d is demonstration d of group g.  The solve, the sweeps and
 * lfsd_normal_matrix run on the B rows as ever (the parameters of the groups are expanded to rows with lfsd_gather_rows and the index
 * row -> row / group_size); this call sums their results per group, and the update entry points then run on n_groups rows unchanged.
 * J^T J of the stacked residuals of a group is the sum of its rows' matrices.
 *   loss [B], grad [B][n_param], H [B][n_param][n_param] or NULL;  row_ok [B] int32 or NULL (= every row counts)
 *   loss_g [G], grad_g [G][n_param], H_g [G][n_param][n_param] or NULL (given exactly when H is);  n_ok [G] int32
 * For every group and every element (the loss, the n_param gradient components, the n_param^2 entries of H) the output is 0 of type
 * `dtype` plus the values of the rows with row_ok != 0, added one at a time, demonstrations ascending, in that type.  The values of a
 * row that is left out are never added (nor read): they may be NaN.  A NaN in a row that counts propagates to its group and to no
 * other.  n_ok[g] is the number of rows counted; a group with n_ok == 0 gets zeros.  One thread per (group, element), no atomics, one
 * summation order: a group's outputs are the same bits in any batch and at any position in it, and H_g is as bit-symmetric as its
 * inputs.
 * LFSD_EINVAL, before any launch: n_groups, group_size or n_param <= 0, an unknown dtype, a NULL required pointer, exactly one of H and
 * H_g given, an output overlapping an input, more than 2^31-1 workgroups. */
int lfsd_group_reduce(int dtype, int n_groups, int group_size, int n_param,
                      const void* loss, const void* grad, const void* H, const int* row_ok,
                      void* loss_g, void* grad_g, void* H_g, int* n_ok, void* stream);

/* ABI 16 -- waypoint weights and ragged demonstrations in the fused loss.  wp_weight [B][n_waypoints], of arithmetic type `dtype`:
 *   loss = sum_k w_k |y(tau_k) - wp_k|^2,   grad = sum_k w_k (y - wp_k)^T dy/dx dx/dtheta (still no factor 2),   H = sum_k w_k J_k^T J_k.
 * A waypoint with w_k == 0 DOES NOT EXIST: its tau and its target are never read (they may be NaN, negative or beyond the horizon) and
 * it contributes no operation to any sum -- the outputs are the bits of the unweighted call on the list without it.  That is what
 * makes padding demonstrations of different lengths to a common n_waypoints safe.  The other waypoints enter through the scaled
 * residual rs = w r, formed once (loss += rs r, the gradient contracts rs), and H through (w x1) x2: exact for w = 1 and for powers of
 * two, so an array of ones gives the bits of wp_weight == NULL, which is legal and is the unweighted sibling, launch for launch
 * (lfsd_aux_forward, lfsd_aux_forward_cubic, lfsd_normal_matrix; there is no weighted lfsd_aux_solve: call lfsd_aux_riccati[_cubic],
 * which knows no waypoints, then one of these).  The weights must be non-negative and finite: that is the CALLER's to guarantee,
 * nothing on the device checks it (a negative weight gives an indefinite H, a NaN weight a NaN row).  Every other argument, every
 * LFSD_EINVAL case (before any launch) and the treatment of skipped rows are the sibling's; for lfsd_normal_matrix_weighted H must not
 * overlap wp_weight either. */
int lfsd_aux_forward_weighted(int dtype, int batch, int n_grid,
                              const void* horizon, const void* auxvar, const void* consts, int const_per_traj,
                              const void* state_grid, const void* control_grid, const void* costate_grid,
                              const void* Z_grid,
                              int n_waypoints, int n_iface, const int* iface_idx,
                              const void* taus, const void* waypoints, const void* wp_weight,
                              void* loss, void* grad, void* auxX_grid, void* auxU_grid,
                              int substeps, double rtol, int* stats,
                              const int* oc_status, int skip_status_mask, void* stream);
int lfsd_aux_forward_cubic_weighted(int dtype, int batch, int n_grid,
                                    const void* horizon, const void* auxvar, const void* consts, int const_per_traj,
                                    const void* state_grid, const void* control_grid, const void* costate_grid,
                                    const void* state_curv, const void* control_curv, const void* costate_curv,
                                    const void* Z_grid,
                                    int n_waypoints, int n_iface, const int* iface_idx,
                                    const void* taus, const void* waypoints, const void* wp_weight,
                                    void* loss, void* grad, void* auxX_grid, void* auxU_grid,
                                    int substeps, double rtol, int* stats,
                                    const int* oc_status, int skip_status_mask, void* stream);
int lfsd_normal_matrix_weighted(int dtype, int batch, int n_grid, int n_state, int n_param, int n_waypoints, int n_iface,
                                const int* iface_idx, const void* horizon, const void* taus, const void* wp_weight,
                                const void* auxX_grid, void* H, void* stream);

/* ABI 17 -- learnable waypoint times.  The times tau_k of a sparse demonstration are guesses: the reference's human-input path builds
 * them from chord length divided by an average speed, rounded to 0.01 s (lib/InputWaypoints.py:212-228), and the loss of
 * lib/QuadAlgorithm.py:616-673 then takes them as exact.  The time-warp parameter stretches the whole axis by one factor; it cannot
 * repair times that are wrong by different amounts.  lfsd_waypoint_time_grad is the derivative of the fused loss in the times:
 *   dtau[b][k] = w_k r^T (dy/dx)(x(tau_k)) xdot(tau_k) + tau_prior (tau_k - tau_ref[b][k]),      r = y(x(tau_k)) - waypoints[b][k]
 * with NO factor 2 (the convention of the fused gradient: d loss / d tau_k = 2 dtau with tau_prior = 0).  x(t) is the interpolant of
 * state_grid [B][n_grid+1][n_state] -- linear (curv == NULL), or the cubic of lfsd_sample_grid with curv = lfsd_grid_curvature of the
 * state grid (n_grid >= 3) -- interval and fraction as in lfsd_sample_grid (a tau on a node belongs to the interval on its right,
 * tau = horizon is interval n_grid-1 at s = 1), and xdot the derivative in t of that very expression:
 *   (x_k+1 - x_k) / h   [ + ((1 - 3 (1-s)^2) c_k + (3 s^2 - 1) c_k+1) / h ].
 * iface_idx [n_iface] int32 picks state components; NULL selects the interface function compiled into the library (n_iface =
 * lfsd_interface_dim()), evaluated as the fused loss evaluates it, with the constants `consts` [B][n_const] (const_per_traj = 1) or
 * [n_const] (0) it may depend on (the consts of lfsd_aux_forward; never read with an index list, NULL is fine there).  This is why the
 * call lives in the model library.  horizon [B]; taus, dtau, wp_weight, tau_ref [B][n_waypoints]; waypoints [B][n_waypoints][n_iface].
 * wp_weight NULL: weight 1.  A weight of exactly 0 means the waypoint does not exist: dtau = +0.0 and its tau, target and tau_ref are
 * never read (NaN padding is fine).  The other weights enter through the scaled residual w r, formed once: all-ones weights give the
 * bits of NULL, powers of two scale dtau exactly.  tau_ref NULL or tau_prior == 0: no prior term.
 * One thread per (trajectory, waypoint) sums the components in ascending order; no atomics: a row's dtau is the same bits in any
 * batch.  A NaN row of state_grid gives a NaN row of dtau and touches no other.  An entry of iface_idx outside [0, n_state) is found
 * ON THE DEVICE, as lfsd_normal_matrix finds it: the call returns 0 and writes no word of dtau.
 * LFSD_EINVAL, before any launch: batch / n_waypoints / n_iface <= 0, n_grid < 1 (< 3 with curv), an unknown dtype, a NULL state_grid /
 * horizon / taus / waypoints / dtau, iface_idx NULL in a library without a compiled interface, with another n_iface, or without the
 * consts that library needs, tau_prior negative or not finite (also after the cast to `dtype`), dtau overlapping an input, more than
 * 2^31-1 workgroups. */
int lfsd_waypoint_time_grad(int dtype, int batch, int n_grid, int n_waypoints, int n_iface,
                            const void* state_grid, const void* curv, const void* horizon,
                            const void* consts, int const_per_traj,
                            const void* taus, const void* waypoints, const int* iface_idx,
                            const void* wp_weight, const void* tau_ref, double tau_prior, void* dtau, void* stream);

/* The projection of an updated (or looked-ahead) time vector: it keeps the existing waypoints of a row strictly ordered and inside
 * (0, horizon).  tau_ref [B][n_waypoints]: ordered times, typically those the step started from; tau_io [B][n_waypoints]: in the
 * proposal, out the projected times.  For every existing waypoint k (wp_weight NULL or wp_weight[b][k] != 0), with prev / next the
 * nearest existing waypoints on either side in tau_ref (0 before the first, horizon[b] after the last) and c = max_shift:
 *   tau_io[k] <- clamp(clamp(tau_io[k], tau_lo[b][k], tau_hi[b][k]),  ref_k - c (ref_k - ref_prev),  ref_k + c (ref_next - ref_k)).
 * With 0 < c < 0.5 the gap of two neighbours stays at least (1 - 2c) of what it was, whatever the update rule proposed.  The window
 * is applied last: where tau_lo / tau_hi (either may be NULL) do not intersect it, the order wins.  A proposal that is not finite
 * keeps ref_k.  Rows with row_active[b] == 0 and waypoints that do not exist keep tau_io bit for bit (and nothing of such a waypoint
 * is read).  One thread per row; every clamp reads tau_ref only.
 * LFSD_EINVAL, before any launch: batch or n_waypoints <= 0, an unknown dtype, a NULL tau_ref / tau_io / horizon, max_shift outside
 * (0, 0.5) as a double or after the cast to `dtype` (a NaN included), tau_io overlapping another array. */
int lfsd_tau_project(int dtype, int batch, int n_waypoints, const void* tau_ref, void* tau_io, const void* horizon,
                     const void* wp_weight, const void* tau_lo, const void* tau_hi, double max_shift,
                     const int* row_active, void* stream);

/* ABI 18 -- Levenberg-Marquardt over parameters and waypoint times jointly.  With the times tau_k free, the residual block of waypoint k
 * of a row, r_k = y(tau_k) - wp_k, has the Jacobian J_k [n_iface x p] in theta (lfsd_normal_matrix) and the column t_k [n_iface] -- the
 * interface rows of the slope xdot(tau_k) of lfsd_waypoint_time_grad -- in tau_k, and depends on no other time.  The Gauss-Newton matrix
 * in (theta, tau) is an arrow: H = sum_k w_k J_k^T J_k in the corner, and per waypoint
 *   C[b][k][q] = w_k sum_c t_c X(tau_k)[q][idx_c]      (the coupling c_k = w_k J_k^T t_k;  C [B][n_waypoints][n_param])
 *   d[b][k]    = w_k sum_c t_c t_c                     (the time block, diagonal;          d [B][n_waypoints])
 * ("no factor 2" throughout, as H and the gradients).  lfsd_time_normal_blocks forms both: X the LINEAR interpolant of auxX_grid
 * [B][n_grid+1][n_param][n_state] with the expressions of lfsd_normal_matrix; t from state_grid [B][n_grid+1][n_state] and, with
 * curv = lfsd_grid_curvature of it (n_grid >= 3), along the cubic interpolant, with the expressions of lfsd_waypoint_time_grad's index
 * path; iface_idx [n_iface] int32 (the interface compiled into a library is not served); horizon [B]; taus, wp_weight [B][n_waypoints].
 * One thread per (row, waypoint, parameter) sums the interface components in ascending order; the weight is applied once, as (w t_c):
 * all-ones weights give the bits of wp_weight == NULL.  A waypoint of weight exactly 0 gets +0.0 and its tau is never read (NaN padding
 * is legal).  No atomics: a row's outputs are the same bits in any batch; a NaN row poisons only itself.  An entry of iface_idx outside
 * [0, n_state) is found ON THE DEVICE, as lfsd_normal_matrix finds it: the call returns 0 and writes nothing.
 * LFSD_EINVAL, before any launch: a NULL required pointer, a non-positive size, n_grid < 1 (< 3 with curv), C or d overlapping an input
 * or each other, an unknown dtype, more than 2^31-1 workgroups. */
int lfsd_time_normal_blocks(int dtype, int batch, int n_grid, int n_state, int n_param, int n_waypoints, int n_iface,
                            const int* iface_idx, const void* horizon, const void* taus, const void* wp_weight,
                            const void* state_grid, const void* curv, const void* auxX_grid, void* C, void* d, void* stream);

/* lfsd_lm_step with the times as unknowns: the accept / reject state machine over the point (theta, tau) and the damped solve of the
 * arrow system, one GROUP per lane.  A group is one parameter vector and the group_size consecutive rows that learn it (B = n_groups *
 * group_size; group_size = 1: every row its own theta); a row owns n_waypoints times.
 * Per group (in/out), as in lfsd_lm_step: theta, grad_acc, theta_trial [G][p], loss_acc, lambda [G], H_acc [G][p][p].
 * Per row (in/out): tau [B][K] the accepted times; tau_trial [B][K] on input the times just evaluated, on output the next (NOT yet
 * projected) times; gtau_acc [B][K], C_acc [B][K][p], d_acc [B][K] the time gradient (lfsd_waypoint_time_grad with tau_prior = 0) and
 * the blocks above at the accepted point; ok_acc [B] int32 the rows that counted there.
 * Inputs: loss_t [G], grad_t [G][p], H_t [G][p][p] the evaluation at (theta_trial, tau_trial) per group -- lfsd_group_reduce's outputs,
 * or the rows' own arrays when group_size = 1; gtau_t, C_t, d_t per row; row_ok [B] int32 or NULL (rows with 0 did not count: their
 * values are never read); wp_weight [B][K] or NULL (weight 0: the waypoint does not exist); proj_lo [p] or NULL; group_active [G] int32
 * or NULL (a group with 0 keeps every word of its state and of its rows'); accepted [G] int32 or NULL.  For every active group:
 *   1. accept iff loss_t < loss_acc and loss_t, grad_t, H_t and gtau_t, C_t, d_t of the counted rows' existing waypoints are finite:
 *      the copies of lfsd_lm_step, tau <- tau_trial for every row of the group, (gtau, C, d)_acc <- (gtau, C, d)_t for the counted rows,
 *      ok_acc <- row_ok; lambda moves as in lfsd_lm_step;
 *   2. under lfsd_lm_step's conditions the group cannot move: theta_trial <- theta, tau_trial <- tau;
 *   3. with floor = 1e-8 max_j H_acc[j][j] and ftau = 1e-8 max d_acc (over the waypoints that enter): D_k = d_k + lambda (d_k + ftau),
 *        S = H_acc + lambda (diag H_acc + floor I) - sum_k c_k c_k^T / D_k,      b = -grad_acc + sum_k c_k gtau_k / D_k,
 *      summed rows ascending, then waypoints ascending, over the rows with ok_acc != 0 and their existing waypoints; a waypoint whose
 *      D_k is not > 0 does not move and contributes nothing;
 *   4. Cholesky of S without pivoting with lfsd_lm_step's retry rule (S and b are formed again for each raised lambda); solved:
 *      theta_trial <- max(theta + dtheta, proj_lo); not solved: theta_trial <- theta, tau_trial <- tau;
 *   5. dtau_k = -(gtau_k + c_k . dtheta) / D_k, tau_trial_k <- tau_k + dtau_k; rows that are not counted, absent and skipped waypoints
 *      get tau_trial_k <- tau_k.
 * With every c_k and d_k zero no correction is executed: theta, theta_trial, lambda and accepted are the bits of lfsd_lm_step.  Fixed
 * operation order, no atomics: a group's outputs are the same bits in any batch.  Order and bounds of the proposed times are not this
 * call's business: lfsd_tau_project(tau_ref = tau, tau_io = tau_trial, ...) follows.  The arrays must not overlap (not checked).
 * LFSD_EINVAL: lfsd_lm_step's cases (n_groups for batch), group_size <= 0, n_waypoints <= 0, a NULL per-row array. */
int lfsd_lm_step_times(int dtype, int n_groups, int group_size, int n_param, int n_waypoints,
                       double lambda_down, double lambda_up, double lambda_min, double lambda_max,
                       void* theta, void* loss_acc, void* grad_acc, void* H_acc, void* lambda, void* theta_trial,
                       void* tau, void* tau_trial, void* gtau_acc, void* C_acc, void* d_acc, int* ok_acc,
                       const void* loss_t, const void* grad_t, const void* H_t,
                       const void* gtau_t, const void* C_t, const void* d_t,
                       const int* row_ok, const void* wp_weight, const void* proj_lo,
                       const int* group_active, int* accepted, void* stream);

/* ABI 10 -- the per-seed stop rule of the learning loop.  The reference learns every seed on its own and leaves its loop when
 * `loss > 0.9 and norm(diff_loss) > 0.05` fails (lib/QuadAlgorithm.py:239-257; Examples/robotarm_random.py:60-73 solve the seeds
 * one after the other).  One launch (one workgroup) applies that test to the `n_rows` rows of a batch of seeds still learning and
 * compacts the survivors, stably and deterministically (no atomics):
 *   loss [n_rows], grad [n_rows][n_param] of arithmetic type `dtype`; the norm is formed in that type
 *   keep(i) = loss[i] > loss_tol && ||grad[i]||_2 > grad_tol       (a NaN loss or gradient stops the seed, as the reference's test)
 *   rows_in  [n_rows] original row ids in ascending order, NULL = identity
 *   eligible [n_rows] or NULL: rows with 0 are kept whatever their loss / gradient (frozen this step, gradient zeroed)
 *   rows_out [n_rows] original id of the k-th survivor, pos_out [n_rows] its position in the input list (entries from *n_out on
 *            are left alone), n_out [1] their number; rows_out must not be rows_in
 *   active, stop_iter: FULL-batch arrays indexed by original id; a row that stops now gets active = 0, stop_iter = iter_idx + 1
 * n_rows > 0, n_param > 0, iter_idx >= 0, thresholds not NaN. */
int lfsd_stop_compact(int dtype, int n_rows, int n_param, const void* loss, const void* grad,
                      const int* rows_in, const int* eligible,
                      double loss_tol, double grad_tol, int iter_idx,
                      int* rows_out, int* pos_out, int* n_out, int* active, int* stop_iter, void* stream);

/* ABI 10 -- rows of `row_bytes` bytes between a full batch and the dense batch of the seeds still learning (what the solver
 * entry points above are then called with: lib/QuadAlgorithm.py:239-257 per seed):
 *   lfsd_gather_rows   dst[i][:] = src[index[i]][:]      lfsd_scatter_rows   dst[index[i]][:] = src[i][:]      i < n_rows
 * Type-blind bit copies.  row_bytes and both base addresses must be multiples of 4; 16-byte accesses are used when all three
 * are multiples of 16.  index [n_rows] int32, entries distinct for a scatter; src and dst must not overlap. */
int lfsd_gather_rows(int n_rows, long long row_bytes, const int* index, const void* src, void* dst, void* stream);
int lfsd_scatter_rows(int n_rows, long long row_bytes, const int* index, const void* src, void* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif
