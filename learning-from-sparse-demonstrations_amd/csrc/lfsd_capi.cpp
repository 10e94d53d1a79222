// C ABI (include/lfsd_cpdp.h) over the kernels of cpdp_kernels.h for ONE model.
// Build:  runtime.build_library (two translation units, see lfsd_internal.h), or as a single one:
//         hipcc -x hip --offload-arch=gfx950 -DLFSD_MODEL_HEADER='"gen/<hash>.h"' -DLFSD_G=<lanes> ...
// (tests/emu builds the same file with g++ -DLFSD_EMU for the CPU SIMT emulator.)
#include "lfsd_internal.h"
#include <cmath>
#include <cstdlib>
#include <algorithm>
#if !defined(LFSD_SPLIT_RICCATI)
#include "lfsd_riccati.inc"
#include "lfsd_cubic.inc"
#endif

LFSD_API int lfsd_get_model_info(lfsd_model_info* out) {
  if (!out) return LFSD_EINVAL;
  out->abi_version = LFSD_ABI_VERSION;
  out->n_state = Model::NX; out->n_control = Model::NU; out->n_auxvar = Model::NP; out->n_const = Model::NC_REAL;
  out->time_varying = Model::TIME_VARYING ? 1 : 0;
  out->lanes_per_trajectory = G;
#if defined(LFSD_EMU)
  out->is_emulator = 1;
#else
  out->is_emulator = 0;
#endif
  out->name = Model::name();
  out->hash = Model::hash();
  return 0;
}

LFSD_API int lfsd_interface_dim(void) { return Model::NIF; }

LFSD_API double lfsd_const_default(int i) {
  if (i < 0 || i >= Model::NC_REAL) return 0.0;
  return Model::const_default(i);
}

// fp32 lean OC kernel of the 32-lane models: packed roll-out, four trajectories per wavefront (cpdp_kernels.h, PK)
static constexpr bool OC_PK = (G == 32) && (Model::NX + Model::NU + 1) / 2 <= 16;
static constexpr int OC_GPB = OC_PK ? 4 : GPB;      // scratch slots are padded to whole workgroups of either mapping
static long long padded_batch(int batch) { return ((long long)(batch + OC_GPB - 1) / OC_GPB) * OC_GPB; }

// Which mapping solves a batch.  The lock-step kernels (several trajectories per wavefront, intervals in sequence) fill the
// machine from ~4096 trajectories up; below ~1500 most of the 1024 SIMDs would have no wavefront, and where an iteration is
// expensive -- exact stage Hessians: robot arm, rocket -- the WIDE kernel (one trajectory per wavefront, intervals in
// parallel: oc_solve_wide_kernel) is 3.5-6x faster (robot arm 1024 seeds 108 -> 18.6 ms, rocket n_grid 100 763 -> 215 ms).
// Models that converge in a handful of cheap iterations (quadrotor: 5, pendulum, cart-pole) are faster on the lock-step
// mapping from a few thousand trajectories up, the fp32 packed / MFMA lean kernel at every batch size; models that spend
// most iterations on exact stage Hessians are faster on the wide mapping at every batch size measured (robot arm 4096:
// 113 -> 41 ms, 8192: 202 -> 75 ms; rocket 4096: 1315 -> 525 ms; profiles/r02_d_wide_vs_lockstep.txt).  The caller can say
// so (`mapping`: LFSD_MAP_AUTO / _LOCKSTEP / _WIDE; lfsd_amd.models does for the robot arm).  A bounded problem
// (control_lb / control_ub) always runs the wide kernel.
static bool use_wide(int dtype, int batch, int exact_after, int mapping, bool bounded) {
  if (bounded) return true;
  if (mapping == LFSD_MAP_LOCKSTEP) return false;
  if (mapping == LFSD_MAP_WIDE) return true;
  if (exact_after == 0) return true;      // Newton from the first iteration (rocket): wide wins at every batch size measured
  const bool lean_mfma = OC_PK && dtype == LFSD_F32;
  return batch <= lfsd::kWideMaxBatch && !lean_mfma;
}

// fp64 on the lock-step mapping, 32-lane models (the class with a mesh continuation), no bounds, not Newton-from-start: a cold
// start is solved in fp32 first (the lean MFMA kernel, a quarter of the fp64 kernel's time per iteration) and the fp64 kernel
// starts from those controls with the Hamiltonian model -- 3-4 fp64 iterations on the reference's grid instead of 8-9 (5 of
// them coarse).  Every returned number is the fp64 kernel's, every convergence test runs in fp64 on the NLP of CPDP.py:110-175:
// the fp32 solve only changes the path to its KKT point, as the mesh continuation does.  Measured on the benchmark's fp64 leg:
// DESIGN.md section 3.1, profiles/r04_w_mixed_precision_probe.txt.
// LFSD_F64_SEED=0 in the environment switches it off (the kernel-level tests that compare the fp64 kernel's own iterates).
static bool seeded_f64(int dtype, int batch, int exact_after, int mapping, bool bounded) {
  const char* e = getenv("LFSD_F64_SEED");
  if (e && atoi(e) == 0) return false;
  return OC_PK && dtype == LFSD_F64 && !bounded && exact_after != 0 &&
         !use_wide(dtype, batch, exact_after, mapping, bounded);
}
// staging area behind the fp64 scratch (byte offsets from its end, 256-byte aligned)
struct SeedLayout {
  size_t ws32, x0, hz, th, cs, xs, us, ls, cost, it, st, u0, ui, end;
  SeedLayout(int batch, int n_grid, int const_rows) {
    const size_t B = (size_t)batch, N1 = (size_t)n_grid + 1;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) / 256 * 256; return at; };
    ws32 = take((size_t)padded_batch(batch) * (size_t)lfsd::OcLayout<Model>::template ws_elems<G>(n_grid) * 4);
    x0 = take(B * Model::NX * 4); hz = take(B * 4); th = take(B * Model::NP * 4);
    cs = take(B * (size_t)(Model::NC > 0 ? Model::NC : 1) * 4);      // (sized for per-trajectory constants whatever the call passes)
    xs = take(B * N1 * Model::NX * 4); us = take(B * N1 * Model::NU * 4); ls = take(B * N1 * Model::NX * 4);
    cost = take(B * 4); it = take(B * 4); st = take(B * 4);
    u0 = take(B * (size_t)n_grid * Model::NU * 8);
    ui = take(B * (size_t)n_grid * Model::NU * 4);      // the caller's initial guess in fp32 (rows of zeros = cold start)
    end = o; (void)const_rows;
  }
  size_t total(size_t f64_bytes) const { return (f64_bytes + 255) / 256 * 256 + end; }
};

// ---- wide mapping with several wavefronts per trajectory (oc_solve_wide_kernel<..., W>; fp32, the models whose interval-parallel
// phases take several rounds of one wavefront: rocket, quadrotor) ----
// A wide launch lasts as long as its slowest trajectory (rocket learner step: median 53 iterations, slowest 160), and for most of that
// time most SIMDs hold a finished workgroup.  A workgroup of WIDE_W wavefronts runs the two interval-parallel phases of ONE trajectory
// (exact stage Hessians + linearisation: 53 % of a rocket iteration) on the four SIMDs of a CU; a CU holds one such workgroup (512
// registers per wavefront, 116 KB of LDS).  So:  batch <= CUs -- every trajectory gets such a workgroup from the start;  otherwise the
// solve is TWO launches on the stream: one wavefront per trajectory until all but `CUs` trajectories are finished (a device counter;
// the rest park their solver state in the workspace), then the rest with WIDE_W wavefronts each.  No host read in between: the second
// launch is enqueued unconditionally, one workgroup per entry of the hand-over list the first one wrote (the others leave at once).  Same arithmetic per item whoever runs it:
// results do not depend on when a trajectory was handed over (asserted by the GPU tier: bit-identical to the one-launch solve).
// Environment (test hooks / A-B): LFSD_WIDE_WAVES=1 one wavefront per trajectory always, =4 WIDE_W from the start at any batch;
// LFSD_WIDE_CAPACITY=<n> in place of the CU count; LFSD_WIDE_SUSPEND_IT=<k> hand over at iteration k instead of by the counter.
static constexpr int WIDE_W = 4;
template <typename T> static constexpr bool wide_multi() { return sizeof(T) == 4 && !lfsd::OcLayout<Model>::HALL; }
static int env_int(const char* name, int dflt) { const char* e = getenv(name); return (e && *e) ? atoi(e) : dflt; }
static size_t wide_sched_offset(size_t solver_bytes) { return (solver_bytes + 255) / 256 * 256; }      // the counters + hand-over list behind the solver scratch
static size_t wide_sched_bytes(int batch) { return ((size_t)(2 + batch) * sizeof(int) + 255) / 256 * 256; }

// exactly what lfsd_coc_solve needs for the mapping the same arguments select (ABI 6; ABI 5 returned the larger of the two
// layouts whatever the batch: 9.6 GB instead of 6.4 GB at 32768 quadrotor trajectories)
LFSD_API size_t lfsd_coc_workspace_bytes(int dtype, int batch, int n_grid, int exact_after, int mapping, int bounded) {
  if (batch <= 0 || n_grid <= 0 || (dtype != LFSD_F32 && dtype != LFSD_F64)) return 0;
  if (mapping < LFSD_MAP_AUTO || mapping > LFSD_MAP_WIDE) return 0;
  const size_t es = dtype == LFSD_F32 ? 4 : 8;
  if (use_wide(dtype, batch, exact_after, mapping, bounded != 0))
    return wide_sched_offset((size_t)batch * (size_t)lfsd::OcLayout<Model>::ws_elems_wide(n_grid) * es) + wide_sched_bytes(batch);
  const size_t lock = (size_t)padded_batch(batch) * (size_t)lfsd::OcLayout<Model>::template ws_elems<G>(n_grid) * es;
  if (seeded_f64(dtype, batch, exact_after, mapping, bounded != 0)) return SeedLayout(batch, n_grid, 1).total(lock);
  return lock;
}

static int coc_solve_seeded(int batch, int n_grid, int steps_per_grid, const void* ini_state, const void* horizon,
                            const void* auxvar, const void* consts, int const_per_traj, const void* u_init, void* state_grid,
                            void* control_grid, void* costate_grid, void* cost, int* iters, int* status, int max_iter, double tol,
                            int exact_after, int mapping, void* workspace, size_t workspace_bytes, void* stream);

template <typename T>
static int coc_solve_t(int batch, int n_grid, int steps_per_grid, const void* ini_state, const void* horizon,
                       const void* auxvar, const void* consts, int const_per_traj, const void* u_init,
                       const void* control_lb, const void* control_ub,
                       const void* state_lb, const void* state_ub, const void* state_mult, double state_rho,
                       void* state_grid, void* control_grid, void* costate_grid, void* cost, int* iters, int* status,
                       int max_iter, double tol, int exact_after, int mapping, void* workspace, size_t workspace_bytes,
                       void* stream, int start_mode = 0) {
  if constexpr (sizeof(T) == 8) {
    // (start_mode 1 marks the fp64 half of a seeded solve: it must not seed itself again)
    // (and a caller-held workspace sized while LFSD_F64_SEED=0 was in the environment has no staging area: that solve runs
    //  unseeded instead of failing with LFSD_ENOSPC -- the seed changes the path to the KKT point, not the point)
    if (start_mode == 0 && seeded_f64(LFSD_F64, batch, exact_after, mapping, control_lb != nullptr) &&
        workspace_bytes >= SeedLayout(batch, n_grid, 1).total((size_t)padded_batch(batch) * (size_t)lfsd::OcLayout<Model>::template ws_elems<G>(n_grid) * 8))
      return coc_solve_seeded(batch, n_grid, steps_per_grid, ini_state, horizon, auxvar, consts, const_per_traj, u_init, state_grid,
                              control_grid, costate_grid, cost, iters, status, max_iter, tol, exact_after, mapping, workspace,
                              workspace_bytes, stream);
  }
  lfsd::OcArgs<T> a;
  a.sched = nullptr; a.suspend_at = 0; a.suspend_it = -1;
  a.batch = batch; a.n_grid = n_grid; a.steps_per_grid = steps_per_grid; a.max_iter = max_iter;
  a.ini_state = (const T*)ini_state; a.horizon = (const T*)horizon; a.auxvar = (const T*)auxvar;
  a.consts = consts ? (const T*)consts : (const T*)horizon;      // NC_REAL == 0: any readable word, never used
  a.const_stride = (consts && const_per_traj) ? Model::NC : 0;
  a.u_init = (const T*)u_init;
  a.u_lb = (const T*)control_lb; a.u_ub = (const T*)control_ub;
  a.x_lb = (const T*)state_lb; a.x_ub = (const T*)state_ub; a.x_mult = (const T*)state_mult; a.x_rho = (T)state_rho;
  a.state_grid = (T*)state_grid; a.control_grid = (T*)control_grid; a.costate_grid = (T*)costate_grid;
  a.cost = (T*)cost; a.iters = iters; a.status = status;
  a.ws = (T*)workspace; a.ws_stride = lfsd::OcLayout<Model>::template ws_elems<G>(n_grid);
  a.tol = (T)tol;
  a.exact_after = exact_after;
  a.mu_stage_frac = (exact_after == 0) ? (T)(lfsd::kMuStageFracNewton) : T(0);
  a.start_mode = start_mode;
  if (use_wide(sizeof(T) == 4 ? LFSD_F32 : LFSD_F64, batch, exact_after, mapping, control_lb != nullptr)) {       // bounded problems: the wide kernel at every batch size
    a.ws_stride = lfsd::OcLayout<Model>::ws_elems_wide(n_grid);
    const size_t solver_bytes = (size_t)batch * (size_t)a.ws_stride * sizeof(T);
    if (workspace_bytes < solver_bytes) return LFSD_ENOSPC;
    a.it_start = 0; a.resume = 0; a.max_iter_total = max_iter;
    a.sched = nullptr; a.suspend_at = 0; a.suspend_it = -1;
    if (control_lb) { LFSD_LAUNCH((lfsd::oc_solve_wide_kernel<Model, T, true, true>), (unsigned)batch, 64, stream, a); }
    else if (exact_after < 0) { LFSD_LAUNCH((lfsd::oc_solve_wide_kernel<Model, T, false>), (unsigned)batch, 64, stream, a); }
    else {
      if constexpr (wide_multi<T>()) {
        const int waves = env_int("LFSD_WIDE_WAVES", 0);
        const int cap = std::max(1, env_int("LFSD_WIDE_CAPACITY", device_cu_count()));
        if (waves == WIDE_W || (waves == 0 && batch <= cap)) {
          LFSD_LAUNCH((lfsd::oc_solve_wide_kernel<Model, T, true, false, WIDE_W>), (unsigned)batch, 64 * WIDE_W, stream, a);
          return launch_status();
        }
        if (waves == 0 && max_iter > 8 && workspace_bytes >= wide_sched_offset(solver_bytes) + wide_sched_bytes(batch)) {
          a.sched = (int*)((char*)workspace + wide_sched_offset(solver_bytes));
          a.suspend_at = batch - cap;
          a.suspend_it = env_int("LFSD_WIDE_SUSPEND_IT", -1);
          LFSD_ZERO(a.sched, 2 * sizeof(int), stream);
          LFSD_LAUNCH((lfsd::oc_solve_wide_kernel<Model, T, true>), (unsigned)batch, 64, stream, a);
          int rc = launch_status();
          if (rc) return rc;
          // (by the counter at most `cap` trajectories are handed over: all but suspend_at = batch - cap were finished; the test hook may hand over all)
          a.resume = 2;
          LFSD_LAUNCH((lfsd::oc_solve_wide_kernel<Model, T, true, false, WIDE_W>), (unsigned)(a.suspend_it >= 0 ? batch : cap), 64 * WIDE_W, stream, a);
          return launch_status();
        }
      }
      LFSD_LAUNCH((lfsd::oc_solve_wide_kernel<Model, T, true>), (unsigned)batch, 64, stream, a);
    }
    return launch_status();
  }
  const size_t need = (size_t)padded_batch(batch) * (size_t)a.ws_stride * sizeof(T);
  if (workspace_bytes < need) return LFSD_ENOSPC;
  const unsigned grid = (unsigned)(padded_batch(batch) / GPB);
  a.it_start = 0; a.resume = 0; a.max_iter_total = max_iter;
  // fp32: packed roll-out (+ MFMA sweep); fp64: one live column per lane of a 16-lane group (OcSolver::rollout_sens_live)
  constexpr bool PK = OC_PK && (sizeof(T) == 4 || lfsd::OcLayout<Model>::LIVE <= 16);
  const unsigned grid_lean = PK ? (unsigned)(padded_batch(batch) / OC_GPB) : grid;
  if (exact_after < 0) {                       // Gauss-Newton / Hamiltonian models only
    LFSD_LAUNCH((lfsd::oc_solve_kernel<Model, T, G, false, PK>), grid_lean, 64, stream, a);
    return launch_status();
  }
  if (exact_after == 0) {                      // Newton from the first iteration
    LFSD_LAUNCH((lfsd::oc_solve_kernel<Model, T, G, true>), grid, 64, stream, a);
    return launch_status();
  }
  // default: lean kernel for the first `exact_after` iterations, then the exact-capable kernel resumes
  // (warm-started from control_grid) the trajectories that are still at MAXITER
  a.max_iter = max_iter < exact_after ? max_iter : exact_after;
  if (max_iter <= exact_after) a.max_iter_total = 0;      // no phase 2: never hand over
  LFSD_LAUNCH((lfsd::oc_solve_kernel<Model, T, G, false, PK>), grid_lean, 64, stream, a);
  int rc = launch_status();
  if (rc || max_iter <= exact_after) return rc;
  a.max_iter = max_iter; a.it_start = exact_after; a.resume = 1;
  LFSD_LAUNCH((lfsd::oc_solve_kernel<Model, T, G, true>), grid, 64, stream, a);
  return launch_status();
}

// `u_init` (may be NULL): the caller's initial guess.  The fp32 solve starts from it too -- an all-zero row is a cold start for both
// kernels, so a learner that hands zeros for every row but the ones it continues (SparseDemoLearner with skip_unconverged) gets
// every row seeded -- and a row the fp32 solve failed on starts the fp64 kernel from the caller's row.
static int coc_solve_seeded(int batch, int n_grid, int steps_per_grid, const void* ini_state, const void* horizon,
                            const void* auxvar, const void* consts, int const_per_traj, const void* u_init, void* state_grid,
                            void* control_grid, void* costate_grid, void* cost, int* iters, int* status, int max_iter, double tol,
                            int exact_after, int mapping, void* workspace, size_t workspace_bytes, void* stream) {
  const size_t f64_bytes = (size_t)padded_batch(batch) * (size_t)lfsd::OcLayout<Model>::template ws_elems<G>(n_grid) * 8;
  const SeedLayout L(batch, n_grid, 1);
  if (workspace_bytes < L.total(f64_bytes)) return LFSD_ENOSPC;
  char* base = (char*)workspace + (f64_bytes + 255) / 256 * 256;
  auto cast = [&](const void* src, void* dst, long long n, int to_f32) {
    lfsd::CastArgs c{src, dst, n, to_f32};
    LFSD_LAUNCH(lfsd::cast_kernel<void>, (unsigned)((n + 255) / 256), 256, stream, c);
  };
  cast(ini_state, base + L.x0, (long long)batch * Model::NX, 1);
  cast(horizon, base + L.hz, batch, 1);
  cast(auxvar, base + L.th, (long long)batch * Model::NP, 1);
  if (consts) cast(consts, base + L.cs, const_per_traj ? (long long)batch * Model::NC : (long long)Model::NC, 1);
  if (u_init) cast(u_init, base + L.ui, (long long)batch * n_grid * Model::NU, 1);
  int rc = launch_status();
  if (rc) return rc;
  const double tol32 = tol > 1e-6 ? tol : 1e-6;      // (runtime.py's default for an fp32 solve)
  rc = coc_solve_t<float>(batch, n_grid, steps_per_grid, base + L.x0, base + L.hz, base + L.th, consts ? base + L.cs : nullptr,
                          const_per_traj, u_init ? base + L.ui : nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, base + L.xs, base + L.us,
                          base + L.ls, base + L.cost, (int*)(base + L.it), (int*)(base + L.st), max_iter, tol32, exact_after,
                          LFSD_MAP_LOCKSTEP, base + L.ws32, L.x0 - L.ws32, stream);
  if (rc) return rc;
  {
    lfsd::SeedArgs sa{(const float*)(base + L.us), (const float*)(base + L.cost), (const int*)(base + L.st), (const double*)u_init,
                      (double*)(base + L.u0), batch, n_grid, Model::NU};
    const long long n = (long long)batch * n_grid * Model::NU;
    LFSD_LAUNCH(lfsd::seed_controls_kernel<void>, (unsigned)((n + 255) / 256), 256, stream, sa);
  }
  rc = coc_solve_t<double>(batch, n_grid, steps_per_grid, ini_state, horizon, auxvar, consts, const_per_traj, base + L.u0, nullptr,
                           nullptr, nullptr, nullptr, nullptr, 0.0, state_grid, control_grid, costate_grid, cost, iters, status,
                           max_iter, tol, exact_after, mapping, workspace, f64_bytes, stream, /*start_mode=*/1);
  if (rc) return rc;
  lfsd::AddItersArgs ia{iters, (const int*)(base + L.it), batch};      // iterations reported: both solves
  LFSD_LAUNCH(lfsd::add_iters_kernel<void>, (unsigned)((batch + 255) / 256), 256, stream, ia);
  return launch_status();
}

LFSD_API int lfsd_coc_solve(int dtype, int batch, int n_grid, int steps_per_grid, const void* ini_state,
                              const void* horizon, const void* auxvar, const void* consts, int const_per_traj,
                              const void* u_init, const void* control_lb, const void* control_ub,
                              const void* state_lb, const void* state_ub, const void* state_mult, double state_rho,
                              void* state_grid, void* control_grid, void* costate_grid, void* cost,
                              int* iters, int* status, int max_iter, double tol, int exact_after, int mapping,
                              void* workspace, size_t workspace_bytes, void* stream) {
  if (batch <= 0 || n_grid <= 0 || steps_per_grid <= 0 || max_iter < 0 || !(tol >= 0)) return LFSD_EINVAL;
  if (mapping < LFSD_MAP_AUTO || mapping > LFSD_MAP_WIDE) return LFSD_EINVAL;
  if (steps_per_grid > lfsd::OcLayout<Model>::SMAX) return LFSD_EINVAL;
  if (!ini_state || !horizon || !auxvar || !state_grid || !control_grid || !costate_grid || !cost || !iters ||
      !status || !workspace)
    return LFSD_EINVAL;
  if (Model::NC_REAL > 0 && !consts) return LFSD_EINVAL;
  if ((control_lb == nullptr) != (control_ub == nullptr)) return LFSD_EINVAL;
  // state bounds: all three arrays or none, a positive penalty, and the control-bound arrays beside them (the bounded
  // kernel reads both boxes; entries of +-1e20 mean "no bound")
  if (state_lb || state_ub || state_mult) {
    if (!state_lb || !state_ub || !state_mult || !control_lb || !(state_rho > 0)) return LFSD_EINVAL;
  }
  if (dtype == LFSD_F32)
    return coc_solve_t<float>(batch, n_grid, steps_per_grid, ini_state, horizon, auxvar, consts, const_per_traj, u_init,
                              control_lb, control_ub, state_lb, state_ub, state_mult, state_rho, state_grid, control_grid, costate_grid,
                              cost, iters, status, max_iter, tol, exact_after, mapping, workspace, workspace_bytes, stream);
  if (dtype == LFSD_F64)
    return coc_solve_t<double>(batch, n_grid, steps_per_grid, ini_state, horizon, auxvar, consts, const_per_traj,
                               u_init, control_lb, control_ub, state_lb, state_ub, state_mult, state_rho, state_grid, control_grid,
                               costate_grid, cost, iters, status, max_iter, tol, exact_after, mapping, workspace, workspace_bytes, stream);
  return LFSD_EINVAL;
}

template <typename T>
static int aux_phase_t(int phases, int batch, int n_grid, const void* horizon, const void* auxvar, const void* consts,
                       int const_per_traj, const void* state_grid, const void* control_grid, const void* costate_grid,
                       void* Z_grid, int n_waypoints, int n_iface, const int* iface_idx, const void* taus,
                       const void* waypoints, void* loss, void* grad, void* auxX_grid, void* auxU_grid, int substeps,
                       double rtol, int* stats, const int* oc_status, int skip_mask, void* stream,
                       const void* state_curv = nullptr, const void* control_curv = nullptr, const void* costate_curv = nullptr,
                       const void* wp_weight = nullptr) {
  // (interpolation level 2 when the three curvature grids are given: the level-1 launches take the AuxArgs base, as ever)
  lfsd::AuxArgsCubic<T> a;
  const bool cubic = state_curv != nullptr;
  a.state_curv = (const T*)state_curv; a.control_curv = (const T*)control_curv; a.costate_curv = (const T*)costate_curv;
  // rtol > 0: error-controlled sub-stepping from `substeps` (default 1) units per interval upwards;
  // rtol = 0: a fixed minimum of `substeps` (default 4) units, refined for stiffness only (the round-1 behaviour)
  a.batch = batch; a.n_grid = n_grid; a.substeps = substeps > 0 ? substeps : (rtol > 0 ? 1 : 4);
  a.rtol = (T)rtol;
  // Stiffness cap of a split unit: dt * |Huu^-1 fu^T P fu| <= 8 / substeps (substeps = 4 -> 2), and at most max_refine x
  // `substeps` units per interval.  The last interval before a heavy final cost is the hard one: on the robot arm
  // (h_xx = 200, control weight 0.5) dgrid * rate is ~2000 there, the splitting is stiffly accurate to ~1e-4 at any unit
  // count below a few hundred, and leaves that plateau only once dt * rate < 1 -- thousands of units (profiles/
  // r04_d_dudtheta_refinement.txt).  The error control sees it (such an interval is reported in `stats` as accepted above
  // rtol when the cap binds), but with the default cap a tolerance below 1e-3 could not be met there: a tighter rtol therefore
  // tightens the stiffness cap (fourth root: the extrapolated pair is fourth order in dt * rate) and widens max_refine with
  // it.  At rtol >= 1e-3 -- the reference's own tolerance, the default -- nothing changes.
  const double tight = (rtol > 0 && rtol < 1e-3) ? std::pow(1e-3 / rtol, 0.25) : 1.0;
  a.rate_max = (T)(8.0 / a.substeps / tight);
  a.max_refine = 256;
  while (a.max_refine < 256 * tight && a.max_refine < 16384) a.max_refine *= 2;
  // a budget of 24 units per interval on average (twice what a well-posed robot-arm row spends, ten times a quadrotor row; 64 until
  // round 5: the diverged rows of one learner step then held both sweeps at 12-14 ms against 2.1 / 1.2) for rows whose OC solve did
  // not converge (status not 1 / 2; needs oc_status): rows
  // a fixed learning rate has driven to parameters of 1e14 refined EVERY interval to the cap (8 864 units against the 565 of
  // a well-posed robot-arm row: Riccati launch 35 ms against 2.1, profiles/r04_l_steps_robotarm_fast_trig.txt); what they
  // return is flagged in `stats`.  Converged rows are never budgeted (a stiff last interval alone may need thousands of units).
  a.unit_budget = (int)std::min<double>(24.0 * n_grid * a.substeps * tight, (double)(1LL << 30));      // (in double: the fourth-root factor must not truncate to 1)
  a.horizon = (const T*)horizon; a.auxvar = (const T*)auxvar;
  a.consts = consts ? (const T*)consts : (const T*)horizon;
  a.const_stride = (consts && const_per_traj) ? Model::NC : 0;
  a.state_grid = (const T*)state_grid; a.control_grid = (const T*)control_grid; a.costate_grid = (const T*)costate_grid;
  a.Z_grid = (T*)Z_grid;
  a.n_waypoints = n_waypoints; a.n_iface = n_iface; a.iface_idx = iface_idx;
  a.taus = (const T*)taus; a.waypoints = (const T*)waypoints;
  a.loss = (T*)loss; a.grad = (T*)grad; a.auxX_grid = (T*)auxX_grid; a.auxU_grid = (T*)auxU_grid;
  a.stats = stats;
  a.oc_status = oc_status; a.skip_mask = skip_mask;      // (the status also decides which rows the unit budget applies to)
  const unsigned grid = (unsigned)(((long long)batch + GPB - 1) / GPB);
  if (phases & 1) {
    int rc;
    if constexpr (sizeof(T) == 4) rc = cubic ? lfsd_detail::launch_riccati_cubic_f32(grid, stream, a) : lfsd_detail::launch_riccati_f32(grid, stream, a);
    else rc = cubic ? lfsd_detail::launch_riccati_cubic_f64(grid, stream, a) : lfsd_detail::launch_riccati_f64(grid, stream, a);
    if (rc) return rc;
  }
  if (phases & 2) {
    // the forward sweep packs more trajectories into a wavefront than the Riccati sweep (lfsd::fwd_lanes)
    constexpr int GF = lfsd::fwd_lanes<Model>() < G ? lfsd::fwd_lanes<Model>() : G;
    constexpr int GPBF = 64 / GF;
    const unsigned grid_f = (unsigned)(((long long)batch + GPBF - 1) / GPBF);
    if (wp_weight) {      // (ABI 16: the weighted sweeps are kernels of their own; without weights the launches below, as ever)
      if constexpr (sizeof(T) == 4) return lfsd_detail::launch_forward_weighted_f32(grid_f, stream, a, cubic, (const float*)wp_weight);
      else return lfsd_detail::launch_forward_weighted_f64(grid_f, stream, a, cubic, (const double*)wp_weight);
    }
    if (cubic) {
      if constexpr (sizeof(T) == 4) return lfsd_detail::launch_forward_cubic_f32(grid_f, stream, a);
      else return lfsd_detail::launch_forward_cubic_f64(grid_f, stream, a);
    }
    const lfsd::AuxArgs<T>& a1 = a;
    LFSD_LAUNCH((lfsd::aux_forward_kernel<Model, T, GF>), grid_f, 64, stream, a1);
    return launch_status();
  }
  return 0;
}

static int aux_dispatch(int phases, int dtype, int batch, int n_grid, const void* horizon, const void* auxvar,
                        const void* consts, int const_per_traj, const void* state_grid, const void* control_grid,
                        const void* costate_grid, void* Z_grid, int n_waypoints, int n_iface, const int* iface_idx,
                        const void* taus, const void* waypoints, void* loss, void* grad, void* auxX_grid,
                        void* auxU_grid, int substeps, double rtol, int* stats, const int* oc_status, int skip_mask,
                        void* stream, int level = 1, const void* state_curv = nullptr, const void* control_curv = nullptr,
                        const void* costate_curv = nullptr, const void* wp_weight = nullptr) {
  if (level == 2 && (!state_curv || !control_curv || !costate_curv || n_grid < 3)) return LFSD_EINVAL;      // (scipy's cubic needs four nodes)
  if (level != 2) state_curv = control_curv = costate_curv = nullptr;
  if (batch <= 0 || n_grid <= 0 || n_waypoints < 0 || n_iface < 0 || substeps < 0 || !(rtol >= 0)) return LFSD_EINVAL;
  if (!horizon || !auxvar || !state_grid || !control_grid || !costate_grid || !Z_grid) return LFSD_EINVAL;
  if ((phases & 2) && (!loss || !grad)) return LFSD_EINVAL;
  if ((phases & 2) && n_waypoints > 0 && (n_iface <= 0 || !taus || !waypoints)) return LFSD_EINVAL;
  // iface_idx == NULL selects the interface function compiled into the library: it must exist and n_iface must be its size
  if ((phases & 2) && n_waypoints > 0 && !iface_idx && (Model::NIF == 0 || n_iface != Model::NIF)) return LFSD_EINVAL;
  if (Model::NC_REAL > 0 && !consts) return LFSD_EINVAL;
  if (skip_mask < 0 || (skip_mask != 0 && !oc_status)) return LFSD_EINVAL;
  if (dtype == LFSD_F32)
    return aux_phase_t<float>(phases, batch, n_grid, horizon, auxvar, consts, const_per_traj, state_grid, control_grid,
                              costate_grid, Z_grid, n_waypoints, n_iface, iface_idx, taus, waypoints, loss, grad,
                              auxX_grid, auxU_grid, substeps, rtol, stats, oc_status, skip_mask, stream, state_curv, control_curv,
                              costate_curv, wp_weight);
  if (dtype == LFSD_F64)
    return aux_phase_t<double>(phases, batch, n_grid, horizon, auxvar, consts, const_per_traj, state_grid,
                               control_grid, costate_grid, Z_grid, n_waypoints, n_iface, iface_idx, taus, waypoints,
                               loss, grad, auxX_grid, auxU_grid, substeps, rtol, stats, oc_status, skip_mask, stream, state_curv,
                               control_curv, costate_curv, wp_weight);
  return LFSD_EINVAL;
}

LFSD_API int lfsd_aux_solve(int dtype, int batch, int n_grid, const void* horizon, const void* auxvar,
                            const void* consts, int const_per_traj, const void* state_grid, const void* control_grid,
                            const void* costate_grid, void* Z_grid, int n_waypoints, int n_iface,
                            const int* iface_idx, const void* taus, const void* waypoints, void* loss, void* grad,
                            void* auxX_grid, void* auxU_grid, int substeps, double rtol, int* stats,
                            const int* oc_status, int skip_status_mask, void* stream) {
  return aux_dispatch(3, dtype, batch, n_grid, horizon, auxvar, consts, const_per_traj, state_grid, control_grid,
                      costate_grid, Z_grid, n_waypoints, n_iface, iface_idx, taus, waypoints, loss, grad, auxX_grid,
                      auxU_grid, substeps, rtol, stats, oc_status, skip_status_mask, stream);
}

LFSD_API int lfsd_aux_riccati(int dtype, int batch, int n_grid, const void* horizon, const void* auxvar,
                              const void* consts, int const_per_traj, const void* state_grid,
                              const void* control_grid, const void* costate_grid, void* Z_grid, int substeps,
                              double rtol, int* stats, const int* oc_status, int skip_status_mask, void* stream) {
  return aux_dispatch(1, dtype, batch, n_grid, horizon, auxvar, consts, const_per_traj, state_grid, control_grid,
                      costate_grid, Z_grid, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                      substeps, rtol, stats, oc_status, skip_status_mask, stream);
}

LFSD_API int lfsd_aux_forward(int dtype, int batch, int n_grid, const void* horizon, const void* auxvar,
                              const void* consts, int const_per_traj, const void* state_grid,
                              const void* control_grid, const void* costate_grid, const void* Z_grid, int n_waypoints,
                              int n_iface, const int* iface_idx, const void* taus, const void* waypoints, void* loss,
                              void* grad, void* auxX_grid, void* auxU_grid, int substeps, double rtol, int* stats,
                              const int* oc_status, int skip_status_mask, void* stream) {
  return aux_dispatch(2, dtype, batch, n_grid, horizon, auxvar, consts, const_per_traj, state_grid, control_grid,
                      costate_grid, const_cast<void*>(Z_grid), n_waypoints, n_iface, iface_idx, taus, waypoints, loss,
                      grad, auxX_grid, auxU_grid, substeps, rtol, stats, oc_status, skip_status_mask, stream);
}

template <typename T>
static int opt_step_t(int method, int batch, int n_param, int iter_idx, double lr, double mu, double beta1,
                      double beta2, double eps, void* theta, const void* grad, void* m, void* v, void* vhat,
                      const void* proj_lo, const int* row_active, void* stream) {
  lfsd::OptArgs<T> a;
  a.batch = batch; a.n_param = n_param; a.method = method; a.iter_idx = iter_idx;
  a.lr = (T)lr; a.mu = (T)mu; a.beta1 = (T)beta1; a.beta2 = (T)beta2; a.eps = (T)eps;
  a.theta = (T*)theta; a.grad = (const T*)grad; a.m = (T*)m; a.v = (T*)v; a.vhat = (T*)vhat;
  a.proj_lo = (const T*)proj_lo; a.row_active = row_active;
  const long long n = (long long)batch * n_param;
  const unsigned grid = (unsigned)((n + 63) / 64);
  LFSD_LAUNCH((lfsd::optimizer_kernel<T>), grid, 64, stream, a);
  return launch_status();
}

LFSD_API int lfsd_optimizer_step(int dtype, int method, int batch, int n_param, int iter_idx, double lr, double mu,
                                   double beta1, double beta2, double eps, void* theta, const void* grad, void* m,
                                   void* v, void* vhat, const void* proj_lo, const int* row_active, void* stream) {
  if (batch <= 0 || n_param <= 0 || iter_idx < 0 || !theta || !grad) return LFSD_EINVAL;
  if (method < LFSD_OPT_VANILLA || method > LFSD_OPT_AMSGRAD) return LFSD_EINVAL;
  if (method == LFSD_OPT_NESTEROV && !m) return LFSD_EINVAL;
  if (method >= LFSD_OPT_ADAM && (!m || !v)) return LFSD_EINVAL;
  if (method == LFSD_OPT_AMSGRAD && !vhat) return LFSD_EINVAL;
  if (dtype == LFSD_F32)
    return opt_step_t<float>(method, batch, n_param, iter_idx, lr, mu, beta1, beta2, eps, theta, grad, m, v, vhat,
                             proj_lo, row_active, stream);
  if (dtype == LFSD_F64)
    return opt_step_t<double>(method, batch, n_param, iter_idx, lr, mu, beta1, beta2, eps, theta, grad, m, v, vhat,
                              proj_lo, row_active, stream);
  return LFSD_EINVAL;
}

LFSD_API int lfsd_lookahead(int dtype, long long n, double mu, const void* theta, const void* v, void* out,
                              void* stream) {
  if (n <= 0 || !theta || !v || !out) return LFSD_EINVAL;
  const unsigned grid = (unsigned)((n + 63) / 64);
  if (dtype == LFSD_F32) {
    const float muf = (float)mu; const float* th = (const float*)theta; const float* vv = (const float*)v; float* o = (float*)out;
#if defined(LFSD_EMU)
    emu::launch(dim3(grid), dim3(64), [&] { lfsd::lookahead_kernel<float>(n, muf, th, vv, o); });
#else
    hipLaunchKernelGGL((lfsd::lookahead_kernel<float>), dim3(grid), dim3(64), 0, (hipStream_t)stream, n, muf, th, vv, o);
#endif
    return launch_status();
  }
  if (dtype == LFSD_F64) {
    const double* th = (const double*)theta; const double* vv = (const double*)v; double* o = (double*)out;
#if defined(LFSD_EMU)
    emu::launch(dim3(grid), dim3(64), [&] { lfsd::lookahead_kernel<double>(n, mu, th, vv, o); });
#else
    hipLaunchKernelGGL((lfsd::lookahead_kernel<double>), dim3(grid), dim3(64), 0, (hipStream_t)stream, n, mu, th, vv, o);
#endif
    return launch_status();
  }
  return LFSD_EINVAL;
}

// ---- per-seed stop rule and the rows of a shrinking batch (cpdp_rows.h; lib/QuadAlgorithm.py:239-257) ----
// The emulator runs every lane as a fiber with a stack of its own: its launches stay small (two wavefronts still cross the LDS
// hand-over of the compaction).
#if defined(LFSD_EMU)
static constexpr int kStopBlock = 128, kCopyBlock = 64, kCopyMaxGrid = 4;
#else
static constexpr int kStopBlock = 1024, kCopyBlock = 256, kCopyMaxGrid = 2048;
#endif

template <typename T>
static int stop_compact_t(int n_rows, int n_param, const void* loss, const void* grad, const int* rows_in, const int* eligible,
                          double loss_tol, double grad_tol, int iter_idx, int* rows_out, int* pos_out, int* n_out, int* active,
                          int* stop_iter, void* stream) {
  lfsd::StopArgs<T> a;
  a.n_rows = n_rows; a.n_param = n_param; a.iter_idx = iter_idx;
  a.loss_tol = (T)loss_tol; a.grad_tol = (T)grad_tol;
  a.loss = (const T*)loss; a.grad = (const T*)grad; a.rows_in = rows_in; a.eligible = eligible;
  a.rows_out = rows_out; a.pos_out = pos_out; a.n_out = n_out; a.active = active; a.stop_iter = stop_iter;
  const int block = std::min(kStopBlock, (n_rows + 63) / 64 * 64);      // whole wavefronts
  LFSD_LAUNCH((lfsd::stop_compact_kernel<T>), 1u, (unsigned)block, stream, a);
  return launch_status();
}

LFSD_API int lfsd_stop_compact(int dtype, int n_rows, int n_param, const void* loss, const void* grad, const int* rows_in,
                               const int* eligible, double loss_tol, double grad_tol, int iter_idx, int* rows_out, int* pos_out,
                               int* n_out, int* active, int* stop_iter, void* stream) {
  if (n_rows <= 0 || n_param <= 0 || iter_idx < 0 || loss_tol != loss_tol || grad_tol != grad_tol) return LFSD_EINVAL;
  if (!loss || !grad || !rows_out || !pos_out || !n_out || !active || !stop_iter) return LFSD_EINVAL;
  if (rows_in && rows_in == rows_out) return LFSD_EINVAL;
  if (dtype == LFSD_F32)
    return stop_compact_t<float>(n_rows, n_param, loss, grad, rows_in, eligible, loss_tol, grad_tol, iter_idx, rows_out, pos_out,
                                 n_out, active, stop_iter, stream);
  if (dtype == LFSD_F64)
    return stop_compact_t<double>(n_rows, n_param, loss, grad, rows_in, eligible, loss_tol, grad_tol, iter_idx, rows_out, pos_out,
                                  n_out, active, stop_iter, stream);
  return LFSD_EINVAL;
}

static int copy_rows_launch(bool scatter, int n_rows, long long row_bytes, const int* index, const void* src, void* dst,
                            void* stream) {
  if (n_rows <= 0 || row_bytes <= 0 || !index || !src || !dst) return LFSD_EINVAL;
  const unsigned long long bits = (unsigned long long)row_bytes | (unsigned long long)(size_t)src | (unsigned long long)(size_t)dst;
  if (bits & 3ull) return LFSD_EINVAL;
  const bool wide = (bits & 15ull) == 0;
  lfsd::RowCopyArgs a;
  a.n_rows = n_rows; a.row_words = row_bytes / (wide ? 16 : 4); a.index = index; a.src = src; a.dst = dst;
  const long long total = (long long)n_rows * a.row_words;
  const unsigned grid = (unsigned)std::min<long long>((total + kCopyBlock - 1) / kCopyBlock, kCopyMaxGrid);
  if (scatter) {
    if (wide) { LFSD_LAUNCH((lfsd::scatter_rows_kernel<lfsd::RowWord16>), grid, kCopyBlock, stream, a); }
    else { LFSD_LAUNCH((lfsd::scatter_rows_kernel<unsigned>), grid, kCopyBlock, stream, a); }
  } else {
    if (wide) { LFSD_LAUNCH((lfsd::gather_rows_kernel<lfsd::RowWord16>), grid, kCopyBlock, stream, a); }
    else { LFSD_LAUNCH((lfsd::gather_rows_kernel<unsigned>), grid, kCopyBlock, stream, a); }
  }
  return launch_status();
}

LFSD_API int lfsd_gather_rows(int n_rows, long long row_bytes, const int* index, const void* src, void* dst, void* stream) {
  return copy_rows_launch(false, n_rows, row_bytes, index, src, dst, stream);
}

LFSD_API int lfsd_scatter_rows(int n_rows, long long row_bytes, const int* index, const void* src, void* dst, void* stream) {
  return copy_rows_launch(true, n_rows, row_bytes, index, src, dst, stream);
}

// ---- interpolation level 2 (ABI 11): the same three calls along the cubic interpolant of the grids (CPDP.py:388-390) ----
LFSD_API int lfsd_aux_solve_cubic(int dtype, int batch, int n_grid, const void* horizon, const void* auxvar,
                                  const void* consts, int const_per_traj, const void* state_grid, const void* control_grid,
                                  const void* costate_grid, const void* state_curv, const void* control_curv,
                                  const void* costate_curv, void* Z_grid, int n_waypoints, int n_iface,
                                  const int* iface_idx, const void* taus, const void* waypoints, void* loss, void* grad,
                                  void* auxX_grid, void* auxU_grid, int substeps, double rtol, int* stats,
                                  const int* oc_status, int skip_status_mask, void* stream) {
  return aux_dispatch(3, dtype, batch, n_grid, horizon, auxvar, consts, const_per_traj, state_grid, control_grid,
                      costate_grid, Z_grid, n_waypoints, n_iface, iface_idx, taus, waypoints, loss, grad, auxX_grid,
                      auxU_grid, substeps, rtol, stats, oc_status, skip_status_mask, stream, 2, state_curv, control_curv,
                      costate_curv);
}

LFSD_API int lfsd_aux_riccati_cubic(int dtype, int batch, int n_grid, const void* horizon, const void* auxvar,
                                    const void* consts, int const_per_traj, const void* state_grid,
                                    const void* control_grid, const void* costate_grid, const void* state_curv,
                                    const void* control_curv, const void* costate_curv, void* Z_grid, int substeps,
                                    double rtol, int* stats, const int* oc_status, int skip_status_mask, void* stream) {
  return aux_dispatch(1, dtype, batch, n_grid, horizon, auxvar, consts, const_per_traj, state_grid, control_grid,
                      costate_grid, Z_grid, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                      substeps, rtol, stats, oc_status, skip_status_mask, stream, 2, state_curv, control_curv, costate_curv);
}

LFSD_API int lfsd_aux_forward_cubic(int dtype, int batch, int n_grid, const void* horizon, const void* auxvar,
                                    const void* consts, int const_per_traj, const void* state_grid,
                                    const void* control_grid, const void* costate_grid, const void* state_curv,
                                    const void* control_curv, const void* costate_curv, const void* Z_grid,
                                    int n_waypoints, int n_iface, const int* iface_idx, const void* taus,
                                    const void* waypoints, void* loss, void* grad, void* auxX_grid, void* auxU_grid,
                                    int substeps, double rtol, int* stats, const int* oc_status, int skip_status_mask,
                                    void* stream) {
  return aux_dispatch(2, dtype, batch, n_grid, horizon, auxvar, consts, const_per_traj, state_grid, control_grid,
                      costate_grid, const_cast<void*>(Z_grid), n_waypoints, n_iface, iface_idx, taus, waypoints, loss,
                      grad, auxX_grid, auxU_grid, substeps, rtol, stats, oc_status, skip_status_mask, stream, 2, state_curv,
                      control_curv, costate_curv);
}

// ---- ABI 16: a weight per waypoint in the fused loss.  wp_weight == NULL is the unweighted sibling, launch for launch ----
LFSD_API int lfsd_aux_forward_weighted(int dtype, int batch, int n_grid, const void* horizon, const void* auxvar,
                                       const void* consts, int const_per_traj, const void* state_grid,
                                       const void* control_grid, const void* costate_grid, const void* Z_grid, int n_waypoints,
                                       int n_iface, const int* iface_idx, const void* taus, const void* waypoints,
                                       const void* wp_weight, void* loss, void* grad, void* auxX_grid, void* auxU_grid,
                                       int substeps, double rtol, int* stats, const int* oc_status, int skip_status_mask,
                                       void* stream) {
  return aux_dispatch(2, dtype, batch, n_grid, horizon, auxvar, consts, const_per_traj, state_grid, control_grid,
                      costate_grid, const_cast<void*>(Z_grid), n_waypoints, n_iface, iface_idx, taus, waypoints, loss,
                      grad, auxX_grid, auxU_grid, substeps, rtol, stats, oc_status, skip_status_mask, stream, 1, nullptr, nullptr,
                      nullptr, n_waypoints > 0 ? wp_weight : nullptr);
}

LFSD_API int lfsd_aux_forward_cubic_weighted(int dtype, int batch, int n_grid, const void* horizon, const void* auxvar,
                                             const void* consts, int const_per_traj, const void* state_grid,
                                             const void* control_grid, const void* costate_grid, const void* state_curv,
                                             const void* control_curv, const void* costate_curv, const void* Z_grid,
                                             int n_waypoints, int n_iface, const int* iface_idx, const void* taus,
                                             const void* waypoints, const void* wp_weight, void* loss, void* grad,
                                             void* auxX_grid, void* auxU_grid, int substeps, double rtol, int* stats,
                                             const int* oc_status, int skip_status_mask, void* stream) {
  return aux_dispatch(2, dtype, batch, n_grid, horizon, auxvar, consts, const_per_traj, state_grid, control_grid,
                      costate_grid, const_cast<void*>(Z_grid), n_waypoints, n_iface, iface_idx, taus, waypoints, loss,
                      grad, auxX_grid, auxU_grid, substeps, rtol, stats, oc_status, skip_status_mask, stream, 2, state_curv,
                      control_curv, costate_curv, n_waypoints > 0 ? wp_weight : nullptr);
}

// curvature grids of the not-a-knot cubic spline through each component of a grid (cpdp_spline.h)
LFSD_API int lfsd_grid_curvature(int dtype, int batch, int n_grid, int n_comp, const void* grid, void* curv, void* stream) {
  if (batch <= 0 || n_grid < 3 || n_comp <= 0 || !grid || !curv || grid == curv) return LFSD_EINVAL;
  if (dtype == LFSD_F32) return lfsd_detail::launch_grid_curvature_f32(batch, n_grid, n_comp, (const float*)grid, (float*)curv, stream);
  if (dtype == LFSD_F64) return lfsd_detail::launch_grid_curvature_f64(batch, n_grid, n_comp, (const double*)grid, (double*)curv, stream);
  return LFSD_EINVAL;
}

// ---- ABI 12: the interpolants at arbitrary times, and the chain rule of a user-written loss (cpdp_sample.h) ----
// [lo, lo + bytes) and [p, p + other) overlap (a NULL `p` overlaps nothing)
static bool spans_overlap(const void* lo, unsigned long long bytes, const void* p, unsigned long long other) {
  if (!p) return false;
  const unsigned long long a = (unsigned long long)(size_t)lo, b = (unsigned long long)(size_t)p;
  return a < b + other && b < a + bytes;
}

LFSD_API int lfsd_sample_grid(int dtype, int batch, int n_grid, int n_comp, int n_times, int times_per_traj, const void* grid,
                              const void* curv, const void* horizon, const void* times, void* out, void* stream) {
  if (batch <= 0 || n_grid < 1 || n_comp <= 0 || n_times <= 0 || (times_per_traj != 0 && times_per_traj != 1)) return LFSD_EINVAL;
  if (curv && n_grid < 3) return LFSD_EINVAL;      // (scipy's cubic needs four nodes)
  if (!grid || !horizon || !times || !out) return LFSD_EINVAL;
  if (dtype != LFSD_F32 && dtype != LFSD_F64) return LFSD_EINVAL;
  const unsigned long long es = dtype == LFSD_F32 ? 4 : 8, B = (unsigned long long)batch;
  const unsigned long long grid_bytes = B * (unsigned long long)(n_grid + 1) * n_comp * es, out_bytes = B * n_times * n_comp * es;
  if (spans_overlap(out, out_bytes, grid, grid_bytes) || spans_overlap(out, out_bytes, curv, grid_bytes) ||
      spans_overlap(out, out_bytes, horizon, B * es) || spans_overlap(out, out_bytes, times, (times_per_traj ? B : 1ull) * n_times * es))
    return LFSD_EINVAL;
  if (dtype == LFSD_F32) {
    lfsd::SampleArgs<float> a{batch, n_grid, n_comp, n_times, times_per_traj, (const float*)grid, (const float*)curv,
                              (const float*)horizon, (const float*)times, (float*)out};
    return lfsd_detail::launch_grid_sample_f32(a, stream);
  }
  lfsd::SampleArgs<double> a{batch, n_grid, n_comp, n_times, times_per_traj, (const double*)grid, (const double*)curv,
                             (const double*)horizon, (const double*)times, (double*)out};
  return lfsd_detail::launch_grid_sample_f64(a, stream);
}

LFSD_API int lfsd_waypoint_vjp(int dtype, int batch, int n_grid, int n_state, int n_control, int n_param, int n_waypoints,
                               const void* horizon, const void* taus, const void* rx, const void* ru, const void* auxX_grid,
                               const void* auxU_grid, void* grad, void* stream) {
  if (batch <= 0 || n_grid < 1 || n_state <= 0 || n_control <= 0 || n_param <= 0 || n_waypoints <= 0) return LFSD_EINVAL;
  if (!horizon || !taus || !rx || !auxX_grid || !grad) return LFSD_EINVAL;
  if ((ru == nullptr) != (auxU_grid == nullptr)) return LFSD_EINVAL;
  if (dtype != LFSD_F32 && dtype != LFSD_F64) return LFSD_EINVAL;
  const unsigned long long es = dtype == LFSD_F32 ? 4 : 8, B = (unsigned long long)batch, K = (unsigned long long)n_waypoints;
  const unsigned long long nodes = B * (unsigned long long)(n_grid + 1) * n_param, gb = B * n_param * es;
  if (spans_overlap(grad, gb, horizon, B * es) || spans_overlap(grad, gb, taus, B * K * es) ||
      spans_overlap(grad, gb, rx, B * K * n_state * es) || spans_overlap(grad, gb, ru, B * K * n_control * es) ||
      spans_overlap(grad, gb, auxX_grid, nodes * n_state * es) || spans_overlap(grad, gb, auxU_grid, nodes * n_control * es))
    return LFSD_EINVAL;
  if (dtype == LFSD_F32) {
    lfsd::WaypointVjpArgs<float> a{batch, n_grid, n_state, n_control, n_param, n_waypoints, (const float*)horizon, (const float*)taus,
                                   (const float*)rx, (const float*)ru, (const float*)auxX_grid, (const float*)auxU_grid, (float*)grad};
    return lfsd_detail::launch_waypoint_vjp_f32(a, stream);
  }
  lfsd::WaypointVjpArgs<double> a{batch, n_grid, n_state, n_control, n_param, n_waypoints, (const double*)horizon, (const double*)taus,
                                  (const double*)rx, (const double*)ru, (const double*)auxX_grid, (const double*)auxU_grid, (double*)grad};
  return lfsd_detail::launch_waypoint_vjp_f64(a, stream);
}

// ---- ABI 13: hyper-parameter sweeps in one batch -- every row its own update rule and hyper-parameters, traces on the device
// (cpdp_opt.h; test/opt_methods_comparison.py, test/*_learning_rate_comparison.py, lib/QuadAlgorithm.py:244-252) ----
LFSD_API int lfsd_optimizer_step_rows(int dtype, int batch, int n_param, int iter_idx, const int* method, const void* hyper,
                                      void* theta, const void* grad, void* m, void* v, void* vhat, const void* proj_lo,
                                      const int* row_active, void* stream) {
  if (batch <= 0 || n_param <= 0 || iter_idx < 0) return LFSD_EINVAL;
  if (!method || !hyper || !theta || !grad || !m || !v || !vhat) return LFSD_EINVAL;      // (the batch may mix rules: all state)
  if (dtype == LFSD_F32) {
    lfsd::OptRowsArgs<float> a{batch, n_param, iter_idx, method, (const float*)hyper, (float*)theta, (const float*)grad, (float*)m,
                               (float*)v, (float*)vhat, (const float*)proj_lo, row_active};
    return lfsd_detail::launch_optimizer_rows_f32(a, stream);
  }
  if (dtype == LFSD_F64) {
    lfsd::OptRowsArgs<double> a{batch, n_param, iter_idx, method, (const double*)hyper, (double*)theta, (const double*)grad,
                                (double*)m, (double*)v, (double*)vhat, (const double*)proj_lo, row_active};
    return lfsd_detail::launch_optimizer_rows_f64(a, stream);
  }
  return LFSD_EINVAL;
}

LFSD_API int lfsd_lookahead_rows(int dtype, int batch, int n_param, const int* method, const void* hyper, const void* theta,
                                 const void* m, void* out, void* stream) {
  if (batch <= 0 || n_param <= 0 || !method || !hyper || !theta || !m || !out) return LFSD_EINVAL;
  if (dtype != LFSD_F32 && dtype != LFSD_F64) return LFSD_EINVAL;
  const unsigned long long bytes = (unsigned long long)batch * n_param * (dtype == LFSD_F32 ? 4 : 8);
  if (spans_overlap(out, bytes, theta, bytes) || spans_overlap(out, bytes, m, bytes)) return LFSD_EINVAL;
  if (dtype == LFSD_F32) {
    lfsd::LookaheadRowsArgs<float> a{batch, n_param, method, (const float*)hyper, (const float*)theta, (const float*)m, (float*)out};
    return lfsd_detail::launch_lookahead_rows_f32(a, stream);
  }
  lfsd::LookaheadRowsArgs<double> a{batch, n_param, method, (const double*)hyper, (const double*)theta, (const double*)m, (double*)out};
  return lfsd_detail::launch_lookahead_rows_f64(a, stream);
}

LFSD_API int lfsd_trace_append(int dtype, int batch, int n_param, int iter_idx, int capacity, const void* loss, const void* grad,
                               const void* theta, const int* row_active, void* loss_trace, void* gnorm_trace, void* theta_trace,
                               void* stream) {
  if (batch <= 0 || n_param <= 0 || capacity <= 0 || iter_idx < 0 || iter_idx >= capacity) return LFSD_EINVAL;
  if (!loss || !grad || !theta) return LFSD_EINVAL;
  if (!loss_trace && !gnorm_trace && !theta_trace) return LFSD_EINVAL;
  if (dtype == LFSD_F32) {
    lfsd::TraceArgs<float> a{batch, n_param, iter_idx, capacity, (const float*)loss, (const float*)grad, (const float*)theta,
                             row_active, (float*)loss_trace, (float*)gnorm_trace, (float*)theta_trace};
    return lfsd_detail::launch_trace_append_f32(a, stream);
  }
  if (dtype == LFSD_F64) {
    lfsd::TraceArgs<double> a{batch, n_param, iter_idx, capacity, (const double*)loss, (const double*)grad, (const double*)theta,
                              row_active, (double*)loss_trace, (double*)gnorm_trace, (double*)theta_trace};
    return lfsd_detail::launch_trace_append_f64(a, stream);
  }
  return LFSD_EINVAL;
}

// ---- ABI 14: Levenberg-Marquardt outer update from per-seed Gauss-Newton matrices (cpdp_lm.h; no counterpart in the reference) ----
static int normal_matrix_dispatch(int dtype, int batch, int n_grid, int n_state, int n_param, int n_waypoints, int n_iface,
                                  const int* iface_idx, const void* horizon, const void* taus, const void* wp_weight,
                                  const void* auxX_grid, void* H, void* stream) {
  if (batch <= 0 || n_grid < 1 || n_state <= 0 || n_param <= 0 || n_waypoints <= 0 || n_iface <= 0) return LFSD_EINVAL;
  if (!iface_idx || !horizon || !taus || !auxX_grid || !H) return LFSD_EINVAL;
  if (dtype != LFSD_F32 && dtype != LFSD_F64) return LFSD_EINVAL;
  const unsigned long long es = dtype == LFSD_F32 ? 4 : 8, B = (unsigned long long)batch, P = (unsigned long long)n_param;
  const unsigned long long hb = B * P * P * es;
  if (spans_overlap(H, hb, iface_idx, (unsigned long long)n_iface * sizeof(int)) || spans_overlap(H, hb, horizon, B * es) ||
      spans_overlap(H, hb, taus, B * n_waypoints * es) || spans_overlap(H, hb, wp_weight, B * n_waypoints * es) ||
      spans_overlap(H, hb, auxX_grid, B * (unsigned long long)(n_grid + 1) * P * n_state * es))
    return LFSD_EINVAL;
  if (dtype == LFSD_F32) {
    lfsd::NormalMatrixArgs<float> a{batch, n_grid, n_state, n_param, n_waypoints, n_iface, iface_idx, (const float*)horizon,
                                    (const float*)taus, (const float*)auxX_grid, (float*)H, (const float*)wp_weight};
    return lfsd_detail::launch_normal_matrix_f32(a, stream);
  }
  lfsd::NormalMatrixArgs<double> a{batch, n_grid, n_state, n_param, n_waypoints, n_iface, iface_idx, (const double*)horizon,
                                   (const double*)taus, (const double*)auxX_grid, (double*)H, (const double*)wp_weight};
  return lfsd_detail::launch_normal_matrix_f64(a, stream);
}

LFSD_API int lfsd_normal_matrix(int dtype, int batch, int n_grid, int n_state, int n_param, int n_waypoints, int n_iface,
                                const int* iface_idx, const void* horizon, const void* taus, const void* auxX_grid, void* H,
                                void* stream) {
  return normal_matrix_dispatch(dtype, batch, n_grid, n_state, n_param, n_waypoints, n_iface, iface_idx, horizon, taus, nullptr,
                                auxX_grid, H, stream);
}

// (ABI 16) H = sum_k w_k J_k^T J_k; wp_weight == NULL: lfsd_normal_matrix
LFSD_API int lfsd_normal_matrix_weighted(int dtype, int batch, int n_grid, int n_state, int n_param, int n_waypoints, int n_iface,
                                         const int* iface_idx, const void* horizon, const void* taus, const void* wp_weight,
                                         const void* auxX_grid, void* H, void* stream) {
  return normal_matrix_dispatch(dtype, batch, n_grid, n_state, n_param, n_waypoints, n_iface, iface_idx, horizon, taus, wp_weight,
                                auxX_grid, H, stream);
}

LFSD_API int lfsd_lm_step(int dtype, int batch, int n_param, double lambda_down, double lambda_up, double lambda_min,
                          double lambda_max, void* theta, void* loss_acc, void* grad_acc, void* H_acc, void* lambda,
                          void* theta_trial, const void* loss_t, const void* grad_t, const void* H_t, const void* proj_lo,
                          const int* row_active, int* accepted, void* stream) {
  if (batch <= 0 || n_param <= 0 || n_param > lfsd::LM_MAX_PARAM) return LFSD_EINVAL;
  if (!theta || !loss_acc || !grad_acc || !H_acc || !lambda || !theta_trial || !loss_t || !grad_t || !H_t) return LFSD_EINVAL;
  // (every comparison is false for a NaN: written so that a NaN scalar fails one of them)
  if (!(lambda_down > 0 && lambda_down <= 1) || !(lambda_up >= 1) || !(lambda_min > 0) || !(lambda_min <= lambda_max)) return LFSD_EINVAL;
  if (dtype == LFSD_F32) {
    // the same conditions on the values the kernel gets: 1e-50 is positive as a double and 0 as a float, and a damping of 0 stays 0
    const float dn = (float)lambda_down, up = (float)lambda_up, lo = (float)lambda_min, hi = (float)lambda_max;
    if (!(dn > 0 && dn <= 1) || !(up >= 1) || !(lo > 0) || !(lo <= hi) || !(hi <= 3.0e38f)) return LFSD_EINVAL;
    lfsd::LmStepArgs<float> a{batch, n_param, (float)lambda_down, (float)lambda_up, (float)lambda_min, (float)lambda_max,
                              (float*)theta, (float*)loss_acc, (float*)grad_acc, (float*)H_acc, (float*)lambda, (float*)theta_trial,
                              (const float*)loss_t, (const float*)grad_t, (const float*)H_t, (const float*)proj_lo, row_active, accepted};
    return lfsd_detail::launch_lm_step_f32(a, stream);
  }
  if (dtype == LFSD_F64) {
    lfsd::LmStepArgs<double> a{batch, n_param, lambda_down, lambda_up, lambda_min, lambda_max,
                               (double*)theta, (double*)loss_acc, (double*)grad_acc, (double*)H_acc, (double*)lambda, (double*)theta_trial,
                               (const double*)loss_t, (const double*)grad_t, (const double*)H_t, (const double*)proj_lo, row_active, accepted};
    return lfsd_detail::launch_lm_step_f64(a, stream);
  }
  return LFSD_EINVAL;
}

// ---- ABI 15: several demonstrations per seed -- loss, gradient and J^T J summed per group in a fixed order (cpdp_groups.h) ----
LFSD_API int lfsd_group_reduce(int dtype, int n_groups, int group_size, int n_param, const void* loss, const void* grad,
                               const void* H, const int* row_ok, void* loss_g, void* grad_g, void* H_g, int* n_ok, void* stream) {
  if (n_groups <= 0 || group_size <= 0 || n_param <= 0) return LFSD_EINVAL;
  if (dtype != LFSD_F32 && dtype != LFSD_F64) return LFSD_EINVAL;
  if (!loss || !grad || !loss_g || !grad_g || !n_ok) return LFSD_EINVAL;
  if ((H == nullptr) != (H_g == nullptr)) return LFSD_EINVAL;
  // the sizes first: the byte counts of the overlap test below must not wrap (B p^2 * 8 < 2^64 needs more than p < 2^15.5 alone)
  if (n_param > 46340) return LFSD_EINVAL;
  {
    const unsigned long long per = 1ull + (unsigned long long)n_param + (H ? (unsigned long long)n_param * n_param : 0ull);
    if (((unsigned long long)n_groups * per + 255ull) / 256ull > 0x7fffffffull) return LFSD_EINVAL;      // (the launcher's workgroup limit)
    if ((unsigned long long)n_groups * (unsigned long long)group_size > (0xffffffffffffffffull / 8ull) / ((unsigned long long)n_param * n_param))
      return LFSD_EINVAL;
  }
  const unsigned long long es = dtype == LFSD_F32 ? 4 : 8, G = (unsigned long long)n_groups, P = (unsigned long long)n_param;
  const unsigned long long B = G * (unsigned long long)group_size;
  const void* in[4] = {loss, grad, H, row_ok};
  const unsigned long long in_bytes[4] = {B * es, B * P * es, B * P * P * es, B * sizeof(int)};
  const void* out[4] = {loss_g, grad_g, H_g, n_ok};
  const unsigned long long out_bytes[4] = {G * es, G * P * es, G * P * P * es, G * sizeof(int)};
  for (int o = 0; o < 4; ++o)
    for (int i = 0; i < 4; ++i)
      if (out[o] && spans_overlap(out[o], out_bytes[o], in[i], in_bytes[i])) return LFSD_EINVAL;
  if (dtype == LFSD_F32) {
    lfsd::GroupReduceArgs<float> a{n_groups, group_size, n_param, (const float*)loss, (const float*)grad, (const float*)H, row_ok,
                                   (float*)loss_g, (float*)grad_g, (float*)H_g, n_ok};
    return lfsd_detail::launch_group_reduce_f32(a, stream);
  }
  lfsd::GroupReduceArgs<double> a{n_groups, group_size, n_param, (const double*)loss, (const double*)grad, (const double*)H, row_ok,
                                  (double*)loss_g, (double*)grad_g, (double*)H_g, n_ok};
  return lfsd_detail::launch_group_reduce_f64(a, stream);
}

// ---- ABI 17: learnable waypoint times -- dLoss/dtau of the waypoint loss and the ordered update (cpdp_times.h) ----
template <typename T>
static int waypoint_time_grad_t(int batch, int n_grid, int n_waypoints, int n_iface, const void* state_grid, const void* curv,
                                const void* horizon, const void* consts, int const_per_traj, const void* taus, const void* waypoints,
                                const int* iface_idx, const void* wp_weight, const void* tau_ref, double tau_prior, void* dtau,
                                void* stream) {
  lfsd::TimeGradArgs<T> a;
  a.batch = batch; a.n_grid = n_grid; a.n_waypoints = n_waypoints; a.n_iface = n_iface;
  a.state_grid = (const T*)state_grid; a.curv = (const T*)curv; a.horizon = (const T*)horizon;
  a.consts = consts ? (const T*)consts : (const T*)horizon;      // (a model without constants: a readable word, as aux_phase_t does)
  a.const_stride = (consts && const_per_traj) ? Model::NC : 0;
  a.taus = (const T*)taus; a.waypoints = (const T*)waypoints; a.iface_idx = iface_idx;
  a.wp_weight = (const T*)wp_weight; a.tau_ref = (const T*)tau_ref; a.tau_prior = (T)tau_prior; a.dtau = (T*)dtau;
  if constexpr (sizeof(T) == 4) return lfsd_detail::launch_waypoint_time_grad_f32(a, stream);
  else return lfsd_detail::launch_waypoint_time_grad_f64(a, stream);
}

LFSD_API int lfsd_waypoint_time_grad(int dtype, int batch, int n_grid, int n_waypoints, int n_iface, const void* state_grid,
                                     const void* curv, const void* horizon, const void* consts, int const_per_traj,
                                     const void* taus, const void* waypoints, const int* iface_idx, const void* wp_weight,
                                     const void* tau_ref, double tau_prior, void* dtau, void* stream) {
  if (batch <= 0 || n_grid < 1 || n_waypoints <= 0 || n_iface <= 0) return LFSD_EINVAL;
  if (curv && n_grid < 3) return LFSD_EINVAL;
  if (dtype != LFSD_F32 && dtype != LFSD_F64) return LFSD_EINVAL;
  if (!state_grid || !horizon || !taus || !waypoints || !dtau) return LFSD_EINVAL;
  // iface_idx == NULL selects the interface function compiled into the library: it must exist, n_iface must be its size, and the
  // constants it may read must be there
  if (!iface_idx && (Model::NIF == 0 || n_iface != Model::NIF || (Model::NC_REAL > 0 && !consts))) return LFSD_EINVAL;
  if (!(tau_prior >= 0) || !(tau_prior <= 1.7e308)) return LFSD_EINVAL;      // (false for a NaN)
  if (dtype == LFSD_F32 && !(tau_prior <= 3.0e38)) return LFSD_EINVAL;      // (compared as a double: no cast of a value float cannot hold)
  if (((unsigned long long)batch * (unsigned long long)n_waypoints + 255ull) / 256ull > 0x7fffffffull) return LFSD_EINVAL;
  const unsigned long long es = dtype == LFSD_F32 ? 4 : 8, B = (unsigned long long)batch, K = (unsigned long long)n_waypoints;
  const unsigned long long ob = B * K * es, gb = B * (unsigned long long)(n_grid + 1) * Model::NX * es;
  if (spans_overlap(dtau, ob, state_grid, gb) || spans_overlap(dtau, ob, curv, gb) || spans_overlap(dtau, ob, horizon, B * es) ||
      spans_overlap(dtau, ob, taus, ob) || spans_overlap(dtau, ob, waypoints, ob * (unsigned long long)n_iface) ||
      spans_overlap(dtau, ob, iface_idx, (unsigned long long)n_iface * sizeof(int)) || spans_overlap(dtau, ob, wp_weight, ob) ||
      spans_overlap(dtau, ob, tau_ref, ob) ||
      spans_overlap(dtau, ob, consts, (const_per_traj ? B : 1ull) * (unsigned long long)Model::NC * es))
    return LFSD_EINVAL;
  if (dtype == LFSD_F32)
    return waypoint_time_grad_t<float>(batch, n_grid, n_waypoints, n_iface, state_grid, curv, horizon, consts, const_per_traj, taus,
                                       waypoints, iface_idx, wp_weight, tau_ref, tau_prior, dtau, stream);
  return waypoint_time_grad_t<double>(batch, n_grid, n_waypoints, n_iface, state_grid, curv, horizon, consts, const_per_traj, taus,
                                      waypoints, iface_idx, wp_weight, tau_ref, tau_prior, dtau, stream);
}

LFSD_API int lfsd_tau_project(int dtype, int batch, int n_waypoints, const void* tau_ref, void* tau_io, const void* horizon,
                              const void* wp_weight, const void* tau_lo, const void* tau_hi, double max_shift,
                              const int* row_active, void* stream) {
  if (batch <= 0 || n_waypoints <= 0) return LFSD_EINVAL;
  if (dtype != LFSD_F32 && dtype != LFSD_F64) return LFSD_EINVAL;
  if (!tau_ref || !tau_io || !horizon) return LFSD_EINVAL;
  if (!(max_shift > 0 && max_shift < 0.5)) return LFSD_EINVAL;      // (false for a NaN)
  if (dtype == LFSD_F32 && !((float)max_shift > 0 && (float)max_shift < 0.5f)) return LFSD_EINVAL;      // ... and after the cast
  const unsigned long long es = dtype == LFSD_F32 ? 4 : 8, B = (unsigned long long)batch, ob = B * (unsigned long long)n_waypoints * es;
  if (spans_overlap(tau_io, ob, tau_ref, ob) || spans_overlap(tau_io, ob, horizon, B * es) || spans_overlap(tau_io, ob, wp_weight, ob) ||
      spans_overlap(tau_io, ob, tau_lo, ob) || spans_overlap(tau_io, ob, tau_hi, ob) ||
      spans_overlap(tau_io, ob, row_active, B * sizeof(int)))
    return LFSD_EINVAL;
  if (dtype == LFSD_F32) {
    lfsd::TauProjectArgs<float> a{batch, n_waypoints, (const float*)tau_ref, (float*)tau_io, (const float*)horizon,
                                  (const float*)wp_weight, (const float*)tau_lo, (const float*)tau_hi, (float)max_shift, row_active};
    return lfsd_detail::launch_tau_project_f32(a, stream);
  }
  lfsd::TauProjectArgs<double> a{batch, n_waypoints, (const double*)tau_ref, (double*)tau_io, (const double*)horizon,
                                 (const double*)wp_weight, (const double*)tau_lo, (const double*)tau_hi, max_shift, row_active};
  return lfsd_detail::launch_tau_project_f64(a, stream);
}

// ---- ABI 18: Levenberg-Marquardt over parameters and waypoint times jointly (cpdp_lm_times.h; no counterpart in the reference) ----
LFSD_API int lfsd_time_normal_blocks(int dtype, int batch, int n_grid, int n_state, int n_param, int n_waypoints, int n_iface,
                                     const int* iface_idx, const void* horizon, const void* taus, const void* wp_weight,
                                     const void* state_grid, const void* curv, const void* auxX_grid, void* C, void* d,
                                     void* stream) {
  if (batch <= 0 || n_grid < 1 || n_state <= 0 || n_param <= 0 || n_waypoints <= 0 || n_iface <= 0) return LFSD_EINVAL;
  if (curv && n_grid < 3) return LFSD_EINVAL;
  if (dtype != LFSD_F32 && dtype != LFSD_F64) return LFSD_EINVAL;
  if (!iface_idx || !horizon || !taus || !state_grid || !auxX_grid || !C || !d) return LFSD_EINVAL;
  const unsigned long long es = dtype == LFSD_F32 ? 4 : 8, B = (unsigned long long)batch, P = (unsigned long long)n_param;
  const unsigned long long BK = B * (unsigned long long)n_waypoints;      // (below 2^62)
  // one thread per (row, waypoint, parameter): the launcher's workgroup limit, tested without forming a product that could wrap
  if (BK > (0x7fffffffull * 256ull) / P) return LFSD_EINVAL;
  const unsigned long long cb = BK * P * es, db = BK * es, gb = B * (unsigned long long)(n_grid + 1) * (unsigned long long)n_state * es;
  const void* in[7] = {iface_idx, horizon, taus, wp_weight, state_grid, curv, auxX_grid};
  const unsigned long long in_bytes[7] = {(unsigned long long)n_iface * sizeof(int), B * es, db, db, gb, gb, gb * P};
  for (int i = 0; i < 7; ++i)
    if (spans_overlap(C, cb, in[i], in_bytes[i]) || spans_overlap(d, db, in[i], in_bytes[i])) return LFSD_EINVAL;
  if (spans_overlap(C, cb, d, db)) return LFSD_EINVAL;
  if (dtype == LFSD_F32) {
    lfsd::TimeBlocksArgs<float> a{batch, n_grid, n_state, n_param, n_waypoints, n_iface, iface_idx, (const float*)horizon,
                                  (const float*)taus, (const float*)wp_weight, (const float*)state_grid, (const float*)curv,
                                  (const float*)auxX_grid, (float*)C, (float*)d};
    return lfsd_detail::launch_time_blocks_f32(a, stream);
  }
  lfsd::TimeBlocksArgs<double> a{batch, n_grid, n_state, n_param, n_waypoints, n_iface, iface_idx, (const double*)horizon,
                                 (const double*)taus, (const double*)wp_weight, (const double*)state_grid, (const double*)curv,
                                 (const double*)auxX_grid, (double*)C, (double*)d};
  return lfsd_detail::launch_time_blocks_f64(a, stream);
}

template <typename T>
static int lm_step_times_t(int n_groups, int group_size, int n_param, int n_waypoints, double lambda_down, double lambda_up,
                           double lambda_min, double lambda_max, void* theta, void* loss_acc, void* grad_acc, void* H_acc, void* lambda,
                           void* theta_trial, void* tau, void* tau_trial, void* gtau_acc, void* C_acc, void* d_acc, int* ok_acc,
                           const void* loss_t, const void* grad_t, const void* H_t, const void* gtau_t, const void* C_t,
                           const void* d_t, const int* row_ok, const void* wp_weight, const void* proj_lo, const int* group_active,
                           int* accepted, void* stream) {
  lfsd::LmStepTimesArgs<T> a;
  a.n_groups = n_groups; a.group_size = group_size; a.n_param = n_param; a.n_waypoints = n_waypoints;
  a.lambda_down = (T)lambda_down; a.lambda_up = (T)lambda_up; a.lambda_min = (T)lambda_min; a.lambda_max = (T)lambda_max;
  a.theta = (T*)theta; a.loss_acc = (T*)loss_acc; a.grad_acc = (T*)grad_acc; a.H_acc = (T*)H_acc; a.lambda = (T*)lambda;
  a.theta_trial = (T*)theta_trial; a.tau = (T*)tau; a.tau_trial = (T*)tau_trial; a.gtau_acc = (T*)gtau_acc; a.C_acc = (T*)C_acc;
  a.d_acc = (T*)d_acc; a.ok_acc = ok_acc; a.loss_t = (const T*)loss_t; a.grad_t = (const T*)grad_t; a.H_t = (const T*)H_t;
  a.gtau_t = (const T*)gtau_t; a.C_t = (const T*)C_t; a.d_t = (const T*)d_t; a.row_ok = row_ok; a.wp_weight = (const T*)wp_weight;
  a.proj_lo = (const T*)proj_lo; a.group_active = group_active; a.accepted = accepted;
  if constexpr (sizeof(T) == 4) return lfsd_detail::launch_lm_step_times_f32(a, stream);
  else return lfsd_detail::launch_lm_step_times_f64(a, stream);
}

LFSD_API int lfsd_lm_step_times(int dtype, int n_groups, int group_size, int n_param, int n_waypoints, double lambda_down,
                                double lambda_up, double lambda_min, double lambda_max, void* theta, void* loss_acc, void* grad_acc,
                                void* H_acc, void* lambda, void* theta_trial, void* tau, void* tau_trial, void* gtau_acc, void* C_acc,
                                void* d_acc, int* ok_acc, const void* loss_t, const void* grad_t, const void* H_t, const void* gtau_t,
                                const void* C_t, const void* d_t, const int* row_ok, const void* wp_weight, const void* proj_lo,
                                const int* group_active, int* accepted, void* stream) {
  if (n_groups <= 0 || group_size <= 0 || n_waypoints <= 0 || n_param <= 0 || n_param > lfsd::LM_MAX_PARAM) return LFSD_EINVAL;
  if (!theta || !loss_acc || !grad_acc || !H_acc || !lambda || !theta_trial || !loss_t || !grad_t || !H_t) return LFSD_EINVAL;
  if (!tau || !tau_trial || !gtau_acc || !C_acc || !d_acc || !ok_acc || !gtau_t || !C_t || !d_t) return LFSD_EINVAL;
  // (every comparison is false for a NaN: written so that a NaN scalar fails one of them)
  if (!(lambda_down > 0 && lambda_down <= 1) || !(lambda_up >= 1) || !(lambda_min > 0) || !(lambda_min <= lambda_max)) return LFSD_EINVAL;
  if (dtype == LFSD_F32) {
    // the same conditions on the values the kernel gets, as lfsd_lm_step
    const float dn = (float)lambda_down, up = (float)lambda_up, lo = (float)lambda_min, hi = (float)lambda_max;
    if (!(dn > 0 && dn <= 1) || !(up >= 1) || !(lo > 0) || !(lo <= hi) || !(hi <= 3.0e38f)) return LFSD_EINVAL;
    return lm_step_times_t<float>(n_groups, group_size, n_param, n_waypoints, lambda_down, lambda_up, lambda_min, lambda_max, theta,
                                  loss_acc, grad_acc, H_acc, lambda, theta_trial, tau, tau_trial, gtau_acc, C_acc, d_acc, ok_acc, loss_t,
                                  grad_t, H_t, gtau_t, C_t, d_t, row_ok, wp_weight, proj_lo, group_active, accepted, stream);
  }
  if (dtype == LFSD_F64)
    return lm_step_times_t<double>(n_groups, group_size, n_param, n_waypoints, lambda_down, lambda_up, lambda_min, lambda_max, theta,
                                   loss_acc, grad_acc, H_acc, lambda, theta_trial, tau, tau_trial, gtau_acc, C_acc, d_acc, ok_acc, loss_t,
                                   grad_t, H_t, gtau_t, C_t, d_t, row_ok, wp_weight, proj_lo, group_active, accepted, stream);
  return LFSD_EINVAL;
}
