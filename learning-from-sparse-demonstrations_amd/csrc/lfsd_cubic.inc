// Launchers of interpolation level 2 (ABI 11) -- the two auxiliary sweeps along the cubic interpolant and the curvature fit -- and of
// the sampling kernels (ABI 12: cpdp_sample.h), the per-row rules (ABI 13: cpdp_opt.h) and the Levenberg-Marquardt kernels (ABI 14:
// cpdp_lm.h), the per-group reduction (ABI 15: cpdp_groups.h), the weighted forward sweeps (ABI 16) and the kernels of the learnable waypoint
// times (ABI 17: cpdp_times.h) and of the joint Levenberg-Marquardt step (ABI 18: cpdp_lm_times.h).  They live
// in a translation unit of their own (lfsd_cubic.cpp): the device code of the two older units is then what it was before level 2
// existed, kernel for kernel (DESIGN.md section 11).  Single-unit builds include this file from lfsd_capi.cpp.
namespace lfsd_detail {
int launch_riccati_cubic_f32(unsigned grid, void* stream, const lfsd::AuxArgsCubic<float>& a) {
  LFSD_LAUNCH((lfsd::aux_riccati_cubic_kernel<Model, float, G>), grid, 64, stream, a);
  return launch_status();
}
int launch_riccati_cubic_f64(unsigned grid, void* stream, const lfsd::AuxArgsCubic<double>& a) {
  LFSD_LAUNCH((lfsd::aux_riccati_cubic_kernel<Model, double, G>), grid, 64, stream, a);
  return launch_status();
}
// (the forward sweep packs more trajectories into a wavefront than the Riccati sweep: lfsd::fwd_lanes, as in lfsd_capi.cpp)
static constexpr int GF_CUBIC = lfsd::fwd_lanes<Model>() < G ? lfsd::fwd_lanes<Model>() : G;
int launch_forward_cubic_f32(unsigned grid, void* stream, const lfsd::AuxArgsCubic<float>& a) {
  LFSD_LAUNCH((lfsd::aux_forward_cubic_kernel<Model, float, GF_CUBIC>), grid, 64, stream, a);
  return launch_status();
}
int launch_forward_cubic_f64(unsigned grid, void* stream, const lfsd::AuxArgsCubic<double>& a) {
  LFSD_LAUNCH((lfsd::aux_forward_cubic_kernel<Model, double, GF_CUBIC>), grid, 64, stream, a);
  return launch_status();
}
// ---- ABI 16: the forward sweeps with a weight per waypoint, both levels (kernels of their own: cpdp_aux.h) ----
template <typename T> static int launch_forward_weighted(unsigned grid, void* stream, const lfsd::AuxArgsCubic<T>& a, bool cubic, const T* wp_weight) {
  if (cubic) {
    lfsd::AuxArgsCubicWeighted<T> w;
    static_cast<lfsd::AuxArgsCubic<T>&>(w) = a;
    w.wp_weight = wp_weight;
    LFSD_LAUNCH((lfsd::aux_forward_cubic_weighted_kernel<Model, T, GF_CUBIC>), grid, 64, stream, w);
  } else {
    lfsd::AuxArgsWeighted<T> w;
    static_cast<lfsd::AuxArgs<T>&>(w) = a;
    w.wp_weight = wp_weight;
    LFSD_LAUNCH((lfsd::aux_forward_weighted_kernel<Model, T, GF_CUBIC>), grid, 64, stream, w);
  }
  return launch_status();
}
int launch_forward_weighted_f32(unsigned grid, void* stream, const lfsd::AuxArgsCubic<float>& a, bool cubic, const float* wp_weight) {
  return launch_forward_weighted<float>(grid, stream, a, cubic, wp_weight);
}
int launch_forward_weighted_f64(unsigned grid, void* stream, const lfsd::AuxArgsCubic<double>& a, bool cubic, const double* wp_weight) {
  return launch_forward_weighted<double>(grid, stream, a, cubic, wp_weight);
}
// The emulator runs every lane as a fiber with a stack of its own: its launches stay small.
#if defined(LFSD_EMU)
static constexpr int kSplineBlock = 64;
#else
static constexpr int kSplineBlock = 256;
#endif
template <typename T> static int launch_grid_curvature(int batch, int n_grid, int n_comp, const T* grid, T* curv, void* stream) {
  const long long threads = (long long)batch * n_comp;
  const long long blocks = (threads + kSplineBlock - 1) / kSplineBlock;
  if (blocks > 0x7fffffffLL) return LFSD_EINVAL;
  lfsd::SplineArgs<T> a{batch, n_grid, n_comp, grid, curv};
  LFSD_LAUNCH((lfsd::grid_curvature_kernel<T>), (unsigned)blocks, kSplineBlock, stream, a);
  return launch_status();
}
int launch_grid_curvature_f32(int batch, int n_grid, int n_comp, const float* grid, float* curv, void* stream) {
  return launch_grid_curvature<float>(batch, n_grid, n_comp, grid, curv, stream);
}
int launch_grid_curvature_f64(int batch, int n_grid, int n_comp, const double* grid, double* curv, void* stream) {
  return launch_grid_curvature<double>(batch, n_grid, n_comp, grid, curv, stream);
}
// ---- ABI 12: opt_sol(t) / auxsys_sol(t) for a batch, and the chain rule of a user-written loss (cpdp_sample.h) ----
template <typename T> static int launch_grid_sample(const lfsd::SampleArgs<T>& a, void* stream) {
  const long long rows = (long long)a.batch * a.n_times;      // (below 2^62; the product with n_comp must not wrap either)
  if (rows > (0x7fffffffLL * kSplineBlock) / a.n_comp) return LFSD_EINVAL;
  const long long blocks = (rows * a.n_comp + kSplineBlock - 1) / kSplineBlock;
  if (blocks > 0x7fffffffLL) return LFSD_EINVAL;
  LFSD_LAUNCH((lfsd::grid_sample_kernel<T>), (unsigned)blocks, kSplineBlock, stream, a);
  return launch_status();
}
int launch_grid_sample_f32(const lfsd::SampleArgs<float>& a, void* stream) { return launch_grid_sample<float>(a, stream); }
int launch_grid_sample_f64(const lfsd::SampleArgs<double>& a, void* stream) { return launch_grid_sample<double>(a, stream); }
template <typename T> static int launch_waypoint_vjp(const lfsd::WaypointVjpArgs<T>& a, void* stream) {
  const long long threads = (long long)a.batch * a.n_param;
  const long long blocks = (threads + kSplineBlock - 1) / kSplineBlock;
  if (blocks > 0x7fffffffLL) return LFSD_EINVAL;
  LFSD_LAUNCH((lfsd::waypoint_vjp_kernel<T>), (unsigned)blocks, kSplineBlock, stream, a);
  return launch_status();
}
int launch_waypoint_vjp_f32(const lfsd::WaypointVjpArgs<float>& a, void* stream) { return launch_waypoint_vjp<float>(a, stream); }
int launch_waypoint_vjp_f64(const lfsd::WaypointVjpArgs<double>& a, void* stream) { return launch_waypoint_vjp<double>(a, stream); }
// ---- ABI 13: per-row update rules, the evaluation point of a mixed batch, device traces (cpdp_opt.h) ----
// one thread per (row, parameter); batch and n_param are positive ints, so the thread count stays below 2^62
static bool rows_grid(int batch, int n_param, unsigned* grid) {
  const long long blocks = ((long long)batch * n_param + kSplineBlock - 1) / kSplineBlock;
  if (blocks > 0x7fffffffLL) return false;
  *grid = (unsigned)blocks;
  return true;
}
template <typename T> static int launch_optimizer_rows(const lfsd::OptRowsArgs<T>& a, void* stream) {
  unsigned grid;
  if (!rows_grid(a.batch, a.n_param, &grid)) return LFSD_EINVAL;
  LFSD_LAUNCH((lfsd::optimizer_rows_kernel<T>), grid, kSplineBlock, stream, a);
  return launch_status();
}
int launch_optimizer_rows_f32(const lfsd::OptRowsArgs<float>& a, void* stream) { return launch_optimizer_rows<float>(a, stream); }
int launch_optimizer_rows_f64(const lfsd::OptRowsArgs<double>& a, void* stream) { return launch_optimizer_rows<double>(a, stream); }
template <typename T> static int launch_lookahead_rows(const lfsd::LookaheadRowsArgs<T>& a, void* stream) {
  unsigned grid;
  if (!rows_grid(a.batch, a.n_param, &grid)) return LFSD_EINVAL;
  LFSD_LAUNCH((lfsd::lookahead_rows_kernel<T>), grid, kSplineBlock, stream, a);
  return launch_status();
}
int launch_lookahead_rows_f32(const lfsd::LookaheadRowsArgs<float>& a, void* stream) { return launch_lookahead_rows<float>(a, stream); }
int launch_lookahead_rows_f64(const lfsd::LookaheadRowsArgs<double>& a, void* stream) { return launch_lookahead_rows<double>(a, stream); }
template <typename T> static int launch_trace_append(const lfsd::TraceArgs<T>& a, void* stream) {
  unsigned grid;
  if (!rows_grid(a.batch, a.n_param, &grid)) return LFSD_EINVAL;
  LFSD_LAUNCH((lfsd::trace_append_kernel<T>), grid, kSplineBlock, stream, a);
  return launch_status();
}
int launch_trace_append_f32(const lfsd::TraceArgs<float>& a, void* stream) { return launch_trace_append<float>(a, stream); }
int launch_trace_append_f64(const lfsd::TraceArgs<double>& a, void* stream) { return launch_trace_append<double>(a, stream); }
// ---- ABI 14: Gauss-Newton matrix of the waypoint loss, Levenberg-Marquardt step (cpdp_lm.h) ----
// one thread per (row, q1, q2): batch and n_param are positive ints, n_param^2 * batch stays below 2^62 in 64 bits only while
// n_param < 2^15.5 -- larger ones are refused with the workgroup count
template <typename T> static int launch_normal_matrix(const lfsd::NormalMatrixArgs<T>& a, void* stream) {
  if (a.n_param > 46340) return LFSD_EINVAL;
  const long long threads = (long long)a.batch * a.n_param * a.n_param;
  const long long blocks = (threads + kSplineBlock - 1) / kSplineBlock;
  if (blocks > 0x7fffffffLL) return LFSD_EINVAL;
  LFSD_LAUNCH((lfsd::normal_matrix_kernel<T>), (unsigned)blocks, kSplineBlock, stream, a);
  return launch_status();
}
int launch_normal_matrix_f32(const lfsd::NormalMatrixArgs<float>& a, void* stream) { return launch_normal_matrix<float>(a, stream); }
int launch_normal_matrix_f64(const lfsd::NormalMatrixArgs<double>& a, void* stream) { return launch_normal_matrix<double>(a, stream); }
// one row per lane, one wavefront per workgroup (batch is a positive int: at most 2^25 workgroups)
template <typename T> static int launch_lm_step(const lfsd::LmStepArgs<T>& a, void* stream) {
  const unsigned grid = (unsigned)(((long long)a.batch + lfsd::LM_BLOCK - 1) / lfsd::LM_BLOCK);
  LFSD_LAUNCH((lfsd::lm_step_kernel<T>), grid, lfsd::LM_BLOCK, stream, a);
  return launch_status();
}
int launch_lm_step_f32(const lfsd::LmStepArgs<float>& a, void* stream) { return launch_lm_step<float>(a, stream); }
int launch_lm_step_f64(const lfsd::LmStepArgs<double>& a, void* stream) { return launch_lm_step<double>(a, stream); }
// ---- ABI 15: loss, gradient and Gauss-Newton matrix of several demonstrations summed per seed (cpdp_groups.h) ----
// one thread per (group, element), 1 + p + p^2 elements per group: n_groups and n_param are positive ints, the product stays below
// 2^62 while n_param < 2^15.5 -- larger ones are refused with the workgroup count
template <typename T> static int launch_group_reduce(const lfsd::GroupReduceArgs<T>& a, void* stream) {
  if (a.n_param > 46340) return LFSD_EINVAL;
  const long long per = 1 + (long long)a.n_param + (a.H ? (long long)a.n_param * a.n_param : 0);
  const long long threads = (long long)a.n_groups * per;
  const long long blocks = (threads + kSplineBlock - 1) / kSplineBlock;
  if (blocks > 0x7fffffffLL) return LFSD_EINVAL;
  LFSD_LAUNCH((lfsd::group_reduce_kernel<T>), (unsigned)blocks, kSplineBlock, stream, a);
  return launch_status();
}
int launch_group_reduce_f32(const lfsd::GroupReduceArgs<float>& a, void* stream) { return launch_group_reduce<float>(a, stream); }
int launch_group_reduce_f64(const lfsd::GroupReduceArgs<double>& a, void* stream) { return launch_group_reduce<double>(a, stream); }
// ---- ABI 17: learnable waypoint times -- dLoss/dtau of the waypoint loss, the ordered update (cpdp_times.h) ----
// one thread per (trajectory, waypoint); batch and n_waypoints are positive ints, so the thread count stays below 2^62
template <typename T> static int launch_waypoint_time_grad(const lfsd::TimeGradArgs<T>& a, void* stream) {
  unsigned grid;
  if (!rows_grid(a.batch, a.n_waypoints, &grid)) return LFSD_EINVAL;
  LFSD_LAUNCH((lfsd::waypoint_time_grad_kernel<Model, T>), grid, kSplineBlock, stream, a);
  return launch_status();
}
int launch_waypoint_time_grad_f32(const lfsd::TimeGradArgs<float>& a, void* stream) { return launch_waypoint_time_grad<float>(a, stream); }
int launch_waypoint_time_grad_f64(const lfsd::TimeGradArgs<double>& a, void* stream) { return launch_waypoint_time_grad<double>(a, stream); }
// one thread per row
template <typename T> static int launch_tau_project(const lfsd::TauProjectArgs<T>& a, void* stream) {
  unsigned grid;
  if (!rows_grid(a.batch, 1, &grid)) return LFSD_EINVAL;
  LFSD_LAUNCH((lfsd::tau_project_kernel<T>), grid, kSplineBlock, stream, a);
  return launch_status();
}
int launch_tau_project_f32(const lfsd::TauProjectArgs<float>& a, void* stream) { return launch_tau_project<float>(a, stream); }
int launch_tau_project_f64(const lfsd::TauProjectArgs<double>& a, void* stream) { return launch_tau_project<double>(a, stream); }
// ---- ABI 18: Levenberg-Marquardt over parameters and waypoint times jointly (cpdp_lm_times.h) ----
// one thread per (trajectory, waypoint, parameter); the entry point has bounded the product (it stays below 2^39)
template <typename T> static int launch_time_blocks(const lfsd::TimeBlocksArgs<T>& a, void* stream) {
  const long long threads = (long long)a.batch * a.n_waypoints * a.n_param;
  const long long blocks = (threads + kSplineBlock - 1) / kSplineBlock;
  if (blocks > 0x7fffffffLL) return LFSD_EINVAL;
  LFSD_LAUNCH((lfsd::time_blocks_kernel<T>), (unsigned)blocks, kSplineBlock, stream, a);
  return launch_status();
}
int launch_time_blocks_f32(const lfsd::TimeBlocksArgs<float>& a, void* stream) { return launch_time_blocks<float>(a, stream); }
int launch_time_blocks_f64(const lfsd::TimeBlocksArgs<double>& a, void* stream) { return launch_time_blocks<double>(a, stream); }
// one group per lane, one wavefront per workgroup (n_groups is a positive int: at most 2^25 workgroups)
template <typename T> static int launch_lm_step_times(const lfsd::LmStepTimesArgs<T>& a, void* stream) {
  const unsigned grid = (unsigned)(((long long)a.n_groups + lfsd::LM_BLOCK - 1) / lfsd::LM_BLOCK);
  LFSD_LAUNCH((lfsd::lm_step_times_kernel<T>), grid, lfsd::LM_BLOCK, stream, a);
  return launch_status();
}
int launch_lm_step_times_f32(const lfsd::LmStepTimesArgs<float>& a, void* stream) { return launch_lm_step_times<float>(a, stream); }
int launch_lm_step_times_f64(const lfsd::LmStepTimesArgs<double>& a, void* stream) { return launch_lm_step_times<double>(a, stream); }
}
