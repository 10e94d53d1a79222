// Launchers of interpolation level 2 (ABI 11): the two auxiliary sweeps along the cubic interpolant and the curvature fit.  They live
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
}
