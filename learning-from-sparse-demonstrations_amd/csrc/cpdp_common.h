// Platform macros, build switches, tuning constants, packed/MFMA primitives and the small dense helpers shared by every kernel.
// Part of the kernel sources collected by cpdp_kernels.h (include that header, not this one).
#pragma once


#include <type_traits>
#include <utility>
#if defined(LFSD_EMU)
#include "simt_emu.h"
#define LFSD_LAMBDA_INLINE
#define LFSD_HD
#else
#include <hip/hip_runtime.h>
#define LFSD_DEV __device__ __forceinline__
#define LFSD_HD __host__ __device__
// lambdas inside kernels must be inlined as well: a real call passes their by-reference captures through scratch
#define LFSD_LAMBDA_INLINE __attribute__((always_inline))
#endif

// ---- build switches ----------------------------------------------------------------------------------------------------------
// The schedules of the OC solve that the GPU tier and the emulator tests compare with a plain solve (lfsd_amd.runtime.
// GPU_TIER_VARIANTS, tests/test_emu_kernels.py): each is set on the command line of a variant build.  Every other tuning choice
// is a constant below.
// Mesh continuation of the lean OC kernels (cpdp_oc.h, oc_solve_kernel): one RK4 step per grid interval while full steps gain
// more than kCoarseSwitch of the cost, then the reference's steps_per_grid; 0 switches it off.  Measured on the benchmark
// (profiles/r03_d_ab_coarse_exit.txt, r03_e_ab_coarse_switch.txt), oc_solve per launch: off 3.79 ms; switch at 3.0 (after the
// first step) 3.20; 0.3 (with the Gauss-Newton -> Hamiltonian hand-over) 2.93; 1e-2 2.94; 1e-3 (one Newton-like step more on
// the coarse grid) 2.85; 1e-4 2.98; 0 (only when the coarse problem has converged) 3.66.
#ifndef LFSD_COARSE_START
#define LFSD_COARSE_START 1
#endif
// lean matrix-core kernels: level 0 of the mesh continuation merges LFSD_LEAN_TC control intervals (1: off) with kLeanTcS RK4
// steps per merged interval for the first kLeanTcIters iterations of a cold start; never below kLeanTcMin intervals.
// Measured on BOTH workloads of the benchmark (oc_solve per launch, 20 steps; profiles/r04_z_ab_lean_time_coarsening.txt) --
// independent seeds (one start / goal, 4 096 parameter vectors: a homogeneous batch whose trajectories all walk the same path) |
// shared parameters (4 096 random starts / goals / waypoints, the N > 1 workload: the launch lasts as long as its slowest path):
//   off 2.57 | 2.70;   2 x 1 step for 2 / 3 / 4 iterations 2.34 / 2.40 / 2.62 | 2.48 / 2.40 / 2.96;
//   5 x 2 for 2 / 3 iterations 2.45 / 2.16 | 2.43 / 2.90;   5 x 1 for 2 / 3 iterations 2.46 / 2.10 | 2.40 / 2.85.
// 5 merged intervals for 3 iterations is the best on the homogeneous batch and WORSE than no level 0 on the diverse one; shipped is
// the setting that gains on both, 2 x 1 x 3.
#ifndef LFSD_LEAN_TC
#define LFSD_LEAN_TC 2
#endif
// wide kernel (one trajectory per wavefront): the interval-parallel (multiple-shooting) iteration of OcWide::ms_* (cpdp_oc.h) --
// the reference's own lifted formulation, CPDP.py:136-172 -- for unbounded problems with at least kMsMinGrid intervals; 0: single
// shooting only.  The phase hands over to the single-shooting iteration through a closed-loop roll-out, so every convergence test
// is unchanged.
#ifndef LFSD_MS
#define LFSD_MS 1
#endif
// wide kernel: control intervals merged in the coarse phase (1: none, the coarse phase only takes one RK4 step per interval)
#ifndef LFSD_COARSE_TIME
#define LFSD_COARSE_TIME 4
#endif
// wide kernel, small fp32 models (at most 8 columns, NX * NXU <= 32): the backward sweep on LDS-staged operands, every lane running
// the whole recursion (OcWide::backward_small, 1), or the generic sweep (0)
#ifndef LFSD_BW_SMALL
#define LFSD_BW_SMALL 1
#endif
// fp32 Riccati sweep of the 32-lane models (cpdp_aux.h, aux_node_slots): the coefficient nodes of two consecutive split units are
// staged in one pass on nine lanes (1), or every unit stages its own five (0).  The results are bit for bit the same.
#ifndef LFSD_RIC_PAIR_STAGE
#define LFSD_RIC_PAIR_STAGE 1
#endif
// lean fp32 OC kernel of the 32-lane models (cpdp_oc.h, OcSolver::backward_sc / costate_sweep_sc): the per-stage hand-overs inside a
// trajectory's 16-lane group -- Q_uu and Q_u, the gains, Q_ux, V_x and the costate -- are row broadcasts in registers (row_bcast
// below, 1), or go through LDS (0).  Data movement only: the results are bit for bit the same.
#ifndef LFSD_OC_DPP_XCHG
#define LFSD_OC_DPP_XCHG 1
#endif

// ---- scheduling fences and LDS hand-overs -------------------------------------------------------------------------------------
// LFSD_ROW_FENCE / LFSD_SCHED_FENCE64(T): the instruction scheduler moves nothing across this point (bounds the live ranges of
// the fully unrolled contractions); LFSD_SCHED_FENCE64 only in fp64 instantiations, one per row of the backward sweep's dense
// products (see pin64 below).  No-ops in the emulator build.
#if defined(LFSD_EMU)
#define LFSD_ROW_FENCE()
#define LFSD_SCHED_FENCE64(T)
#else
#define LFSD_ROW_FENCE() __builtin_amdgcn_sched_barrier(0)
#define LFSD_SCHED_FENCE64(T) do { if constexpr (sizeof(T) == 8) __builtin_amdgcn_sched_barrier(0); } while (0)
#endif

// LFSD_WAVE_SYNC: LDS hand-over between lanes of ONE wavefront (kernels whose workgroup is a single wavefront: the
// auxiliary sweeps).  Release/acquire fences restricted to the LDS address space (s_waitcnt lgkmcnt(0); global loads in
// flight are not drained) around a wave_barrier, which emits nothing and only keeps the compiler from moving LDS accesses
// across it.  Unlike __syncthreads() it is well defined under control flow that differs between the lanes of the wavefront.
// The CPU emulator runs every lane as a fiber and needs a real rendez-vous there.
#if defined(LFSD_EMU)
#define LFSD_WAVE_SYNC() __syncthreads()
#else
#define LFSD_WAVE_SYNC()                                            \
  do {                                                              \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local"); \
    __builtin_amdgcn_wave_barrier();                                \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local"); \
  } while (0)
#endif

// LFSD_STAGE_SYNC: the hand-overs INSIDE a stage of the lean kernels' backward sweep (one wavefront per workgroup; every one of
// them goes through LDS).  __syncthreads() is a workgroup fence over ALL address spaces: on this hardware it compiles to
// `s_waitcnt vmcnt(0) lgkmcnt(0)` (the s_barrier of a one-wave workgroup is elided), so the sync that follows the stage's
// global stores of the gains parks the wavefront until those stores are acknowledged by the L2 -- once per stage, ~1 600 of a
// stage's 7 200 cycles by the phase clocks (profiles/r03_g_ab_prefetch_pin.txt, "K+Vupdate"), and it drains whatever was
// prefetched for the next stage with it.  The gains are read by the NEXT roll-out, behind the block-wide votes of the main
// loop (real __syncthreads); nothing inside the sweep reads them back.  So an LDS-scoped fence is used there instead, and the
// stage's loads are waited for at its top (cpdp_oc.h, backward_sc).  MEASURED (profiles/r04_j_ab_stage_sync.txt): the
// `s_waitcnt vmcnt(0)` behind the stores is gone from the stage's ISA and oc_solve takes exactly as long -- 2.587 ms against
// 2.589 with the old syncs, 2.629 with the next stage's loads prefetched on top: the stores are long acknowledged when the wait
// is reached; the sweep is bound by issue, as round 3 concluded.  Kept: it is the narrower fence.
#if defined(LFSD_EMU)
#define LFSD_STAGE_SYNC() __syncthreads()
#else
#define LFSD_STAGE_SYNC() LFSD_WAVE_SYNC()
#endif
// ... the same inside a stage of the GENERIC backward sweep (wide kernel, lock-step kernels without MFMA): there the next
// stage's global loads ARE issued a stage ahead (fp32), and every __syncthreads() of the stage drained them.
// Measured (profiles/r04_k_ab_generic_stage_sync.txt): rocket 107.8 / 107.5 ms, robot arm 17.8 / 17.7 ms with / without: nothing.
#if defined(LFSD_EMU)
#define LFSD_STAGE_SYNC_GEN() __syncthreads()
#else
#define LFSD_STAGE_SYNC_GEN() LFSD_WAVE_SYNC()
#endif

namespace lfsd {

// ---- tuning constants (measured on MI355X; the alternatives are in the history) ---------------------------------------------
// Levenberg shift ladder of the OC solve: sqrt(10) rungs up after a failed backward sweep / line search, down after an accepted
// full step; x10 / x0.1 over-damps the accepted steps (profiles/r01_tune_step_control.txt)
constexpr double kMuUp = 3.1623;
constexpr double kMuDown = 0.31623;
// accepted full steps to hold before the shift returns to a level that has just failed (slowest robot-arm seed 87 -> 65 iterations)
constexpr int kMuHold = 1;
// generic backward sweep of a Newton-from-start solve (exact_after == 0, the rocket): fraction of the shift a stage keeps when its
// Q_uu factorises with it; rocket learner step 207 -> 150 ms (profiles/r04_s_rocket_time_coarsening_stage_shift_ab.txt)
constexpr double kMuStageFracNewton = 0.001;
// Gauss-Newton -> Hamiltonian stage-Hessian model after the first accepted full step that gains less than this fraction of the
// new cost: 0.9 changes nothing, 3.0 (right after the first step) costs 2 % of the trajectories a 7th iteration
constexpr double kHamSwitch = 0.3;

// mesh continuation (LFSD_COARSE_START): the coarse phase ends after a full step that gains less than this fraction of the cost
// (profiles/r03_e_ab_coarse_switch.txt)
constexpr double kCoarseSwitch = 1e-3;
// lean kernels, level 0 (LFSD_LEAN_TC): RK4 steps per merged interval, cold-start iterations on it, fewest merged intervals
// (n_grid 20 -> 10 merged intervals cost 14 % instead of saving: profiles/r05_held_out_schedule_ab.jsonl)
constexpr int kLeanTcS = 1;
constexpr int kLeanTcIters = 3;
constexpr int kLeanTcMin = 12;
// lean kernels: accepted steps after the transfer from level 0 during which a refused or shortened full step is answered by a line
// search on the one-step-per-interval level instead of by leaving for the reference's grid (profiles/r04_bc_ab_grace_after_transfer.txt)
constexpr int kLeanTcGrace = 2;
// wide kernel: smallest n_grid with a coarse phase, and with a multiple-shooting phase (LFSD_MS)
constexpr int kCoarseMinGrid = 40;
constexpr int kMsMinGrid = 40;
// wide kernel, coarse phase with merged intervals (LFSD_COARSE_TIME): RK4 steps per merged interval (at most one per merged
// interval; profiles/r04_af_rocket_coarse_rk4_steps_ab.txt) and the smallest coarse grid it may produce
constexpr int kCoarseTimeS = 2;
constexpr int kCoarseTimeMin = 20;
// wide kernel: a step that gains less than kCoarseSwitch ends the coarse phase only when it was taken at a shift below this
// (profiles/r04_u_rocket_coarse_exit_rule_ab.txt)
constexpr double kCoarseExitMu = 1e-2;
// wide kernel's costate sweep: stages of look-ahead of its column loads
constexpr int kCsAhead = 3;
// lfsd_coc_solve, automatic mapping: largest batch that runs the wide kernel where the lean MFMA kernel does not apply (below ~1500
// trajectories most SIMDs would have no wavefront of the lock-step kernels: lfsd_capi.cpp, use_wide)
constexpr int kWideMaxBatch = 1536;

// Auxiliary sweeps: the non-stiff part of a split unit is the explicit midpoint rule in fp32 (the sweeps' rounding floor hides
// the two orders RK4 gains: Riccati 2.12 -> 1.47 ms) and classical RK4 in fp64 (profiles/r02_m_substeps_accuracy.txt)
constexpr int kAuxRk32 = 2;
constexpr int kAuxRk64 = 4;
// the next interval starts with HALF the units of this one when this one's worst per-unit estimate is at most 1/kAuxDown of its
// tolerance: the O(h^3) estimate grows 7.4-8x when the units are halved (profiles/r02_h_aux_units.txt)
constexpr int kAuxDown = 8;
// Riccati sweep: intervals that need at least this many uniform units are integrated with step-size control inside the interval
// (cpdp_aux.h, aux_riccati_kernel)
constexpr int kRicAdapt = 16;

// debug aid for the emulator build: start every kernel with NaN-filled LDS so that a read of
// never-written shared memory cannot go unnoticed (tests build with -DLFSD_POISON_LDS)
template <typename T> LFSD_DEV void poison_lds(T* p, int n) {
#if defined(LFSD_POISON_LDS)
  for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = T(0) / T(0);
  __syncthreads();
#else
  (void)p; (void)n;
#endif
}

enum Status { ST_RUNNING = 0, ST_CONVERGED = 1, ST_STALLED = 2, ST_MAXITER = 3, ST_FAILED = 4 };
enum OptMethod { OPT_VANILLA = 0, OPT_NESTEROV = 1, OPT_ADAM = 2, OPT_NADAM = 3, OPT_AMSGRAD = 4 };

// Two values per lane, for the kernels that carry two tangent columns on one lane: native 2-vectors on the GPU (the
// tangent code is linear, so it compiles to v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 at the scalar issue rate), a plain
// struct in the CPU emulator build.
#if defined(LFSD_EMU)
template <typename T> struct pk2 {
  T x, y;
  pk2() = default;
  pk2(T s) : x(s), y(s) {}
  pk2(T a, T b) : x(a), y(b) {}
};
template <typename T> inline pk2<T> operator+(pk2<T> a, pk2<T> b) { return pk2<T>(a.x + b.x, a.y + b.y); }
template <typename T> inline pk2<T> operator-(pk2<T> a, pk2<T> b) { return pk2<T>(a.x - b.x, a.y - b.y); }
template <typename T> inline pk2<T> operator-(pk2<T> a) { return pk2<T>(-a.x, -a.y); }
template <typename T> inline pk2<T> operator*(pk2<T> a, pk2<T> b) { return pk2<T>(a.x * b.x, a.y * b.y); }
template <typename T> inline pk2<T> operator*(T a, pk2<T> b) { return pk2<T>(a * b.x, a * b.y); }
template <typename T> inline pk2<T> operator*(pk2<T> a, T b) { return pk2<T>(a.x * b, a.y * b); }
template <typename T> inline pk2<T> operator+(T a, pk2<T> b) { return pk2<T>(a + b.x, a + b.y); }
template <typename T> inline pk2<T> operator+(pk2<T> a, T b) { return pk2<T>(a.x + b, a.y + b); }
template <typename T> inline pk2<T> operator/(pk2<T> a, T b) { return pk2<T>(a.x / b, a.y / b); }
template <typename T> inline pk2<T> operator/(pk2<T> a, pk2<T> b) { return pk2<T>(a.x / b.x, a.y / b.y); }
template <typename T> inline pk2<T> operator-(pk2<T> a, T b) { return pk2<T>(a.x - b, a.y - b); }
template <typename T> inline pk2<T> operator-(T a, pk2<T> b) { return pk2<T>(a - b.x, a - b.y); }
template <typename T> inline pk2<T>& operator+=(pk2<T>& a, pk2<T> b) { a.x += b.x; a.y += b.y; return a; }
template <typename T> inline pk2<T>& operator-=(pk2<T>& a, pk2<T> b) { a.x -= b.x; a.y -= b.y; return a; }
#else
template <typename T> using pk2 = T __attribute__((ext_vector_type(2)));
#endif
template <typename T> LFSD_DEV pk2<T> mk2(T a, T b) { pk2<T> v; v.x = a; v.y = b; return v; }

// ---- wave-level matrix helpers of the MFMA backward sweep (fp32, four 16-lane trajectories per wavefront) --------------
// mfma4b: v_mfma_f32_16x16x1_4b_f32 -- four independent 16x16 rank-1 updates, block b fed by the lanes of 16-lane group b:
//   D_b[i][j] += a(lane 16b+i) * b(lane 16b+j);  D_b[i][j] lives in register 4b + i%4 of lane 16(i/4) + j.
// tile_transpose: afterwards lane 16b+j holds D_b[i][j] in register i (column j of ITS block: the column-per-lane layout
//   of the rest of the kernel), by 8 v_permlane32_swap + 8 v_permlane16_swap.
// Both must be reached by all 64 lanes.  The emulator build restates them with an exchange buffer.
#if defined(LFSD_EMU)
struct f32x16 {
  float v[16];
  float& operator[](int i) { return v[i]; }
  const float& operator[](int i) const { return v[i]; }
};
// (exchange buffers of the emulated cross-lane operations: one slot per thread of the workgroup, a wavefront = 64 consecutive
//  threads -- workgroups of several wavefronts, oc_solve_wide_kernel<..., W>, exchange inside their own 64 slots)
constexpr int EMU_MAXT = 256;
inline void mfma4b(float a, float b, f32x16& acc) {
  static float sa[EMU_MAXT], sb[EMU_MAXT];
  const int t = threadIdx.x, w0 = t & ~63, l = t & 63;
  sa[t] = a; sb[t] = b;
  __syncthreads();
  for (int r = 0; r < 16; ++r) {
    const int blk = r / 4, i = 4 * (l >> 4) + r % 4, j = l & 15;
    acc[r] = std::fmaf(sa[w0 + 16 * blk + i], sb[w0 + 16 * blk + j], acc[r]);      // the hardware's k-ordered fmaf chain
  }
  __syncthreads();
}
inline void tile_transpose(f32x16& acc) {
  static float sx[EMU_MAXT][16];
  const int t = threadIdx.x, w0 = t & ~63, l = t & 63, b = l >> 4, j = l & 15;
  for (int r = 0; r < 16; ++r) sx[t][r] = acc[r];
  __syncthreads();
  for (int q = 0; q < 4; ++q)
    for (int r = 0; r < 4; ++r) acc[4 * q + r] = sx[w0 + 16 * q + j][4 * b + r];
  __syncthreads();
}
#else
typedef float f32x16 __attribute__((ext_vector_type(16)));
LFSD_DEV void mfma4b(float a, float b, f32x16& acc) { acc = __builtin_amdgcn_mfma_f32_16x16x1f32(a, b, acc, 0, 0, 0); }
LFSD_DEV void tile_transpose(f32x16& acc) {
  // exchange the block index (register group 4R..4R+3) with the lane-group index, one bit per stage
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int R0 = 0; R0 < 2; ++R0) {        // bit 1: register groups R0 / R0+2  <->  lane halves
      const float lo = acc[4 * R0 + r], hi = acc[4 * (R0 + 2) + r];      // (scalars first: __builtin_bit_cast applied to a
      const auto v = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, lo),      //  vector ELEMENT reads element 0)
                                                      __builtin_bit_cast(unsigned, hi), false, false);
      const unsigned v0 = v[0], v1 = v[1];
      acc[4 * R0 + r] = __builtin_bit_cast(float, v0);
      acc[4 * (R0 + 2) + r] = __builtin_bit_cast(float, v1);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int R1 = 0; R1 < 2; ++R1) {        // bit 0: register groups 2R1 / 2R1+1  <->  odd / even 16-lane rows
      const float lo = acc[8 * R1 + r], hi = acc[8 * R1 + 4 + r];
      const auto v = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, lo),
                                                      __builtin_bit_cast(unsigned, hi), false, false);
      const unsigned v0 = v[0], v1 = v[1];
      acc[8 * R1 + r] = __builtin_bit_cast(float, v0);
      acc[8 * R1 + 4 + r] = __builtin_bit_cast(float, v1);
    }
  }
}
#endif

// lane_get(v, j): the value lane j of the wavefront holds in v, on every lane (j is the same on all of them: v_readlane_b32).  Must be
// reached by all 64 lanes.
#if defined(LFSD_EMU)
template <typename T> inline T lane_get(T v, int j) {
  static T sb[EMU_MAXT];
  sb[threadIdx.x] = v;
  __syncthreads();
  const T r = sb[(threadIdx.x & ~63) + j];
  __syncthreads();
  return r;
}
#else
LFSD_DEV float lane_get(float v, int j) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j)); }
LFSD_DEV double lane_get(double v, int j) { return __shfl(v, j); }
#endif

// quarter_sum(v): sum of v over the four lanes l, l^16, l^32, l^48 of the wavefront, in every one of them (the wide kernel's
// backward sweep splits the rows of its dense products over the four 16-lane quarters).  Must be reached by all 64 lanes.
#if defined(LFSD_EMU)
template <typename T> inline T quarter_sum(T v) {
  static T sq[EMU_MAXT];
  const int t = threadIdx.x, w0 = t & ~63, l = t & 15;
  sq[t] = v;
  __syncthreads();
  const T r = (sq[w0 + l] + sq[w0 + l + 16]) + (sq[w0 + l + 32] + sq[w0 + l + 48]);
  __syncthreads();
  return r;
}
#else
LFSD_DEV float quarter_sum(float v) {
  // v_permlane32_swap(a, b): a' = [a.lo32, b.lo32], b' = [a.hi32, b.hi32]; with a = b = v their sum is v.lo + v.hi everywhere
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto p = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  const unsigned p0 = p[0], p1 = p[1];
  const float w = __builtin_bit_cast(float, p0) + __builtin_bit_cast(float, p1);
  const unsigned uw = __builtin_bit_cast(unsigned, w);
  const auto q = __builtin_amdgcn_permlane16_swap(uw, uw, false, false);
  const unsigned q0 = q[0], q1 = q[1];
  return __builtin_bit_cast(float, q0) + __builtin_bit_cast(float, q1);
}
LFSD_DEV double quarter_sum(double v) {
  const double w = v + __shfl_xor(v, 32);
  return w + __shfl_xor(w, 16);
}
#endif

// LFSD_ISSUE_FENCE(): the loads written above it are ISSUED above it.  Without it the compiler sinks a software prefetch
// ("load stage k-1 while stage k is processed") down to the first use of its values -- the copy at the end of the loop
// body -- i.e. it undoes the prefetch, and the next stage starts by waiting for its own operands (seen in the ISA of the
// backward sweeps: s_waitcnt vmcnt(15) ... vmcnt(3) between the first thirteen MFMAs of a stage; round 2 measured
// "prefetch on / off: no difference" for exactly that reason).  A compiler-level memory clobber: no instruction, and no
// wait either -- the s_waitcnt still goes where the values are first used.
#if defined(LFSD_EMU)
#define LFSD_ISSUE_FENCE()
#else
#define LFSD_ISSUE_FENCE() asm volatile("" ::: "memory")
#endif

// sched_load / sched_add: the counter of finished trajectories of a two-launch wide solve (OcArgs::sched): relaxed device-scope
// operations performed in the L2 (a plain load could be served by the scalar cache or the vector L1 for ever).  The emulator runs the
// workgroups of a launch one after the other.
#if defined(LFSD_EMU)
inline int sched_load(const int* p) { return *p; }
inline int sched_load_uniform(const int* p) { return *p; }
inline int sched_add(int* p, int v) { const int o = *p; *p += v; return o; }
#else
LFSD_DEV int sched_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// ... by all lanes of a wavefront at once, the same value on every lane (no LDS hand-over, no barrier)
LFSD_DEV int sched_load_uniform(int* p) { return __builtin_amdgcn_readfirstlane(sched_load(p)); }
LFSD_DEV int sched_add(int* p, int v) { return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#endif

// pin(x): the value is materialised HERE, unconditionally.  Needed where a load feeds one arm of a per-lane select
//   r = own_column ? f(lds[addr]) : other;
// -- clang turns that into a divergent branch around the load, and a sequence of thirteen of them into thirteen serialised
// LDS round trips (measured in the backward sweep of the OC solve, profiles/r03_g_ab_prefetch_pin.txt: 1600 of 8300 cycles
// per stage for the symmetrisation of V_xx alone).  With the loads issued back to back and pinned, the select is a v_cndmask.
// (Tried and dropped in the forward auxiliary sweep, which runs at 256 + 256 registers with spills: batching the loads of
// its stiff steps this way doubled its scratch traffic, 1.01 -> 2.13 ms; batching only its node staging cost 3 %.)
#if defined(LFSD_EMU)
template <typename T> LFSD_DEV void pin(T&) {}
#else
template <typename T> LFSD_DEV void pin(T& x) { asm volatile("" : "+v"(x)); }
#endif

// lds_fetch<N>(src, dst): N consecutive LDS words into registers, ALL reads issued back to back, the values materialised
// here.  Where a phase applies staged coefficients through the generated sparse operators the compiler, left to itself,
// emits read - wait - four FMAs - read - wait ...: one exposed LDS round trip per 16 bytes (185 of them per split unit of
// the forward auxiliary sweep, ~100 cycles each on a wavefront that is alone on its SIMD: two thirds of the kernel's time).
// Fetched first, the operators run on registers and the phase waits once.
// lds_issue / lds_land: the two halves, for several arrays fetched together (issue all, then land all).
template <int N, typename T> LFSD_DEV void lds_issue(const T* src, T* dst) {
#pragma unroll
  for (int i = 0; i < N; ++i) dst[i] = src[i];
}
template <int N, typename T> LFSD_DEV void lds_issue_strided(const T* src, int stride, T* dst) {      // N words `stride` apart
#pragma unroll
  for (int i = 0; i < N; ++i) dst[i] = src[i * stride];
}
template <int N, typename T> LFSD_DEV void lds_land(T* dst) {
#pragma unroll
  for (int i = 0; i < N; ++i) pin(dst[i]);
}
template <int N, typename T> LFSD_DEV void lds_fetch(const T* src, T* dst) { lds_issue<N>(src, dst); lds_land<N>(dst); }

// pin64(x): pin() in the fp64 instantiations only.  There a dense product whose result is first used beyond a branch had
// its FMAs sunk to that use by the compiler while its LDS reads stayed put (they cannot cross the barrier in between): all
// 221 operands of Q = [A B]^T Y of the backward sweep were read, spilled to scratch and reloaded one by one -- 157 scratch
// round trips per stage that miss the L2 (116 KB of scratch per wavefront), 95 000 cycles of a stage that computes for
// about 5 000 (profiles/r03_o_fp64_backward.txt).  A pinned result keeps the FMAs with their reads; with it the fp64 sweep
// has a scheduling fence per row (LFSD_SCHED_FENCE64) and two row buffers, a row's LDS reads issued while the previous row is
// multiplied (cpdp_oc.h, OcSolver::backward).
template <typename T> LFSD_DEV void pin64(T& x) { if constexpr (sizeof(T) == 8) pin(x); }

template <typename T> struct Eps;
template <> struct Eps<float> { static LFSD_DEV float v() { return 1.1920929e-07f; } };
template <> struct Eps<double> { static LFSD_DEV double v() { return 2.220446049250313e-16; } };

template <typename T> LFSD_HD constexpr int aux_rk() { return sizeof(T) == 4 ? kAuxRk32 : kAuxRk64; }

template <typename T> LFSD_DEV T t_abs(T a) { return a < T(0) ? -a : a; }
template <typename T> LFSD_DEV T t_max(T a, T b) { return a > b ? a : b; }
template <typename T> LFSD_DEV T t_min(T a, T b) { return a < b ? a : b; }
template <typename T> LFSD_DEV bool t_finite(T a) { return (a - a) == T(0); }
LFSD_DEV float t_sqrt(float a) { return sqrtf(a); }
LFSD_DEV double t_sqrt(double a) { return sqrt(a); }
// Reciprocal and reciprocal square root of a PIVOT (positive, well inside the normal range): the hardware estimate
// (v_rcp_f32 / v_rsq_f32, 1 ulp) refined by one Newton step -- three to four instructions where the IEEE division and
// square root of the compiler are ten-instruction dependent sequences each.  fp64 and the CPU emulator divide.
#if defined(LFSD_EMU)
LFSD_DEV float t_rcp(float a) { return 1.0f / a; }
LFSD_DEV float t_rsqrt(float a) { return 1.0f / sqrtf(a); }
#else
LFSD_DEV float t_rcp(float a) { float r = __builtin_amdgcn_rcpf(a); return fmaf(fmaf(-a, r, 1.0f), r, r); }
LFSD_DEV float t_rsqrt(float a) { float r = __builtin_amdgcn_rsqf(a); return r * fmaf(-0.5f * a * r, r, 1.5f); }
#endif
LFSD_DEV double t_rcp(double a) { return 1.0 / a; }
LFSD_DEV double t_rsqrt(double a) { return 1.0 / sqrt(a); }
// sin / cos of the generated model code (codegen.py prints lfsd::t_sin / lfsd::t_cos).  The device library's sinf / cosf are
// ~140-instruction routines each (150 for both through sincosf; tools/probes/trig_probe.hip), and the robot arm's dynamics
// call four of them per evaluation -- 800 evaluations per iteration of its roll-outs, the largest phase of its solve
// (profiles/r04_g_arm_wide_clock.txt).  fp32 on the GPU: one Cody-Waite reduction by multiples of pi/2 (three constants, exact
// products for |x| <= 100) + the two degree-7 / degree-8 minimax polynomials of cephes' sinf / cosf on [-pi/4, pi/4]; t_sin(a)
// and t_cos(a) of the same argument share the reduction after inlining.  Measured against fp64 on 2^24 arguments in
// [-100, 100] (trig_probe): see profiles/r04_l_trig_probe.txt.  Beyond |x| = 100, in fp64 and in the CPU emulator: the library.
LFSD_DEV double t_sin(double a) { return sin(a); }
LFSD_DEV double t_cos(double a) { return cos(a); }
#if defined(LFSD_EMU)
LFSD_DEV float t_sin(float a) { return sinf(a); }
LFSD_DEV float t_cos(float a) { return cosf(a); }
#else
LFSD_DEV void sincos_pio4(float x, float& sr, float& cr, int& quad) {
  const float q = __builtin_rintf(x * 0.63661977236758134f);          // nearest multiple of pi/2
  float r = fmaf(q, -1.57073974609375f, x);                             // pi/2 = A + B + C, A and B with short mantissas
  r = fmaf(q, -5.657970905303955078125e-05f, r);
  r = fmaf(q, -9.920936294705029468e-10f, r);
  const float z = r * r;
  sr = fmaf(fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f) * z, r, r);
  cr = fmaf(fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f) * z, z, fmaf(-0.5f, z, 1.0f));
  quad = (int)q;
}
LFSD_DEV float t_sin(float x) {
  float sr, cr; int n;
  sincos_pio4(x, sr, cr, n);
  float v = (n & 1) ? cr : sr;
  v = (n & 2) ? -v : v;
  if (!(__builtin_fabsf(x) <= 100.0f)) v = sinf(x);
  return v;
}
LFSD_DEV float t_cos(float x) {
  float sr, cr; int n;
  sincos_pio4(x, sr, cr, n);
  float v = (n & 1) ? sr : cr;
  v = ((n + 1) & 2) ? -v : v;
  if (!(__builtin_fabsf(x) <= 100.0f)) v = cosf(x);
  return v;
}
#endif
LFSD_DEV float t_floor(float a) { return floorf(a); }
LFSD_DEV double t_floor(double a) { return floor(a); }
LFSD_DEV float t_pow(float a, float b) { return powf(a, b); }
LFSD_DEV double t_pow(double a, double b) { return pow(a, b); }

// ---- tiny dense helpers on group-uniform n x n matrices (row-major, in registers) -----------
// Cholesky A = L L^T in place (lower); false if not positive definite.  The DIAGONAL of the result holds 1 / L_jj: the
// substitutions of chol_solve then multiply instead of divide (an IEEE fp32 division is a ten-instruction dependent
// sequence on this hardware, and the backward sweep of the OC solve runs two solves per stage on every lane).
template <int n, typename T> LFSD_DEV bool chol_factor(T* A, T& dmin) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < n; ++j) {
    T d = A[j * n + j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= A[j * n + k] * A[j * n + k];
    if (!(d > T(0))) { if (ok && d < dmin) dmin = d; ok = false; d = T(1); }    // only the first failing pivot is meaningful
    const T inv = t_rsqrt(d);
    A[j * n + j] = inv;
#pragma unroll
    for (int i = j + 1; i < n; ++i) {
      T s = A[i * n + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= A[i * n + k] * A[j * n + k];
      A[i * n + j] = s * inv;
    }
  }
  return ok;
}
template <int n, typename T> LFSD_DEV void chol_solve(const T* Lm, T* b) {
#pragma unroll
  for (int i = 0; i < n; ++i) {
    T s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= Lm[i * n + k] * b[k];
    b[i] = s * Lm[i * n + i];
  }
#pragma unroll
  for (int i = n - 1; i >= 0; --i) {
    T s = b[i];
#pragma unroll
    for (int k = i + 1; k < n; ++k) s -= Lm[k * n + i] * b[k];
    b[i] = s * Lm[i * n + i];
  }
}
// Box-constrained stage problem of the control-limited backward sweep (finite control_lb / control_ub of
// COCSys.setControlVariable, CPDP.py:33-46, which the reference hands to IPOPT as lbw / ubw):
//     min_x  1/2 x^T Q x + q^T x   s.t.  lo <= x <= hi            (Q = Q_uu + mu I positive definite, n <= 4 controls)
// by a primal active-set iteration on the masked system (clamped rows / columns replaced by identity): solve, clamp the
// components that left the box, re-solve; when nothing moves, release the clamped component whose multiplier has the
// wrong sign most.  Returns the Cholesky factor of the final masked matrix in Lf (the feedback gains of the free
// components are solved with it; clamped components get zero gain) and the clamp mask.
template <int n, typename T> LFSD_DEV bool box_qp(const T* Q, const T* q, const T* lo, const T* hi, T* x, unsigned& mask, T* Lf, T& dmin) {
  mask = 0u;
  T xc[n];
#pragma unroll
  for (int i = 0; i < n; ++i) xc[i] = T(0);
  bool ok = true;
  for (int round = 0; round < 3 * n + 2; ++round) {
    T b[n];
#pragma unroll
    for (int i = 0; i < n; ++i) {
      const bool ci = (mask >> i) & 1u;
      T s = ci ? xc[i] : -q[i];
#pragma unroll
      for (int j = 0; j < n; ++j) {
        const bool cj = (mask >> j) & 1u;
        Lf[i * n + j] = (ci || cj) ? ((i == j) ? T(1) : T(0)) : Q[i * n + j];
        if (!ci && cj) s -= Q[i * n + j] * xc[j];
      }
      b[i] = s;
    }
    T dd = T(0);
    if (!chol_factor<n>(Lf, dd)) { ok = false; if (dd < dmin) dmin = dd; break; }
    chol_solve<n>(Lf, b);
    unsigned newmask = mask;
#pragma unroll
    for (int i = 0; i < n; ++i) {
      if ((mask >> i) & 1u) continue;
      if (b[i] < lo[i]) { newmask |= 1u << i; xc[i] = lo[i]; }
      else if (b[i] > hi[i]) { newmask |= 1u << i; xc[i] = hi[i]; }
    }
#pragma unroll
    for (int i = 0; i < n; ++i) x[i] = ((newmask >> i) & 1u) ? xc[i] : b[i];
    if (newmask != mask) { mask = newmask; continue; }
    // stationary for this active set: multipliers g_i = (Q x + q)_i of the clamped components must push outward
    int worst = -1;
    T wv = T(0);
#pragma unroll
    for (int i = 0; i < n; ++i) {
      if (!((mask >> i) & 1u)) continue;
      T g = q[i];
#pragma unroll
      for (int j = 0; j < n; ++j) g += Q[i * n + j] * x[j];
      const T viol = (xc[i] <= lo[i]) ? -g : g;         // at the lower bound the gradient must be >= 0, at the upper <= 0
      if (viol > wv) { wv = viol; worst = i; }
    }
    if (worst < 0) break;
    mask &= ~(1u << worst);
  }
  return ok;
}
// LU without pivoting, in place (unit lower + upper).  For I + small and SPD-like matrices.  As in chol_factor the
// diagonal of the result holds the RECIPROCAL pivots, and lu_solve multiplies by them.
template <int n, typename T> LFSD_DEV void lu_factor(T* A) {
#pragma unroll
  for (int j = 0; j < n; ++j) {
    const T inv = t_rcp(A[j * n + j]);
    A[j * n + j] = inv;
#pragma unroll
    for (int i = j + 1; i < n; ++i) {
      const T f = A[i * n + j] * inv;
      A[i * n + j] = f;
#pragma unroll
      for (int k = j + 1; k < n; ++k) A[i * n + k] -= f * A[j * n + k];
    }
  }
}
template <int n, typename T> LFSD_DEV void lu_solve(const T* A, T* b) {
#pragma unroll
  for (int i = 0; i < n; ++i) {
#pragma unroll
    for (int k = 0; k < i; ++k) b[i] -= A[i * n + k] * b[k];
  }
#pragma unroll
  for (int i = n - 1; i >= 0; --i) {
#pragma unroll
    for (int k = i + 1; k < n; ++k) b[i] -= A[i * n + k] * b[k];
    b[i] *= A[i * n + i];
  }
}
template <int n, typename T> LFSD_DEV void mat_inverse(const T* A, T* Ainv) {
  T F[n * n];
#pragma unroll
  for (int i = 0; i < n * n; ++i) F[i] = A[i];
  lu_factor<n>(F);
#pragma unroll
  for (int c = 0; c < n; ++c) {
    T b[n];
#pragma unroll
    for (int i = 0; i < n; ++i) b[i] = (i == c) ? T(1) : T(0);
    lu_solve<n>(F, b);
#pragma unroll
    for (int i = 0; i < n; ++i) Ainv[i * n + c] = b[i];
  }
}
template <int n, typename T> LFSD_DEV void matmul(const T* A, const T* B, T* C) {
#pragma unroll
  for (int i = 0; i < n; ++i) {
#pragma unroll
    for (int j = 0; j < n; ++j) {
      T s = T(0);
#pragma unroll
      for (int k = 0; k < n; ++k) s += A[i * n + k] * B[k * n + j];
      C[i * n + j] = s;
    }
  }
}
// P = phi1(M) = M^-1 (I - exp(-M)) for a small matrix with non-negative spectrum
// (scaling and squaring: Taylor of degree 8 on M/2^s, then phi1(2A) = (I + e^-A) phi1(A) / 2).
template <typename T> struct PhiDeg;
template <> struct PhiDeg<float> { static constexpr int v = 6; };
template <> struct PhiDeg<double> { static constexpr int v = 9; };
// P = phi1(M), P2 = phi1(2M)
template <int n, typename T> LFSD_DEV void phi1_neg(const T* M, T* P, T* P2) {
  T nrm = T(0);
#pragma unroll
  for (int i = 0; i < n; ++i) {
    T r = T(0);
#pragma unroll
    for (int j = 0; j < n; ++j) r += t_abs(M[i * n + j]);
    nrm = t_max(nrm, r);
  }
  int sq = 0;
  T sc = T(1);
  while (nrm * sc > T(0.25) && sq < 60) { sc *= T(0.5); ++sq; }
  T A[n * n], E[n * n], W[n * n];
#pragma unroll
  for (int i = 0; i < n * n; ++i) { A[i] = M[i] * sc; P[i] = T(0); }
  const T ck[10] = {T(1), T(1) / T(2), T(1) / T(6), T(1) / T(24), T(1) / T(120), T(1) / T(720), T(1) / T(5040),
                    T(1) / T(40320), T(1) / T(362880), T(1) / T(3628800)};
  constexpr int DEG = PhiDeg<T>::v;       // |A| <= 1/4: truncation 4^-(DEG+1)/(DEG+2)! below round-off
#pragma unroll
  for (int i = 0; i < n; ++i) P[i * n + i] = ck[DEG];
#pragma unroll
  for (int k = DEG - 1; k >= 0; --k) {
    matmul<n>(A, P, W);
#pragma unroll
    for (int i = 0; i < n * n; ++i) P[i] = -W[i];
#pragma unroll
    for (int i = 0; i < n; ++i) P[i * n + i] += ck[k];
  }
  matmul<n>(A, P, W);
#pragma unroll
  for (int i = 0; i < n * n; ++i) E[i] = -W[i];
#pragma unroll
  for (int i = 0; i < n; ++i) E[i * n + i] += T(1);
  for (int it = 0; it < sq; ++it) {
    matmul<n>(E, P, W);
#pragma unroll
    for (int i = 0; i < n * n; ++i) P[i] = T(0.5) * (P[i] + W[i]);
    matmul<n>(E, E, W);
#pragma unroll
    for (int i = 0; i < n * n; ++i) E[i] = W[i];
  }
  matmul<n>(E, P, W);
#pragma unroll
  for (int i = 0; i < n * n; ++i) P2[i] = T(0.5) * (P[i] + W[i]);
}
// ---- a small matrix spread ROW PER LANE over a sub-group of Q = 1 / 2 / 4 adjacent lanes (Q | 4, sub-group aligned) ------
// sub_bcast<Q>(v, k): v of lane k of the caller's sub-group, in every lane of it.  On the GPU a DPP move (quad_perm), i.e. a
// register-to-register instruction without LDS; k must be a constant after unrolling.  Every lane that could be a SOURCE
// has to be active: the callers run whole lane groups through the same control flow.  The CPU emulator restates it with an
// exchange buffer (all lanes of the sub-group must call it together).
template <int Q> constexpr bool sub_ok() { return Q == 1 || Q == 2 || Q == 4; }
#if defined(LFSD_EMU)
template <int Q, typename T> inline T sub_bcast(T v, int k) {
  static_assert(sub_ok<Q>(), "sub-group of 1, 2 or 4 lanes");
  if (Q == 1) return v;
  static T sb[EMU_MAXT];
  const int l = threadIdx.x;
  sb[l] = v;
  __syncthreads();
  const T r = sb[(l & ~(Q - 1)) | k];
  __syncthreads();
  return r;
}
#else
template <int CTRL> LFSD_DEV float dpp_mov(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int CTRL> LFSD_DEV double dpp_mov(double v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const int lo = __builtin_amdgcn_mov_dpp((int)(unsigned)u, CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_mov_dpp((int)(unsigned)(u >> 32), CTRL, 0xf, 0xf, true);
  return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}
template <int Q, typename T> LFSD_DEV T sub_bcast(T v, int k) {
  static_assert(sub_ok<Q>(), "sub-group of 1, 2 or 4 lanes");
  if constexpr (Q == 1) return v;
  else if constexpr (Q == 2) return k == 0 ? dpp_mov<0xA0>(v) : dpp_mov<0xF5>(v);            // quad_perm [0,0,2,2] / [1,1,3,3]
  else return k == 0 ? dpp_mov<0x00>(v) : (k == 1 ? dpp_mov<0x55>(v) : (k == 2 ? dpp_mov<0xAA>(v) : dpp_mov<0xFF>(v)));
}
#endif
// row_bcast(v, k): v of lane k (0..15) of the caller's 16-lane row -- lanes 16r .. 16r+15 of the wavefront, the lane group of the lean
// OC kernels' backward sweep -- in every lane of it.  On the GPU one DPP move (row_newbcast:k), which the compiler folds into the
// instruction that consumes it where that instruction takes a DPP operand (v_fmac_f32, v_max_f32, ...): no LDS trip and no wait; k
// must be a constant after unrolling (the switch below folds to one move then; a k that is not would compile to sixteen).  bound_ctrl is
// set, so a SOURCE lane that EXEC has switched off would deliver 0 instead of its value.  A source lane always lies in the reader's
// own row, so what the callers have to keep is that control flow is uniform WITHIN a row: a row is a lane group, and a group takes
// every branch as one (padded and finished groups ride along; groups may part from each other).  The sweeps in fact run whole
// wavefronts through one control flow, which is what the emulator's exchange buffer needs.
// row_max(v, first, n): max of t_max-folded v over lanes first .. first+n-1 of the row, from T(0), in lane order, on every lane.
constexpr bool row_xchg_ok(int lanes) { return lanes == 16; }      // a lane group that is exactly one DPP row
#if defined(LFSD_EMU)
template <typename T> inline T row_bcast(T v, int k) {
  static T sb[EMU_MAXT];
  const int l = threadIdx.x;
  sb[l] = v;
  __syncthreads();
  const T r = sb[(l & ~15) | k];
  __syncthreads();
  return r;
}
#else
LFSD_DEV float row_bcast(float v, int k) {
  switch (k) {
    case 0: return dpp_mov<0x150>(v);   case 1: return dpp_mov<0x151>(v);   case 2: return dpp_mov<0x152>(v);   case 3: return dpp_mov<0x153>(v);
    case 4: return dpp_mov<0x154>(v);   case 5: return dpp_mov<0x155>(v);   case 6: return dpp_mov<0x156>(v);   case 7: return dpp_mov<0x157>(v);
    case 8: return dpp_mov<0x158>(v);   case 9: return dpp_mov<0x159>(v);   case 10: return dpp_mov<0x15A>(v);  case 11: return dpp_mov<0x15B>(v);
    case 12: return dpp_mov<0x15C>(v);  case 13: return dpp_mov<0x15D>(v);  case 14: return dpp_mov<0x15E>(v);  default: return dpp_mov<0x15F>(v);
  }
}
#endif
// fmac2_row_bcast<K>(acc, a, wa, b, wb): acc += row_bcast(a, K) * wa; acc += row_bcast(b, K) * wb -- in this order, each ONE
// v_fmac_f32 with the broadcast as its DPP operand (the fused multiply-adds the compiler contracts the two statements to, so the
// bits are those of the LDS-fed statements; it does not fold a DPP move into them by itself -- 104 moves per stage of the
// backward sweep).  The compiler's hazard recognizer does not look into the statement: the DPP operands a, b must have been
// written at least two wait states earlier, and a vector write of EXEC five.  The callers pass values that a dependent chain
// separates from this point and start a run with dpp_settle(), but neither binds the register allocator or the scheduler (a copy
// back from an AGPR may land anywhere): what GUARANTEES the distances is the scan of every build's assembly, isa_check.py's
// find_dpp_hazards, which rejects a build that has a writer too close to any DPP instruction (runtime.py: _checked_build).
#if defined(LFSD_EMU)
inline void dpp_settle() {}
template <int K> inline void fmac2_row_bcast(float& acc, float a, float wa, float b, float wb) {
  acc += row_bcast(a, K) * wa;
  acc += row_bcast(b, K) * wb;
}
#else
LFSD_DEV void dpp_settle() { asm volatile("s_nop 4"); }
template <int K> LFSD_DEV void fmac2_row_bcast(float& acc, float a, float wa, float b, float wb) {
  static_assert(K >= 0 && K < 16, "lane of the row");
  asm volatile("v_fmac_f32_dpp %0, %1, %2 row_newbcast:%5 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
               "v_fmac_f32_dpp %0, %3, %4 row_newbcast:%5 row_mask:0xf bank_mask:0xf bound_ctrl:1"
               : "+v"(acc) : "v"(a), "v"(wa), "v"(b), "v"(wb), "n"(K));
}
#endif
template <typename T> LFSD_DEV T row_max(T v, int first, int n) {
  T r = T(0);
#pragma unroll
  for (int a = 0; a < n; ++a) r = t_max(r, row_bcast(v, first + a));
  return r;
}
// smallest sub-group that holds one row per lane of an n x n matrix (n <= 4)
template <int n> constexpr int sub_lanes() { return n <= 1 ? 1 : (n == 2 ? 2 : 4); }
// W = A B, row a of each matrix in lane a of the sub-group (lanes a >= n carry zeros); same summation order as matmul<n>
template <int n, int Q, typename T> LFSD_DEV void matmul_rows(const T* Arow, const T* Brow, T* Wrow) {
#pragma unroll
  for (int j = 0; j < n; ++j) Wrow[j] = T(0);
#pragma unroll
  for (int k = 0; k < n; ++k) {
#pragma unroll
    for (int j = 0; j < n; ++j) Wrow[j] += Arow[k] * sub_bcast<Q>(Brow[j], k);
  }
}
// phi1_neg with the matrix spread row per lane: lane a of the sub-group holds row a of M and receives row a of
// P = phi1(M) and P2 = phi1(2M).  The scaling (sc = 2^-sq with |M| sc <= 1/4) comes from the caller, who makes it uniform
// over everything that runs through here together (over-scaling is harmless: more squarings of a smaller argument).
template <int n, int Q, typename T> LFSD_DEV void phi1_neg_rows(const T* Mrow, int a, int sq, T sc, T* P, T* P2) {
  T A[n], E[n], W[n];
  const T ck[10] = {T(1), T(1) / T(2), T(1) / T(6), T(1) / T(24), T(1) / T(120), T(1) / T(720), T(1) / T(5040),
                    T(1) / T(40320), T(1) / T(362880), T(1) / T(3628800)};
  constexpr int DEG = PhiDeg<T>::v;
#pragma unroll
  for (int j = 0; j < n; ++j) { A[j] = Mrow[j] * sc; P[j] = (j == a) ? ck[DEG] : T(0); }
#pragma unroll
  for (int k = DEG - 1; k >= 0; --k) {
    matmul_rows<n, Q>(A, P, W);
#pragma unroll
    for (int j = 0; j < n; ++j) P[j] = ((j == a) ? ck[k] : T(0)) - W[j];
  }
  matmul_rows<n, Q>(A, P, W);
#pragma unroll
  for (int j = 0; j < n; ++j) E[j] = ((j == a) ? T(1) : T(0)) - W[j];
  for (int it = 0; it < sq; ++it) {
    matmul_rows<n, Q>(E, P, W);
#pragma unroll
    for (int j = 0; j < n; ++j) P[j] = T(0.5) * (P[j] + W[j]);
    matmul_rows<n, Q>(E, E, W);
#pragma unroll
    for (int j = 0; j < n; ++j) E[j] = W[j];
  }
  matmul_rows<n, Q>(E, P, W);
#pragma unroll
  for (int j = 0; j < n; ++j) P2[j] = T(0.5) * (P[j] + W[j]);
}
template <int n, typename T> LFSD_DEV void matvec(const T* A, const T* v, T* y) {
#pragma unroll
  for (int i = 0; i < n; ++i) {
    T s = T(0);
#pragma unroll
    for (int k = 0; k < n; ++k) s += A[i * n + k] * v[k];
    y[i] = s;
  }
}

}  // namespace lfsd
