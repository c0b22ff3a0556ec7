// wave_prims.h -- wavefront primitives shared by the wavefront-per-trajectory solvers (hs_solver_wave.h, hs_solver_fused.h,
// shoot_solver_wave.h): the phase barrier, butterfly reductions, the small L D L^T, lane movement (DPP, v_readlane, permlane swaps)
// and the affine wave scans.  Free functions; nothing here knows a solver's records.
#pragma once
#include <hip/hip_runtime.h>
#include "hs_solver.h"   // detail::dmax

namespace myriad {
// Barrier of the phases of ONE wavefront.  A workgroup of a single wavefront uses the hardware barrier; network systems pack
// several independent wavefronts into a workgroup (they share the weights in LDS) and may not meet at a workgroup barrier:
// there the phases of a wavefront are ordered by a fence (all its LDS / global accesses retired) + the wave barrier.
template <bool MULTI>
__device__ inline void wave_sync() {
  if constexpr (MULTI) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); }
  else __syncthreads();
}
__device__ inline double wv_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline double wv_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const double t = __shfl_xor(v, o, 64); v = v > t ? v : t; }
  return v;
}
__device__ inline double wv_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const double t = __shfl_xor(v, o, 64); v = v < t ? v : t; }
  return v;
}
// reciprocal from v_rcp_f64 + two Newton steps (the operands here are pivots already known to exceed reg_floor)
__device__ inline double fast_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  double e = fma(-x, r, 1.0);
  r = fma(r, e, r);
  e = fma(-x, r, 1.0);
  return fma(r, e, r);
}
// L D L^T of a small SPD block with the SAME pivot rule as detail::chol_reg (the pivots d_j are the squares of the
// Cholesky diagonal): a <- unit lower factor (strict lower part), dinv <- 1 / d.  No sqrt, one reciprocal per pivot.
template <int n>
__device__ inline int ldl_reg(double* a, double* dinv, double floor_) {
  int nreg = 0;
  double d[n];
#pragma unroll
  for (int j = 0; j < n; ++j) {
    double dj = a[j * n + j];
#pragma unroll
    for (int k = 0; k < j; ++k) dj -= a[j * n + k] * a[j * n + k] * d[k];
    if (!(dj > floor_)) { dj = detail::dmax(fabs(dj), floor_); ++nreg; }
    d[j] = dj;
    dinv[j] = fast_rcp(dj);
#pragma unroll
    for (int i = j + 1; i < n; ++i) {
      double t = a[i * n + j];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= a[i * n + k] * a[j * n + k] * d[k];
      a[i * n + j] = t * dinv[j];
    }
  }
  return nreg;
}
template <int n>
__device__ inline void ldl_solve(const double* a, const double* dinv, double* b) {
#pragma unroll
  for (int i = 0; i < n; ++i) {
#pragma unroll
    for (int k = 0; k < i; ++k) b[i] -= a[i * n + k] * b[k];
  }
#pragma unroll
  for (int i = 0; i < n; ++i) b[i] *= dinv[i];
#pragma unroll
  for (int i = n - 1; i >= 0; --i) {
#pragma unroll
    for (int k = i + 1; k < n; ++k) b[i] -= a[k * n + i] * b[k];
  }
}

// every lane <- lane LANE of its own row of 16 lanes (DPP row_newbcast: stays in the vector pipe, ~10 cycles; v_readlane
// goes through the scalar register file and costs ~55 cycles before a vector instruction can use the value)
template <int LANE>
__device__ inline double wv_row_bcast(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v), rlo, rhi;
  asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %2 row_newbcast:%4 row_mask:0xf bank_mask:0xf\n\t"
               "v_mov_b32_dpp %1, %3 row_newbcast:%4 row_mask:0xf bank_mask:0xf"
               : "=&v"(rlo), "=&v"(rhi) : "v"(lo), "v"(hi), "n"(LANE));
  return __hiloint2double(rhi, rlo);
}
template <int NQ_>
struct RowBcast {       // q[i] = value of lane i (i < NQ_ <= 16) of the caller's row, for all i
  template <int I = 0>
  __device__ static inline void all(double v, double* q) {
    if constexpr (I < NQ_) { q[I] = wv_row_bcast<I>(v); all<I + 1>(v, q); }
  }
};

__device__ inline int wv_isum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Affine maps x -> A x + b (n x n) in registers, one per lane: composition and the two wave scans built on it.
// `wv_down(v, d)` = value of lane + d (own value beyond the wave), `wv_up` = lane - d.
__device__ inline double wv_down(double v, int d) { return __shfl_down(v, d, 64); }
__device__ inline double wv_up(double v, int d) { return __shfl_up(v, d, 64); }
template <int n>
__device__ inline void affine_after(double* A, double* b, const double* A2, const double* b2) {   // (A,b) <- (A,b) o (A2,b2)
  double R[n * n], r[n];
#pragma unroll
  for (int i = 0; i < n; ++i) {
    double v = b[i];
#pragma unroll
    for (int k = 0; k < n; ++k) v += A[i * n + k] * b2[k];
    r[i] = v;
#pragma unroll
    for (int j = 0; j < n; ++j) {
      double w = 0.0;
#pragma unroll
      for (int k = 0; k < n; ++k) w += A[i * n + k] * A2[k * n + j];
      R[i * n + j] = w;
    }
  }
#pragma unroll
  for (int i = 0; i < n * n; ++i) A[i] = R[i];
#pragma unroll
  for (int i = 0; i < n; ++i) b[i] = r[i];
}
// suffix scan: lane l <- T_l o T_{l+1} o .. o T_63        prefix scan: lane l <- T_l o T_{l-1} o .. o T_0
template <int n, bool SUFFIX>
__device__ inline void affine_scan(double* A, double* b) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    double A2[n * n], b2[n];
#pragma unroll
    for (int i = 0; i < n * n; ++i) A2[i] = SUFFIX ? wv_down(A[i], d) : wv_up(A[i], d);
#pragma unroll
    for (int i = 0; i < n; ++i) b2[i] = SUFFIX ? wv_down(b[i], d) : wv_up(b[i], d);
    if (SUFFIX ? (lane + d < 64) : (lane >= d)) affine_after<n>(A, b, A2, b2);
  }
}
// The prefix scan with DPP moves instead of ds_bpermute (one VALU move per dword and round): four shifts inside the rows
// of 16 lanes, then row_bcast:15 (rows 1, 3 take lane 15 / 47) and row_bcast:31 (lanes 32..63 take lane 31) -- the
// wave-scan idiom of GFX9.  Inline asm, executed by all lanes: a DPP builtin sunk into the divergent branch that consumes
// it would read 0 from the lanes EXEC has switched off (see dpp_row_shr4 below).
template <int STEP>
__device__ inline double dpp_scan_src(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v), rlo, rhi;
  if constexpr (STEP == 0)
    asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %2 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_mov_b32_dpp %1, %3 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "=&v"(rlo), "=&v"(rhi) : "v"(lo), "v"(hi));
  else if constexpr (STEP == 1)
    asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %2 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_mov_b32_dpp %1, %3 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "=&v"(rlo), "=&v"(rhi) : "v"(lo), "v"(hi));
  else if constexpr (STEP == 2)
    asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %2 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_mov_b32_dpp %1, %3 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "=&v"(rlo), "=&v"(rhi) : "v"(lo), "v"(hi));
  else if constexpr (STEP == 3)
    asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %2 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_mov_b32_dpp %1, %3 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "=&v"(rlo), "=&v"(rhi) : "v"(lo), "v"(hi));
  else if constexpr (STEP == 4)
    asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %2 row_bcast:15 row_mask:0xa bank_mask:0xf\n\tv_mov_b32_dpp %1, %3 row_bcast:15 row_mask:0xa bank_mask:0xf" : "=&v"(rlo), "=&v"(rhi) : "v"(lo), "v"(hi));
  else
    asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %2 row_bcast:31 row_mask:0xc bank_mask:0xf\n\tv_mov_b32_dpp %1, %3 row_bcast:31 row_mask:0xc bank_mask:0xf" : "=&v"(rlo), "=&v"(rhi) : "v"(lo), "v"(hi));
  return __hiloint2double(rhi, rlo);
}
template <int n, int STEP>
__device__ inline void affine_prefix_round(double* A, double* b) {
  const int lane = threadIdx.x & 63, l16 = lane & 15;
  double A2[n * n], b2[n];
#pragma unroll
  for (int i = 0; i < n * n; ++i) A2[i] = dpp_scan_src<STEP>(A[i]);
#pragma unroll
  for (int i = 0; i < n; ++i) b2[i] = dpp_scan_src<STEP>(b[i]);
  const bool take = STEP < 4 ? (l16 >= (1 << STEP)) : (STEP == 4 ? ((lane >> 4) & 1) != 0 : lane >= 32);
  if (take) affine_after<n>(A, b, A2, b2);
}
template <int n>
__device__ inline void affine_prefix_scan_dpp(double* A, double* b) {       // lane l <- T_l o T_{l-1} o .. o T_0
  affine_prefix_round<n, 0>(A, b); affine_prefix_round<n, 1>(A, b); affine_prefix_round<n, 2>(A, b);
  affine_prefix_round<n, 3>(A, b); affine_prefix_round<n, 4>(A, b); affine_prefix_round<n, 5>(A, b);
}

// every lane <- lane l (l wave-uniform): through the scalar register file
__device__ inline double rdlane(double v, int l) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_readlane(lo, l);
  hi = __builtin_amdgcn_readlane(hi, l);
  return __hiloint2double(hi, lo);
}
// lane l <- lane l-4 within its row of 16 lanes (0 where l%16 < 4).  Inline asm on purpose: the compiler sinks the
// DPP builtin into the divergent branch of the select that consumes it, and a DPP read of a lane that EXEC has
// switched off returns 0 -- the shifted value must be produced with every lane enabled.
// (s_nop 1 in every DPP helper of this file: a DPP read needs two wait states behind the vector instruction that wrote its source, and
// nothing inserts them inside inline asm.)
__device__ inline double dpp_row_shr4(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v), rlo, rhi;
  asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %2 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
               "v_mov_b32_dpp %1, %3 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1"
               : "=&v"(rlo), "=&v"(rhi) : "v"(lo), "v"(hi));
  return __hiloint2double(rhi, rlo);
}
__device__ inline double dpp_row_shr8(double v) {      // lane l <- lane l-8 within its row of 16
  int lo = __double2loint(v), hi = __double2hiint(v), rlo, rhi;
  asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %2 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
               "v_mov_b32_dpp %1, %3 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1"
               : "=&v"(rlo), "=&v"(rhi) : "v"(lo), "v"(hi));
  return __hiloint2double(rhi, rlo);
}
// every lane group <- the values of lane groups 0..3 (same lane within the group): v_permlane32_swap, then v_permlane16_swap twice
__device__ inline void gather4(double x, double* o) {
  const auto lo = __builtin_amdgcn_permlane32_swap(__double2loint(x), __double2loint(x), false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap(__double2hiint(x), __double2hiint(x), false, false);
  // [0]: groups (0, 1, 0, 1); [1]: groups (2, 3, 2, 3)
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const auto l2 = __builtin_amdgcn_permlane16_swap(lo[h], lo[h], false, false);
    const auto h2 = __builtin_amdgcn_permlane16_swap(hi[h], hi[h], false, false);
    o[2 * h] = __hiloint2double(h2[0], l2[0]);
    o[2 * h + 1] = __hiloint2double(h2[1], l2[1]);
  }
}

// A condition that is the same in every lane by the algorithm but not by the compiler's analysis, as a wave-uniform value: the branch on
// it is a scalar branch (s_cbranch_scc), not an EXEC-masked region.  Used by the sweeps of the W > 1 kernels (inlined into a kernel whose
// wavefronts take different paths; measured there: B = 256 / 512 kernel 2.95 / 3.10 ms against 3.01 / 3.15 ms); the sweep W = 1 calls as a
// function keeps the per-lane form (all-or-none masks in uniform control flow, gated by the same tests: the scalar form costs it 1.6 %,
// 14.55 against 14.33 ms -- profiles/r04/README.md; the switch that forced one form everywhere is in the history at 2373201).
template <bool ON>
__device__ inline bool uniform_if(bool c) {
  if constexpr (ON) return __builtin_amdgcn_readfirstlane((int)c) != 0;
  else return c;
}

// lane l <- lane l - 1 (lane 0: unspecified, the callers overwrite it)
__device__ inline double lane_up1(double v) { return __shfl_up(v, 1, 64); }

}  // namespace myriad
