// riccati_tile.h -- the 16x16 matrix-core tile that carries ONE Riccati stage (one control, NS <= 4), written once for the five
// sweeps that run on it: HsWave::riccati_mfma / riccati_mfma_trap (hs_solver_wave.h), HsFused::riccati_tile / riccati_tile_trap
// (hs_solver_fused.h: plain sweep and two-level chunk) and ShootWave::riccati_mfma (shoot_solver_wave.h).
// Forced-inline device code on values: the slot map, the 0/1 lane factors, the products of a stage, the gain rules and the epilogue.  What a sweep reads
// and in which order -- its records and streams, the loop over the stages, the prefetch ring and its refill position, what an abort does -- stays with it.
#pragma once
#include <hip/hip_runtime.h>
#include "wave_prims.h"

namespace myriad {

typedef double mfma_d4 __attribute__((ext_vector_type(4)));
#define MYR_TILE_FN __device__ __forceinline__

MYR_TILE_FN mfma_d4 tile_mfma(double a, double b, mfma_d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// ---- the stage on v_mfma_f64_16x16x4_f64 ------------------------------------------------------------------------------
// The stage update is three small dense products,
//     R~      = P' [Ge^ | ge^] + [0 | pc']                          (NW x (NY+NC))
//     [Q|qc]  = [Qm | qcm] + Ge^^T R~                               (NY x (NY+NC))
//     [P|pc]  = [Qss | qc_s] - Qsq (Qqq^-1 [Qqs | qc_q])            (NW x (NW+NC))   (+ the dual bookkeeping rows)
// and one 16x16 matrix-core tile holds all of a stage: the SAME slot placement is used for rows and for columns,
//     0..3 dx_s | 4,5 du_s (twice) | 6 rhs "1" (where ge enters) | 7 rhs mu | 8,9 du_e (twice) | 10,11,14,15 rhs nu_1..4 |
//     12,13 du_m (twice),
// chosen for the register layout of the instruction (A[i][k] and B[k][j] one value per lane at lane 16k+i / 16k+j; C/D
// element (i,j) at lane 16 (i%4) + j, register i/4 -- probed on the hardware, tools/dev/mfma/probe_f64.hip):
//   * rows 0..3 of a result (register 0) ARE the B operand of the next product, and, P and Q being symmetric, also its A
//     operand: the three products chain without any data movement between lanes;
//   * the rows of the two eliminated controls du_m (12,13) and du_e (8,9) share lanes (registers 3 and 2 of lane groups
//     0 and 1), so every column's gain is a per-lane 2x2 solve; keeping du_s, du_m, du_e TWICE gives lane groups 0 and 1
//     each their own copy, which is exactly where the rank-2 update wants its two K-slots;
//   * the dual bookkeeping Tnu (the rows ge^T pc' and -qc_q^T kc of HsWave::riccati()) falls out of the same instructions as
//     extra result rows (6 and 10,11,14,15) that are otherwise unused.
// Hermite-Simpson (HS): five products a stage, two eliminated controls.  The three-product forms (trapezoidal, shooting): one
// eliminated control du_e, slots 12, 13 unused.
// A lane is g = lane >> 4 (its register-0 row; a state row while g < NS) and j = lane & 15 (its slot).  What slot j stands for:
template <int NS>
MYR_TILE_FN int tile_scol(int j) { return j < 4 ? (j < NS ? j : -1) : (j < 6 ? NS : -1); }                 // index into s = (dx, du), or -1
template <int NS, bool HS>
MYR_TILE_FN int tile_ycol(int j, int scol) {                                                                // ... into the stage unknowns y
  if constexpr (HS) return scol >= 0 ? scol : ((j == 12 || j == 13) ? NS + 1 : ((j == 8 || j == 9) ? NS + 2 : -1));
  else return scol >= 0 ? scol : ((j == 8 || j == 9) ? NS + 1 : -1);
}
template <int NC>
MYR_TILE_FN int tile_rcc(int j) {                                                                           // ... as a right-hand-side column
  const int cc = j == 6 ? 0 : (j == 7 ? 1 : (j == 10 ? 2 : (j == 11 ? 3 : (j == 14 ? 4 : (j == 15 ? 5 : -1)))));
  return (cc >= 0 && cc < NC) ? cc : -1;
}
// (Plain functions of values, not a record of the lane built in one place: behind a struct the out-of-line sweeps of HsFused compile to other
// code.  The terminal seed and the gain address are not here at all: as functions they changed the code of every sweep that used them, so each
// sweep writes those few lines out -- profiles/r12_riccati_tile/README.md.)

// Lane selections are per-lane 0/1 factors folded into multiply-adds (one fp64 instruction instead of two 32-bit
// selects plus an add).  A factor 0 meets only finite values: the unused rows / columns of the tile hold finite
// combinations of the inputs (if an input is not finite the solve is reported NAN anyway).
// CHUNK (level 1 of the two-level sweep): row 7 -- the control's multiplier -- is carried like row 6 and takes the rank
// update like the rows nu_x.
template <bool CHUNK, bool HS>
struct TileMask {
  double f_a1;               // A operand of the R~ products: P' / H_m columns
  double f_keep;             // C operand: the right-hand-side columns pass
  double f_she, f_shm;       // selector columns du_e, du_m
  double f_x1, f_t1, f_t23;  // rows of registers 1..3
  double f_a3m, f_a3e;       // A operand of the rank update: lane group 0 (du_m; the only one of the three-product forms), 1 (du_e)
  MYR_TILE_FN TileMask(int g, int j, int rcc) {
    f_a1 = j < 6 ? 1.0 : 0.0;
    f_keep = rcc >= 0 ? 1.0 : 0.0;
    f_she = (j == 8 || j == 9) ? 1.0 : 0.0; f_shm = (j == 12 || j == 13) ? 1.0 : 0.0;
    f_x1 = g < 2 ? 1.0 : 0.0; f_t1 = (CHUNK ? g >= 2 : g == 2) ? 1.0 : 0.0; f_t23 = g >= 2 ? 1.0 : 0.0;
    // (the column test is written out in both forms: the compiler lowers it with the test on g around it)
    if constexpr (HS) {
      const bool a3_on = g < 2 && (j < 6 || (CHUNK && j == 7) || j == 10 || j == 11 || j == 14 || j == 15);
      f_a3m = (a3_on && g == 0) ? -1.0 : 0.0; f_a3e = (a3_on && g == 1) ? -1.0 : 0.0;
    } else {
      f_a3m = (g == 0 && (j < 6 || (CHUNK && j == 7) || j == 10 || j == 11 || j == 14 || j == 15)) ? -1.0 : 0.0; f_a3e = 0.0;
    }
  }
};

// First product of a pair, R = X [G | g] + [0 | x_c]: the selector row of G (SHR = 4: du_e, factor f_she; SHR = 8: du_m, f_shm)
// is the shifted column du of X.  `C`: the upper half of the C operand (zero; HsFused passes the previous result, whose upper
// half is zero and stays zero).
template <int SHR>
MYR_TILE_FN mfma_d4 tile_prod1(double X0, double X1, double G, double f_a1, double f_keep, double f_sh, mfma_d4 C) {
  static_assert(SHR == 4 || SHR == 8, "du_e or du_m");
  double sh0, sh1;
  if constexpr (SHR == 4) { sh0 = dpp_row_shr4(X0); sh1 = dpp_row_shr4(X1); }
  else { sh0 = dpp_row_shr8(X0); sh1 = dpp_row_shr8(X1); }
  C[0] = fma(sh0, f_sh, X0 * f_keep);
  C[1] = fma(sh1, f_sh, X1 * f_keep);
  return tile_mfma(X0 * f_a1, G, C);
}

// C operand of [Q | qc] = Qm^ + Ge^^T R~ (Hermite-Simpson; selector row: the du_e rows take R~'s row du); rows 6, 10.. carry Tnu
MYR_TILE_FN mfma_d4 tile_c2_hs(const mfma_d4& D3, const mfma_d4& D1, const mfma_d4& Qm, double f_t1, double f_t23) {
  mfma_d4 C2;
  C2[0] = Qm[0]; C2[1] = fma(D3[1], f_t1, Qm[1]); C2[2] = fma(D3[2], f_t23, Qm[2]) + D1[1]; C2[3] = fma(D3[3], f_t23, Qm[3]);
  return C2;
}

// The end-point part of a three-product stage (trapezoidal, shooting) behind (a) X = previous result + own terms, which is the
// caller's: (b) R~ = X [G | g] + [0 | x_c], (c) [Q | qc] = G^T R~ -- plus, EXTRA, the full step Hessian H0..H2 (rows dx, du,
// du_next) of the shooting form in the C operand.
struct TileEnd { mfma_d4 D1, D2; };
template <bool EXTRA>
MYR_TILE_FN TileEnd tile_end_part(const mfma_d4& D3, double X0, double X1, double G, double f_a1, double f_keep, double f_she, double f_t1, double f_t23,
                                  double H0 = 0.0, double H1 = 0.0, double H2 = 0.0) {
  TileEnd r;
  r.D1 = tile_prod1<4>(X0, X1, G, f_a1, f_keep, f_she, mfma_d4{0.0, 0.0, 0.0, 0.0});
  mfma_d4 C2;
  if constexpr (EXTRA) { C2[0] = H0; C2[1] = fma(D3[1], f_t1, H1); C2[2] = fma(D3[2], f_t23, r.D1[1]) + H2; C2[3] = D3[3] * f_t23; }
  else { C2[0] = 0.0; C2[1] = D3[1] * f_t1; C2[2] = fma(D3[2], f_t23, r.D1[1]); C2[3] = D3[3] * f_t23; }
  r.D2 = tile_mfma(G, r.D1[0], C2);
  return r;
}

// This column's gains [K | kc] = Qqq^-1 [Qqs | qc_q] of a Hermite-Simpson stage.  Pivots of the L D L^T of Qqq as in ldl_reg:
// d0 = q00, d1 = q11 - q10^2 / q00 = det / q00, both required > reg_floor.  When they are (always, except inside the inertia
// correction's probing), the 2x2 solve is Cramer's rule with ONE reciprocal, 1 / det, whose dependent chain (product, fma,
// rcp + Newton, product) is a third of the factor-and-substitute one; the numerators do not depend on it.
// The pivot test is wave-uniform -- the pivots come from v_readlane -- but the compiler sees per-lane values.  UNIFORM: decided in
// the vector unit and made a SCALAR branch through readfirstlane, so that no matrix instruction of the sweep around it sits inside
// an EXEC-masked region (v_mfma does not honour EXEC on this part, tools/dev/litmus/mfma_exec.hip).  nreg counts the regularised
// pivots; stop() is asked once they are counted, true leaves at once (`stop` set, gains undefined).
struct TileGain2 { double kk0, kk1; bool stop; };
template <bool UNIFORM, class Stop>
MYR_TILE_FN TileGain2 tile_gain2(const mfma_d4& D2, double reg_floor, int& nreg, Stop stop) {
  const double q00 = rdlane(D2[3], 12), q10 = rdlane(D2[2], 12), q11 = rdlane(D2[2], 8);
  const double det = fma(q00, q11, -(q10 * q10));
  const double rdet = fast_rcp(det);
  const double b0 = D2[3], b1 = D2[2];
  double kk0 = fma(q11, b0, -(q10 * b1)) * rdet;
  double kk1 = fma(q00, b1, -(q10 * b0)) * rdet;
  const bool rare_ = !(q00 > reg_floor) || !(det > reg_floor * q00);
  if (uniform_if<UNIFORM>(rare_)) {                                       // rare
    const double u00 = q00, u10 = q10, u11 = q11;
    double d0 = u00;
    if (!(d0 > reg_floor)) { d0 = detail::dmax(fabs(d0), reg_floor); ++nreg; }
    const double i0 = fast_rcp(d0);
    const double l10 = u10 * i0;
    double d1 = u11 - l10 * l10 * d0;
    if (!(d1 > reg_floor)) { d1 = detail::dmax(fabs(d1), reg_floor); ++nreg; }
    if (stop()) return {kk0, kk1, true};
    const double i1 = fast_rcp(d1);
    kk0 = b0; kk1 = b1;
    kk1 -= l10 * kk0;
    kk0 *= i0; kk1 *= i1;
    kk0 -= l10 * kk1;
  }
  return {kk0, kk1, false};
}
// ... of a three-product stage: the single pivot Q[du_e][du_e], read from lane 8 of register 2 (same pivot rule as chol_reg)
struct TileGain1 { double kk; bool stop; };
template <bool UNIFORM, class Stop>
MYR_TILE_FN TileGain1 tile_gain1(const mfma_d4& D2, double reg_floor, int& nreg, Stop stop) {
  const double q11 = rdlane(D2[2], 8);
  double d = q11;
  const bool rare_ = !(d > reg_floor);
  if (uniform_if<UNIFORM>(rare_)) {                                       // rare
    d = detail::dmax(fabs(d), reg_floor); ++nreg;
    if (stop()) return {0.0, true};
  }
  return {D2[2] * fast_rcp(d), false};
}
struct TileNoStop { MYR_TILE_FN bool operator()() const { return false; } };

// [P | pc] = [Qss | qc_s] - Qsq [K | kc]; rows 10, 11, 14, 15: Tnu -= qc_q[:, nu]^T kc.  Rank 2 (Hermite-Simpson), rank 1.
MYR_TILE_FN mfma_d4 tile_update2(const mfma_d4& D2, double kk0, double kk1, double f_a3m, double f_a3e, int g) {
  const double A3 = fma(D2[3], f_a3m, D2[2] * f_a3e);
  const double B3 = g == 0 ? kk0 : (g == 1 ? kk1 : 0.0);     // (a select: groups 2, 3 may hold non-finite junk)
  return tile_mfma(A3, B3, D2);
}
MYR_TILE_FN mfma_d4 tile_update1(const mfma_d4& D2, double kk, double f_a3, int g) {
  const double A3 = D2[2] * f_a3;
  const double B3 = g == 0 ? kk : 0.0;
  return tile_mfma(A3, B3, D2);
}

// Epilogue: hand P | pc | Tnu of the last result (rows 0..5 [P | pc], rows 6, 10, 11, 14, 15 Tnu) to the first point (layouts of
// HsWave::riccati()), or -- CHUNK -- the chunk's P | pc | T to tl_join: T has the rows nu_x (NS), then the row of nu_u (row 7).
// X1 is read in group 0 only, the T rows in groups 2, 3 only.
template <bool CHUNK, int NS, int NC, class Ptr, class Sync>
MYR_TILE_FN void tile_store_first(const mfma_d4& D3, int g, int j, int scol, int rcc, bool rowx, Ptr sP, Ptr sPc, Ptr sTnu, Sync sync) {
  constexpr int NW = NS + 1;
  const double X0 = D3[0], X1 = D3[1], T1 = D3[1], T2 = D3[2], T3 = D3[3];
  if (scol >= 0 && j != 5) {
    if (rowx) sP[g * NW + scol] = X0;
    if (g == 0) sP[NS * NW + scol] = X1;
  }
  if (rcc >= 0) {
    if (rowx) sPc[g * NC + rcc] = X0;
    if (g == 0) sPc[NS * NC + rcc] = X1;
    if (g >= 2 && g - 2 < NS) sTnu[(g - 2) * NC + rcc] = T2;
    if (g >= 2 && g < NS) sTnu[g * NC + rcc] = T3;
    if constexpr (CHUNK) { if (g == 3) sTnu[NS * NC + rcc] = T1; }
  }
  sync();
  // row 6: ge^T pc'[:, nu_i], summed over the stages -- the part of T[nu_m]["1"] that the products leave in row "1"
  if (g == 2 && rcc >= 2) sTnu[(rcc - 2) * NC + 0] += T1;
  if constexpr (CHUNK) { if (g == 2 && rcc == 1) sTnu[NS * NC + 0] += T1; }
  sync();
}

#undef MYR_TILE_FN

}  // namespace myriad
