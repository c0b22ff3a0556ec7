// fit_gn.h -- trajectory-matching loss, its gradient and its Gauss-Newton matrix in the model parameters (K9g in DESIGN.md).
// The loss of fit.h is a weighted nonlinear least-squares problem in very few unknowns: with the residuals r_t = xh_t - xs_obs_t and the forward
// sensitivities S_t = d xh_t / d p [NS][NP] of the rolled-out states,
//   loss = sum_t wt[t] |r_t|^2,   grad = 2 sum_t wt[t] S_t^T r_t,   gn = 2 sum_t wt[t] S_t^T S_t      (t = 1..num_steps: xh_0 = xs_obs_0 is data)
// so that loss(p + d) = loss + grad . d + d . gn d / 2 to second order in d for small residuals: the matrix a Gauss-Newton / Levenberg-Marquardt
// step solves with, and the Fisher information of the fit.  S rides along with the state in ONE forward pass -- nothing is stored per step, where
// fit.h's reverse sweep keeps the whole state trajectory.  One trajectory per lane; host/device shared.  No call site in the reference.
#pragma once
#include "fit.h"

namespace myriad {

template <class Sys>
struct FitGnLane {
  static constexpr int NS = Sys::NS, NU = Sys::NU, NP = Sys::NP;
  static constexpr int NT = NP * (NP + 1) / 2;      // entries of the upper triangle
  static constexpr int NG = NP + NP * NP;           // doubles of one result row: grad, then gn

  // dK <- A(X, U) (S + c dK) + P(X, U), A = df/dx (Sys::lin), P = df/dp: the sensitivity of the stage derivative at the stage point X whose own
  // sensitivity is S + c dK (dK: that of the stage before; c = 0 for the first stage).  Column by column, so that dK is replaced in place; row i of P
  // is vjp_p with the unit cotangent e_i -- a constant once this is inlined: the generated sums fold to that row.
  MYR_HD static inline void dstage(const double* X, const double* U, const double* p, const double (*S)[NP], double c, double (*dK)[NP]) {
    double fo[NS], A[NS * NS], Bm[NS * NU], go, gw[NS + NU];
    Sys::lin(X, U, p, fo, A, Bm, &go, gw);
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      double col[NS], out[NS];
#pragma unroll
      for (int i = 0; i < NS; ++i) col[i] = S[i][k] + c * dK[i][k];
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < NS; ++q) t += A[i * NS + q] * col[q];
        out[i] = t;
      }
#pragma unroll
      for (int i = 0; i < NS; ++i) dK[i][k] = out[i];
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      double e[NS], row[NP];
#pragma unroll
      for (int q = 0; q < NS; ++q) e[q] = q == i ? 1.0 : 0.0;
      SysDp<Sys>::vjp_p(X, U, p, e, row);
#pragma unroll
      for (int k = 0; k < NP; ++k) dK[i][k] += row[k];
    }
  }

  // xs_obs, us, wt, p: as FitLane::run.  Returns the loss; gp[NP] receives the gradient (want_grad; the same for every lane of a launch) and
  // gu[NT] the upper triangle of gn, row by row ((k, l), k <= l, at k NP - k (k - 1) / 2 + l - k).  The state advances in the arithmetic of
  // FitLane::stages<true>, which is Rollout<Sys>::run's, and the loss is summed as FitLane::run sums it (on the host: the same bits).
  MYR_HD static double run(int method, int num_steps, double h, int u_rows, const double* xs_obs, const double* us, const double* wt,
                           const double* p, double* gp, double* gu, bool want_grad = true) {
    double x[NS], X[4][NS], Uc[4][NU];
    double S[NS][NP], dK[NS][NP], acc[NS][NP];      // the three live blocks: S, the stage sensitivity, sum_j bw[j] dK_j
    double loss = 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      x[i] = xs_obs[i];
#pragma unroll
      for (int k = 0; k < NP; ++k) S[i][k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) gp[k] = 0.0;
#pragma unroll
    for (int k = 0; k < NT; ++k) gu[k] = 0.0;
    double av[4], bv[4];      // (fit.h: fit_stage_weights)
    fit_stage_weights(method, av, bv);
    for (int s = 0; s < num_steps; ++s) {
      const int nst = FitLane<Sys>::template stages<true>(method, s, h, u_rows, us, p, x, X, Uc);
#pragma unroll
      for (int i = 0; i < NS; ++i) {
#pragma unroll
        for (int k = 0; k < NP; ++k) { dK[i][k] = 0.0; acc[i][k] = 0.0; }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < nst) {                                      // (the same for every lane: the method is a kernel argument)
          dstage(X[j], Uc[j], p, S, (j == 0 ? 0.0 : av[j - 1]) * h, dK);      // (stage point j was made from stage j - 1)
#pragma unroll
          for (int i = 0; i < NS; ++i) {
#pragma unroll
            for (int k = 0; k < NP; ++k) acc[i][k] += bv[j] * dK[i][k];
          }
        }
      }
#pragma unroll
      for (int i = 0; i < NS; ++i) {
#pragma unroll
        for (int k = 0; k < NP; ++k) S[i][k] += h * acc[i][k];
      }
      const double w = wt ? wt[s + 1] : 1.0;
      double r[NS], e = 0.0;
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        r[i] = x[i] - xs_obs[(long)(s + 1) * NS + i];
        e += r[i] * r[i];
      }
      loss += w * e;
      const double w2 = 2.0 * w;
      if (want_grad) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          double t = 0.0;
#pragma unroll
          for (int i = 0; i < NS; ++i) t += S[i][k] * r[i];
          gp[k] += w2 * t;
        }
      }
      int m = 0;
#pragma unroll
      for (int k = 0; k < NP; ++k) {
#pragma unroll
        for (int l = k; l < NP; ++l, ++m) {
          double t = 0.0;
#pragma unroll
          for (int i = 0; i < NS; ++i) t += S[i][k] * S[i][l];
          gu[m] += w2 * t;
        }
      }
    }
    return loss;
  }

  // gn [NP][NP] from its upper triangle: both halves from the same accumulator, so gn is symmetric to the bit
  MYR_HD static inline void mirror(const double* gu, double* gn) {
    int m = 0;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
#pragma unroll
      for (int l = k; l < NP; ++l, ++m) {
        gn[k * NP + l] = gu[m];
        gn[l * NP + k] = gu[m];
      }
    }
  }
};

#if defined(__HIPCC__)
// One trajectory per lane, with the lane / set / data addressing of fit_lane_kernel: lane b is trajectory b mod R of parameter set b / R, reads
// parameter row b / pdiv and the data of trajectory b (of b mod R with data_shared); set boundaries fall inside wavefronts, and the lanes of the last
// wavefront that have no trajectory redo the last one with masked stores -- no other branch depends on the lane.  No scratch: the lane keeps S in
// registers.  Results: loss [B] or null; grad, row b at grad + b * grad_ld (null: not formed), and gn, row b [NP][NP] at gn + b * gn_ld.  The host
// passes grad_ld = NP, gn_ld = NP * NP for the caller's own arrays, and grad = rows, gn = rows + NP, grad_ld = gn_ld = NP + NP * NP for the packed
// rows one fit_reduce_sets_kernel launch sums.
template <class Sys>
__global__ __launch_bounds__(64)
void fit_gn_lane_kernel(int B, int R, int pdiv, int data_shared, int method, int num_steps, double h, int u_rows,
                        const double* __restrict__ xs_obs, const double* __restrict__ us, const double* __restrict__ wt,
                        const double* __restrict__ params, double* __restrict__ loss, double* __restrict__ grad, long grad_ld,
                        double* __restrict__ gn, long gn_ld) {
  using L = FitGnLane<Sys>;
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const FitLaneAddr at(b, B, R, pdiv, data_shared);
  SysParams<Sys> pp;
  pp.load(params, at.prow, Sys::NP);
  double gp[L::NP], gu[L::NT];
  const double l = L::run(method, num_steps, h, u_rows, xs_obs + at.d * (long)(num_steps + 1) * Sys::NS, us + at.d * (long)u_rows * Sys::NU, wt,
                          pp.get(), gp, gu, grad != nullptr);
  if (at.live) {
    if (loss) loss[b] = l;
    if (grad) {
#pragma unroll
      for (int k = 0; k < L::NP; ++k) grad[b * grad_ld + k] = gp[k];
    }
    L::mirror(gu, gn + b * gn_ld);
  }
}
#endif  // __HIPCC__

}  // namespace myriad
