// fit.h -- trajectory-matching loss and its gradient in the model parameters (K9 in DESIGN.md).
// Restates the reference's myriad/experiments/mle_sysid.py:89-136 (the loss whose jax.grad it descends): integrate the
// recorded controls from the recorded start state with the fixed-step rules of rollout.h (utils.py:80-131; quirks Q5, Q6, Q11), take
//   l = sum_{t=0..S} wt[t] sum_i (xh[t][i] - xs_obs[t][i])^2,
// and push the cotangent back through the steps: a forward rollout that keeps the states, then one reverse sweep that recomputes the
// stage points of each step from its stored state.  One trajectory per lane; host/device shared.
#pragma once
#include "systems_gen.h"
#include "systems_dp_gen.h"
#if defined(__HIPCC__)
#include "node_system.h"
#include "node_mfma.h"
#endif

namespace myriad {

// The fixed-step rules, by `method` (0 Euler, 1 Heun, 2 midpoint, 3 RK4).  Every rule is X[0] = x, X[j+1] = x + a[j] h f(X[j], Uc[j]) and
// x+ = x + h sum_j bw[j] f(X[j], Uc[j]):
//   Euler     1 stage,  bw = {1}
//   Heun      2 stages, a = {1}, bw = {1/2, 1/2}, controls u_s, u_{s+1}
//   midpoint  2 stages, a = {1}, bw = {0, 1},     controls u_s, (u_s + u_{s+1}) / 2      (a full Euler predictor: Q11)
//   RK4       4 stages, a = {1/2, 1/2, 1}, bw = {1/6, 1/3, 1/3, 1/6}, controls u_{2s}, u_{2s+1}, u_{2s+1}, u_{2s+2}   (Q5)
// fit_stage_weights(method, a, bw) is that table as numbers, for the sweeps that differentiate a step (FitLane::run, FitGnLane::run; NodeFit::plan
// keeps a copy): a[j] is the weight of stage j in the NEXT stage point X[j+1], bw[j] its weight in the step (four entries each: those from the last
// stage on are not read; the number of stages is what FitLane::stages returns).  It writes the caller's arrays entry by entry and is always inlined:
// so the callers' device code is that of the table written out in place (a table returned by value, or filled by a constructor, or a stage count
// returned beside it, changed fit_lane_kernel and fit_gn_lane_kernel).
MYR_HD inline __attribute__((always_inline)) void fit_stage_weights(int method, double* a, double* bw) {
  a[0] = method == 3 ? 0.5 : 1.0; a[1] = 0.5; a[2] = 1.0; a[3] = 0.0;
  bw[0] = method == 0 ? 1.0 : (method == 1 ? 0.5 : (method == 2 ? 0.0 : 1.0 / 6.0));
  bw[1] = method == 1 ? 0.5 : (method == 2 ? 1.0 : 1.0 / 3.0); bw[2] = 1.0 / 3.0; bw[3] = 1.0 / 6.0;
}

template <class Sys>
struct FitLane {
  static constexpr int NS = Sys::NS, NU = Sys::NU, NP = Sys::NP;

  // Stage points X[j] and controls Uc[j] of step s from its state x, by the table above fit_stage_weights.
  // With NEXT the state after the step replaces x, in the arithmetic of Rollout<Sys>::run.  Returns the number of stages.
  template <bool NEXT>
  MYR_HD static inline int stages(int method, int s, double h, int u_rows, const double* us, const double* p, double* x,
                                  double (*X)[NS], double (*Uc)[NU]) {
    auto U = [&](int i) { return us + (long)(i < u_rows ? i : u_rows - 1) * NU; };
    double k1[NS], k2[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) X[0][i] = x[i];
    if (method == 0) {
#pragma unroll
      for (int c = 0; c < NU; ++c) Uc[0][c] = U(s)[c];
      if constexpr (NEXT) {
        Sys::f(X[0], Uc[0], p, k1);
#pragma unroll
        for (int i = 0; i < NS; ++i) x[i] += h * k1[i];
      }
      return 1;
    }
    if (method == 1 || method == 2) {
#pragma unroll
      for (int c = 0; c < NU; ++c) {
        Uc[0][c] = U(s)[c];
        Uc[1][c] = method == 1 ? U(s + 1)[c] : 0.5 * (U(s)[c] + U(s + 1)[c]);
      }
      Sys::f(X[0], Uc[0], p, k1);
#pragma unroll
      for (int i = 0; i < NS; ++i) X[1][i] = x[i] + h * k1[i];
      if constexpr (NEXT) {
        Sys::f(X[1], Uc[1], p, k2);
        if (method == 1) {
#pragma unroll
          for (int i = 0; i < NS; ++i) x[i] += 0.5 * h * (k1[i] + k2[i]);
        } else {
#pragma unroll
          for (int i = 0; i < NS; ++i) x[i] += h * k2[i];
        }
      }
      return 2;
    }
    double k3[NS], k4[NS];
#pragma unroll
    for (int c = 0; c < NU; ++c) {
      Uc[0][c] = U(2 * s)[c];
      Uc[1][c] = U(2 * s + 1)[c];
      Uc[2][c] = U(2 * s + 1)[c];
      Uc[3][c] = U(2 * s + 2)[c];
    }
    Sys::f(X[0], Uc[0], p, k1);
#pragma unroll
    for (int i = 0; i < NS; ++i) X[1][i] = x[i] + 0.5 * h * k1[i];
    Sys::f(X[1], Uc[1], p, k2);
#pragma unroll
    for (int i = 0; i < NS; ++i) X[2][i] = x[i] + 0.5 * h * k2[i];
    Sys::f(X[2], Uc[2], p, k3);
#pragma unroll
    for (int i = 0; i < NS; ++i) X[3][i] = x[i] + h * k3[i];
    if constexpr (NEXT) {
      Sys::f(X[3], Uc[3], p, k4);
#pragma unroll
      for (int i = 0; i < NS; ++i) x[i] += h / 6.0 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
    }
    return 4;
  }

  // xs_obs: [num_steps+1][NS] and us: [u_rows][NU] of this trajectory; wt: [num_steps+1] or null (= 1); p: the lane's parameter buffer.
  // xh: this lane's column of the state scratch, entry (t, i) at xh[(t * NS + i) * ld] (ld = padded batch on the device, 1 on the host).
  // gp[NP] receives dl/dp; returns l.  want_grad == false (the same for every lane of a launch): the loss only, the reverse sweep is not run and
  // gp is not written.
  MYR_HD static double run(int method, int num_steps, double h, int u_rows, const double* xs_obs, const double* us, const double* wt,
                           const double* p, double* xh, long ld, double* gp, bool want_grad = true) {
    double x[NS], X[4][NS], Uc[4][NU], lam[NS];
    double loss = 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      x[i] = xs_obs[i];
      xh[(long)i * ld] = x[i];
    }
    for (int s = 0; s < num_steps; ++s) {                     // forward: xh[0] = xs_obs[0] adds nothing to the loss
      stages<true>(method, s, h, u_rows, us, p, x, X, Uc);
      const double w = wt ? wt[s + 1] : 1.0;
      double e = 0.0;
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        xh[((long)(s + 1) * NS + i) * ld] = x[i];
        const double d = x[i] - xs_obs[(long)(s + 1) * NS + i];
        e += d * d;
      }
      loss += w * e;
    }
    if (!want_grad) return loss;
#pragma unroll
    for (int k = 0; k < NP; ++k) gp[k] = 0.0;
    {
      const double w = wt ? wt[num_steps] : 1.0;
#pragma unroll
      for (int i = 0; i < NS; ++i) lam[i] = 2.0 * w * (x[i] - xs_obs[(long)num_steps * NS + i]);
    }
    for (int s = num_steps - 1; s >= 0; --s) {                // reverse: lam_s = (d step / d x)^T lam_{s+1} + 2 wt[s] (xh_s - xs_obs_s)
#pragma unroll
      for (int i = 0; i < NS; ++i) x[i] = xh[((long)s * NS + i) * ld];
      const int nst = stages<false>(method, s, h, u_rows, us, p, x, X, Uc);
      double av[4], bv[4];
      fit_stage_weights(method, av, bv);
      double wx[NS], acc[NS];                                 // wx: cotangent of the stage point behind the current one
#pragma unroll
      for (int i = 0; i < NS; ++i) { wx[i] = 0.0; acc[i] = 0.0; }
#pragma unroll
      for (int j = 3; j >= 0; --j) {
        if (j < nst) {                                        // (the same for every lane: the method is a kernel argument)
          double v[NS], fo[NS], A[NS * NS], Bm[NS * NU], go, gw[NS + NU], gs[NP];
#pragma unroll
          for (int i = 0; i < NS; ++i) v[i] = bv[j] * h * lam[i] + av[j] * h * wx[i];
          Sys::lin(X[j], Uc[j], p, fo, A, Bm, &go, gw);
          SysDp<Sys>::vjp_p(X[j], Uc[j], p, v, gs);
#pragma unroll
          for (int k = 0; k < NP; ++k) gp[k] += gs[k];
#pragma unroll
          for (int c = 0; c < NS; ++c) {
            double t = 0.0;
#pragma unroll
            for (int i = 0; i < NS; ++i) t += A[i * NS + c] * v[i];
            wx[c] = t;
            acc[c] += t;
          }
        }
      }
      const double w = wt ? wt[s] : 1.0;
#pragma unroll
      for (int i = 0; i < NS; ++i) lam[i] += acc[i] + 2.0 * w * (x[i] - xs_obs[(long)s * NS + i]);
    }
    return loss;
  }
};

#if defined(__HIPCC__)
// Where lane b of fit_lane_kernel / fit_gn_lane_kernel works (the rule is told below).  live: it has a trajectory of its own; t: the trajectory it
// runs (the last one where it has none); d, prow: the rows of its data and of its parameters
struct FitLaneAddr {
  bool live; long t, d, prow;
  __device__ FitLaneAddr(long b, int B, int R, int pdiv, int data_shared) {
    live = b < B;
    t = live ? b : (long)B - 1;
    d = data_shared ? t % R : t;
    prow = t / pdiv;
  }
};

// One trajectory per lane: lane b of the launch is trajectory b mod R of parameter set b / R (B = E R lanes; myr_fit_grad is one set).  It reads
// parameter row b / pdiv of `params` (pdiv = R: a row per set; pdiv = 1: a row per trajectory, myr_fit_grad with params_stride == np) and the data of
// trajectory b, or of b mod R where every set reads the same R trajectories (data_shared).  Set boundaries fall inside wavefronts: a lane's arithmetic
// depends on nothing but its own rows.  The lanes of the last wavefront that have no trajectory redo the last one, with its own set's parameters (the
// same loop trip counts and the same branches for the whole wavefront), in a scratch column of their own; their stores of the results are masked.
// grad == nullptr: the loss only.
template <class Sys>
__global__ __launch_bounds__(64)
void fit_lane_kernel(int B, int R, int pdiv, int data_shared, long Bp, int method, int num_steps, double h, int u_rows,
                     const double* __restrict__ xs_obs, const double* __restrict__ us, const double* __restrict__ wt,
                     const double* __restrict__ params, double* __restrict__ xh, double* __restrict__ loss, double* __restrict__ grad) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;      // < Bp: the scratch has a column for every lane of the grid
  const FitLaneAddr at(b, B, R, pdiv, data_shared);
  SysParams<Sys> pp;
  pp.load(params, at.prow, Sys::NP);
  double gp[Sys::NP];
  const double l = FitLane<Sys>::run(method, num_steps, h, u_rows, xs_obs + at.d * (long)(num_steps + 1) * Sys::NS, us + at.d * (long)u_rows * Sys::NU,
                                     wt, pp.get(), xh + b, Bp, gp, grad != nullptr);
  if (at.live) {
    if (loss) loss[b] = l;
    if (grad) {
#pragma unroll
      for (int k = 0; k < Sys::NP; ++k) grad[b * Sys::NP + k] = gp[k];
    }
  }
}

// The same loss and gradient for the network system (x' = MLP([x; u]), hidden (64, 64); neural_ode/node_training.py:31-61).  A lane cannot hold the
// 4 804 accumulators of the weight gradient, so ONE WAVEFRONT takes one trajectory and lane j is hidden unit j of both layers: the state, the
// cotangents and the stage points are wave-uniform, lane j keeps column j of dW1 and dW2, row j of dW3 and entry j of db1, db2.  The weights sit in
// LDS in the layout of NodeMfma64::load_weights (W2 padded to 65 columns: lane j reading column j and lane i reading row i are both free of bank
// conflicts); the WPB wavefronts (trajectories) of a workgroup share one copy.  Hidden activations travel between lanes by v_readlane, the four
// outputs and the four entries of A^T v are butterfly sums over the wavefront (every lane ends with the same bits).  No branch depends on the lane.
struct NodeFit {
  using NM = NodeMfma64;
  using Sys = SysNODE_CARTPOLE;
  static constexpr int NS = NM::NS, NU = NM::NU, NW = NM::NW, H = NM::H, NP = Sys::NP, WPB = 4;
  static_assert(Sys::O_W2 == NM::O_W2 && Sys::O_B3 == NM::O_B3 && NU == 1, "parameter order of node_system.h");

  __device__ static inline double bcast(double v, int k) {      // every lane <- lane k (k: wave-uniform)
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
  }
  __device__ static inline double wsum(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
  }
  __device__ static inline double sig(double a) { return 1.0 / (1.0 + exp(-a)); }

  // network at the wave-uniform point w = [x; u]: this lane's hidden activations and the output f[NS] (the same in every lane)
  __device__ static inline void fwd(const double* wl, int lane, const double* w, double& h1, double& h2, double* f) {
    double a = wl[NM::L_B1 + lane];
#pragma unroll
    for (int c = 0; c < NW; ++c) a += w[c] * wl[NM::L_W1 + c * H + lane];
    h1 = sig(a);
    a = wl[NM::L_B2 + lane];
#pragma unroll 8
    for (int i = 0; i < H; ++i) a += bcast(h1, i) * wl[NM::L_W2 + i * NM::LD2 + lane];
    h2 = sig(a);
#pragma unroll
    for (int r = 0; r < NS; ++r) f[r] = wl[NM::L_B3 + r] + wsum(h2 * wl[NM::L_W3 + lane * NS + r]);
  }

  // this lane's share of a direction v in the weights (node_fit_gnvp_kernel): column `lane` of V1 and V2, row `lane` of V3, entry `lane` of vb1 and
  // vb2, and vb3 -- Acc's shape, read instead of accumulated.  Registers for the whole forward pass, as Acc is for the reverse sweep
  struct Dir {
    double w1[NW], b1, w2[H], b2, w3[NS], b3[NS];
    __device__ inline void load(const double* v, int lane) {      // v [NP] in the parameter order of node_system.h
#pragma unroll
      for (int c = 0; c < NW; ++c) w1[c] = v[Sys::O_W1 + c * H + lane];
      b1 = v[Sys::O_B1 + lane];
#pragma unroll
      for (int k = 0; k < H; ++k) w2[k] = v[Sys::O_W2 + k * H + lane];
      b2 = v[Sys::O_B2 + lane];
#pragma unroll
      for (int r = 0; r < NS; ++r) { w3[r] = v[Sys::O_W3 + lane * NS + r]; b3[r] = v[Sys::O_B3 + r]; }
    }
  };

  // tangent of fwd at the point w = [x; u] with activations (h1, h2): input tangent [dx; 0], weight tangent d.  df[NS] = (df/dx) dx + (df/dp) v, the
  // same bits in every lane
  __device__ static inline void tan(const double* wl, int lane, const Dir& d, const double* w, const double* dx, double h1, double h2, double* df) {
    double a = d.b1;
#pragma unroll
    for (int c = 0; c < NS; ++c) a += dx[c] * wl[NM::L_W1 + c * H + lane];
#pragma unroll
    for (int c = 0; c < NW; ++c) a += w[c] * d.w1[c];
    const double t1 = h1 * (1.0 - h1) * a;
    a = d.b2;
#pragma unroll
    for (int i = 0; i < H; ++i) {                                // (unrolled: the direction is registers)
      a += bcast(t1, i) * wl[NM::L_W2 + i * NM::LD2 + lane];
      a += bcast(h1, i) * d.w2[i];
      if ((i & 7) == 7) __builtin_amdgcn_sched_barrier(0);       // (as in bwd: eight pairs of broadcasts in flight)
    }
    const double t2 = h2 * (1.0 - h2) * a;
#pragma unroll
    for (int r = 0; r < NS; ++r) df[r] = d.b3[r] + wsum(t2 * wl[NM::L_W3 + lane * NS + r] + h2 * d.w3[r]);
  }

  struct Acc {                // this lane's share of the weight gradient
    double w1[NW], b1, w2[H], b2, w3[NS], b3[NS];
  };

  // cotangent v[NS] of the output at the point w with activations (h1, h2): adds to the weight gradient, ax[NS] = (df/dx)^T v
  __device__ static inline void bwd(const double* wl, int lane, const double* w, double h1, double h2, const double* v, Acc& g, double* ax) {
    double g2 = 0.0;
#pragma unroll
    for (int r = 0; r < NS; ++r) {
      g.w3[r] += h2 * v[r];
      g.b3[r] += v[r];
      g2 += wl[NM::L_W3 + lane * NS + r] * v[r];
    }
    const double e2 = g2 * h2 * (1.0 - h2);
    g.b2 += e2;
    double g1 = 0.0;
#pragma unroll
    for (int k = 0; k < H; ++k) {                                // (unrolled: the accumulators are registers)
      g.w2[k] += bcast(h1, k) * e2;                              // dW2[k][lane]
      g1 += wl[NM::L_W2 + lane * NM::LD2 + k] * bcast(e2, k);    // row `lane` of W2
      if ((k & 7) == 7) __builtin_amdgcn_sched_barrier(0);       // eight broadcasts in flight, not sixty-four: they live in scalar registers
    }
    const double e1 = g1 * h1 * (1.0 - h1);
    g.b1 += e1;
#pragma unroll
    for (int c = 0; c < NW; ++c) g.w1[c] += w[c] * e1;
#pragma unroll
    for (int c = 0; c < NS; ++c) ax[c] = wsum(wl[NM::L_W1 + c * H + lane] * e1);
  }

  // stage controls and weights of step s.  The table of fit_stage_weights once more, in its index convention: a call of it here, in any of the forms
  // tried, changed node_fit_kernel's instruction sequence
  __device__ static inline int plan(int method, int s, int u_rows, const double* us, double* uc, double* av, double* bv) {
    auto U = [&](int i) { return us[i < u_rows ? i : u_rows - 1]; };
    av[0] = method == 3 ? 0.5 : 1.0; av[1] = 0.5; av[2] = 1.0; av[3] = 0.0;
    bv[0] = method == 0 ? 1.0 : (method == 1 ? 0.5 : (method == 2 ? 0.0 : 1.0 / 6.0));
    bv[1] = method == 1 ? 0.5 : (method == 2 ? 1.0 : 1.0 / 3.0); bv[2] = 1.0 / 3.0; bv[3] = 1.0 / 6.0;
    if (method == 3) { uc[0] = U(2 * s); uc[1] = U(2 * s + 1); uc[2] = uc[1]; uc[3] = U(2 * s + 2); return 4; }
    uc[0] = U(s);
    uc[1] = method == 1 ? U(s + 1) : 0.5 * (U(s) + U(s + 1));
    uc[2] = uc[1]; uc[3] = uc[1];
    return method == 0 ? 1 : 2;
  }
};

// E weight sets of R trajectories each (myr_fit_grad: E = 1).  grid: E * ceil(R / WPB) workgroups of WPB wavefronts -- workgroup g serves set
// g / ceil(R / WPB) alone, its LDS holds that set's weights, and its wavefront w takes row (g mod ceil(R / WPB)) WPB + w of the set.  params: [E][NP];
// xs_obs, us: a trajectory per (set, row), or per row where every set reads the same R trajectories (data_shared); xh: [num_steps+1][NS][Bp], column
// e R + r; loss [E][R] or null; grad: [E][R][NP] rows, or null: the loss only, the wavefront stops behind the forward rollout.  Every branch is
// wave-uniform.  (A template, so that only the object that launches it holds its code.)
template <class F>
__global__ __launch_bounds__(64 * F::WPB)
void node_fit_kernel(int R, int data_shared, long Bp, int method, int num_steps, double h, int u_rows, const double* __restrict__ xs_obs,
                     const double* __restrict__ us, const double* __restrict__ wt, const double* __restrict__ params,
                     double* __restrict__ xh, double* __restrict__ loss, double* __restrict__ grad) {
  constexpr int NS = F::NS, NW = F::NW, H = F::H;
  __shared__ double wl[NodeMfma64::L_N];
  const int gps = (R + F::WPB - 1) / F::WPB;                     // workgroups per set
  const int e = (int)(blockIdx.x / (unsigned)gps);
  NodeMfma64::load_weights(params + (long)e * F::NP, wl, threadIdx.x, 64 * F::WPB);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int r = (int)(blockIdx.x - (unsigned)e * (unsigned)gps) * F::WPB + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (r >= R) return;                                            // a whole wavefront, behind the only barrier
  const long b = (long)e * R + r;
  const long d = data_shared ? (long)r : b;
  const double* xo = xs_obs + d * (long)(num_steps + 1) * NS;
  const double* ub = us + d * (long)u_rows;
  double* xc = xh + b;
  // per wavefront and stage: the stage point [x; u] (every lane writes the same values) and the two activation vectors.  Written and read by the
  // same wavefront only: no barrier
  __shared__ double stg[F::WPB][4][8 + 2 * H];
  double (*st)[8 + 2 * H] = stg[__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))];
  double x[NS], w[NW], f[NS], uc[4], av[4], bv[4];
  double l = 0.0;
#pragma unroll
  for (int i = 0; i < NS; ++i) { x[i] = xo[i]; xc[(long)i * Bp] = x[i]; }      // (wave-uniform values: every lane stores)
  for (int s = 0; s < num_steps; ++s) {
    const int nst = F::plan(method, s, u_rows, ub, uc, av, bv);
    double ks[NS];                                               // sum_j bw[j] f(X[j]) in the arithmetic of Rollout<Sys>::run
#pragma unroll
    for (int i = 0; i < NS; ++i) { w[i] = x[i]; ks[i] = 0.0; }
#pragma unroll 1
    for (int j = 0; j < nst; ++j) {
      double h1, h2;
      w[NS] = uc[j];
      F::fwd(wl, lane, w, h1, h2, f);
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        ks[i] = j == 0 ? f[i] : (method == 2 ? f[i] : (method == 1 || j == 3 ? ks[i] + f[i] : ks[i] + 2.0 * f[i]));
        w[i] = x[i] + av[j] * h * f[i];
      }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) x[i] += (method == 1 ? 0.5 * h : (method == 3 ? h / 6.0 : h)) * ks[i];
    double e = 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      xc[((long)(s + 1) * NS + i) * Bp] = x[i];
      const double d = x[i] - xo[(long)(s + 1) * NS + i];
      e += d * d;
    }
    l += (wt ? wt[s + 1] : 1.0) * e;
  }
  if (!grad) {                                                   // (a kernel argument: the same for every wavefront)
    if (loss) loss[b] = l;
    return;
  }
  typename F::Acc g;
#pragma unroll
  for (int c = 0; c < NW; ++c) g.w1[c] = 0.0;
#pragma unroll
  for (int k = 0; k < H; ++k) g.w2[k] = 0.0;
#pragma unroll
  for (int r = 0; r < NS; ++r) { g.w3[r] = 0.0; g.b3[r] = 0.0; }
  g.b1 = 0.0; g.b2 = 0.0;
  double lam[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) lam[i] = 2.0 * (wt ? wt[num_steps] : 1.0) * (x[i] - xo[(long)num_steps * NS + i]);
  for (int s = num_steps - 1; s >= 0; --s) {
#pragma unroll
    for (int i = 0; i < NS; ++i) { x[i] = xc[((long)s * NS + i) * Bp]; w[i] = x[i]; }
    const int nst = F::plan(method, s, u_rows, ub, uc, av, bv);
#pragma unroll 1
    for (int j = 0; j < nst; ++j) {                              // the stage points and their activations, forward
      double h1, h2;
      w[NS] = uc[j];
      F::fwd(wl, lane, w, h1, h2, f);
#pragma unroll
      for (int c = 0; c < NW; ++c) st[j][c] = w[c];
      st[j][8 + lane] = h1;
      st[j][8 + H + lane] = h2;
#pragma unroll
      for (int i = 0; i < NS; ++i) w[i] = x[i] + av[j] * h * f[i];
    }
    double wx[NS], acc[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) { wx[i] = 0.0; acc[i] = 0.0; }
#pragma unroll 1
    for (int j = nst - 1; j >= 0; --j) {                         // the stage cotangents, backward
      double v[NS];
#pragma unroll
      for (int i = 0; i < NS; ++i) v[i] = bv[j] * h * lam[i] + av[j] * h * wx[i];
#pragma unroll
      for (int c = 0; c < NW; ++c) w[c] = st[j][c];
      F::bwd(wl, lane, w, st[j][8 + lane], st[j][8 + H + lane], v, g, wx);
#pragma unroll
      for (int i = 0; i < NS; ++i) acc[i] += wx[i];
    }
    const double ws = wt ? wt[s] : 1.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) lam[i] += acc[i] + 2.0 * ws * (x[i] - xo[(long)s * NS + i]);
  }
  if (loss) loss[b] = l;
  double* gr = grad + b * (long)F::NP;                           // the parameter order of node_system.h
  using S_ = typename F::Sys;
#pragma unroll
  for (int c = 0; c < NW; ++c) gr[S_::O_W1 + c * H + lane] = g.w1[c];
  gr[S_::O_B1 + lane] = g.b1;
#pragma unroll
  for (int k = 0; k < H; ++k) gr[S_::O_W2 + k * H + lane] = g.w2[k];
  gr[S_::O_B2 + lane] = g.b2;
#pragma unroll
  for (int r = 0; r < NS; ++r) { gr[S_::O_W3 + lane * NS + r] = g.w3[r]; gr[S_::O_B3 + r] = g.b3[r]; }
}

// Gauss-Newton product of the network fit (myr_fit_gnvp*; K9v in DESIGN.md): with S_b[t] = d xh_b[t] / d params, jv[b][t] = S_b[t] v and
// out[b] = 2 sum_t wt[t] S_b[t]^T S_b[t] v -- myr_fit_gn's gn[b] times v, without the 4 804 x 4 804 matrix.  node_fit_kernel's mapping (grid, sets,
// rows, LDS weights, one wavefront per trajectory, lane j = hidden unit j; every branch wave-uniform).  The forward pass carries the tangent dx = S v
// beside the state through the same stage table (F::tan; this lane's share of v sits in registers, F::Dir), keeps xh AND dx per step in column-major
// scratch (xh, dxh: [num_steps+1][NS][Bp] each) and writes dx to jv [E][R][num_steps+1][NS] when asked.  The reverse sweep is node_fit_kernel's with the
// cotangent source 2 wt[s] dx[s] where that one has 2 wt[s] (xh[s] - xs_obs[s]): a copy, not a shared function -- node_fit_kernel's instruction
// sequence is sensitive to how its body is cut up (see plan).  v: [E][NP], a direction per set.  out: [E][R][NP] rows, or null: the wavefront stops
// behind the forward pass.  xs_obs gives the start state only.
template <class F>
__global__ __launch_bounds__(64 * F::WPB)
void node_fit_gnvp_kernel(int R, int data_shared, long Bp, int method, int num_steps, double h, int u_rows, const double* __restrict__ xs_obs,
                          const double* __restrict__ us, const double* __restrict__ wt, const double* __restrict__ params,
                          const double* __restrict__ vdir, double* __restrict__ xh, double* __restrict__ dxh, double* __restrict__ jv,
                          double* __restrict__ out) {
  constexpr int NS = F::NS, NW = F::NW, H = F::H;
  __shared__ double wl[NodeMfma64::L_N];
  const int gps = (R + F::WPB - 1) / F::WPB;                     // workgroups per set
  const int e = (int)(blockIdx.x / (unsigned)gps);
  NodeMfma64::load_weights(params + (long)e * F::NP, wl, threadIdx.x, 64 * F::WPB);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int r = (int)(blockIdx.x - (unsigned)e * (unsigned)gps) * F::WPB + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (r >= R) return;                                            // a whole wavefront, behind the only barrier
  const long b = (long)e * R + r;
  const long d = data_shared ? (long)r : b;
  const double* xo = xs_obs + d * (long)(num_steps + 1) * NS;
  const double* ub = us + d * (long)u_rows;
  double* xc = xh + b;
  double* dc = dxh + b;
  double* jb = jv ? jv + b * (long)(num_steps + 1) * NS : nullptr;
  __shared__ double stg[F::WPB][4][8 + 2 * H];                   // (node_fit_kernel: per wavefront and stage, no barrier)
  double (*st)[8 + 2 * H] = stg[__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))];
  double x[NS], dx[NS], w[NW], f[NS], uc[4], av[4], bv[4];
  {
    typename F::Dir dir;                                         // live in the forward pass only
    dir.load(vdir + (long)e * F::NP, lane);
#pragma unroll
    for (int i = 0; i < NS; ++i) {                               // (wave-uniform values: every lane stores)
      x[i] = xo[i]; dx[i] = 0.0;
      xc[(long)i * Bp] = x[i]; dc[(long)i * Bp] = 0.0;
      if (jb) jb[i] = 0.0;
    }
    for (int s = 0; s < num_steps; ++s) {
      const int nst = F::plan(method, s, u_rows, ub, uc, av, bv);
      double ks[NS], dks[NS], dw[NS], df[NS];                    // ks, dks: sum_j bw[j] f(X[j]) and its tangent, in node_fit_kernel's arithmetic
#pragma unroll
      for (int i = 0; i < NS; ++i) { w[i] = x[i]; dw[i] = dx[i]; ks[i] = 0.0; dks[i] = 0.0; }
#pragma unroll 1
      for (int j = 0; j < nst; ++j) {
        double h1, h2;
        w[NS] = uc[j];
        F::fwd(wl, lane, w, h1, h2, f);
        F::tan(wl, lane, dir, w, dw, h1, h2, df);
#pragma unroll
        for (int i = 0; i < NS; ++i) {
          ks[i] = j == 0 ? f[i] : (method == 2 ? f[i] : (method == 1 || j == 3 ? ks[i] + f[i] : ks[i] + 2.0 * f[i]));
          dks[i] = j == 0 ? df[i] : (method == 2 ? df[i] : (method == 1 || j == 3 ? dks[i] + df[i] : dks[i] + 2.0 * df[i]));
          w[i] = x[i] + av[j] * h * f[i];
          dw[i] = dx[i] + av[j] * h * df[i];
        }
      }
      const double hs = method == 1 ? 0.5 * h : (method == 3 ? h / 6.0 : h);
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        x[i] += hs * ks[i];
        dx[i] += hs * dks[i];
        xc[((long)(s + 1) * NS + i) * Bp] = x[i];
        dc[((long)(s + 1) * NS + i) * Bp] = dx[i];
        if (jb) jb[(long)(s + 1) * NS + i] = dx[i];
      }
    }
  }
  if (!out) return;                                              // (a kernel argument: the same for every wavefront)
  typename F::Acc g;
#pragma unroll
  for (int c = 0; c < NW; ++c) g.w1[c] = 0.0;
#pragma unroll
  for (int k = 0; k < H; ++k) g.w2[k] = 0.0;
#pragma unroll
  for (int r = 0; r < NS; ++r) { g.w3[r] = 0.0; g.b3[r] = 0.0; }
  g.b1 = 0.0; g.b2 = 0.0;
  double lam[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) lam[i] = 2.0 * (wt ? wt[num_steps] : 1.0) * dx[i];
  for (int s = num_steps - 1; s >= 0; --s) {
#pragma unroll
    for (int i = 0; i < NS; ++i) { x[i] = xc[((long)s * NS + i) * Bp]; dx[i] = dc[((long)s * NS + i) * Bp]; w[i] = x[i]; }
    const int nst = F::plan(method, s, u_rows, ub, uc, av, bv);
#pragma unroll 1
    for (int j = 0; j < nst; ++j) {                              // the stage points and their activations, forward
      double h1, h2;
      w[NS] = uc[j];
      F::fwd(wl, lane, w, h1, h2, f);
#pragma unroll
      for (int c = 0; c < NW; ++c) st[j][c] = w[c];
      st[j][8 + lane] = h1;
      st[j][8 + H + lane] = h2;
#pragma unroll
      for (int i = 0; i < NS; ++i) w[i] = x[i] + av[j] * h * f[i];
    }
    double wx[NS], acc[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) { wx[i] = 0.0; acc[i] = 0.0; }
#pragma unroll 1
    for (int j = nst - 1; j >= 0; --j) {                         // the stage cotangents, backward
      double v[NS];
#pragma unroll
      for (int i = 0; i < NS; ++i) v[i] = bv[j] * h * lam[i] + av[j] * h * wx[i];
#pragma unroll
      for (int c = 0; c < NW; ++c) w[c] = st[j][c];
      F::bwd(wl, lane, w, st[j][8 + lane], st[j][8 + H + lane], v, g, wx);
#pragma unroll
      for (int i = 0; i < NS; ++i) acc[i] += wx[i];
    }
    const double ws = wt ? wt[s] : 1.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) lam[i] += acc[i] + 2.0 * ws * dx[i];
  }
  double* gr = out + b * (long)F::NP;                            // the parameter order of node_system.h
  using S_ = typename F::Sys;
#pragma unroll
  for (int c = 0; c < NW; ++c) gr[S_::O_W1 + c * H + lane] = g.w1[c];
  gr[S_::O_B1 + lane] = g.b1;
#pragma unroll
  for (int k = 0; k < H; ++k) gr[S_::O_W2 + k * H + lane] = g.w2[k];
  gr[S_::O_B2 + lane] = g.b2;
#pragma unroll
  for (int r = 0; r < NS; ++r) { gr[S_::O_W3 + lane * NS + r] = g.w3[r]; gr[S_::O_B3 + r] = g.b3[r]; }
}
#endif  // __HIPCC__

}  // namespace myriad
