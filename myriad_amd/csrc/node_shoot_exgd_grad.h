// node_shoot_exgd_grad.h -- derivative of `nsteps` unrolled extragradient steps in the 4 804 weights of the network system under the SHOOTING
// transcription (K15 in DESIGN.md; C-ABI myr_exgd_grad_node_shoot).  The route the reference's experiments/node_e2e_sysid.py runs by default.
//
// The sweep is K13's (shoot_exgd_grad.h: items 1-5 over the shooting Lagrangian, 2 nsteps + 1 pair passes with the masks between them, a_lam in a
// column per pair, item 5 of step s fused with item 1 of step s - 1); ShootExgdGrad::pass_of / out_z / mask and ShootHvp::gather_z are used as
// they stand.
// The stage tableaux and control-row rules are K14's (NodeShootProd::rule / stage_point).  The network at a stage point is K12's
// (node_exgd_grad.h).  What is new is the pair pass that joins them: ShootHvp::interval<true> with the closed-form stage rule replaced by the
// layer-by-layer one.  For a stage point w_j = [X_j; U_j] of a step with tangent d_j, costate kap_j on f(w_j), its tangent kapd_j and cost
// weight om_j = h b_j:
//   first order    xbar  = J^T kap + om dg                                          (the TRUE system's running cost, integrated along the rollout)
//   second order   dbar  = J^T kapd + (sum_r kap_r d2 f_r) d + om d2g d
//   weights        gp   += the gradient of  kapd^T f(w) + kap^T J(w) d             (K12's item (a) with v = kapd plus item (c) with mu = kap)
// and the forward halves need f(w) and J d.  The cost has no weights, but it sits on stage points that depend on them: its dg enters every kap
// and its d2g d every dbar -- without them the gradient is that of another objective.
//
// NodeShootExgd<M> is the pair and step algebra, host/device shared and templated on how the network is evaluated:
//   Net::val(w, f)                         f(w)
//   Net::tan(w, d, f, fd)                  f(w), fd = J(w) d
//   Net::vjp(w, kap, jt)                   jt[NW] = J^T kap                          (the forward steps: no weight gradient)
//   Net::rule(w, d, kap, kapd, jt, dj)     jt = J^T kap, dj[NW] = J^T kapd + (sum_r kap_r d2 f_r) d, and the weight gradient added to the net's own
// NseHostNet: plain loops (NodeExgdHost::first / second, SysNODE::f / lin) -- node_shoot_exgd_grad_host, tests/hostsim/node_shoot_exgd_grad_twin.cpp.
// NseWaveNet: one wavefront, lane j = hidden unit j of both layers (NodeFit::fwd, NodeExgdWave::first / second), the gradient in NodeFit::Acc.
//
// node_shoot_exgd_grad_kernel<M>: one workgroup per instance, WPI in {1, 2, 4} wavefronts (from I alone: an instance's bits do not depend on the
// batch) that take the intervals k = w, w + WPI, ...; every value of a pair is wave-uniform.  ONE launch per chunk: the forward steps run in the
// kernel (the gradient of the Lagrangian is the first-order half of the same pair pass: interval<false>) and write x_s, x_bar_s, lam_s to the
// history; then the 2 nsteps + 1 seeded passes, each followed by a barrier and the elementwise mask over [n] with all 64 WPI lanes.  Per stage
// nothing of the network is stored: the step-start state and tangent are, and NodeFit::fwd is recomputed at the stage point in the reverse.  The
// weight gradient stays in registers through the call; at the end the wavefronts add theirs in the order 0, 1, ... into the idle weight copy.
// No atomics.
//
// Dynamic LDS (doubles): weights NodeMfma64::L_N | point [n] | x_bar, then the direction [n] | a_x [n] | lam [NS][I] | a_lam [NS][I] |
// step-start (x, xd) [2 NS cpi][I] | side record (node | control rows) [NS + (M cpi + 1) NU][I]  -- pair-minor, as K13's columns.
// Capacity: that sum must fit 160 KB -- 48 I cpi + 115 doubles beside the weights at I = 4 (16 S + 40 under RK4 at I = 1): about 1 250 integration
// steps I cpi in all, 950 under RK4; myr_exgd_grad_node_shoot refuses more with MYR_E_CAPACITY.
// History of one instance (doubles, global): per step x_s [n], x_bar_s [n], lam_s [I][NS]; behind the last step x_n [n].
#pragma once
#include "shoot_exgd_grad.h"
#include "node_shoot_products.h"
#include "node_exgd_grad.h"

namespace myriad {

template <int M>
struct NodeShootExgd {
  using Sys = SysNODE_CARTPOLE;
  using P = NodeShootProd<Sys, M>;
  using G = ShootExgdGrad<Sys, M>;
  using HV = ShootHvp<Sys, M>;
  using Rule = typename P::Rule;
  static constexpr int NS = Sys::NS, NU = Sys::NU, NW = Sys::NW, NP = Sys::NP, NST = P::NST, NR = M + 1;
  MYR_HD static inline long nvars(int I, int cpi) { return P::nvars(I, cpi); }
  MYR_HD static inline long pair_hist_doubles(int cpi) { return (long)cpi * 2 * NS; }                 // (x, xd) at the start of every step
  MYR_HD static inline long side_doubles(int cpi) { return NS + HV::ctrl_doubles(cpi); }              // ShootHvp's side record without the parameter row
  MYR_HD static inline long hist_doubles(int I, int cpi, int nsteps) { return G::hist_doubles(I, cpi, nsteps); }
  // per instance, beside the weight copy
  MYR_HD static inline long work_doubles(int I, int cpi) {
    return 3 * nvars(I, cpi) + (long)I * (2 * NS + pair_hist_doubles(cpi) + side_doubles(cpi));
  }

  // one step forward, with its tangent when TAN: (x, xd) <- (x+, xd+).  uc, ud: the step's NR control rows and their tangents
  template <bool TAN, class Net>
  MYR_HD static inline void step_fwd(Net& net, const Rule& R, double h, const double* uc, const double* ud, double* x, double* xd) {
    double kp[NS], kd[NS], acc[NS], accd[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) { kp[c] = 0.0; kd[c] = 0.0; acc[c] = 0.0; accd[c] = 0.0; }
#pragma unroll 1
    for (int j = 0; j < R.nst; ++j) {
      double w[NW], d[NW], F[NS], Fd[NS];
      P::stage_point(R, h, j, x, kp, uc, w, w + NS);
      if constexpr (TAN) {
        P::stage_point(R, h, j, xd, kd, ud, d, d + NS);
        net.tan(w, d, F, Fd);
      } else {
        net.val(w, F);
      }
#pragma unroll
      for (int c = 0; c < NS; ++c) {
        kp[c] = F[c]; acc[c] += R.b[j] * F[c];
        if constexpr (TAN) { kd[c] = Fd[c]; accd[c] += R.b[j] * Fd[c]; }
      }
    }
#pragma unroll
    for (int c = 0; c < NS; ++c) {
      x[c] = x[c] + h * acc[c];
      if constexpr (TAN) xd[c] = xd[c] + h * accd[c];
    }
  }

  // one step backwards (ShootHvp::step_back).  (x, xd): state and tangent at the START of the step; (a, ad): cotangent of x+ and its tangent,
  // replaced by those of x; ub[NR NU] += the cotangent of the step's control rows -- second order when SECOND, first order otherwise (then xd, ud,
  // ad are not read)
  template <bool SECOND, class Net>
  MYR_HD static inline void step_back(Net& net, const Rule& R, double h, const double* x, const double* xd, const double* uc, const double* ud,
                                      const double* p, double cw, double* a, double* ad, double* ub) {
    double W[NST][NW], D[NST][NW];
    {
      double kp[NS], kd[NS];
#pragma unroll
      for (int c = 0; c < NS; ++c) { kp[c] = 0.0; kd[c] = 0.0; }
#pragma unroll 1
      for (int j = 0; j < R.nst; ++j) {
        P::stage_point(R, h, j, x, kp, uc, W[j], W[j] + NS);
        if constexpr (SECOND) P::stage_point(R, h, j, xd, kd, ud, D[j], D[j] + NS);
        if (j + 1 < R.nst) {
          if constexpr (SECOND) net.tan(W[j], D[j], kp, kd); else net.val(W[j], kp);
        }
      }
    }
    double xb[NW], db[NW], sa[NS], sad[NS];
#pragma unroll
    for (int c = 0; c < NW; ++c) { xb[c] = 0.0; db[c] = 0.0; }
#pragma unroll
    for (int c = 0; c < NS; ++c) { sa[c] = a[c]; sad[c] = SECOND ? ad[c] : 0.0; }
#pragma unroll 1
    for (int j = R.nst - 1; j >= 0; --j) {
      const double hb = h * R.b[j];
      const double hn = j + 1 < R.nst ? h * R.c[j + 1] : 0.0;      // what stage j + 1 hands back: X_{j+1} = x + c_{j+1} h k_j
      const double om = cw * hb;
      double kap[NS], kapd[NS], jt[NW], dj[NW], go, gw[NW];
#pragma unroll
      for (int c = 0; c < NS; ++c) { kap[c] = hb * a[c] + hn * xb[c]; kapd[c] = SECOND ? hb * ad[c] + hn * db[c] : 0.0; }
      if constexpr (SECOND) net.rule(W[j], D[j], kap, kapd, jt, dj); else net.vjp(W[j], kap, jt);
      Sys::cost_grad(W[j], W[j] + NS, p, &go, gw);
#pragma unroll
      for (int c = 0; c < NW; ++c) xb[c] = jt[c] + om * gw[c];
      if constexpr (SECOND) {
        double hc[NW];
        NodeExgdHost::cost_hd(W[j], om, D[j], hc);
#pragma unroll
        for (int c = 0; c < NW; ++c) db[c] = dj[c] + hc[c];
      }
#pragma unroll
      for (int c = 0; c < NS; ++c) { sa[c] += xb[c]; if constexpr (SECOND) sad[c] += db[c]; }
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int c = 0; c < NU; ++c) ub[r * NU + c] += R.cu[j][r] * (SECOND ? db[NS + c] : xb[NS + c]);
    }
#pragma unroll
    for (int c = 0; c < NS; ++c) { a[c] = sa[c]; if constexpr (SECOND) ad[c] = sad[c]; }
  }

  // One (instance, interval) pair: ShootHvp::interval<true> when SECOND.  zb, vb: the instance's point and direction; lk: lam_k, al: a_lam,k, hist:
  // pair_hist_doubles and side: side_doubles of this pair, all with consecutive doubles `stride` apart (the instance's I pairs side by side).
  // SECOND: al gains the pair's rows of J v, the reverse starts from ad = scale al; side = ad at the node | second-order cotangent of the control
  // rows.  Otherwise (vb, al not read): side = the pair's share of grad_z (f + lam^T c) without the linear term -lam_{k-1} (out_z adds it).
  template <bool SECOND, class Net>
  MYR_HD static inline void interval(Net& net, const Rule& R, int I, int cpi, int k, double h, const double* zb, const double* vb, const double* lk,
                                     const double* p, double cw, double* hist, double* side, long stride, double* al, double scale) {
    const double* zu = zb + (long)(I + 1) * NS;
    const double* vu = SECOND ? vb + (long)(I + 1) * NS : nullptr;
    double x[NS], xd[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) { x[q] = zb[(long)k * NS + q]; xd[q] = SECOND ? vb[(long)k * NS + q] : 0.0; }
    for (int j = 0; j < cpi; ++j) {
      const long i = (long)k * cpi + j;
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        hist[((long)j * 2 * NS + q) * stride] = x[q];
        if constexpr (SECOND) hist[((long)j * 2 * NS + NS + q) * stride] = xd[q];
      }
      step_fwd<SECOND>(net, R, h, zu + M * i * NU, SECOND ? vu + M * i * NU : nullptr, x, xd);
    }
    double a[NS], ad[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) { a[q] = lk ? lk[(long)q * stride] : 0.0; ad[q] = 0.0; }
    if constexpr (SECOND) {
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        const double al_q = al[(long)q * stride] + (xd[q] - vb[(long)(k + 1) * NS + q]);
        al[(long)q * stride] = al_q;
        ad[q] = scale * al_q;
      }
    }
    double* su = side + (long)NS * stride;
    double carry[NU];      // what the step behind has for the row it shares with this one
#pragma unroll
    for (int c = 0; c < NU; ++c) carry[c] = 0.0;
    for (int j = cpi - 1; j >= 0; --j) {
      const long i = (long)k * cpi + j;
      double ub[NR * NU];
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        x[q] = hist[((long)j * 2 * NS + q) * stride];
        if constexpr (SECOND) xd[q] = hist[((long)j * 2 * NS + NS + q) * stride];
      }
#pragma unroll
      for (int c = 0; c < NR * NU; ++c) ub[c] = 0.0;
      step_back<SECOND>(net, R, h, x, xd, zu + M * i * NU, SECOND ? vu + M * i * NU : nullptr, p, cw, a, ad, ub);
#pragma unroll
      for (int c = 0; c < NU; ++c) {
        su[((long)(M * j + M) * NU + c) * stride] = ub[M * NU + c] + carry[c];
        if (M == 2) su[((long)(M * j + 1) * NU + c) * stride] = ub[NU + c];
        carry[c] = ub[c];
      }
    }
#pragma unroll
    for (int c = 0; c < NU; ++c) su[(long)c * stride] = carry[c];
#pragma unroll
    for (int q = 0; q < NS; ++q) side[(long)q * stride] = SECOND ? ad[q] : a[q];
  }

  // the pair's row of the constraints c_k = x_end(x_k, u) - x_{k+1} (the multiplier step)
  template <class Net>
  MYR_HD static inline void residual(Net& net, const Rule& R, int I, int cpi, int k, double h, const double* zb, double* ck) {
    const double* zu = zb + (long)(I + 1) * NS;
    double x[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) x[q] = zb[(long)k * NS + q];
    for (int j = 0; j < cpi; ++j) step_fwd<false>(net, R, h, zu + M * ((long)k * cpi + j) * NU, nullptr, x, nullptr);
#pragma unroll
    for (int q = 0; q < NS; ++q) ck[q] = x[q] - zb[(long)(k + 1) * NS + q];
  }
};

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host twin: the network in plain loops, the weight gradient straight into gp ---------------------------------------------------------------
struct NseHostNet {
  using E = NodeExgdHost;
  using Sys = E::Sys;
  const double* p; double* gp;
  inline void val(const double* w, double* f) const { Sys::f(w, w + E::NS, p, f); }
  inline void tan(const double* w, const double* d, double* f, double* fd) const {
    double A[E::NS * E::NS], Bm[E::NS * E::NU], g, gw[E::NW];
    Sys::lin(w, w + E::NS, p, f, A, Bm, &g, gw);
    for (int r = 0; r < E::NS; ++r) {
      double s = 0.0;
      for (int c = 0; c < E::NS; ++c) s += A[r * E::NS + c] * d[c];
      for (int c = 0; c < E::NU; ++c) s += Bm[r * E::NU + c] * d[E::NS + c];
      fd[r] = s;
    }
  }
  inline void vjp(const double* w, const double* kap, double* jt) const {
    double f[E::NS];
    E::first(w, p, kap, f, jt, nullptr);
  }
  inline void rule(const double* w, const double* d, const double* kap, const double* kapd, double* jt, double* dj) const {
    double f[E::NS], j1[E::NW], wo[E::NS], hd[E::NW];
    E::first(w, p, kapd, f, j1, gp);
    E::first(w, p, kap, f, jt, nullptr);
    E::second(w, p, kap, d, wo, hd, gp);
    for (int c = 0; c < E::NW; ++c) dj[c] = j1[c] + hd[c];
  }
};

// One instance on the host.  p: the NP shared weights; hist: hist_doubles(I, cpi, nsteps) doubles; work: work_doubles(I, cpi) + n doubles (the
// carve of the kernel's LDS, then a zero direction for the unfused order); seed_lam, dz0, dlam0 may be null; gp[NP].  fused == false runs
// items 1 .. 5 as THREE passes a step (ShootExgdGrad::pass_of_unfused), as shoot_exgd_grad_host does, for the test of the fusion.
template <int M>
inline void node_shoot_exgd_grad_host(int method, int I, int cpi, double T, const double* z, const double* lam, const double* lb, const double* ub,
                                      const double* p, double eta_x, double eta_v, int nsteps, const double* seed_z, const double* seed_lam,
                                      double* hist, double* work, double* gp, double* dz0, double* dlam0, bool fused = true) {
  using A = NodeShootExgd<M>;
  using G = typename A::G;
  constexpr int NS = A::NS, NP = A::NP;
  const long n = A::nvars(I, cpi), m = (long)I * NS, hs = 2 * n + m;
  const double h = T / ((double)I * cpi);
  const typename A::Rule R = A::P::rule(method);
  double* zx = work;
  double* zb = zx + n;                                         // x_bar of the forward steps, the direction of the reverse sweep
  double* ax = zb + n;
  double* lc = ax + n;                                         // [NS][I]: pair-minor, as on the device
  double* al = lc + m;
  double* phist = al + m;
  double* side = phist + A::pair_hist_doubles(cpi) * I;
  double* zero = side + A::side_doubles(cpi) * I;
  for (int e = 0; e < NP; ++e) gp[e] = 0.0;
  NseHostNet net{p, gp};
  // ---- forward ----
  for (long i = 0; i < n; ++i) zx[i] = z[i];
  for (int k = 0; k < I; ++k)
    for (int q = 0; q < NS; ++q) lc[k + (long)q * I] = lam[(long)k * NS + q];
  for (int s = 0; s < nsteps; ++s) {
    double* Hh = hist + s * hs;
    for (long i = 0; i < n; ++i) Hh[i] = zx[i];
    for (int k = 0; k < I; ++k)
      for (int q = 0; q < NS; ++q) Hh[2 * n + (long)k * NS + q] = lc[k + (long)q * I];
    for (int half = 0; half < 2; ++half) {
      const double* src = half == 0 ? zx : zb;
      double* dst = half == 0 ? zb : zx;
      for (int k = 0; k < I; ++k)
        A::template interval<false>(net, R, I, cpi, k, h, src, nullptr, lc + k, p, 1.0, phist + k, side + k, I, nullptr, 0.0);
      for (long i = 0; i < n; ++i) dst[i] = A::P::clip_step(zx[i], G::out_z(I, cpi, i, side, lc, 1.0, I), eta_x, lb[i], ub[i]);
      if (half == 0) for (long i = 0; i < n; ++i) Hh[n + i] = zb[i];
    }
    for (int k = 0; k < I; ++k) {
      double ck[NS];
      A::residual(net, R, I, cpi, k, h, zx, ck);
      for (int q = 0; q < NS; ++q) lc[k + (long)q * I] += eta_v * ck[q];
    }
  }
  for (long i = 0; i < n; ++i) hist[nsteps * hs + i] = zx[i];
  // ---- reverse ----
  for (long i = 0; i < n; ++i) { ax[i] = seed_z[i]; zb[i] = 0.0; zero[i] = 0.0; }
  for (int k = 0; k < I; ++k)
    for (int q = 0; q < NS; ++q) al[k + (long)q * I] = seed_lam ? seed_lam[(long)k * NS + q] : 0.0;
  auto pass = [&](const double* pt, const double* lk, const double* v, double scale, int mode) {
    if (lk)
      for (int k = 0; k < I; ++k)
        for (int q = 0; q < NS; ++q) lc[k + (long)q * I] = lk[(long)k * NS + q];
    for (int k = 0; k < I; ++k)
      A::template interval<true>(net, R, I, cpi, k, h, pt, v, lk ? lc + k : nullptr, p, 1.0, phist + k, side + k, I, al + k, scale);
    for (long i = 0; i < n; ++i) G::mask(mode, G::out_z(I, cpi, i, side, al, scale, I), pt[i], lb[i], ub[i], eta_x, ax[i], zb[i]);
  };
  for (int ps = 0; ps < (fused ? G::passes(nsteps) : G::passes_unfused(nsteps)); ++ps) {
    const typename G::Pass q = fused ? G::pass_of(ps, nsteps, eta_v) : G::pass_of_unfused(ps, nsteps, eta_v);
    const double* Hh = hist + q.s * hs;
    pass(q.at_bar ? Hh + n : Hh, q.alone ? nullptr : Hh + 2 * n, q.alone ? zero : zb, q.scale, q.mode);
  }
  if (dz0) for (long i = 0; i < n; ++i) dz0[i] = ax[i];
  if (dlam0)
    for (int k = 0; k < I; ++k)
      for (int q = 0; q < NS; ++q) dlam0[(long)k * NS + q] = al[k + (long)q * I];
}
#endif  // !__HIP_DEVICE_COMPILE__

#if defined(__HIPCC__)
// the network on one wavefront at a wave-uniform point: every lane ends with the same f, fd, jt, dj
struct NseWaveNet {
  using F = NodeFit;
  using NM = NodeMfma64;
  using W = NodeExgdWave;
  static constexpr int NS = F::NS, NW = F::NW, H = F::H;
  const double* wl; int lane; NodeFit::Acc* g;
  __device__ inline void val(const double* w, double* f) const {
    double h1, h2;
    F::fwd(wl, lane, w, h1, h2, f);
  }
  __device__ inline void tan(const double* w, const double* d, double* f, double* fd) const {
    double h1, h2;
    F::fwd(wl, lane, w, h1, h2, f);
    double da1 = 0.0;
#pragma unroll
    for (int c = 0; c < NW; ++c) da1 += d[c] * wl[NM::L_W1 + c * H + lane];
    const double dh1 = h1 * (1.0 - h1) * da1;
    double da2 = 0.0;
#pragma unroll 8
    for (int k = 0; k < H; ++k) da2 += F::bcast(dh1, k) * wl[NM::L_W2 + k * NM::LD2 + lane];
    const double dh2 = h2 * (1.0 - h2) * da2;
#pragma unroll
    for (int r = 0; r < NS; ++r) fd[r] = F::wsum(dh2 * wl[NM::L_W3 + lane * NS + r]);
  }
  __device__ inline void vjp(const double* w, const double* kap, double* jt) const {
    double h1, h2, f[NS];
    F::fwd(wl, lane, w, h1, h2, f);
    W::template first<false>(wl, lane, w, h1, h2, kap, *g, jt);
  }
  __device__ inline void rule(const double* w, const double* d, const double* kap, const double* kapd, double* jt, double* dj) const {
    double h1, h2, f[NS], j1[NW], wo[NS], hd[NW];
    F::fwd(wl, lane, w, h1, h2, f);
    W::template first<true>(wl, lane, w, h1, h2, kapd, *g, j1);
    W::template first<false>(wl, lane, w, h1, h2, kap, *g, jt);
    W::second(wl, lane, w, h1, h2, kap, d, *g, wo, hd);
#pragma unroll
    for (int c = 0; c < NW; ++c) dj[c] = j1[c] + hd[c];
  }
};

struct NseArgs {
  int B, I, cpi, method, nsteps;
  int inst0, R;      // weight sets: the chunk's first instance is number inst0 of the call; R instances to a set
  double T, eta_x, eta_v;
  const double *z, *lam, *lb, *ub, *seed_z, *seed_lam;      // the chunk's
  const double* params;                                      // the call's [E][NP]: does not advance with the chunk
  double *hist, *grad, *dz0, *dlam0;
};

template <int M>
inline size_t node_shoot_exgd_grad_lds_bytes(int I, int cpi) {
  return (size_t)(NodeMfma64::L_N + NodeShootExgd<M>::work_doubles(I, cpi)) * 8 + 16;
}
// wavefronts per instance: from I alone
inline int node_shoot_exgd_grad_wpi(int I) { return I >= 4 ? 4 : (I >= 2 ? 2 : 1); }

// One workgroup of WPI = blockDim.x / 64 wavefronts per instance (blockIdx.x: the instance within this launch's chunk; every pointer is the
// chunk's, but params: instance i of the call reads the row of set i / R, as node_exgd_grad_kernel).  In a pair pass wavefront w takes the intervals k = w, w + WPI, ... one after the other and writes only their columns (wave-uniform
// values: every lane stores); an idle wavefront of the last round skips the pair's work behind a wave-uniform test and reaches every barrier.
template <int M>
__global__ __launch_bounds__(256)
void node_shoot_exgd_grad_kernel(NseArgs a) {
  using A = NodeShootExgd<M>;
  using G = typename A::G;
  using S_ = typename A::Sys;
  constexpr int NS = A::NS, NW = A::NW, NP = A::NP, H = NodeFit::H;
  extern __shared__ __attribute__((aligned(16))) char smem_node_shoot_exgd_grad[];
  const long b = blockIdx.x;
  if (b >= a.B) return;                                           // (the whole workgroup)
  const int tid = threadIdx.x, lane = tid & 63, NT = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int WPI = __builtin_amdgcn_readfirstlane(NT >> 6);
  const int I = a.I, cpi = a.cpi, nsteps = a.nsteps;
  const long n = A::nvars(I, cpi), m = (long)I * NS, hs = 2 * n + m;
  const double h = a.T / ((double)I * cpi);
  double* wl = reinterpret_cast<double*>(smem_node_shoot_exgd_grad);
  double* zx = wl + NodeMfma64::L_N;
  double* zb = zx + n;
  double* ax = zb + n;
  double* lc = ax + n;
  double* al = lc + m;
  double* phist = al + m;
  double* side = phist + A::pair_hist_doubles(cpi) * I;
  const double* lo = a.lb + b * n;
  const double* hi = a.ub + b * n;
  double* hb = a.hist + b * A::hist_doubles(I, cpi, nsteps);
  const double* params = a.params + (long)((a.inst0 + (int)blockIdx.x) / a.R) * NP;      // this instance's weight set: every use below
  NodeMfma64::load_weights(params, wl, tid, NT);
  for (long i = tid; i < n; i += NT) zx[i] = a.z[b * n + i];
  for (long i = tid; i < m; i += NT) { const long k = i / NS, q = i - k * NS; lc[k + q * I] = a.lam[b * m + i]; }
  __syncthreads();
  const typename A::Rule R = A::P::rule(a.method);
  NodeFit::Acc acc;
  NodeExgdWave::zero(acc);
  NseWaveNet net{wl, lane, &acc};
  // ---- forward ----
  for (int s = 0; s < nsteps; ++s) {
    double* Hh = hb + s * hs;
    for (long i = tid; i < n; i += NT) Hh[i] = zx[i];
    for (long i = tid; i < m; i += NT) { const long k = i / NS, q = i - k * NS; Hh[2 * n + i] = lc[k + q * I]; }
    for (int half = 0; half < 2; ++half) {
      const double* src = half == 0 ? zx : zb;
      double* dst = half == 0 ? zb : zx;
      for (int k = wave; k < I; k += WPI)                          // (wave-uniform bounds; no barrier inside)
        A::template interval<false>(net, R, I, cpi, k, h, src, nullptr, lc + k, params, 1.0, phist + k, side + k, I, nullptr, 0.0);
      __syncthreads();
      for (long i = tid; i < n; i += NT) {
        const double v = A::P::clip_step(zx[i], G::out_z(I, cpi, i, side, lc, 1.0, I), a.eta_x, lo[i], hi[i]);
        dst[i] = v;
        if (half == 0) Hh[n + i] = v;
      }
      __syncthreads();
    }
    for (int k = wave; k < I; k += WPI) {
      double ck[NS];
      A::residual(net, R, I, cpi, k, h, zx, ck);
#pragma unroll
      for (int q = 0; q < NS; ++q) lc[k + (long)q * I] += a.eta_v * ck[q];
    }
    __syncthreads();
  }
  for (long i = tid; i < n; i += NT) hb[nsteps * hs + i] = zx[i];
  // ---- reverse ----
  for (long i = tid; i < n; i += NT) { ax[i] = a.seed_z[b * n + i]; zb[i] = 0.0; }
  for (long i = tid; i < m; i += NT) { const long k = i / NS, q = i - k * NS; al[k + q * I] = a.seed_lam ? a.seed_lam[b * m + i] : 0.0; }
  __syncthreads();
  const int npass = G::passes(nsteps);
  for (int ps = 0; ps < npass; ++ps) {
    const typename G::Pass q = G::pass_of(ps, nsteps, a.eta_v);
    const double* Hh = hb + q.s * hs;
    const double* pt = q.at_bar ? Hh + n : Hh;
    const bool has_lam = q.s < nsteps;                             // (= !q.alone in this order; the pass at x_n runs on the cleared direction zb)
    for (long i = tid; i < n; i += NT) zx[i] = pt[i];
    if (has_lam)
      for (long i = tid; i < m; i += NT) { const long k = i / NS, r = i - k * NS; lc[k + r * I] = Hh[2 * n + i]; }
    __syncthreads();
    for (int k = wave; k < I; k += WPI)
      A::template interval<true>(net, R, I, cpi, k, h, zx, zb, has_lam ? lc + k : nullptr, params, 1.0, phist + k, side + k, I, al + k, q.scale);
    __syncthreads();
    for (long i = tid; i < n; i += NT) {
      double av = ax[i], dv;
      G::mask(q.mode, G::out_z(I, cpi, i, side, al, q.scale, I), zx[i], lo[i], hi[i], a.eta_x, av, dv);
      ax[i] = av; zb[i] = dv;
    }
    __syncthreads();
  }
  if (a.dz0) for (long i = tid; i < n; i += NT) a.dz0[b * n + i] = ax[i];
  if (a.dlam0) for (long i = tid; i < m; i += NT) { const long k = i / NS, q = i - k * NS; a.dlam0[b * m + i] = al[k + q * I]; }
  // the weight gradient: wavefront 0 writes its share over the weight copy (idle behind the last barrier) in the parameter order of
  // node_system.h, wavefronts 1, 2, ... add theirs in turn; no atomics, the same bits on every call
  double* gl = wl;
  static_assert(NP <= NodeMfma64::L_N, "the row fits the weight copy");
  double b3v = acc.b3[0];                                          // (the same in every lane: lane r < NS stores entry r)
#pragma unroll
  for (int r = 1; r < NS; ++r) b3v = lane == r ? acc.b3[r] : b3v;
  for (int wv = 0; wv < WPI; ++wv) {
    if (wave == wv) {                                              // (wave-uniform)
      const bool first = wv == 0;
#pragma unroll
      for (int c = 0; c < NW; ++c) { double* q = gl + S_::O_W1 + c * H + lane; *q = first ? acc.w1[c] : *q + acc.w1[c]; }
      { double* q = gl + S_::O_B1 + lane; *q = first ? acc.b1 : *q + acc.b1; }
#pragma unroll
      for (int k = 0; k < H; ++k) { double* q = gl + S_::O_W2 + k * H + lane; *q = first ? acc.w2[k] : *q + acc.w2[k]; }
      { double* q = gl + S_::O_B2 + lane; *q = first ? acc.b2 : *q + acc.b2; }
#pragma unroll
      for (int r = 0; r < NS; ++r) { double* q = gl + S_::O_W3 + lane * NS + r; *q = first ? acc.w3[r] : *q + acc.w3[r]; }
      {
        const bool own = lane < NS;
        double* q = gl + S_::O_B3 + (own ? lane : 0);
        const double v = first ? b3v : *q + b3v;
        if (own) *q = v;
      }
    }
    __syncthreads();
  }
  for (int i = tid; i < NP; i += NT) a.grad[b * NP + i] = gl[i];
}
#endif  // __HIPCC__

}  // namespace myriad
