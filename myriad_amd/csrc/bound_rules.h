// bound_rules.h -- the rules that treat ONE bounded variable of the barrier problem, each written once for the lane cores
// (hs_solver.h, os_solver.h), HsWave, HsFused and ShootWave.  Functions of values, forced inline like the rules of ip_policy.h:
// loads, stores, lane striding, `live` masks and reductions stay at the call sites.  Plain fp64 / int code for the device and the
// host twin; included by hs_solver.h behind detail::rcp_ / dmax / dmin.  ("The bound rules".)
//
// The solvers differ in three deliberate ways, each stated at its call site:
//   * division: bound_accept<false> divides (HsSolver::update, ShootWave::update), bound_accept<true> multiplies by detail::rcp_
//     (HsWave::points_lin / update, HsFused::step_at / lin_at) -- different bits on the device, the same on the host;
//   * the new point `zn` is formed by the caller: zv + ap * d (lane cores, HsWave), fma(ap, d, zv) (HsFused: the stored network
//     activations belong to exactly that point), the stored trial point zt[i] (ShootWave, when the accepted step was the last trial);
//   * logs: one per point in collocation (SlackLog), one per variable in shooting (log(slack_pair(..))).
#pragma once

#define MYR_BOUND MYR_HD inline __attribute__((always_inline))

namespace myriad {

// bound classes of a variable: free to move (l < u; otherwise pinned, a NaN bound included), lower / upper bound present
struct BoundKind { bool fr, hl, hu; };
MYR_BOUND BoundKind bound_kind(double l, double u) {
  const bool fr = l < u;
  return {fr, fr && (l > -INFINITY), fr && (u < INFINITY)};
}

// starting point: a pinned variable on its value, the others pushed strictly inside their bounds; multipliers 1 on present sides
struct BoundStart { double z, zL, zU; };
MYR_BOUND BoundStart bound_start(double v0, double l, double u) {
  const double k1 = 1e-2, k2 = 1e-2;
  const BoundKind k = bound_kind(l, u);
  const double width = (k.hl && k.hu) ? (u - l) : INFINITY;
  const double pl = detail::dmin(k1 * detail::dmax(1.0, fabs(l)), k2 * width);
  const double pu = detail::dmin(k1 * detail::dmax(1.0, fabs(u)), k2 * width);
  double v = v0;
  v = k.hl ? detail::dmax(v, l + pl) : v;
  v = k.hu ? detail::dmin(v, u - pu) : v;
  v = k.fr ? v : l;
  return {v, k.hl ? 1.0 : 0.0, k.hu ? 1.0 : 0.0};
}

// accepted step: zL += a_d dzL, zU += a_d dzU at the old point zv, then kept within [m / ksig, m ksig], m = mu / (new slack);
// `zn` is the new point as the caller formed and stores it, iks = 1 / ksig
struct BoundMult { double zL, zU; };
template <bool RCP>
MYR_BOUND double bound_div(double x, double s) { if constexpr (RCP) return x * detail::rcp_(s); else return x / s; }
template <bool RCP>
MYR_BOUND BoundMult bound_accept(BoundKind k, double l, double u, double zv, double zn, double d, double zl, double zu,
                                 double ad, double mu, double ksig, double iks) {
  const double sl = k.hl ? zv - l : 1.0, su = k.hu ? u - zv : 1.0;
  const double snl = k.hl ? zn - l : 1.0, snu = k.hu ? u - zn : 1.0;
  double vl = zl + ad * (-zl + bound_div<RCP>(mu - zl * d, sl));
  double vu = zu + ad * (-zu + bound_div<RCP>(mu + zu * d, su));
  const double ml = bound_div<RCP>(mu, snl), mu_ = bound_div<RCP>(mu, snu);      // one division per new slack
  vl = detail::dmax(detail::dmin(vl, ksig * ml), ml * iks);
  vu = detail::dmax(detail::dmin(vu, ksig * mu_), mu_ * iks);
  return {k.hl ? vl : 0.0, k.hu ? vu : 0.0};
}

// slack pair (v - l)(u - v) of a point's variable at value v, absent and violated sides as 1; `bad` counts the violated ones
MYR_BOUND double slack_pair(BoundKind k, double v, double l, double u, int& bad) {
  const double sl = k.hl ? v - l : 1.0, su = k.hu ? u - v : 1.0;
  bad += (sl > 0.0 ? 0 : 1) + (su > 0.0 ? 0 : 1);
  return (sl > 0.0 ? sl : 1.0) * (su > 0.0 ? su : 1.0);
}
// sum of log(slack) over the variables of one point with ONE log (fp64 log is a long software sequence): the slack pairs are
// multiplied as mantissas, their binary exponents summed, so no product can under- or overflow
struct SlackLog {
  double slk = 1.0; int sexp = 0, bad = 0;
  MYR_BOUND void add(BoundKind k, double v, double l, double u) { int e_; slk *= frexp(slack_pair(k, v, l, u, bad), &e_); sexp += e_; }
  MYR_BOUND double value() const { return log(slk) + sexp * 0.6931471805599453; }
};

// sum and count of the bound multipliers (for the KKT error's scaling)
MYR_BOUND void mult_sum(BoundKind k, double zl, double zu, double& sm, int& nm) {
  sm += (k.hl ? zl : 0.0) + (k.hu ? zu : 0.0);
  nm += (k.hl ? 1 : 0) + (k.hu ? 1 : 0);
}

// (bound_terms and step_limits keep their class lines literal: with bound_kind inside them the fused kernel's passes compile to other code, r14's README)
// bound data of one variable (branch-free): barrier Hessian sigma, (-zL + zU) for the adjoint,
// mu-coefficient g1 = -1/(z-l) + 1/(u-z); complementarity extremes; pinned flag
struct BoundTerms { double sigma, g1, zlu; bool pinned; };
MYR_BOUND BoundTerms bound_terms(double zv, double l, double u, double zl, double zu, double& compl_max, double& compl_min) {
  BoundTerms r;
  const bool fr = l < u;
  const bool hl = fr && (l > -INFINITY), hu = fr && (u < INFINITY);
  const double sl = hl ? zv - l : 1.0, su = hu ? u - zv : 1.0;
  const double zlv = hl ? zl : 0.0, zuv = hu ? zu : 0.0;
  const double il = hl ? detail::rcp_(sl) : 0.0, iu = hu ? detail::rcp_(su) : 0.0;
  r.pinned = !fr;
  r.sigma = zlv * il + zuv * iu;
  r.g1 = iu - il;
  r.zlu = zuv - zlv;
  const double cl = sl * zlv, cu = su * zuv;
  compl_max = detail::dmax(compl_max, detail::dmax(hl ? cl : compl_max, hu ? cu : compl_max));
  compl_min = detail::dmin(compl_min, detail::dmin(hl ? cl : compl_min, hu ? cu : compl_min));
  return r;
}

// accumulates gphi = grad(phi_mu)^T dz and the fraction-to-the-boundary limits for z (primal) and zL, zU (dual) in a core's
// FwdOut {alpha_p, alpha_d, gphi}; branch-free, operands already in registers
template <class FwdOut>
MYR_BOUND void step_limits(double zv, double l, double u, double zl, double zu, double d, double mu, double wg_grad, double tau,
                           FwdOut& fo) {
  const bool fr = l < u;
  const bool hl = fr && (l > -INFINITY), hu = fr && (u < INFINITY);
  const double sl = hl ? zv - l : 1.0, su = hu ? u - zv : 1.0;
  const double zlv = hl ? zl : 1.0, zuv = hu ? zu : 1.0;
  // five fp64 divisions instead of eight (each is a ~35-instruction sequence): one reciprocal per slack, one for the
  // step component (only the bound the step moves towards can limit it)
  const double rsl = detail::rcp_(sl), rsu = detail::rcp_(su);
  double gb = wg_grad;
  gb -= hl ? mu * rsl : 0.0;
  gb += hu ? mu * rsu : 0.0;
  const double dzl = -zlv + (mu - zlv * d) * rsl;
  const double dzu = -zuv + (mu + zuv * d) * rsu;
  const bool tol_ = hl && d < 0.0, tou_ = hu && d > 0.0;
  const double ap_ = (tol_ || tou_) ? tau * (tol_ ? sl : su) * detail::rcp_(fabs(d)) : 1.0;
  const double ad_l = (hl && dzl < 0.0) ? -tau * zlv * detail::rcp_(dzl) : 1.0;
  const double ad_u = (hu && dzu < 0.0) ? -tau * zuv * detail::rcp_(dzu) : 1.0;
  fo.alpha_p = detail::dmin(fo.alpha_p, ap_);
  fo.alpha_d = detail::dmin(fo.alpha_d, detail::dmin(ad_l, ad_u));
  fo.gphi += fr ? gb * d : 0.0;
}

}  // namespace myriad
