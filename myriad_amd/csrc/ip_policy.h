// ip_policy.h -- the scalar policy of the interior-point outer loop: its state and every rule on it, each written ONCE,
// for IpLoop<Core>::run (hs_solver.h), HsWave::solve and HsFused::solve.  The loops keep their pass orchestration and
// differ in a few deliberate places, each visible at its call site ("The interior-point policy").
// Plain fp64 / int code for the device and the host twin; included by hs_solver.h behind HsSolveOpts and detail::.
// Every rule is forced inline: as ordinary inline functions their mere presence changes the inliner's decisions for the
// big passes of the fused kernel (profiles/r10_ip_policy/README.md).
#pragma once

#define MYR_POLICY MYR_HD inline __attribute__((always_inline))

namespace myriad {

// penalty relaxation of the l1 merit function (compile-time: the by-value options struct of the kernels is left alone,
// see DESIGN.md on the compiler's sensitivity to its layout): the penalty only has to dominate the CURRENT multipliers;
// steps blocked by bounds early on can push it orders of magnitude above that, after which every full step is rejected
// for a marginal increase of the constraint violation (Maratos-type crawl: config 3's stragglers).  When it has
// exceeded PEN_RELAX_RATIO x the value the descent condition asks for during PEN_RELAX consecutive iterations it is
// reset to twice that value, at most PEN_RELAX_MAX times per solve (so the monotone argument applies from then on).
#ifndef MYR_PEN_RELAX
#define MYR_PEN_RELAX 5          // 0 = off
#endif
// warm-started inertia correction (delta_warm): the first attempt of an iteration uses delta_last / DELTA_WARM_DIV; a
// failed attempt multiplies by 8, i.e. lands at 1.33 delta_last.  Measured on the headline workload (ms per 4096
// solves / median / p99 iterations): div 3: 39.1 / 21 / 34, 4: 39.7 / 21 / 34, 5: 38.0 / 21 / 26, 6: 36.1 / 20 / 25,
// 8: 38.9 / 20 / 25, 12: 38.7 / 21 / 27 -- with 3 the retry overshoots to 2.7 delta_last and the correction ratchets up.
#ifndef MYR_DW_DIV
#define MYR_DW_DIV 6.0
#endif
constexpr double DELTA_WARM_DIV = MYR_DW_DIV;
constexpr int PEN_RELAX = MYR_PEN_RELAX, PEN_RELAX_MAX = 8;
#ifndef MYR_PEN_RELAX_LAM
#define MYR_PEN_RELAX_LAM 1.1
#endif
constexpr double PEN_RELAX_RATIO = 10.0, PEN_RELAX_LAM = MYR_PEN_RELAX_LAM;
constexpr int NMMAX = 8;         // longest non-monotone Armijo memory (HsSolveOpts::nonmono)

// KKT error with the usual multiplier scaling; !finite ends the solve with status 2, converged with status 0
struct IpKkt { double sd, stat, comp; bool finite, converged; };

template <int NS>
struct IpState {
  double mu, pen;
  int pen_over, pen_cuts, stall, small_steps;
  double delta_last, lm;           // last rung of the inertia ladder that was needed (0: none); Levenberg-Marquardt floor
  int nhist, hpos;                 // the non-monotone Armijo history `hist` (beside the state, see below): entries, write position,
  double hist_mu, hist_pen;        // and the ONE merit function its values belong to
  double nuT[NS];                  // multipliers of the pinned terminal states
  double mu_min;

  // The history's values, `double hist[NMMAX]`, are a local of the loop BESIDE the state: indexed at run time, as a member it kept the whole state
  // from scalar replacement (+160 bytes of private segment per kernel).  It starts uninitialised; HsFused::solve clears it (its park record holds all of it).
  MYR_POLICY void start(const HsSolveOpts& o) {
    mu = o.mu_init; pen = 1.0;
    pen_over = 0; pen_cuts = 0; stall = 0; small_steps = 0;
    delta_last = 0.0; lm = 0.0;
    nhist = 0; hpos = 0; hist_mu = -1.0; hist_pen = -1.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) nuT[i] = 0.0;
    mu_min = detail::dmin(o.tol_compl, o.tol_stat) * 0.1;
  }

  // ---- 1. inertia correction (global, as in interior-point NLP codes): retry the factorisation with W + delta I until
  // every stage pivot is positive.  First rung: the Levenberg-Marquardt floor, warm-started from the last iteration's
  // rung (skips the doomed delta = 0 attempt); ladder (IPOPT's): 1e-4 or a third of the last one, then x 100 / x 8.
  MYR_POLICY double first_delta(const HsSolveOpts& o) const {
    return (o.delta_warm && delta_last > o.delta_warm_min) ? detail::dmax(lm, delta_last / DELTA_WARM_DIV) : lm;
  }
  MYR_POLICY double next_delta(double d) const {
    return d == 0.0 ? ((delta_last > 0.0) ? detail::dmax(1e-8, delta_last / 3.0) : 1e-4) : d * ((delta_last > 0.0) ? 8.0 : 100.0);
  }
  // Does rung `tr_` give up at its first regularised pivot?  Not the last rung, and -- in the wavefront kernels -- not
  // one beyond 1e8, which keeps the stage-local convexification and ends the ladder.  (IpLoop has its own rule.)
  MYR_POLICY static bool rung_aborts(int tr_, double delta) { return (tr_ < 11) && !(delta > 1e8); }
  MYR_POLICY void close_ladder(double delta) { delta_last = (delta > lm) ? delta : 0.0; }

  // ---- 2. KKT scaling and status.  sum_mult / n_mult: every multiplier, the bounds' included.
  MYR_POLICY static IpKkt kkt(const HsSolveOpts& o, double sum_mult, int n_mult, double f, double stat_raw, double compl_max, double cinf) {
    IpKkt k;
    k.sd = n_mult > 0 ? detail::dmax(1.0, sum_mult / n_mult / 100.0) : 1.0;
    k.stat = stat_raw / k.sd; k.comp = compl_max / k.sd;
    k.finite = detail::finite_(f) && detail::finite_(cinf) && detail::finite_(stat_raw);
    k.converged = cinf <= o.tol_feas && k.stat <= o.tol_stat && k.comp <= o.tol_compl;
    return k;
  }

  // ---- 3. barrier update (monotone, superlinear): error of the barrier problem against kappa_eps times mu
  MYR_POLICY void barrier_update(const HsSolveOpts& o, const IpKkt& k, double cinf, double compl_min, double compl_max) {
    for (int guard = 0; guard < 8; ++guard) {
      // error of the barrier problem: complementarity |s*z - mu| from the extreme products
      const double cerr = (compl_min <= compl_max) ? detail::dmax(fabs(compl_max - mu), fabs(compl_min - mu)) : 0.0;
      const double emu = detail::dmax(detail::dmax(k.stat, cinf), cerr / k.sd);
      if (emu <= o.kappa_eps * mu && mu > mu_min) {
        mu = detail::dmax(mu_min, detail::dmin(o.kappa_mu * mu, pow(mu, o.theta_mu)));
      } else break;
    }
  }

  // ---- 4. l1 merit: penalty large enough to make dz a descent direction, relaxed as described at PEN_RELAX; never
  // relaxed below `floor_`.  Returns the merit function's slope along dz.
  MYR_POLICY double penalty_update(double gphi, double c1, double floor_ = 0.0) {
    if (c1 > 0.0) {
      const double need = gphi / (0.9 * c1);
      if (pen < need) pen = need + 1.0;
      if (PEN_RELAX > 0) {
        const double want = detail::dmax(2.0 * detail::dmax(need, 0.0) + 1.0, floor_);
        pen_over = (pen > PEN_RELAX_RATIO * want) ? pen_over + 1 : 0;
        if (pen_over >= PEN_RELAX && pen_cuts < PEN_RELAX_MAX) { pen = want; pen_over = 0; ++pen_cuts; }
      }
    }
    return gphi - pen * c1;
  }

  // ---- 5. non-monotone Armijo reference (Grippo-Lampariello-Lucidi): the largest of the last NM merit values of the
  // SAME merit function (history is dropped whenever mu or the penalty changes); cures Maratos-type stalls
  MYR_POLICY double merit_reference(const HsSolveOpts& o, double* hist, double phi0) {
    if (mu != hist_mu || pen != hist_pen) { nhist = 0; hpos = 0; hist_mu = mu; hist_pen = pen; }
    double phiref = phi0;
    for (int j = 0; j < nhist; ++j) phiref = detail::dmax(phiref, hist[j]);
    if (o.nonmono > 0) { hist[hpos % o.nonmono] = phi0; ++hpos; if (nhist < o.nonmono) ++nhist; }
    return phiref;
  }
  MYR_POLICY static bool accepts(double phit, double phiref, double a, double Dphi, double phi0) {
    return phit <= phiref + 1e-8 * a * Dphi + 1e-13 * fabs(phi0);
  }
  // no acceptable step along dz: take the tiny step anyway a few times (helps past round-off), then give up (status 3)
  MYR_POLICY bool stalled(bool ok) { stall = ok ? 0 : stall + 1; return stall > 5; }

  // ---- 6. after the step.  Bound multipliers follow the primal backtracking factor when asked to (keeps s*z near mu when the step is cut).
  MYR_POLICY static double dual_step(const HsSolveOpts& o, double a, double alpha_p, double alpha_d) {
    return o.dual_follow ? alpha_d * (a / alpha_p) : alpha_d;
  }
  // (terminal multiplier i, the loop at the call site: with `nu` handed over as an array the two-wavefront headline kernel spills 32 bytes more)
  MYR_POLICY void follow_nu(int i, double a, double nu_i) { nuT[i] += a * (nu_i - nuT[i]); }
  MYR_POLICY void after_step(const HsSolveOpts& o, double a, double alpha_p) {
    // step-quality feedback: a step cut hard by the line search means the quadratic model over-reaches ->
    // damp the next Newton system (W + lm I); full steps relax the damping again
    if (o.lm_init > 0.0) {
      const double ratio = o.lm_abs ? a : a / alpha_p;   // step actually taken, relative to the full Newton step
      if (ratio <= 0.25) lm = detail::dmin(1e2, detail::dmax(o.lm_init, 4.0 * lm));
      else if (ratio >= 0.99) { lm *= 0.25; if (lm < 0.1 * o.lm_init) lm = 0.0; }
    }
    // re-centering: a run of tiny accepted steps means the iterate left the neighbourhood of the central path for
    // this mu (barrier parameter reduced too early); go back up one decade instead of crawling
    if (o.recenter > 0) {
      small_steps = (a < o.recenter_alpha) ? small_steps + 1 : 0;
      if (small_steps >= o.recenter && mu < o.mu_init) { mu = detail::dmin(o.mu_init, 10.0 * mu); small_steps = 0; }
    }
  }

  // ---- 7. the record of a parked trajectory (HsFused::solve): state, history and pending step, RECORD doubles (mu_min
  // follows from the options).  Offsets: 0-11 the scalars in the order below, 12-16 the step, 17 nuT, 17 + NS hist.
  static constexpr int RECORD = 17 + NS + NMMAX;
  template <class Step>
  MYR_POLICY void save(double* sv, const double* hist, const Step& p) const {
    sv[0] = mu; sv[1] = pen; sv[2] = (double)pen_over; sv[3] = (double)pen_cuts; sv[4] = (double)stall; sv[5] = (double)small_steps;
    sv[6] = delta_last; sv[7] = lm; sv[8] = (double)nhist; sv[9] = (double)hpos; sv[10] = hist_mu; sv[11] = hist_pen;
    sv[12] = p.on ? 1.0 : 0.0; sv[13] = p.ap; sv[14] = p.ad; sv[15] = p.mu; sv[16] = p.ksig;
#pragma unroll
    for (int i = 0; i < NS; ++i) sv[17 + i] = nuT[i];
#pragma unroll
    for (int i = 0; i < NMMAX; ++i) sv[17 + NS + i] = hist[i];
  }
  template <class Step>
  MYR_POLICY void load(const double* sv, double* hist, Step& p) {
    mu = sv[0]; pen = sv[1]; pen_over = (int)sv[2]; pen_cuts = (int)sv[3]; stall = (int)sv[4]; small_steps = (int)sv[5];
    delta_last = sv[6]; lm = sv[7]; nhist = (int)sv[8]; hpos = (int)sv[9]; hist_mu = sv[10]; hist_pen = sv[11];
    p.on = sv[12] != 0.0; p.ap = sv[13]; p.ad = sv[14]; p.mu = sv[15]; p.ksig = sv[16];
#pragma unroll
    for (int i = 0; i < NS; ++i) nuT[i] = sv[17 + i];
#pragma unroll
    for (int i = 0; i < NMMAX; ++i) hist[i] = sv[17 + NS + i];
  }
};

}  // namespace myriad
