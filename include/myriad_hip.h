/*
 * myriad_hip.h -- C-ABI of libmyriad_hip.so, the MI355X (gfx950) batched trajectory-optimisation engine.
 *
 * This is the drop-in boundary for the reference's hot path (nikihowe/myriad, citations relative to
 * /root/reference/).  The reference is pure Python; the interface it would bind through ctypes is:
 *
 *   reference interface                                              entry point here
 *   --------------------------------------------------------------  ---------------------------
 *   get_optimizer(hp,cfg,system)  trajectory_optimizers/__init__.py:12-28     myr_create / myr_destroy
 *   jit(objective), jit(grad(objective)), jit(constraints),
 *   jit(jacrev(constraints))      nlp_solvers/__init__.py:32-40               myr_eval
 *   solve(hp,cfg,opt_dict) -> minimize_ipopt(...)
 *                                 nlp_solvers/__init__.py:18-98 (:57-58)      myr_solve
 *   get_state_trajectory_and_cost / get_defect   utils.py:258-324            myr_rollout
 *   Python exceptions / solution['success']      nlp_solvers/__init__.py:59-64  return codes, status[], myr_last_error
 *   jax.grad(lagrangian, argnums=0)(x, lmbda)    nlp_solvers/extra_gradient.py:21-33,
 *                                                experiments/e2e_sysid.py:113-125           myr_vjp (add_gradf=1), myr_jvp
 *   step(x, lmbda) (extragradient iteration)     nlp_solvers/extra_gradient.py:25-33        myr_exgd
 *   FBSM(hp,cfg,system).solve()                  trajectory_optimizers/forward_backward_sweep.py:88-116   myr_fbsm
 *   many_steps_grad / lookahead_update           experiments/e2e_sysid.py:148-177, 209-218  myr_exgd_grad
 *   many_steps_grad: dx/dp, dlam/dp themselves   experiments/e2e_sysid.py:148-177           myr_exgd_jac
 *   many_steps_grad / lookahead_update in the network weights
 *                                                experiments/node_e2e_sysid.py:139-166, 187-196  myr_exgd_grad_node
 *   many_steps_grad / lookahead_update under SHOOTING (the default hyperparameters)
 *                                                experiments/e2e_sysid.py:148-177, 209-218  myr_exgd_grad_shoot
 *   ... in the network weights under SHOOTING     experiments/node_e2e_sysid.py:139-166, 187-196  myr_exgd_grad_node_shoot
 *   jax.hessian / jax.jvp(jax.grad(lagrangian))  (no call site in the reference: the exact second derivative
 *                                                an external second-order method asks for)  myr_hvp
 *   ... of the network system                    (the same, in the 4 804 weights)                 myr_hvp_node
 *   jax.grad(loss)(params, minibatch), one model per call
 *                                                experiments/mle_sysid.py:89-136, neural_ode/node_training.py:31-61   myr_fit_grad
 *   ... of many independent models at once (study_scripts.py:28-43 trains one per noise level, one after the
 *                                                other; hp.num_experiments, seed sweeps)          myr_fit_grad_sets
 *   the Gauss-Newton matrix of that loss, 2 J^T W J (no call site in the reference: what a Levenberg-Marquardt fit and a
 *                                                parameter covariance ask for)                    myr_fit_gn, myr_fit_gn_sets
 *   ... its product with a vector for the network system, matrix-free (no call site in the reference: the inner
 *                                                conjugate-gradient solve of a Levenberg-Marquardt step)   myr_fit_gnvp, myr_fit_gnvp_sets
 *   many_steps_grad / the Lagrangian Hessian product of many independent networks at once (the reference's
 *                                                node_e2e_sysid.py loop trains one)               myr_exgd_grad_node_sets, myr_hvp_node_sets
 *
 * Conventions
 *   - all floating point is IEEE fp64 (the reference sets jax_enable_x64, run.py:15);
 *   - every array is caller-allocated, C-contiguous; the library never retains or frees caller memory;
 *   - `mem` says whether ALL array arguments of that call are host pointers (MYR_MEM_HOST: staged through
 *     the handle's device scratch) or device pointers on the handle's device (MYR_MEM_DEVICE: zero-copy);
 *   - per-instance arrays are instance-major: z[B][n] uses exactly the reference's ravel_pytree layout
 *     per instance (states row-major first, then controls);
 *   - calls block until the result is complete; a handle is not thread-safe;
 *   - functions return 0 on success, <0 on error (myr_last_error() gives the thread-local message);
 *     non-convergence is NOT an error (as in the reference): it is reported per instance in status[].
 */
#ifndef MYRIAD_HIP_H
#define MYRIAD_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* system ids: members of myriad.systems.SystemType on the hot path (systems/__init__.py:29-50) */
enum { MYR_SYS_CARTPOLE = 0, MYR_SYS_VANDERPOL = 1, MYR_SYS_CANCERTREATMENT = 2, MYR_SYS_SIMPLECASE = 3,
       /* NodeSystem over CARTPOLE with a (64,64) sigmoid MLP (systems/neural_ode/node_system.py:14-42,
          neural_ode/create_node.py:110-117): params = the 4804 weights, see csrc/node_system.h for the order */
       MYR_SYS_NODE_CARTPOLE = 4,
       /* further autonomous systems without terminal cost (systems/lenhart/<name>.py, miscellaneous/seir.py) */
       MYR_SYS_BIOREACTOR = 5, MYR_SYS_GLUCOSE = 6, MYR_SYS_MOULDFUNGICIDE = 7, MYR_SYS_SIMPLECASEWITHBOUNDS = 8,
       MYR_SYS_HIVTREATMENT = 9, MYR_SYS_EPIDEMICSEIRN = 10, MYR_SYS_SEIR = 11, MYR_SYS_BEARPOPULATIONS = 12,
       /* classical_control/{pendulum,mountain_car}.py (gym-style clips kept), miscellaneous/rocket_landing.py */
       MYR_SYS_PENDULUM = 13, MYR_SYS_MOUNTAINCAR = 14, MYR_SYS_ROCKETLANDING = 15,
       /* systems with a (linear) terminal cost: lenhart/bacteria.py, miscellaneous/tumour.py.  The terminal
          term is applied where the reference applies it for collocation -- the TRAPEZOIDAL objective (trapezoidal.py:126-127)
          the rollout (utils.py:295-296) and, on the integrated end state of the last interval, the SHOOTING objective
          (shooting.py:206-208); not the Hermite-Simpson objective */
       MYR_SYS_BACTERIA = 16, MYR_SYS_TUMOUR = 17,
       /* running cost g(x,u,t) with explicit time (lenhart/harvest.py:61-62, timber_harvest.py:84-85): every transcription
          evaluates it at the reference's point / step times */
       MYR_SYS_HARVEST = 18, MYR_SYS_TIMBERHARVEST = 19,
       /* lenhart/predator_prey.py: terminal cost and ONE pinned terminal state (x_T = [None, None, B]) */
       MYR_SYS_PREDATORPREY = 20,
       /* ELASTIC twins (100 + id; no counterpart in the reference -- the feasibility-restoration device of the solver, DESIGN.md
          "Elastic mode"): x' = f(x,u) + s with NS slack controls s appended to u and the running cost g + rho/2 |s|^2, rho the
          LAST model parameter.  All entry points work on them like on any system (NU = nu + ns controls), except myr_solve under
          MYR_TR_SHOOTING (every twin): MYR_E_UNSUPPORTED, "... built for the collocation transcriptions".  (Up to round 4 ROCKETLANDING's
          twin had no trapezoidal solver either.)  Every system with pinned terminal states has one (round 4).
          Under myr_set_var_scale a twin does NOT solve the same problem in other variables: its penalty is rho/2 sum_i (s_i / sc_i)^2,
          sc_i the scale entry of slack i (entry ns + nu + i of the twin's vector) -- every slack is weighed against the magnitude the
          caller states for it.  The library's own elastic phase (myr_solve_opts.restoration) gives each slack the scale of its state.
          With unit scales, and in every entry point but the scaled solve, the penalty is rho/2 |s|^2. */
       MYR_SYS_CARTPOLE_ELASTIC = 100, MYR_SYS_VANDERPOL_ELASTIC = 101, MYR_SYS_PENDULUM_ELASTIC = 113, MYR_SYS_MOUNTAINCAR_ELASTIC = 114,
       MYR_SYS_ROCKETLANDING_ELASTIC = 115,
       /* lenhart/invasive_plant.py: DISCRETE-time (five foci, five controls).  Only myr_fbsm (its discrete recurrences)
          accepts it; the direct-transcription entry points return MYR_E_UNSUPPORTED, as the reference's direct optimisers
          raise NotImplementedError for it (trajectory_optimizers/base.py:66-67) */
       MYR_SYS_INVASIVEPLANT = 21 };
/* transcription: OptimizerType x QuadratureRule (config.py:12-57) */
enum { MYR_TR_HERMITE_SIMPSON = 0, MYR_TR_TRAPEZOIDAL = 1, MYR_TR_SHOOTING = 2 };
/* IntegrationMethod (config.py:46-50) */
enum { MYR_INT_EULER = 0, MYR_INT_HEUN = 1, MYR_INT_MIDPOINT = 2, MYR_INT_RK4 = 3 };
enum { MYR_MEM_HOST = 0, MYR_MEM_DEVICE = 1 };
/* per-instance solve status */
enum { MYR_STATUS_CONVERGED = 0, MYR_STATUS_MAXITER = 1, MYR_STATUS_NAN = 2, MYR_STATUS_STALLED = 3,
       /* never written by myr_solve itself: the verdict of the host's elastic phase ("Elastic mode") on an instance
          whose elastic twin converges with a slack that does not vanish as its penalty grows */
       MYR_STATUS_INFEASIBLE = 4 };
/* kernel ids for myr_kernel_time */
enum { MYR_K_EVAL = 0, MYR_K_SOLVE = 1, MYR_K_ROLLOUT = 2, MYR_K_RESID = 3, MYR_K_PROD = 4, MYR_K_FBSM = 5, MYR_K_FIT = 6,
       MYR_K_HVP_NODE = 7, MYR_K_HVP_NODE_SHOOT = 8,      /* myr_hvp_node: the Hermite-Simpson kernel / the SHOOTING kernel (each with its batch sum) */
       MYR_K_COUNT = 9 };
/* error codes */
enum { MYR_OK = 0, MYR_E_ARG = -1, MYR_E_UNSUPPORTED = -2, MYR_E_HIP = -3, MYR_E_CAPACITY = -4 };

typedef struct myr_handle_s* myr_handle;

typedef struct {
  int32_t system_id;             /* MYR_SYS_*                                         */
  int32_t transcription;         /* MYR_TR_*                                          */
  int32_t integration_method;    /* MYR_INT_* (shooting + rollout)                    */
  int32_t intervals;             /* hp.intervals                                      */
  int32_t controls_per_interval; /* hp.controls_per_interval (1 for collocation)      */
  int32_t device;                /* HIP device ordinal                                */
  int32_t max_batch;             /* HINT: batch the handle pre-sizes its scratch for; larger batches are accepted
                                    (scratch grows on demand, MYR_E_HIP if the device cannot hold it)          */
  int32_t reserved;
  double  T;                     /* horizon system.T                                  */
} myr_problem_desc;

typedef struct {
  int32_t n;        /* decision variables per instance                                  */
  int32_t m;        /* equality constraints per instance                                */
  int32_t ns, nu, np;
  int32_t x_rows, u_rows;   /* rows of the unravelled (xs, us)                          */
  int32_t jblk;     /* doubles of stage-block Jacobian per instance (see myr_eval)      */
  int32_t ngrad;    /* doubles of objective-gradient output per instance (see myr_eval) */
  int32_t reserved;
} myr_dims;

typedef struct {
  int32_t max_iter;     /* hp.max_iter (config.py:70): bounds the iterations of ONE attempt   */
  int32_t restarts;     /* attempts after a first one that ends without a KKT point: -1 = the library's default (2 for the
                           shooting wavefront kernel, 0 for every other kernel), 0 = a single attempt of at most max_iter
                           iterations -- `iters` <= max_iter then holds --, k > 0 = up to k more (at most 4).  With restarts
                           the first attempt is cut at max(100, max_iter / 8) iterations, a restart takes the caller's point
                           again with another initial barrier parameter (mu_init x 3, / 3, x 9, / 9: a different one per attempt) and the full max_iter, and
                           `iters` reports the sum over the attempts.  Only the shooting wavefront kernel restarts; the lane
                           kernels (MYRIAD_SOLVE_MODE=lane, iterates too large for LDS) ignore the field. */
  double  tol_feas;     /* converged: max|c| <= tol_feas                  (default 1e-8)  */
  double  tol_stat;     /* converged: scaled ||grad f + J^T lam - zL + zU||_inf <= tol_stat (1e-6) */
  double  tol_compl;    /* converged: complementarity <= tol_compl        (default 1e-7)  */
  double  mu_init;      /* initial barrier parameter                      (default 0.1)   */
  int32_t restoration;  /* what stands in for IPOPT's feasibility-restoration phase (the reference gets it from inside the one
                           minimize_ipopt call, nlp_solvers/__init__.py:57-58), applied INSIDE myr_solve / myr_solve_x0 to the
                           instances the first attempt leaves without a KKT point -- a bit mask:
                             1  elastic phase: the instance is solved on the system's ELASTIC TWIN (x' = f(x,u) + s, cost
                                g + rho/2 |s|^2; systems listed above as *_ELASTIC, collocation transcriptions) for rho = 1,
                                1e2, 1e4, each from the previous solution, and the twin's trajectory starts the problem itself;
                                a twin that converges with a slack that neither vanishes (> 1e-3) nor shrinks (> 1/10 of its
                                value at the previous rho) marks the instance MYR_STATUS_INFEASIBLE;
                             2  second starts: excitation guesses -- controls u(t) = centre + 0.95 amp sin(2 pi c t / T) over
                                the control bounds, states by a rollout of the true dynamics -- for c = 2, 3, 5 cycles, first
                                success wins;
                           0 = one attempt from the caller's point and nothing else (the reference's call, minus IPOPT's own
                           restoration); -1 = the library's default (3; the environment variables MYRIAD_ELASTIC=0 /
                           MYRIAD_SECOND_STARTS=0 clear the bits, MYRIAD_SECOND_STARTS="2,7" sets other cycle counts).
                           `iters` then sums the attempts of an instance; myr_solve_info reports which start produced it. */
  int32_t park_iter;    /* two-phase launch of the one-wavefront collocation kernel (a scheduling matter: the iterates of an instance
                           are the same, bit for bit).  A batch much larger than the number of resident wavefronts runs as several
                           whole solves per wavefront and ends with the wavefronts that drew the long solves last; instead every
                           instance first gets `park_iter` iterations, the unfinished ones are parked (40 KB each) and resumed
                           longest-first by their residuals at that point (a wavefront that finds no fresh instance keeps iterating the one
                           it holds until every instance has had its `park_iter` iterations, and parks it there).  0 = the library decides (Hermite-Simpson, closed-form systems: 8 / 10 /
                           12 iterations from 1.5 / 2 / 3 solves per resident wavefront on; whole solves otherwise; MYRIAD_PARK_ITER overrides), -1 = whole
                           solves, k > 0 = k iterations (an explicit k > 0 also selects the one-wavefront form for small batches, which the
                           library would otherwise give two wavefronts per trajectory: the two-wavefront form has no parking).  Needs the
                           per-instance `status` and `kkt` outputs; ignored by the other kernels. */
} myr_solve_opts;

int myr_create(const myr_problem_desc* desc, myr_handle* out);
int myr_destroy(myr_handle h);
int myr_get_dims(myr_handle h, myr_dims* out);
void myr_default_solve_opts(myr_solve_opts* o);

/*
 * Evaluate the transcription at B decision vectors: replaces the four jitted callbacks of
 * nlp_solvers/__init__.py:32-40 for B instances at once.
 *   z      [B][n]      in
 *   params [B][np] if params_stride==np, or [np] shared if params_stride==0; NULL = system defaults
 *   f      [B]         out  objective
 *   gradf  [B][ngrad]  out  d f / d z.  If the system's running cost does not depend on x (CARTPOLE)
 *                           only the control part is stored (ngrad = u_rows*nu, the non-zeros);
 *                           otherwise ngrad = n in z layout.
 *   c      [B][m]      out  constraints, reference row order
 *   jblk   [B][jblk]   out  constraint Jacobian as stage blocks.  HERMITE_SIMPSON: per interval k,
 *                           row-major blocks  Dxs,Dxm,Dxe (ns x ns), Dus,Dum,Due (ns x nu)  [defect rows]
 *                           then              Ixs,Ixe (ns x ns), Ius,Iue (ns x nu)           [interp rows];
 *                           the identity d interp / d x_m is implied and not stored
 *                           (jblk = N*(5 ns^2 + 5 ns nu)).
 *                           TRAPEZOIDAL: per interval  Cxs = h/2 A_s + I, Cxe = h/2 A_e - I (ns x ns),
 *                           Cus = h/2 B_s, Cue = h/2 B_e (ns x nu)   (jblk = N*(2 ns^2 + 2 ns nu)).
 *                           SHOOTING: per interval  Jx = d c_k/d x_k (ns x ns), then Ju = d c_k / d (the interval's control
 *                           rows) (ns x (mc cpi + 1) nu, mc = 2 for RK4 else 1); d c_k/d x_{k+1} = -I implied;
 *                           gradf is the full gradient (ngrad = n).
 * Any output pointer may be NULL to skip it.
 */
int myr_eval(myr_handle h, int32_t B, const double* z, const double* params, int32_t params_stride,
             double* f, double* gradf, double* c, double* jblk, int32_t mem);

/*
 * Solve B independent NLP instances (replaces the minimize_ipopt call, nlp_solvers/__init__.py:57-58).
 *   z      [B][n]  in: initial guess (reference rule: linspace(x0,xT) / zeros)   out: solution
 *   lb,ub  [B][n]  bounds per instance (lb==ub pins a variable, e.g. x[0]=x0, x[-1]=x_T;
 *                  +-inf allowed)
 *   lam    [B][m]  out: equality multipliers, sign convention of scipy/ipopt `mult_g`
 *                  (stationarity: grad f + J^T lam - zL + zU = 0)
 *   cost   [B]     out: objective at the solution
 *   status [B], iters [B]  out (int32): MYR_STATUS_* per instance (non-convergence is a status, never an error return);
 *                  iterations spent.  SHOOTING on the wavefront kernel gives the first start max(100, max_iter / 8) iterations
 *                  and restarts a solve that ended without a KKT point from the caller's point with another initial barrier
 *                  parameter (x3, then /3, each with the full max_iter): `iters` sums the attempts and may exceed max_iter.
 *   kkt    [B][3]  out (may be NULL): final {max|c|, stationarity, complementarity}
 * Restoration (myr_solve_opts.restoration, on by default): instances the first attempt leaves without a KKT point go through the
 * elastic phase and the second starts described at the field, inside this call; a converged instance is never touched.
 */
int myr_solve(myr_handle h, int32_t B, double* z, const double* lb, const double* ub,
              const double* params, int32_t params_stride, const myr_solve_opts* opts,
              double* lam, double* cost, int32_t* status, int32_t* iters, double* kkt, int32_t mem);

/*
 * Per-instance account of the LAST myr_solve / myr_solve_x0 call on this handle (HOST arrays of B int32 each, any may be NULL):
 *   start    0 = the caller's point produced the returned result, c > 0 = the excitation guess with c cycles
 *   attempts device solves the instance went through (1 = the first attempt only; the elastic phase counts 4: three twin solves
 *            and the solve of the problem itself)
 *   restored 1 = the returned result comes out of the elastic phase
 * B must be the batch size of that call.
 */
int myr_solve_info(myr_handle h, int32_t B, int32_t* start, int32_t* attempts, int32_t* restored);

/*
 * How the library ran the FIRST attempt of the last myr_solve / myr_solve_x0 call on this handle (a scheduling matter: no entry changes a result).
 * One source of truth for what a measurement says about its own launch (bench.py used to restate the library's rules).  plan[8]:
 *   [0] kernel form: 0 one trajectory per lane, 1 fused-phase wavefront kernel, 2 round-2 wavefront kernel, 3 shooting wavefront kernel
 *   [1] wavefronts per trajectory            [2] iterations of phase 1 of the two-phase launch (0 = whole solves)
 *   [3] solver-kernel launches per solve     [4] resident trajectory slots of the launch
 *   [5] helper workgroups per trajectory at most (network kernel; 0 = none)     [6], [7] reserved (0)
 */
int myr_solve_plan(myr_handle h, int32_t* plan);

/*
 * myr_solve for B instances that differ in their START STATE only (EXTENSION; the reference builds guess and bounds of an
 * instance from system.x_0 in the optimiser's constructor: collocation/hermite_simpson.py:37-48 (guess), :55-81 (bounds);
 * collocation/trapezoidal.py:36-50, 55-77; shooting.py:56-74, 247-275 -- this entry point applies that constructor to B start
 * states ON THE DEVICE, so a caller sends B x ns doubles instead of three [B][n] arrays).
 *   x0s    [B][ns]  start states
 *   g0,g1  [n]      guess rule: z0[b][i] = g0[i] + g1[i] * x0s[b][i mod ns] for the state entries (i < x_rows*ns: the product and
 *                   the sum are rounded separately, i.e. bit for bit numpy's x0*(1-lin) + x_T*lin with g1 = 1-lin, g0 = x_T*lin),
 *                   z0[b][i] = g0[i] for the controls.  A guess that does not depend on x0 (ones*0.1) has g1 = 0.
 *   lb,ub  [n]      bounds shared by the instances; the first point's state entries (i < ns) are replaced by x0s[b] (x[0] = x0)
 *   z      [B][n]   out: solutions (NOT read on entry)
 *   params, opts, lam, cost, status, iters, kkt, mem: as myr_solve.  MYR_MEM_DEVICE: every pointer is a device pointer.
 * Results are those of myr_solve on the expanded arrays (tests/test_gpu_solve.py::test_solve_x0_matches_solve).
 */
int myr_solve_x0(myr_handle h, int32_t B, const double* x0s, const double* g0, const double* g1, const double* lb,
                 const double* ub, const double* params, int32_t params_stride, const myr_solve_opts* opts,
                 double* z, double* lam, double* cost, int32_t* status, int32_t* iters, double* kkt, int32_t mem);

/*
 * Variable scaling of the SOLVE path.  scale [ns+nu] (states, then controls; NULL = all 1): myr_solve then works on
 * z/s, lb/s, ub/s with the dynamics f(s x)/s -- the same optimisation problem in better-conditioned variables (IPOPT's
 * user scaling, which the reference reaches through `nlp_scaling_method`); inputs and outputs of myr_solve stay in the
 * ORIGINAL variables (z, lam) except kkt[][0], the constraint violation, which is measured in scaled states.
 * Not available for NODE systems.  Power-of-two scales make the change of variables exact in floating point.
 * The *_ELASTIC twins are the exception to "the same problem": their slack penalty is written in the scaled variables,
 * rho/2 sum_i (s_i / sc_i)^2 with sc_i the scale entry of slack i, so on a twin handle the scale changes the problem that is
 * solved (the cost returned is that weighted cost).  The elastic phase of the restoration sets each slack's entry to the scale of
 * its state.  A refused vector (MYR_E_ARG) changes nothing: the scales set before stay in force.
 */
int myr_set_var_scale(myr_handle h, const double* scale);

/*
 * True-dynamics rollout under given controls (utils.py:258-298) + terminal state.
 *   x0 [B][ns], us [B][u_rows_rollout][nu]  ->  xs [B][num_steps+1][ns] (may be NULL), cost [B]
 *   u_rows_rollout = (RK4 ? 2 : 1)*num_steps + 1 consumed entries (reference indexing utils.py:57-65).
 */
int myr_rollout(myr_handle h, int32_t B, int32_t num_steps, int32_t u_rows, const double* x0, const double* us,
                const double* params, int32_t params_stride, double* xs, double* cost, int32_t mem);

/*
 * Matrix-free products with the constraint Jacobian -- what jax.grad(lagrangian) computes through the dense transcription in
 * nlp_solvers/extra_gradient.py:21-33 and experiments/e2e_sysid.py:113-141.
 *   myr_vjp:  out[B][n] = J(z)^T lam   (+ grad f(z) when add_gradf != 0: the gradient of the Lagrangian in z)
 *   myr_jvp:  out[B][m] = J(z) v
 * z [B][n], lam [B][m], v [B][n]; layouts and row order as in myr_eval.  Collocation: pointwise / intervalwise kernels;
 * SHOOTING (EULER, HEUN, MIDPOINT, RK4 -- whatever hp.integration_method selects, utils.py:91-96, shooting.py:230-241): reverse
 * sweep seeded with lam / forward tangents through the steps (RK4: two control rows per step, u[2i], u[2i+1], u[2i+2]).
 * MYR_SYS_NODE_CARTPOLE (library version 0.7): HERMITE_SIMPSON and SHOOTING with all four integration rules; params required,
 * params_stride 0 or np; MYR_TR_TRAPEZOIDAL is MYR_E_UNSUPPORTED.  Under SHOOTING a lane holds one (instance, interval) pair and the 64
 * lanes of a wavefront pairs of different instances, so that a network pass fills up to four 16-point matrix-core tiles
 * (csrc/node_shoot_products.h); a workgroup owns whole instances (params_stride == np: one).  How many depends on intervals,
 * controls_per_interval and params_stride only: an instance's result has the same bits whatever its batch.  MYR_E_CAPACITY beyond
 * ~12 000 intervals.
 */
int myr_vjp(myr_handle h, int32_t B, const double* z, const double* lam, const double* params, int32_t params_stride,
            double* out, int32_t add_gradf, int32_t mem);
int myr_jvp(myr_handle h, int32_t B, const double* z, const double* v, const double* params, int32_t params_stride,
            double* out, int32_t mem);

/*
 * `nsteps` extragradient iterations on B instances, iterate resident on the device (extra_gradient.py:25-33):
 *   x_bar = clip(x - eta_x dL/dx(x, lam), lb, ub);  x_new = clip(x - eta_x dL/dx(x_bar, lam), lb, ub);
 *   lam_new = lam + eta_v c(x_new)
 * z [B][n] and lam [B][m] are updated in place; lb, ub [B][n].
 * MYR_SYS_NODE_CARTPOLE under SHOOTING (version 0.7): ONE launch for the whole call -- the workgroup that owns an instance loops over the steps
 * with z, x_bar, the gradient and lam in LDS (in the handle's global scratch where one instance does not fit); coverage and packing as myr_vjp.
 */
int myr_exgd(myr_handle h, int32_t B, double* z, double* lam, const double* lb, const double* ub, const double* params,
             int32_t params_stride, double eta_x, double eta_v, int32_t nsteps, int32_t mem);

/*
 * Batched Forward-Backward Sweep, the reference's indirect solver (trajectory_optimizers/forward_backward_sweep.py:20-116;
 * RK4 sweeps utils.py:138-197; stopping rule trajectory_optimizers/base.py:128-141) for B instances of the handle's
 * system.  Built for all fourteen IndirectFHCS systems: SIMPLECASE, CANCERTREATMENT, BACTERIA, BEARPOPULATIONS, BIOREACTOR,
 * EPIDEMICSEIRN, GLUCOSE, HARVEST, HIVTREATMENT, MOULDFUNGICIDE, SIMPLECASEWITHBOUNDS, TIMBERHARVEST, PREDATORPREY, and the
 * discrete-time INVASIVEPLANT (others return MYR_E_UNSUPPORTED).  The secant `sequencesolver` for a terminal state
 * condition (PREDATORPREY) is a host loop over this call with different adj_T.  The handle's transcription is not used.
 * Discrete systems (forward_backward_sweep.py:33-41, utils.py:184-188): N = int(T) unit steps, direct recurrences instead
 * of RK4, `us` is [B][N][nu] (one control row per step) and `params` is required.
 *   N = hp.fbsm_intervals; x0 [B][ns]; adj_T [ns] or NULL (= 0); params as in myr_eval;
 *   clip_lo / clip_hi [nu]: the bounds each control's optim_characterization is clipped with (+-inf = not clipped);
 *   bang: max|bounds[-1]| for the bang-bang characterisations; delta: stopping tolerance (0.001)
 *   xs, adjs [B][N+1][ns], us [B][N+1][nu], sweeps [B] (may be NULL).  Host arrays only.
 */
int myr_fbsm(myr_handle h, int32_t B, int32_t N, const double* x0, const double* adj_T, const double* params,
             int32_t params_stride, const double* clip_lo, const double* clip_hi, double bang, double delta,
             int32_t max_sweeps, double* xs, double* us, double* adjs, int32_t* sweeps, int32_t mem);

/*
 * Trajectory-matching loss and its gradient in the model parameters (experiments/mle_sysid.py:89-136,
 * neural_ode/node_training.py:31-61): for each of B recorded trajectories, integrate its controls from its first recorded state with the
 * handle's integration_method and h = T / num_steps (the steps of myr_rollout: utils.py:80-131, control rows beyond u_rows clamp to the
 * last one), and take
 *   loss[b] = sum_{t=0..num_steps} wt[t] * sum_i (xh_b[t][i] - xs_obs_b[t][i])^2,      grad[b][k] = d loss[b] / d params[k]
 * by one forward rollout and one reverse sweep on the device.
 *   xs_obs [B][num_steps+1][ns]; us [B][u_rows][nu]; wt [num_steps+1] or NULL (= 1);
 *   params as in myr_rollout (NULL = the system's defaults; NODE: required, params_stride 0 only); loss [B] (may be NULL);
 *   grad [B][np] if grad_stride == np, [np] = sum over the batch if grad_stride == 0.
 * The sum over the batch runs in a fixed order without atomics: the same bits on every call, for MYR_MEM_HOST and MYR_MEM_DEVICE alike.
 * A parameter that enters the running cost only has gradient 0.  MYR_E_UNSUPPORTED: INVASIVEPLANT, the elastic twins (fit the system
 * itself), per-instance NODE weights; MYR_E_ARG: a grad_stride or params_stride other than 0 and np, bad sizes.
 */
int myr_fit_grad(myr_handle h, int32_t B, int32_t num_steps, int32_t u_rows, const double* xs_obs, const double* us,
                 const double* wt, const double* params, int32_t params_stride,
                 double* loss, double* grad, int32_t grad_stride, int32_t mem);

/*
 * myr_fit_grad for E independent parameter sets (models) of R trajectories each, in one call (library version 0.10): ensembles over noise
 * levels, seeds or initialisations of one architecture on data of one shape.
 *   params [E][np], required (NODE: the 4 804 weights per set, in the order of csrc/node_system.h);
 *   data_shared == 0: xs_obs [E][R][num_steps+1][ns], us [E][R][u_rows][nu];
 *   data_shared == 1: xs_obs [R][num_steps+1][ns], us [R][u_rows][nu], read by every set (an ensemble over initialisations on one minibatch);
 *   wt [num_steps+1] or NULL (= 1), shared by all sets; loss [E][R] or NULL;
 *   grad [E][R][np] if grad_stride == np; [E][np] if grad_stride == 0: per set, the fixed-order sum over that set's R rows; NULL: the loss
 *   only -- the reverse sweep is not run (validation and recorded losses).  loss and grad must not both be NULL.
 * Contract: for every set e the outputs of set e have the bits of myr_fit_grad(h, R, ..., that set's data, wt, params + e * np, 0, ...,
 * grad_stride, mem) on that set alone -- for MYR_MEM_HOST and MYR_MEM_DEVICE, on every call, whatever E is and whatever ran on the handle
 * before.  The per-set sum runs in myr_fit_grad's order over the set's own row index, without atomics.
 * When the rows behind the per-set sums (E * R * np doubles of scratch) would pass 1 GiB the call runs in chunks of whole sets, at least one
 * set each, with the state scratch sized for one chunk; chunked and unchunked runs give the same bits.  MYRIAD_FIT_ROWS_BYTES, read at call
 * time, lowers that bound (tests).  Timed on MYR_K_FIT.
 * Errors, in this order: MYR_E_ARG -- a null h, xs_obs, us or params; loss and grad both NULL; E < 0, R < 1, num_steps < 1, u_rows < 1; a
 * grad_stride other than 0 and np; a data_shared other than 0 and 1; a bad mem.  MYR_E_UNSUPPORTED, with myr_fit_grad's messages --
 * INVASIVEPLANT, the elastic twins, systems without generated parameter derivatives.  E == 0 writes nothing and returns MYR_OK.
 */
int myr_fit_grad_sets(myr_handle h, int32_t E, int32_t R, int32_t num_steps, int32_t u_rows, const double* xs_obs, const double* us,
                      int32_t data_shared, const double* wt, const double* params, double* loss, double* grad, int32_t grad_stride,
                      int32_t mem);

/*
 * myr_fit_grad's loss and gradient together with the Gauss-Newton matrix of the fit, by forward sensitivities in one pass on the device
 * (csrc/fit_gn.h; an extension with no call site in the reference -- what a Gauss-Newton / Levenberg-Marquardt fit solves with, and the
 * Fisher information of the fit).  With r_b[t] = xh_b[t] - xs_obs_b[t] and S_b[t] = d xh_b[t] / d params [ns][np]:
 *   loss[b] = sum_t wt[t] |r_b[t]|^2,   grad[b] = 2 sum_t wt[t] S_b[t]^T r_b[t],   gn[b] = 2 sum_t wt[t] S_b[t]^T S_b[t]
 * so that loss(params + d) = loss + grad . d + d . gn d / 2 to second order in d (to first order in the residuals).  gn[b] is symmetric to the
 * bit and positive semidefinite; a parameter that enters the running cost only has a 0 in grad and a row and column of 0 in gn.
 *   xs_obs, us, wt, params, params_stride, loss: as in myr_fit_grad (closed-form systems; params NULL = the defaults);
 *   out_stride == np: grad [B][np] (may be NULL), gn [B][np][np];
 *   out_stride == 0:  grad [np] (may be NULL), gn [np][np]: the sums over the batch, in myr_fit_grad's fixed order, without atomics.
 * gn is required.  Contract: the same bits for MYR_MEM_HOST and MYR_MEM_DEVICE, on every call, whatever ran on the handle before, with
 * loss or grad NULL or not; row b of a batched call has the bits of the call on trajectory b alone.  Timed on MYR_K_FIT.  Detected by the export: myr_version() is unchanged.
 * Errors, in this order: MYR_E_ARG -- a null h, xs_obs, us or gn; B < 0, num_steps < 1, u_rows < 1; an out_stride or params_stride other
 * than 0 and np; a bad mem.  MYR_E_UNSUPPORTED -- the network system (its 4 804 x 4 804 matrix is not formed: use myr_fit_grad); then,
 * with myr_fit_grad's messages, the elastic twins, INVASIVEPLANT, systems without generated parameter derivatives.  B == 0 writes
 * nothing and returns MYR_OK.
 */
int myr_fit_gn(myr_handle h, int32_t B, int32_t num_steps, int32_t u_rows, const double* xs_obs, const double* us,
               const double* wt, const double* params, int32_t params_stride,
               double* loss, double* grad, double* gn, int32_t out_stride, int32_t mem);

/*
 * myr_fit_gn for E independent parameter sets of R trajectories each, in one call: the lockstep iterations of many Levenberg-Marquardt fits.
 *   inputs as in myr_fit_grad_sets (params [E][np] required; data_shared 0 / 1); loss [E][R] or NULL;
 *   out_stride == np: grad [E][R][np] (may be NULL), gn [E][R][np][np];
 *   out_stride == 0:  grad [E][np] (may be NULL), gn [E][np][np]: per set, the fixed-order sums over that set's R rows.
 * Contract: the outputs of set e have the bits of myr_fit_gn on that set alone, as myr_fit_grad_sets' have myr_fit_grad's.  When the rows
 * behind the per-set sums (E * R * (np + np^2) doubles of scratch) would pass 1 GiB the call runs in chunks of whole sets with the same bits;
 * MYRIAD_FIT_ROWS_BYTES lowers that bound (tests).
 * Errors, in this order: MYR_E_ARG -- a null h, xs_obs, us, gn or params; E < 0, R < 1, num_steps < 1, u_rows < 1; an out_stride other than
 * 0 and np; a data_shared other than 0 and 1; a bad mem.  MYR_E_UNSUPPORTED as myr_fit_gn.  E == 0 writes nothing and returns MYR_OK.
 */
int myr_fit_gn_sets(myr_handle h, int32_t E, int32_t R, int32_t num_steps, int32_t u_rows, const double* xs_obs, const double* us,
                    int32_t data_shared, const double* wt, const double* params,
                    double* loss, double* grad, double* gn, int32_t out_stride, int32_t mem);

/*
 * The Gauss-Newton product of the network fit, matrix-free (csrc/fit.h: node_fit_gnvp_kernel): what a conjugate-gradient Levenberg-Marquardt step
 * multiplies with where myr_fit_gn's 4 804 x 4 804 matrix is not formed.  With S_b[t] = d xh_b[t] / d params [ns][np], the S of myr_fit_gn:
 *   jv[b][t] = S_b[t] v                          [B][num_steps+1][ns], may be NULL; row t = 0 is exactly 0
 *   out[b]   = 2 sum_t wt[t] S_b[t]^T S_b[t] v   myr_fit_gn's gn[b] times v, with the same factor 2
 * by a forward tangent rollout and myr_fit_grad's reverse sweep with 2 wt[t] jv[b][t] in the place of the residual's cotangent.
 *   xs_obs, us, wt: as in myr_fit_grad; xs_obs supplies only the start states xs_obs[b][0] (the product does not depend on the residuals: the
 *   argument stays so that the call takes the arrays of the fit calls unchanged);
 *   params [np], v [np]: both required;
 *   out_stride == np: out [B][np]; out_stride == 0: out [np], the sum over the batch in myr_fit_grad's fixed order, without atomics;
 *   out may be NULL: only the forward tangent runs.  jv and out must not both be NULL.
 * Contract: the same bits for MYR_MEM_HOST and MYR_MEM_DEVICE, on every call, whatever ran on the handle before, with jv NULL or not; row b of a
 * batched call has the bits of the call on trajectory b alone.  Timed on MYR_K_FIT.  Detected by the export: myr_version() is unchanged.
 * Errors, in this order: MYR_E_ARG -- a null h, xs_obs, us, params or v; jv and out both NULL; B < 0, num_steps < 1, u_rows < 1; an out_stride
 * other than 0 and np; a bad mem.  MYR_E_UNSUPPORTED -- every handle that is not the network system (use myr_fit_gn, which forms gn, and
 * multiply).  B == 0 writes nothing and returns MYR_OK.
 */
int myr_fit_gnvp(myr_handle h, int32_t B, int32_t num_steps, int32_t u_rows, const double* xs_obs, const double* us,
                 const double* wt, const double* params, const double* v, double* jv, double* out, int32_t out_stride, int32_t mem);

/*
 * myr_fit_gnvp for E independent weight sets of R trajectories each, in one call: the lockstep conjugate-gradient iterations of an ensemble.
 *   data as in myr_fit_grad_sets (data_shared 0 / 1); params [E][np] and v [E][np] (one direction per set), both required;
 *   jv [E][R][num_steps+1][ns] or NULL; out [E][R][np] if out_stride == np, [E][np] -- per set, the fixed-order sum over its R rows -- if
 *   out_stride == 0, or NULL.
 * Contract: set e has the bits of myr_fit_gnvp on that set alone.  When the rows behind the per-set sums (E * R * np doubles of scratch) would
 * pass 1 GiB the call runs in chunks of whole sets with the same bits; MYRIAD_FIT_ROWS_BYTES lowers that bound (tests).
 * Errors, in this order: MYR_E_ARG -- a null h, xs_obs, us, params or v; jv and out both NULL; E < 0, R < 1, num_steps < 1, u_rows < 1, E * R
 * not an int; an out_stride other than 0 and np; a data_shared other than 0 and 1; a bad mem.  MYR_E_UNSUPPORTED as myr_fit_gnvp.  E == 0
 * writes nothing and returns MYR_OK.
 */
int myr_fit_gnvp_sets(myr_handle h, int32_t E, int32_t R, int32_t num_steps, int32_t u_rows, const double* xs_obs, const double* us,
                      int32_t data_shared, const double* wt, const double* params, const double* v,
                      double* jv, double* out, int32_t out_stride, int32_t mem);

/*
 * Derivative of `nsteps` extragradient steps (myr_exgd) in the model parameters, by one reverse sweep through the steps on the device
 * (experiments/e2e_sysid.py:148-177 carries dz/dp, dlam/dp forward from a starting point held fixed; this is the same derivative, contracted
 * with a seed, for any number of parameters; library version 0.3).  With (z_n, lam_n) the iterate after `nsteps` steps from (z, lam):
 *   grad[b][k] = seed_z[b] . d z_n / d params[k] + seed_lam[b] . d lam_n / d params[k]
 *   dz0[b] = (d z_n / d z)^T seed_z[b] + (d lam_n / d z)^T seed_lam[b],   dlam0[b] likewise in lam.
 * A variable that a step leaves on a bound (and a pinned one, lb == ub) passes nothing on.
 *   z [B][n], lam [B][m] (not modified); lb, ub [B][n]; params, eta_x, eta_v, nsteps as in myr_exgd; seed_z [B][n]; seed_lam [B][m] or NULL (= 0);
 *   grad [B][np] if grad_stride == np, [np] = sum over the batch if grad_stride == 0 (fixed order, no atomics: the same bits on every
 *   call, for MYR_MEM_HOST and MYR_MEM_DEVICE alike); dz0 [B][n] or NULL; dlam0 [B][m] or NULL.
 * nsteps == 0 gives grad = 0, dz0 = seed_z, dlam0 = seed_lam.  The steps' history (nsteps (2 n + m) + n doubles per instance) lives in the
 * handle's scratch; a batch whose history would pass 1 GiB runs in chunks of instances.
 * MYR_E_UNSUPPORTED: SHOOTING, the network system, the elastic twins, INVASIVEPLANT; MYR_E_CAPACITY: the reverse sweep's
 * (3 n + 2 m + x_rows ns) doubles pass the 160 KiB LDS; MYR_E_ARG: null z / lam / lb / ub / seed_z / grad, negative nsteps, a grad_stride
 * or params_stride other than 0 and np.
 */
int myr_exgd_grad(myr_handle h, int32_t B, const double* z, const double* lam, const double* lb, const double* ub,
                  const double* params, int32_t params_stride, double eta_x, double eta_v, int32_t nsteps,
                  const double* seed_z, const double* seed_lam, double* grad, int32_t grad_stride,
                  double* dz0, double* dlam0, int32_t mem);

/*
 * The Jacobian of `nsteps` extragradient steps (myr_exgd) in the model parameters itself, carried forward through the steps on the device as
 * experiments/e2e_sysid.py:148-177 (many_steps_grad) carries dx/dp, dlam/dp: np tangent columns in one call, where myr_exgd_grad gives one
 * seeded row.  No history is kept: the memory does not depend on nsteps.  With (z_n, lam_n) the iterate after `nsteps` steps from (z, lam):
 *   jz[b][k] = d z_n / d params[k]  ([B][np][n]: parameter-major, each row in z's layout),   jlam[b][k] = d lam_n / d params[k]  ([B][np][m]).
 * A variable that a half-step leaves on a bound (and a pinned one, lb == ub) has a zero row entry, as in myr_exgd_grad.
 *   z [B][n], lam [B][m] (not modified); lb, ub [B][n]; params, params_stride, eta_x, eta_v, nsteps as in myr_exgd_grad;
 *   jz0 [B][np][n], jlam0 [B][np][m] or NULL (= 0): the tangents of the starting point.  NULL holds the start fixed (many_steps_grad); with the
 *   jz, jlam (and zn, lamn) of a previous call, a run of a + b steps splits into two calls with the bits of the one;
 *   zn [B][n], lamn [B][m] or NULL: the advanced iterate, with the bits of myr_exgd on the same inputs;
 *   jz, jlam: either may be NULL, not both.
 * nsteps == 0 gives jz = jz0, jlam = jlam0 (or 0), zn = z, lamn = lam; B == 0 writes nothing.  The same bits for MYR_MEM_HOST and
 * MYR_MEM_DEVICE, on every call, for an instance alone or in any batch, and with any subset of the optional outputs; no atomics.  Timed on
 * MYR_K_PROD.  Detected by its export: myr_version() is unchanged.
 * One wavefront per (instance, group of columns), iterate and columns in LDS (csrc/exgd_jac.h): the iterate's (2 n + m + x_rows ns) doubles and as
 * many again per column.  The columns run in the fewest equal groups that fit the 160 KiB (MYRIAD_EXGD_JAC_LDS_BYTES, read at call time,
 * lowers that budget); a column has the same bits in every grouping.
 * Errors, in this order.  MYR_E_ARG: null h / z / lam / lb / ub; jz and jlam both NULL; B < 0; nsteps < 0; a params_stride other than 0 and
 * np; a bad mem.  MYR_E_UNSUPPORTED: SHOOTING (myr_exgd_grad_shoot has seeded rows), the network system (myr_exgd_grad_node), the elastic
 * twins, INVASIVEPLANT, a system without generated derivatives.  MYR_E_CAPACITY: the iterate and ONE column do not fit; nothing is written.
 */
int myr_exgd_jac(myr_handle h, int32_t B, const double* z, const double* lam, const double* lb, const double* ub,
                 const double* params, int32_t params_stride, double eta_x, double eta_v, int32_t nsteps,
                 const double* jz0, const double* jlam0,
                 double* zn, double* lamn, double* jz, double* jlam, int32_t mem);

/*
 * myr_exgd_grad in the np = 4804 weights of the network system (experiments/node_e2e_sysid.py:139-166, 187-196; library version 0.5): the same
 * step, the same seeds and outputs, the same history in the handle's scratch (chunks under the same 1 GiB bound), the same bits for
 * MYR_MEM_HOST and MYR_MEM_DEVICE and on every call.  A variable on a bound or pinned passes nothing on; nsteps == 0 gives grad = 0,
 * dz0 = seed_z, dlam0 = seed_lam; inputs are not modified; B == 0 writes nothing.
 *   params [np]: ONE weight set shared by the batch, in the order of csrc/node_system.h, required (there is no params_stride);
 *   grad [B][np] if grad_stride == np, [np] = their fixed-order sum if grad_stride == 0; seed_lam, dz0, dlam0 may be NULL.
 * One workgroup of four wavefronts per instance, lane j = hidden unit j of both layers (csrc/node_exgd_grad.h).
 * MYR_E_UNSUPPORTED: a handle whose system is not MYR_SYS_NODE_CARTPOLE (use myr_exgd_grad), a transcription other than
 * MYR_TR_HERMITE_SIMPSON (the one myr_vjp / myr_exgd build for the network system); MYR_E_ARG: null z / lam / lb / ub / seed_z / grad /
 * params, negative nsteps or B, a grad_stride other than 0 and np, a bad mem; MYR_E_CAPACITY: the weight copy (5 064 doubles) and the
 * sweep's (3 n + 2 m + x_rows ns) doubles pass the 160 KiB LDS (N = 400 does).  myr_exgd_grad and myr_hvp keep refusing the network system.
 */
int myr_exgd_grad_node(myr_handle h, int32_t B, const double* z, const double* lam, const double* lb, const double* ub,
                       const double* params, double eta_x, double eta_v, int32_t nsteps,
                       const double* seed_z, const double* seed_lam, double* grad, int32_t grad_stride,
                       double* dz0, double* dlam0, int32_t mem);

/*
 * myr_exgd_grad under MYR_TR_SHOOTING (the transcription the reference's experiments/e2e_sysid.py runs with its default hyperparameters;
 * library version 0.6): the same step, seeds, outputs and null rules, the same history in the handle's scratch (chunks of instances under the
 * same 1 GiB bound), the same bits for MYR_MEM_HOST and MYR_MEM_DEVICE and on every call; nsteps == 0 gives grad = 0, dz0 = seed_z,
 * dlam0 = seed_lam; inputs are not modified; B == 0 writes nothing.  All four integrators, every closed-form system.
 * The reverse sweep is 2 nsteps + 1 passes of one lane per (instance, interval) pair -- a forward tangent rollout and myr_hvp's second-order
 * reverse, started from the multiplier cotangent, so that one pass gives H v + J^T alpha, its parameter part and the pair's rows of J v --,
 * each followed by an elementwise mask pass (csrc/shoot_exgd_grad.h).
 * MYR_E_UNSUPPORTED: a transcription other than MYR_TR_SHOOTING (use myr_exgd_grad), the network system, the elastic twins, INVASIVEPLANT;
 * MYR_E_CAPACITY: more than 2^30 (instance, interval) pairs in one call; MYR_E_ARG: as myr_exgd_grad.  myr_exgd_grad keeps refusing SHOOTING.
 */
int myr_exgd_grad_shoot(myr_handle h, int32_t B, const double* z, const double* lam, const double* lb, const double* ub,
                        const double* params, int32_t params_stride, double eta_x, double eta_v, int32_t nsteps,
                        const double* seed_z, const double* seed_lam, double* grad, int32_t grad_stride,
                        double* dz0, double* dlam0, int32_t mem);

/*
 * myr_exgd_grad_node under MYR_TR_SHOOTING (the transcription the reference's experiments/node_e2e_sysid.py runs with its default
 * hyperparameters; library version 0.8): the step is myr_exgd's on a MYR_SYS_NODE_CARTPOLE + MYR_TR_SHOOTING handle, with all four
 * integrators.  Arguments, null rules, outputs and MYR_E_ARG cases are myr_exgd_grad_node's: ONE weight set params [np], required; grad [B][np]
 * if grad_stride == np, [np] = their fixed-order sum if grad_stride == 0; seed_lam, dz0, dlam0 may be NULL; nsteps == 0 gives grad = 0,
 * dz0 = seed_z, dlam0 = seed_lam; B == 0 writes nothing; inputs are not modified; a variable on a bound or pinned passes nothing on; the same
 * history in the handle's scratch (chunks under the same 1 GiB bound, chunked and unchunked the same bits), the same bits for MYR_MEM_HOST
 * and MYR_MEM_DEVICE, on every call, and for an instance alone or inside any batch.
 * One workgroup of 1, 2 or 4 wavefronts (from the number of intervals alone) per instance, one wavefront per (instance, interval) pair, lane j =
 * hidden unit j of both layers; myr_exgd_grad_shoot's 2 nsteps + 1 pair passes with the network differentiated layer by layer at every
 * stage point, the running cost of the true system included at each (csrc/node_shoot_exgd_grad.h).
 * MYR_E_UNSUPPORTED: a handle whose system is not MYR_SYS_NODE_CARTPOLE (use myr_exgd_grad_shoot), MYR_TR_HERMITE_SIMPSON (use
 * myr_exgd_grad_node), MYR_TR_TRAPEZOIDAL; MYR_E_CAPACITY: the weight copy (5 064 doubles) and the sweep's
 * 3 n + I (3 ns + 2 ns cpi + (M cpi + 1) nu) doubles (M = 2 for RK4, 1 otherwise) pass the 160 KiB LDS -- about 1 250 integration steps
 * I cpi in all, 950 under RK4 (1 x 100 HEUN needs 50 KiB; 1 x 2 000 is refused).  myr_exgd_grad_node keeps refusing every transcription but Hermite-Simpson,
 * myr_exgd_grad_shoot and myr_hvp the network system.
 */
int myr_exgd_grad_node_shoot(myr_handle h, int32_t B, const double* z, const double* lam, const double* lb, const double* ub,
                             const double* params, double eta_x, double eta_v, int32_t nsteps,
                             const double* seed_z, const double* seed_lam, double* grad, int32_t grad_stride,
                             double* dz0, double* dlam0, int32_t mem);

/*
 * Lagrangian Hessian-vector product, matrix-free and exact, for all three transcriptions (library version 0.4).  With
 * L(z, lam, p) = f(z, p) + lam^T c(z, p), a direction v and psi(z, lam, p) = <grad_z L(z, lam, p), v>:
 *   out_z[b] = grad_z psi = (d^2 L / dz dz) v[b],      out_p[b] = grad_p psi = (d^2 L / dp dz) v[b].
 * (grad_lam psi = J v is myr_jvp.)  with_cost == 0 drops f from L in both outputs and leaves sum_i lam_i (d^2 c_i / dz dz) v -- the
 * constraint-Hessian callback of SciPy's trust-constr.
 *   z [B][n]; lam [B][m] or NULL (= 0); v [B][n]; params as in myr_vjp; out_z [B][n] or NULL;
 *   out_p [B][np] if p_stride == np, [np] = the sum over the batch if p_stride == 0 (fixed order, no atomics: the same bits on every
 *   call, for MYR_MEM_HOST and MYR_MEM_DEVICE alike), or NULL.  Inputs are not modified; B == 0 does nothing.
 * Collocation: the Hessian is block-diagonal over the points.  SHOOTING: per (instance, interval) a forward tangent rollout and a
 * second-order reverse sweep through the integrator's stages (EULER, HEUN, MIDPOINT, RK4); the terminal cost of BACTERIA, TUMOUR and
 * PREDATORPREY sits on the integrated end state of the last interval (shooting.py:206-208) and takes part through that interval's costate.
 * MYR_E_ARG: null z / v, both outputs null, a p_stride or params_stride other than 0 and np, a bad mem;
 * MYR_E_UNSUPPORTED: the network system, the elastic twins, INVASIVEPLANT; MYR_E_CAPACITY: SHOOTING with more than 2^30 (instance, interval)
 * pairs in one call (the collocation kernel reads its inputs where they lie: no horizon is too long for it).
 */
int myr_hvp(myr_handle h, int32_t B, const double* z, const double* lam, const double* v, const double* params,
            int32_t params_stride, int32_t with_cost, double* out_z, double* out_p, int32_t p_stride, int32_t mem);

/*
 * myr_hvp for the network system (library version 0.9): the same two products on a MYR_SYS_NODE_CARTPOLE handle under
 * MYR_TR_HERMITE_SIMPSON or MYR_TR_SHOOTING (all four integrators), out_p in the 4 804 weights in the order of csrc/node_system.h.
 * With L = with_cost f + lam^T c and psi = <grad_z L, v>:  out_z[b] = grad_z psi,  out_p[b] = grad_p psi.
 *   z [B][n]; lam [B][m] or NULL (= 0); v [B][n]; params [np]: ONE weight set shared by the batch, required (no params_stride, as in
 *   myr_exgd_grad_node); out_z [B][n] or NULL; out_p [B][np] if p_stride == np, [np] = the fixed-order sum over the batch if p_stride == 0
 *   (no atomics), or NULL -- not both NULL.  Inputs are not modified; B == 0 writes nothing.
 * The running cost is the TRUE system's: it has no weights, but its second derivative enters out_z, and under SHOOTING its gradient enters
 * every stage costate and so out_p.  The same bits on every call, for MYR_MEM_HOST and MYR_MEM_DEVICE, for an instance alone or inside any
 * batch, whatever ran on the handle before; out_z has the same bits with and without out_p.
 * Hermite-Simpson: one workgroup of 4 wavefronts per instance, a wavefront per collocation point (lane j = hidden unit j), the inputs read
 * where they lie -- no horizon is refused.  SHOOTING: one workgroup of 1, 2 or 4 wavefronts (from the number of intervals alone) per
 * instance, a wavefront per (instance, interval) pair (csrc/node_hvp.h).
 * MYR_E_UNSUPPORTED: a handle whose system is not MYR_SYS_NODE_CARTPOLE (use myr_hvp), MYR_TR_TRAPEZOIDAL -- both before the size checks;
 * MYR_E_ARG: null h / z / v / params, both outputs NULL, a p_stride other than 0 and np, negative B, a bad mem;
 * MYR_E_CAPACITY (SHOOTING only): the weight copy (5 064 doubles) and the pairs' records, I (3 ns + 2 ns cpi + (M cpi + 1) nu) doubles
 * (M = 2 for RK4, 1 otherwise), pass the 160 KiB LDS: 15 414 doubles beside the weights -- single shooting up to 1 x 1 711 (1 x 1 540
 * under RK4), 700 x 1, 20 x 84 (1 x 2 000 is refused).
 * myr_hvp keeps refusing the network system.
 */
int myr_hvp_node(myr_handle h, int32_t B, const double* z, const double* lam, const double* v, const double* params,
                 int32_t with_cost, double* out_z, double* out_p, int32_t p_stride, int32_t mem);

/*
 * myr_exgd_grad_node / myr_exgd_grad_node_shoot for E independent weight sets of R instances each in ONE call (an ensemble of networks that
 * differ in seed, noise level or learning rate: E launches of one workgroup each become one launch of E R workgroups).  Served on a
 * MYR_SYS_NODE_CARTPOLE handle under MYR_TR_HERMITE_SIMPSON and MYR_TR_SHOOTING alike: the call dispatches on the handle's transcription.
 *   params [E][np]: the weight sets, required; every per-instance array is [E][R][...], instance (e, r) is row e R + r: z, lb, ub, seed_z,
 *   dz0 [E][R][n]; lam, seed_lam, dlam0 [E][R][m]; grad [E][R][np] if grad_stride == np, [E][np] if grad_stride == 0: row e is the fixed-order sum
 *   over the R rows of set e.  seed_lam, dz0, dlam0 may be NULL.  Inputs are not modified; E == 0 writes nothing.
 * For every set e the outputs of set e have the BITS of the single-set call on that set alone (B = R, params + e np, the same stride and
 * mem): for MYR_MEM_HOST and MYR_MEM_DEVICE, on every call, whatever E is and whatever ran on the handle before, with the history in one chunk
 * or in many (a chunk of instances may begin and end inside a set).  The two single-set calls are the E = 1, R = B case of this one.
 * MYR_E_ARG: null h / z / lam / lb / ub / seed_z / grad / params, E < 0, R < 1, E R past the int range, negative nsteps, a grad_stride other
 * than 0 and np, a bad mem; MYR_E_UNSUPPORTED (before the size checks): a handle whose system is not MYR_SYS_NODE_CARTPOLE, MYR_TR_TRAPEZOIDAL;
 * MYR_E_CAPACITY: the LDS bounds of the single-set call of the handle's transcription, unchanged.
 */
int myr_exgd_grad_node_sets(myr_handle h, int32_t E, int32_t R, const double* z, const double* lam, const double* lb, const double* ub,
                            const double* params, double eta_x, double eta_v, int32_t nsteps,
                            const double* seed_z, const double* seed_lam, double* grad, int32_t grad_stride,
                            double* dz0, double* dlam0, int32_t mem);

/*
 * myr_hvp_node for E independent weight sets of R instances each in one call, under MYR_TR_HERMITE_SIMPSON or MYR_TR_SHOOTING.
 *   params [E][np], required; z, v, out_z [E][R][n]; lam [E][R][m] or NULL (= 0); out_p [E][R][np] if p_stride == np, [E][np] if p_stride == 0
 *   (row e: the fixed-order sum over the R rows of set e), or NULL -- out_z and out_p not both NULL.  E == 0 writes nothing.
 * For every set e the outputs of set e have the bits of myr_hvp_node on that set alone (B = R, params + e np, the same stride and mem), for
 * MYR_MEM_HOST and MYR_MEM_DEVICE, on every call.  myr_hvp_node is the E = 1, R = B case of this call.
 * MYR_E_ARG: null h / z / v / params, both outputs NULL, E < 0, R < 1, E R past the int range, a p_stride other than 0 and np, a bad mem;
 * MYR_E_UNSUPPORTED (before the size checks): a handle whose system is not MYR_SYS_NODE_CARTPOLE, MYR_TR_TRAPEZOIDAL;
 * MYR_E_CAPACITY (SHOOTING only): myr_hvp_node's LDS bound, unchanged.
 */
int myr_hvp_node_sets(myr_handle h, int32_t E, int32_t R, const double* z, const double* lam, const double* v, const double* params,
                      int32_t with_cost, double* out_z, double* out_p, int32_t p_stride, int32_t mem);

/* Average device time (HIP events on the handle's stream) of the launches of one kernel since the last reset. */
int myr_kernel_time(myr_handle h, int32_t kernel_id, double* avg_ms, int32_t* launches);
int myr_kernel_time_reset(myr_handle h);

/* Devices the library can create handles on (hipGetDeviceCount; 0 when there is none or the runtime fails).  The reference
 * has no multi-device code; the host mirror uses it to fan a batch out over the GPUs of a node beneath the
 * unchanged TrajectoryOptimizer API (myriad/trajectory_optimizers/base.py:69-93): one handle and one host thread per device. */
int myr_device_count(void);

const char* myr_last_error(void);
const char* myr_version(void);

/* ABI guard (round 5): the bytes this build of the library reads and writes through a `myr_solve_opts*`, a `myr_problem_desc*` and a
 * `myr_dims*`.  The structs carry no size field and `myr_solve_opts` has grown before (round 4: restoration, park_iter: 40 -> 48 bytes);
 * a binding compares these numbers with the sizes of its OWN declarations once, at load time, and refuses a library that disagrees
 * (myriad_amd/_lib.py: load()) instead of letting the library read past a shorter struct.  `which`: 0 = myr_solve_opts,
 * 1 = myr_problem_desc, 2 = myr_dims; anything else returns -1. */
int32_t myr_abi_sizeof(int32_t which);

#ifdef __cplusplus
}
#endif
#endif
