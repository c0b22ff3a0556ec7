// node_hvp_twin.cpp -- TEST-ONLY host build of the Lagrangian Hessian-vector product of the network system (myriad_amd/csrc/node_hvp.h):
// node_hvp_host -- the point algebra (NodeExgdHost::second, cost_hd) and the pair algebra (NodeShootExgd<M>::interval<true> over NseHostNet) the
// device kernels run, in plain loops over a batch.  Compiled by tests/node_hvp_cases.py with g++ -O2 -std=c++17; never loaded by the package.
#include "../../myriad_amd/csrc/node_hvp.h"

using namespace myriad;

// transcription: 0 Hermite-Simpson, 2 SHOOTING; method: 0 Euler, 1 Heun, 2 midpoint, 3 RK4 (SHOOTING only).  params [4804] shared; lam, out_z,
// out_p ([B][4804]) may be null.  Returns 0, or -1 for anything else.
extern "C" int node_hvp_twin(int transcription, int method, int B, int I, int cpi, double T, const double* z, const double* lam, const double* v,
                             const double* params, int with_cost, double* out_z, double* out_p) {
  return node_hvp_host(transcription, method, B, I, cpi, T, z, lam, v, params, with_cost, out_z, out_p);
}

// One collocation point two ways: layer by layer (what node_hvp_colloc_host and the kernel run) and SysNODE::hessian -- the dense 5 x 5 block the
// solvers are built on -- contracted with d.  w [5] = [x; u], mu [4], d [5]; hd_layer [5], hd_dense [5]
extern "C" void node_hvp_point_two_ways(const double* w, const double* params, const double* mu, double wq, const double* d, double* hd_layer,
                                        double* hd_dense) {
  using Sys = SysNODE_CARTPOLE;
  constexpr int NS = Sys::NS, NW = Sys::NW;
  static double gp[Sys::NP];
  double wo[NS], W[NW * NW], D2[Sys::NNZ2] = {0.0};
  NodeExgdPoint::hess(w, params, mu, wq, false, 0.0, d, hd_layer, wo, gp);
  Sys::hessian(w, w + NS, params, D2, mu, wq, W);
  for (int a = 0; a < NW; ++a) {
    double s = 0.0;
    for (int b = 0; b < NW; ++b) s += W[a * NW + b] * d[b];
    hd_dense[a] = s;
  }
}
