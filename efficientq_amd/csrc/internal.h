// Entry points the library's translation units call in each other that are not part of the public C ABI
// (include/effq_hip.h).  Each is declared here once; the file that defines it includes this header, so the compiler
// checks the definition against the declaration (C linkage would link a mismatch silently).
#pragma once
#include "common.h"

namespace effq {
struct ProjFused;   // project_dual.h
struct ProjNext;

// prox_solve.hip: the K slices a prox solve left for the caller's next kernel to add up ([nsplit][c2][ldp] floats), or
// part == NULL: the product had one slice and wstar / bstar are complete
struct ProxParts {
  const float* part;
  int nsplit, ldp;
};
// One prox solve  [wstar|bstar] = Bm * Ainv,  Bm = B0 + eta [W0|b0] + rho [G - dual|0]  (operands as effq_prox_solve).
struct ProxSolve {
  const float *B0, *Ainv, *W0, *b0, *G, *dual;
  int c2, n, has_bias;
  double rho, eta;
  double shift;        // effq_prox_solve_shifted: rho_inv - rho, nterms terms of the series (plain solve: 0, 1)
  int nterms;
  bool prebuilt;       // Bm of the first term already stands in the workspace (the last projection wrote it: ProjNext)
  float *wstar, *bstar;
  void* ws;
  size_t ws_bytes;
  ProxParts* parts;    // not NULL: leave the K slices of the product and describe them here instead of adding them up
};
}

extern "C" {

// fixed_point_values.hip: effq_fixed_point_small with pf != NULL running the projection of the ADMM iteration as the
// epilogue
int effq_fixed_point_small_fused(const float* a, const float* b, float* v_out, size_t n, int levels, double lo, double hi,
                                 double tol, int max_iter, effq_fp_state* state_dev, const effq::ProjFused* pf_in,
                                 void* stream);
// project_dual.hip: effq_admm_project_dual with the convergence check of state_dev folded in (err_flag_dev) and, with
// nx != NULL, also leaving the right-hand side of the next prox solve in nx->Bm
int effq_project_dual_impl(const float* v, const float* wstar, const effq_fp_state* state_dev, int levels, float* G,
                           float* dual, float dual_div, int8_t* Gq_out, size_t n, int32_t* err_flag_dev,
                           const effq::ProjNext* nx, void* stream);

// prox_solve.hip: Bm (the start of the prox workspace) and its row length; the one entry behind effq_prox_solve and
// effq_prox_solve_shifted, which the fused run calls directly
float* effq_prox_bm(void* ws, int c2, int n, int* ldb);
int effq_prox_enqueue(const effq::ProxSolve* s, void* stream);

// fixed_point_traj.hip: the trajectory fixed point on the slices of the prox product (effq::ProxParts)
int effq_fixed_point_traj_parts(const float* part, int nsplit, int ldp, int c2, int nwrow, int has_bias, const float* dual,
                                float* wstar_out, float* bstar_out, float* v_out, int levels, double lo, double hi, double tol,
                                int max_iter, effq_fp_state* state_dev, void* pred_dev, void* ws, size_t ws_bytes,
                                void* stream);

}  // extern "C"
