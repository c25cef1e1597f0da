// Entry points the library's translation units call in each other that are not part of the public C ABI
// (include/effq_hip.h).  Each is declared here once; the file that defines it includes this header, so the compiler
// checks the definition against the declaration (C linkage would link a mismatch silently).
#pragma once
#include "common.h"

namespace effq {
struct ProjFused;   // project_dual.h
struct ProjNext;
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

// solve.hip: Bm (the start of the prox workspace) and its row length; the prox solve on a Bm already written, whole or
// as the slices of its product (*part_out != NULL)
float* effq_prox_bm(void* ws, int c2, int n, int* ldb);
int effq_prox_solve_prebuilt(const float* B0, const float* Ainv, const float* W0, const float* b0, const float* G,
                             const float* dual, int c2, int n, int has_bias, double rho, double eta, float* wstar,
                             float* bstar, void* ws, size_t ws_bytes, void* stream);
int effq_prox_solve_prebuilt_parts(const float* B0, const float* Ainv, const float* W0, const float* b0, const float* G,
                                   const float* dual, int c2, int n, int has_bias, double rho, double eta, float* wstar,
                                   float* bstar, void* ws, size_t ws_bytes, void* stream, const float** part_out,
                                   int* nsplit_out, int* ldp_out);

// fixed_point_traj.hip: the trajectory fixed point on the slices of the prox product (effq_prox_solve_prebuilt_parts)
int effq_fixed_point_traj_parts(const float* part, int nsplit, int ldp, int c2, int nwrow, int has_bias, const float* dual,
                                float* wstar_out, float* bstar_out, float* v_out, int levels, double lo, double hi, double tol,
                                int max_iter, effq_fp_state* state_dev, void* pred_dev, void* ws, size_t ws_bytes,
                                void* stream);

}  // extern "C"
