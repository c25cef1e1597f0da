// The argument checks of the effq_prep_denoise_* entry points as a stand-alone host program, for a sanitizer build (make
// check-denoise-args: AddressSanitizer and UBSan on the host code; no device is touched, since every call here is
// refused before its first launch).  It links prep_denoise.hip alone, so the library's error sink is a stub.
#include <cmath>
#include <cstdio>
#include "../../include/effq_hip.h"

namespace effq { void set_error(const char*, ...) {} }

int main() {
  alignas(16) static float v[128], y[64];
  alignas(16) static double change[2], ws[64];
  int refused = 0, calls = 0;
  auto expect = [&](int got, int want) { ++calls; refused += got == want; };
  auto off = [](auto* p, int bytes) { return reinterpret_cast<decltype(p)>(reinterpret_cast<char*>(p) + bytes); };
  auto nlm = [&](const float* vv, int D, int mode, int M, double s2, float* yy, double* ch, void* w, size_t bytes,
                 int want) {
    expect(effq_prep_denoise_nlm(vv, D, 4, 4, mode, M, s2, yy, ch, w, bytes, nullptr), want);
  };
  size_t need = 0;
  expect(effq_prep_denoise_ws_bytes(4, 4, 4, &need) == EFFQ_OK && need == 16 && need <= sizeof(ws), 1);
  expect(effq_prep_denoise_ws_bytes(4, 4, 4, nullptr), EFFQ_ERR_ARG);
  expect(effq_prep_denoise_ws_bytes(4, 0, 4, &need), EFFQ_ERR_ARG);
  size_t big = 0;                                                               // three tiles along W, two along D and H
  expect(effq_prep_denoise_ws_bytes(EFFQ_PREP_DENOISE_TILE_D + 1, EFFQ_PREP_DENOISE_TILE_H + 1,
                                    2 * EFFQ_PREP_DENOISE_TILE_W + 3, &big) == EFFQ_OK && big == 12 * 16, 1);
  nlm(nullptr, 4, 0, 3, 1.0, y, change, ws, need, EFFQ_ERR_ARG);                // null pointers
  nlm(v, 4, 0, 3, 1.0, nullptr, change, ws, need, EFFQ_ERR_ARG);
  nlm(v, 4, 0, 3, 1.0, y, nullptr, ws, need, EFFQ_ERR_ARG);
  nlm(v, 4, 0, 3, 1.0, y, change, nullptr, need, EFFQ_ERR_ARG);
  nlm(v, 0, 0, 3, 1.0, y, change, ws, need, EFFQ_ERR_ARG);                      // extents
  nlm(v, 40000, 0, 3, 1.0, y, change, ws, need, EFFQ_ERR_ARG);
  nlm(v, 4, 2, 3, 1.0, y, change, ws, need, EFFQ_ERR_ARG);                      // the mask
  nlm(v, 4, -1, 3, 1.0, y, change, ws, need, EFFQ_ERR_ARG);
  nlm(v, 4, 0, 0, 1.0, y, change, ws, need, EFFQ_ERR_ARG);                      // the search radius
  nlm(v, 4, 0, 6, 1.0, y, change, ws, need, EFFQ_ERR_ARG);
  nlm(v, 4, 0, 3, 0.0, y, change, ws, need, EFFQ_ERR_ARG);                      // sigma2
  nlm(v, 4, 0, 3, -1.0, y, change, ws, need, EFFQ_ERR_ARG);
  nlm(v, 4, 0, 3, NAN, y, change, ws, need, EFFQ_ERR_ARG);
  nlm(v, 4, 0, 3, INFINITY, y, change, ws, need, EFFQ_ERR_ARG);
  nlm(v, 4, 0, 3, 1e-45, y, change, ws, need, EFFQ_ERR_ARG);                    // the folded constant overflows fp32
  nlm(v, 4, 0, 3, 1e300, y, change, ws, need, EFFQ_ERR_ARG);                    // ... and vanishes
  nlm(v, 4, 0, 3, 1.0, v + 32, change, ws, need, EFFQ_ERR_ARG);                 // v and y overlap
  nlm(v, 4, 0, 3, 1.0, v, change, ws, need, EFFQ_ERR_ARG);
  nlm(off(v, 2), 4, 0, 3, 1.0, y, change, ws, need, EFFQ_ERR_ARG);              // alignment
  nlm(v, 4, 0, 3, 1.0, off(y, 2), change, ws, need, EFFQ_ERR_ARG);
  nlm(v, 4, 0, 3, 1.0, y, off(change, 4), ws, need, EFFQ_ERR_ARG);
  nlm(v, 4, 0, 3, 1.0, y, change, off(ws, 4), need, EFFQ_ERR_ARG);
  nlm(v, 4, 0, 3, 1.0, y, change, ws, need - 1, EFFQ_ERR_WORKSPACE);            // a short workspace
  expect(effq_prep_denoise_residual(nullptr, 4, 4, 4, 0, y, nullptr), EFFQ_ERR_ARG);
  expect(effq_prep_denoise_residual(v, 4, 4, 4, 0, nullptr, nullptr), EFFQ_ERR_ARG);
  expect(effq_prep_denoise_residual(v, 4, 4, -4, 0, y, nullptr), EFFQ_ERR_ARG);
  expect(effq_prep_denoise_residual(v, 4, 4, 4, 3, y, nullptr), EFFQ_ERR_ARG);
  expect(effq_prep_denoise_residual(v, 4, 4, 4, 0, v + 63, nullptr), EFFQ_ERR_ARG);
  expect(effq_prep_denoise_residual(off(v, 1), 4, 4, 4, 0, y, nullptr), EFFQ_ERR_ARG);
  printf("%d of %d checks held\n", refused, calls);
  return refused == calls ? 0 : 1;
}
