// The argument checks of the effq_prep_bias_* entry points as a stand-alone host program, for a sanitizer build (make
// check-bias-args: AddressSanitizer and UBSan on the host code; no device is touched, since every call here is refused
// before its first launch).  It links prep_bias.hip alone, so the library's error sink is a stub.
#include <cmath>
#include <cstdio>
#include <vector>
#include "../../include/effq_hip.h"

namespace effq { void set_error(const char*, ...) {} }

int main() {
  alignas(16) static float u[64], f[64];
  alignas(16) static unsigned char m[64];
  alignas(16) static unsigned long long hist[EFFQ_PREP_BIAS_BINS + 2];
  alignas(16) static double phi[1331], sums[2], lat[EFFQ_PREP_BIAS_LATTICE], ws[4096];
  std::vector<double> E(EFFQ_PREP_BIAS_BINS, 0.25);
  const int one[3] = {1, 1, 1}, zero[3] = {0, 0, 0}, bad_s[3] = {1, 0, 1}, bad_o[3] = {0, 4, 0}, neg_o[3] = {0, 0, -1};
  int refused = 0, calls = 0;
  auto expect = [&](int got, int want) { ++calls; refused += got == want; };
  auto fit = [&](const float* uu, int D, const int* s, const int* o, int level, float lo, float hi, const double* e,
                 size_t bytes, int want) {
    expect(effq_prep_bias_fit(uu, m, f, D, 4, 4, s, o, level, lo, hi, e, phi, lat, sums, ws, bytes, nullptr), want);
  };
  const size_t need = effq_bias_fit_ws_bytes(4, 4, 4, one, zero);
  expect(need > 0 && need <= sizeof(ws), 1);
  expect(effq_bias_fit_ws_bytes(4, 4, 4, bad_s, zero) == 0 && effq_bias_fit_ws_bytes(4, 4, 4, one, bad_o) == 0, 1);
  fit(nullptr, 4, one, zero, 0, 0, 1, E.data(), need, EFFQ_ERR_ARG);             // null pointers
  fit(u, 4, one, zero, 0, 0, 1, nullptr, need, EFFQ_ERR_ARG);
  fit(u, 4, nullptr, zero, 0, 0, 1, E.data(), need, EFFQ_ERR_ARG);
  fit(u, 0, one, zero, 0, 0, 1, E.data(), need, EFFQ_ERR_ARG);                   // extents
  fit(u, 40000, one, zero, 0, 0, 1, E.data(), need, EFFQ_ERR_ARG);
  fit(u, 4, bad_s, zero, 0, 0, 1, E.data(), need, EFFQ_ERR_ARG);                 // a stride below 1, offsets outside
  fit(u, 4, one, bad_o, 0, 0, 1, E.data(), need, EFFQ_ERR_ARG);
  fit(u, 4, one, neg_o, 0, 0, 1, E.data(), need, EFFQ_ERR_ARG);
  fit(u, 4, one, zero, -1, 0, 1, E.data(), need, EFFQ_ERR_ARG);                  // the level
  fit(u, 4, one, zero, EFFQ_PREP_BIAS_LEVELS, 0, 1, E.data(), need, EFFQ_ERR_ARG);
  fit(u, 4, one, zero, 0, 1, 1, E.data(), need, EFFQ_ERR_ARG);                   // the range
  fit(u, 4, one, zero, 0, NAN, 1, E.data(), need, EFFQ_ERR_ARG);
  fit(u, 4, one, zero, 0, 0, INFINITY, E.data(), need, EFFQ_ERR_ARG);
  fit(reinterpret_cast<const float*>(reinterpret_cast<const char*>(u) + 2), 4, one, zero, 0, 0, 1, E.data(), need,
      EFFQ_ERR_ARG);
  fit(u, 4, one, zero, 0, 0, 1, E.data(), need - 1, EFFQ_ERR_WORKSPACE);
  E.back() = NAN;                                                                 // the last entry of the table is read
  fit(u, 4, one, zero, 0, 0, 1, E.data(), need, EFFQ_ERR_ARG);
  expect(effq_prep_bias_hist(u, m, f, 4, 4, 4, one, zero, nullptr, nullptr), EFFQ_ERR_ARG);
  expect(effq_prep_bias_hist(u, m, f, 4, 4, 4, one, bad_o, hist, nullptr), EFFQ_ERR_ARG);
  expect(effq_prep_bias_hist(u, m, f, 4, 4, 4, one, zero, reinterpret_cast<unsigned long long*>(
                                 reinterpret_cast<char*>(hist) + 4), nullptr), EFFQ_ERR_ARG);
  expect(effq_prep_bias_log(u, 4, 4, 4, 2, f, m, nullptr), EFFQ_ERR_ARG);
  expect(effq_prep_bias_log(u, 4, 4, 4, 0, nullptr, m, nullptr), EFFQ_ERR_ARG);
  expect(effq_prep_bias_apply(u, m, 4, 4, 4, lat, f, nullptr, nullptr), EFFQ_ERR_ARG);       // m without range
  expect(effq_prep_bias_apply(u, nullptr, 4, 4, -4, lat, f, nullptr, nullptr), EFFQ_ERR_ARG);
  expect(effq_prep_bias_apply(u, nullptr, 4, 4, 4, nullptr, f, nullptr, nullptr), EFFQ_ERR_ARG);
  printf("%d of %d checks held\n", refused, calls);
  return refused == calls ? 0 : 1;
}
