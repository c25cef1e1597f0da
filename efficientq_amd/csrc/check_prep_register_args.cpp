// The argument checks of effq_prep_bins and effq_prep_joint_hist as a stand-alone host program, for a sanitizer build
// (make check-register-args: AddressSanitizer and UBSan on the host code; no device is touched, since every call here is
// refused before its first launch).  It links prep_register.hip alone, so the library's error sink is a stub.
#include <cmath>
#include <cstdio>
#include <vector>
#include "../../include/effq_hip.h"

namespace effq { void set_error(const char*, ...) {} }

int main() {
  std::vector<double> m(12 * EFFQ_PREP_REGISTER_MAX_K, 0.5);
  alignas(16) static float mov[64];
  alignas(16) static unsigned char fbin[64];
  alignas(16) static unsigned long long hist[EFFQ_PREP_REGISTER_MAX_K * 1024];
  int refused = 0, calls = 0;
  auto hist_call = [&](const unsigned char* f, int D, const float* mv, int MD, const double* mm, int K, float lo, float scale,
                       int sd, unsigned long long* h) {
    ++calls;
    refused += effq_prep_joint_hist(f, D, 4, 4, mv, MD, 4, 4, mm, K, lo, scale, sd, 1, 1, h, nullptr) == EFFQ_ERR_ARG;
  };
  hist_call(nullptr, 4, mov, 4, m.data(), 13, 0, 1, 1, hist);                 // null pointers
  hist_call(fbin, 4, nullptr, 4, m.data(), 13, 0, 1, 1, hist);
  hist_call(fbin, 4, mov, 4, nullptr, 13, 0, 1, 1, hist);
  hist_call(fbin, 4, mov, 4, m.data(), 13, 0, 1, 1, nullptr);
  hist_call(fbin, 0, mov, 4, m.data(), 13, 0, 1, 1, hist);                    // extents
  hist_call(fbin, 40000, mov, 4, m.data(), 13, 0, 1, 1, hist);
  hist_call(fbin, 4, mov, -1, m.data(), 13, 0, 1, 1, hist);
  hist_call(fbin, 4, mov, 4, m.data(), 0, 0, 1, 1, hist);                     // K
  hist_call(fbin, 4, mov, 4, m.data(), EFFQ_PREP_REGISTER_MAX_K + 1, 0, 1, 1, hist);
  hist_call(fbin, 4, mov, 4, m.data(), 13, 0, 1, 0, hist);                    // a stride below 1
  hist_call(fbin, 4, mov, 4, m.data(), 13, NAN, 1, 1, hist);                  // the bin range
  hist_call(fbin, 4, mov, 4, m.data(), 13, 0, 0, 1, hist);
  hist_call(fbin, 4, mov, 4, m.data(), 13, 0, INFINITY, 1, hist);
  hist_call(fbin, 4, reinterpret_cast<const float*>(reinterpret_cast<const char*>(mov) + 2), 4, m.data(), 13, 0, 1, 1, hist);
  hist_call(fbin, 4, mov, 4, m.data(), 13, 0, 1, 1, reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(hist) + 4));
  m.back() = NAN;                                                             // the last entry of the last matrix is read
  hist_call(fbin, 4, mov, 4, m.data(), EFFQ_PREP_REGISTER_MAX_K, 0, 1, 1, hist);
  for (int bad = 0; bad < 3; ++bad) {
    ++calls;
    refused += effq_prep_bins(bad == 0 ? nullptr : mov, 4, 4, 4, 0, bad == 1 ? -1.0f : 1.0f, bad == 2 ? 2 : 0, fbin, nullptr) ==
               EFFQ_ERR_ARG;
  }
  printf("%d of %d calls refused\n", refused, calls);
  return refused == calls ? 0 : 1;
}
