// The argument checks of effq_seg_crf and effq_seg_crf_ws_bytes as a stand-alone host program, for a sanitizer build (make
// check-crf-args: AddressSanitizer and UBSan on the host code; no device is touched, since every call here is refused
// before its first launch).  It links seg_crf.hip alone, so the library's error sink is a stub.
#include <cmath>
#include <cstdio>
#include "../../include/effq_hip.h"

namespace effq { void set_error(const char*, ...) {} }

struct Call {                                             // a call that would be accepted: 2 x 4 x 4 x 4 logits, one modality
  alignas(16) static inline float v[256], x[128], out[128], ws[1024 + 256 + 8];
  alignas(16) static inline unsigned changed[2];
  const float *logits = v, *images = x;
  int C = 2, M = 1, D = 4, H = 4, W = 4, mode = EFFQ_SEG_ARGMAX, iters = 5;
  double s_d = 1.0, s_h = 1.0, s_w = 1.0, w_a = 4.0, w_s = 1.0, theta_p = 3.0, theta_i = 0.5, theta_s = 1.0;
  float thresh = 0.0f;
  float* o = out;
  unsigned* ch = changed;
  void* w = ws;
  size_t bytes = 4096 + 2 * 4 * 128;
  int run() const {
    return effq_seg_crf(logits, C, images, M, D, H, W, s_d, s_h, s_w, mode, w_a, w_s, theta_p, theta_i, theta_s, iters, thresh,
                        o, ch, w, bytes, nullptr);
  }
};

int main() {
  int held = 0, calls = 0;
  auto expect = [&](int got, int want) { ++calls; held += got == want; };
  auto refused = [&](auto change, int want = EFFQ_ERR_ARG) {
    Call c;
    change(c);
    expect(c.run(), want);
  };
  auto off = [](auto* p, int bytes) { return reinterpret_cast<decltype(p)>(reinterpret_cast<char*>(p) + bytes); };
  size_t need = 0;
  expect(effq_seg_crf_ws_bytes(2, 4, 4, 4, &need) == EFFQ_OK && need == Call().bytes && need <= sizeof(Call::ws), 1);
  expect(effq_seg_crf_ws_bytes(2, 4, 4, 4, nullptr), EFFQ_ERR_ARG);
  expect(effq_seg_crf_ws_bytes(0, 4, 4, 4, &need), EFFQ_ERR_ARG);
  expect(effq_seg_crf_ws_bytes(9, 4, 4, 4, &need), EFFQ_ERR_ARG);
  expect(effq_seg_crf_ws_bytes(2, 4, 0, 4, &need), EFFQ_ERR_ARG);
  expect(effq_seg_crf_ws_bytes(2, 2048, 2048, 256, &need), EFFQ_ERR_ARG);          // 2^31 elements
  expect(effq_seg_crf_ws_bytes(2, 2147483647, 2147483647, 2147483647, &need), EFFQ_ERR_ARG);
  refused([](Call& c) { c.logits = nullptr; });                                    // null pointers
  refused([](Call& c) { c.images = nullptr; });
  refused([](Call& c) { c.o = nullptr; });
  refused([](Call& c) { c.ch = nullptr; });
  refused([](Call& c) { c.w = nullptr; });
  refused([](Call& c) { c.C = 0; });                                               // the classes
  refused([](Call& c) { c.C = 9; });
  refused([](Call& c) { c.C = 1; });                                               // a softmax over one class
  refused([](Call& c) { c.mode = 2; });
  refused([](Call& c) { c.mode = -1; });
  refused([](Call& c) { c.M = 0; });                                               // the modalities
  refused([](Call& c) { c.M = 5; });
  refused([](Call& c) { c.D = 0; });                                               // the extents
  refused([](Call& c) { c.W = -4; });
  refused([](Call& c) { c.D = 2048; c.H = 2048; c.W = 256; });
  refused([](Call& c) { c.D = c.H = c.W = 2147483647; });
  refused([](Call& c) { c.s_d = 0.0; });                                           // the spacing
  refused([](Call& c) { c.s_h = -1.0; });
  refused([](Call& c) { c.s_w = NAN; });
  refused([](Call& c) { c.s_w = INFINITY; });
  refused([](Call& c) { c.w_a = -1.0; });                                          // the weights
  refused([](Call& c) { c.w_s = NAN; });
  refused([](Call& c) { c.w_a = 60.0; c.w_s = 4.5; });
  refused([](Call& c) { c.w_a = INFINITY; });
  refused([](Call& c) { c.theta_p = 0.0; });                                       // the widths
  refused([](Call& c) { c.theta_i = -0.5; });
  refused([](Call& c) { c.theta_s = NAN; });
  refused([](Call& c) { c.theta_p = INFINITY; });
  refused([](Call& c) { c.theta_i = 0.99e-18; });                                  // below and above the range of a width
  refused([](Call& c) { c.theta_i = 1.01e18; });
  refused([](Call& c) { c.theta_s = 1e-19; });
  refused([](Call& c) { c.theta_p = 1e19; });
  refused([](Call& c) { c.iters = 0; });                                           // the iterations
  refused([](Call& c) { c.iters = 21; });
  refused([](Call& c) { c.thresh = NAN; });
  refused([](Call& c) { c.thresh = INFINITY; });
  refused([](Call& c) { c.s_d = c.s_h = c.s_w = 7.0; });                           // all radii 0
  refused([](Call& c) { c.o = Call::v + 64; });                                    // out overlaps the logits
  refused([](Call& c) { c.o = Call::v; });
  refused([](Call& c) { c.o = Call::x + 32; });                                    // ... the images
  refused([](Call& c) { c.w = Call::out; });                                       // the workspace overlaps out
  refused([](Call& c) { c.ch = reinterpret_cast<unsigned*>(Call::out + 5); });     // changed inside out, the images, ws
  refused([](Call& c) { c.ch = reinterpret_cast<unsigned*>(Call::x); });
  refused([](Call& c) { c.ch = reinterpret_cast<unsigned*>(Call::ws + 1030); });
  refused([&](Call& c) { c.logits = off(Call::v, 2); });                           // alignment
  refused([&](Call& c) { c.o = off(Call::out, 1); });
  refused([&](Call& c) { c.ch = off(Call::changed, 2); });
  refused([&](Call& c) { c.w = off(Call::ws, 2); });
  refused([](Call& c) { c.bytes -= 1; }, EFFQ_ERR_WORKSPACE);                      // a short workspace
  printf("%d of %d checks held\n", held, calls);
  return held == calls ? 0 : 1;
}
