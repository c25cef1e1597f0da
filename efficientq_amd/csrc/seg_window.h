// The sliding-window rule of window.hip (gather, put, stitch): one definition of the window starts, the raster numbering
// and the argument checks.  seg_eval.hip sizes its grids with grid_for.
//
// Windows: along each axis the starts are  min(i * (patch - overlap), size - patch)  for i = 0 .. n-1 with
// n = ceil((size - patch) / (patch - overlap)) + 1, i.e. evaluate.window_starts: steps while a whole patch ends strictly
// before the border, then one patch flush with it.  Windows are numbered in (d, h, w) raster order.
#pragma once
#include "common.h"

namespace effq {

struct WinAxes {
  int D, H, W;        // volume extent
  int pd, ph, pw;     // window extent
  int sd, sh, sw;     // step = patch - overlap
  int nd, nh, nw;     // windows per axis
};

constexpr int STITCH_MAX_C = 8;

static inline int n_windows(int size, int patch, int step) {
  return (size - patch + step - 1) / step + 1;
}

__device__ __forceinline__ int win_start(int i, int size, int patch, int step) {
  const int s = i * step;
  return s < size - patch ? s : size - patch;
}

static bool make_axes(int D, int H, int W, int pd, int ph, int pw, int od, int oh, int ow, WinAxes& a) {
  if (pd <= 0 || ph <= 0 || pw <= 0 || pd > D || ph > H || pw > W) return false;
  if (od < 0 || oh < 0 || ow < 0 || od >= pd || oh >= ph || ow >= pw) return false;
  a.D = D; a.H = H; a.W = W; a.pd = pd; a.ph = ph; a.pw = pw;
  a.sd = pd - od; a.sh = ph - oh; a.sw = pw - ow;
  a.nd = n_windows(D, pd, a.sd); a.nh = n_windows(H, ph, a.sh); a.nw = n_windows(W, pw, a.sw);
  return true;
}

static unsigned grid_for(size_t items, size_t cap) {
  size_t nb = (items + 255) / 256;
  if (nb < 1) nb = 1;
  return (unsigned)(nb < cap ? nb : cap);
}

}  // namespace effq
