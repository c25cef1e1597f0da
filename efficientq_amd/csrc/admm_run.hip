// The whole ADMM loop of one layer (EfficientQConv.py:99-144) enqueued by ONE C call.
//
// The loop body is launch-bound for most layers of a network (a few tens of microseconds of GPU work per iteration),
// so issuing it from the host language costs more than running it.  effq_admm_run() enqueues all iterations on up to
// three caller-owned HIP streams:
//   main : prox solve -> scale fixed point -> projection + dual update            (the serial chain)
//   loss : conv + squared error of iteration i, while main computes i+1            (best-iterate selection only)
//   side : the inverses of A(rho) for the later rho values, under the iterations that precede their first use
// Every per-iteration result the loss stream reads lives in a RING indexed by the iteration (G, its int8 operands,
// b*, the scale state): slots are written once, so main never waits for loss.  The squared errors land in hist[i];
// the best iterate is picked AFTER the loop (effq_admm_select_best), which is what lets a data-parallel caller
// all-reduce the whole history with one collective per layer instead of one per iteration.
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "common.h"
#include "internal.h"
#include "project_dual.h"

namespace effq {

// ---- sampling profiler of effq_admm_run (off by default): HIP-event pairs, on the stream the work is launched on,
// around the ops of every `every`-th iteration.  bench.py reads them back after the timed region.
struct ProfRec {
  int kind, iter, loss_kind, c2, n;
  effq_geom geom;
  hipEvent_t e0, e1;
};
static thread_local std::vector<ProfRec> g_prof;
static thread_local int g_prof_every = 0;
// PROF_WAIT brackets the points where the MAIN stream waits for another stream (the inverse of the next rho, the joins
// at the end of the layer): two records on the main stream around the wait = the time the chain stood still there
enum { PROF_PROX = 1, PROF_FIXED_POINT = 2, PROF_PROJECT = 3, PROF_LOSS = 4, PROF_INVERSE = 5, PROF_WAIT = 6 };

struct ProfScope {          // records e0 now, e1 at close()
  bool on;
  hipStream_t stream;
  ProfRec rec;
  ProfScope(bool enabled, int kind, int iter, const effq_admm_run_args* a, hipStream_t st) : on(enabled), stream(st) {
    if (!on) return;
    rec.kind = kind;
    rec.iter = iter;
    rec.loss_kind = a->loss_kind;
    rec.c2 = a->c2;
    rec.n = a->n;
    rec.geom = a->geom;
    if (hipEventCreate(&rec.e0) != hipSuccess || hipEventCreate(&rec.e1) != hipSuccess) {
      on = false;
      return;
    }
    (void)hipEventRecord(rec.e0, stream);
  }
  void close() {
    if (!on) return;
    (void)hipEventRecord(rec.e1, stream);
    g_prof.push_back(rec);
    on = false;
  }
};

constexpr int ADMM_MAX_RHOS = 16;

struct RhoPlan {
  int count;                       // distinct rho values, in order of first use
  double rho[ADMM_MAX_RHOS];
  int first_iter[ADMM_MAX_RHOS];   // iteration of first use
  bool shifted_first;              // rho[0] serves iteration 0 only: solved through the inverse of A(rho[1])
  bool overflow;
};

// EfficientQConv.py:129-137: at i % period == 0 (after the iteration), rho doubles while 2*rho <= rho_max, else -> rho_max
static RhoPlan plan_rhos(double rho, double rho_max, int iters, int period) {
  RhoPlan p;
  p.count = 0;
  p.overflow = false;
  double r = rho;
  for (int i = 0; i < iters; ++i) {
    if (p.count == 0 || p.rho[p.count - 1] != r) {
      if (p.count == ADMM_MAX_RHOS) {
        p.overflow = true;
        break;
      }
      p.rho[p.count] = r;
      p.first_iter[p.count] = i;
      ++p.count;
    }
    if (i % period == 0) r = (r * 2 <= rho_max) ? r * 2 : rho_max;
  }
  p.shifted_first = p.count > 1 && p.first_iter[1] == 1 && p.rho[1] > p.rho[0];
  return p;
}

static int shift_terms(double rho, double eta, double rho_inv) {
  // sweeps of the contraction (factor d / (rho_inv + eta)) to reach 2^-26
  const double d = rho_inv - rho;
  if (d <= 0) return 1;
  int t = (int)ceil(-26.0 * log(2.0) / log(d / (rho_inv + eta)));
  return t < 2 ? 2 : (t > 64 ? 64 : t);
}

// ---- Gram system packed for the data-parallel exchange: upper triangle of A0 (row-major, n(n+1)/2) then B0 (c2 x n) ----
__global__ __launch_bounds__(256) void k_gram_pack(const float* __restrict__ A0, const float* __restrict__ B0, int n, int c2,
                                                   float* __restrict__ buf) {
  const size_t tri = (size_t)n * (n + 1) / 2, nb = (size_t)c2 * n;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < (size_t)n * n + nb; e += stride) {
    if (e < (size_t)n * n) {
      const int i = (int)(e / n), j = (int)(e % n);
      if (j >= i) buf[(size_t)i * n - (size_t)i * (i - 1) / 2 + (j - i)] = A0[e];
    } else {
      buf[tri + (e - (size_t)n * n)] = B0[e - (size_t)n * n];
    }
  }
}
__global__ __launch_bounds__(256) void k_gram_unpack(const float* __restrict__ buf, int n, int c2, float* __restrict__ A0,
                                                     float* __restrict__ B0) {
  const size_t tri = (size_t)n * (n + 1) / 2, nb = (size_t)c2 * n;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < (size_t)n * n + nb; e += stride) {
    if (e < (size_t)n * n) {
      int i = (int)(e / n), j = (int)(e % n);
      if (j < i) {              // mirror: A0 is exactly symmetric
        const int t = i;
        i = j;
        j = t;
      }
      A0[e] = buf[(size_t)i * n - (size_t)i * (i - 1) / 2 + (j - i)];
    } else {
      B0[e - (size_t)n * n] = buf[tri + (e - (size_t)n * n)];
    }
  }
}

__global__ __launch_bounds__(256) void k_select_best(const double* __restrict__ hist, int iters,
                                                     const float* __restrict__ G_ring, const float* __restrict__ b_ring,
                                                     size_t nw, size_t nb, float* __restrict__ best_G,
                                                     float* __restrict__ best_b, double* __restrict__ best_out) {
  // "if i == 0 or lossf < best" (EfficientQConv.py:139-142): the EARLIEST minimum; every thread scans the same doubles
  int bi = 0;
  double bl = hist[0];
  for (int i = 1; i < iters; ++i) {
    const double l = hist[2 * (size_t)i];
    if (l < bl) {
      bl = l;
      bi = i;
    }
  }
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float* g = G_ring + (size_t)bi * nw;
  for (size_t i = t0; i < nw; i += stride) best_G[i] = g[i];
  if (b_ring != nullptr)
    for (size_t i = t0; i < nb; i += stride) best_b[i] = b_ring[(size_t)bi * nb + i];
  if (t0 == 0) {
    best_out[0] = bl;
    best_out[1] = (double)bi;
  }
}

// lwq_verbose (EfficientQConv.py:114-116): sum (w* - G)^2 and sum (G - G0)^2 of an iteration -> res[0], res[1] (the host
// takes the roots and multiplies the second by rho).  A diagnostic: fp64 atomics, printed to four decimals.
__global__ __launch_bounds__(256) void k_admm_residuals(const float* __restrict__ wstar, const float* __restrict__ G,
                                                        const float* __restrict__ G0, size_t n, double* __restrict__ res) {
  __shared__ double sh[2][4];
  double a = 0.0, b = 0.0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const double p = (double)wstar[i] - (double)G[i], q = (double)G[i] - (double)G0[i];
    a += p * p;
    b += q * q;
  }
  a = wave_sum_f64_dpp(a);
  b = wave_sum_f64_dpp(b);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    sh[0][wid] = a;
    sh[1][wid] = b;
  }
  __syncthreads();
  if (threadIdx.x < 2) atomicAdd(res + threadIdx.x, (sh[threadIdx.x][0] + sh[threadIdx.x][1]) + (sh[threadIdx.x][2] + sh[threadIdx.x][3]));
}

struct AdmmPlan {                  // what effq_admm_run decides once per layer
  int c2, n, has_b;
  size_t nw;                       // weights, c2 x (n - has_b)
  RhoPlan rhos;
  int first, n_inv;                // the n_inv inverses in ainv_pool are those of rhos.rho[first ...]
  size_t ainv_elems;               // floats per inverse
  bool chan, bucket, traj;         // channel mode; whether the bucketed / the trajectory fixed point may run
  int traj_after;                  // iterations after a change of rho before the trajectory fixed point
  hipStream_t s_main, s_loss, s_side, s_side2;
  bool fork_loss, fork_side, two_sides;
  int side_iter;                   // the iteration that enqueues the later inverses first (-1: there are none)
  int loss_group;                  // iterates the loss stream picks up at a time
  float* bm;                       // Bm, the right-hand side of the prox solve (start of prox_ws), rows of bm_ld
  int bm_ld;
};
// The argument and workspace checks, then the plan.  No HIP call: a rejected run has enqueued nothing.
static int admm_plan(const effq_admm_run_args* a, AdmmPlan* p) {
  EFFQ_CHECK_ARG(a != nullptr);
  EFFQ_CHECK_ARG(a->A0 && a->B0 && a->W0 && a->dual && a->wstar && a->v && a->G_ring && a->state_ring && a->hist &&
                 a->err_flag && a->ainv_pool && a->prox_ws && a->red_ws && a->inv_ws && a->conv_ws && a->y_fp);
  EFFQ_CHECK_ARG(a->c2 > 0 && a->n > 1 && a->iters > 0 && a->rho_period > 0 && a->w_levels >= 2 && a->w_levels <= 256);
  EFFQ_CHECK_ARG((a->has_bias != 0) == (a->b0 != nullptr) && (a->has_bias != 0) == (a->b_ring != nullptr));
  EFFQ_CHECK_ARG((a->loss_kind >= 0 && a->loss_kind <= 2) || a->loss_kind == 4 || a->loss_kind == 5);
  if (a->loss_kind == 4)
    EFFQ_CHECK_ARG(a->loss_Au != nullptr && a->loss_Bu != nullptr && a->loss_syy != nullptr);
  else if (a->loss_kind == 5)
    EFFQ_CHECK_ARG(a->loss_Au != nullptr && a->loss_Bu != nullptr && a->loss_syy != nullptr && a->loss_planes != nullptr &&
                   a->loss_nplanes > 0 && a->Gq_ring != nullptr && a->act_alpha_dev != nullptr &&
                   effq_gram_loss_i8_supported(a->c2, a->n, a->has_bias, a->w_levels));
  else
    EFFQ_CHECK_ARG(a->loss_kind == 0 ? (a->xq != nullptr) : (a->xidx != nullptr && a->Gq_ring != nullptr &&
                                                            a->act_alpha_dev != nullptr));
  p->c2 = a->c2;
  p->n = a->n;
  p->has_b = a->has_bias ? 1 : 0;
  const size_t nw = p->nw = (size_t)p->c2 * (size_t)(p->n - p->has_b);
  EFFQ_CHECK_ARG(nw == (size_t)a->geom.C2 * a->geom.C1 * a->geom.KD * a->geom.KH * a->geom.KW);
  // channel mode: one scale per output row (effq_fixed_point_channels_proj).  The integer loss paths fold ONE scalar scale
  // into their arithmetic (conv3d_i8*.hip epilogues, effq_gram_loss_i8's integer Q): only the losses that take G as fp32
  // values are accepted
  p->chan = a->channel_wise != 0;
  if (p->chan)
    EFFQ_CHECK_ARG((a->loss_kind == 0 || a->loss_kind == 4) && a->alpha_ring != nullptr &&
                   p->n - p->has_b <= effq_fp_channels_max_row());
  if (nw > effq_fp_coop_max()) {
    set_error("admm_run: %zu weights exceed the single-launch fixed points", nw);
    return EFFQ_ERR_ARG;
  }
  // weight-scale fixed point, by measured speed on MI355X (scripts/prof_fp.py, microseconds per call at 4 levels,
  // all-values kernel / bucketed: 2048 values 16 / 22; 8192 36 / 28; 27648 84 / 37; 110592 125 / 51; 442368 143 / 65;
  // 1.77 M 171 / 163 alone but slower inside the loop (1261 vs 1224 ms per calibration); at 256 levels the all-values
  // kernels win at every size)
  constexpr size_t bucket_max = (size_t)1 << 19;
  p->bucket = !p->chan && a->fp_ws != nullptr && a->w_levels <= 16 && nw > 4096 && nw <= bucket_max;
  if (p->bucket && a->fp_ws_bytes < effq_fp_bucket_ws_bytes(nw)) {
    set_error("admm_run: fixed-point workspace %zu < %zu", a->fp_ws_bytes, effq_fp_bucket_ws_bytes(nw));
    return EFFQ_ERR_WORKSPACE;
  }
  // ... and, where it is the faster one, the projection that starts from the previous iteration's iterates
  // (effq_fixed_point_traj: one launch, no grid barrier).  Its last workgroup scans lists whose length follows the drift
  // of the iterates from call to call, which is largest right after rho has changed: measured inside the calibration
  // (ms per calibration, all on one box: older kernels only 715; trajectory kernel from the third iteration of a layer on
  // 743; from 5 / 10 / 15 iterations after a change of rho, layers of 65 536 ... 2^20 weights only: 702 / 703 / 699; and
  // for larger layers from 30 iterations after: 698).  The iterations in between run the kernels above, which leave
  // their iterates behind.  (At 16 levels the fixed point takes ~50 iterations: the one hull slot for everything past the
  // seventh keeps a third of the values on the list, and the older kernels are faster - measured, scripts/prof_fp_traj.py;
  // hence at most 4 levels, effq_admm_uses_traj.)
  p->traj_after = (nw > ((size_t)1 << 20)) ? 30 : 12;
  p->traj = !p->chan && a->fp_pred != nullptr && a->fp_traj_ws != nullptr && effq_admm_uses_traj(nw, a->w_levels) != 0;
  if (p->traj && a->fp_traj_ws_bytes < effq_fp_traj_ws_bytes(nw)) {
    set_error("admm_run: trajectory fixed-point workspace %zu < %zu", a->fp_traj_ws_bytes, effq_fp_traj_ws_bytes(nw));
    return EFFQ_ERR_WORKSPACE;
  }
  p->rhos = plan_rhos(a->rho, a->rho_max, a->iters, a->rho_period);
  EFFQ_CHECK_ARG(!p->rhos.overflow);
  p->first = p->rhos.shifted_first ? 1 : 0;
  p->n_inv = p->rhos.count - p->first;
  EFFQ_CHECK_ARG(a->n_ainv >= p->n_inv);
  p->ainv_elems = (size_t)p->n * (size_t)effq_ainv_ld(p->n);
  p->s_main = as_stream(a->stream_main);
  p->s_loss = a->stream_loss ? as_stream(a->stream_loss) : p->s_main;
  p->s_side = (a->stream_side && a->inv_ws_side) ? as_stream(a->stream_side) : p->s_main;
  p->fork_loss = p->s_loss != p->s_main;
  p->fork_side = p->s_side != p->s_main;
  // a second side stream: the later inverses alternate between the two (a Gauss-Jordan sweep is a chain of ~100 dependent
  // launches with serial pivot phases: two sweeps side by side fill each other's bubbles, and the last inverse of a wide
  // layer is ready before the chain reaches the iteration that needs it)
  p->s_side2 = (p->fork_side && a->stream_side2 && a->inv_ws_side2) ? as_stream(a->stream_side2) : p->s_side;
  p->two_sides = p->s_side2 != p->s_side;
  // The later inverses (side stream) are ENQUEUED a few iterations into the loop: their ~30 - 650 launches take the host
  // 0.2 - 2.6 ms, during which the main stream - done with its own inverse on the small layers - had nothing queued (under
  // a profiler, at 3 x the launch cost, 6 ms per layer); the side stream still starts at the fork.  They are queued before
  // the iteration that uses the first of them, and at once without a side stream (they then run on the main stream).
  // (plan_rhos records first_iter only below iters, and first_iter[first + 1] >= 1: side_iter lies in [0, iters - 1], the
  // first iteration that met the condition the loop tested before, so no enqueue is left for after the loop.)
  constexpr int SIDE_AFTER_ITERS = 8;
  p->side_iter = p->n_inv <= 1 ? -1 : !p->fork_side ? 0 : std::min(SIDE_AFTER_ITERS, p->rhos.first_iter[p->first + 1] - 1);
  // loss group size: the last group is evaluated after the chain has finished (it delays the join by one group of
  // losses), so the cheap losses from the Gram system travel in larger groups than the conv passes.  EFFQ_LOSS_GROUP
  // overrides the Gram group (bench.py's model reads it too)
  static const int group_gram = getenv("EFFQ_LOSS_GROUP") ? atoi(getenv("EFFQ_LOSS_GROUP")) : 8;
  constexpr int group_conv = 4;
  const int group_size = (a->loss_kind == 4 || a->loss_kind == 5) ? group_gram : group_conv;
  p->loss_group = (p->fork_loss && group_size > 1) ? group_size : 1;
  p->bm = effq_prox_bm(a->prox_ws, p->c2, p->n, &p->bm_ld);
  return EFFQ_OK;
}

// The events of one run: the fork, one per inverse formed on a side stream, a few for main -> loss, one per join.  They
// come from a per-thread, per-device pool that is never destroyed (a wait captures the record that precedes it, so an
// event may be re-recorded by the next run while an older wait on it is still queued).
struct EventPool {
  std::vector<hipEvent_t>* pool = nullptr;
  size_t used = 0;
  hipError_t open() {              // the calling thread's pool of the current device
    static thread_local std::vector<std::vector<hipEvent_t>> per_device;
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess && (int)per_device.size() <= dev) per_device.resize(dev + 1);
    if (e == hipSuccess) pool = &per_device[dev];
    return e;
  }
  hipError_t take(hipEvent_t* ev) {
    if (used == pool->size()) {
      hipEvent_t fresh;
      const hipError_t e = hipEventCreateWithFlags(&fresh, hipEventDisableTiming);
      if (e != hipSuccess) return e;
      pool->push_back(fresh);
    }
    *ev = (*pool)[used++];
    return hipSuccess;
  }
  // into waits for what is queued on from so far, through ev or, if that is NULL, an event taken from the pool
  hipError_t hand_over(hipStream_t from, hipStream_t into, hipEvent_t ev = nullptr) {
    hipError_t e = ev ? hipSuccess : take(&ev);
    if (e == hipSuccess) e = hipEventRecord(ev, from);
    return e == hipSuccess ? hipStreamWaitEvent(into, ev, 0) : e;
  }
};

// The inverses of A(rho) for the later rho values, into ainv_pool; on a side stream each one records ev_inv[r].
static int enqueue_later_inverses(const effq_admm_run_args* a, const AdmmPlan& p, EventPool& events, hipEvent_t* ev_inv) {
  for (int r = p.first + 1; r < p.rhos.count; ++r) {
    float* dst = a->ainv_pool + (size_t)(r - p.first) * p.ainv_elems;
    const bool on2 = p.two_sides && ((r - p.first) % 2 == 0);   // first later inverse on side 1, the next on side 2 ...
    hipStream_t sr = on2 ? p.s_side2 : p.s_side;
    void* ws = !p.fork_side ? a->inv_ws : (on2 ? a->inv_ws_side2 : a->inv_ws_side);
    const size_t wsb = !p.fork_side ? a->inv_ws_bytes : (on2 ? a->inv_ws_side2_bytes : a->inv_ws_side_bytes);
    ProfScope ps(g_prof_every > 0, PROF_INVERSE, -1 - r, a, sr);
    const int rc = effq_spd_inverse(a->A0, p.n, p.has_b, p.rhos.rho[r], a->eta, dst, ws, wsb, sr);
    if (rc != EFFQ_OK) return rc;
    ps.close();
    if (p.fork_side) {
      EFFQ_HIP(events.take(&ev_inv[r]));
      EFFQ_HIP(hipEventRecord(ev_inv[r], sr));
    }
  }
  return EFFQ_OK;
}

struct AdmmIter {                  // iteration i: the rho it runs with and hands on, its slots of the rings
  int i;
  double rho, rho_next;
  float dual_div;                  // the dual's rescale for rho_next
  bool use_shift, use_traj, prof;  // use_shift: rho[0], solved through the inverse of A(rho[1])
  bool next_rhs;                   // not the last iteration: the projection leaves the next prox right-hand side in Bm
  const float* G_prev;
  float *G, *bstar;
  int8_t* Gq;
  effq_fp_state* st;
  ProxParts parts;                 // set by enqueue_prox where it leaves the K slices of the product for the trajectory
                                   // kernel to add up in its prologue (one launch less); part == NULL: the product is whole
};
static AdmmIter admm_iter(const effq_admm_run_args* a, const AdmmPlan& p, int i, double rho, bool use_traj) {
  const bool step = i % a->rho_period == 0, doubles = rho * 2 <= a->rho_max;   // rho changes after this iteration
  const bool use_shift = p.rhos.shifted_first && i == 0;
  const bool prof = g_prof_every > 0 && !use_shift && (i % g_prof_every) == g_prof_every / 2;
  return AdmmIter{i, rho, !step ? rho : doubles ? rho * 2 : a->rho_max,
                  !step ? 1.0f : doubles ? 2.0f : (float)(a->rho_max / rho), use_shift, use_traj, prof, i + 1 < a->iters,
                  (i == 0) ? a->W0 : a->G_ring + (size_t)(i - 1) * p.nw, a->G_ring + (size_t)i * p.nw,
                  p.has_b ? a->b_ring + (size_t)i * p.c2 : nullptr, a->Gq_ring ? a->Gq_ring + (size_t)i * p.nw : nullptr,
                  a->state_ring + i, ProxParts{nullptr, 1, 0}};
}

static int enqueue_prox(const effq_admm_run_args* a, const AdmmPlan& p, AdmmIter* it, const float* Ainv, bool bm_ready) {
  // prebuilt: Bm written by the last projection or not
  ProxSolve s = {a->B0, Ainv, a->W0, a->b0, it->G_prev, a->dual, p.c2, p.n, p.has_b, it->rho, a->eta, 0.0, 1, bm_ready,
                 a->wstar, it->bstar, a->prox_ws, a->prox_ws_bytes, nullptr};
  if (it->use_shift) {             // through the inverse of A(rho[1]), its Bm rebuilt for every term
    const double rho_inv = p.rhos.rho[1];
    EFFQ_CHECK_ARG(rho_inv >= it->rho && it->rho > 0.0 && a->eta >= 0.0);
    s.Ainv = a->ainv_pool;
    s.shift = rho_inv - it->rho;
    s.nterms = shift_terms(it->rho, a->eta, rho_inv);
    s.prebuilt = false;
  } else if (bm_ready && it->use_traj && p.c2 <= 512) {
    s.parts = &it->parts;
  }
  return effq_prox_enqueue(&s, p.s_main);
}

enum class FpKind { channels, traj, bucket, small, coop };   // the weight-scale fixed point of an iteration
static FpKind fp_kind(const AdmmPlan& p, bool use_traj) {
  if (p.chan) return FpKind::channels;
  if (use_traj) return FpKind::traj;
  if (p.bucket) return FpKind::bucket;
  return p.nw <= effq_fp_small_max() ? FpKind::small : FpKind::coop;
}

// The fixed point, then the projection + dual update, which also leaves the right-hand side of the NEXT prox solve in
// Bm (the first solve of the layer builds Bm itself: bias column, padding).  *bm_ready: Bm holds it.
static int enqueue_fixed_point(const effq_admm_run_args* a, const AdmmPlan& p, const AdmmIter& it, bool* bm_ready) {
  const int nwrow = p.n - p.has_b;
  ProjNext nx;                     // zero (Bm == NULL) on the last iteration
  memset(&nx, 0, sizeof(nx));
  if (it.next_rhs) nx = ProjNext{p.bm, a->B0, a->W0, nwrow, p.n, p.bm_ld, (float)it.rho_next, (float)a->eta};
  const ProjNext* nxp = it.next_rhs ? &nx : nullptr;
  const FpKind kind = fp_kind(p, it.use_traj);
  // The projection as the EPILOGUE of a single-workgroup fixed point: one launch per iteration less.  Measured (us per
  // iteration, fused against fixed point + projection): 2048 weights 13.8 against 12.2 + 7.1, 3456 at 256 levels 231.8
  // against 229.3 + 8.3.  So: the small kernel's layers (<= 32768 weights), and the channel kernel.  (The bucketed kernel
  // has only the 256 threads of its iteration phase left for an epilogue: slower, DESIGN.md.)
  const bool fuse_proj = kind == FpKind::channels ||
                         (kind == FpKind::small && proj_vec_ok(a->v, a->wstar, it.G, a->dual, it.Gq, p.nw, nxp));
  ProjFused pf;                    // (the small kernel's epilogue)
  memset(&pf, 0, sizeof(pf));
  pf.wstar = a->wstar; pf.G = it.G; pf.dual = a->dual; pf.Gq = it.Gq; pf.err_flag = a->err_flag;
  pf.d = 2.0 / (double)(a->w_levels - 1); pf.dual_div = it.dual_div; pf.lm1 = a->w_levels - 1;
  pf.n4 = (unsigned)(p.nw / 4);
  pf.nx = nx;
  void* rec = p.traj ? a->fp_pred : nullptr;
  const int maxit = 100 * a->w_levels;
  ProfScope p_fp(it.prof, PROF_FIXED_POINT, it.i, a, p.s_main);
  int rc;
  if (kind == FpKind::channels)       // every row's fixed point, projection, dual update and the next Bm in one launch
    rc = effq_fixed_point_channels_proj(a->wstar, a->dual, a->v, p.c2, nwrow, a->w_levels, a->tol, maxit,
                                        a->alpha_ring + (size_t)it.i * p.c2,
                                        a->w_iters_ring ? a->w_iters_ring + (size_t)it.i * p.c2 : nullptr, a->err_flag,
                                        it.G, it.dual_div, it.next_rhs ? p.bm : nullptr, a->B0, a->W0, p.n, p.bm_ld,
                                        it.rho_next, a->eta, p.s_main);
  else if (kind == FpKind::traj && it.parts.part != nullptr)
    rc = effq_fixed_point_traj_parts(it.parts.part, it.parts.nsplit, it.parts.ldp, p.c2, nwrow, p.has_b, a->dual, a->wstar, it.bstar,
                                     a->v, a->w_levels, -1.0, 1.0, a->tol, maxit, it.st, a->fp_pred, a->fp_traj_ws,
                                     a->fp_traj_ws_bytes, p.s_main);
  else if (kind == FpKind::traj)
    rc = effq_fixed_point_traj(a->wstar, a->dual, a->v, p.nw, a->w_levels, -1.0, 1.0, a->tol, maxit, it.st, a->fp_pred,
                               a->fp_traj_ws, a->fp_traj_ws_bytes, p.s_main);
  else if (kind == FpKind::bucket)
    rc = effq_fixed_point_bucket_rec(a->wstar, a->dual, a->v, p.nw, a->w_levels, -1.0, 1.0, a->tol, maxit, it.st, a->fp_ws,
                                     a->fp_ws_bytes, rec, p.s_main);
  else if (kind == FpKind::small)
    rc = effq_fixed_point_small_fused(a->wstar, a->dual, a->v, p.nw, a->w_levels, -1.0, 1.0, a->tol, maxit, it.st,
                                      fuse_proj ? &pf : nullptr, p.s_main);
  else
    rc = effq_fixed_point_coop_rec(a->wstar, a->dual, a->v, p.nw, a->w_levels, -1.0, 1.0, a->tol, maxit, it.st, a->red_ws,
                                   rec, p.s_main);
  if (rc != EFFQ_OK) return rc;
  p_fp.close();
  *bm_ready = it.next_rhs;
  if (fuse_proj) return EFFQ_OK;
  ProfScope p_pr(it.prof, PROF_PROJECT, it.i, a, p.s_main);
  rc = effq_project_dual_impl(a->v, a->wstar, it.st, a->w_levels, it.G, a->dual, it.dual_div, it.Gq, p.nw, a->err_flag,
                              nxp, p.s_main);
  if (rc != EFFQ_OK) return rc;
  p_pr.close();
  return EFFQ_OK;
}

// The losses of iterates j0 .. i, on the loss stream: kind 5 for up to 16 iterates in one launch pair (the digit planes of
// the Gram system are read once per group), the other kinds one iterate at a time.
static int enqueue_losses(const effq_admm_run_args* a, const AdmmPlan& p, int j0, int i) {
  const int step = a->loss_kind == 5 ? 16 : 1;
  for (int j = j0; j <= i; j += step) {
    const int cnt = (i - j + 1 < step) ? (i - j + 1) : step;
    const float* Gj = a->G_ring + (size_t)j * p.nw;
    const int8_t* Gqj = a->Gq_ring ? a->Gq_ring + (size_t)j * p.nw : nullptr;
    const float* bj = p.has_b ? a->b_ring + (size_t)j * p.c2 : nullptr;
    const effq_fp_state* stj = a->state_ring + j;
    double* sq = a->hist + 2 * (size_t)j;
    const bool prof = g_prof_every > 0 && (a->loss_kind == 5 ? (j / p.loss_group) % 2 == 1 :
                      !(p.rhos.shifted_first && j == 0) && (j % g_prof_every) == g_prof_every / 2);
    ProfScope p_loss(prof, PROF_LOSS, j, a, p.s_loss);
    int rc;
    if (a->loss_kind == 5)
      rc = effq_gram_loss_i8(a->loss_planes, a->loss_nplanes, a->loss_Au, a->loss_Bu, a->loss_syy, Gqj, bj, stj,
                             a->act_alpha_dev, a->act_levels, a->w_levels, p.c2, p.n, p.has_b, cnt, sq, a->conv_ws,
                             a->conv_ws_bytes, p.s_loss);
    else if (a->loss_kind == 1)
      rc = conv3d_calib_step_i8(a->xidx, Gqj, bj, a->y_fp, &a->geom, a->act_alpha_dev, a->act_levels, stj, a->w_levels,
                                sq, a->conv_ws, a->conv_ws_bytes, p.s_loss);
    else if (a->loss_kind == 2)
      rc = conv3d_calib_step_i8s(a->xidx, Gqj, bj, a->y_fp, &a->geom, a->act_alpha_dev, a->act_levels, stj, a->w_levels,
                                 j == 0 ? 1 : 0, sq, a->conv_ws, a->conv_ws_bytes, p.s_loss);
    else if (a->loss_kind == 4)
      rc = effq_gram_loss(a->loss_Au, a->loss_Bu, a->loss_syy, Gj, bj, p.c2, p.n, p.has_b, sq, a->conv_ws,
                          a->conv_ws_bytes, p.s_loss);
    else
      rc = conv3d_quant_calib_step(a->xq, Gj, bj, a->y_fp, nullptr, &a->geom, nullptr, 0, sq, nullptr, a->conv_ws,
                                   a->conv_ws_bytes, p.s_loss);   // unweighted MSE (quirk Q5)
    if (rc != EFFQ_OK) return rc;
    p_loss.close();
  }
  return EFFQ_OK;
}

}  // namespace effq
using namespace effq;

extern "C" {

// whether effq_admm_run would use effq_fixed_point_traj for a layer of nw weights at w_levels levels (the caller then
// provides fp_pred / fp_traj_ws; otherwise both may be NULL)
int effq_admm_uses_traj(size_t nw, int w_levels) {
  constexpr int traj_levels = 4;          // see the measurements in admm_plan
  constexpr size_t traj_min = 65536;
  return (w_levels <= traj_levels && nw >= traj_min && nw <= effq_fp_traj_max()) ? 1 : 0;
}

int effq_admm_num_inverses(double rho, double rho_max, int iters, int period) {
  if (!(rho > 0.0) || iters <= 0 || period <= 0) return -1;
  const RhoPlan p = plan_rhos(rho, rho_max, iters, period);
  if (p.overflow) return -1;
  return p.count - (p.shifted_first ? 1 : 0);
}

int effq_admm_run(const effq_admm_run_args* a) {
  AdmmPlan p;
  if (const int rc = admm_plan(a, &p); rc != EFFQ_OK) return rc;
  constexpr int LOSS_EVENTS = 4;
  EventPool events;
  EFFQ_HIP(events.open());
  hipEvent_t ev_inv[ADMM_MAX_RHOS] = {}, ev_loss[LOSS_EVENTS] = {};
  EFFQ_HIP(hipMemsetAsync(a->dual, 0, p.nw * sizeof(float), p.s_main));               // dual <- 0 (EfficientQConv.py:40)
  if (a->res_ring != nullptr) EFFQ_HIP(hipMemsetAsync(a->res_ring, 0, 2 * (size_t)a->iters * sizeof(double), p.s_main));
  if (p.traj) EFFQ_HIP(hipMemsetAsync(a->fp_pred, 0, effq_fp_traj_pred_bytes(), p.s_main));   // nothing known about this layer
  // the inverse the first iterations need, on the main stream; the later ones on the side stream, which starts at once,
  // beside the first inverse (all of them only read A0): with n = 13825 an inverse takes longer than the 50 iterations it has
  // to be ready after, and the chain waited for each of the three later ones in turn (LiTS: 3.08 -> 3.03 s per calibration;
  // BraTS 900 -> 893 ms).
  if (p.fork_side && p.n_inv > 1) {
    hipEvent_t ev_fork;
    EFFQ_HIP(events.take(&ev_fork));
    EFFQ_HIP(hipEventRecord(ev_fork, p.s_main));         // A0 (and everything before the call) is ready
    EFFQ_HIP(hipStreamWaitEvent(p.s_side, ev_fork, 0));
    if (p.two_sides) EFFQ_HIP(hipStreamWaitEvent(p.s_side2, ev_fork, 0));
  }
  ProfScope p_inv(g_prof_every > 0, PROF_INVERSE, -1, a, p.s_main);
  if (const int rc = effq_spd_inverse(a->A0, p.n, p.has_b, p.rhos.rho[p.first], a->eta, a->ainv_pool, a->inv_ws,
                                      a->inv_ws_bytes, p.s_main); rc != EFFQ_OK)
    return rc;
  p_inv.close();
  if (p.fork_loss)
    for (int e = 0; e < LOSS_EVENTS; ++e) EFFQ_HIP(events.take(&ev_loss[e]));
  bool bm_ready = false;
  const float* Ainv = nullptr;
  int k = 0;                       // p.rhos.rho[k]: this iteration's rho (plan_rhos ran the schedule of EfficientQConv.py)
  int cur = -1;                    // index into p.rhos.rho of the inverse in use
  int loss_next = 0;
  for (int i = 0; i < a->iters; ++i) {
    if (k + 1 < p.rhos.count && p.rhos.first_iter[k + 1] == i) ++k;
    if (i == p.side_iter)
      if (const int rc = enqueue_later_inverses(a, p, events, ev_inv); rc != EFFQ_OK) return rc;
    // (iterations since rho last changed: the drift from call to call - and with it the length of the lists the
    // trajectory kernel's single last workgroup has to scan - is largest right after a change.  traj_after >= 12 also
    // keeps it off the first two iterations and off the one after a change, whose dual is rescaled.)
    AdmmIter it = admm_iter(a, p, i, p.rhos.rho[k], p.traj && i - p.rhos.first_iter[k] >= p.traj_after);
    if (!it.use_shift && cur != k) {
      EFFQ_CHECK_ARG(p.rhos.rho[k] == p.rhos.rho[k]);   // (a NaN rho, from a NaN rho_max, has no inverse)
      if (p.fork_side && ev_inv[k] != nullptr) {
        ProfScope p_wait(g_prof_every > 0, PROF_WAIT, i, a, p.s_main);
        EFFQ_HIP(hipStreamWaitEvent(p.s_main, ev_inv[k], 0));
        p_wait.close();
      }
      Ainv = a->ainv_pool + (size_t)(k - p.first) * p.ainv_elems;
      cur = k;
    }
    // ---- the chain (main stream) ----
    ProfScope p_prox(it.prof, PROF_PROX, i, a, p.s_main);
    if (const int rc = enqueue_prox(a, p, &it, Ainv, bm_ready); rc != EFFQ_OK) return rc;
    p_prox.close();
    if (const int rc = enqueue_fixed_point(a, p, it, &bm_ready); rc != EFFQ_OK) return rc;
    if (a->res_ring != nullptr) {                 // lwq_verbose: residuals of this iteration (w* is overwritten by the next)
      const size_t nb = std::min<size_t>((p.nw + 1023) / 1024, 256);
      hipLaunchKernelGGL(k_admm_residuals, dim3((unsigned)nb), dim3(256), 0, p.s_main, a->wstar, it.G, it.G_prev, p.nw,
                         a->res_ring + 2 * (size_t)i);
      EFFQ_LAUNCH_CHECK();
    }
    // ---- the losses (loss stream), in groups of loss_group iterates ----
    // An event record is a barrier packet in the main queue: the next chain kernel starts ~7 us later than it would
    // behind a kernel (kernel trace: the only gap of an iteration sat between the projection and the next prox GEMM).
    // The iterates are kept in rings, so the loss stream may as well pick them up a few at a time.
    if (!p.fork_loss || (i + 1) % p.loss_group == 0 || i + 1 == a->iters) {
      if (p.fork_loss) EFFQ_HIP(events.hand_over(p.s_main, p.s_loss, ev_loss[(i / p.loss_group) % LOSS_EVENTS]));
      if (const int rc = enqueue_losses(a, p, loss_next, i); rc != EFFQ_OK) return rc;
      loss_next = i + 1;
    }
  }
  // join: everything the caller reads next (hist, rings) is ordered on the main stream
  ProfScope p_join(g_prof_every > 0 && (p.fork_loss || p.fork_side), PROF_WAIT, a->iters, a, p.s_main);
  if (p.fork_loss) EFFQ_HIP(events.hand_over(p.s_loss, p.s_main));
  if (p.fork_side && p.n_inv > 1) EFFQ_HIP(events.hand_over(p.s_side, p.s_main));
  if (p.fork_side && p.n_inv > 1 && p.two_sides) EFFQ_HIP(events.hand_over(p.s_side2, p.s_main));
  p_join.close();
  return EFFQ_OK;
}

size_t effq_gram_packed_elems(int n, int c2) {
  return (n > 0 && c2 > 0) ? (size_t)n * (n + 1) / 2 + (size_t)c2 * n : 0;
}

int effq_gram_pack(const float* A0, const float* B0, int n, int c2, float* buf, void* stream) {
  EFFQ_CHECK_ARG(A0 && B0 && buf && n > 0 && c2 > 0);
  size_t blocks = ((size_t)n * n + (size_t)c2 * n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(k_gram_pack, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), A0, B0, n, c2, buf);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_gram_unpack(const float* buf, int n, int c2, float* A0, float* B0, void* stream) {
  EFFQ_CHECK_ARG(A0 && B0 && buf && n > 0 && c2 > 0);
  size_t blocks = ((size_t)n * n + (size_t)c2 * n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(k_gram_unpack, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), buf, n, c2, A0, B0);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_prof_enable(int every) {
  for (ProfRec& r : g_prof) {
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
  }
  g_prof.clear();
  g_prof_every = every > 0 ? every : 0;
  return EFFQ_OK;
}

int effq_prof_count(void) { return (int)g_prof.size(); }

int effq_prof_read(int i, effq_prof_record* out) {
  EFFQ_CHECK_ARG(out != nullptr && i >= 0 && i < (int)g_prof.size());
  const ProfRec& r = g_prof[(size_t)i];
  float ms = 0.0f;
  EFFQ_HIP(hipEventElapsedTime(&ms, r.e0, r.e1));      // the caller has synchronised the device
  out->kind = r.kind;
  out->iter = r.iter;
  out->loss_kind = r.loss_kind;
  out->c2 = r.c2;
  out->n = r.n;
  out->geom = r.geom;
  out->ms = ms;
  return EFFQ_OK;
}

int effq_admm_select_best(const double* hist, int iters, const float* G_ring, const float* b_ring, size_t nw, size_t nb,
                          float* best_G, float* best_b, double* best_out, void* stream) {
  EFFQ_CHECK_ARG(hist && G_ring && best_G && best_out && iters > 0 && nw > 0);
  EFFQ_CHECK_ARG((b_ring == nullptr) == (best_b == nullptr));
  size_t blocks = (nw + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(k_select_best, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), hist, iters, G_ring, b_ring,
                     nw, nb, best_G, best_b, best_out);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
