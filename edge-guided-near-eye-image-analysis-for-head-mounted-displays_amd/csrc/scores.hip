// Score tracking of train.py / test.py on the device (egne_amd.scores): what the reference's loops compute per batch on host copies
// of the class map and the labels (utils.py:120-170 getSeg_metrics / getPoint_metric / getAng_metric, train.py:289-338) from the
// tensors that are in HBM already.  Two launches per batch, nothing synchronises, results stay on the device:
//
// egne_seg_confusion_counts:  counts_k   one read of the two int64 maps (16 bytes per pixel) -> per frame and class (n_true, n_pred, n_both)
// egne_score_rows:            rows_k     one thread per sample: the counts and the ellipse vectors -> one row of float64 in a ledger
//
// rows_k restates float32 / float64 NumPy and torch expressions operation for operation (tests/scores_refs.py); this file is compiled
// without FMA contraction (Makefile).  Division and square root are the correctly rounded ones (hipcc's default for fp32, always for fp64).
#include "common.h"

namespace {

constexpr int kThreads = 256;                       // four waves
constexpr int kWaves = kThreads / 64;
constexpr int kStep = kThreads * 2;                 // pixels one pass of the workgroup covers: a pair per lane
constexpr int kChunk = EGNE_SCORES_CHUNK;           // pixels of a frame per workgroup
constexpr int kMaxCls = 3;
static_assert(kChunk % kStep == 0, "a chunk is a whole number of passes, so that chunk starts keep the pairs' alignment");

typedef long long ll2 __attribute__((ext_vector_type(2)));

// class of a stored value, or -1 for anything outside [0, ncls): such a pixel counts for no class
__device__ __forceinline__ int cls_of(long long v, int ncls) { return (v >= 0 && v < ncls) ? (int)v : -1; }

// A frame's pixels are walked in a coordinate q = p + head, where head (0 or 1) is the number of int64 elements between the last
// 16-byte boundary and the frame's first element: pairs (q, q + 1) with q even are then 16-byte aligned in BOTH maps whenever the two
// base pointers agree modulo 16 (VEC; with H * W odd every second frame starts only 8-byte aligned, head = 1 there).  q = 0 with
// head = 1 is the element BEFORE the frame and is never read; nor is q = n + head.  Without VEC every element is an 8-byte load.
// grid (chunks, B), 256 threads.  cnt[f][c] = (n_true, n_pred, n_both), zeroed by the caller; one atomic add per non-zero counter.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void counts_k(const long long* __restrict__ yt, const long long* __restrict__ yp, int n, int ncls,
                                                     int base_head, unsigned* __restrict__ cnt) {
  __shared__ unsigned sh[kWaves][kMaxCls * 3];
  const int f = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long fo = (long long)f * n;
  const int head = VEC ? (int)((fo + base_head) & 1) : 0;
  const long long* t = yt + fo - head;              // indexed by q; t[0] is outside the frame when head = 1
  const long long* p = yp + fo - head;
  const long long lo = head, hi = (long long)n + head;        // valid q: [lo, hi)
  const long long q_begin = (long long)blockIdx.x * kChunk;
  const long long q_end = q_begin + kChunk < hi ? q_begin + kChunk : hi;
  unsigned acc[kMaxCls * 3];
#pragma unroll
  for (int k = 0; k < kMaxCls * 3; ++k) acc[k] = 0;

  // ballot + popcount into wave-uniform counters; both = the AND of the two lane masks
  auto tally = [&](int ct, int cp) {
#pragma unroll
    for (int c = 0; c < kMaxCls; ++c) {
      const unsigned long long mt = __builtin_amdgcn_ballot_w64(ct == c), mp = __builtin_amdgcn_ballot_w64(cp == c);
      acc[3 * c] += (unsigned)__builtin_popcountll(mt);
      acc[3 * c + 1] += (unsigned)__builtin_popcountll(mp);
      acc[3 * c + 2] += (unsigned)__builtin_popcountll(mt & mp);
    }
  };

  for (long long q0 = q_begin; q0 < q_end; q0 += kStep) {      // (bounds are uniform over the workgroup: every lane takes every ballot)
    const long long q = q0 + 2 * threadIdx.x;
    int ct0 = -1, cp0 = -1, ct1 = -1, cp1 = -1;
    if (q0 >= lo && q0 + kStep <= q_end) {                     // a whole pass inside the frame: one 16-byte load per map and lane
      if (VEC) {
        const ll2 a = *reinterpret_cast<const ll2*>(t + q), b = *reinterpret_cast<const ll2*>(p + q);
        ct0 = cls_of(a[0], ncls); ct1 = cls_of(a[1], ncls); cp0 = cls_of(b[0], ncls); cp1 = cls_of(b[1], ncls);
      } else {
        ct0 = cls_of(t[q], ncls); ct1 = cls_of(t[q + 1], ncls); cp0 = cls_of(p[q], ncls); cp1 = cls_of(p[q + 1], ncls);
      }
    } else {                                                   // the frame's first pass (head) and a chunk's ragged last one
      if (q >= lo && q < q_end) { ct0 = cls_of(t[q], ncls); cp0 = cls_of(p[q], ncls); }
      if (q + 1 >= lo && q + 1 < q_end) { ct1 = cls_of(t[q + 1], ncls); cp1 = cls_of(p[q + 1], ncls); }
    }
    tally(ct0, cp0);
    tally(ct1, cp1);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kMaxCls * 3; ++k) sh[wave][k] = acc[k];
  }
  __syncthreads();
  if ((int)threadIdx.x < ncls * 3) {
    unsigned s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += sh[w][threadIdx.x];
    if (s) atomicAdd(cnt + (long long)f * ncls * 3 + threadIdx.x, s);
  }
}

struct RowArgs {
  const unsigned* cnt;
  const float *elOut, *elPred, *pc, *ic, *elNorm, *cond, *loss;
  int B, ncls, ncond, H, W, batch_no;
  double* rows;
};

__device__ __forceinline__ double centre_dist(const float* gt, const float* pred, float hw, float hh) {
  // utils.unnormPts then utils.getPoint_metric on float32 arrays: (0.5 * W) * (x + 1), differences, squares, one add, sqrt
  const float ux = hw * (pred[0] + 1.0f), uy = hh * (pred[1] + 1.0f);
  const float dx = gt[0] - ux, dy = gt[1] - uy;
  const float s = dx * dx + dy * dy;
  return (double)sqrtf(s);
}

__device__ __forceinline__ double scale_ratio(const float* gt_ab, const float* pred_ab) {
  // train.py:323-329, sqrt(sum(gt ** 2) / sum(pred ** 2)) in float32 with every operation rounded once; a zero denominator gives inf or NaN,
  // as torch.  (torch's own CPU square root is within an ulp of this one and differs between hosts: tests/scores_refs.py)
  const float g = gt_ab[0] * gt_ab[0] + gt_ab[1] * gt_ab[1], q = pred_ab[0] * pred_ab[0] + pred_ab[1] * pred_ab[1];
  return (double)sqrtf(g / q);
}

// one thread per sample; row layout: EGNE_SCORE_* of include/egne_hip.h
__global__ __launch_bounds__(64) void rows_k(RowArgs a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.B) return;
  const double nan = __builtin_nan("");
  double* r = a.rows + (long long)i * EGNE_SCORE_FIELDS;
  const float c0 = a.cond[(long long)i * a.ncond], c1 = a.cond[(long long)i * a.ncond + 1];
  const bool skip = c1 != 0.0f;
  for (int c = 0; c < 3; ++c) {
    double v = nan;
    if (!skip && c < a.ncls) {
      const unsigned* k = a.cnt + ((long long)i * a.ncls + c) * 3;
      const unsigned nt = k[0], np = k[1], nb = k[2];
      // utils._jaccard over the classes np.unique finds in the truth: n_both / union as ONE float64 division (nt > 0 makes the union > 0)
      if (nt != 0) v = (double)nb / (double)((unsigned long long)nt + np - nb);
    }
    r[EGNE_SCORE_IOU + c] = v;
  }
  const float hw = 0.5f * (float)a.W, hh = 0.5f * (float)a.H;      // (exact: the host forms 0.5 * W in float64 and NumPy narrows it)
  const float *eo = a.elOut + (long long)i * 10, *ep = a.elPred + (long long)i * 10, *en = a.elNorm + (long long)i * 10;
  r[EGNE_SCORE_DIST_PUPIL_LATENT] = centre_dist(a.pc + 2 * (long long)i, eo + 5, hw, hh);
  r[EGNE_SCORE_DIST_PUPIL_SEG] = centre_dist(a.pc + 2 * (long long)i, ep + 5, hw, hh);
  r[EGNE_SCORE_DIST_IRIS_LATENT] = centre_dist(a.ic + 2 * (long long)i, eo, hw, hh);
  r[EGNE_SCORE_DIST_IRIS_SEG] = centre_dist(a.ic + 2 * (long long)i, ep, hw, hh);
  // utils.getAng_metric: float32 |a - b|, widened, times the constant of np.rad2deg (180.0 / pi in float64)
  const double deg = 180.0 / 3.141592653589793238462643383279502884;
  r[EGNE_SCORE_ANG_IRIS] = (double)fabsf(en[4] - eo[4]) * deg;
  r[EGNE_SCORE_ANG_PUPIL] = (double)fabsf(en[9] - eo[9]) * deg;
  r[EGNE_SCORE_SCALE_IRIS] = scale_ratio(en + 2, eo + 2);
  r[EGNE_SCORE_SCALE_PUPIL] = scale_ratio(en + 7, eo + 7);
  r[EGNE_SCORE_COND0] = c0 != 0.0f ? 1.0 : 0.0;
  r[EGNE_SCORE_COND1] = skip ? 1.0 : 0.0;
  r[EGNE_SCORE_LOSS] = a.loss ? (double)a.loss[0] : nan;
  r[EGNE_SCORE_BATCH] = (double)a.batch_no;
  r[EGNE_SCORE_SAMPLE] = (double)i;
}

}  // namespace

extern "C" int egne_seg_confusion_counts(const void* y_true, const void* y_pred, int B, int H, int W, int ncls, void* counts, void* stream) {
  EGNE_REQUIRE(y_true && y_pred && counts, "egne_seg_confusion_counts: null pointer");
  EGNE_REQUIRE(B > 0 && H > 0 && W > 0, "egne_seg_confusion_counts: B, H, W must be positive (got %d, %d, %d)", B, H, W);
  EGNE_REQUIRE(ncls == 2 || ncls == 3, "egne_seg_confusion_counts: ncls must be 2 or 3 (got %d)", ncls);
  EGNE_REQUIRE((long long)H * W < (1ll << 31), "egne_seg_confusion_counts: H * W must stay below 2^31 (the counters are 32-bit)");
  EGNE_REQUIRE(B <= 65535, "egne_seg_confusion_counts: at most 65535 frames per call (got %d)", B);
  const uintptr_t at = (uintptr_t)y_true, ap = (uintptr_t)y_pred;
  EGNE_REQUIRE(at % 8 == 0 && ap % 8 == 0 && (uintptr_t)counts % 4 == 0, "egne_seg_confusion_counts: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  const int n = H * W;
  if (hipMemsetAsync(counts, 0, (size_t)B * ncls * 3 * sizeof(unsigned), st) != hipSuccess) return egne::check_launch("egne_seg_confusion_counts: memset");
  const dim3 grid(egne::cdiv((long long)n + 1, kChunk), B);        // (+ 1: the walk starts one element early in frames with head = 1)
  if (((at ^ ap) & 15) == 0)
    counts_k<true><<<grid, kThreads, 0, st>>>((const long long*)y_true, (const long long*)y_pred, n, ncls, (int)((at >> 3) & 1), (unsigned*)counts);
  else
    counts_k<false><<<grid, kThreads, 0, st>>>((const long long*)y_true, (const long long*)y_pred, n, ncls, 0, (unsigned*)counts);
  return egne::check_launch("egne_seg_confusion_counts");
}

extern "C" int egne_score_rows(const void* counts, int B, int ncls, const void* elOut, const void* elPred, const void* pupil_center,
                               const void* iris_center, const void* elNorm, const void* cond, int ncond, const void* loss_terms, int H, int W,
                               int batch_no, void* ledger, int64_t row_offset, int64_t capacity_rows, void* stream) {
  EGNE_REQUIRE(counts && elOut && elPred && pupil_center && iris_center && elNorm && cond && ledger, "egne_score_rows: null pointer");
  EGNE_REQUIRE(B > 0 && H > 0 && W > 0, "egne_score_rows: B, H, W must be positive (got %d, %d, %d)", B, H, W);
  EGNE_REQUIRE(ncls == 2 || ncls == 3, "egne_score_rows: ncls must be 2 or 3 (got %d)", ncls);
  EGNE_REQUIRE(ncond >= 2, "egne_score_rows: cond needs two columns (got %d)", ncond);
  EGNE_REQUIRE(row_offset >= 0 && row_offset + B <= capacity_rows, "egne_score_rows: rows [%lld, %lld) do not fit a ledger of %lld rows",
               (long long)row_offset, (long long)row_offset + B, (long long)capacity_rows);
  RowArgs a;
  a.cnt = (const unsigned*)counts;
  a.elOut = (const float*)elOut; a.elPred = (const float*)elPred; a.pc = (const float*)pupil_center; a.ic = (const float*)iris_center;
  a.elNorm = (const float*)elNorm; a.cond = (const float*)cond; a.loss = (const float*)loss_terms;
  a.B = B; a.ncls = ncls; a.ncond = ncond; a.H = H; a.W = W; a.batch_no = batch_no;
  a.rows = (double*)ledger + row_offset * EGNE_SCORE_FIELDS;
  rows_k<<<egne::cdiv(B, 64), 64, 0, (hipStream_t)stream>>>(a);
  return egne::check_launch("egne_score_rows");
}
