// Ellipse scores of test.py against ground truth on the device (egne_amd.scores.EllipseLedger): the block the reference keeps behind
// bbox_iou_flag (test.py:108-155) -- the IoU of the rotated bounding boxes of two ellipses (calc_box_iou.py:13-54) and the absolute
// differences of their five parameters -- plus the IoU of the two ellipses themselves and of either against the class map, which the
// reference's search computes and drops (utils.py:405-406).
//
// egne_ellipse_pair_scores:  pair_scores_k   one workgroup of eight waves per (sample, region) -> 43 float64 of the sample's ledger row
// egne_ellipse_box_corners:  box_corners_k   the corners alone, one thread per ellipse         (tests, ellipses from elsewhere)
// egne_box_iou_counts:       box_counts_k    the box IoU alone, one workgroup per pair         (tests, boxes from elsewhere)
// all three run the same device functions (box_corners, box_pair_counts).
//
// The box fill is the closed quadrilateral of the truncated corners in exact integer arithmetic (include/egne_hip.h states the rule);
// the ellipse maps go through the membership rule and the evaluation of the search (fit_core.h).  Every count is an integer summed by
// wave shuffles and one LDS step: no atomics, the same bits on every run.  float64 expressions restate calc_bbox operation for operation
// (tests/ellipse_scores_refs.py); this file is compiled without FMA contraction (Makefile).
#include "common.h"

namespace {

#include "fit_core.h"

constexpr int kThreads = 512;                       // eight waves: a workgroup's time is the chain of its waves' loads of the class map
constexpr int kWaves = kThreads / 64;
constexpr int kRegion = EGNE_ELLSCORE_REGION_FIELDS;

// np.array(v, dtype=np.int32) of a float64: truncation toward zero; NaN and values outside int32 give INT_MIN (what the x86 conversion
// NumPy compiles to returns)
__device__ __forceinline__ int to_i32(double v) {
  return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : (int)0x80000000;
}

// calc_box_iou.py:8-12 in float64
__device__ __forceinline__ void roa(double x, double y, double a, double& xx, double& yy) {
  const double c = cos(a), s = sin(a);
  xx = c * x - s * y;
  yy = s * x + c * y;
}

// calc_box_iou.py:13-27 and the int32 conversion of :52-54: corners[8] = (x0, y0, ..., x3, y3)
__device__ void box_corners(const double* el, int* corners) {
  double xx, yy;
  roa(el[0], el[1], -el[4], xx, yy);
  const double px[4] = {xx - el[2], xx - el[2], xx + el[2], xx + el[2]};
  const double py[4] = {yy - el[3], yy + el[3], yy + el[3], yy - el[3]};
  for (int k = 0; k < 4; ++k) {
    double rx, ry;
    roa(px[k], py[k], el[4], rx, ry);
    corners[2 * k] = to_i32(rx);
    corners[2 * k + 1] = to_i32(ry);
  }
}

// A quadrilateral of integer corners as a closed pixel set.  T = long long while every coordinate stays below 2^29 in magnitude (edge
// cross products then stay below 2^62), __int128 for the boxes of absurd ellipses.
template <typename T>
struct Quad {
  T x[4], y[4];
  int sgn;                                  // orientation: sign of twice the signed area; 0 = no area
  __device__ void set(const int* c) {
    for (int k = 0; k < 4; ++k) { x[k] = (T)c[2 * k]; y[k] = (T)c[2 * k + 1]; }
    const T a2 = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0]) + (x[2] - x[0]) * (y[3] - y[0]) - (y[2] - y[0]) * (x[3] - x[0]);
    sgn = a2 > 0 ? 1 : (a2 < 0 ? -1 : 0);
  }
  __device__ bool has(int pxi, int pyi) const {
    const T px = (T)pxi, py = (T)pyi;
    bool all = true, seg = false;
    for (int k = 0; k < 4; ++k) {
      const int n = (k + 1) & 3;
      const T cr = (x[n] - x[k]) * (py - y[k]) - (y[n] - y[k]) * (px - x[k]);
      all = all && (sgn > 0 ? cr >= 0 : cr <= 0);
      const T xl = x[k] < x[n] ? x[k] : x[n], xh = x[k] < x[n] ? x[n] : x[k], yl = y[k] < y[n] ? y[k] : y[n], yh = y[k] < y[n] ? y[n] : y[k];
      seg = seg || (cr == 0 && px >= xl && px <= xh && py >= yl && py <= yh);
    }
    return sgn != 0 ? all : seg;            // no area: the pixels exactly on its four segments
  }
};

// the canvas rows and columns a box can touch: [x0, x1] x [y0, y1], empty when x1 < x0 or y1 < y0
struct Clip { int x0, x1, y0, y1; };
__device__ __forceinline__ Clip clip_of(const int* c, int H, int W) {
  int xl = c[0], xh = c[0], yl = c[1], yh = c[1];
  for (int k = 1; k < 4; ++k) { xl = min(xl, c[2 * k]); xh = max(xh, c[2 * k]); yl = min(yl, c[2 * k + 1]); yh = max(yh, c[2 * k + 1]); }
  Clip r = {max(xl, 0), min(xh, W - 1), max(yl, 0), min(yh, H - 1)};
  return r;
}

// sum of three counters over the workgroup (every thread calls it): wave shuffles, one LDS step.  sh: 3 * kWaves words.
__device__ __forceinline__ void wg_sum3(unsigned& a, unsigned& b, unsigned& c, unsigned* sh) {
  for (int o = 32; o >= 1; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); c += __shfl_xor(c, o); }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                          // (the words may still be read from the sum before)
  if (lane == 0) { sh[wave * 3] = a; sh[wave * 3 + 1] = b; sh[wave * 3 + 2] = c; }
  __syncthreads();
  a = b = c = 0;
  for (int w = 0; w < kWaves; ++w) { a += sh[w * 3]; b += sh[w * 3 + 1]; c += sh[w * 3 + 2]; }
}

template <typename T>
__device__ void box_pair_counts_t(const int* ca, const int* cb, int H, int W, unsigned& n_a, unsigned& n_b, unsigned& n_and) {
  Quad<T> A, B;
  A.set(ca); B.set(cb);
  const Clip ka = clip_of(ca, H, W), kb = clip_of(cb, H, W);
  n_a = n_b = n_and = 0;
  if (ka.x1 >= ka.x0 && ka.y1 >= ka.y0) {
    const int w = ka.x1 - ka.x0 + 1, n = w * (ka.y1 - ka.y0 + 1);            // (at most H * W < 2^31)
    for (int i = threadIdx.x; i < n; i += kThreads) {
      const int x = ka.x0 + i % w, y = ka.y0 + i / w;
      if (A.has(x, y)) { ++n_a; if (B.has(x, y)) ++n_and; }
    }
  }
  if (kb.x1 >= kb.x0 && kb.y1 >= kb.y0) {
    const int w = kb.x1 - kb.x0 + 1, n = w * (kb.y1 - kb.y0 + 1);
    for (int i = threadIdx.x; i < n; i += kThreads) {
      const int x = kb.x0 + i % w, y = kb.y0 + i / w;
      if (B.has(x, y)) ++n_b;
    }
  }
}

// Pixels of the H x W canvas in both boxes and in either (whole workgroup; the result is on every thread).
__device__ void box_pair_counts(const int* ca, const int* cb, int H, int W, unsigned* sh, unsigned& n_and, unsigned& n_or) {
  bool small = true;
  for (int k = 0; k < 8; ++k) small = small && ca[k] > -(1 << 29) && ca[k] < (1 << 29) && cb[k] > -(1 << 29) && cb[k] < (1 << 29);
  unsigned n_a, n_b;
  if (small) box_pair_counts_t<long long>(ca, cb, H, W, n_a, n_b, n_and);
  else box_pair_counts_t<__int128>(ca, cb, H, W, n_a, n_b, n_and);
  wg_sum3(n_a, n_b, n_and, sh);
  n_or = n_a + n_b - n_and;
}

// calc_box_iou.py:36: the quotient of the counts (the reference divides sums of 255s: the same double); 0 / 0 is NaN as in NumPy
__device__ __forceinline__ double box_iou_of(unsigned n_and, unsigned n_or) {
  return n_or ? (double)n_and / (double)n_or : __builtin_nan("");
}

struct PairArgs {
  const float* elNorm;       // [B,2,5]
  const double* pred;        // [B,2,5] pixel ellipses
  const long long* mask;     // [B,H,W]
  const float* cond;         // [B,ncond]
  const float *xs, *ys;
  int B, ncond, H, W, cls[2], batch_no;
  double* rows;
};

// grid 2 * B: workgroup e scores region e & 1 (0 iris, 1 pupil) of sample e >> 1.  LDS: xs[W], ys[H], 3 * kWaves sums, the class map's
// bits [H][wpr], the ground-truth ellipse's bits [H][wpr].
__global__ __launch_bounds__(kThreads) void pair_scores_k(PairArgs a) {
  extern __shared__ unsigned es_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x >> 1, r = blockIdx.x & 1, H = a.H, W = a.W;
  const int wpr = (W + 31) >> 5;
  float* lxs = (float*)es_lds;
  float* lys = lxs + W;
  unsigned* sums = es_lds + W + H;
  unsigned* mbits = sums + 3 * kWaves;
  unsigned* gbits = mbits + H * wpr;
  double* row = a.rows + (long long)i * EGNE_ELLSCORE_FIELDS;
  double* out = row + r * kRegion;
  const double nan = __builtin_nan("");
  if (r == 0 && threadIdx.x == 0) {
    row[EGNE_ELLSCORE_COND0] = a.cond[(long long)i * a.ncond] != 0.0f ? 1.0 : 0.0;
    row[EGNE_ELLSCORE_COND1] = a.cond[(long long)i * a.ncond + 1] != 0.0f ? 1.0 : 0.0;
    row[EGNE_ELLSCORE_BATCH] = (double)a.batch_no;
    row[EGNE_ELLSCORE_SAMPLE] = (double)i;
  }
  const int k = a.cls[r];
  if (k < 0) {                              // a region the model does not predict (the whole workgroup leaves)
    if (threadIdx.x < kRegion) out[threadIdx.x] = nan;
    return;
  }
  for (int j = threadIdx.x; j < W; j += kThreads) lxs[j] = a.xs[j];
  for (int j = threadIdx.x; j < H; j += kThreads) lys[j] = a.ys[j];

  // every thread forms the two pixel ellipses and the two boxes: the same operations on the same values
  double gn[5], gt[5], pd[5];
  for (int j = 0; j < 5; ++j) { gn[j] = (double)a.elNorm[((long long)i * 2 + r) * 5 + j]; pd[j] = a.pred[((long long)i * 2 + r) * 5 + j]; }
  norm_to_pixel(gn, H, W, gt);
  int cp[8], cg[8];
  box_corners(pd, cp);
  box_corners(gt, cg);
  unsigned n_and, n_or;
  box_pair_counts(cp, cg, H, W, sums, n_and, n_or);

  // what one evaluation of the search is handed: axes in pixels, the angle in the reference's degrees
  const double qp[3] = {pd[2], pd[3], pd[4] * 180. / PI_REF}, qg[3] = {gt[2], gt[3], gt[4] * 180. / PI_REF};
  __syncthreads();                          // lxs, lys
  unsigned n_seg = pack_mask_rows(a.mask + (long long)i * H * W, k, H, W, mbits, wpr, lane, wave, kWaves);
  const Ell Eg = ell_on_mesh(H, W, gt[0], gt[1], qg);
  unsigned n_gt = pack_ellipse_rows(Eg, H, W, lxs, lys, gbits, wpr, lane, wave, kWaves);
  // the packing counts by ballots and evaluate_ell leaves a wave's sum on all of its lanes: one lane per wave contributes
  unsigned zero = 0;
  if (lane != 0) n_seg = n_gt = 0;
  wg_sum3(n_seg, n_gt, zero, sums);         // (its barriers also order the packed words of all waves before the evaluations)
  unsigned mp_ne, mp_ni, mg_ne, mg_ni, ar_ne, ar_ni;
  evaluate_ell<kWaves>(H, W, lxs, lys, mbits, wpr, pd[0], pd[1], lane, wave, qp, mp_ne, mp_ni);
  evaluate_ell<kWaves>(H, W, lxs, lys, mbits, wpr, gt[0], gt[1], lane, wave, qg, mg_ne, mg_ni);
  evaluate_ell<kWaves>(H, W, lxs, lys, gbits, wpr, pd[0], pd[1], lane, wave, qp, ar_ne, ar_ni);
  unsigned s0 = lane == 0 ? mp_ne : 0, s1 = lane == 0 ? mp_ni : 0, s2 = lane == 0 ? mg_ne : 0;
  wg_sum3(s0, s1, s2, sums);
  unsigned s3 = lane == 0 ? mg_ni : 0, s4 = lane == 0 ? ar_ne : 0, s5 = lane == 0 ? ar_ni : 0;
  wg_sum3(s3, s4, s5, sums);
  if (threadIdx.x != 0) return;
  for (int j = 0; j < 5; ++j) {
    out[EGNE_ELLSCORE_ELL_PRED + j] = pd[j];
    out[EGNE_ELLSCORE_ELL_GT + j] = gt[j];
    out[EGNE_ELLSCORE_PARA + j] = fabs(pd[j] - gt[j]);
  }
  for (int j = 0; j < 8; ++j) {
    out[EGNE_ELLSCORE_CORNERS_PRED + j] = (double)cp[j];
    out[EGNE_ELLSCORE_CORNERS_GT + j] = (double)cg[j];
  }
  out[EGNE_ELLSCORE_BOX_IOU] = box_iou_of(n_and, n_or);
  out[EGNE_ELLSCORE_BOX_AND] = (double)n_and;
  out[EGNE_ELLSCORE_BOX_OR] = (double)n_or;
  out[EGNE_ELLSCORE_AREA] = (double)s4;               // pixels of the scored ellipse
  out[EGNE_ELLSCORE_AREA + 1] = (double)n_gt;         // of the ground-truth ellipse (its map, pixel by pixel)
  out[EGNE_ELLSCORE_AREA + 2] = (double)s5;           // of both
  out[EGNE_ELLSCORE_MAP_PRED] = (double)n_seg;
  out[EGNE_ELLSCORE_MAP_PRED + 1] = (double)s0;
  out[EGNE_ELLSCORE_MAP_PRED + 2] = (double)s1;
  out[EGNE_ELLSCORE_MAP_GT] = (double)n_seg;
  out[EGNE_ELLSCORE_MAP_GT + 1] = (double)s2;         // (the row intervals of the search: equal to AREA + 1)
  out[EGNE_ELLSCORE_MAP_GT + 2] = (double)s3;
}

__global__ __launch_bounds__(64) void box_corners_k(const double* __restrict__ ell, int n, int* __restrict__ corners) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= n) return;
  int c[8];
  box_corners(ell + (long long)e * 5, c);
  for (int j = 0; j < 8; ++j) corners[(long long)e * 8 + j] = c[j];
}

// out [n][3] = (IoU, n_and, n_or)
__global__ __launch_bounds__(kThreads) void box_counts_k(const int* __restrict__ ca, const int* __restrict__ cb, int H, int W, double* __restrict__ out) {
  __shared__ unsigned sums[3 * kWaves];
  const long long e = blockIdx.x;
  int a[8], b[8];
  for (int j = 0; j < 8; ++j) { a[j] = ca[e * 8 + j]; b[j] = cb[e * 8 + j]; }
  unsigned n_and, n_or;
  box_pair_counts(a, b, H, W, sums, n_and, n_or);
  if (threadIdx.x == 0) {
    out[e * 3] = box_iou_of(n_and, n_or);
    out[e * 3 + 1] = (double)n_and;
    out[e * 3 + 2] = (double)n_or;
  }
}

}  // namespace

extern "C" int egne_ellipse_pair_scores(const void* elNorm, const void* pred_px, const void* mask, const void* cond, int ncond, int B, int H, int W,
                                        int cls_iris, int cls_pupil, const void* xs, const void* ys, int batch_no, void* ledger,
                                        int64_t row_offset, int64_t capacity_rows, void* stream) {
  EGNE_REQUIRE(elNorm && pred_px && mask && cond && xs && ys && ledger, "egne_ellipse_pair_scores: null pointer");
  EGNE_REQUIRE(B > 0 && H > 1 && W > 1, "egne_ellipse_pair_scores: B must be positive, H and W at least 2 (got %d, %d, %d)", B, H, W);
  EGNE_REQUIRE(B <= (1 << 30), "egne_ellipse_pair_scores: at most 2^30 samples per call (got %d)", B);
  EGNE_REQUIRE(ncond >= 2, "egne_ellipse_pair_scores: cond needs two columns (got %d)", ncond);
  EGNE_REQUIRE(cls_iris >= 0 || cls_pupil >= 0, "egne_ellipse_pair_scores: no region to score (classes %d, %d)", cls_iris, cls_pupil);
  EGNE_REQUIRE((uintptr_t)mask % 8 == 0 && (uintptr_t)pred_px % 8 == 0 && (uintptr_t)ledger % 8 == 0 && (uintptr_t)elNorm % 4 == 0 &&
               (uintptr_t)cond % 4 == 0, "egne_ellipse_pair_scores: misaligned pointer");
  EGNE_REQUIRE(row_offset >= 0 && row_offset + B <= capacity_rows, "egne_ellipse_pair_scores: rows [%lld, %lld) do not fit a ledger of %lld rows",
               (long long)row_offset, (long long)row_offset + B, (long long)capacity_rows);
  // the limit of egne_ellipse_fit: two bit maps of the frame next to the mesh axes in the default 64 KB of dynamic LDS
  const size_t per_map = ((size_t)H * ((W + 31) / 32) + 32) * 4, fixed = (size_t)(W + H) * 4;
  EGNE_REQUIRE(2 * per_map + fixed <= 64 * 1024, "egne_ellipse_pair_scores: %dx%d maps do not fit LDS", H, W);
  PairArgs a;
  a.elNorm = (const float*)elNorm; a.pred = (const double*)pred_px; a.mask = (const long long*)mask; a.cond = (const float*)cond;
  a.xs = (const float*)xs; a.ys = (const float*)ys;
  a.B = B; a.ncond = ncond; a.H = H; a.W = W; a.cls[0] = cls_iris; a.cls[1] = cls_pupil; a.batch_no = batch_no;
  a.rows = (double*)ledger + row_offset * EGNE_ELLSCORE_FIELDS;
  const size_t lds = fixed + (3 * kWaves + 2 * (size_t)H * ((W + 31) / 32)) * 4;
  pair_scores_k<<<2 * (unsigned)B, kThreads, lds, (hipStream_t)stream>>>(a);
  return egne::check_launch("egne_ellipse_pair_scores");
}

extern "C" int egne_ellipse_box_corners(const void* ell_px, int n, void* corners, void* stream) {
  EGNE_REQUIRE(ell_px && corners, "egne_ellipse_box_corners: null pointer");
  EGNE_REQUIRE(n > 0, "egne_ellipse_box_corners: n must be positive (got %d)", n);
  box_corners_k<<<egne::cdiv(n, 64), 64, 0, (hipStream_t)stream>>>((const double*)ell_px, n, (int*)corners);
  return egne::check_launch("egne_ellipse_box_corners");
}

extern "C" int egne_box_iou_counts(const void* corners_a, const void* corners_b, int n, int H, int W, void* out, void* stream) {
  EGNE_REQUIRE(corners_a && corners_b && out, "egne_box_iou_counts: null pointer");
  EGNE_REQUIRE(n > 0 && H > 0 && W > 0, "egne_box_iou_counts: n, H, W must be positive (got %d, %d, %d)", n, H, W);
  EGNE_REQUIRE((long long)H * W < (1ll << 31), "egne_box_iou_counts: H * W must stay below 2^31 (the counters are 32-bit)");
  box_counts_k<<<(unsigned)n, kThreads, 0, (hipStream_t)stream>>>((const int*)corners_a, (const int*)corners_b, H, W, (double*)out);
  return egne::check_launch("egne_box_iou_counts");
}
