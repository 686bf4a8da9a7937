// Prediction overlay grid of train.py / test.py --disp 1 on the device (egne_amd.dispgrid.image_grid): the reference's
// generateImageGrid (utils.py:206-399) -- the first frames of a batch, histogram-equalised, the predicted classes painted in, the
// predicted ellipses drawn on top, tiled as torchvision.utils.make_grid tiles them.  include/egne_hip.h states the rules.
//
// egne_disp_grid:  zero_k     grid (chunks, 4): the workspace, the status words, and -- for the padding and the cells behind the last
//                                frame -- the grid and the uint8 image, by 16-byte stores.  A kernel of this file and not
//                                hipMemsetAsync: as memset nodes of a captured graph the fills were lost from the second replay on
//                                when the eager warm-up had run on another stream (seen on MI355X: the bins kept the last replay's
//                                counts and the padding held garbage); eager calls and kernel nodes were right every time
//                  -> minmax_k   grid (chunks, n): min / max of a frame chunk by 16-byte loads, wave shuffles, one LDS step, then integer
//                                atomic max on order-preserving keys (the minimum as the complement of its key)
//                  -> hist_k     grid (chunks, n): 256-bin histogram of u, one private LDS histogram per wave (integer LDS atomics),
//                                merged into int32 [n,256] by integer atomics; u is computed again, not stored
//                  -> paint_k    grid (chunks, n): every workgroup rebuilds the frame's 256-entry grey table in LDS (first occupied
//                                bin by ballot, running sum by a wave scan), then writes its pixels of the three planes and of the
//                                uint8 image
//                  -> outline_k  grid (n): the ground-truth outlines (on request), the iris outline, the pupil outline, separated by
//                                barriers so that the later paint wins
// Only integer atomics: the same bits on every run.  The arithmetic a host can run lives in dispgrid_core.h (tests/dispgrid_host.cpp);
// this file is compiled without FMA contraction (Makefile).
#include "common.h"
#include "dispgrid_core.h"

namespace {

#include "fit_core.h"

namespace dg = egne_dispgrid;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 4096;                      // pixels of a frame per workgroup of the two reduction passes
constexpr int kPaintChunk = 2048;                 // pixels per workgroup of the paint pass (the table is rebuilt once per workgroup)
constexpr int kWsWords = 258;                     // per frame: key of the maximum, complemented key of the minimum, 256 bins

struct Args {
  const float* img;          // [B,H,W]
  const long long* mask;     // [B,H,W]
  const float* el;           // [B,2,5]
  const float* el_gt;        // [B,2,5] or null
  const float* cond;         // [B,ncond] or null
  const double* cs;          // cos t [720], sin t [720]
  int ncond, H, W, n, override_, draw_gt, vec;
  dg::Layout lay;
  float* grid;               // [3,Hg,Wg]
  uint8_t* bgr;              // [Hg,Wg,3] or null
  int* status;               // [n]
  unsigned* ws;              // [n,kWsWords]
};

// pixels [p0, p1) of frame i, four per step where the frame allows 16-byte loads (a.vec): f(x) for every pixel
template <class F>
__device__ __forceinline__ void for_chunk(const Args& a, int i, F f) {
  const long long HW = (long long)a.H * a.W;
  const float* src = a.img + (long long)i * HW;
  const long long p0 = (long long)blockIdx.x * kChunk, p1 = p0 + kChunk < HW ? p0 + kChunk : HW;
  if (a.vec) {
    for (long long p = p0 + 4 * threadIdx.x; p < p1; p += 4 * kThreads) {      // (HW % 4 == 0 and kChunk % 4 == 0: whole vectors)
      const egne_f32x4 v = *(const egne_f32x4*)(src + p);
      f(v[0]); f(v[1]); f(v[2]); f(v[3]);
    }
  } else {
    for (long long p = p0 + threadIdx.x; p < p1; p += kThreads) f(src[p]);
  }
}

struct ZeroArgs { void* p[4]; unsigned long long n[4]; };

// range blockIdx.y: n bytes from p (null: nothing) -- bytes up to a 16-byte boundary, 16-byte vectors, the bytes behind them
__global__ __launch_bounds__(kThreads) void zero_k(ZeroArgs z) {
  unsigned char* p = (unsigned char*)z.p[blockIdx.y];
  const unsigned long long n = z.n[blockIdx.y];
  if (!p) return;
  unsigned long long head = (16 - (unsigned long long)(uintptr_t)p % 16) % 16;
  if (head > n) head = n;
  const unsigned long long nvec = (n - head) / 16, tid = (unsigned long long)blockIdx.x * kThreads + threadIdx.x,
                           stride = (unsigned long long)gridDim.x * kThreads;
  for (unsigned long long i = tid; i < head; i += stride) p[i] = 0;
  egne_u32x4* v = (egne_u32x4*)(p + head);
  for (unsigned long long i = tid; i < nvec; i += stride) v[i] = egne_u32x4{0u, 0u, 0u, 0u};
  for (unsigned long long i = head + nvec * 16 + tid; i < n; i += stride) p[i] = 0;
}

__global__ __launch_bounds__(kThreads) void minmax_k(Args a) {
  __shared__ unsigned sh[2 * kWaves];
  const int i = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned kmax = 0u, kmin = 0u;            // keys of finite values are never 0 or ~0: 0 = nothing seen
  bool bad = false;
  for_chunk(a, i, [&](float x) {
    if (dg::finite_f32(x)) {
      const unsigned k = dg::order_key(x);
      kmax = max(kmax, k);
      kmin = max(kmin, ~k);
    } else {
      bad = true;
    }
  });
  for (int o = 32; o >= 1; o >>= 1) {
    kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o));
    kmin = max(kmin, (unsigned)__shfl_xor((int)kmin, o));
  }
  const bool any_bad = __ballot(bad) != 0ull;
  if (lane == 0) { sh[wave] = kmax; sh[kWaves + wave] = kmin; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; ++w) { kmax = max(kmax, sh[w]); kmin = max(kmin, sh[kWaves + w]); }
    unsigned* ws = a.ws + (long long)i * kWsWords;
    atomicMax(ws, kmax);
    atomicMax(ws + 1, kmin);
  }
  if (lane == 0 && any_bad) atomicOr(a.status + i, (int)dg::ST_NONFINITE);
}

// minimum and span of frame i from the keys minmax_k left
__device__ __forceinline__ void frame_range(const Args& a, int i, float& mn, float& d) {
  const unsigned* ws = a.ws + (long long)i * kWsWords;
  const float mx = dg::key_value(ws[0]);
  mn = dg::key_value(~ws[1]);
  d = mx - mn;
}

__global__ __launch_bounds__(kThreads) void hist_k(Args a) {
  __shared__ unsigned h[kWaves][256];
  const int i = blockIdx.y, wave = threadIdx.x >> 6;
  for (int k = threadIdx.x; k < kWaves * 256; k += kThreads) (&h[0][0])[k] = 0u;
  float mn, d;
  frame_range(a, i, mn, d);
  __syncthreads();
  for_chunk(a, i, [&](float x) { atomicAdd(&h[wave][dg::to_u8(x, mn, d)], 1u); });
  __syncthreads();
  unsigned s = 0;
  for (int w = 0; w < kWaves; ++w) s += h[w][threadIdx.x];
  if (s) atomicAdd(a.ws + (long long)i * kWsWords + 2 + threadIdx.x, s);
}

__global__ __launch_bounds__(kThreads) void paint_k(Args a) {
  __shared__ float grey[256];
  __shared__ int wsum[kWaves], wfirst[kWaves], wmin[kWaves], wmax[kWaves];
  const int i = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = threadIdx.x;
  const int H = a.H, W = a.W;
  const long long HW = (long long)H * W;
  const int total = (int)HW;
  float mn, d;
  frame_range(a, i, mn, d);
  const bool constant = d == 0.0f;                   // mx == mn: grey 0, status bit 0
  // ---- the 256-entry table: thread k owns bin k -------------------------------------------------------------------------------------
  const int hk = (int)a.ws[(long long)i * kWsWords + 2 + k];
  int cum = hk;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(cum, o);
    if (lane >= o) cum += t;
  }
  const unsigned long long occ = __ballot(hk > 0);
  if (lane == 63) wsum[wave] = cum;
  if (lane == 0) wfirst[wave] = occ ? wave * 64 + __builtin_ctzll(occ) : 256;
  __syncthreads();
  int i0 = 256;
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) cum += wsum[w];
    i0 = min(i0, wfirst[w]);
  }
  int h0 = 0;
  if (i0 < 256) h0 = (int)a.ws[(long long)i * kWsWords + 2 + i0];
  const int e = i0 < 256 ? (int)dg::lut_of_bin(k, i0, h0, cum, total) : 0;
  int emin = hk > 0 ? e : 255, emax = hk > 0 ? e : 0;
  for (int o = 32; o >= 1; o >>= 1) {
    emin = min(emin, __shfl_xor(emin, o));
    emax = max(emax, __shfl_xor(emax, o));
  }
  if (lane == 0) { wmin[wave] = emin; wmax[wave] = emax; }
  __syncthreads();
  for (int w = 0; w < kWaves; ++w) { emin = min(emin, wmin[w]); emax = max(emax, wmax[w]); }
  if (i0 == 256) emin = emax = 0;
  grey[k] = constant ? 0.0f : dg::grey_of((uint8_t)e, (uint8_t)emin, (uint8_t)emax);
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0 && constant) atomicOr(a.status + i, (int)dg::ST_CONSTANT);
  // ---- the pixels ---------------------------------------------------------------------------------------------------------------------
  const bool painted = a.override_ || (a.cond && a.cond[(long long)i * a.ncond + 1] == 0.0f);
  int r0, c0;
  dg::grid_origin(i, a.n, a.lay, H, W, &r0, &c0);
  const long long plane = (long long)a.lay.Hg * a.lay.Wg;
  const float* src = a.img + (long long)i * HW;
  const long long* m = a.mask + (long long)i * HW;
  const long long p0 = (long long)blockIdx.x * kPaintChunk, p1 = p0 + kPaintChunk < HW ? p0 + kPaintChunk : HW;
  for (long long p = p0 + threadIdx.x; p < p1; p += kThreads) {
    const float v = grey[dg::to_u8(src[p], mn, d)];
    float c[3] = {v, v, v};
    if (painted) {
      const long long cls = m[p];
      if (cls == 1) { c[0] = 0.0f; c[1] = 255.0f; c[2] = 0.0f; }           // utils.py:281-284: green, then yellow
      else if (cls == 2) { c[0] = 255.0f; c[1] = 255.0f; c[2] = 0.0f; }
    }
    const int pi = (int)p;                  // (H * W <= 2^30)
    const long long o = (long long)(r0 + pi / W) * a.lay.Wg + c0 + pi % W;
    a.grid[o] = c[0]; a.grid[plane + o] = c[1]; a.grid[2 * plane + o] = c[2];
    if (a.bgr) { a.bgr[3 * o] = dg::u8_of_grid(c[2]); a.bgr[3 * o + 1] = dg::u8_of_grid(c[1]); a.bgr[3 * o + 2] = dg::u8_of_grid(c[0]); }
  }
}

// one outline of frame i (whole workgroup): the transform of egne_ellipse_init_from_pred, truncated centre and axes, 720 samples.
// Samples of one outline that share a pixel write the same value; outlines are separated by the caller's barriers.
__device__ void draw_outline(const Args& a, int i, const float* el5, float c0, float c1, float c2, int skip_bit) {
  double en[5], el[5];
  for (int k = 0; k < 5; ++k) en[k] = (double)el5[k];
  norm_to_pixel(en, a.H, a.W, el);
  if (!dg::ellipse_drawn(el)) {
    if (threadIdx.x == 0) atomicOr(a.status + i, skip_bit);
    return;
  }
  const double cx = trunc(el[0]), cy = trunc(el[1]), ax = trunc(el[2]), bx = trunc(el[3]);
  const double ca = cos(el[4]), sa = sin(el[4]);
  int r0, c0g;
  dg::grid_origin(i, a.n, a.lay, a.H, a.W, &r0, &c0g);
  const long long plane = (long long)a.lay.Hg * a.lay.Wg;
  for (int s = threadIdx.x; s < 720; s += kThreads) {
    int row, col;
    dg::outline_px(cx, cy, ax, bx, ca, sa, a.cs[s], a.cs[720 + s], a.H, a.W, &row, &col);
    const long long o = (long long)(r0 + row) * a.lay.Wg + c0g + col;
    a.grid[o] = c0; a.grid[plane + o] = c1; a.grid[2 * plane + o] = c2;
    if (a.bgr) { a.bgr[3 * o] = dg::u8_of_grid(c2); a.bgr[3 * o + 1] = dg::u8_of_grid(c1); a.bgr[3 * o + 2] = dg::u8_of_grid(c0); }
  }
}

__global__ __launch_bounds__(kThreads) void outline_k(Args a) {
  const int i = blockIdx.x;
  const bool painted = a.override_ || (a.cond && a.cond[(long long)i * a.ncond + 1] == 0.0f);
  if (!painted) return;                     // (uniform over the workgroup)
  if (a.draw_gt) {                          // the colour of the reference's commented-out lines, utils.py:331-332
    draw_outline(a, i, a.el_gt + ((long long)i * 2) * 5, 0.0f, 102.0f, 255.0f, dg::ST_SKIP_GT_IRIS);
    __syncthreads();
    draw_outline(a, i, a.el_gt + ((long long)i * 2 + 1) * 5, 0.0f, 102.0f, 255.0f, dg::ST_SKIP_GT_PUPIL);
    __syncthreads();
  }
  draw_outline(a, i, a.el + ((long long)i * 2) * 5, 0.0f, 0.0f, 255.0f, dg::ST_SKIP_IRIS);           // utils.py:349
  __syncthreads();
  draw_outline(a, i, a.el + ((long long)i * 2 + 1) * 5, 255.0f, 0.0f, 0.0f, dg::ST_SKIP_PUPIL);      // utils.py:350: painted last
}

}  // namespace

extern "C" int64_t egne_disp_grid_workspace_bytes(int frames) {
  return frames > 0 ? (int64_t)frames * kWsWords * 4 : 16;
}

extern "C" int egne_disp_grid(const void* img, const void* mask, const void* el, const void* el_gt, const void* cond, int ncond, int B, int H,
                              int W, int override_, int draw_gt, int count, int nrow, const void* cos_sin, void* grid, void* bgr_u8,
                              void* status, void* workspace, void* stream) {
  EGNE_REQUIRE(img && mask && el && cos_sin && grid && status && workspace, "egne_disp_grid: null pointer");
  EGNE_REQUIRE(!draw_gt || el_gt, "egne_disp_grid: draw_gt needs el_gt");
  EGNE_REQUIRE(B > 0 && count > 0 && nrow > 0, "egne_disp_grid: B, count and nrow must be positive (got %d, %d, %d)", B, count, nrow);
  EGNE_REQUIRE(H >= 6 && W >= 6, "egne_disp_grid: frames of at least 6 x 6 (the outline's clip to [6, size - 6]; got %d x %d)", H, W);
  EGNE_REQUIRE(!cond || ncond >= 2, "egne_disp_grid: cond needs two columns (got %d)", ncond);
  const int n = count < B ? count : B;
  EGNE_REQUIRE(n <= 65535, "egne_disp_grid: at most 65535 frames per grid (got %d)", n);
  EGNE_REQUIRE((long long)H * W <= (1ll << 30), "egne_disp_grid: H * W must stay within 2^30 (the bins are 32-bit)");
  const dg::Layout lay = dg::grid_layout(n, nrow, H, W);
  EGNE_REQUIRE((long long)lay.ym * (H + 2) + 2 < (1ll << 31) && (long long)lay.xm * (W + 2) + 2 < (1ll << 31), "egne_disp_grid: grid too large");
  EGNE_REQUIRE((uintptr_t)img % 4 == 0 && (uintptr_t)mask % 8 == 0 && (uintptr_t)el % 4 == 0 && (uintptr_t)el_gt % 4 == 0 &&
               (uintptr_t)cond % 4 == 0 && (uintptr_t)cos_sin % 8 == 0 && (uintptr_t)grid % 4 == 0 && (uintptr_t)status % 4 == 0 &&
               (uintptr_t)workspace % 4 == 0, "egne_disp_grid: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  Args a;
  a.img = (const float*)img; a.mask = (const long long*)mask; a.el = (const float*)el; a.el_gt = (const float*)el_gt;
  a.cond = (const float*)cond; a.cs = (const double*)cos_sin;
  a.ncond = ncond; a.H = H; a.W = W; a.n = n; a.override_ = override_ != 0; a.draw_gt = draw_gt != 0;
  a.vec = ((long long)H * W) % 4 == 0 && (uintptr_t)img % 16 == 0;
  a.lay = lay;
  a.grid = (float*)grid; a.bgr = (uint8_t*)bgr_u8; a.status = (int*)status; a.ws = (unsigned*)workspace;
  const long long HW = (long long)H * W, cells = (long long)lay.Hg * lay.Wg;
  ZeroArgs z = {{workspace, status, nullptr, nullptr}, {(unsigned long long)n * kWsWords * 4, (unsigned long long)n * 4, 0ull, 0ull}};
  if (n > 1) {                              // the padding and the cells behind the last frame; one frame covers its grid
    z.p[2] = grid; z.n[2] = (unsigned long long)cells * 3 * 4;
    z.p[3] = bgr_u8; z.n[3] = (unsigned long long)cells * 3;
  }
  const unsigned long long most = z.n[2] > z.n[0] ? z.n[2] : z.n[0];
  const int zb = egne::cdiv((long long)most, 16ll * kThreads);
  zero_k<<<dim3(zb < 1024 ? zb : 1024, 4), kThreads, 0, st>>>(z);
  const dim3 red(egne::cdiv(HW, kChunk), n), pnt(egne::cdiv(HW, kPaintChunk), n);
  minmax_k<<<red, kThreads, 0, st>>>(a);
  hist_k<<<red, kThreads, 0, st>>>(a);
  paint_k<<<pnt, kThreads, 0, st>>>(a);
  outline_k<<<n, kThreads, 0, st>>>(a);
  return egne::check_launch("egne_disp_grid");
}
