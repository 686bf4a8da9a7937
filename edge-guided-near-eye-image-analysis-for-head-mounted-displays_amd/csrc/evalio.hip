// Device-side frame preparation and overlay rendering of evaluate.py (--device_io 1): the stages between "uint8 video frame in
// HBM" and the network input, and between the fit result and the two uint8 BGR frames a video writer takes.  Both are pinned bit
// for bit against the host restatement in evaluate.py (preprocess_frame / resize_lanczos4, rescale_to_original,
// plot_segmap_ellpreds / _draw_ellipse, the edge frame of draw()); this file is compiled without FMA contraction (Makefile).
//
// egne_eval_prep:   [lanczos_k]  ->  sums_k  ->  normalise_k
//   lanczos_k    (resample_core.h, shared with csrc/loader.hip) one workgroup per output row of an eye: the 8-tap row pass of that row in float64 into LDS (sequential sum, as NumPy
//                reduces a middle axis), then the 8-tap column pass out of LDS (pairwise sum, as NumPy reduces a contiguous axis of 8),
//                rint + clip to uint8.  Tap indices and weights come from the host's tables (same bits as resize_lanczos4's).
//   sums_k       one workgroup per eye: S = sum(x), Q = sum(x*x) in 64-bit integers over the rows that survive the centre crop
//                (padding rows are zero and add nothing).  Integer sums are exact whatever the order.
//   normalise_k  mean = S / n, std = sqrt(n*Q - S*S) / n in float64, out = float((x - mean) / std); padding rows are (0 - mean) / std.
// egne_eval_render: render_k -> outline_k (iris) -> outline_k (pupil); three launches on one stream, so later writes win.
#include "common.h"
#include "resample_core.h"

namespace {

struct EyeView {          // where eye e's uint8 image lives: base + (e / eyes) * frame_stride + (e % eyes) * eye_stride, rows ld apart
  const uint8_t* base;
  long long frame_stride;
  int eyes, eye_stride, ld;
  __device__ __forceinline__ const uint8_t* at(int e) const { return base + (long long)(e / eyes) * frame_stride + (long long)(e % eyes) * eye_stride; }
};

// grid (Hr, E), 256 threads, dynamic LDS: We doubles
__global__ __launch_bounds__(256) void lanczos_k(EyeView src, int Hs, int We, int Hr, int Wr, const int* __restrict__ ridx,
                                                 const double* __restrict__ rw, const int* __restrict__ cidx,
                                                 const double* __restrict__ cw, uint8_t* __restrict__ out) {
  extern __shared__ double rowbuf[];
  const int y = blockIdx.x, e = blockIdx.y;
  const uint8_t* s = src.at(e);
  const int ld = src.ld;
  egne::lanczos4_row([=](int r, int x) { return s[(long long)r * ld + x]; }, Hs, We, Wr, y, ridx, rw, cidx, cw, rowbuf,
                     out + ((long long)e * Hr + y) * Wr);
}

// grid (E), 1024 threads: stats[e] = {S, Q} over rows [r0, r0 + nr) x W columns of eye e.  vec: every row start is 4-byte aligned.
__global__ __launch_bounds__(1024) void sums_k(EyeView img, int r0, int nr, int W, int vec, unsigned long long* __restrict__ stats) {
  __shared__ unsigned long long sh[2][16];
  const int e = blockIdx.x;
  const uint8_t* p = img.at(e) + (long long)r0 * img.ld;
  unsigned long long S = 0, Q = 0;
  if (vec) {
    const int W4 = W / 4, n4 = nr * W4;
    for (int i = threadIdx.x; i < n4; i += 1024) {
      const int y = i / W4, x = (i - y * W4) * 4;
      const unsigned v = *reinterpret_cast<const unsigned*>(p + (long long)y * img.ld + x);
      const unsigned a = v & 255u, b = (v >> 8) & 255u, c = (v >> 16) & 255u, d = v >> 24;
      S += a + b + c + d;
      Q += a * a + b * b + c * c + d * d;
    }
  } else {
    const int n = nr * W;
    for (int i = threadIdx.x; i < n; i += 1024) {
      const int y = i / W, x = i - y * W;
      const unsigned a = p[(long long)y * img.ld + x];
      S += a;
      Q += a * a;
    }
  }
  for (int d = 32; d >= 1; d >>= 1) { S += __shfl_down(S, d, 64); Q += __shfl_down(Q, d, 64); }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { sh[0][wave] = S; sh[1][wave] = Q; }
  __syncthreads();
  if (threadIdx.x == 0) {
    S = 0; Q = 0;
    for (int k = 0; k < 16; ++k) { S += sh[0][k]; Q += sh[1][k]; }
    stats[2 * e] = S;
    stats[2 * e + 1] = Q;
  }
}

// grid (ceil(Ho*Wo / PX / 256), E): PX pixels of one output row per thread (PX == 4 needs Wo % 4 == 0; vec as in sums_k).
// Output row y holds source row r0 + y - top when 0 <= y - top < nr, zeros otherwise.
template <int PX>
__global__ __launch_bounds__(256) void normalise_k(EyeView img, int r0, int top, int nr, int Ho, int Wo, int vec,
                                                   const unsigned long long* __restrict__ stats, float* __restrict__ out,
                                                   uint8_t* __restrict__ u8out) {
  const int e = blockIdx.y;
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * PX;
  const long long n = (long long)Ho * Wo;
  if (i >= n) return;
  const unsigned long long S = stats[2 * e], Q = stats[2 * e + 1];
  const double mean = (double)S / (double)n;
  const double sd = sqrt((double)((unsigned long long)n * Q - S * S)) / (double)n;
  const int y = (int)(i / Wo), x = (int)(i - (long long)y * Wo), ys = y - top;
  unsigned px[PX];
  for (int k = 0; k < PX; ++k) px[k] = 0;
  if (ys >= 0 && ys < nr) {
    const uint8_t* p = img.at(e) + (long long)(r0 + ys) * img.ld + x;
    if (PX == 4 && vec) {
      const unsigned v = *reinterpret_cast<const unsigned*>(p);
      for (int k = 0; k < PX; ++k) px[k] = (v >> (8 * k)) & 255u;
    } else {
      for (int k = 0; k < PX; ++k) px[k] = p[k];
    }
  }
  float r[PX];
  for (int k = 0; k < PX; ++k) r[k] = (float)(((double)px[k] - mean) / sd);
  float* o = out + (long long)e * n + i;
  if constexpr (PX == 4) {
    *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
    if (u8out) *reinterpret_cast<unsigned*>(u8out + (long long)e * n + i) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
  } else {
    for (int k = 0; k < PX; ++k) { o[k] = r[k]; if (u8out) u8out[(long long)e * n + i + k] = (uint8_t)px[k]; }
  }
}

struct RenderGeom {
  int N, Hs, Ws, eyes, We, Ho, Wo;
  int Hm;        // rows of a network map once the padding is removed / the cropped rows are put back as zeros: Ho - shift
  int off;       // network row = un-padded row + off
  double ry, rx; // nearest neighbour: source index = floor(dst * ratio), clamped
};

// grid (ceil(Hs*Ws / PX / 256), N): PX pixels of one frame row per thread (PX == 4 needs Ws % 4 == 0); both BGR frames
template <int PX>
__global__ __launch_bounds__(256) void render_k(RenderGeom g, const uint8_t* __restrict__ src, const long long* __restrict__ seg,
                                                const float* __restrict__ edge, uint8_t* __restrict__ overlay,
                                                uint8_t* __restrict__ edge_frame) {
  const int n = blockIdx.y;
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * PX;
  if (i >= (long long)g.Hs * g.Ws) return;
  const int y = (int)(i / g.Ws), x0 = (int)(i - (long long)y * g.Ws);
  const uint8_t* sp = src + ((long long)n * g.Hs + y) * g.Ws + x0;
  unsigned grey[PX];
  if constexpr (PX == 4) {
    const unsigned v = *reinterpret_cast<const unsigned*>(sp);
    for (int k = 0; k < PX; ++k) grey[k] = (v >> (8 * k)) & 255u;
  } else {
    for (int k = 0; k < PX; ++k) grey[k] = sp[k];
  }
  long long yi = (long long)((double)y * g.ry);
  if (yi > g.Hm - 1) yi = g.Hm - 1;
  const long long yn = yi + g.off;
  const bool row_ok = yn >= 0 && yn < g.Ho;
  uint8_t ov[3 * PX], ef[3 * PX];
  for (int k = 0; k < PX; ++k) {
    const int x = x0 + k, eye = x / g.We;
    unsigned b = grey[k], gr = grey[k], r = grey[k], ev = grey[k];
    if (eye < g.eyes) {
      long long cls = 0;
      float em = 0.0f;                     // rows put back by a negative shift: class 0, edge frame 0 (black)
      if (row_ok) {
        long long xi = (long long)((double)(x - eye * g.We) * g.rx);
        if (xi > g.Wo - 1) xi = g.Wo - 1;
        const long long at = (((long long)n * g.eyes + eye) * g.Ho + yn) * g.Wo + xi;
        cls = seg[at];
        const float m = 255.0f * edge[at];    // fp32, multiply and subtract rounded separately (NumPy: float * float32 array)
        em = 255.0f - m;
      }
      if (cls == 1) { b = 120; gr = 183; r = 53; }
      else if (cls == 2) { b = 36; gr = 231; r = 253; }
      em = em < 0.0f ? 0.0f : (em > 255.0f ? 255.0f : em);
      ev = (unsigned)(int)em;
    }
    ov[3 * k] = (uint8_t)b; ov[3 * k + 1] = (uint8_t)gr; ov[3 * k + 2] = (uint8_t)r;
    ef[3 * k] = ef[3 * k + 1] = ef[3 * k + 2] = (uint8_t)ev;
  }
  const long long o = (((long long)n * g.Hs + y) * g.Ws + x0) * 3;
  if constexpr (PX == 4) {
    unsigned wo[3], we[3];
    for (int k = 0; k < 3; ++k) {
      wo[k] = ov[4 * k] | (ov[4 * k + 1] << 8) | (ov[4 * k + 2] << 16) | ((unsigned)ov[4 * k + 3] << 24);
      we[k] = ef[4 * k] | (ef[4 * k + 1] << 8) | (ef[4 * k + 2] << 16) | ((unsigned)ef[4 * k + 3] << 24);
    }
    unsigned* po = reinterpret_cast<unsigned*>(overlay + o);
    unsigned* pe = reinterpret_cast<unsigned*>(edge_frame + o);
    for (int k = 0; k < 3; ++k) { po[k] = wo[k]; pe[k] = we[k]; }
  } else {
    for (int k = 0; k < 3 * PX; ++k) { overlay[o + k] = ov[k]; edge_frame[o + k] = ef[k]; }
  }
}

// grid (E), 256 threads: ellipse `which` (0 iris, 1 pupil) of eye e back to the source geometry -> ell_out[e][which], then its outline
// into the eye's crop of the overlay.  cs = cos(t) [720] then sin(t) [720], t = linspace(0, 2 pi, 720, endpoint=False) from the host.
__global__ __launch_bounds__(256) void outline_k(RenderGeom g, const double* __restrict__ fit, int which, int shift_floor, double inv_scale,
                                                 const double* __restrict__ cs, double* __restrict__ ell_out, uint8_t* __restrict__ overlay) {
  const int e = blockIdx.x;
  double el[5];
  for (int k = 0; k < 5; ++k) el[k] = fit[((long long)e * 2 + which) * 5 + k];
  el[1] = el[1] - (double)shift_floor;
  for (int k = 0; k < 4; ++k) el[k] = el[k] * inv_scale;
  if (threadIdx.x < 5) ell_out[((long long)e * 2 + which) * 5 + threadIdx.x] = el[threadIdx.x];
  bool all_m1 = true, finite = true;
  for (int k = 0; k < 5; ++k) { all_m1 = all_m1 && el[k] == -1.0; finite = finite && isfinite(el[k]); }
  if (all_m1 || !finite) return;
  const double cx = trunc(el[0]), cy = trunc(el[1]), a = trunc(el[2]), b = trunc(el[3]);
  const double ca = cos(el[4]), sa = sin(el[4]);
  const int n = e / g.eyes, eye = e % g.eyes;
  const uint8_t c0 = which == 0 ? 255 : 0, c2 = which == 0 ? 0 : 255;     // BGR: iris (255,0,0), pupil (0,0,255)
  for (int i = threadIdx.x; i < 720; i += 256) {
    const double ct = cs[i], st = cs[720 + i];
    const double x = cx + a * ct * ca - b * st * sa;
    const double y = cy + a * ct * sa + b * st * ca;
    const double xr = rint(x), yr = rint(y);
    if (xr >= 0.0 && xr < (double)g.We && yr >= 0.0 && yr < (double)g.Hs) {
      uint8_t* o = overlay + (((long long)n * g.Hs + (int)yr) * g.Ws + eye * g.We + (int)xr) * 3;
      o[0] = c0; o[1] = 0; o[2] = c2;
    }
  }
}

inline long long up16(long long v) { return (v + 15) / 16 * 16; }

}  // namespace

extern "C" int64_t egne_eval_prep_workspace_bytes(int N, int eyes, int Hr, int Wr, int resize) {
  if (N <= 0 || eyes <= 0 || Hr <= 0 || Wr <= 0) return 16;
  const long long E = (long long)N * eyes;
  return up16(E * 2 * (long long)sizeof(unsigned long long)) + (resize ? up16(E * Hr * Wr) : 0);
}

extern "C" int egne_eval_prep(const uint8_t* src, int N, int Hs, int Ws, int eyes, int We, int Hr, int Wr, const int32_t* row_idx,
                              const double* row_w, const int32_t* col_idx, const double* col_w, int Ho, int Wo, float* out,
                              uint8_t* u8_out, void* ws, void* stream) {
  EGNE_REQUIRE(src && out && ws && N > 0 && Hs > 0 && Ws > 0 && eyes > 0 && We > 0 && Hr > 0 && Wr > 0 && Ho > 0 && Wo > 0,
               "eval_prep: bad arguments (N %d source %dx%d eyes %d of %d columns, resized %dx%d, target %dx%d)", N, Hs, Ws, eyes, We, Hr, Wr, Ho, Wo);
  EGNE_REQUIRE((long long)eyes * We <= Ws, "eval_prep: %d eyes of %d columns do not fit a frame of %d columns", eyes, We, Ws);
  EGNE_REQUIRE(Wr == Wo, "eval_prep: the resized width %d must equal the target width %d", Wr, Wo);
  EGNE_REQUIRE(!row_idx == !row_w && !col_idx == !col_w, "eval_prep: a tap table needs both its indices and its weights");
  EGNE_REQUIRE((row_idx || Hr == Hs) && (col_idx || Wr == We), "eval_prep: resized shape %dx%d differs from the source's %dx%d without a tap table", Hr, Wr, Hs, We);
  EGNE_REQUIRE((long long)N * eyes <= 65535 && Hs < 32768 && Ws < 32768 && Hr < 32768 && (long long)Ho * Wo <= (1 << 23) && (long long)Hr * Wr <= (1 << 23),
               "eval_prep: shape out of range");
  hipStream_t st = (hipStream_t)stream;
  const int E = N * eyes;
  unsigned long long* stats = (unsigned long long*)ws;
  EyeView img{src, (long long)Hs * Ws, eyes, We, Ws};
  if (row_idx || col_idx) {
    const size_t lds = (size_t)We * sizeof(double);
    EGNE_REQUIRE(lds <= 64 * 1024, "eval_prep: eye too wide for LDS (%d columns)", We);
    uint8_t* resized = (uint8_t*)ws + up16((long long)E * 2 * sizeof(unsigned long long));
    hipLaunchKernelGGL(lanczos_k, dim3(Hr, E), dim3(256), lds, st, img, Hs, We, Hr, Wr, row_idx, row_w, col_idx, col_w, resized);
    img = EyeView{resized, (long long)Hr * Wr, 1, 0, Wr};
  }
  // rows: zero-pad pad // 2 above when short, centre-crop cut // 2 when tall
  const int top = Ho > Hr ? (Ho - Hr) / 2 : 0, r0 = Hr > Ho ? (Hr - Ho) / 2 : 0, nr = Hr < Ho ? Hr : Ho;
  const int vec = img.frame_stride % 4 == 0 && img.eye_stride % 4 == 0 && img.ld % 4 == 0 && Wo % 4 == 0 && ((uintptr_t)img.base & 3) == 0;
  hipLaunchKernelGGL(sums_k, dim3(E), dim3(1024), 0, st, img, r0, nr, Wo, vec, stats);
  const long long n = (long long)Ho * Wo;
  if (Wo % 4 == 0 && ((uintptr_t)out & 15) == 0 && (!u8_out || ((uintptr_t)u8_out & 3) == 0))
    hipLaunchKernelGGL(normalise_k<4>, dim3(egne::cdiv(n / 4, 256), E), dim3(256), 0, st, img, r0, top, nr, Ho, Wo, vec, stats, out, u8_out);
  else
    hipLaunchKernelGGL(normalise_k<1>, dim3(egne::cdiv(n, 256), E), dim3(256), 0, st, img, r0, top, nr, Ho, Wo, 0, stats, out, u8_out);
  return egne::check_launch("egne_eval_prep");
}

extern "C" int egne_eval_render(const uint8_t* src, int N, int Hs, int Ws, int eyes, int We, const int64_t* seg, const float* edge,
                                const double* fit, int Ho, int Wo, double inv_scale, int shift, const double* cos_sin,
                                uint8_t* overlay, uint8_t* edge_frame, double* ell_out, void* stream) {
  EGNE_REQUIRE(src && seg && edge && fit && cos_sin && overlay && edge_frame && ell_out && N > 0 && Hs > 0 && Ws > 0 && eyes > 0 && We > 0 &&
               Ho > 0 && Wo > 0, "eval_render: bad arguments (N %d source %dx%d eyes %d of %d columns, maps %dx%d)", N, Hs, Ws, eyes, We, Ho, Wo);
  EGNE_REQUIRE((long long)eyes * We <= Ws, "eval_render: %d eyes of %d columns do not fit a frame of %d columns", eyes, We, Ws);
  EGNE_REQUIRE(shift < Ho && (long long)Ho - shift < 32768 && (long long)N * eyes <= 65535 && N <= 65535 && Hs < 32768 && Ws < 32768 && Ho < 32768 && Wo < 32768,
               "eval_render: shape out of range (row shift %d on %d rows)", shift, Ho);
  hipStream_t st = (hipStream_t)stream;
  RenderGeom g;
  g.N = N; g.Hs = Hs; g.Ws = Ws; g.eyes = eyes; g.We = We; g.Ho = Ho; g.Wo = Wo;
  g.Hm = Ho - shift;
  g.off = shift > 0 ? shift / 2 : -((-shift) / 2);
  g.ry = (double)g.Hm / (double)Hs;
  g.rx = (double)Wo / (double)We;
  const long long px = (long long)Hs * Ws;
  if (Ws % 4 == 0 && (((uintptr_t)src | (uintptr_t)overlay | (uintptr_t)edge_frame) & 3) == 0)
    hipLaunchKernelGGL(render_k<4>, dim3(egne::cdiv(px / 4, 256), N), dim3(256), 0, st, g, src, (const long long*)seg, edge, overlay, edge_frame);
  else
    hipLaunchKernelGGL(render_k<1>, dim3(egne::cdiv(px, 256), N), dim3(256), 0, st, g, src, (const long long*)seg, edge, overlay, edge_frame);
  const int shift_floor = shift >= 0 ? shift / 2 : -((-shift + 1) / 2);     // Python's shift // 2
  for (int which = 0; which < 2; ++which)       // pupil over iris over the class colours
    hipLaunchKernelGGL(outline_k, dim3(N * eyes), dim3(256), 0, st, g, fit, which, shift_floor, inv_scale, cos_sin, ell_out, overlay);
  return egne::check_launch("egne_eval_render");
}
