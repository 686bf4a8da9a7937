// Device-side training loader (egne_amd.loader.device_batch): the first and the last stage of the reference's Dataset item path
// (CurriculumLib.py:94-166) around the augmentation, for a whole batch of raw frames that already sits in HBM.
//
// egne_loader_stage   pad2Size (helperfunctions.py:406-428: every frame centred in the canvas, constant zeros) and, with tap tables,
//                     scaleFn (CurriculumLib.py:78-89) of the padded canvas: the image through the 8-tap Lanczos resampling of
//                     evaluate.resize_lanczos4 (resample_core.h, the code egne_eval_prep runs), the label through resize_nearest.
//                     uint8 image and int8 label in, uint8 image and int64 label out: what egne_augment takes.
// egne_loader_finish  after the augmentation: the label remap of CurriculumLib.py:123-125 (1 -> 0, 2 -> 1, 3 -> 2) and the z-score of
//                     :139 with the statistics of egne_zscore (zscore_core.h), bit-identical to it on the float of the same pixels.
//
// Both are memory-bound passes: 8 pixels per lane where rows allow it (8-byte image accesses, 16-byte label stores).  The raw frames
// are never read outside [0, src rows) x [0, src columns) clamped to the buffer, whatever src_hw holds; the host refuses frames that
// do not fit the canvas before the launch.  This file is compiled without FMA contraction (Makefile), as csrc/evalio.hip is.
#include "common.h"
#include "resample_core.h"
#include "zscore_core.h"

namespace {

struct RawFrames {        // B raw frames zero-padded into [B][Rmax][Cmax]; frame b holds src_hw[b] = (rows, columns) valid pixels
  const uint8_t* img;
  const int8_t* lab;
  const int* src_hw;
  int Rmax, Cmax, H, W;   // H x W: the canvas pad2Size centres a frame in
};

struct Placed {           // frame b inside the canvas: canvas (y, x) = source (y - up_r, x - up_c) when that is inside r x c, else 0
  const uint8_t* img;
  const int8_t* lab;
  int r, c, up_r, up_c, ld;
  __device__ __forceinline__ bool inside(int y, int x) const {
    const int sy = y - up_r, sx = x - up_c;
    return sy >= 0 && sy < r && sx >= 0 && sx < c;
  }
  __device__ __forceinline__ long long at(int y, int x) const { return (long long)(y - up_r) * ld + (x - up_c); }
  __device__ __forceinline__ uint8_t pixel(int y, int x) const { return inside(y, x) ? img[at(y, x)] : (uint8_t)0; }
  __device__ __forceinline__ long long label(int y, int x) const { return inside(y, x) ? (long long)lab[at(y, x)] : 0ll; }
};

__device__ __forceinline__ Placed place(const RawFrames& f, int b) {
  Placed p;
  const long long off = (long long)b * f.Rmax * f.Cmax;
  p.img = f.img + off;
  p.lab = f.lab + off;
  p.r = egne::clampi(f.src_hw[2 * b], 0, f.Rmax);
  p.c = egne::clampi(f.src_hw[2 * b + 1], 0, f.Cmax);
  p.up_r = (f.H - p.r) / 2;
  p.up_c = (f.W - p.c) / 2;
  p.ld = f.Cmax;
  return p;
}

typedef long long ll2 __attribute__((ext_vector_type(2)));

// canvas pixels (y, x0 .. x0 + 7) of frame b
__device__ __forceinline__ void pad_chunk(const RawFrames& f, const Placed& p, int b, int y, int x0, int vec, uint8_t* __restrict__ oimg,
                                          long long* __restrict__ olab) {
  uint8_t px[8];
  long long lb[8];
  const int sy = y - p.up_r, sx0 = x0 - p.up_c;
  if (sy >= 0 && sy < p.r && sx0 >= 0 && sx0 + 8 <= p.c) {          // all 8 inside the source: one 8-byte load each when aligned
    const uint8_t* ip = p.img + (long long)sy * p.ld + sx0;
    const int8_t* lp = p.lab + (long long)sy * p.ld + sx0;
    if ((((uintptr_t)ip | (uintptr_t)lp) & 7) == 0) {
      const unsigned long long vi = *reinterpret_cast<const unsigned long long*>(ip);
      const unsigned long long vl = *reinterpret_cast<const unsigned long long*>(lp);
#pragma unroll
      for (int k = 0; k < 8; ++k) { px[k] = (uint8_t)(vi >> (8 * k)); lb[k] = (long long)(int8_t)(vl >> (8 * k)); }
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) { px[k] = ip[k]; lb[k] = (long long)lp[k]; }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) { px[k] = p.pixel(y, x0 + k); lb[k] = p.label(y, x0 + k); }
  }
  const long long o = ((long long)b * f.H + y) * f.W + x0;
  if (vec) {
    unsigned long long v = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) v |= (unsigned long long)px[k] << (8 * k);
    *reinterpret_cast<unsigned long long*>(oimg + o) = v;
#pragma unroll
    for (int k = 0; k < 8; k += 2) *reinterpret_cast<ll2*>(olab + o + k) = ll2{lb[k], lb[k + 1]};
  } else {
    for (int k = 0; k < 8 && x0 + k < f.W; ++k) { oimg[o + k] = px[k]; olab[o + k] = lb[k]; }
  }
}

// grid (X, B), X * B capped near 2048 workgroups: 8 pixels of one canvas row per thread and round of the grid-stride loop.
// vec: W % 8 == 0 and both outputs 16-byte aligned.
__global__ __launch_bounds__(256) void loader_pad_k(RawFrames f, int vec, uint8_t* __restrict__ oimg, long long* __restrict__ olab) {
  const int b = blockIdx.y, per_row = (f.W + 7) / 8;
  const Placed p = place(f, b);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < f.H * per_row; i += gridDim.x * 256)
    pad_chunk(f, p, b, i / per_row, (i % per_row) * 8, vec, oimg, olab);
}

// grid (Hs, B), 256 threads, dynamic LDS: W doubles.  Output row y of frame b: the image as lanczos4_row of the canvas, the label at
// canvas (nrow[y], ncol[x]) (evaluate.resize_nearest's indices, from the host).
__global__ __launch_bounds__(256) void loader_scale_k(RawFrames f, int Hs, int Ws, const int* __restrict__ ridx,
                                                      const double* __restrict__ rw, const int* __restrict__ cidx,
                                                      const double* __restrict__ cw, const int* __restrict__ nrow,
                                                      const int* __restrict__ ncol, uint8_t* __restrict__ oimg,
                                                      long long* __restrict__ olab) {
  extern __shared__ double rowbuf[];
  const int y = blockIdx.x, b = blockIdx.y;
  const Placed p = place(f, b);
  const long long o = ((long long)b * Hs + y) * Ws;
  egne::lanczos4_row([=](int r, int x) { return p.pixel(r, x); }, f.H, f.W, Ws, y, ridx, rw, cidx, cw, rowbuf, oimg + o);
  const int cy = egne::clampi(nrow[y], 0, f.H - 1);
  for (int x = threadIdx.x; x < Ws; x += 256) olab[o + x] = p.label(cy, egne::clampi(ncol[x], 0, f.W - 1));
}

__device__ __forceinline__ long long remap(long long v) { return (v >= 1 && v <= 3) ? v - 1 : v; }

// grid (1 + R, B), 256 threads.  Block 0 of a frame: the z-score (one workgroup per image, as zscore_k: the order of its sums is
// part of the result).  Blocks 1..R: the label remap, two labels per 16-byte access when vec (n even, 16-byte aligned labels).
// vec4: n % 4 == 0, image 4-byte and output 16-byte aligned.
__global__ __launch_bounds__(256) void loader_finish_k(const uint8_t* __restrict__ img, const long long* __restrict__ lab, int n, int vec,
                                                       int vec4, float* __restrict__ out, long long* __restrict__ olab) {
  __shared__ double sh[256];
  const int b = blockIdx.y;
  if (blockIdx.x == 0) {
    const uint8_t* xi = img + (long long)b * n;
    float* yi = out + (long long)b * n;
    double mean, sd;
    egne::zscore_stats([=](int i) { return (float)xi[i]; }, n, sh, mean, sd);
    if (vec4) {
      for (int i = threadIdx.x * 4; i < n; i += 1024) {
        const unsigned v = *reinterpret_cast<const unsigned*>(xi + i);
        float r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = (float)(((float)((v >> (8 * k)) & 255u) - mean) / sd);
        *reinterpret_cast<float4*>(yi + i) = make_float4(r[0], r[1], r[2], r[3]);
      }
    } else {
      for (int i = threadIdx.x; i < n; i += 256) yi[i] = (float)(((float)xi[i] - mean) / sd);
    }
    return;
  }
  const long long* l = lab + (long long)b * n;
  long long* o = olab + (long long)b * n;
  const int t = (blockIdx.x - 1) * 256 + threadIdx.x, stride = (gridDim.x - 1) * 256;
  if (vec) {
    for (int i = t; i < n / 2; i += stride) {
      const ll2 v = *reinterpret_cast<const ll2*>(l + 2 * i);
      *reinterpret_cast<ll2*>(o + 2 * i) = ll2{remap(v[0]), remap(v[1])};
    }
  } else {
    for (int i = t; i < n; i += stride) o[i] = remap(l[i]);
  }
}

}  // namespace

extern "C" int egne_loader_stage(const uint8_t* img, const int8_t* label, const int32_t* src_hw, int B, int Rmax, int Cmax, int H, int W,
                                 int Hs, int Ws, const int32_t* row_idx, const double* row_w, const int32_t* col_idx,
                                 const double* col_w, const int32_t* near_row, const int32_t* near_col, uint8_t* out_img,
                                 int64_t* out_label, void* stream) {
  EGNE_REQUIRE(img && label && src_hw && out_img && out_label && B > 0 && B <= 65535 && Rmax > 0 && Cmax > 0 && H > 0 && W > 0 && Hs > 0 && Ws > 0,
               "loader_stage: bad arguments (B %d raw %dx%d canvas %dx%d out %dx%d)", B, Rmax, Cmax, H, W, Hs, Ws);
  EGNE_REQUIRE(H < 32768 && W < 32768 && Hs < 32768 && Ws < 32768 && Rmax < 32768 && Cmax < 32768, "loader_stage: shape out of range");
  EGNE_REQUIRE(!row_idx == !row_w && !col_idx == !col_w, "loader_stage: a tap table needs both its indices and its weights");
  EGNE_REQUIRE((row_idx || Hs == H) && (col_idx || Ws == W), "loader_stage: output %dx%d differs from the canvas %dx%d without a tap table", Hs, Ws, H, W);
  const bool scaled = row_idx || col_idx || near_row || near_col;
  EGNE_REQUIRE(!scaled || (near_row && near_col), "loader_stage: scaling needs the nearest-neighbour index tables of the label");
  hipStream_t st = (hipStream_t)stream;
  RawFrames f{img, label, src_hw, Rmax, Cmax, H, W};
  if (scaled) {
    const size_t lds = (size_t)W * sizeof(double);
    EGNE_REQUIRE(lds <= 64 * 1024, "loader_stage: canvas too wide for LDS (%d columns)", W);
    hipLaunchKernelGGL(loader_scale_k, dim3(Hs, B), dim3(256), lds, st, f, Hs, Ws, row_idx, row_w, col_idx, col_w, near_row, near_col,
                       out_img, (long long*)out_label);
  } else {
    const int vec = W % 8 == 0 && (((uintptr_t)out_img | (uintptr_t)out_label) & 15) == 0;
    const int want = egne::cdiv((long long)H * ((W + 7) / 8), 256), cap = 2048 / B < 1 ? 1 : 2048 / B;
    hipLaunchKernelGGL(loader_pad_k, dim3(want < cap ? want : cap, B), dim3(256), 0, st, f, vec, out_img, (long long*)out_label);
  }
  return egne::check_launch("egne_loader_stage");
}

extern "C" int egne_loader_finish(const uint8_t* img, const int64_t* label, float* out_img, int64_t* out_label, int B, int n, void* stream) {
  EGNE_REQUIRE(img && label && out_img && out_label && B > 0 && B <= 65535 && n > 1, "loader_finish: bad arguments (B %d, %d pixels)", B, n);
  const int vec = n % 2 == 0 && (((uintptr_t)label | (uintptr_t)out_label) & 15) == 0;
  const int vec4 = n % 4 == 0 && ((uintptr_t)img & 3) == 0 && ((uintptr_t)out_img & 15) == 0;
  const int want = egne::cdiv(vec ? n / 2 : n, 256), cap = 2048 / B < 1 ? 1 : 2048 / B;      // remap workgroups per frame, grid-stride
  const int R = want < cap ? want : cap;
  hipLaunchKernelGGL(loader_finish_k, dim3(1 + R, B), dim3(256), 0, (hipStream_t)stream, img, (const long long*)label, n, vec, vec4, out_img,
                     (long long*)out_label);
  return egne::check_launch("egne_loader_finish");
}
