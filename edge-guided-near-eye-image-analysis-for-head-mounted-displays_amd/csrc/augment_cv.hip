// The OpenCV branches of data_augment.augment (data_augment.py:38-42 blur, :67-79 glint lines, :99-120 rotation) over a batch,
// second launch of egne_amd.data_augment.augment_batch(on_cv2="device") behind egne_augment (dataprep.hip), which has already
// copied image and label of these frames to the outputs.
// PIXEL PARITY WITH OPENCV UNPINNED (no OpenCV in the build container): the kernels are byte-identical to the NumPy restatement of
// OpenCV's documented behaviour in tests/augment_cv2_refs.py; the draws, the arguments handed to OpenCV and the geometry ARE pinned
// by the reference itself (tests/golden/augment_cv2.npz).  Built with -ffp-contract=off: the restatement rounds every float64
// operation on its own.
//   1 blur      separable 7 taps, BORDER_REFLECT_101, 8-bit fixed-point taps q (sum 256): r = sum q*src (16 bit), s = sum q*r,
//               out = (s + 32768) >> 16.  Tile + 3-pixel reflected halo as bytes in LDS, row pass into a 16-bit LDS plane.
//   5 lines     pixel = 255 iff its squared distance to one of the frame's <= 9 segments is <= 4.0 (capsule of radius 2), float64.
//   6 rotation  source position (X, Y) = inverse matrix * (x, y); image: quantised to 1/32 pixel, 8x8 Lanczos taps from a [32][8]
//               float64 phase table, taps outside the frame read 0 (BORDER_CONSTANT), rows summed left to right, then the column,
//               clip(rint(v)); label: nearest, src[floor(Y+.5)][floor(X+.5)] or 0.  The source bounding box of the output tile is
//               staged in LDS (a 32x32 tile at any angle touches at most 54 rows / columns); a tap outside the staged box (only a
//               matrix that is no rotation gets there) is read from memory.
#include "common.h"

namespace {

constexpr int CT = 32;                    // output tile (CT x CT pixels, 256 threads)
constexpr int BHALO = 3, BSRC = CT + 2 * BHALO, BSTRIDE = BSRC + 2;
constexpr int RBOX = 56;                  // staged source box of the rotation
constexpr int MAXLINES = 9;

__device__ __forceinline__ int reflect101(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return i < 0 ? 0 : (i >= n ? n - 1 : i);          // (beyond one reflection: only halo positions nothing reads)
}

__device__ __forceinline__ void blur_tile(const unsigned char* __restrict__ img, const int* __restrict__ q8, int sigma,
                                          unsigned char* __restrict__ oimg, int H, int W, int y0, int x0, unsigned char* sb,
                                          unsigned short* rowp) {
  const int tid = threadIdx.x;
  for (int i = tid; i < BSRC * BSRC; i += 256) {
    const int r = i / BSRC, c = i - r * BSRC;
    const int gy = reflect101(y0 + r - BHALO, H), gx = reflect101(x0 + c - BHALO, W);
    sb[r * BSTRIDE + c] = img[(long long)gy * W + gx];
  }
  int q[7];
  sigma = sigma < 2 ? 2 : (sigma > 6 ? 6 : sigma);
#pragma unroll
  for (int k = 0; k < 7; ++k) q[k] = q8[(sigma - 2) * 7 + k];
  __syncthreads();
  for (int i = tid; i < BSRC * CT; i += 256) {
    const int r = i / CT, c = i - r * CT;
    int s = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) s += q[k] * (int)sb[r * BSTRIDE + c + k];
    rowp[i] = (unsigned short)s;                      // <= 256 * 255
  }
  __syncthreads();
  for (int i = tid; i < CT * CT; i += 256) {
    const int r = i / CT, c = i - r * CT, y = y0 + r, x = x0 + c;
    if (y >= H || x >= W) continue;
    int s = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) s += q[k] * (int)rowp[(r + k) * CT + c];
    oimg[(long long)y * W + x] = (unsigned char)((s + 32768) >> 16);
  }
}

__device__ __forceinline__ double clamp_pos(double v) {       // keeps the conversion to int defined; anything this far is outside
  if (!(v > -1.0e9)) v = -1.0e9;
  return v > 1.0e9 ? 1.0e9 : v;
}

__device__ __forceinline__ void rotate_tile(const unsigned char* __restrict__ img, const long long* __restrict__ label,
                                            const double* __restrict__ m, const double* __restrict__ phase,
                                            unsigned char* __restrict__ oimg, long long* __restrict__ olabel, int H, int W, int y0,
                                            int x0, unsigned char* sb, double* ph) {
  const int tid = threadIdx.x;
  ph[tid] = phase[tid];                               // [32][8]
  const double i00 = m[0], i01 = m[1], i02 = m[2], i10 = m[3], i11 = m[4], i12 = m[5];
  const int x1 = min(x0 + CT - 1, W - 1), y1 = min(y0 + CT - 1, H - 1);
  double mnx = 1.0e9, mny = 1.0e9;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double x = (k & 1) ? x1 : x0, y = (k & 2) ? y1 : y0;
    const double X = ((i00 * x) + (i01 * y)) + i02, Y = ((i10 * x) + (i11 * y)) + i12;
    mnx = fmin(mnx, clamp_pos(X));
    mny = fmin(mny, clamp_pos(Y));
  }
  const int bx0 = (int)floor(mnx) - 4, by0 = (int)floor(mny) - 4;
  for (int i = tid; i < RBOX * RBOX; i += 256) {
    const int r = i / RBOX, c = i - r * RBOX, sy = by0 + r, sx = bx0 + c;
    const bool in = sy >= 0 && sy < H && sx >= 0 && sx < W;
    sb[i] = in ? img[(long long)sy * W + sx] : (unsigned char)0;
  }
  __syncthreads();
  for (int p = tid; p < CT * CT; p += 256) {
    const int r = p / CT, c = p - r * CT, y = y0 + r, x = x0 + c;
    if (y >= H || x >= W) continue;
    const double X = ((i00 * (double)x) + (i01 * (double)y)) + i02, Y = ((i10 * (double)x) + (i11 * (double)y)) + i12;
    const int ix = (int)clamp_pos(floor(32.0 * X + 0.5)), iy = (int)clamp_pos(floor(32.0 * Y + 0.5));
    const int sx0 = (ix >> 5) - 3, sy0 = (iy >> 5) - 3;
    const double* wx = ph + (ix & 31) * 8;
    const double* wy = ph + (iy & 31) * 8;
    const int lx = sx0 - bx0, ly = sy0 - by0;
    const bool staged = lx >= 0 && ly >= 0 && lx + 8 <= RBOX && ly + 8 <= RBOX;
    double v = 0.0;
    for (int ky = 0; ky < 8; ++ky) {
      double t = 0.0;
      if (staged) {
        const unsigned char* s = sb + (ly + ky) * RBOX + lx;
#pragma unroll
        for (int kx = 0; kx < 8; ++kx) t = t + wx[kx] * (double)s[kx];
      } else {
        const int sy = sy0 + ky;
        for (int kx = 0; kx < 8; ++kx) {
          const int sx = sx0 + kx;
          const bool in = sy >= 0 && sy < H && sx >= 0 && sx < W;
          const double s = in ? (double)img[(long long)sy * W + sx] : 0.0;
          t = t + wx[kx] * s;
        }
      }
      v = v + wy[ky] * t;
    }
    v = rint(v);
    v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
    oimg[(long long)y * W + x] = (unsigned char)(int)v;
    const int nx = (int)clamp_pos(floor(X + 0.5)), ny = (int)clamp_pos(floor(Y + 0.5));
    const bool in = ny >= 0 && ny < H && nx >= 0 && nx < W;
    olabel[(long long)y * W + x] = in ? label[(long long)ny * W + nx] : 0ll;
  }
}

// as augment_k: one thread per 8 pixels of a row, the frame's workgroups stride over it
__device__ __forceinline__ void lines_frame(const double* __restrict__ segs, int n, unsigned char* __restrict__ oimg, int H, int W,
                                            double* sg) {
  n = n < 0 ? 0 : (n > MAXLINES ? MAXLINES : n);
  if ((int)threadIdx.x < 4 * MAXLINES) sg[threadIdx.x] = segs[threadIdx.x];
  __syncthreads();
  const int per_row = (W + 7) / 8;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < H * per_row; i += gridDim.x * blockDim.x) {
    const int y = i / per_row, x0 = (i - y * per_row) * 8;
    for (int k = 0; k < 8 && x0 + k < W; ++k) {
      const int x = x0 + k;
      bool hit = false;
      for (int j = 0; j < n; ++j) {
        const double ax = sg[4 * j], ay = sg[4 * j + 1];
        const double dx = sg[4 * j + 2] - ax, dy = sg[4 * j + 3] - ay;
        const double dxx = dx * dx, dyy = dy * dy;
        const double len2 = dxx + dyy;
        const double px = (double)x - ax, py = (double)y - ay;
        const double pdx = px * dx, pdy = py * dy;
        const double dot = pdx + pdy;
        double t = 0.0;
        if (len2 != 0.0) t = dot / len2;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
        const double cx = t * dx, cy = t * dy;
        const double ex = px - cx, ey = py - cy;
        const double exx = ex * ex, eyy = ey * ey;
        const double d2 = exx + eyy;
        hit = hit || d2 <= 4.0;
      }
      if (hit) oimg[(long long)y * W + x] = 255;
    }
  }
}

// grid (tiles, B): frame[b] = {choice, sigma, kept lines}; the choice is uniform within a workgroup
__global__ __launch_bounds__(256) void augment_cv_k(const unsigned char* __restrict__ img, const long long* __restrict__ label,
                                                     const int* __restrict__ frame, const double* __restrict__ segs,
                                                     const double* __restrict__ rot, const int* __restrict__ q8,
                                                     const double* __restrict__ phase, unsigned char* __restrict__ oimg,
                                                     long long* __restrict__ olabel, int H, int W, int tiles_x) {
  __shared__ __attribute__((aligned(16))) unsigned char sb[RBOX * RBOX];          // >= BSRC * BSTRIDE
  __shared__ __attribute__((aligned(16))) double tab[320];                        // phase table / 16-bit row plane / segments
  static_assert(RBOX * RBOX >= BSRC * BSTRIDE && sizeof(double) * 320 >= sizeof(unsigned short) * BSRC * CT &&
                256 >= 4 * MAXLINES, "LDS planes");
  const int b = blockIdx.y, ch = frame[3 * b];
  if (ch != 1 && ch != 5 && ch != 6) return;
  const long long fb = (long long)b * H * W;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  if (ch == 1) blur_tile(img + fb, q8, frame[3 * b + 1], oimg + fb, H, W, ty * CT, tx * CT, sb, (unsigned short*)tab);
  else if (ch == 6) rotate_tile(img + fb, label + fb, rot + 6 * b, phase, oimg + fb, olabel + fb, H, W, ty * CT, tx * CT, sb, tab);
  else lines_frame(segs + (long long)b * 4 * MAXLINES, frame[3 * b + 2], oimg + fb, H, W, tab);
}

}  // namespace

extern "C" int egne_augment_cv(const uint8_t* img, const int64_t* label, const int32_t* frame, const int32_t* frame_host,
                               const double* segs, const double* rot, const int32_t* q8, const double* phase, uint8_t* out_img,
                               int64_t* out_label, int B, int H, int W, void* stream) {
  EGNE_REQUIRE(img && label && frame && frame_host && segs && rot && q8 && phase && out_img && out_label, "augment_cv: null pointer");
  EGNE_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && H <= 32768 && W <= 32768, "augment_cv: bad shape (B %d H %d W %d)", B, H, W);
  EGNE_REQUIRE((const void*)img != (const void*)out_img && (const void*)label != (const void*)out_label,
               "augment_cv: in place is not supported (blur and rotation read neighbours)");
  bool any = false;
  for (int b = 0; b < B; ++b) {
    const int ch = frame_host[3 * b], sigma = frame_host[3 * b + 1], nl = frame_host[3 * b + 2];
    if (ch == 1) {
      EGNE_REQUIRE(H >= 4 && W >= 4, "augment_cv: a blurred frame needs H, W >= 4 (one reflection), got %dx%d", H, W);
      EGNE_REQUIRE(sigma >= 2 && sigma <= 6, "augment_cv: frame %d: sigma %d outside 2..6", b, sigma);
    }
    if (ch == 5) EGNE_REQUIRE(nl >= 0 && nl <= MAXLINES, "augment_cv: frame %d: %d lines (at most %d)", b, nl, MAXLINES);
    any = any || ch == 1 || ch == 5 || ch == 6;
  }
  if (!any) return EGNE_OK;
  const int tiles_x = (W + CT - 1) / CT, tiles_y = (H + CT - 1) / CT;
  hipLaunchKernelGGL(augment_cv_k, dim3(tiles_x * tiles_y, B), dim3(256), 0, (hipStream_t)stream, img, (const long long*)label, frame,
                     segs, rot, q8, phase, out_img, (long long*)out_label, H, W, tiles_x);
  return egne::check_launch("egne_augment_cv");
}
