// Prediction overlay grid (csrc/dispgrid.hip): the arithmetic that can go wrong on a host -- the uint8 conversion of a
// frame, the equalisation table, the grey table behind it, the roundings, the outline's clip and the grid offsets.  Plain C++ without
// a HIP type: the kernels include it, and tests/dispgrid_host.cpp compiles the very same text with a host compiler under
// -fsanitize=address,undefined.  Every float32 operation here is meant to round once: the including file is built without FMA
// contraction (Makefile; the host program likewise).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EGNE_DG_HD __host__ __device__ inline
#else
#define EGNE_DG_HD inline
#endif

namespace egne_dispgrid {

// status bits of a drawn frame (include/egne_hip.h)
enum { ST_CONSTANT = 1, ST_NONFINITE = 2, ST_SKIP_IRIS = 4, ST_SKIP_PUPIL = 8, ST_SKIP_GT_IRIS = 16, ST_SKIP_GT_PUPIL = 32 };

EGNE_DG_HD uint32_t f32_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
EGNE_DG_HD float bits_f32(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

// A float32 as an unsigned key whose integer order is the float order (-0 below +0): integer atomic max / min across workgroups.
EGNE_DG_HD uint32_t order_key(float x) {
  const uint32_t u = f32_bits(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
EGNE_DG_HD float key_value(uint32_t k) { return bits_f32((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// float32 division rounded to nearest: IEEE on a host, __fdiv_rn in device code
EGNE_DG_HD float div_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(a, b);
#else
  return a / b;
#endif
}
EGNE_DG_HD bool finite_f32(float x) { return (f32_bits(x) & 0x7f800000u) != 0x7f800000u; }

// np.uint8(255 * (x - mn) / d) of utils.py:270-272 with d = fl32(mx - mn): three float32 operations, the division correctly rounded,
// the conversion truncates.  What NumPy leaves undefined is defined: NaN and negative quotients give 0, quotients from 255 up give 255.
EGNE_DG_HD uint8_t to_u8(float x, float mn, float d) {
  const float t = 255.0f * (x - mn);
  const float q = div_rn(t, d);
  if (!(q >= 0.0f)) return 0;
  if (q >= 255.0f) return 255;
  return (uint8_t)(int)q;
}

// ---- OpenCV's published equalizeHist rule ------------------------------------------------------------------------------------------
// i0 = first occupied bin; if it holds every pixel the output is i0 everywhere; otherwise scale = 255.f / float(total - hist[i0]),
// lut[i0] = 0 and lut[k] = saturate(round_half_even(float(sum_{i0 < j <= k} hist[j]) * scale)) behind it.
EGNE_DG_HD float lut_scale(int total, int h0) { return div_rn(255.0f, (float)(total - h0)); }
EGNE_DG_HD uint8_t lut_entry(int sum, float scale) {
  const float r = rintf((float)sum * scale);          // ties to even in the default rounding mode
  return r <= 0.0f ? 0 : (r >= 255.0f ? 255 : (uint8_t)(int)r);
}
// the table entry of bin k from the INCLUSIVE running sum cum_k = sum_{j <= k} hist[j] (bins below i0 are empty)
EGNE_DG_HD uint8_t lut_of_bin(int k, int i0, int h0, int cum_k, int total) {
  if (h0 == total) return (uint8_t)i0;
  if (k <= i0) return 0;
  return lut_entry(cum_k - h0, lut_scale(total, h0));
}
// utils.py:273-274: e - min(e) in uint8, then float32(double(e) / double(max(e))) -- emin / emax: the extremes of lut over the
// OCCUPIED bins.  For a non-constant frame u takes the value 0 and the last occupied bin's running sum is total, so emin = 0 and
// emax = 255; the general form stays.  A frame whose e is constant (emax == emin: the reference divides 0 by 0) is grey 0.
EGNE_DG_HD float grey_of(uint8_t e, uint8_t emin, uint8_t emax) {
  if (emax == emin) return 0.0f;
  return (float)((double)(uint8_t)(e - emin) / (double)(uint8_t)(emax - emin));
}

// Sequential form of the whole table (the kernel does the running sum by a wave scan and calls the same entry functions):
// hist[256] -> lut[256], grey[256] (entries of empty bins are defined, never read).  Returns i0, -1 for an empty histogram.
EGNE_DG_HD int build_tables(const int* hist, int total, uint8_t* lut, float* grey) {
  int i0 = -1;
  for (int k = 0; k < 256 && i0 < 0; ++k)
    if (hist[k] > 0) i0 = k;
  const int h0 = i0 < 0 ? 0 : hist[i0];
  int cum = 0, emin = 255, emax = 0;
  for (int k = 0; k < 256; ++k) {
    cum += hist[k];
    lut[k] = i0 < 0 ? 0 : lut_of_bin(k, i0, h0, cum, total);
    if (hist[k] > 0) { emin = lut[k] < emin ? lut[k] : emin; emax = lut[k] > emax ? lut[k] : emax; }
  }
  if (i0 < 0) emin = emax = 0;
  for (int k = 0; k < 256; ++k) grey[k] = grey_of(lut[k], (uint8_t)emin, (uint8_t)emax);
  return i0;
}

// the uint8 form of a grid value: rint(255 * min(max(g, 0), 1)) in float32 (the painted 255s saturate; this project's choice)
EGNE_DG_HD uint8_t u8_of_grid(float g) {
  const float c = g > 0.0f ? (g < 1.0f ? g : 1.0f) : 0.0f;
  return (uint8_t)(int)rintf(255.0f * c);
}

// ---- outlines ----------------------------------------------------------------------------------------------------------------------
// a pixel ellipse (cx, cy, a, b, theta) is drawn iff its parameters are finite and int(a), int(b) are at least 1
EGNE_DG_HD bool ellipse_drawn(const double* el) {
  for (int k = 0; k < 5; ++k)
    if (!(fabs(el[k]) <= 1.7976931348623157e308)) return false;
  return trunc(el[2]) >= 1.0 && trunc(el[3]) >= 1.0;
}
// ndarray.clip(6, n - 6) taken literally: min(max(v, 6), n - 6), also where n - 6 < 6.  Done in float64 before the conversion, so
// that a coordinate beyond int32 is defined too (NaN: 6, then the upper bound).  n >= 6 keeps the result inside [0, n).
EGNE_DG_HD int clip_px(double v, int n) { return (int)fmin(fmax(v, 6.0), (double)(n - 6)); }
// sample (ct, st) = (cos t, sin t) of the outline of the ellipse with truncated centre (cx, cy), truncated axes (a, b) and
// (ca, sa) = (cos theta, sin theta): evaluate._draw_ellipse's expressions in float64, rounded to the nearest integer (ties to even),
// then the reference's clip
EGNE_DG_HD void outline_px(double cx, double cy, double a, double b, double ca, double sa, double ct, double st, int H, int W, int* row,
                           int* col) {
  const double x = cx + a * ct * ca - b * st * sa;
  const double y = cy + a * ct * sa + b * st * ca;
  *col = clip_px(rint(x), W);
  *row = clip_px(rint(y), H);
}

// ---- torchvision.utils.make_grid(nrow, padding=2, pad_value=0) by its documented layout ---------------------------------------------
struct Layout { int xm, ym, Hg, Wg; };
EGNE_DG_HD Layout grid_layout(int n, int nrow, int H, int W) {
  Layout g;
  if (n == 1) { g.xm = g.ym = 1; g.Hg = H; g.Wg = W; return g; }          // one frame: the frame itself, no padding
  g.xm = nrow < n ? nrow : n;
  g.ym = (n + g.xm - 1) / g.xm;
  g.Hg = g.ym * (H + 2) + 2;
  g.Wg = g.xm * (W + 2) + 2;
  return g;
}
EGNE_DG_HD void grid_origin(int k, int n, const Layout& g, int H, int W, int* row, int* col) {
  if (n == 1) { *row = *col = 0; return; }
  *row = (k / g.xm) * (H + 2) + 2;
  *col = (k % g.xm) * (W + 2) + 2;
}

}  // namespace egne_dispgrid
