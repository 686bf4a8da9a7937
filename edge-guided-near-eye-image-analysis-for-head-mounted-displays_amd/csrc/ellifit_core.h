// ElliFit + RANSAC on boundary points (csrc/ellifit.hip): everything that is plain arithmetic -- the workspace layout, the draw
// generator, the moments, the 5x5 solve, the model and its residual -- so that the stand-alone host program of
// tests/test_host_ellifit.py compiles the very same text with a host compiler.  No HIP type appears here.
// Float64 throughout; the translation unit that includes this is built without FMA contraction.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define EF_HD __host__ __device__ __forceinline__
#else
#define EF_HD inline
#endif

#define EF_MAX_PTS 16384
#define EF_MAX_NMIN 64
#define EF_MAX_ITERS 4096
#define EF_DRAW_ROUNDS 4      // generated draws: at most 4 x 64 attempts per sample

// ---- workspace: per row  [hdr 128 B][bits u64 H*wpr][offs i32 H*wpr, padded to 8 B][pts u32 max_pts] -------------------------------
struct EfLayout {
  size_t wpr, nwords, off_bits, off_offs, off_pts, row_bytes;
};

EF_HD bool ef_shape_ok(int H, int W) { return H >= 2 && W >= 2 && H <= 1024 && W <= 1024; }
EF_HD bool ef_pts_ok(int max_pts) { return max_pts >= 1 && max_pts <= EF_MAX_PTS; }

EF_HD EfLayout ef_layout(int H, int W, int max_pts) {
  EfLayout l;
  l.wpr = (size_t)(W + 63) / 64;
  l.nwords = (size_t)H * l.wpr;
  l.off_bits = 128;
  l.off_offs = l.off_bits + l.nwords * 8;
  l.off_pts = l.off_offs + ((l.nwords * 4 + 7) & ~(size_t)7);
  l.row_bytes = l.off_pts + (((size_t)max_pts * 4 + 7) & ~(size_t)7);
  return l;
}

// negative: refused
EF_HD int64_t ef_workspace_bytes(int n, int H, int W, int max_pts) {
  if (n < 1 || !ef_shape_ok(H, W) || !ef_pts_ok(max_pts)) return -1;
  return (int64_t)((size_t)n * ef_layout(H, W, max_pts).row_bytes);
}

// dynamic LDS of the RANSAC kernel: points, one sample per wave, one result slot per wave, one flag word
EF_HD size_t ef_lds_bytes(int max_pts) { return (size_t)max_pts * 4 + 4 * EF_MAX_NMIN * 4 + 4 * 16 * 8 + 16; }

// ---- draws: counter-based hash of (seed, row, iteration, attempt), reduced to [0, N) by multiply-high -----------------------------
EF_HD uint32_t ef_mix(uint32_t x) {      // a 32-bit finaliser (xor-shift / multiply rounds)
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
EF_HD uint32_t ef_hash(uint32_t seed, uint32_t row, uint32_t iter, uint32_t attempt) {
  uint32_t h = ef_mix(seed + 0x9e3779b9u);
  h = ef_mix(h ^ row);
  h = ef_mix(h ^ iter);
  return ef_mix(h ^ attempt);
}
EF_HD int ef_draw_index(uint32_t h, int N) { return (int)(((uint64_t)h * (uint64_t)(uint32_t)N) >> 32); }

// ---- Fit -------------------------------------------------------------------------------------------------------------------------
// the 13 sums of monomials of the centred points that X^T X and X^T Y are made of (X = [x^2, 2xy, -2x, -2y, -1], Y = -y^2):
//   0 x^4  1 x^3y  2 x^2y^2  3 xy^3  4 x^3  5 x^2y  6 xy^2  7 y^3  8 x^2  9 xy  10 y^2  11 x  12 y     (the 14th is the count)
#define EF_NMOM 13
EF_HD void ef_accum(double* s, double x, double y) {
  const double x2 = x * x, y2 = y * y, xy = x * y;
  s[0] += x2 * x2; s[1] += x2 * xy; s[2] += x2 * y2; s[3] += xy * y2;
  s[4] += x2 * x;  s[5] += x2 * y;  s[6] += x * y2;  s[7] += y2 * y;
  s[8] += x2;      s[9] += xy;      s[10] += y2;     s[11] += x;      s[12] += y;
}

EF_HD bool ef_finite(double v) { return v - v == 0.0; }

// Phi from the normal equations by a Cholesky factorisation (the matrix is a Gram matrix; no pivoting, every index static).
// false: a pivot that is not a positive finite number (singular or indefinite in floating point)
EF_HD bool ef_solve(const double* s, double cnt, double* Phi) {
  double A[5][5], r[5];
  A[0][0] = s[0];  A[1][0] = 2.0 * s[1];  A[2][0] = -2.0 * s[4];  A[3][0] = -2.0 * s[5];  A[4][0] = -s[8];
  A[1][1] = 4.0 * s[2];  A[2][1] = -4.0 * s[5];  A[3][1] = -4.0 * s[6];  A[4][1] = -2.0 * s[9];
  A[2][2] = 4.0 * s[8];  A[3][2] = 4.0 * s[9];   A[4][2] = 2.0 * s[11];
  A[3][3] = 4.0 * s[10]; A[4][3] = 2.0 * s[12];
  A[4][4] = cnt;
  r[0] = -s[2]; r[1] = -2.0 * s[3]; r[2] = 2.0 * s[6]; r[3] = 2.0 * s[7]; r[4] = s[10];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    double d = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
    ok = ok && d > 0.0 && ef_finite(d);
    const double l = sqrt(d);
    A[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < 5; ++i) {
      double v = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= A[i][k] * A[j][k];
      A[i][j] = v / l;
    }
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {          // L z = r
    double v = r[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= A[i][k] * r[k];
    r[i] = v / A[i][i];
  }
#pragma unroll
  for (int i = 4; i >= 0; --i) {         // L^T Phi = z
    double v = r[i];
#pragma unroll
    for (int k = i + 1; k < 5; ++k) v -= A[k][i] * r[k];
    r[i] = v / A[i][i];
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) { Phi[i] = r[i]; ok = ok && ef_finite(r[i]); }
  return ok;
}

// (cx, cy, a, b, theta) of the conic x^2 p0 + 2xy p1 - 2x p2 - 2y p3 - p4 = -y^2 in centred coordinates, operations in the order of
// helperfunctions.py:249-257 (sums left to right); false (and five times -1) for a model with a non-finite entry
EF_HD bool ef_model(const double* Phi, double xm, double ym, double* model) {
  const double p0 = Phi[0], p1 = Phi[1], p2 = Phi[2], p3 = Phi[3], p4 = Phi[4];
  const double den = p0 - p1 * p1;
  const double cx = (p2 - p3 * p1) / den;
  const double cy = (p0 * p3 - p2 * p1) / den;
  const double om = 1.0 - p0;
  const double spread = sqrt(om * om + 4.0 * (p1 * p1));
  const double scale = p4 + cy * cy + (cx * cx) * p0 + 2.0 * p1;
  const double trace = 1.0 + p0;
  const double b = sqrt(2.0 * scale / (trace + spread));
  const double a = sqrt(2.0 * scale / (trace - spread));
  const double tilt = 0.5 * atan2(2.0 * p1, om);
  model[0] = cx + xm; model[1] = cy + ym; model[2] = a; model[3] = b; model[4] = -tilt;
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 5; ++i) ok = ok && ef_finite(model[i]);
  if (!ok) {
#pragma unroll
    for (int i = 0; i < 5; ++i) model[i] = -1.0;
  }
  return ok;
}

// helperfunctions.py:267-276: what a residual needs of a model, and the residual of one point
struct EfErr {
  double cx, cy, c, s, ia, ib;
};
EF_HD EfErr ef_err_prep(const double* model) {
  EfErr e;
  e.cx = model[0]; e.cy = model[1];
  e.c = cos(model[4]); e.s = sin(model[4]);
  e.ia = 1.0 / (model[2] * model[2]);
  e.ib = 1.0 / (model[3] * model[3]);
  return e;
}
EF_HD double ef_err(const EfErr& e, double x, double y) {
  const double dx = x - e.cx, dy = y - e.cy;
  const double t1 = dx * e.c, t2 = dy * e.s, t3 = dx * e.s, t4 = dy * e.c;
  const double u = t1 - t2, v = t3 + t4;
  return fabs(e.ia * (u * u) + e.ib * (v * v) - 1.0);
}

// my_ellipse(model).verify of one point: p^T M p with M = param2mat(model) (helperfunctions.py:25-33), i.e. the conic whose
// rotation is rotation_2d(-theta) -- NOT the residual above, whose rotation has the other sign
EF_HD double ef_verify_pt(const EfErr& e, double x, double y) {
  const double dx = x - e.cx, dy = y - e.cy;
  const double u = dx * e.c + dy * e.s, v = dy * e.c - dx * e.s;
  return e.ia * (u * u) + e.ib * (v * v) - 1.0;
}

// the fitted ellipse in the coordinate convention of the search.  The model is the ellipse my_ellipse draws from it:
// a lies along (cos t, sin t), t = model[4], x = column, y = row (on drawn ellipses this is the drawn one; the residual above turns
// the other way, which is the reference's).  Second-moment form, scaled by sx = W/(W-1), sy = H/(H-1), read back as calc_ell_iou does
EF_HD void ef_to_search(const double* model, int H, int W, double* init) {
  const double sx = (double)W / (W - 1), sy = (double)H / (H - 1);
  const double c = cos(model[4]), s = sin(model[4]);
  const double a2 = model[2] * model[2], b2 = model[3] * model[3];
  const double mxx = (a2 * (c * c) + b2 * (s * s)) * (sx * sx);
  const double myy = (a2 * (s * s) + b2 * (c * c)) * (sy * sy);
  const double mxy = ((a2 - b2) * (c * s)) * (sx * sy);
  const double d = mxx - myy, rr = sqrt(d * d + 4.0 * mxy * mxy);
  init[0] = model[0] * sx;
  init[1] = model[1] * sy;
  init[2] = sqrt((mxx + myy + rr) / 2.0);
  init[3] = sqrt(fmax((mxx + myy - rr) / 2.0, 0.0));
  init[4] = 0.5 * atan2(2.0 * mxy, d);
}
