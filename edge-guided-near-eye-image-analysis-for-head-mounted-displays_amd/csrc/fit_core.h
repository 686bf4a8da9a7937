// The device functions of the ellipse fit (csrc/fit.hip): the float64 conic algebra of helperfunctions.py:13-63,102-129, the
// normalised <-> pixel ellipse transforms, the reference's float32 membership rule (utils.py:185-196) and ONE IoU evaluation of an
// ellipse against a bit-packed map.  Shared by csrc/fit.hip (search, counts, seeds from the regression head) and
// csrc/ellipse_scores.hip (ellipse scores against ground truth), so that both give the same bits for the same ellipse.
// Device code; include it inside the including file's anonymous namespace, after common.h.  The including file is built without FMA
// contraction (Makefile): every float32 operation of the rule is rounded once, as NumPy rounds it.
#pragma once

constexpr double PI_REF = 3.14159;
constexpr double EPS_B = 1e-40;  // helperfunctions.py:10

struct M3 { double v[3][3]; };

__device__ M3 mul(const M3& a, const M3& b) {
  M3 r;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = a.v[i][0] * b.v[0][j];
      s = s + a.v[i][1] * b.v[1][j];
      s = s + a.v[i][2] * b.v[2][j];
      r.v[i][j] = s;
    }
  return r;
}
__device__ M3 tr(const M3& a) {
  M3 r;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r.v[i][j] = a.v[j][i];
  return r;
}
__device__ M3 rot(double t) {
  const double c = cos(t), s = sin(t);
  M3 r = {{{c, -s, 0.0}, {s, c, 0.0}, {0.0, 0.0, 1.0}}};
  return r;
}
__device__ M3 trans(double x, double y) {
  M3 r = {{{1.0, 0.0, x}, {0.0, 1.0, y}, {0.0, 0.0, 1.0}}};
  return r;
}

// pixel ellipse (cx,cy,a,b,theta) -> parameters on the normalised mesh (helperfunctions.py:25-33,
// :124-129 with H = [[2/W,0,-1],[0,2/H,-1],[0,0,1]], :50-63)
__device__ void normalise(const double* el, int Hh, int Ww, double* out) {
  const M3 Hr = rot(-el[4]), Ht = trans(-el[0], -el[1]);
  M3 Q = {{{1.0 / (el[2] * el[2]), 0, 0}, {0, 1.0 / (el[3] * el[3]), 0}, {0, 0, -1.0}}};
  M3 mat = mul(mul(mul(mul(tr(Ht), tr(Hr)), Q), Hr), Ht);
  // inverse of the normalising homography, analytically
  M3 Hi = {{{Ww / 2.0, 0, Ww / 2.0}, {0, Hh / 2.0, Hh / 2.0}, {0, 0, 1.0}}};
  M3 mt = mul(mul(tr(Hi), mat), Hi);
  const double a = mt.v[0][0], b = 2 * mt.v[0][1], c = mt.v[1][1], dd = 2 * mt.v[0][2], e = 2 * mt.v[1][2];
  double theta;
  if (fabs(b) <= EPS_B && a <= c) theta = 0.0;
  else if (fabs(b) <= EPS_B && a > c) theta = 3.141592653589793 / 2;
  else theta = 0.5 * atan2(b, a - c);
  const double den = b * b - 4 * a * c;
  const double tx = (2 * c * dd - b * e) / den, ty = (2 * a * e - b * dd) / den;
  const M3 R = rot(theta), T = trans(tx, ty);
  M3 mn = mul(mul(mul(mul(tr(R), tr(T)), mt), T), R);
  out[0] = tx; out[1] = ty;
  out[2] = sqrt(1.0 / mn.v[0][0]); out[3] = sqrt(1.0 / mn.v[1][1]);
  out[4] = theta;
}

// normalised ellipse (cx,cy,a,b,theta on the [-1,1] mesh, widened float32) -> pixel ellipse: my_ellipse(p).transform(H)[0][:-1] with
// H = [[W/2,0,W/2],[0,H/2,H/2],[0,0,1]] (evaluate.py:135-151, test.py:113-121; helperfunctions.py:25-33, :50-63, :124-129) in float64
__device__ void norm_to_pixel(const double* el, int H, int W, double* out) {
  const M3 Hr = rot(-el[4]), Ht = trans(-el[0], -el[1]);
  M3 Q = {{{1.0 / (el[2] * el[2]), 0, 0}, {0, 1.0 / (el[3] * el[3]), 0}, {0, 0, -1.0}}};
  const M3 mat = mul(mul(mul(mul(tr(Ht), tr(Hr)), Q), Hr), Ht);
  const M3 Hi = {{{2.0 / W, 0, -1.0}, {0, 2.0 / H, -1.0}, {0, 0, 1.0}}};       // inverse of the un-normalising homography
  const M3 mt = mul(mul(tr(Hi), mat), Hi);
  const double a = mt.v[0][0], b = 2 * mt.v[0][1], c = mt.v[1][1], dd = 2 * mt.v[0][2], ee = 2 * mt.v[1][2];
  double theta;
  if (fabs(b) <= EPS_B && a <= c) theta = 0.0;
  else if (fabs(b) <= EPS_B && a > c) theta = 3.141592653589793 / 2;
  else theta = 0.5 * atan2(b, a - c);
  const double den = b * b - 4 * a * c;
  const double tx = (2 * c * dd - b * ee) / den, ty = (2 * a * ee - b * dd) / den;
  const M3 R = rot(theta), T = trans(tx, ty);
  const M3 mn = mul(mul(mul(mul(tr(R), tr(T)), mt), T), R);
  out[0] = tx; out[1] = ty;
  out[2] = sqrt(1.0 / mn.v[0][0]); out[3] = sqrt(1.0 / mn.v[1][1]);
  out[4] = theta;
}

struct Ell { float cx, cy, a, b, ct, st; };

// the float32 ellipse one evaluation rasterises: (cx, cy, q[0], q[1]) pixels and q[2] DEGREES -> the normalised mesh (calc_ell_iou with
// nor=False, angle_nor=True: utils.py:178-183)
__device__ __forceinline__ Ell ell_on_mesh(int H, int W, double cx, double cy, const double* q) {
  double el[5] = {cx, cy, q[0], q[1], q[2] / 180. * PI_REF};
  double nm[5];
  normalise(el, H, W, nm);
  const Ell E = {(float)nm[0], (float)nm[1], (float)nm[2], (float)nm[3], (float)cos(nm[4]), (float)sin(nm[4])};
  return E;
}

__device__ __forceinline__ bool inside_px(const Ell& e, float xv, float dyst, float dyct) {
  const float dx = __fsub_rn(xv, e.cx);
  const float X = __fadd_rn(__fmul_rn(dx, e.ct), dyst);
  const float Y = __fadd_rn(__fmul_rn(-dx, e.st), dyct);
  const float u = __fdiv_rn(X, e.a), v = __fdiv_rn(Y, e.b);
  const float wt = __fsub_rn(__fadd_rn(__fmul_rn(u, u), __fmul_rn(v, v)), 1.0f);
  return wt <= 0.f;
}

// bits of row `rowbits` (wpr words) in pixel range [x0, x1] (inclusive, 0 <= x0 <= x1 < W): popcount
__device__ __forceinline__ unsigned row_pop(const unsigned* rowbits, int x0, int x1) {
  unsigned n = 0;
  for (int w = x0 >> 5; w <= (x1 >> 5); ++w) {
    unsigned m = 0xffffffffu;
    if (w == (x0 >> 5)) m &= 0xffffffffu << (x0 & 31);
    if (w == (x1 >> 5)) m &= 0xffffffffu >> (31 - (x1 & 31));
    n += __popc(rowbits[w] & m);
  }
  return n;
}

// Bit-packs the class-k pixels of rows first, first + step, ... of frame m into bits[H][wpr] and returns how many there are (wave-uniform:
// ballots); the waves that share a mask pack its rows in turn.
__device__ __forceinline__ unsigned pack_mask_rows(const long long* __restrict__ m, int k, int H, int W, unsigned* bits, int wpr, int lane,
                                                   int first, int step) {
  unsigned cnt = 0;
  for (int y = first; y < H; y += step)
    for (int x0 = 0; x0 < W; x0 += 64) {          // one coalesced 512-byte load per step, the class test of 64 pixels as one ballot
      const int x = x0 + lane;
      const unsigned long long bal = __ballot(x < W && m[(long long)y * W + x] == k);
      cnt += (unsigned)__popcll(bal);
      if (lane == 0) bits[y * wpr + (x0 >> 5)] = (unsigned)bal;
      if (lane == 1 && (x0 >> 5) + 1 < wpr) bits[y * wpr + (x0 >> 5) + 1] = (unsigned)(bal >> 32);
    }
  return cnt;
}

// The map of an ellipse itself in the layout of pack_mask_rows: every pixel of rows first, first + step, ... through the membership
// rule (inside_px, the operations of evaluate_ell's exact tests in their order); returns how many are inside (wave-uniform).
__device__ __forceinline__ unsigned pack_ellipse_rows(const Ell& E, int H, int W, const float* lxs, const float* lys, unsigned* bits, int wpr,
                                                      int lane, int first, int step) {
  unsigned cnt = 0;
  for (int y = first; y < H; y += step) {
    const float dy = __fsub_rn(lys[y], E.cy);
    const float dyst = __fmul_rn(dy, E.st), dyct = __fmul_rn(dy, E.ct);
    for (int x0 = 0; x0 < W; x0 += 64) {
      const int x = x0 + lane;
      const unsigned long long bal = __ballot(x < W && inside_px(E, lxs[x < W ? x : 0], dyst, dyct));
      cnt += (unsigned)__popcll(bal);
      if (lane == 0) bits[y * wpr + (x0 >> 5)] = (unsigned)bal;
      if (lane == 1 && (x0 >> 5) + 1 < wpr) bits[y * wpr + (x0 >> 5) + 1] = (unsigned)(bal >> 32);
    }
  }
  return cnt;
}

// IoU counts of the packed mask with the ellipse (cx, cy, q[0], q[1], q[2] degrees): pixels inside the ellipse (ne) and those of them set in
// the mask (ni), over the rows y_lo + part * 64 + lane (+ 64 * ROWW ...) of its bounding box, summed over the wave; every lane computes the
// same parameters.  One evaluation of the search (ellipse_fit_k) and the whole of ellipse_counts_k.
template <int ROWW>
__device__ __forceinline__ void evaluate_ell(int H, int W, const float* lxs, const float* lys, const unsigned* bits, int wpr, double cx, double cy,
                                             int lane, int part, const double* q, unsigned& ne_out, unsigned& ni_out) {
  const Ell E = ell_on_mesh(H, W, cx, cy, q);
  // Only pixels inside the ellipse count (ne, ni), and the ellipse lies within max(a, b) of its centre: rows of the
  // bounding box (0.1 % + 2 pixels of slack, orders of magnitude above float32 round-off) instead of the frame.
  // Degenerate parameters (NaN / huge axes) fall back to the full frame, every pixel tested.
  int y_lo = 0, y_hi = H - 1, x_lo = 0, x_hi = W - 1;
  const float rr = fmaxf(E.a, E.b) * 1.001f;
  const bool tame = rr < 4.f && fabsf(E.cx) < 4.f && fabsf(E.cy) < 4.f && fminf(E.a, E.b) > 1e-3f;
  const float sx = 0.5f * (float)(W - 1), sy = 0.5f * (float)(H - 1);
  if (tame) {
    const int xl = (int)floorf((E.cx - rr + 1.f) * sx) - 2, xh = (int)ceilf((E.cx + rr + 1.f) * sx) + 2;
    const int yl = (int)floorf((E.cy - rr + 1.f) * sy) - 2, yh = (int)ceilf((E.cy + rr + 1.f) * sy) + 2;
    y_lo = max(yl, 0); y_hi = min(yh, H - 1);
    x_lo = max(xl, 0); x_hi = min(xh, W - 1);
  }
  unsigned ne = 0, ni = 0;
  if (y_hi >= y_lo && x_hi >= x_lo) {
    // the row quadratic A dx^2 + Bq dx + C <= 0 (approximate arithmetic: it only seeds the exact walk)
    const float ia = 1.f / (E.a * E.a), ib = 1.f / (E.b * E.b);
    const float A = E.ct * E.ct * ia + E.st * E.st * ib, Bc = 2.f * E.st * E.ct * (ia - ib), Cc = E.st * E.st * ia + E.ct * E.ct * ib;
    for (int y = y_lo + part * 64 + lane; y <= y_hi; y += 64 * ROWW) {
      const float dy = __fsub_rn(lys[y], E.cy);
      const float dyst = __fmul_rn(dy, E.st), dyct = __fmul_rn(dy, E.ct);
      const unsigned* rowbits = bits + y * wpr;
      // pixels [t0, t1] of the row tested one by one; an interval [il, ir] counted as a whole
      int t0 = 0, t1 = -1, il = 0, ir = -1;
      if (!tame) {
        t0 = x_lo; t1 = x_hi;
      } else {
        const float Bq = Bc * dy, C = Cc * dy * dy - 1.f, disc = Bq * Bq - 4.f * A * C;
        const int xv = (int)floorf((-Bq / (2.f * A) + E.cx + 1.f) * sx);        // pixel next to the row's closest approach
        bool whole = false;
        if (!(disc > 0.f)) {
          // the row misses the ellipse (or grazes it): round-off can only matter next to the closest approach
          t0 = max(xv - 4, 0); t1 = min(xv + 5, W - 1);
          whole = t1 >= t0 && (inside_px(E, lxs[t0], dyst, dyct) || inside_px(E, lxs[t1], dyst, dyct));
        } else {
          const float sq = sqrtf(disc), dl = (-Bq - sq) / (2.f * A), dr = (-Bq + sq) / (2.f * A);
          il = (int)ceilf((dl + E.cx + 1.f) * sx);
          ir = (int)floorf((dr + E.cx + 1.f) * sx);
          if (ir - il < 12) {
            // short interval (tangent rows): its pixels and four more on either side, one by one; the outermost must be outside
            t0 = max(il - 4, 0); t1 = min(ir + 4, W - 1);
            whole = t1 >= t0 && ((t0 > 0 && inside_px(E, lxs[t0], dyst, dyct)) || (t1 < W - 1 && inside_px(E, lxs[t1], dyst, dyct)));
            il = 0; ir = -1;
          } else {
            // walk each end with the exact predicate: il inside and il - 1 outside (or il = 0), ir inside and ir + 1 outside (or ir = W - 1)
            il = min(max(il, 0), W - 1); ir = min(max(ir, 0), W - 1);
            int steps = 0;
            while (steps < 8 && il > 0 && inside_px(E, lxs[il - 1], dyst, dyct)) { --il; ++steps; }
            while (steps < 8 && il < W - 1 && !inside_px(E, lxs[il], dyst, dyct)) { ++il; ++steps; }
            steps = 0;
            while (steps < 8 && ir < W - 1 && inside_px(E, lxs[ir + 1], dyst, dyct)) { ++ir; ++steps; }
            while (steps < 8 && ir > 0 && !inside_px(E, lxs[ir], dyst, dyct)) { --ir; ++steps; }
            const bool settled = il <= ir && inside_px(E, lxs[il], dyst, dyct) && (il == 0 || !inside_px(E, lxs[il - 1], dyst, dyct)) &&
                                 inside_px(E, lxs[ir], dyst, dyct) && (ir == W - 1 || !inside_px(E, lxs[ir + 1], dyst, dyct));
            if (!settled) { whole = true; il = 0; ir = -1; }
          }
        }
        if (whole) { t0 = 0; t1 = W - 1; }          // something unexpected: every pixel of the row, as the reference does
      }
      for (int x = t0; x <= t1; ++x)
        if (inside_px(E, lxs[x], dyst, dyct)) { ++ne; ni += (rowbits[x >> 5] >> (x & 31)) & 1u; }
      if (ir >= il) {
        ne += (unsigned)(ir - il + 1);
        ni += row_pop(rowbits, il, ir);
      }
    }
  }
  for (int o = 32; o >= 1; o >>= 1) { ne += __shfl_xor(ne, o); ni += __shfl_xor(ni, o); }
  ne_out = ne; ni_out = ni;
}
