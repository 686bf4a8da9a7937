// Label maps from TEyeD annotations (csrc/annot.hip): the rules that decide a pixel -- the eyeball circle, the iris and
// pupil ellipses, the eyelid polygon -- and the packed record they are read from.  Plain C++ without a HIP type: the kernel includes
// it, and tests/annot_host.cpp compiles the very same text with a host compiler under -fsanitize=address,undefined.  Everything is
// integer-exact or float64 with every operation rounded on its own: the including file is built without FMA contraction (Makefile;
// the host program likewise).  tests/annot_refs.py restates it in NumPy, byte for byte.
//
// The rules are this project's own, NOT OpenCV's pixels (include/egne_hip.h states them in full); what the reference pins is the
// arguments its scripts hand to cv2.circle / cv2.ellipse / cv2.fillPoly (tests/golden/annot.npz).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EGNE_AN_HD __host__ __device__ inline
#else
#define EGNE_AN_HD inline
#endif

namespace egne_annot {

// ---- the record of one frame: kRecordWords 32-bit words (dataprep.pack_annotations writes it) -------------------------------------
//   word 0        flags: which shapes are present
//   word 1        n: vertices of the lid polygon, 0 .. kMaxVerts (larger or negative values are read as clamped)
//   words 2..4    ball: bx, by, br                     (int32)
//   word 5        0
//   words 6..9    iris: ex, ey, A, B                   (int32), words 10..13: c, s (float64: cos and sin of the angle)
//   words 14..17  pupil: ex, ey, A, B                  (int32), words 18..21: c, s (float64)
//   words 22..    lid: x0, y0, x1, y1, ...             (int32, kMaxVerts pairs; pairs from n on are ignored)
// Every integer is at most kMaxCoord in magnitude: no int64 product below can overflow.
enum { HAS_BALL = 1, HAS_IRIS = 2, HAS_PUPIL = 4, HAS_LID = 8 };
// status bits of a painted frame
enum { ST_IRIS_ZERO_AXIS = 1, ST_PUPIL_ZERO_AXIS = 2, ST_EMPTY = 4 };
constexpr int kMaxVerts = 64;
constexpr int kMaxCoord = 1 << 20;
constexpr int kBallWord = 2, kIrisWord = 6, kPupilWord = 14, kLidWord = 22;
constexpr int kRecordWords = kLidWord + 2 * kMaxVerts;        // 150 words, 600 bytes: a multiple of 8, the float64 words stay aligned

struct Ellipse {
  int ex, ey, A, B;
  double c, s;
};

EGNE_AN_HD Ellipse load_ellipse(const int32_t* w) {
  Ellipse e;
  e.ex = w[0]; e.ey = w[1]; e.A = w[2]; e.B = w[3];
  memcpy(&e.c, w + 4, 8);
  memcpy(&e.s, w + 6, 8);
  return e;
}
EGNE_AN_HD int lid_count(const int32_t* rec) {
  const int n = rec[1];
  return n < 0 ? 0 : (n > kMaxVerts ? kMaxVerts : n);
}

// ---- circle: dx * dx + dy * dy <= br * br in int64; br == 0 is the centre pixel, br < 0 nothing ---------------------------------
EGNE_AN_HD bool in_circle(int x, int y, int bx, int by, int br) {
  if (br < 0) return false;
  const int64_t dx = (int64_t)x - bx, dy = (int64_t)y - by, r = br;
  return dx * dx + dy * dy <= r * r;
}

// ---- ellipse -------------------------------------------------------------------------------------------------------------------------
// X = dx * c + dy * s, Y = dy * c - dx * s (cv2.ellipse's convention: first axis along (c, s), y down); the pixel belongs iff
// (X * B) * (X * B) + (Y * A) * (Y * A) <= (A * B) * (A * B), every operation rounded on its own in this order.  A half-axis of zero
// (or below) paints nothing.  The rule is evaluated inside the square |dx|, |dy| <= max(A, B) + 1 only: with c * c + s * s = 1 to
// within rounding, which pack_annotations' cos / sin give, no pixel outside it satisfies the inequality (X * X + Y * Y is dx * dx +
// dy * dy to ~1e-15 relative, the margin is a whole pixel), and the kernel skips what lies outside.
EGNE_AN_HD bool ellipse_drawn(const Ellipse& e) { return e.A > 0 && e.B > 0; }
EGNE_AN_HD int ellipse_reach(const Ellipse& e) { return (e.A > e.B ? e.A : e.B) + 1; }
EGNE_AN_HD bool in_ellipse(int x, int y, const Ellipse& e) {
  const int64_t ix = (int64_t)x - e.ex, iy = (int64_t)y - e.ey;
  const int64_t m = ellipse_reach(e);
  if (ix < -m || ix > m || iy < -m || iy > m) return false;
  const double dx = (double)ix, dy = (double)iy, A = (double)e.A, B = (double)e.B;
  const double X = dx * e.c + dy * e.s;
  const double Y = dy * e.c - dx * e.s;
  const double XB = X * B, YA = Y * A, AB = A * B;
  return XB * XB + YA * YA <= AB * AB;
}

// ---- polygon: even-odd, boundary included ---------------------------------------------------------------------------------------------
// The definition, per pixel: every edge with y0 != y1, oriented so that y0 < y1, toggles the parity of a pixel with y0 <= y < y1 and
// (x - x0) * (y1 - y0) - (x1 - x0) * (y - y0) < 0; a pixel with a zero cross product inside an edge's bounding box belongs regardless.
EGNE_AN_HD bool in_polygon(int x, int y, const int32_t* v, int n) {
  bool odd = false, on = false;
  for (int i = 0; i < n; ++i) {
    const int j = i + 1 == n ? 0 : i + 1;
    int64_t x0 = v[2 * i], y0 = v[2 * i + 1], x1 = v[2 * j], y1 = v[2 * j + 1];
    if (y0 > y1) { const int64_t tx = x0, ty = y0; x0 = x1; y0 = y1; x1 = tx; y1 = ty; }
    const int64_t cross = ((int64_t)x - x0) * (y1 - y0) - (x1 - x0) * ((int64_t)y - y0);
    if (y0 != y1 && y >= y0 && y < y1 && cross < 0) odd = !odd;
    const int64_t xl = x0 < x1 ? x0 : x1, xh = x0 < x1 ? x1 : x0;
    if (cross == 0 && y >= y0 && y <= y1 && x >= xl && x <= xh) on = true;
  }
  return odd || on;
}

// The same rule, per ROW (what the kernel runs: a lane per edge, once per row): on row y an edge toggles the pixels with x < xc
// (toggles == false: none), and the pixels bl <= x <= bh lie on it (bl > bh: none).  With dy = y1 - y0 > 0 and
// T = x0 * dy + (x1 - x0) * (y - y0) the cross product is x * dy - T: negative iff x < ceil(T / dy), zero iff dy divides T and
// x = T / dy.  A horizontal edge on its own row contributes its whole extent.
struct EdgeRow {
  int toggles, xc, bl, bh;
};
EGNE_AN_HD EdgeRow edge_row(int ax, int ay, int bx, int by, int y) {
  EdgeRow r;
  r.toggles = 0; r.xc = 0; r.bl = 0; r.bh = -1;
  int64_t x0 = ax, y0 = ay, x1 = bx, y1 = by;
  if (y0 > y1) { const int64_t tx = x0, ty = y0; x0 = x1; y0 = y1; x1 = tx; y1 = ty; }
  if (y < y0 || y > y1) return r;
  if (y0 == y1) {
    r.bl = (int)(x0 < x1 ? x0 : x1);
    r.bh = (int)(x0 < x1 ? x1 : x0);
    return r;
  }
  const int64_t dy = y1 - y0, T = x0 * dy + (x1 - x0) * ((int64_t)y - y0);
  int64_t q = T / dy;
  const int64_t rem = T - q * dy;
  if (rem == 0) { r.bl = (int)q; r.bh = (int)q; }
  if (rem > 0) ++q;                 // ceil (the division truncates towards zero)
  if (y < y1) { r.toggles = 1; r.xc = (int)q; }
  return r;
}

// ---- one pixel of Masks_noSkin: zero, then ball -> 1, iris -> 2, pupil -> 3 (the definition; the kernel clips by the shapes' boxes) ----
EGNE_AN_HD int8_t noskin_at(const int32_t* rec, int x, int y) {
  const int flags = rec[0];
  int8_t v = 0;
  if ((flags & HAS_BALL) && in_circle(x, y, rec[kBallWord], rec[kBallWord + 1], rec[kBallWord + 2])) v = 1;
  if (flags & HAS_IRIS) {
    const Ellipse e = load_ellipse(rec + kIrisWord);
    if (ellipse_drawn(e) && in_ellipse(x, y, e)) v = 2;
  }
  if (flags & HAS_PUPIL) {
    const Ellipse e = load_ellipse(rec + kPupilWord);
    if (ellipse_drawn(e) && in_ellipse(x, y, e)) v = 3;
  }
  return v;
}
// the status bits the record alone decides
EGNE_AN_HD int record_status(const int32_t* rec) {
  const int flags = rec[0];
  int st = 0;
  if ((flags & HAS_IRIS) && !ellipse_drawn(load_ellipse(rec + kIrisWord))) st |= ST_IRIS_ZERO_AXIS;
  if ((flags & HAS_PUPIL) && !ellipse_drawn(load_ellipse(rec + kPupilWord))) st |= ST_PUPIL_ZERO_AXIS;
  return st;
}

}  // namespace egne_annot
