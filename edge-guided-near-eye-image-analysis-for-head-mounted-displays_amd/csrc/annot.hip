// Label maps from TEyeD annotations (egne_amd.dataprep.labels_from_annotations): what the reference's
// dataset_generation/Extract_TEyeD_*_histo.py scripts draw per kept frame -- the eyeball circle, the iris and pupil ellipses, and the
// eyelid polygon that cuts Masks out of Masks_noSkin -- for a batch of packed records (csrc/annot_core.h), int8 maps out.
//
// The floor is the write: 1-2 bytes per pixel.  A workgroup owns kTileRows rows of ONE frame: it loads the frame's record into LDS
// once; for the polygon every wave turns its rows' edges into crossings (a lane per edge, one 64-bit division per edge that meets the
// row) and compacts them, so that a pixel only meets the two to four edges its row crosses; the pixel pass then hands every lane 16
// pixels of a row, tests the shapes whose boxes meet them, and stores 16 bytes per map where the rows are 16-byte aligned.  The lid
// is only asked where a pixel carries a class.  No synchronisation with the host, no float atomics: the only atomic is an integer
// atomicOr on the frame's status word, so the three launches are fit for graph capture.  Compiled without FMA contraction (Makefile).
#include "common.h"
#include "annot_core.h"

namespace an = egne_annot;

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64, kTileRows = 16, kChunk = 16;
constexpr int kPainted = 1 << 30;         // between paint_k and finish_k only: some pixel of the frame carries a class

struct Args {
  const int32_t* rec;
  const int* src_hw;
  int B, R, C, vec;
  int8_t* noskin;
  int8_t* skin;
  int* status;
};

__global__ __launch_bounds__(kThreads) void annot_init_k(Args a) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b < a.B) a.status[b] = an::record_status(a.rec + (long long)b * an::kRecordWords);
}

__global__ __launch_bounds__(kThreads) void annot_finish_k(Args a) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= a.B) return;
  const int s = a.status[b];
  a.status[b] = (s & kPainted) ? (s & ~kPainted) : (s | (int)an::ST_EMPTY);
}

__device__ __forceinline__ int clamp0(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// 16 pixels (x0 .. x0 + 15) of one map row: one 16-byte store where the rows allow it, bytes below C otherwise
__device__ __forceinline__ void store_chunk(int8_t* row, int x0, int C, int vec, const unsigned (&w)[4]) {
  if (vec) {
    *reinterpret_cast<uint4*>(row + x0) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int k = 0; k < kChunk; ++k)
      if (x0 + k < C) row[x0 + k] = (int8_t)((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
  }
}

// does the square of half-width m about (cx, cy) meet the pixels (x0 .. xe - 1, y)?  (64-bit: a record may hold any int32)
__device__ __forceinline__ bool box_meets(int cx, int cy, int m, int x0, int xe, int y) {
  const long long lo = (long long)cx - m, hi = (long long)cx + m;
  return m >= 0 && y >= (long long)cy - m && y <= (long long)cy + m && xe - 1 >= lo && x0 <= hi;
}

__global__ __launch_bounds__(kThreads) void annot_paint_k(Args a) {
  __shared__ __attribute__((aligned(16))) int32_t rec[an::kRecordWords + 2];
  __shared__ int s_xc[kTileRows][an::kMaxVerts], s_bl[kTileRows][an::kMaxVerts], s_bh[kTileRows][an::kMaxVerts];
  __shared__ int s_nt[kTileRows], s_nb[kTileRows];
  const int b = blockIdx.y, y0 = blockIdx.x * kTileRows;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < an::kRecordWords; i += kThreads) rec[i] = a.rec[(long long)b * an::kRecordWords + i];
  // the frame's own rows and columns: pixels at or beyond them stay 0 (the RawBatch layout)
  const int r = a.src_hw ? clamp0(a.src_hw[2 * b], a.R) : a.R;
  const int c = a.src_hw ? clamp0(a.src_hw[2 * b + 1], a.C) : a.C;
  __syncthreads();
  const int flags = rec[0];
  const int n = an::lid_count(rec);
  const bool lid = a.skin != nullptr && (flags & an::HAS_LID);
  if (lid) {                                  // (uniform over the workgroup)
    for (int rr = wave; rr < kTileRows; rr += kWaves) {
      const int y = y0 + rr;
      an::EdgeRow e;
      e.toggles = 0; e.xc = 0; e.bl = 0; e.bh = -1;
      if (lane < n && y < r) {
        const int j = lane + 1 == n ? 0 : lane + 1;
        e = an::edge_row(rec[an::kLidWord + 2 * lane], rec[an::kLidWord + 2 * lane + 1], rec[an::kLidWord + 2 * j],
                         rec[an::kLidWord + 2 * j + 1], y);
      }
      const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
      const unsigned long long mt = __ballot(e.toggles != 0), mb = __ballot(e.bl <= e.bh);
      if (e.toggles) s_xc[rr][__popcll(mt & below)] = e.xc;
      if (e.bl <= e.bh) {
        const int p = __popcll(mb & below);
        s_bl[rr][p] = e.bl;
        s_bh[rr][p] = e.bh;
      }
      if (lane == 0) { s_nt[rr] = __popcll(mt); s_nb[rr] = __popcll(mb); }
    }
    __syncthreads();
  }
  const an::Ellipse iris = an::load_ellipse(rec + an::kIrisWord), pupil = an::load_ellipse(rec + an::kPupilWord);
  const int bx = rec[an::kBallWord], by = rec[an::kBallWord + 1], br = rec[an::kBallWord + 2];
  const bool has_ball = (flags & an::HAS_BALL) != 0;
  const bool has_iris = (flags & an::HAS_IRIS) && an::ellipse_drawn(iris);
  const bool has_pupil = (flags & an::HAS_PUPIL) && an::ellipse_drawn(pupil);
  const int cpr = (a.C + kChunk - 1) / kChunk, items = kTileRows * cpr;
  bool painted = false;
  for (int it = threadIdx.x; it < items; it += kThreads) {
    const int rr = it / cpr, x0 = (it - rr * cpr) * kChunk, y = y0 + rr;
    if (y >= a.R) break;                      // (rr grows with it)
    int8_t v[kChunk];
#pragma unroll
    for (int k = 0; k < kChunk; ++k) v[k] = 0;
    bool any = false;
    if (y < r && x0 < c) {
      const int xe = x0 + kChunk < c ? x0 + kChunk : c;
      if (has_ball && box_meets(bx, by, br, x0, xe, y)) {
#pragma unroll
        for (int k = 0; k < kChunk; ++k)
          if (x0 + k < xe && an::in_circle(x0 + k, y, bx, by, br)) v[k] = 1;
      }
      if (has_iris && box_meets(iris.ex, iris.ey, an::ellipse_reach(iris), x0, xe, y)) {
#pragma unroll
        for (int k = 0; k < kChunk; ++k)
          if (x0 + k < xe && an::in_ellipse(x0 + k, y, iris)) v[k] = 2;
      }
      if (has_pupil && box_meets(pupil.ex, pupil.ey, an::ellipse_reach(pupil), x0, xe, y)) {
#pragma unroll
        for (int k = 0; k < kChunk; ++k)
          if (x0 + k < xe && an::in_ellipse(x0 + k, y, pupil)) v[k] = 3;
      }
#pragma unroll
      for (int k = 0; k < kChunk; ++k) any = any || v[k] != 0;
    }
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < kChunk; ++k) w[k >> 2] |= (unsigned)(uint8_t)v[k] << (8 * (k & 3));
    const long long row = ((long long)b * a.R + y) * a.C;
    store_chunk(a.noskin + row, x0, a.C, a.vec, w);
    painted = painted || any;
    if (a.skin) {
      if (lid && any) {                       // Masks: the same map where the lid polygon holds, else 0
        const int nt = s_nt[rr], nb = s_nb[rr];
#pragma unroll
        for (int k = 0; k < kChunk; ++k) {
          if (v[k] == 0) continue;
          const int x = x0 + k;
          bool hold = false;
          for (int t = 0; t < nt; ++t) hold ^= x < s_xc[rr][t];
          for (int t = 0; t < nb; ++t) hold = hold || (x >= s_bl[rr][t] && x <= s_bh[rr][t]);
          if (!hold) w[k >> 2] &= ~(0xffu << (8 * (k & 3)));
        }
      }
      store_chunk(a.skin + row, x0, a.C, a.vec, w);
    }
  }
  if (__ballot(painted) && lane == 0) atomicOr(a.status + b, kPainted);
}

}  // namespace

extern "C" int egne_labels_from_annotations(const void* records, const int* src_hw, int B, int R, int C, int8_t* noskin, int8_t* skin,
                                            int* status, void* stream) {
  EGNE_REQUIRE(records && noskin && status, "egne_labels_from_annotations: null pointer");
  EGNE_REQUIRE(B > 0 && B <= 65535, "egne_labels_from_annotations: 1 .. 65535 frames per call (got %d)", B);
  EGNE_REQUIRE(R > 0 && C > 0 && R <= an::kMaxCoord && C <= an::kMaxCoord, "egne_labels_from_annotations: canvas of 1 .. 2^20 rows and columns (got %d x %d)", R, C);
  EGNE_REQUIRE((uintptr_t)records % 8 == 0 && (uintptr_t)src_hw % 4 == 0 && (uintptr_t)status % 4 == 0,
               "egne_labels_from_annotations: misaligned pointer");
  EGNE_REQUIRE(noskin != skin, "egne_labels_from_annotations: the two maps must not share a buffer");
  hipStream_t st = (hipStream_t)stream;
  Args a;
  a.rec = (const int32_t*)records; a.src_hw = src_hw; a.B = B; a.R = R; a.C = C;
  a.noskin = noskin; a.skin = skin; a.status = status;
  a.vec = C % kChunk == 0 && (uintptr_t)noskin % 16 == 0 && (uintptr_t)skin % 16 == 0;
  const int fb = egne::cdiv(B, kThreads);
  annot_init_k<<<fb, kThreads, 0, st>>>(a);
  annot_paint_k<<<dim3(egne::cdiv(R, kTileRows), B), kThreads, 0, st>>>(a);
  annot_finish_k<<<fb, kThreads, 0, st>>>(a);
  return egne::check_launch("egne_labels_from_annotations");
}
