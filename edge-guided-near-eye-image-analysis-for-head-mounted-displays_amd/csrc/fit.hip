// Ellipse fit of evaluate.py on the device: utils.py:450-486 (coordinate hill-climb over a, b, angle)
// with utils.py:176-204 (IoU of the class mask with a rasterised ellipse on the [-1,1] mesh) and the
// float64 conic algebra of helperfunctions.py:13-63,102-129.
//
// One wave per (frame, class).  The class mask is bit-packed into LDS once; every IoU evaluation is then a pass
// over the rows of the ellipse's bounding box (exact end points of the inside interval + a popcount), so the
// <=281 sequential evaluations of the search never leave the CU (the reference builds each map on the host,
// copies it and calls .item() three times).
//
// Numerics follow the reference bit for bit: float32 mesh supplied by the host (torch.linspace, the
// same call create_meshgrid makes), float32 map arithmetic with one rounding per operation (built with
// -ffp-contract=off and written with the _rn intrinsics), float64 conic normalisation, 3.14159.
#include "common.h"

namespace {

// the conic algebra, the membership rule, the mask packing and one IoU evaluation (evaluate_ell): shared with csrc/ellipse_scores.hip
#include "fit_core.h"

// ------------------------------------------------------------------------------------------------------------------------
// A PAIR of waves per (frame, class), two searches per workgroup.
//
// Why not a workgroup per search (rounds 1-2: 512 threads, the mask scanned word by word): the 128 searches of a 64-frame batch
// then sit on 128 CUs for 3.2 ms with ~12 KB of LDS each, and while they do, the network's persistent kernels on the other
// stream (one 100-160 KB workgroup per CU) can only be placed on the remaining CUs -- the fit stage cost the step 3.4 ms although it
// is 1.4 % of its work.  Here a batch's searches occupy 32 CUs for about a millisecond.
//
// What makes one wave enough: an evaluation no longer tests every pixel of the ellipse's bounding box.  On a row the inside set
// of the reference's float32 predicate  ((dx ct + dy st)/a)^2 + ((-dx st + dy ct)/b)^2 - 1 <= 0  is an interval; lane = row solves
// the row's quadratic for approximate end points and then walks each end with the EXACT predicate (same operations, one rounding
// each) until pixel il is inside and il - 1 is not (likewise ir): the count is ir - il + 1 and the overlap a popcount of the
// row's mask bits under the interval.  Rows whose interval is short (tangent rows, where round-off could matter over more than a
// pixel) or empty are tested pixel by pixel around it; walks that do not settle within a few steps and degenerate ellipses fall
// back to testing every pixel of the row -- so the result is the reference's bit for bit (tests/golden/fit_cases.npz,
// evaluate_real_frames.npz).
//
// The search itself is a chain of up to 281 dependent evaluations (utils.py:450-486), ~8 us each: its length is the latency of a
// one- or two-frame call.  Two things shorten the chain without changing a single result.  (1) The two candidates of a coordinate
// step, now[j] - d and (now[j] - d) + 2d, are known before either is scored: the waves of a pair score one each at the same time
// and swap the scores through LDS; the step then takes the reference's decisions in the reference's order (the evaluation counter
// counts what the reference would have evaluated).  (2) The score a sweep ends with is the score of a parameter vector that has
// usually been scored already -- nothing accepted: the vector the sweep started from; one coordinate accepted: that candidate --
// so it is looked up by exact (bitwise) comparison of the three parameters and only evaluated on a miss (the reference's
// subtract / add-twice / subtract sequence can move a rejected coordinate by a rounding, which is then a miss).
// s_barrier waits on the surviving waves only, so a pair that finishes leaves the other pair of its workgroup running.
// ------------------------------------------------------------------------------------------------------------------------
// FIT_PAIRS searches per workgroup, ROWW waves per candidate.  A whole batch: two searches of two waves (64 compute units for its 128
// searches; eight per workgroup were measured too: the lock step of 16 waves at every barrier stretches the launch from 1.85 to
// 3.0 ms and the step gains nothing).  Few searches (a one- or two-frame call, where the chain IS the latency): a workgroup of eight
// waves per search, four per candidate, so that the ~140 rows of an iris ellipse are one pass of 256 lanes instead of three of 64;
// the partial counts of the waves are integers, so their sum does not depend on the split.

// LOCAL: the waves of a search meet through LDS flags of their own instead of the workgroup barrier, so that MANY searches can share a
// workgroup without running in lock step (eight searches per workgroup: 16 of the chip's 256 compute units host the batch's 128
// searches instead of 64 -- a compute unit that hosts a search wave cannot take a workgroup of the network's persistent kernels,
// whose two 256-register waves per SIMD need the whole register file, and that workgroup's share of the tiles then waits).
template <int FIT_PAIRS, int ROWW, bool LOCAL = false>
__global__ __launch_bounds__(128 * FIT_PAIRS * ROWW) void ellipse_fit_k(const long long* __restrict__ mask, int nframes, const int* __restrict__ frame_of,
                                                                       const int* __restrict__ cls, int n, int H, int W,
                                                                       const float* __restrict__ xs, const float* __restrict__ ys,
                                                                       const double* __restrict__ init, double* __restrict__ out,
                                                                       int* __restrict__ evals) {
  // NW = 2 * ROWW waves per search: wave w scores candidate sub = w / ROWW over the rows y = y_lo + part * 64 + lane (+ 64 * ROWW ...)
  constexpr int NW = 2 * ROWW, SWAP = 2 * NW * 2;     // swap area per search: [2 parities][NW waves][ne, ni]
  extern __shared__ unsigned fit_lds[];  // xs[W], ys[H], swap areas, then per search [H][wpr] packed mask
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, pair = wave / NW, wv = wave % NW, sub = wv / ROWW, part = wv % ROWW;
  const int wpr = (W + 31) >> 5, nwords = H * wpr;
  float* lxs = (float*)fit_lds;
  float* lys = lxs + W;
  volatile unsigned* swap = fit_lds + W + H + pair * SWAP;
  volatile unsigned* flags = fit_lds + W + H + FIT_PAIRS * SWAP + pair * NW;       // LOCAL: exchange count of every wave of the search
  unsigned* bits = fit_lds + W + H + FIT_PAIRS * (SWAP + NW) + pair * nwords;
  for (int i = threadIdx.x; i < W; i += blockDim.x) lxs[i] = xs[i];
  for (int i = threadIdx.x; i < H; i += blockDim.x) lys[i] = ys[i];
  if (threadIdx.x < FIT_PAIRS * NW) fit_lds[W + H + FIT_PAIRS * SWAP + threadIdx.x] = 0u;
  __syncthreads();
  unsigned seq = 0;
  const int e = blockIdx.x * FIT_PAIRS + pair;
  if (e >= n) return;                     // (whole searches: all waves of a search take every barrier below together)
  const int fr = frame_of[e];
  if (fr < 0 || fr >= nframes) {   // a fit that names a frame the mask tensor does not hold: report NaN, read nothing
    if (wv == 0 && lane < 5) out[e * 5 + lane] = __longlong_as_double(0x7ff8000000000000ll);
    if (wv == 0 && lane == 0 && evals) evals[e] = 0;
    return;
  }
  const long long* m = mask + (long long)fr * H * W;
  const int k = cls[e];
  const unsigned cnt = pack_mask_rows(m, k, H, W, bits, wpr, lane, wv, NW);   // the waves of the search pack the rows in turn
  int parity = 0;
  // every wave leaves its two words, all meet at the barrier and read the sums per candidate (double buffered: one barrier per exchange)
  auto exchange = [&](unsigned m0, unsigned m1, unsigned* s0, unsigned* s1) {
    volatile unsigned* sw = swap + parity * NW * 2;
    if (lane == 0) { sw[wv * 2] = m0; sw[wv * 2 + 1] = m1; }
    if constexpr (LOCAL) {
      // release: this wave's words (and, the first time, its rows of the packed mask) before its count; then wait for the counts of
      // all waves of THIS search.  The areas are double buffered and a wave can run at most one exchange ahead of its partners.
      ++seq;
      __threadfence_block();
      if (lane == 0) flags[wv] = seq;
      if (lane < NW) { while (flags[lane] < seq) __builtin_amdgcn_s_sleep(2); }
      __threadfence_block();
    } else {
      __syncthreads();
    }
    s0[0] = s0[1] = s1[0] = s1[1] = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) { s0[i / ROWW] += sw[i * 2]; s1[i / ROWW] += sw[i * 2 + 1]; }
    parity ^= 1;
  };
  unsigned ca[2], cb[2];
  exchange(cnt, 0u, ca, cb);              // (the barrier also orders the mask words of all waves before the first evaluation)
  const int nseg = (int)(ca[0] + ca[1]);

  const double cx = init[e * 5 + 0], cy = init[e * 5 + 1];
  double now[3] = {init[e * 5 + 2], init[e * 5 + 3], init[e * 5 + 4] * 180. / PI_REF}, d[3] = {1.0, 1.0, 1.0};

  auto evaluate = [&](const double* q, unsigned& ne_out, unsigned& ni_out) {
    evaluate_ell<ROWW>(H, W, lxs, lys, bits, wpr, cx, cy, lane, part, q, ne_out, ni_out);
  };
  auto iou = [&](unsigned ne, unsigned ni) -> float {
    const float fi = (float)ni;
    return __fdiv_rn(fi, __fsub_rn(__fadd_rn((float)nseg, (float)ne), fi));
  };
  // one round: candidate qa on the waves with sub = 0, qb on the others (each over its share of the rows), both scores to every wave
  auto score2 = [&](const double* qa, const double* qb, float& sa, float& sb) {
    unsigned ne, ni, nes[2], nis[2];
    evaluate(sub ? qb : qa, ne, ni);
    exchange(ne, ni, nes, nis);
    sa = iou(nes[0], nis[0]); sb = iou(nes[1], nis[1]);
  };

  auto same = [](const double* a, const double* b) {
    return __double_as_longlong(a[0]) == __double_as_longlong(b[0]) && __double_as_longlong(a[1]) == __double_as_longlong(b[1]) &&
           __double_as_longlong(a[2]) == __double_as_longlong(b[2]);
  };
  int nev = 1;
  float base_sc, unused;
  score2(now, now, base_sc, unused);           // score of `now` at the start of the sweep
  double base_q[3] = {now[0], now[1], now[2]};
  double rt = (double)base_sc;
  for (int sweep = 0; sweep < 40; ++sweep) {
    int flag = 0;
    float acc_sc = 0.f;                          // the last accepted candidate and its score
    double acc_q[3] = {0., 0., 0.};
    bool have_acc = false;
    for (int j = 0; j < 3; ++j) {
      const double lo = now[j] - d[j], hi = lo + 2. * d[j];          // the reference's two candidates, in its arithmetic
      double qa[3] = {now[0], now[1], now[2]}, qb[3] = {now[0], now[1], now[2]};
      qa[j] = lo; qb[j] = hi;
      float sc_lo, sc_hi;
      score2(qa, qb, sc_lo, sc_hi);
      ++nev;
      if ((double)sc_lo > rt) {                  // (rt only changes between sweeps)
        now[j] = lo; flag = 1; have_acc = true; acc_sc = sc_lo;
        acc_q[0] = now[0]; acc_q[1] = now[1]; acc_q[2] = now[2];
        continue;
      }
      ++nev;
      if ((double)sc_hi > rt) {
        now[j] = hi; flag = 1; have_acc = true; acc_sc = sc_hi;
        acc_q[0] = now[0]; acc_q[1] = now[1]; acc_q[2] = now[2];
        continue;
      }
      now[j] = hi - d[j]; d[j] *= 0.8;
    }
    ++nev;
    float sc;
    if (same(now, base_q)) sc = base_sc;
    else if (have_acc && same(now, acc_q)) sc = acc_sc;
    else score2(now, now, sc, unused);
    if ((double)sc > rt) rt = (double)sc;
    base_sc = sc; base_q[0] = now[0]; base_q[1] = now[1]; base_q[2] = now[2];
    if (!flag) break;
  }
  if (wv == 0 && lane == 0) {
    out[e * 5 + 0] = cx; out[e * 5 + 1] = cy; out[e * 5 + 2] = now[0]; out[e * 5 + 3] = now[1];
    out[e * 5 + 4] = now[2] / 180.0 * PI_REF;
    if (evals) evals[e] = nev;
  }
}

// One evaluation per ellipse through the functions the search calls: a workgroup of ROWW waves per ellipse, wave = part.  counts[e] = (pixels
// of class cls[e] in frame frame_of[e], pixels inside the ellipse, pixels in both); ell[e] = (cx, cy, a, b) pixels, angle in degrees.
template <int ROWW>
__global__ __launch_bounds__(64 * ROWW) void ellipse_counts_k(const long long* __restrict__ mask, int nframes, const int* __restrict__ frame_of,
                                                              const int* __restrict__ cls, int H, int W, const float* __restrict__ xs,
                                                              const float* __restrict__ ys, const double* __restrict__ ell,
                                                              unsigned* __restrict__ counts) {
  extern __shared__ unsigned fit_lds[];  // xs[W], ys[H], [ROWW waves][nseg, ne, ni], [H][wpr] packed mask
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wpr = (W + 31) >> 5;
  float* lxs = (float*)fit_lds;
  float* lys = lxs + W;
  unsigned* sums = fit_lds + W + H;
  unsigned* bits = sums + 3 * ROWW;
  for (int i = threadIdx.x; i < W; i += blockDim.x) lxs[i] = xs[i];
  for (int i = threadIdx.x; i < H; i += blockDim.x) lys[i] = ys[i];
  const int e = blockIdx.x;
  const int fr = frame_of[e];
  if (fr < 0 || fr >= nframes) {   // a frame the mask tensor does not hold: all ones, read nothing (the whole workgroup leaves)
    if (threadIdx.x < 3) counts[e * 3 + threadIdx.x] = 0xffffffffu;
    return;
  }
  const unsigned cnt = pack_mask_rows(mask + (long long)fr * H * W, cls[e], H, W, bits, wpr, lane, wave, ROWW);
  __syncthreads();
  unsigned ne, ni;
  evaluate_ell<ROWW>(H, W, lxs, lys, bits, wpr, ell[e * 5 + 0], ell[e * 5 + 1], lane, wave, ell + e * 5 + 2, ne, ni);
  if (lane == 0) { sums[wave * 3] = cnt; sums[wave * 3 + 1] = ne; sums[wave * 3 + 2] = ni; }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned t = 0;
    for (int w = 0; w < ROWW; ++w) t += sums[w * 3 + threadIdx.x];
    counts[e * 3 + threadIdx.x] = t;
  }
}

// evaluate.py:135-151: the regressed ellipses (normalised [-1,1] coordinates, float32) -> pixel ellipses that seed the
// search: my_ellipse(p).transform(H)[0][:-1] with H = [[W/2,0,W/2],[0,H/2,H/2],[0,0,1]] (helperfunctions.py:25-33,
// :50-63,:124-129) in float64.  Fit 2f = iris (elPred[f,0:5], class 1), fit 2f+1 = pupil (elPred[f,5:10], class 2).
__global__ void ellipse_init_k(const float* __restrict__ elPred, int nframes, int H, int W, double* __restrict__ init,
                               int* __restrict__ frame_of, int* __restrict__ cls) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 2 * nframes) return;
  const int f = e >> 1, k = e & 1;
  double el[5];
  for (int i = 0; i < 5; ++i) el[i] = (double)elPred[f * 10 + 5 * k + i];
  norm_to_pixel(el, H, W, init + e * 5);
  frame_of[e] = f;
  cls[e] = 1 + k;
}

}  // namespace

extern "C" int egne_ellipse_init_from_pred(const float* elPred, int nframes, int H, int W, double* init, int32_t* frame_of,
                                           int32_t* cls, void* stream) {
  EGNE_REQUIRE(elPred && init && frame_of && cls && nframes > 0 && H > 1 && W > 1, "ellipse_init_from_pred: bad arguments");
  hipLaunchKernelGGL(ellipse_init_k, dim3((2 * nframes + 63) / 64), dim3(64), 0, (hipStream_t)stream, elPred, nframes, H, W, init,
                     frame_of, cls);
  return egne::check_launch("egne_ellipse_init_from_pred");
}

extern "C" int egne_ellipse_fit(const int64_t* mask, int nframes, const int32_t* frame_of, const int32_t* cls, int n, int H, int W,
                                const float* xs, const float* ys, const double* init, double* out, int32_t* evals,
                                void* stream) {
  EGNE_REQUIRE(mask && frame_of && cls && xs && ys && init && out, "ellipse_fit: null pointer");
  EGNE_REQUIRE(n > 0 && nframes > 0 && H > 1 && W > 1, "ellipse_fit: bad shape");
  const size_t per_search = ((size_t)H * ((W + 31) / 32) + 32) * 4, fixed = (size_t)(W + H) * 4;
  EGNE_REQUIRE(2 * per_search + fixed <= 64 * 1024, "ellipse_fit: %dx%d masks do not fit LDS", H, W);
  hipStream_t st = (hipStream_t)stream;
  const long long* mk = (const long long*)mask;
  static const int dense = [] { const char* e = getenv("EGNE_FIT_DENSE"); return e ? atoi(e) : 4; }();      // searches per workgroup of a large batch (2: round 3's form; 4 measured best: 32.3 vs 32.5 ms per step with the fit stage, 8 spills at 128 registers)
  if (n >= 64 && dense == 8 && 8 * per_search + fixed <= 150 * 1024) {
    // a large batch: EIGHT searches of two waves per workgroup, pair-local synchronisation (see LOCAL above)
    const size_t lds = fixed + 8 * ((size_t)H * ((W + 31) / 32) + 8 + 2) * 4;
    if (!egne::raise_lds((const void*)ellipse_fit_k<8, 1, true>, 150 * 1024)) return egne::fail(EGNE_ERR_LAUNCH, "ellipse_fit: cannot raise the dynamic LDS limit");
    hipLaunchKernelGGL((ellipse_fit_k<8, 1, true>), dim3((unsigned)((n + 7) / 8)), dim3(1024), lds, st, mk, nframes, frame_of, cls, n, H, W, xs, ys, init, out, evals);
  } else if (n >= 64 && dense == 4 && fixed + 4 * ((size_t)H * ((W + 31) / 32) + 8 + 2) * 4 <= 64 * 1024) {
    // (masks where two searches fit the default 64 KB of dynamic LDS but four do not -- 320x480, 384x512 -- take the two-search form below)
    const size_t lds = fixed + 4 * ((size_t)H * ((W + 31) / 32) + 8 + 2) * 4;
    hipLaunchKernelGGL((ellipse_fit_k<4, 1, true>), dim3((unsigned)((n + 3) / 4)), dim3(512), lds, st, mk, nframes, frame_of, cls, n, H, W, xs, ys, init, out, evals);
  } else if (n >= 16) {           // a batch: two searches of two waves per workgroup
    const size_t lds = fixed + 2 * ((size_t)H * ((W + 31) / 32) + 8 + 2) * 4;
    hipLaunchKernelGGL((ellipse_fit_k<2, 1>), dim3((unsigned)((n + 1) / 2)), dim3(256), lds, st, mk, nframes, frame_of, cls, n, H, W, xs, ys, init, out, evals);
  } else {                 // one or two frames: a workgroup of eight waves per search (the rows of an evaluation in one pass)
    const size_t lds = fixed + ((size_t)H * ((W + 31) / 32) + 32 + 8) * 4;
    hipLaunchKernelGGL((ellipse_fit_k<1, 4>), dim3((unsigned)n), dim3(512), lds, st, mk, nframes, frame_of, cls, n, H, W, xs, ys, init, out, evals);
  }
  return egne::check_launch("egne_ellipse_fit");
}

extern "C" int egne_ellipse_iou_counts(const int64_t* mask, int nframes, const int32_t* frame_of, const int32_t* cls, int n, int H, int W,
                                       const float* xs, const float* ys, const double* ell, uint32_t* counts, int roww, void* stream) {
  EGNE_REQUIRE(mask && frame_of && cls && xs && ys && ell && counts, "ellipse_iou_counts: null pointer");
  EGNE_REQUIRE(n > 0 && nframes > 0 && H > 1 && W > 1, "ellipse_iou_counts: bad shape");
  EGNE_REQUIRE(roww == 1 || roww == 4, "ellipse_iou_counts: roww must be 1 or 4, got %d", roww);
  const size_t per_search = ((size_t)H * ((W + 31) / 32) + 32) * 4, fixed = (size_t)(W + H) * 4;
  EGNE_REQUIRE(2 * per_search + fixed <= 64 * 1024, "ellipse_iou_counts: %dx%d masks do not fit LDS", H, W);
  hipStream_t st = (hipStream_t)stream;
  const long long* mk = (const long long*)mask;
  const size_t lds = fixed + per_search;            // (per_search leaves 32 words for the 3 * roww partial sums)
  if (roww == 4)
    hipLaunchKernelGGL((ellipse_counts_k<4>), dim3((unsigned)n), dim3(256), lds, st, mk, nframes, frame_of, cls, H, W, xs, ys, ell, counts);
  else
    hipLaunchKernelGGL((ellipse_counts_k<1>), dim3((unsigned)n), dim3(64), lds, st, mk, nframes, frame_of, cls, H, W, xs, ys, ell, counts);
  return egne::check_launch("egne_ellipse_iou_counts");
}
