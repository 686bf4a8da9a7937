// Ellipses from class-map boundaries: the reference's ElliFit (helperfunctions.py:209-276) under its RANSAC loop (:278-310) on the
// device, per (frame, region) row.  The arithmetic is in ellifit_core.h (shared with a host program); DESIGN.md 6h has the contract.
//
// Five launches; the launch boundary is the only synchronisation between workgroups:
//   ef_pack_k    a wave's ballot of "boundary point" -> one 64-bit word per 64 columns
//   ef_scan_k    one workgroup per row: exclusive prefix of the words' popcounts (raster order), N
//   ef_emit_k    every set bit writes its (x, y) at prefix + rank: the point list, row-major, capped at max_pts
//   ef_ransac_k  one workgroup (four waves) per row, points in LDS.  Job 0 is the all-points fit (candidate -1), job 1 + i is
//                iteration i; wave w runs jobs w, w + 4, ...  A job is evaluated on its own (the reference's loop depends on the
//                order of its iterations only through "smallest error, earliest iteration"), each wave keeps its best by
//                (error, iteration), wave 0 picks among the four and adds verify.
//   ef_final_k   one thread per row: the outputs, the search-convention form, the status bits
// Every loop is bounded by max_pts, iters or a constant; nothing allocates or synchronises.
#include "common.h"
#include "ellifit_core.h"

namespace {

typedef unsigned long long u64;

struct EfRow {
  int* hdr;        // 0: N (all boundary points, may exceed max_pts)
  u64* bits;
  int* offs;
  unsigned* pts;   // x | y << 16
};

__device__ __forceinline__ EfRow ef_row(char* ws, int i, const EfLayout& l) {
  char* p = ws + (size_t)i * l.row_bytes;
  EfRow r;
  r.hdr = (int*)p;
  r.bits = (u64*)(p + l.off_bits);
  r.offs = (int*)(p + l.off_offs);
  r.pts = (unsigned*)(p + l.off_pts);
  return r;
}

__device__ __forceinline__ bool has_bit(unsigned bits, long long k) { return k >= 0 && k < 32 && ((bits >> (int)k) & 1u); }

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// samp[] is written by some lanes and read by all of the same wave: order the LDS accesses, keep the compiler from moving them
__device__ __forceinline__ void ef_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// which (row, image row, word) this wave works on; false past the end.  bpr = workgroups (four waves = four words) per row
__device__ __forceinline__ bool locate(int H, int wpr, int bpr, int& i, int& y, int& c) {
  i = blockIdx.x / bpr;
  const int word = (blockIdx.x % bpr) * 4 + (threadIdx.x >> 6);
  y = word / wpr;
  c = word % wpr;
  return word < H * wpr;
}

__global__ __launch_bounds__(256) void ef_pack_k(const long long* __restrict__ mask, int nframes, const int* __restrict__ frame_of,
                                                 const int* __restrict__ class_bits, const int* __restrict__ exclude_bits, int H, int W,
                                                 int bpr, EfLayout lay, char* ws, int* status) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *status = 0;      // (the later launches only ever OR into it)
  int i, y, c;
  if (!locate(H, (int)lay.wpr, bpr, i, y, c)) return;
  const int l = threadIdx.x & 63, x = c * 64 + l;
  const EfRow r = ef_row(ws, i, lay);
  const int fr = frame_of[i];
  const unsigned cb = (unsigned)class_bits[i], eb = (unsigned)exclude_bits[i];
  bool pt = false;
  if (fr >= 0 && fr < nframes && cb != 0u && x < W) {        // a frame the mask tensor does not hold: read nothing
    const long long* m = mask + (size_t)fr * H * W;
    if (has_bit(cb, m[(size_t)y * W + x])) {
      bool edge = false, excl = false;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int yy = y + dy, xx = x + dx;
          if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;      // the frame edge contributes nothing
          const long long k = m[(size_t)yy * W + xx];
          excl = excl || has_bit(eb, k);
          if ((dx == 0) != (dy == 0)) edge = edge || !has_bit(cb, k);
        }
      }
      pt = edge && !excl;
    }
  }
  const u64 w = __ballot(pt);
  if (l == 0) r.bits[(size_t)y * lay.wpr + c] = w;
}

__global__ __launch_bounds__(256) void ef_scan_k(EfLayout lay, char* ws) {
  __shared__ int part[256];
  const EfRow r = ef_row(ws, blockIdx.x, lay);
  const int nwords = (int)lay.nwords, per = (nwords + 255) / 256;      // per <= 64
  const int t = threadIdx.x, w0 = t * per, w1 = min(w0 + per, nwords);
  int sum = 0;
  for (int w = w0; w < w1; ++w) sum += __popcll(r.bits[w]);
  part[t] = sum;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {                                   // inclusive scan, 8 steps
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - sum;
  for (int w = w0; w < w1; ++w) {
    r.offs[w] = run;
    run += __popcll(r.bits[w]);
  }
  if (t == 255) r.hdr[0] = part[255];
}

__global__ __launch_bounds__(256) void ef_emit_k(int H, int bpr, int max_pts, EfLayout lay, char* ws, short* __restrict__ points_out) {
  int i, y, c;
  if (!locate(H, (int)lay.wpr, bpr, i, y, c)) return;
  const int l = threadIdx.x & 63;
  const EfRow r = ef_row(ws, i, lay);
  const size_t word = (size_t)y * lay.wpr + c;
  const u64 w = r.bits[word];
  if (!((w >> l) & 1ull)) return;
  const int idx = r.offs[word] + __popcll(w & ((1ull << l) - 1ull));
  if (idx < 0 || idx >= max_pts) return;
  const int x = c * 64 + l;
  r.pts[idx] = (unsigned)x | ((unsigned)y << 16);
  if (points_out) {
    points_out[((size_t)i * max_pts + idx) * 2 + 0] = (short)x;
    points_out[((size_t)i * max_pts + idx) * 2 + 1] = (short)y;
  }
}

struct EfParams {
  int nframes, off_pts, H, W, max_pts, n_min, iters, n_good, generated, period;
  unsigned seed;
  double thres;
};

struct EfBest {
  double err, model[5];
  int iter, cnt;
};

// wave slot w of the result area: 0 err, 1..5 model, 6 iter, 7 cnt, 8 candidates (doubles hold the integers exactly)
// The row's result goes to its workspace header (ef_final_k writes the outputs: fewer pointers live across the job loop):
//   int 0 N, 1 best iteration, 2 |I|, 3 candidates, 4 flags (1 bad sample, 2 present);  double at byte 32: error, verify, model[5]
__global__ __launch_bounds__(256) void ef_ransac_k(EfParams P, char* __restrict__ ws_pts, size_t row_bytes,
                                                   const int* __restrict__ frame_of, const int* __restrict__ class_bits,
                                                   const int* __restrict__ draws, int* __restrict__ draws_out) {
  extern __shared__ unsigned ef_lds[];
  unsigned* pts = ef_lds;
  int* samp_all = (int*)(ef_lds + P.max_pts);
  double* slot_all = (double*)(samp_all + 4 * EF_MAX_NMIN);      // max_pts*4 + 1024 bytes: a multiple of 8 for even max_pts (see launcher)
  int* flag = (int*)(slot_all + 4 * 16);

  const int row = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, l = tid & 63;
  const unsigned* row_pts = (const unsigned*)(ws_pts + (size_t)row * row_bytes);      // ws_pts: the workspace advanced to row 0's points
  const int fr = frame_of[row];
  int* hdr = (int*)(ws_pts - P.off_pts + (size_t)row * row_bytes);
  const int Nall = hdr[0];
  const bool over = Nall > P.max_pts;
  const int N = over ? 0 : Nall;
  const bool runs = fr >= 0 && fr < P.nframes && class_bits[row] != 0 && !over && N >= 7;
  const bool loops = runs && P.iters >= 0 && N > P.n_min;
  const int K1 = P.iters + 1;                                      // iterations 0..iters

  for (int p = tid; p < N; p += 256) pts[p] = row_pts[p];
  if (tid == 0) *flag = 0;
  if (draws_out && !loops)
    for (int p = tid; p < K1 * P.n_min; p += 256) draws_out[(size_t)row * K1 * P.n_min + p] = -1;
  __syncthreads();

  int* samp = samp_all + wv * EF_MAX_NMIN;
  EfBest best;
  best.err = INFINITY; best.iter = 0x7fffffff; best.cnt = 0;
#pragma unroll
  for (int k = 0; k < 5; ++k) best.model[k] = -1.0;
  int ncand = 0;
  const int D = P.n_good > P.n_min ? P.n_good : P.n_min;
  const int jobs = !runs ? 0 : (loops ? K1 + 1 : 1);

  for (int j = wv; j < jobs; j += 4) {
    const int it = j - 1;
    const bool all = it < 0;
    EfErr pot;
    bool pot_ok = false;
    if (!all) {
      // ---- the sample: lanes 0 .. n_min-1 of samp[] ----
      bool bad = false;
      if (P.generated) {
        int have = 0;
        for (int round = 0; round < EF_DRAW_ROUNDS && have < P.n_min; ++round) {
          const int cand = ef_draw_index(ef_hash(P.seed, (unsigned)(row % P.period), (unsigned)it, (unsigned)(round * 64 + l)), N);
          bool fresh = true;
          for (int q = 0; q < have; ++q) fresh = fresh && samp[q] != cand;           // taken in an earlier round
#pragma nounroll
          for (int q = 0; q < 64; ++q) {                                              // or by an earlier attempt of this round
            const int other = __shfl(cand, q, 64);
            fresh = fresh && !(q < l && other == cand);
          }
          const u64 b = __ballot(fresh);
          const int rank = have + __popcll(b & ((1ull << l) - 1ull));
          if (fresh && rank < P.n_min) samp[rank] = cand;
          have = min(P.n_min, have + __popcll(b));
          ef_wave_sync();
        }
        bad = have < P.n_min;
      } else {
        const int* d = draws + ((size_t)row * K1 + it) * P.n_min;
        const int mine = l < P.n_min ? d[l] : -1;
        bool dup = l < P.n_min && (mine < 0 || mine >= N);
#pragma nounroll
        for (int q = 0; q < P.n_min; ++q) {
          const int other = __shfl(mine, q, 64);
          dup = dup || (l < P.n_min && q < l && other == mine);
        }
        if (l < P.n_min) samp[l] = mine;
        bad = __ballot(dup) != 0ull;
        ef_wave_sync();
      }
      if (draws_out && P.generated && l < P.n_min) draws_out[((size_t)row * K1 + it) * P.n_min + l] = bad ? -1 : samp[l];
      if (bad) {
        if (l == 0) atomicOr(flag, 1);
        continue;
      }
      // ---- potModel = Fit(sample) ----
      long long sx = 0, sy = 0;
      unsigned mine = 0u;
      if (l < P.n_min) {
        mine = pts[samp[l]];
        sx = mine & 0xffffu; sy = mine >> 16;
      }
      sx = wave_sum(sx); sy = wave_sum(sy);
      const double xm = (double)sx / (double)P.n_min, ym = (double)sy / (double)P.n_min;
      double s[EF_NMOM];
#pragma unroll
      for (int k = 0; k < EF_NMOM; ++k) s[k] = 0.0;
      if (l < P.n_min) ef_accum(s, (double)(mine & 0xffffu) - xm, (double)(mine >> 16) - ym);
#pragma unroll
      for (int k = 0; k < EF_NMOM; ++k) s[k] = wave_sum(s[k]);
      double Phi[5], model[5];
      pot_ok = P.n_min >= 7 && ef_solve(s, (double)P.n_min, Phi);
      pot_ok = pot_ok && ef_model(Phi, xm, ym, model);
      if (!pot_ok) continue;                                        // |I| = n_min <= D: no candidate
      pot = ef_err_prep(model);
    }
    // a point is in I iff it is in the sample or its residual under potModel is below T
    auto inlier = [&](int p, double x, double y) -> bool {
      if (all) return true;
      bool in = ef_err(pot, x, y) < P.thres;
      for (int q = 0; q < P.n_min; ++q) in = in || samp[q] == p;
      return in;
    };
    // ---- pass A: |I| and its integer sums ----
    long long cnt = 0, sx = 0, sy = 0;
    for (int p = l; p < N; p += 64) {
      const unsigned v = pts[p];
      const int x = v & 0xffffu, y = v >> 16;
      if (inlier(p, (double)x, (double)y)) { cnt += 1; sx += x; sy += y; }
    }
    cnt = wave_sum(cnt); sx = wave_sum(sx); sy = wave_sum(sy);
    if (!all && cnt <= D) continue;
    ncand += 1;
    // ---- pass B: betterModel = Fit(pts[I]) ----
    const double xm = (double)sx / (double)cnt, ym = (double)sy / (double)cnt;
    double s[EF_NMOM];
#pragma unroll
    for (int k = 0; k < EF_NMOM; ++k) s[k] = 0.0;
    for (int p = l; p < N; p += 64) {
      const unsigned v = pts[p];
      const double x = (double)(v & 0xffffu), y = (double)(v >> 16);
      if (inlier(p, x, y)) ef_accum(s, x - xm, y - ym);
    }
#pragma unroll
    for (int k = 0; k < EF_NMOM; ++k) s[k] = wave_sum(s[k]);
    double Phi[5], model[5];
    bool ok = ef_solve(s, (double)cnt, Phi);
    ok = ok && ef_model(Phi, xm, ym, model);
    double err = INFINITY;
    if (ok) {
      // ---- pass C: its error = mean residual over pts[I] ----
      const EfErr be = ef_err_prep(model);
      double acc = 0.0;
      for (int p = l; p < N; p += 64) {
        const unsigned v = pts[p];
        const double x = (double)(v & 0xffffu), y = (double)(v >> 16);
        if (inlier(p, x, y)) acc += ef_err(be, x, y);
      }
      err = wave_sum(acc) / (double)cnt;
      if (!(err == err)) err = INFINITY;
    }
    if (err < best.err || (err == best.err && it < best.iter)) {
      best.err = err; best.iter = it; best.cnt = (int)cnt;
#pragma unroll
      for (int k = 0; k < 5; ++k) best.model[k] = ok ? model[k] : -1.0;
    }
  }

  double* slot = slot_all + wv * 16;
  if (l == 0) {
    slot[0] = best.err;
#pragma unroll
    for (int k = 0; k < 5; ++k) slot[1 + k] = best.model[k];
    slot[6] = (double)best.iter; slot[7] = (double)best.cnt; slot[8] = (double)ncand;
  }
  __syncthreads();
  if (wv != 0) return;

  // ---- wave 0: the best of the four, verify over all points, the row's outputs ----
  int bw = 0, cands = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const double* a = slot_all + w * 16;
    const double* b = slot_all + bw * 16;
    if (a[0] < b[0] || (a[0] == b[0] && a[6] < b[6])) bw = w;
    cands += (int)a[8];
  }
  const double* b = slot_all + bw * 16;
  const bool sample_bad = *flag != 0;
  const bool present = runs && !sample_bad && b[0] < INFINITY;
  double ver = INFINITY;
  if (present) {
    const EfErr e = ef_err_prep(b + 1);
    double acc = 0.0;
    for (int p = l; p < N; p += 64) {
      const unsigned v = pts[p];
      acc += ef_verify_pt(e, (double)(v & 0xffffu), (double)(v >> 16));
    }
    ver = wave_sum(acc) / (double)N;
  }
  if (l != 0) return;
  double* hd = (double*)(hdr + 8);
  hdr[1] = present ? (int)b[6] : -1;
  hdr[2] = present ? (int)b[7] : 0;
  hdr[3] = sample_bad ? 0 : cands;
  hdr[4] = (sample_bad ? 1 : 0) | (present ? 2 : 0);
  hd[0] = present ? b[0] : INFINITY;
  hd[1] = ver;
  for (int k = 0; k < 5; ++k) hd[2 + k] = present ? b[1 + k] : -1.0;
}

__global__ void ef_final_k(int n, int H, int W, int max_pts, EfLayout lay, char* ws, const int* __restrict__ frame_of,
                           const int* __restrict__ search_cls, double* __restrict__ raw, double* __restrict__ init,
                           int* __restrict__ out_frame_of, int* __restrict__ out_cls, int* __restrict__ stats_i,
                           double* __restrict__ stats_f, int* status) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const int* hdr = ef_row(ws, row, lay).hdr;
  const double* hd = (const double*)(hdr + 8);
  if (hdr[0] > max_pts) atomicOr(status, 2);
  if (hdr[4] & 1) atomicOr(status, 1);
  const bool present = (hdr[4] & 2) != 0;
  out_cls[row] = search_cls[row];
  out_frame_of[row] = present ? frame_of[row] : -1;
  for (int k = 0; k < 4; ++k) stats_i[row * 4 + k] = hdr[k];
  stats_f[row * 2 + 0] = hd[0];
  stats_f[row * 2 + 1] = hd[1];
  double model[5], ini[5];
  for (int k = 0; k < 5; ++k) { model[k] = hd[2 + k]; ini[k] = -1.0; }
  if (present) ef_to_search(model, H, W, ini);
  for (int k = 0; k < 5; ++k) { raw[row * 5 + k] = model[k]; init[row * 5 + k] = ini[k]; }
}

}  // namespace

extern "C" int64_t egne_ellipse_ransac_workspace_bytes(int n, int H, int W, int max_pts) { return ef_workspace_bytes(n, H, W, max_pts); }

extern "C" int egne_ellipse_ransac_from_mask(const int64_t* mask, int nframes, const int32_t* frame_of, const int32_t* class_bits,
                                             const int32_t* search_cls, const int32_t* exclude_bits, int n, int H, int W, int max_pts,
                                             int n_min, int iters, double thres, int n_good, const int32_t* draws, uint32_t seed,
                                             int draw_period, int32_t* draws_out, double* raw, double* init, int32_t* out_frame_of, int32_t* out_cls,
                                             int32_t* stats_i, double* stats_f, int16_t* points_out, int32_t* status, void* ws,
                                             void* stream) {
  EGNE_REQUIRE(mask && frame_of && class_bits && search_cls && exclude_bits && raw && init && out_frame_of && out_cls && stats_i &&
                   stats_f && status && ws,
               "ellipse_ransac_from_mask: null pointer");
  EGNE_REQUIRE(n > 0 && nframes > 0, "ellipse_ransac_from_mask: bad counts");
  EGNE_REQUIRE(ef_shape_ok(H, W), "ellipse_ransac_from_mask: %dx%d masks (2..1024 rows and columns)", H, W);
  EGNE_REQUIRE(ef_pts_ok(max_pts) && max_pts % 2 == 0, "ellipse_ransac_from_mask: max_pts %d (even, 2..%d)", max_pts, EF_MAX_PTS);
  EGNE_REQUIRE(n_min >= 1 && n_min <= EF_MAX_NMIN, "ellipse_ransac_from_mask: n_min %d (1..%d)", n_min, EF_MAX_NMIN);
  EGNE_REQUIRE(iters >= -1 && iters < EF_MAX_ITERS, "ellipse_ransac_from_mask: iters %d (-1..%d)", iters, EF_MAX_ITERS - 1);
  EGNE_REQUIRE(n_good >= 0 && thres == thres && draw_period >= 1, "ellipse_ransac_from_mask: bad n_good / thres / draw_period");
  EGNE_REQUIRE(((uintptr_t)ws & 7) == 0, "ellipse_ransac_from_mask: workspace not aligned to 8 bytes");
  const EfLayout lay = ef_layout(H, W, max_pts);
  const int bpr = (int)((lay.nwords + 3) / 4);
  EGNE_REQUIRE((long long)n * bpr < (1ll << 31), "ellipse_ransac_from_mask: %d rows of %dx%d exceed one grid", n, H, W);
  const size_t lds = ef_lds_bytes(max_pts);
  EGNE_REQUIRE(lds <= 65536 || egne::raise_lds((const void*)ef_ransac_k, lds), "ellipse_ransac_from_mask: %zu bytes of LDS refused", lds);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(n * bpr)), block(256);
  char* w = (char*)ws;
  EfParams P;
  P.nframes = nframes; P.off_pts = (int)lay.off_pts; P.H = H; P.W = W; P.max_pts = max_pts; P.n_min = n_min; P.iters = iters; P.n_good = n_good;
  P.generated = draws == nullptr; P.period = draw_period; P.seed = seed; P.thres = thres;
  hipLaunchKernelGGL(ef_pack_k, grid, block, 0, st, (const long long*)mask, nframes, frame_of, class_bits, exclude_bits, H, W, bpr, lay, w,
                     status);
  hipLaunchKernelGGL(ef_scan_k, dim3((unsigned)n), block, 0, st, lay, w);
  hipLaunchKernelGGL(ef_emit_k, grid, block, 0, st, H, bpr, max_pts, lay, w, (short*)points_out);
  hipLaunchKernelGGL(ef_ransac_k, dim3((unsigned)n), block, lds, st, P, w + lay.off_pts, lay.row_bytes, frame_of, class_bits, draws, draws_out);
  hipLaunchKernelGGL(ef_final_k, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, n, H, W, max_pts, lay, w, frame_of, search_cls, raw, init,
                     out_frame_of, out_cls, stats_i, stats_f, status);
  return egne::check_launch("egne_ellipse_ransac_from_mask");
}
