// Device-side Motion-JPEG decoder of evaluate.py (--device_decode 1): the entropy-coded scans of N baseline JPEG files (ITU-T T.81,
// 8 bit, one scan; grey, 4:4:4, 4:2:2 or 4:2:0) in HBM -> uint8 grey frames [N,H,W], byte for byte what libjpeg-turbo's default decode
// path followed by PIL's convert('L') gives (definition: include/egne_hip.h; restatement: tests/jpeg_decode_refs.py).
// The host only parses the marker segments.  Integer arithmetic throughout; no float appears in this file.
//
// egne_jpeg_decode:  unstuff_k -> [sync_k] -> final_k -> dc_k -> idct_k -> grey_k
//   unstuff_k  one workgroup per frame: checks the descriptor, drops the byte behind every 0xFF (the stuffed 0x00, or the m of an RSTm,
//              whose 0xFF goes too) by a prefix-sum compaction, records where every restart interval (segment) starts, cuts the segments
//              into subsequences of sub_bits bits and lists them.
//   sync_k     (mode 1) one workgroup per frame, a window of 256 subsequences at a time, left to right: every lane decodes its
//              subsequence from a guessed entry state, then, round by round, again from the exit state its left neighbour holds, if
//              that differs from the entry it used last; a lane writes nothing but its own slot.  The first lane of a segment (and
//              of a window: it enters with the settled exit of the window before) is right by construction, so after r rounds the
//              first r + 1 lanes are, and a round in which no entry changed ends the window: what stands then IS the sequential
//              decode, not an approximation of it.  A scan over the blocks completed gives every subsequence its first block.
//   final_k    one lane per subsequence (mode 0: per segment, from its known start state): decodes once more from the settled entry
//              state and writes DC differences and AC coefficients; the only kernel that raises a frame's flag.
//   dc_k       one workgroup per frame: prefix sums of the DC differences per component, restarting at every segment.
//   idct_k     eight lanes per block: dequantise, jidctint "islow" columns then rows, clip(x + 128) into padded component planes.
//   grey_k     one lane per pixel: fancy chroma upsampling (h2v2 / h2v1) of the planes cropped to the image, YCbCr -> RGB -> L.
// No workgroup ever waits for another one: __syncthreads is the only wait in this file.
#include "common.h"
#include "jpeg_decode_core.h"

namespace {

constexpr int WG = 256;

// natural index (row * 8 + column) -> zigzag position, T.81 figure A.6
__device__ const unsigned char kZigzagOf[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                                41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                                46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// per-frame words in the workspace
enum { M_BAD = 0, M_ULEN = 1, M_NMARK = 2, M_NSUB = 3, M_NSEG = 4, M_WORDS = 8 };

struct Layout {        // the workspace of one call; every array 16-byte aligned
  long long ub, meta, seg_start, sub_base, sub_seg, state, prefix, coef, mcu_sum, planes, total;
  long long sub_cap, plane_bytes, ypitch, cpitch, yrows, crows;
  int nseg_cap;
};

inline long long up16(long long v) { return (v + 15) / 16 * 16; }

Layout layout(int N, int H, int W, int sampling, long long stream_bytes, int sub_bits, bool own_coef) {
  const jd::Geom g = jd::geometry(H, W, sampling);
  Layout L;
  L.nseg_cap = g.nmcu + 1;
  // frame n lists its subsequences from (scan_off * 8) / sub_bits + n * nseg_cap on: at most scan_len * 8 / sub_bits + its segments
  L.sub_cap = stream_bytes * 8 / sub_bits + (long long)N * L.nseg_cap + 1;
  L.ypitch = (long long)g.mw * g.hs * 8;
  L.yrows = (long long)g.mh * g.vs * 8;
  L.cpitch = sampling == jd::GREY ? 0 : (long long)g.mw * 8;
  L.crows = sampling == jd::GREY ? 0 : (long long)g.mh * 8;
  L.plane_bytes = up16(L.ypitch * L.yrows + 2 * L.cpitch * L.crows);
  long long at = 0;
  auto take = [&](long long bytes) { const long long o = at; at += up16(bytes); return o; };
  L.ub = take(stream_bytes + 8);
  L.meta = take((long long)N * M_WORDS * 4);
  L.seg_start = take((long long)N * (L.nseg_cap + 1) * 4);
  L.sub_base = take((long long)N * (L.nseg_cap + 1) * 4);
  L.sub_seg = take(L.sub_cap * 4);
  L.state = take(L.sub_cap * 8);
  L.prefix = take((L.sub_cap + 1) * 4);
  L.coef = take(own_coef ? (long long)N * g.nmcu * g.bpm * 128 : 0);
  L.mcu_sum = take((long long)N * g.nmcu * 3 * 4);
  L.planes = take((long long)N * L.plane_bytes);
  L.total = at;
  return L;
}

// exclusive scan of v over the workgroup's 256 lanes; *total = the sum.  Two barriers; `tmp` holds 4 words
__device__ __forceinline__ long long block_scan_excl(long long v, long long* tmp, long long* total) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  long long incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long u = __shfl_up(incl, d, 64);
    if (lane >= d) incl += u;
  }
  __syncthreads();
  if (lane == 63) tmp[wave] = incl;
  __syncthreads();
  long long before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { before += k < wave ? tmp[k] : 0; all += tmp[k]; }
  *total = all;
  return before + incl - v;
}

struct FrameDesc {
  const int* w;
  const uint8_t* qt;
  const uint8_t* huff;
};
__device__ __forceinline__ FrameDesc frame_desc(const uint8_t* desc, int n) {
  const uint8_t* d = desc + (long long)n * jd::DESC_BYTES;
  return FrameDesc{reinterpret_cast<const int*>(d), d + jd::DESC_QT, d + jd::DESC_HUFF};
}

__device__ __forceinline__ unsigned table_select(const int* w) {      // bit 2c = DC table, bit 2c+1 = AC table of component c
  unsigned s = 0;
  for (int c = 0; c < 3; ++c) s |= (unsigned)((w[jd::D_TD] >> (8 * c)) & 1) << (2 * c) | (unsigned)((w[jd::D_TA] >> (8 * c)) & 1) << (2 * c + 1);
  return s;
}

__device__ __forceinline__ void build_tables(jd::Tables& T, const uint8_t* huff, int t, int nthreads) {
  if (t < 4) jd::build_limits(T, t, huff + t * jd::HUFF_BYTES);
  __syncthreads();
  for (int i = t; i < 1024; i += nthreads) jd::build_entry(T, i >> 8, i & 255, huff + (i >> 8) * jd::HUFF_BYTES);
  __syncthreads();
}

// blocks the segment `seg` must hold
__device__ __forceinline__ int seg_blocks(int seg, int ri, int nmcu, int bpm) {
  return ri > 0 ? (min(ri, nmcu - seg * ri)) * bpm : nmcu * bpm;
}

// grid (N), 256 threads
__global__ __launch_bounds__(WG) void unstuff_k(const uint8_t* __restrict__ streams, long long stream_bytes, const uint8_t* __restrict__ desc,
                                                int nmcu, int sub_bits, int mode, long long sub_cap, int nseg_cap, uint8_t* __restrict__ ub,
                                                int* __restrict__ meta, int* __restrict__ seg_start, int* __restrict__ sub_base,
                                                int* __restrict__ sub_seg, int* __restrict__ flags, int* __restrict__ stats) {
  __shared__ long long tmp[4];
  const int t = threadIdx.x, n = blockIdx.x;
  const FrameDesc fd = frame_desc(desc, n);
  const long long off = fd.w[jd::D_SCAN_OFF], len = fd.w[jd::D_SCAN_LEN];
  const int ri = fd.w[jd::D_RESTART];
  int* m = meta + (long long)n * M_WORDS;
  int* ss = seg_start + (long long)n * (nseg_cap + 1);
  int* sb = sub_base + (long long)n * (nseg_cap + 1);
  const bool bad = off < 0 || (off & 3) || len < 0 || off + len > stream_bytes || len > (1 << 27) || ri < 0 || ri > 65535;
  const int nseg = bad ? 0 : (ri > 0 ? (nmcu + ri - 1) / ri : 1);       // <= nmcu < nseg_cap
  if (t == 0) {
    flags[n] = bad ? 1 : 0;
    if (stats) { stats[2 * n] = 0; stats[2 * n + 1] = 0; }
  }
  if (bad) {
    if (t == 0) { m[M_BAD] = 1; m[M_ULEN] = 0; m[M_NMARK] = 0; m[M_NSUB] = 0; m[M_NSEG] = 0; }
    return;
  }
  const uint8_t* src = streams + off;
  uint8_t* dst = ub + off;
  long long carry = 0;                                   // low word: bytes kept so far, high word: RSTm seen so far
  for (long long i0 = 0; i0 < len; i0 += WG * 4) {
    const long long i = i0 + t * 4;
    unsigned keep = 0, mark = 0, bytes = 0;
    if (i < len) {
      unsigned prev = i > 0 ? src[i - 1] : 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (i + k < len) {
          const unsigned b = src[i + k], next = i + k + 1 < len ? src[i + k + 1] : 0u;
          const bool second = prev == 0xFFu;             // the byte behind a 0xFF: stuffing or a marker's second byte
          const bool rst = !second && b == 0xFFu && next >= 0xD0u && next <= 0xD7u;
          if (!second && !rst) keep |= 1u << k;
          if (rst) mark |= 1u << k;
          bytes |= b << (8 * k);
          prev = b;
        }
      }
    }
    long long total;
    const long long mine = (long long)__popc(keep) | (long long)__popc(mark) << 32;
    const long long before = carry + block_scan_excl(mine, tmp, &total);
    int at = (int)(before & 0xffffffffLL), mk = (int)(before >> 32);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (keep >> k & 1u) dst[at++] = (uint8_t)(bytes >> (8 * k));
      if (mark >> k & 1u) {
        ++mk;
        if (mk < nseg) ss[mk] = at;                      // segment mk starts behind this marker
      }
    }
    carry += total;
  }
  const int ulen = (int)(carry & 0xffffffffLL), nmark = (int)(carry >> 32);
  if (t == 0) ss[0] = 0;
  for (int k = min(nmark, nseg - 1) + 1 + t; k <= nseg; k += WG) ss[k] = ulen;      // segments whose marker is missing are empty
  __syncthreads();
  // subsequences: segment s holds max(1, ceil(bits / sub_bits)) of them (mode 0: the segment is its own single range)
  long long run = 0;
  for (int s0 = 0; s0 < nseg; s0 += WG) {
    const int s = s0 + t;
    long long ns = 0;
    if (s < nseg) {
      const long long bits = 8LL * (ss[s + 1] - ss[s]);
      ns = mode == 0 ? 1 : max(1LL, (bits + sub_bits - 1) / sub_bits);
    }
    long long total;
    const long long before = run + block_scan_excl(ns, tmp, &total);
    if (s < nseg) sb[s] = (int)before;
    run += total;
  }
  const long long first = off * 8 / sub_bits + (long long)n * nseg_cap;
  const int nsub = (int)min(run, max(0LL, sub_cap - first));                         // (never cut: see layout())
  if (t == 0) {
    sb[nseg] = (int)run;
    m[M_BAD] = 0; m[M_ULEN] = ulen; m[M_NMARK] = nmark; m[M_NSUB] = nsub; m[M_NSEG] = nseg;
    if (stats) stats[2 * n + 1] = nsub;
  }
  __syncthreads();
  for (int g = t; g < nsub; g += WG) {                   // the segment of subsequence g: the last s with sub_base[s] <= g
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (sb[mid] <= g) lo = mid; else hi = mid - 1;
    }
    sub_seg[first + g] = lo;
  }
}

// grid (N), 256 threads
__global__ __launch_bounds__(WG) void sync_k(const uint8_t* __restrict__ desc, int nmcu, int bpm, int nlum, int sub_bits, int nseg_cap,
                                             const uint8_t* __restrict__ ub, const int* __restrict__ meta, const int* __restrict__ seg_start,
                                             const int* __restrict__ sub_base, const int* __restrict__ sub_seg, jd::State* __restrict__ state,
                                             int* __restrict__ prefix, int* __restrict__ stats) {
  __shared__ jd::Tables T;
  __shared__ jd::State exit_of[WG];
  __shared__ long long tmp[4];
  const int t = threadIdx.x, n = blockIdx.x;
  const int* m = meta + (long long)n * M_WORDS;
  if (m[M_BAD]) return;
  const FrameDesc fd = frame_desc(desc, n);
  build_tables(T, fd.huff, t, WG);
  const unsigned tsel = table_select(fd.w);
  const long long off = fd.w[jd::D_SCAN_OFF];
  const uint32_t* words = reinterpret_cast<const uint32_t*>(ub + off);
  const int ulen = m[M_ULEN], nsub = m[M_NSUB];
  const long long first = off * 8 / sub_bits + (long long)n * nseg_cap;
  const int* ss = seg_start + (long long)n * (nseg_cap + 1);
  const int* sb = sub_base + (long long)n * (nseg_cap + 1);
  jd::State carry = {0, 0};
  long long pcarry = 0;
  int deepest = 0;
  for (int w0 = 0; w0 < nsub; w0 += WG) {
    const int g = w0 + t;
    const bool valid = g < nsub;
    int i = 0, byte0 = 0, bits = 0, end_bit = 0;
    if (valid) {
      const int seg = sub_seg[first + g];
      i = g - sb[seg];
      byte0 = ss[seg];
      bits = 8 * (ss[seg + 1] - byte0);
      end_bit = (int)min((long long)bits, (long long)(i + 1) * sub_bits);
    }
    const bool fixed = !valid || i == 0 || t == 0;       // the entry state is known: start of a segment / settled by the window before
    jd::State entry = {i * sub_bits, 0};                 // the guess: a block of the MCU's first component starts at the boundary
    if (valid && i > 0 && t == 0) entry = carry;
    jd::State ex = entry;
    int done = 0;
    if (valid) jd::decode_range<false>(T, words, ulen, byte0, bits, end_bit, ex, done, tsel, bpm, nlum, nullptr, 0, 0, false);
    exit_of[t] = ex;
    __syncthreads();
    int rounds = 0;
    for (int r = 0; r < WG; ++r) {                       // after r rounds lanes 0..r are right: WG - 1 rounds at the most, plus the vote
      const jd::State left = fixed ? entry : exit_of[t - 1];
      const int changed = !jd::same(left, entry);
      __syncthreads();                                   // every lane has read its neighbour's slot
      if (changed) {
        entry = ex = left;
        jd::decode_range<false>(T, words, ulen, byte0, bits, end_bit, ex, done, tsel, bpm, nlum, nullptr, 0, 0, false);
        exit_of[t] = ex;
      }
      if (!__syncthreads_or(changed)) break;
      ++rounds;
    }
    deepest = max(deepest, rounds);
    long long total;
    const long long before = pcarry + block_scan_excl(valid ? done : 0, tmp, &total);
    if (valid) {
      state[first + g] = entry;
      prefix[first + g] = (int)before;                   // blocks completed in front of subsequence g, counted from the frame's start
    }
    pcarry += total;
    carry = exit_of[WG - 1];
    __syncthreads();                                     // before the next window overwrites the slots
  }
  if (t == 0 && stats) stats[2 * n] = deepest;
}

// grid (ceil(ranges / 64), N), 64 threads.  mode 1: one lane per subsequence; mode 0: one lane per segment
__global__ __launch_bounds__(64) void final_k(const uint8_t* __restrict__ desc, int nmcu, int bpm, int nlum, int sub_bits, int mode, int nseg_cap,
                                              const uint8_t* __restrict__ ub, const int* __restrict__ meta, const int* __restrict__ seg_start,
                                              const int* __restrict__ sub_base, const int* __restrict__ sub_seg,
                                              const jd::State* __restrict__ state, const int* __restrict__ prefix, short* __restrict__ coef,
                                              int* __restrict__ flags) {
  __shared__ jd::Tables T;
  const int t = threadIdx.x, n = blockIdx.y;
  const int* m = meta + (long long)n * M_WORDS;
  if (m[M_BAD]) return;
  const int nsub = m[M_NSUB], nseg = m[M_NSEG];
  if ((int)blockIdx.x * 64 >= nsub) return;
  const FrameDesc fd = frame_desc(desc, n);
  build_tables(T, fd.huff, t, 64);
  const int g = blockIdx.x * 64 + t;
  const int ri = fd.w[jd::D_RESTART];
  if (g == 0 && m[M_NMARK] != nseg - 1) flags[n] = 1;   // restart markers missing or in excess
  if (g >= nsub) return;
  const long long off = fd.w[jd::D_SCAN_OFF];
  const long long first = off * 8 / sub_bits + (long long)n * nseg_cap;
  const int* ss = seg_start + (long long)n * (nseg_cap + 1);
  const int* sb = sub_base + (long long)n * (nseg_cap + 1);
  const int seg = mode == 0 ? g : sub_seg[first + g];
  const int i = g - sb[seg];
  const int byte0 = ss[seg], bits = 8 * (ss[seg + 1] - byte0);
  const bool last = g + 1 == sb[seg + 1];
  const int end_bit = last ? bits : (int)min((long long)bits, (long long)(i + 1) * sub_bits);
  jd::State s = {0, 0};
  int blk = 0;
  if (i > 0) {
    s = state[first + g];
    blk = prefix[first + g] - prefix[first + sb[seg]];
  }
  const int nblk = seg_blocks(seg, ri, nmcu, bpm);
  short* c = coef + ((long long)n * nmcu + (long long)seg * ri) * bpm * 64;
  int done;
  if (jd::decode_range<true>(T, reinterpret_cast<const uint32_t*>(ub + off), m[M_ULEN], byte0, bits, end_bit, s, done, table_select(fd.w), bpm,
                             nlum, c, blk, nblk, last))
    flags[n] = 1;
}

// grid (N), 256 threads: coef[.][0] of every block from a difference to the value, predictors 0 at every segment's start
__global__ __launch_bounds__(WG) void dc_k(const uint8_t* __restrict__ desc, int nmcu, int bpm, int nlum, const int* __restrict__ meta,
                                           short* __restrict__ coef, int* __restrict__ mcu_sum) {
  __shared__ long long tmp[4];
  const int t = threadIdx.x, n = blockIdx.x;
  if (meta[(long long)n * M_WORDS + M_BAD]) return;
  const int ri = frame_desc(desc, n).w[jd::D_RESTART];
  short* c = coef + (long long)n * nmcu * bpm * 64;
  int* P = mcu_sum + (long long)n * nmcu * 3;            // inclusive prefix over the MCUs of every component's differences
  long long carry[3] = {0, 0, 0};
  for (int m0 = 0; m0 < nmcu; m0 += WG) {
    const int mc = m0 + t;
    long long v[3] = {0, 0, 0};
    if (mc < nmcu)
      for (int b = 0; b < bpm; ++b) v[b < nlum ? 0 : b - nlum + 1] += c[((long long)mc * bpm + b) * 64];
    for (int k = 0; k < 3; ++k) {
      long long total;
      const long long before = carry[k] + block_scan_excl(v[k], tmp, &total);
      if (mc < nmcu) P[mc * 3 + k] = (int)(before + v[k]);
      carry[k] += total;
    }
  }
  __syncthreads();
  for (int mc = t; mc < nmcu; mc += WG) {
    const int s0 = ri > 0 ? mc / ri * ri : 0;            // the first MCU of this MCU's segment
    int pred[3];
    for (int k = 0; k < 3; ++k) pred[k] = (mc > s0 ? P[(mc - 1) * 3 + k] : 0) - (s0 > 0 && mc > s0 ? P[(s0 - 1) * 3 + k] : 0);
    for (int b = 0; b < bpm; ++b) {
      const int k = b < nlum ? 0 : b - nlum + 1;
      short* dc = c + ((long long)mc * bpm + b) * 64;
      pred[k] += *dc;
      *dc = (short)pred[k];
    }
  }
}

// one 8-point pass of jidctint.c's jpeg_idct_islow (CONST_BITS 13): in[8] -> out[8], descaled by `shift`
__device__ __forceinline__ void idct8(const long long* in, long long* out, int shift) {
  long long z2 = in[2], z3 = in[6];
  long long z1 = (z2 + z3) * 4433;
  const long long t2 = z1 - z3 * 15137, t3 = z1 + z2 * 6270;
  const long long t0 = (in[0] + in[4]) << 13, t1 = (in[0] - in[4]) << 13;
  const long long t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  long long a0 = in[7], a1 = in[5], a2 = in[3], a3 = in[1];
  z1 = a0 + a3;
  z2 = a1 + a2;
  z3 = a0 + a2;
  long long z4 = a1 + a3;
  const long long z5 = (z3 + z4) * 9633;
  a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299;
  z1 *= -7373; z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
  const long long r = 1LL << (shift - 1);
  out[0] = (t10 + a3 + r) >> shift; out[7] = (t10 - a3 + r) >> shift;
  out[1] = (t11 + a2 + r) >> shift; out[6] = (t11 - a2 + r) >> shift;
  out[2] = (t12 + a1 + r) >> shift; out[5] = (t12 - a1 + r) >> shift;
  out[3] = (t13 + a0 + r) >> shift; out[4] = (t13 - a0 + r) >> shift;
}

// grid (ceil(blocks / 32), N), 256 threads: 8 lanes per block.  planes: Y [yrows][ypitch], then Cb, Cr [crows][cpitch] per frame
__global__ __launch_bounds__(WG) void idct_k(const uint8_t* __restrict__ desc, int nmcu, int mw, int hs, int bpm, int nlum,
                                             const int* __restrict__ meta, const short* __restrict__ coef, uint8_t* __restrict__ planes,
                                             long long plane_bytes, int ypitch, int yrows, int cpitch, int crows) {
  __shared__ int ws[32][64];
  const int t = threadIdx.x, n = blockIdx.y, local = t >> 3, j = t & 7;
  const long long nblocks = (long long)nmcu * bpm;
  if (meta[(long long)n * M_WORDS + M_BAD]) return;
  const long long B = (long long)blockIdx.x * 32 + local;
  const bool valid = B < nblocks;
  const FrameDesc fd = frame_desc(desc, n);
  int comp = 0, b = 0, mc = 0;
  if (valid) {
    mc = (int)(B / bpm);
    b = (int)(B - (long long)mc * bpm);
    comp = b < nlum ? 0 : b - nlum + 1;
    const uint8_t* q = fd.qt + 64 * ((fd.w[jd::D_TQ] >> (8 * comp)) & 3);
    const short* c = coef + ((long long)n * nblocks + B) * 64;
    long long in[8], out[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {                        // column j
      const int z = kZigzagOf[r * 8 + j];
      in[r] = (long long)c[z] * q[z];
    }
    idct8(in, out, 11);
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[local][r * 8 + j] = (int)out[r];
  }
  __syncthreads();
  if (valid) {
    long long in[8], out[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) in[k] = ws[local][j * 8 + k];      // row j
    idct8(in, out, 18);
    const int my = mc / mw, mx = mc - my * mw;
    uint8_t* p = planes + (long long)n * plane_bytes;
    long long at;
    if (comp == 0) at = ((long long)(my * (nlum / hs) + b / hs) * 8 + j) * ypitch + (mx * hs + b % hs) * 8;
    else at = (long long)ypitch * yrows + (long long)(comp - 1) * cpitch * crows + ((long long)my * 8 + j) * cpitch + mx * 8;
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lo |= (unsigned)min(max(out[k] + 128, 0LL), 255LL) << (8 * k);
      hi |= (unsigned)min(max(out[k + 4] + 128, 0LL), 255LL) << (8 * k);
    }
    *reinterpret_cast<uint2*>(p + at) = make_uint2(lo, hi);       // 8-byte aligned: pitches and plane sizes are multiples of 8
  }
}

__device__ __forceinline__ int clip255(int v) { return min(max(v, 0), 255); }

// grid (ceil(H*W / 256), N), 256 threads
__global__ __launch_bounds__(WG) void grey_k(int H, int W, int sampling, const int* __restrict__ meta, const uint8_t* __restrict__ planes,
                                             long long plane_bytes, int ypitch, int yrows, int cpitch, int crows, uint8_t* __restrict__ out) {
  const int n = blockIdx.y;
  const long long idx = (long long)blockIdx.x * WG + threadIdx.x;
  if (idx >= (long long)H * W || meta[(long long)n * M_WORDS + M_BAD]) return;
  const int y = (int)(idx / W), x = (int)(idx - (long long)y * W);
  const uint8_t* p = planes + (long long)n * plane_bytes;
  const int Y = p[(long long)y * ypitch + x];
  int L = Y;
  if (sampling != jd::GREY) {
    int c[2];
    for (int k = 0; k < 2; ++k) {
      const uint8_t* q = p + (long long)ypitch * yrows + (long long)k * cpitch * crows;
      if (sampling == jd::S444) {
        c[k] = q[(long long)y * cpitch + x];
      } else {
        const int cw = (W + 1) >> 1, i = x >> 1, nb = (x & 1) ? min(i + 1, cw - 1) : max(i - 1, 0);    // the plane cropped to the image
        if (sampling == jd::S422) {
          const uint8_t* row = q + (long long)y * cpitch;
          c[k] = (3 * row[i] + row[nb] + ((x & 1) ? 2 : 1)) >> 2;
        } else {
          const int ch = (H + 1) >> 1, r = y >> 1, rn = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
          const uint8_t *near = q + (long long)r * cpitch, *far = q + (long long)rn * cpitch;
          const int s = 3 * near[i] + far[i], sn = 3 * near[nb] + far[nb];
          c[k] = (3 * s + sn + ((x & 1) ? 7 : 8)) >> 4;
        }
      }
    }
    const int cb = c[0] - 128, cr = c[1] - 128;
    const int R = clip255(Y + ((91881 * cr + 32768) >> 16));
    const int G = clip255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    const int B = clip255(Y + ((116130 * cb + 32768) >> 16));
    L = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
  }
  out[((long long)n * H + y) * W + x] = (uint8_t)L;
}

bool args_ok(int N, int H, int W, int sampling, long long stream_bytes, int sub_bits) {
  return N > 0 && N <= 65535 && H > 0 && W > 0 && H <= 65535 && W <= 65535 && sampling >= 0 && sampling <= 3 && stream_bytes > 0 &&
         stream_bytes <= (1LL << 30) && sub_bits >= 128 && sub_bits <= 4096 && sub_bits % 32 == 0;
}

}  // namespace

extern "C" int64_t egne_jpeg_decode_workspace_bytes(int N, int H, int W, int sampling, int64_t stream_bytes, int sub_bits, int own_coef) {
  if (!args_ok(N, H, W, sampling, stream_bytes, sub_bits)) return 16;
  return layout(N, H, W, sampling, stream_bytes, sub_bits, own_coef != 0).total;
}

extern "C" int egne_jpeg_decode(const uint8_t* streams, int64_t stream_bytes, const uint8_t* desc, int N, int H, int W, int sampling,
                                int sub_bits, int mode, uint8_t* grey_out, int16_t* coef_out, int32_t* flags, int32_t* stats, void* ws,
                                void* stream) {
  EGNE_REQUIRE(N > 0 && H > 0 && W > 0 && N <= 65535 && H <= 65535 && W <= 65535, "jpeg_decode: bad shape (N %d, frames %dx%d)", N, H, W);
  EGNE_REQUIRE(sampling >= 0 && sampling <= 3, "jpeg_decode: sampling %d is none of 0 (grey), 1 (4:4:4), 2 (4:2:2), 3 (4:2:0)", sampling);
  EGNE_REQUIRE(sub_bits >= 128 && sub_bits <= 4096 && sub_bits % 32 == 0, "jpeg_decode: sub_bits %d is no multiple of 32 in 128..4096", sub_bits);
  EGNE_REQUIRE(mode == 0 || mode == 1, "jpeg_decode: mode %d is neither 0 (one lane per segment) nor 1 (self-synchronising)", mode);
  EGNE_REQUIRE(streams && desc, "jpeg_decode: a table is missing (streams %p, descriptor table %p)", (const void*)streams, (const void*)desc);
  EGNE_REQUIRE(grey_out && flags && ws, "jpeg_decode: null output, flags or workspace");
  EGNE_REQUIRE(stream_bytes > 0 && stream_bytes <= (1LL << 30) && stream_bytes % 4 == 0, "jpeg_decode: stream_bytes %lld is no multiple of 4 in 4..2^30",
               (long long)stream_bytes);
  EGNE_REQUIRE((((uintptr_t)ws) & 15) == 0 && (((uintptr_t)streams) & 3) == 0 && (((uintptr_t)desc) & 3) == 0,
               "jpeg_decode: the workspace must be 16-byte aligned, streams and descriptors 4-byte aligned");
  const jd::Geom g = jd::geometry(H, W, sampling);
  EGNE_REQUIRE((long long)g.nmcu * g.bpm <= (1 << 24), "jpeg_decode: frames of %dx%d have too many blocks", H, W);
  hipStream_t st = (hipStream_t)stream;
  const Layout L = layout(N, H, W, sampling, stream_bytes, sub_bits, coef_out == nullptr);
  char* w = (char*)ws;
  uint8_t* ub = (uint8_t*)(w + L.ub);
  int *meta = (int*)(w + L.meta), *seg_start = (int*)(w + L.seg_start), *sub_base = (int*)(w + L.sub_base), *sub_seg = (int*)(w + L.sub_seg);
  jd::State* state = (jd::State*)(w + L.state);
  int *prefix = (int*)(w + L.prefix), *mcu_sum = (int*)(w + L.mcu_sum);
  short* coef = coef_out ? coef_out : (short*)(w + L.coef);
  uint8_t* planes = (uint8_t*)(w + L.planes);
  const long long nblocks = (long long)g.nmcu * g.bpm;
  if (hipMemsetAsync(coef, 0, (size_t)N * nblocks * 128, st) != hipSuccess) return egne::check_launch("egne_jpeg_decode (memset)");
  hipLaunchKernelGGL(unstuff_k, dim3(N), dim3(WG), 0, st, streams, (long long)stream_bytes, desc, g.nmcu, sub_bits, mode, L.sub_cap, L.nseg_cap,
                     ub, meta, seg_start, sub_base, sub_seg, flags, stats);
  if (mode == 1)
    hipLaunchKernelGGL(sync_k, dim3(N), dim3(WG), 0, st, desc, g.nmcu, g.bpm, g.nlum, sub_bits, L.nseg_cap, ub, meta, seg_start, sub_base, sub_seg,
                       state, prefix, stats);
  // ranges of a frame: at most its scan's bits / sub_bits plus its segments (mode 0: its segments)
  const long long ranges = mode == 0 ? g.nmcu : stream_bytes * 8 / sub_bits + g.nmcu + 1;
  hipLaunchKernelGGL(final_k, dim3(egne::cdiv(ranges, 64), N), dim3(64), 0, st, desc, g.nmcu, g.bpm, g.nlum, sub_bits, mode, L.nseg_cap, ub, meta,
                     seg_start, sub_base, sub_seg, state, prefix, coef, flags);
  hipLaunchKernelGGL(dc_k, dim3(N), dim3(WG), 0, st, desc, g.nmcu, g.bpm, g.nlum, meta, coef, mcu_sum);
  hipLaunchKernelGGL(idct_k, dim3(egne::cdiv(nblocks, 32), N), dim3(WG), 0, st, desc, g.nmcu, g.mw, g.hs, g.bpm, g.nlum, meta, coef, planes,
                     L.plane_bytes, (int)L.ypitch, (int)L.yrows, (int)L.cpitch, (int)L.crows);
  hipLaunchKernelGGL(grey_k, dim3(egne::cdiv((long long)H * W, WG), N), dim3(WG), 0, st, H, W, sampling, meta, planes, L.plane_bytes, (int)L.ypitch,
                     (int)L.yrows, (int)L.cpitch, (int)L.crows, grey_out);
  return egne::check_launch("egne_jpeg_decode");
}
