// Device-side Motion-JPEG encoder and frame-number stamp of evaluate.py (--device_jpeg 1): uint8 BGR frames in HBM -> one complete
// baseline JPEG file (ITU-T T.81, JFIF, 4:2:0, Annex K Huffman tables, restart intervals) per frame.  The arithmetic is integer from
// the first pixel to the last bit (definition: include/egne_hip.h), so the stream is one defined byte string; it is
// pinned byte for byte against the NumPy restatement in tests/jpeg_refs.py.  No float appears in this file.
//
// egne_jpeg_encode:  dct_k -> entropy_k<false> -> layout_k -> entropy_k<true>
//   dct_k        one workgroup per 16 x 16 MCU: loads (edge-replicated), colour, 2 x 2 chroma mean, six 8 x 8 integer DCTs
//                (F = T s T^t, 32-bit first pass, 64-bit second), quantisation, int16 coefficients in zigzag order to the workspace.
//   entropy_k    one wave per restart interval, one 8 x 8 block per iteration with lane k on coefficient k: DC difference, run
//                lengths from a ballot of the non-zero lanes, code + value bits per lane (at most 3 ZRL + 26 bits = 59), a 64-lane
//                scan for the bit offsets, codes OR-ed into a zeroed LDS bit buffer (atomics on zeroed words: order-independent);
//                then 0xFF stuffing with a second scan.  The LDS buffer holds the worst case of 8 MCUs (26 bits per coefficient).
//                <false> only measures the interval's stuffed length; <true> runs the same code again and stores the bytes at
//                their final position, so no staging buffer of worst-case size exists and nothing is written unless the whole
//                file fits.
//   layout_k     one workgroup per frame: scan over the interval lengths -> interval offsets, file length or overflow flag,
//                header and EOI.
#include "common.h"

namespace {

constexpr int MAX_RESTART = 8;                       // restart_mcus the LDS staging is sized for
constexpr int BLOCK_BITS = 64 * 26;                  // worst case of one block: 16-bit code + 10 value bits per coefficient (DC: 11 + 11)
constexpr int BUF_WORDS = MAX_RESTART * 6 * BLOCK_BITS / 32 + 4;
constexpr int HUFF_WORDS = 2 * 16 + 2 * 256;

// zigzag position of the coefficient at natural index row * 8 + column (row = vertical frequency), T.81 figure A.6
__device__ const unsigned char kZigzagOf[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                                41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                                46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// grid (MCUs of a frame, N), 256 threads = the 16 x 16 pixels of the MCU.  coef int16 [N][nm][6][64]: Y00 Y01 Y10 Y11 Cb Cr, zigzag order
__global__ __launch_bounds__(256) void dct_k(const uint8_t* __restrict__ bgr, int H, int W, int mw, const uint8_t* __restrict__ qt,
                                             const int* __restrict__ dct, short* __restrict__ coef) {
  __shared__ int T[64];
  __shared__ int s[6][64];
  __shared__ int full[2][256];
  __shared__ int G[6][64];
  const int t = threadIdx.x, m = blockIdx.x, n = blockIdx.y;
  const int my = m / mw, mx = m - my * mw;
  if (t < 64) T[t] = dct[t];
  const int py = t >> 4, px = t & 15;
  const int y = min(my * 16 + py, H - 1), x = min(mx * 16 + px, W - 1);        // last row / column repeated
  const uint8_t* p = bgr + (((long long)n * H + y) * W + x) * 3;
  const int B = p[0], Gr = p[1], R = p[2];
  s[(py >> 3) * 2 + (px >> 3)][(py & 7) * 8 + (px & 7)] = ((19595 * R + 38470 * Gr + 7471 * B + 32768) >> 16) - 128;
  full[0][t] = (-11059 * R - 21709 * Gr + 32768 * B + 8388608 + 32767) >> 16;
  full[1][t] = (32768 * R - 27439 * Gr - 5329 * B + 8388608 + 32767) >> 16;
  __syncthreads();
  if (t < 128) {
    const int c = t >> 6, j = t & 63;
    const int* q = &full[c][(j >> 3) * 32 + (j & 7) * 2];
    s[4 + c][j] = ((q[0] + q[1] + q[16] + q[17] + 2) >> 2) - 128;
  }
  __syncthreads();
  for (int i = t; i < 384; i += 256) {                 // G[u][x] = sum_y T[u][y] s[y][x]: |G| <= 8 * 4096 * 128
    const int b = i >> 6, u = (i >> 3) & 7, xx = i & 7;
    int acc = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += T[u * 8 + k] * s[b][k * 8 + xx];
    G[b][u * 8 + xx] = acc;
  }
  __syncthreads();
  short* o = coef + ((long long)n * gridDim.x + m) * 384;
  for (int i = t; i < 384; i += 256) {                 // F[u][v] = sum_x G[u][x] T[v][x] in 64 bits, then the divisor
    const int b = i >> 6, u = (i >> 3) & 7, v = i & 7;
    long long F = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) F += (long long)G[b][u * 8 + k] * T[v * 8 + k];
    const int z = kZigzagOf[u * 8 + v];
    unsigned q = qt[(b >= 4 ? 64 : 0) + z];
    q = q ? q : 1u;
    const unsigned long long a = (unsigned long long)(F < 0 ? -F : F);
    // (|F| + q 2^25) / (q 2^26) = ((|F| + q 2^25) >> 26) / q  (nested floor division), the quotient of the shift fits 32 bits
    const unsigned r = (unsigned)((a + ((unsigned long long)q << 25)) >> 26) / q;
    o[b * 64 + z] = (short)(F < 0 ? -(int)r : (int)r);
  }
}

__device__ __forceinline__ int wave_scan_incl(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

// the low `len` bits (1..59) of val to bit positions [pos, pos + len) of the buffer, bit 0 = most significant bit of word 0
__device__ __forceinline__ void put_bits(unsigned* buf, unsigned pos, unsigned long long val, int len) {
  const unsigned w = pos >> 5, off = pos & 31;
  if (w + 2 >= (unsigned)BUF_WORDS) return;          // unreachable with the standard's tables (26 bits per coefficient at most)
  const unsigned long long left = val << (64 - len);
  const unsigned long long a = left >> off;
  const unsigned w0 = (unsigned)(a >> 32), w1 = (unsigned)a, w2 = off ? (unsigned)((left << (64 - off)) >> 32) : 0u;
  if (w0) atomicOr(&buf[w], w0);
  if (w1) atomicOr(&buf[w + 1], w1);          // a non-zero word holds bits below pos + len, which is inside the buffer
  if (w2) atomicOr(&buf[w + 2], w2);
}

// grid (NI intervals, N), 64 threads.  huff: egne_hip.h layout.  WRITE false: ilen[n][i] = stuffed bytes of the interval.  WRITE true:
// the bytes to out + n*cap + ioff[n][i] and RSTm in front of them (i > 0), unless flags[n].
template <bool WRITE>
__global__ __launch_bounds__(64) void entropy_k(const short* __restrict__ coef, int nm, int R, const unsigned* __restrict__ huff,
                                                int* __restrict__ ilen, const long long* __restrict__ ioff, const int* __restrict__ flags,
                                                uint8_t* __restrict__ out, long long cap) {
  __shared__ unsigned tab[HUFF_WORDS];
  __shared__ unsigned buf[BUF_WORDS];
  __shared__ unsigned cw[MAX_RESTART * 6 * 32];
  const int lane = threadIdx.x, i = blockIdx.x, n = blockIdx.y, NI = gridDim.x;
  if (WRITE && flags[n]) return;
  const int m0 = i * R, nblk = (min(m0 + R, nm) - m0) * 6;
  const unsigned* src = reinterpret_cast<const unsigned*>(coef + ((long long)n * nm + m0) * 384);
  for (int k = lane; k < nblk * 32; k += 64) cw[k] = src[k];
  for (int k = lane; k < HUFF_WORDS; k += 64) tab[k] = huff[k];
  for (int k = lane; k < nblk * (BLOCK_BITS / 32) + 4; k += 64) buf[k] = 0u;        // what this interval can reach
  __syncthreads();
  const short* c = reinterpret_cast<const short*>(cw);
  int pred[3] = {0, 0, 0};
  unsigned base = 0;
  const unsigned long long below_me = (1ull << lane) - 1ull;
  for (int b = 0; b < nblk; ++b) {
    const int slot = b % 6, comp = slot < 4 ? 0 : slot - 3;
    const unsigned* dc_tab = tab + (comp ? 16 : 0);
    const unsigned* ac_tab = tab + 32 + (comp ? 256 : 0);
    int v = c[b * 64 + lane];
    const int dc = __shfl(v, 0, 64);
    const int pr = comp == 0 ? pred[0] : (comp == 1 ? pred[1] : pred[2]);
    if (lane == 0) v = dc - pr;
    if (comp == 0) pred[0] = dc; else if (comp == 1) pred[1] = dc; else pred[2] = dc;
    const unsigned long long nz = __ballot(v != 0) & ~1ull;              // the non-zero AC coefficients
    const int a = v < 0 ? -v : v;
    const int sz = a ? 32 - __clz(a) : 0;                                 // category: DC <= 11, AC <= 10
    const unsigned long long extra = (unsigned long long)(unsigned)(v >= 0 ? v : v + (1 << sz) - 1);
    unsigned long long bits = 0;
    int len = 0;
    if (lane == 0) {
      const unsigned e = dc_tab[sz & 15];
      len = (int)(e >> 16) + sz;
      bits = ((unsigned long long)(e & 0xffffu) << sz) | extra;
    } else if (v != 0) {
      const unsigned long long below = nz & below_me;
      const int prev = below ? 63 - __clzll((long long)below) : 0;
      const int run = lane - prev - 1;
      const unsigned zrl = ac_tab[0xF0], e = ac_tab[((run & 15) << 4) | (sz & 15)];
      for (int z = run >> 4; z > 0; --z) {                                // at most 3
        bits = (bits << (zrl >> 16)) | (zrl & 0xffffu);
        len += (int)(zrl >> 16);
      }
      const int l = (int)(e >> 16) + sz;
      bits = (bits << l) | ((unsigned long long)(e & 0xffffu) << sz) | extra;
      len += l;
    } else if (lane == 63) {                                              // coefficient 63 is zero: EOB
      const unsigned e = ac_tab[0];
      bits = e & 0xffffu;
      len = (int)(e >> 16);
    }
    len = min(len, 59);                                                   // (tables of the standard never exceed it)
    const int incl = wave_scan_incl(len, lane);
    if (len > 0) put_bits(buf, base + (unsigned)(incl - len), bits, len);
    base += (unsigned)min(__shfl(incl, 63, 64), BLOCK_BITS);
  }
  const int pad = (int)((0u - base) & 7u);
  if (lane == 0 && pad) put_bits(buf, base, (1ull << pad) - 1ull, pad);  // the last byte is filled with 1-bits
  __syncthreads();
  const int nbytes = (int)((base + 7u) >> 3);
  uint8_t* dst = WRITE ? out + (long long)n * cap + ioff[(long long)n * NI + i] : nullptr;
  int done = 0;
  for (int j0 = 0; j0 < nbytes; j0 += 256) {
    const int j = j0 + lane * 4;
    const unsigned w = j < nbytes ? buf[j >> 2] : 0u;
    const int valid = min(max(nbytes - j, 0), 4);
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt += k < valid ? (((w >> (24 - 8 * k)) & 255u) == 255u ? 2 : 1) : 0;
    const int incl = wave_scan_incl(cnt, lane);
    if (WRITE) {
      uint8_t* o = dst + done + incl - cnt;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < valid) {
          const unsigned byte = (w >> (24 - 8 * k)) & 255u;
          *o++ = (uint8_t)byte;
          if (byte == 255u) *o++ = 0;
        }
    }
    done += __shfl(incl, 63, 64);
  }
  if (lane == 0) {
    if (!WRITE) ilen[(long long)n * NI + i] = done;
    else if (i > 0) { dst[-2] = 0xFF; dst[-1] = (uint8_t)(0xD0 + ((i - 1) & 7)); }
  }
}

// grid (N), 256 threads: ioff[n][i] = header_len + sum_{k<i} (ilen[n][k] + 2) (every interval is followed by a marker: RSTm or EOI)
__global__ __launch_bounds__(256) void layout_k(const int* __restrict__ ilen, int NI, const uint8_t* __restrict__ header, int header_len,
                                                long long cap, long long* __restrict__ ioff, int* __restrict__ lengths,
                                                int* __restrict__ flags, uint8_t* __restrict__ out) {
  __shared__ long long wave_sum[4];
  const int t = threadIdx.x, n = blockIdx.x, lane = t & 63, wave = t >> 6;
  long long carry = header_len;
  for (int i0 = 0; i0 < NI; i0 += 256) {
    const int i = i0 + t;
    const long long v = i < NI ? (long long)ilen[(long long)n * NI + i] + 2 : 0;
    long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long u = __shfl_up(incl, d, 64);
      if (lane >= d) incl += u;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    long long before = 0, all = 0;
    for (int k = 0; k < 4; ++k) { before += k < wave ? wave_sum[k] : 0; all += wave_sum[k]; }
    if (i < NI) ioff[(long long)n * NI + i] = carry + before + incl - v;
    carry += all;
    __syncthreads();
  }
  const bool fits = carry <= cap;                      // carry = the file's length: header, intervals, NI - 1 RSTm, EOI
  if (t == 0) { lengths[n] = fits ? (int)carry : 0; flags[n] = fits ? 0 : 1; }
  if (fits) {
    uint8_t* o = out + (long long)n * cap;
    for (int k = t; k < header_len; k += 256) o[k] = header[k];
    if (t == 0) { o[carry - 2] = 0xFF; o[carry - 1] = 0xD9; }
  }
}

// grid (ceil(cw*ch / 256), N): the clipped patch [cx0, cx0+cw) x [cy0, cy0+ch) of frame n blended with mask[n]
__global__ __launch_bounds__(256) void stamp_k(uint8_t* __restrict__ bgr, int H, int W, const uint8_t* __restrict__ mask, int ph, int pw,
                                               int x0, int y0, int cx0, int cy0, int cw, int ch, int b, int g, int r) {
  const int idx = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (idx >= cw * ch) return;
  const int y = cy0 + idx / cw, x = cx0 + idx % cw;
  const int a = mask[((long long)n * ph + (y - y0)) * pw + (x - x0)];
  uint8_t* p = bgr + (((long long)n * H + y) * W + x) * 3;
  const int ink[3] = {b, g, r};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int t = p[k] * (255 - a) + ink[k] * a + 128;
    p[k] = (uint8_t)(((t >> 8) + t) >> 8);
  }
}

inline long long up16(long long v) { return (v + 15) / 16 * 16; }
inline long long mcus(int H, int W) { return (long long)((H + 15) / 16) * ((W + 15) / 16); }

}  // namespace

extern "C" int64_t egne_jpeg_workspace_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 16;
  const long long nm = mcus(H, W);
  return up16((long long)N * nm * 384 * (long long)sizeof(short)) + up16((long long)N * nm * (long long)sizeof(int)) +
         up16((long long)N * nm * (long long)sizeof(long long));
}

extern "C" int egne_jpeg_encode(const uint8_t* bgr, int N, int H, int W, const uint8_t* qt, const void* huff, const int32_t* dct,
                                const uint8_t* header, int header_len, int restart_mcus, uint8_t* out, int64_t cap, int32_t* lengths,
                                int32_t* flags, void* ws, void* stream) {
  EGNE_REQUIRE(N > 0 && H > 0 && W > 0, "jpeg_encode: bad shape (N %d, frames %dx%d)", N, H, W);
  EGNE_REQUIRE(bgr && out && lengths && flags && ws, "jpeg_encode: null frames, output, lengths, flags or workspace");
  EGNE_REQUIRE(qt && huff && dct && header, "jpeg_encode: a table is missing (divisors %p, code tables %p, DCT matrix %p, header %p)",
               (const void*)qt, huff, (const void*)dct, (const void*)header);
  EGNE_REQUIRE(restart_mcus >= 1 && restart_mcus <= MAX_RESTART, "jpeg_encode: restart_mcus %d outside 1..%d", restart_mcus, MAX_RESTART);
  EGNE_REQUIRE(header_len > 0 && cap > 0 && cap <= 0x7fffffffLL, "jpeg_encode: bad header length %d or capacity %lld", header_len, (long long)cap);
  EGNE_REQUIRE(N <= 65535 && H <= 65535 && W <= 65535, "jpeg_encode: shape out of range (N %d, frames %dx%d)", N, H, W);
  EGNE_REQUIRE((((uintptr_t)ws) & 15) == 0, "jpeg_encode: the workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int mw = (W + 15) / 16, nm = (int)mcus(H, W), NI = (nm + restart_mcus - 1) / restart_mcus;
  short* coef = (short*)ws;
  int* ilen = (int*)((char*)ws + up16((long long)N * nm * 384 * (long long)sizeof(short)));
  long long* ioff = (long long*)((char*)ilen + up16((long long)N * nm * (long long)sizeof(int)));
  const unsigned* ht = (const unsigned*)huff;
  hipLaunchKernelGGL(dct_k, dim3(nm, N), dim3(256), 0, st, bgr, H, W, mw, qt, (const int*)dct, coef);
  hipLaunchKernelGGL(entropy_k<false>, dim3(NI, N), dim3(64), 0, st, coef, nm, restart_mcus, ht, ilen, ioff, flags, out, (long long)cap);
  hipLaunchKernelGGL(layout_k, dim3(N), dim3(256), 0, st, ilen, NI, header, header_len, (long long)cap, ioff, lengths, flags, out);
  hipLaunchKernelGGL(entropy_k<true>, dim3(NI, N), dim3(64), 0, st, coef, nm, restart_mcus, ht, ilen, ioff, flags, out, (long long)cap);
  return egne::check_launch("egne_jpeg_encode");
}

extern "C" int egne_stamp_mask(uint8_t* bgr, int N, int H, int W, const uint8_t* mask, int ph, int pw, int x0, int y0, int b, int g, int r,
                               void* stream) {
  EGNE_REQUIRE(bgr && mask && N > 0 && H > 0 && W > 0 && ph > 0 && pw > 0, "stamp_mask: bad arguments (N %d, frames %dx%d, patch %dx%d)", N, H, W, ph, pw);
  EGNE_REQUIRE(N <= 65535 && H <= 65535 && W <= 65535 && ph <= 65535 && pw <= 65535 && x0 > -65536 && x0 < 65536 && y0 > -65536 && y0 < 65536,
               "stamp_mask: shape out of range");
  EGNE_REQUIRE(((b | g | r) & ~255) == 0, "stamp_mask: ink (%d, %d, %d) outside 0..255", b, g, r);
  const int cx0 = x0 > 0 ? x0 : 0, cy0 = y0 > 0 ? y0 : 0;
  const int cx1 = x0 + pw < W ? x0 + pw : W, cy1 = y0 + ph < H ? y0 + ph : H;
  if (cx1 <= cx0 || cy1 <= cy0) return EGNE_OK;          // the patch lies outside the frame
  const int cw = cx1 - cx0, ch = cy1 - cy0;
  EGNE_REQUIRE((long long)cw * ch <= (1 << 30), "stamp_mask: patch too large");
  hipLaunchKernelGGL(stamp_k, dim3(egne::cdiv((long long)cw * ch, 256), N), dim3(256), 0, (hipStream_t)stream, bgr, H, W, mask, ph, pw, x0, y0,
                     cx0, cy0, cw, ch, b, g, r);
  return egne::check_launch("egne_stamp_mask");
}
