// Split-f16 implicit-GEMM convolution, deep variant for the wide VGG-trunk layers (Cout % 256 == 0 or 128, Cin % 32 == 0):
// 256 x BN tile, 8 waves (wave tile 128 x 64), K step = 32 channels of one tap, TWO LDS stages, ONE barrier per K step.
//
// The 128x128 kernel (conv_f16x3.hip) pays two barriers per 24 MFMAs and tops out at ~285 TFLOP/s algorithmic
// (~860 TFLOP/s of f16 MFMA, the ceiling of that structure).  Here
//   * the weights are packed as ready-made LDS images (hi | lo granules, 128 B per output channel and K step, XOR
//     swizzle applied at pack time) and staged by LDS-DMA (`buffer_load_dwordx4 ... lds`): no registers, no VALU;
//   * the activations stay fp32 in HBM: the loads of step k+1 are issued before the 48 MFMAs of step k, converted to
//     hi / lo afterwards and written to the other LDS stage (buffer addressing with per-row tap masks as in the
//     128x128 kernel);
//   * the product is computed transposed (weights as the A operand), so a lane ends up with 4 consecutive output
//     channels of one pixel and stores 16 bytes.
// LDS image of a stage: row r (pixel or output channel) = 128 bytes = 4 granules of 8 channels, granule = [hi x8 | lo x8];
// the 16-byte chunk c of row r sits at chunk c ^ (((r >> 1) + 6) & 7): conflict free for the ds_read_b128 patterns of BOTH MFMA
// shapes (32 rows x 2 chunk columns for 32x32x16, 16 rows x 4 chunk columns for 16x16x32).
//
// M16 computes the same tile with v_mfma_f32_16x16x32_f16 (one instruction per 32-channel step and 16 x 16 block): the same
// FLOP per cycle, but these kernels run at the power limit and the chip holds a higher clock on this shape (MI355X DVFS).
//
// Split-pair storage in channel order (egne_conv_desc.out_split = 3 / egne_seg.presplit = 3; 16 x 16 x 32 shape, three products): the trunk
// tensors conv3_1 .. conv5_3 / pool3 / pool4 of the calibrated inference plan hold, per pixel and 32-channel block, [hi x32 | lo x32] halves
// of x * s -- the very pair this kernel's staging derives from the fp32 value, computed ONCE in the producer's epilogue.  An input in that
// storage is then staged like the weights: 16-byte pieces by LDS-DMA, the XOR swizzle of the LDS image carried by the per-lane SOURCE address
// (taps outside the image and rows past the batch through the out-of-range offset: zeros), no registers, no VALU, no ds_write.  The operands,
// the K order and the order of the three products are those of the converting path: the results agree bit for bit.
#include "common.h"
#include "kernel_util.h"
#include "split_f16.h"
#include <cstdlib>
#include <type_traits>

namespace {

constexpr int BM = 256, ROWB = 128;

// NB = 32-channel blocks per wave along N (2 -> BN = 256 with 4 waves along N, 1 -> BN = 128)
// NP = products per multiply: 3 (hi hi + hi lo + lo hi) or 1 (hi hi: plain f16 operands; egne_conv_desc.f16_products) -- the lo halves
// are then neither derived, stored nor read (the weight image keeps its layout: the lo chunks of a row are simply not touched)
// PS = storage of the tensors: bit 0 split-pair (channel order) output, bit 1 split-pair input (a calibrating run measures the fp32 output of
// a launch whose input is already split: PS = 2)
template <int NB, bool M16, int NP = 3, int PS = 0>
__global__ __launch_bounds__(512) void conv_f16x3_big_kernel(const egne_conv_desc p, const char* __restrict__ wimg, float a_scale,
                                                             float out_scale) {
  constexpr int BN = 128 * NB;
  constexpr int STAGE = (BM + BN) * ROWB;
  extern __shared__ __attribute__((aligned(1024))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = (PS & 2) ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;     // (uniform: the LDS-DMA's base goes through M0)
  const int wm = wave >> 2, wn = wave & 3;               // 2 x 4 waves; wave tile 128 x (32 * NB)
  const long long M = (long long)p.B * p.Ho * p.Wo;
  const long long m0 = (long long)blockIdx.x * BM;
  const int ntile = blockIdx.y;
  const int T = p.kh * p.kw;
  const egne_seg sg = p.seg[0];
  const int hw = p.Ho * p.Wo, frame_px = p.H * p.W;
  const int b0 = (int)(m0 / hw);
  const long long in_left = ((long long)p.B - b0) * frame_px * sg.pix_stride * 4;
  const __amdgpu_buffer_rsrc_t rin = make_rsrc(sg.ptr + (long long)b0 * frame_px * sg.pix_stride,
                                               (unsigned)(in_left < 0x7fffffffll ? in_left : 0x7fffffffll));
  const int nchunk = sg.Cp >> 5;
  const int nsteps = T * nchunk;
  // weight images: [ntile][step = chunk*T + tap][BN rows x 128 B]
  const __amdgpu_buffer_rsrc_t rw = make_rsrc(wimg + (long long)ntile * nsteps * (BN * ROWB), (unsigned)(nsteps * BN * ROWB));

  // ---- A staging: thread -> 4 items (row = (tid>>3) + 64*i, float4 column c4 = tid&7)
  //      split-pair input: lane -> 4 DMA pieces of 16 bytes (row = 32 wave + 8 i + (lane >> 3), LDS chunk pc = lane & 7 <- the row's chunk
  //      c = pc ^ key(row): hi (c even) or lo (c odd) halves of channels 8 (c >> 1) .. + 7 of the block: source byte (c & 1) * 64 + (c >> 1) * 16) ----
  const int c4 = tid & 7;
  int roff[4];
  unsigned tapmask[4];
  {
    const int dil = p.dil[0];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row_i = (PS & 2) ? 32 * wave + 8 * i + (lane >> 3) : (tid >> 3) + 64 * i;
      const long long m = m0 + row_i;
      const int b = (int)(m / hw);
      const int r = (int)(m - (long long)b * hw);
      const int oy = r / p.Wo, ox = r - oy * p.Wo;
      const int lc = (lane & 7) ^ (((row_i >> 1) + 6) & 7);
      roff[i] = ((((b - b0) * p.H + oy) * p.W + ox) * (int)sg.pix_stride + sg.ch_off) * 4 + ((PS & 2) ? (lc & 1) * 64 + (lc >> 1) * 16 : c4 * 16);
      unsigned mk = 0;
      for (int ky = 0; ky < p.kh; ++ky)
        for (int kx = 0; kx < p.kw; ++kx) {
          const int iy = oy + (ky - p.pad_h) * dil, ix = ox + (kx - p.pad_w) * dil;
          if (m < M && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) mk |= 1u << (ky * p.kw + kx);
        }
      tapmask[i] = mk;
    }
  }
  // LDS destination of item i: row r, granule c4>>1, half (c4&1): hi at chunk 2g, lo at chunk 2g+1, 8 bytes at (c4&1)*8
  int ldst_hi[4], ldst_lo[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (tid >> 3) + 64 * i, g = c4 >> 1, sw = ((r >> 1) + 6) & 7;
    ldst_hi[i] = r * ROWB + (((2 * g) ^ sw) << 4) + (c4 & 1) * 8;
    ldst_lo[i] = r * ROWB + (((2 * g + 1) ^ sw) << 4) + (c4 & 1) * 8;
  }
  // weight DMA: BN rows x 128 B = BN/8 wave instructions of 1 KB, NB*2 per wave; the image is already swizzled: linear copy
  const int wvoff = lane * 16;

  u32x4 ra[4];
  int ky_n = 0, kx_n = 0, c0_n = 0;     // coordinates of the step being loaded
  // (split-pair input: the step's 256 rows x 128 B straight into `stage`, 32 instructions of 1 KB, four per wave)
  auto load_a = [&](int tap, int stage) {
    const int dil = p.dil[0];
    const int tapoff = (((ky_n - p.pad_h) * p.W + (kx_n - p.pad_w)) * dil * (int)sg.pix_stride + c0_n) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ok = (tapmask[i] >> tap) & 1u;
      if constexpr ((PS & 2))
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rin, (lds_ptr)(lds + stage * STAGE + wave * 4096 + i * 1024), 16, ok ? roff[i] + tapoff : (int)OOB, 0, 0, 0);
      else
        ra[i] = __builtin_amdgcn_raw_buffer_load_b128(rin, ok ? roff[i] + tapoff : (int)OOB, 0, 0);
    }
  };
  auto dma_b = [&](int stage, int step) {
    char* base = lds + stage * STAGE + BM * ROWB;
#pragma unroll
    for (int j = 0; j < 2 * NB; ++j) {
      const int blk = wave * 2 * NB + j;      // 1-KB block of the image
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_ptr)(base + blk * 1024), 16, wvoff, step * (BN * ROWB) + blk * 1024, 0, 0);
    }
  };
  auto store_a = [&](int stage) {
    char* base = lds + stage * STAGE;
#pragma unroll
    for (int i = 0; i < ((PS & 2) ? 0 : 4); ++i) {
      const f32x4 v = __builtin_bit_cast(f32x4, ra[i]);
      if constexpr (NP == 1) {
        const f32x2 t0 = {v[0] * a_scale, v[1] * a_scale}, t1 = {v[2] * a_scale, v[3] * a_scale};
        const h2 h0 = __builtin_convertvector(t0, h2), h1 = __builtin_convertvector(t1, h2);
        const h4 hi = {h0[0], h0[1], h1[0], h1[1]};
        *(h4*)(base + ldst_hi[i]) = hi;
        continue;
      }
      h2 h0, h1, l0, l1;                        // x * a_scale = hi + lo, plain (unpacked) VALU: split_f16.h
      egne::split2(v[0], v[1], a_scale, h0, l0);
      egne::split2(v[2], v[3], a_scale, h1, l1);
      const h4 hi = {h0[0], h0[1], h1[0], h1[1]}, lo = {l0[0], l0[1], l1[0], l1[1]};
      *(h4*)(base + ldst_hi[i]) = hi;
      *(h4*)(base + ldst_lo[i]) = lo;
    }
  };
  auto advance = [&]() {
    if (++kx_n == p.kw) { kx_n = 0; ++ky_n; }
    if (ky_n == p.kh) { ky_n = 0; c0_n += 32; }
  };

  // 32x32x16: acc[4][NB] blocks of 32 x 32; 16x16x32: acc[8][2 * NB] blocks of 16 x 16 (same 64 * NB registers)
  constexpr int MB = M16 ? 16 : 32, NTM = 128 / MB, NTN = 32 * NB / MB;
  using acc_t = std::conditional_t<M16, f32x4, f32x16>;
  acc_t acc[NTM][NTN];
#pragma unroll
  for (int a = 0; a < NTM; ++a)
#pragma unroll
    for (int b = 0; b < NTN; ++b) acc[a][b] = (acc_t)(0.f);

  const int lr = lane & (MB - 1), kg = lane / MB;       // row inside a block, 8-channel group (2 or 4 of them)
  int aoffs[NTM], boffs[NTN];
#pragma unroll
  for (int t = 0; t < NTM; ++t) aoffs[t] = (wm * 128 + t * MB + lr) * ROWB;
#pragma unroll
  for (int t = 0; t < NTN; ++t) boffs[t] = BM * ROWB + (wn * 32 * NB + t * MB + lr) * ROWB;
  const int sw = ((lr >> 1) + 6) & 7;

  // prologue: step 0 into stage 0
  load_a(0, 0);
  dma_b(0, 0);
  store_a(0);
  advance();
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  int tap_n = 1 % T;
  for (int step = 0; step < nsteps; ++step) {
    const int st = step & 1;
    const bool more = step + 1 < nsteps;
    if (more) {                     // loads of step+1 in flight during the MFMAs of this step
      load_a(tap_n, st ^ 1);               // (the other stage was last read in step-1: every wave passed the barrier since)
      dma_b(st ^ 1, step + 1);
    }
    const char* base = lds + st * STAGE;
    if constexpr (M16) {
      const int ch = ((2 * kg) ^ sw) << 4, cl = ((2 * kg + 1) ^ sw) << 4;
      h8 bh[NTN], bl[NTN];
#pragma unroll
      for (int t = 0; t < NTN; ++t) {
        bh[t] = *(const h8*)(base + boffs[t] + ch);
        if constexpr (NP == 3) bl[t] = *(const h8*)(base + boffs[t] + cl);
      }
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        h8 ah[4], al[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          ah[t] = *(const h8*)(base + aoffs[half * 4 + t] + ch);
          if constexpr (NP == 3) al[t] = *(const h8*)(base + aoffs[half * 4 + t] + cl);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int tn = 0; tn < NTN; ++tn) {
            acc_t& c = acc[half * 4 + t][tn];
            if constexpr (NP == 3) {
              c = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh[tn], al[t], c, 0, 0, 0);
              c = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl[tn], ah[t], c, 0, 0, 0);
            }
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh[tn], ah[t], c, 0, 0, 0);
          }
      }
    } else {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int ch = ((2 * (2 * ks + kg)) ^ sw) << 4, cl = ((2 * (2 * ks + kg) + 1) ^ sw) << 4;
      h8 ah[4], al[4], bh[NB], bl[NB];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        ah[t] = *(const h8*)(base + aoffs[t] + ch);
        al[t] = *(const h8*)(base + aoffs[t] + cl);
      }
#pragma unroll
      for (int t = 0; t < NB; ++t) {
        bh[t] = *(const h8*)(base + boffs[t] + ch);
        bl[t] = *(const h8*)(base + boffs[t] + cl);
      }
#pragma unroll
      for (int tm = 0; tm < 4; ++tm)
#pragma unroll
        for (int tn = 0; tn < NB; ++tn) {
          if constexpr (!M16) {
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[tn], al[tm], acc[tm][tn], 0, 0, 0);
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl[tn], ah[tm], acc[tm][tn], 0, 0, 0);
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[tn], ah[tm], acc[tm][tn], 0, 0, 0);
          }
        }
    }
    }
    if (more) {
      store_a(st ^ 1);              // the other stage was last read in step-1: every wave passed the barrier since
      advance();
      tap_n = tap_n + 1 == T ? 0 : tap_n + 1;
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

  // ---- epilogue: transposed product, lane = pixel lr of the block; 32x32x16: channels n = 32*blk + 8*j + 4*kg + e (register
  //      4*j + e); 16x16x32: channels n = 16*blk + 4*kg + e (register e) ----
  const float slope = p.act == EGNE_ACT_RELU ? 0.f : (p.act == EGNE_ACT_LEAKY ? 0.01f : 1.f);
  const long long left = M - m0;
  const __amdgpu_buffer_rsrc_t rout = make_rsrc(p.out + m0 * p.out_pix_stride, (unsigned)((left < BM ? left : BM) * p.out_pix_stride * 4));
  constexpr int NJ = M16 ? 1 : 4;
  bool bad = false;
  if constexpr (PS & 1) {
    // Split-pair output, planes in channel order.  A lane ends with channels 4 kg .. + 3 of every 16-channel block: 8 bytes per plane.  The lanes kg and
    // kg ^ 1 (16 lanes apart) trade one piece per pair of blocks (ds_swizzle, no LDS memory), so that an even kg holds channels 8 (kg / 2) .. + 7 of the
    // 32-channel block and an odd kg channels 16 + 8 (kg / 2) .. + 7: ONE 16-byte store per plane and lane, 64 contiguous bytes per pixel and
    // instruction as in the fp32 form.  The stored pair is the one a reader's staging would derive from the fp32 value (split_f16.h).
    static_assert(M16 && NP == 3, "split-pair output: 16 x 16 x 32 shape, three products");
    const float oss = p.out_split_scale;
    const bool odd = kg & 1;
    const int pb = (odd ? 32 : 0) + 16 * (kg >> 1);          // byte of the lane's eight halves inside a plane
#pragma unroll
    for (int bp = 0; bp < NTN / 2; ++bp) {
      const int nb = ntile * BN + wn * 32 * NB + bp * 32;      // first channel of the 32-channel block
      const bool nok = nb < p.Cout_store;
      const f32x4 bv0 = (p.bias && nok) ? *(const f32x4*)(p.bias + nb + 4 * kg) : (f32x4)(0.f);
      const f32x4 bv1 = (p.bias && nok) ? *(const f32x4*)(p.bias + nb + 16 + 4 * kg) : (f32x4)(0.f);
#pragma unroll
      for (int tm = 0; tm < NTM; ++tm) {
        u32x2 hi[2], lo[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float t = acc[tm][2 * bp + q][e] * out_scale + (q ? bv1[e] : bv0[e]);
            v[e] = fmaxf(t, t * slope);
          }
          h2 h0, h1, l0, l1;
          egne::split2(v[0], v[1], oss, h0, l0);
          egne::split2(v[2], v[3], oss, h1, l1);
          if (bp == 0 && q == 0) bad |= egne_nonfinite(v[0]) || egne_nonfinite((float)h0[0]);       // lane = pixel: one channel per pixel (common.h)
          hi[q] = u32x2{__builtin_bit_cast(unsigned, h0), __builtin_bit_cast(unsigned, h1)};
          lo[q] = u32x2{__builtin_bit_cast(unsigned, l0), __builtin_bit_cast(unsigned, l1)};
        }
        // an even kg gives its piece of the second block and takes the neighbour's piece of the first; an odd kg the other way round
        const u32x2 sh = odd ? hi[0] : hi[1], sl = odd ? lo[0] : lo[1];
        u32x2 rh, rl;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          rh[e] = (unsigned)__builtin_amdgcn_ds_swizzle((int)sh[e], 0x401f);      // lane ^ 16
          rl[e] = (unsigned)__builtin_amdgcn_ds_swizzle((int)sl[e], 0x401f);
        }
        const u32x4 oh = odd ? u32x4{rh[0], rh[1], hi[1][0], hi[1][1]} : u32x4{hi[0][0], hi[0][1], rh[0], rh[1]};
        const u32x4 ol = odd ? u32x4{rl[0], rl[1], lo[1][0], lo[1][1]} : u32x4{lo[0][0], lo[0][1], rl[0], rl[1]};
        const int row = wm * 128 + tm * MB + lr;
        const int o = nok ? (row * (int)p.out_pix_stride + p.out_ch_off + nb) * 4 + pb : (int)OOB;
        __builtin_amdgcn_raw_buffer_store_b128(oh, rout, o, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(ol, rout, o + 64, 0, 0);
      }
    }
    egne_ovf_commit(bad, p.ovf_flag);
    return;
  }
#pragma unroll
  for (int tn = 0; tn < NTN; ++tn)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int n = ntile * BN + wn * 32 * NB + tn * MB + (M16 ? 4 * kg : 8 * j + 4 * kg);
      const bool nok = n < p.Cout_store;
      const f32x4 bv = (p.bias && nok) ? *(const f32x4*)(p.bias + n) : (f32x4)(0.f);
#pragma unroll
      for (int tm = 0; tm < NTM; ++tm) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float t = acc[tm][tn][4 * j + e] * out_scale + bv[e];
          v[e] = fmaxf(t, t * slope);
        }
        if (tn == 0 && j == 0) bad |= egne_nonfinite(v[0]);       // lane = pixel: one channel per pixel (common.h)
        const int row = wm * 128 + tm * MB + lr;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rout,
                                               nok ? (row * (int)p.out_pix_stride + p.out_ch_off + n) * 4 : (int)OOB, 0, 0);
      }
    }
  egne_ovf_commit(bad, p.ovf_flag);
}

// OIHW fp32 -> LDS images [ntile][step = chunk*T + tap][BN rows][128 B]: row j = output channel ntile*BN + j, granule g =
// channels chunk*32 + 8g .. +7 as [hi x8 | lo x8], 16-byte chunk c stored at chunk c ^ (((j >> 1) + 6) & 7)
__global__ void pack_weight_f16img_k(const float* __restrict__ w, int Cout, int Cin, int T, int BN, int ntiles, int nchunk,
                                     float wscale, _Float16* __restrict__ out) {
  const long long total = (long long)ntiles * nchunk * T * BN * 64;     // halfs
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int e = (int)(i & 7), pc = (int)((i >> 3) & 7);
    long long q = i >> 6;
    const int j = (int)(q % BN); q /= BN;
    const int step = (int)(q % (nchunk * T));
    const int nt = (int)(q / (nchunk * T));
    const int chunk = step / T, tap = step - chunk * T;
    const int lc = pc ^ (((j >> 1) + 6) & 7), g = lc >> 1, hl = lc & 1;
    const int n = nt * BN + j, ci = chunk * 32 + 8 * g + e;
    const float v = (n < Cout && ci < Cin) ? w[((long long)n * Cin + ci) * T + tap] * wscale : 0.f;
    const _Float16 h = (_Float16)v;
    out[i] = hl ? (_Float16)(v - (float)h) : h;
  }
}

}  // namespace

extern "C" int egne_pack_conv_weight_f16img(const float* w_oihw, int Cout, int Cin, int kh, int kw, int BN, int Ktot, float wscale,
                                            void* wimg, void* stream) {
  EGNE_REQUIRE(w_oihw && wimg && Cout > 0 && Cin > 0 && (BN == 128 || BN == 256) && Ktot >= Cin && Ktot % 32 == 0 && wscale > 0.f,
               "pack_f16img: bad sizes Cout %d Cin %d BN %d Ktot %d", Cout, Cin, BN, Ktot);
  const int ntiles = (Cout + BN - 1) / BN, nchunk = Ktot / 32;
  long long total = (long long)ntiles * nchunk * kh * kw * BN * 64, g = (total + 255) / 256;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(pack_weight_f16img_k, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, w_oihw, Cout, Cin, kh * kw, BN, ntiles,
                     nchunk, wscale, (_Float16*)wimg);
  return egne::check_launch("egne_pack_conv_weight_f16img");
}

// Same descriptor as egne_conv2d_f16x3_fwd: one input slice without fused affine, Cp % 32 == 0, stride 1, zero padding,
// one group, no residual / post affine; d->CoutP = Cout rounded up to BN (128 or 256: CoutP % 256 == 0 selects 256).
// d->out_split = 3 (three products only): the output in channel-order split-pair storage under d->out_split_scale; d->seg[0].presplit = 3:
// the input in that storage, written under THIS launch's a_scale.
extern "C" int egne_conv2d_f16x3_big_fwd(const egne_conv_desc* dp, const void* wimg, float a_scale, float w_scale, void* stream) {
  EGNE_REQUIRE(dp && wimg, "conv_f16x3_big: null pointer");
  const egne_conv_desc& d = *dp;
  EGNE_REQUIRE(d.nseg == 1 && d.ngroups == 1 && d.stride == 1 && d.pad_mode == 0 && !d.seg[0].scale && !d.seg[0].shift && !d.residual &&
               !d.post_scale, "conv_f16x3_big: unsupported descriptor");
  EGNE_REQUIRE(d.kh >= 1 && d.kw >= 1 && d.kh * d.kw <= 32, "conv_f16x3_big: %d taps (%dx%d): the per-row tap mask holds 32", d.kh * d.kw, d.kh, d.kw);
  const egne_seg& g = d.seg[0];
  EGNE_REQUIRE(g.ptr && g.Cp % 32 == 0 && g.Cp == d.Ktot && ((uintptr_t)g.ptr & 15) == 0 && g.ch_off % 4 == 0 && g.pix_stride % 4 == 0,
               "conv_f16x3_big: input slice (Cp %d Ktot %d)", g.Cp, d.Ktot);
  EGNE_REQUIRE(d.CoutP % 128 == 0 && d.Cout_store <= d.CoutP && d.Cout_store % 4 == 0 && d.out && ((uintptr_t)d.out & 15) == 0 &&
               d.out_ch_off % 4 == 0 && d.out_pix_stride % 4 == 0 && d.out_ch_off + d.Cout_store <= d.out_pix_stride &&
               d.out_pix_stride * 1024 < (1ll << 31) && (!d.bias || ((uintptr_t)d.bias & 15) == 0), "conv_f16x3_big: output");
  const int dd = d.dil[0];
  EGNE_REQUIRE(dd >= 1 && d.H + 2 * d.pad_h * dd - dd * (d.kh - 1) == d.Ho && d.W + 2 * d.pad_w * dd - dd * (d.kw - 1) == d.Wo,
               "conv_f16x3_big: output %dx%d inconsistent with geometry", d.Ho, d.Wo);
  EGNE_REQUIRE(((uintptr_t)wimg & 15) == 0 && a_scale > 0.f && w_scale > 0.f, "conv_f16x3_big: weights / scales");
  EGNE_REQUIRE((g.presplit == 0 || g.presplit == 3) && (d.out_split == 0 || d.out_split == 3),
               "conv_f16x3_big: storage (presplit %d, out_split %d): 0 or 3 (channel-order split pairs)", g.presplit, d.out_split);
  const long long M = (long long)d.B * d.Ho * d.Wo;
  const float os = 1.0f / (a_scale * w_scale);
  hipStream_t st = (hipStream_t)stream;
  if (d.out_split == 3 || g.presplit == 3) {
    EGNE_REQUIRE(d.f16_products != 1 && (d.out_split == 0 || (d.out_split_scale > 0.f && d.Cout_store % 32 == 0 && d.out_ch_off % 32 == 0)) &&
                 (g.presplit == 0 || g.ch_off % 32 == 0), "conv_f16x3_big: split-pair slices are whole 32-channel blocks, three products");
    const bool in3 = g.presplit == 3, out3 = d.out_split == 3;
#define EGNE_BIGP_GO(NBV, PSV)                                                                                                               \
  do {                                                                                                                                      \
    if (!egne::raise_lds((const void*)conv_f16x3_big_kernel<NBV, true, 3, PSV>, 2 * (BM + 128 * NBV) * ROWB))                               \
      return egne::fail(EGNE_ERR_LAUNCH, "conv_f16x3_big: cannot raise the dynamic LDS limit");                                             \
    hipLaunchKernelGGL((conv_f16x3_big_kernel<NBV, true, 3, PSV>), dim3((unsigned)((M + BM - 1) / BM), (unsigned)(d.CoutP / (128 * NBV))),  \
                       dim3(512), 2 * (BM + 128 * NBV) * ROWB, st, d, (const char*)wimg, a_scale, os);                                      \
  } while (0)
    if (d.CoutP % 256 == 0) { if (in3 && out3) EGNE_BIGP_GO(2, 3); else if (in3) EGNE_BIGP_GO(2, 2); else EGNE_BIGP_GO(2, 1); }
    else { if (in3 && out3) EGNE_BIGP_GO(1, 3); else if (in3) EGNE_BIGP_GO(1, 2); else EGNE_BIGP_GO(1, 1); }
#undef EGNE_BIGP_GO
    return egne::check_launch("egne_conv2d_f16x3_big_fwd");
  }
  static const bool m16 = !(getenv("EGNE_BIG_M16") && atoi(getenv("EGNE_BIG_M16")) == 0);     // MFMA shape (header)
  // (the kernels are emitted in the order they are named here)
  if (!egne::raise_lds((const void*)conv_f16x3_big_kernel<2, false>, 128 * 1024) || !egne::raise_lds((const void*)conv_f16x3_big_kernel<1, false>, 96 * 1024) ||
      !egne::raise_lds((const void*)conv_f16x3_big_kernel<2, true>, 128 * 1024) || !egne::raise_lds((const void*)conv_f16x3_big_kernel<1, true>, 96 * 1024))
    return egne::fail(EGNE_ERR_LAUNCH, "conv_f16x3_big: cannot raise the dynamic LDS limit");
  if (d.f16_products == 1) {       // plain f16 operands (the edge network next to a bf16-storage training plan): 16x16x32 shape only
    if (!egne::raise_lds((const void*)conv_f16x3_big_kernel<2, true, 1>, 128 * 1024) || !egne::raise_lds((const void*)conv_f16x3_big_kernel<1, true, 1>, 96 * 1024))
      return egne::fail(EGNE_ERR_LAUNCH, "conv_f16x3_big: cannot raise the dynamic LDS limit");
    if (d.CoutP % 256 == 0)
      hipLaunchKernelGGL((conv_f16x3_big_kernel<2, true, 1>), dim3((unsigned)((M + BM - 1) / BM), (unsigned)(d.CoutP / 256)), dim3(512), 2 * (BM + 256) * ROWB, st, d, (const char*)wimg, a_scale, os);
    else
      hipLaunchKernelGGL((conv_f16x3_big_kernel<1, true, 1>), dim3((unsigned)((M + BM - 1) / BM), (unsigned)(d.CoutP / 128)), dim3(512), 2 * (BM + 128) * ROWB, st, d, (const char*)wimg, a_scale, os);
    return egne::check_launch("egne_conv2d_f16x3_big_fwd");
  }
  if (d.CoutP % 256 == 0) {
    dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)(d.CoutP / 256));
    if (m16) hipLaunchKernelGGL((conv_f16x3_big_kernel<2, true>), grid, dim3(512), 2 * (BM + 256) * ROWB, st, d, (const char*)wimg, a_scale, os);
    else hipLaunchKernelGGL((conv_f16x3_big_kernel<2, false>), grid, dim3(512), 2 * (BM + 256) * ROWB, st, d, (const char*)wimg, a_scale, os);
  } else {
    dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)(d.CoutP / 128));
    if (m16) hipLaunchKernelGGL((conv_f16x3_big_kernel<1, true>), grid, dim3(512), 2 * (BM + 128) * ROWB, st, d, (const char*)wimg, a_scale, os);
    else hipLaunchKernelGGL((conv_f16x3_big_kernel<1, false>), grid, dim3(512), 2 * (BM + 128) * ROWB, st, d, (const char*)wimg, a_scale, os);
  }
  return egne::check_launch("egne_conv2d_f16x3_big_fwd");
}
