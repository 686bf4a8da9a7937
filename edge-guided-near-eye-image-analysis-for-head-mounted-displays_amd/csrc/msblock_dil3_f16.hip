// The dilated branch of a BDCN MSBlock for an input in SPLIT-PAIR storage, three f16 products per multiply, on maps of 48 x 64 and
// larger -- every tap read from a ring of PHASE-PLANE rows in LDS that is filled by LDS-DMA:
//   out = o + sum_g relu(conv3x3_{dil g}(o) + b_g), g = 0..2, dilations 4 / 8 / 12 (bdcn_new.py:51-54), score heads fused.
// Same operands and per-accumulator order as msdil_ps_kernel<*, 3> (msblock_dil_ps_f16.hip), and the epilogue both take from
// msblock_dil_common.h: the two agree bit for bit; EGNE_MSDIL3=0 (read at every launch) forces the strip kernel.
//
// Why.  The strip kernel stages, per 8 x 32 tile, nine strips global -> registers -> ds_write: 13.5x the tile's own bytes, every pixel
// of o copied about 13 times; it is bound by that copy, not by its MFMAs.  The plain-f16 ring of msblock_dil1_f16.hip (32 rows x 56
// pixels) does not fit with 128-byte pixels.  But the three dilations are multiples of four: pixels interact only inside their residue
// class (y mod 4, x mod 4), and on each of the 16 phase planes -- plane pixel (r, c) of phase (py, px) is frame pixel (4 r + py,
// 4 c + px) -- the group is an ordinary 3 x 3 group with dilations 1 / 2 / 3 and a reach of 3:
//   * a work item is (frame, phase, 32-pixel column of the plane, vertical segment).  The workgroup walks it DOWN in steps of 8 plane
//     rows, wave w owns row w of the step, two 16-pixel blocks per wave (one where the column's last block is empty);
//   * the ring holds three groups of 8 rows x 38 pixels (32 + 2 x 3), hi and lo plane apart: 114 KB.  With groups that start 3 rows
//     above the step, a step reads two groups (8 + 2 x 3 = 14 rows) while the third takes the next 8 rows: 38 LDS-DMA instructions
//     of 1 KB per step and workgroup (1.2x the tile's bytes), no registers, no ds_write, and since live and incoming rows never
//     share a group, no ordering among the taps;
//   * 16-byte chunk c of ring pixel q sits at c ^ ((q >> 1) & 3), the lo plane 64 bytes past a multiple of 128 -- the LDS image of
//     the strip kernel.  The DMA writes LDS linearly, so a lane fetches the chunk its slot holds: the swizzle is in the source address;
//   * pixels outside the plane take the out-of-range offset and read zeros; every wave issues 5 ring instructions per group (the
//     last two of the 40 go to a scratch KB) and 2 weight instructions per sub-step, so the counted vmcnt is uniform;
//   * weights as in the strip kernel: the 12 fragments of (kernel row, dilation) by DMA into one of three 12 KB buffers, two
//     sub-steps ahead, one s_barrier per sub-step (36 MFMAs of a wave).
// Resources (make msblock_dil3_f16.s, gfx950): 183 VGPRs, 0 AGPRs, no VGPR spills, no scratch, 2 waves per SIMD;
// 106 SGPRs, 63 of them parked in lanes of one VGPR (v_writelane / v_readlane) by the per-item and per-step set-up code -- none
// between the barriers of a sub-step; 155 408 bytes of dynamic LDS (one workgroup of 8 waves per CU).
//
// What it is bound by (MI355X, 64 frames of 240 x 320, profiles/msdil3_per_layer_table.txt): 892-900 us against 1 187-1 192 us of the
// strip kernel in the same call, 11.2 us per full-width step against 10.4 k cycles of MFMA issue (648 MFMAs of 16 cycles per SIMD and
// step: ~40 % of the step).  Taking the lo weights off the LDS read path (registers from L1 / L2) made it 4 % slower, taking all weight
// rotation out of LDS (one barrier per step instead of nine, 243 VGPRs) 3 % faster: neither the LDS bandwidth nor the barriers are
// the limit.  What is left is shared between the MFMA pipe, an item's exposed two-group warm-up, the half-empty eighth step of a
// 60-row plane and 1.4 GB of stride-4 pixel traffic per launch; in-kernel stamps are the next step, not another guess.
#include "common.h"
#include "kernel_util.h"
#include "msblock_dil_common.h"
#include <cstdlib>
#include <type_traits>
#include <utility>

namespace {

constexpr int TW = 32, TH = 8, HALO = 3;
constexpr int RPX = TW + 2 * HALO;                                    // 38 pixels per ring row
constexpr int GPX = TH * RPX, GROUPB = GPX * 64;                      // 304 pixel slots, 19 456 bytes per group and plane
constexpr int NGRP = 3, RROWS = NGRP * TH;                            // 24 ring rows
constexpr int PLANEB = NGRP * GROUPB;                                 // 58 368 bytes per plane
constexpr int OFF_LO = PLANEB + 64;                                   // the lo plane: 64 bytes past a multiple of 128
constexpr int RINGB = 2 * PLANEB + 128;
constexpr int WBUFB = 12 * 1024;                                      // [kx 3][ks 2][hi | lo][64 lanes][16 B]
constexpr int OFF_W = RINGB, OFF_DUMMY = OFF_W + 3 * WBUFB, OFF_CONST = OFF_DUMMY + 1024;
constexpr int LDS_BYTES = OFF_CONST + 164 * 4;
constexpr int GK = GPX / 16;                                          // 19 LDS-DMA instructions per group and plane
constexpr int GI = 2 * GK, GJ = 5;                                    // 38 per group: 5 per wave (two of the 40 into the scratch KB)
constexpr int NS = 9;
static_assert(GPX % 16 == 0 && ((GPX >> 1) & 3) == 0, "a group holds whole instructions and leaves the swizzle key alone");
static_assert(GJ * 8 >= GI && LDS_BYTES <= 163840, "LDS budget");

__global__ __launch_bounds__(512)
void msdil3_kernel(const egne_conv_desc p, const _Float16* __restrict__ fhi, const _Float16* __restrict__ flo, float inv_a, float out_scale,
                   int ncols, int nseg, int seg_rows, int nitems, const float* __restrict__ score_w, const float* __restrict__ score_c,
                   float* __restrict__ s0, float* __restrict__ s1, int accumulate) {
  extern __shared__ __attribute__((aligned(1024))) char lds[];
  float* const lconst = (float*)(lds + OFF_CONST);       // [3][32] biases, [2][32] score vectors, [2] constants
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // = the row of a step this wave owns
  const int l15 = lane & 15, kg = lane >> 4;
  const int H = p.H, W = p.W, B = p.B;
  const egne_seg sg = p.seg[0];

  msdil_fill_lconst(lconst, tid, p, score_w, score_c);

  // ---- weights: the 12 fragments of sub-step S = 3 ky + g ((kx, ks) x (hi, lo), 1 KB each) into weight buffer g, two sub-steps ahead
  // of their use: wave w moves fragments w and 8 + (w & 3) (waves 4-7 repeat what waves 0-3 moved: every wave issues exactly two)
  const unsigned wbytes = 3u * 9u * 2u * 1024u;
  const __amdgpu_buffer_rsrc_t rwh = make_rsrc(fhi, wbytes), rwl = make_rsrc(flo, wbytes);
  auto dma_weights = [&](auto sc) {
    constexpr int S = decltype(sc)::value, g = S % 3, ky = S / 3;
    char* wb = lds + OFF_W + g * WBUFB;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int j = t == 0 ? wave : 8 + (wave & 3), f = j >> 1;
      const int o = ((g * 9 + ky * 3 + (f >> 1)) * 2 + (f & 1)) * 1024;
      __builtin_amdgcn_raw_ptr_buffer_load_lds((j & 1) ? rwl : rwh, (lds_ptr)(wb + j * 1024), 16, lane * 16, o, 0, 0);
    }
  };

  // ---- ring fill.  A group is 304 pixel slots per plane (row-major over 8 x 38) = 19 instructions of 16 slots, hi plane then lo plane;
  // wave w issues instructions 5 w .. 5 w + 4.  Lane l of instruction k: slot 16 (k % 19) + (l >> 2), LDS chunk l & 3, which holds the
  // pixel's chunk (l & 3) ^ key(slot)
  int rel[GJ], rr[GJ], cc[GJ];
#pragma unroll
  for (int j = 0; j < GJ; ++j) {
    const int k = wave * GJ + j, plane = k >= GK, kk = k - plane * GK;
    const int slot = 16 * kk + (lane >> 2);
    const int r = slot / RPX, c = slot - r * RPX;
    rr[j] = k < GI ? r : -100000;
    cc[j] = c - HALO;
    rel[j] = ((r * W + c - HALO) * 4 * (int)sg.pix_stride + sg.ch_off) * 4 + plane * 64 + (((lane & 3) ^ ((slot >> 1) & 3)) << 4);
  }
  // read side: lane (l15, kg) reads chunk kg of ring pixel q = 38 * ring row + column + l15
  const int wl = ((kg >> 1) * 1024 + ((kg & 1) * 32 + l15) * 8) * 2;      // + kx * 4096 + hl * 1024 + nh * 256 (bytes)

  const unsigned frame_in = (unsigned)H * W * (unsigned)sg.pix_stride * 4u;
  const unsigned frame_out = (unsigned)H * W * (unsigned)p.out_pix_stride * 4u;
  bool ovf_bad = false;

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  dma_weights(I0{});
  dma_weights(I1{});

  for (int it = (int)blockIdx.x; it < nitems; it += (int)gridDim.x) {
    // (column slowest: a workgroup's items run from the full columns to the last, possibly narrower one)
    const int sgi = it % nseg, r1 = it / nseg, phase = r1 & 15, r2 = r1 >> 4, b = r2 % B, cx = r2 / B;
    const int py = phase >> 2, px = phase & 3;
    const int Hp = (H - py + 3) >> 2, Wp = (W - px + 3) >> 2;             // this phase's plane
    const int C0 = cx * TW, ys = sgi * seg_rows;
    const int ye = ys + seg_rows < Hp ? ys + seg_rows : Hp;
    if (ys >= ye || C0 >= Wp) continue;                                   // (workgroup-uniform)
    const int nst = (ye - ys + TH - 1) / TH;
    const bool two = Wp - C0 > 16;
    const __amdgpu_buffer_rsrc_t rin = make_rsrc(sg.ptr + (long long)b * H * W * sg.pix_stride, frame_in);
    const __amdgpu_buffer_rsrc_t rout = make_rsrc(p.out ? p.out + (long long)b * H * W * p.out_pix_stride : nullptr, p.out ? frame_out : 0u);
    // plane rows Rg .. Rg + 7 (zeros outside the plane) into ring group `slot`
    auto issue_group = [&](int Rg, int slot, bool on) {
      const int sbase = ((4 * Rg + py) * W + 4 * C0 + px) * (int)sg.pix_stride * 4;
#pragma unroll
      for (int j = 0; j < GJ; ++j) {
        const bool ok = on && (unsigned)(Rg + rr[j]) < (unsigned)Hp && (unsigned)(C0 + cc[j]) < (unsigned)Wp;
        const int k = wave * GJ + j;
        char* dst = k < GI ? lds + (k >= GK ? OFF_LO - GK * 1024 : 0) + slot * GROUPB + k * 1024 : lds + OFF_DUMMY;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rin, (lds_ptr)dst, 16, ok ? rel[j] + sbase : (int)OOB, 0, 0, 0);
      }
    };
    // (the barrier that ended the previous item's last sub-step: its reads of the ring are done)
    issue_group(ys - HALO, 0, true);
    issue_group(ys - HALO + TH, 1, true);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();

    int t3 = 0;
    for (int t = 0; t < nst; ++t) {
      const int y0 = ys + TH * t;
      // ring row of plane row R: (R - ys + 3) % 24; a tap of kernel row ky and plane dilation dd reads row y0 + wave + (ky - 1) dd:
      // seven classes j = 3 + (ky - 1) dd
      int qrow[7];
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        int rho = TH * t3 + wave + j;
        rho = rho >= RROWS ? rho - RROWS : rho;
        qrow[j] = rho * RPX + l15;
      }
      const int gnext = t3 == 0 ? 2 : t3 - 1;                  // group (t + 2) % 3: the one the previous step read last
      const bool more = t + 1 < nst;

      auto step = [&](auto nphc) {
        constexpr int NPH = decltype(nphc)::value;
        f32x4 acc[3][2][2];
        h8 resh[2], resl[2];          // o itself: the operands of the centre tap ARE the lane's 8 channels of its two pixels
        float* sdst = nullptr;
        float sprev = 0.f;

        auto compute = [&](auto sc) {
          constexpr int S = decltype(sc)::value, g = S % 3, ky = S / 3, dd = g + 1, jr = 3 + (ky - 1) * dd;
          const char* wb = lds + OFF_W + g * WBUFB + wl;
          if constexpr (ky == 0) {
#pragma unroll
            for (int a = 0; a < 4; ++a) (&acc[g][0][0])[a] = (f32x4)(0.f);
          }
          h8 wh[2], wo[2], ah[2][2], al[2][2];
          auto fetch_w = [&](auto kc) {
            constexpr int KX = decltype(kc)::value;
#pragma unroll
            for (int nh = 0; nh < 2; ++nh) {
              wh[nh] = *(const h8*)(wb + KX * 4096 + nh * 256);
              wo[nh] = *(const h8*)(wb + KX * 4096 + 1024 + nh * 256);
            }
          };
          auto fetch = [&](auto kc) {
            constexpr int KX = decltype(kc)::value, Bq = KX & 1;
#pragma unroll
            for (int ph = 0; ph < NPH; ++ph) {
              const int qq = qrow[jr] + (HALO + (KX - 1) * dd + 16 * ph);
              const int o = qq * 64 + ((kg ^ ((qq >> 1) & 3)) << 4);
              ah[Bq][ph] = *(const h8*)(lds + o);
              al[Bq][ph] = *(const h8*)(lds + OFF_LO + o);
            }
          };
          fetch(I0{});
          [&]<int... Ks>(std::integer_sequence<int, Ks...>) {
            (([&] {
              constexpr int kx = Ks, Bq = kx & 1;
              fetch_w(std::integral_constant<int, kx>{});
              if constexpr (kx + 1 < 3) fetch(std::integral_constant<int, kx + 1>{});
              if constexpr (S == 3 && kx == 1) {
#pragma unroll
                for (int ph = 0; ph < NPH; ++ph) { resh[ph] = ah[1][ph]; resl[ph] = al[1][ph]; }
              }
              __builtin_amdgcn_sched_barrier(0);
              // three products per accumulator (lo w_hi, hi w_lo, hi w_hi), the accumulators interleaved
#pragma unroll
              for (int ph = 0; ph < NPH; ++ph)
#pragma unroll
                for (int nh = 0; nh < 2; ++nh) acc[g][ph][nh] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[nh], al[Bq][ph], acc[g][ph][nh], 0, 0, 0);
#pragma unroll
              for (int ph = 0; ph < NPH; ++ph)
#pragma unroll
                for (int nh = 0; nh < 2; ++nh) acc[g][ph][nh] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wo[nh], ah[Bq][ph], acc[g][ph][nh], 0, 0, 0);
#pragma unroll
              for (int ph = 0; ph < NPH; ++ph)
#pragma unroll
                for (int nh = 0; nh < 2; ++nh) acc[g][ph][nh] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[nh], ah[Bq][ph], acc[g][ph][nh], 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
            }()), ...);
          }(std::make_integer_sequence<int, 3>{});
        };

        // epilogue of the step's row: lane holds channels n = 16 nh + 4 kg + e of plane pixel (y0 + wave, C0 + 16 ph + l15)
        auto epilogue = [&] {
          const int R = y0 + wave, y = 4 * R + py;
          int pix[2] = {0, 0};
          bool okp[2] = {false, false};
#pragma unroll
          for (int ph = 0; ph < NPH; ++ph) {
            const int Cq = C0 + ph * 16 + l15, x = 4 * Cq + px;
            okp[ph] = R < Hp && Cq < Wp;
            pix[ph] = y * W + x;
          }
          msdil_epilogue<NPH, true>(p, lconst, acc, resh, resl, pix, okp, rout, inv_a, out_scale, kg, score_w, sdst, sprev, accumulate, ovf_bad);
        };

        // sub-step S: [weights of S + 2 -> LDS] [S = 0: the next 8 rows -> the free ring group] [36 MFMAs] [wait for the weights of
        // S + 1] [S = 8: epilogue] [barrier].  Loads retire in order, so a wait allows the LOADS this wave issued after those weights
        // (stores count too, but only ever make a wait longer); no wait stands behind the epilogue's stores, or every step would
        // expose their latency.
        [&]<int... Ss>(std::integer_sequence<int, Ss...>) {
          (([&] {
            constexpr int S = Ss, S2 = (S + 2) % NS;
            dma_weights(std::integral_constant<int, S2>{});
            if constexpr (S == 0) issue_group(y0 + 2 * TH - HALO, gnext, more);
            if constexpr (S == NS - 1) {
              // the running score sums (lane (l15, kg) finishes head kg >> 1 of pixel block kg & 1); unconditional load
              const int R = y0 + wave, Cq = C0 + (kg & 1) * 16 + l15;
              msdil_score_prefetch(p, score_w, s0, s1, kg, b, 4 * R + py, 4 * Cq + px, R < Hp && Cq < Wp, sdst, sprev);
            }
            compute(std::integral_constant<int, S>{});
            // S = 8: everything, i.e. the weights of the next step's sub-steps 0 AND 1 (a sub-step old) and the score load, in front
            // of the stores -- so S = 0 waits for nothing; S = 1: the ring group (5) and this sub-step's weights may stay in flight;
            // S = 2: the group has to land anyway (needed behind sub-step 8, it has had three sub-steps)
            if constexpr (S == NS - 1) {
              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
              epilogue();
            } else if constexpr (S == 1) {
              asm volatile("s_waitcnt vmcnt(%0)" :: "n"(GJ + 2) : "memory");
            } else if constexpr (S > 1) {
              asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            }
            lds_barrier();
          }()), ...);
        }(std::make_integer_sequence<int, NS>{});
      };
      if (two) step(std::integral_constant<int, 2>{});
      else step(I1{});
      t3 = t3 == 2 ? 0 : t3 + 1;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  egne_ovf_commit(ovf_bad, p.ovf_flag);
}

}  // namespace

namespace egne {

bool msdil3_wanted(const egne_conv_desc& d) {
  const char* e = getenv("EGNE_MSDIL3");                   // (read per launch: the tests compare both forms inside one process)
  return !(e && atoi(e) == 0) && d.f16_products != 1 && d.seg[0].presplit == 1 && d.W >= 64 && d.H >= 48;
}

// Called by egne_msblock_dil_scores_f16_fwd, which has validated the descriptor, for three-product operands on maps of 48 x 64 and
// larger.  Work items: (frame, phase, 32-pixel plane column, vertical segment), sized by the largest plane (phase 0, 0); a segment pays
// about one step for its two exposed ring groups.  EGNE_MSDIL3_SEGS = 1..4 (read per launch) forces a segment count (tests).
int msdil3_launch(const egne_conv_desc& d, const void* fhi, const void* flo, float a_scale, float w_scale, const float* score_w,
                  const float* score_c, float* s0, float* s1, int accumulate, hipStream_t st) {
  static_assert(TH == 8, "msdil_segments counts steps of 8 rows");
  const char* e = getenv("EGNE_MSDIL3_SEGS");
  const int Hp = (d.H + 3) / 4, Wp = (d.W + 3) / 4, ncols = (Wp + TW - 1) / TW;
  const msdil_segs sg = msdil_segments(Hp, (long long)d.B * 16 * ncols, 1.0, e ? atoi(e) : 0);
  const long long nitems = (long long)d.B * 16 * ncols * sg.nseg;
  if (nitems > 0x7fffffff - 256) return egne::fail(EGNE_ERR_ARG, "msblock_dil (phase-plane ring): %lld work items", nitems);
  if (!egne::raise_lds((const void*)msdil3_kernel, LDS_BYTES))
    return egne::fail(EGNE_ERR_LAUNCH, "msblock_dil (phase-plane ring): cannot raise the dynamic LDS limit to %d", LDS_BYTES);
  const msdil_scales sc = msdil_scales_of(a_scale, w_scale);
  hipLaunchKernelGGL(msdil3_kernel, dim3((unsigned)(nitems < 256 ? nitems : 256)), dim3(512), LDS_BYTES, st, d, (const _Float16*)fhi,
                     (const _Float16*)flo, sc.inv_a, sc.os, ncols, sg.nseg, sg.seg_rows, (int)nitems, score_w, score_c, s0, s1, accumulate);
  return egne::check_launch("egne_msblock_dil_f16_fwd (phase-plane ring)");
}

}  // namespace egne
