// What the three transposed-product kernels of the dilated MSBlock branch share -- msdil_ps_kernel (strips, msblock_dil_ps_f16.hip),
// msdil1_kernel (plain-f16 ring, msblock_dil1_f16.hip) and msdil3_kernel (phase-plane ring, msblock_dil3_f16.hip): the constants
// they keep in LDS, the prefetch of the running score sums and the epilogue.  All three end a tile row with a lane (l15, kg) holding
// channels n = 16 nh + 4 kg + e of up to two 16-pixel blocks ph, one f32x4 per (dilation, ph, nh); they agree bit for bit because
// every value they store comes out of the ONE set of expressions below (-ffp-contract=on decides contraction per expression).
// msblock_dil_kernel (fp32 input, 32x32 MFMAs, msblock_dil_f16.hip) has another lane layout and an epilogue of its own.
#pragma once
#include "common.h"
#include "kernel_util.h"

// lconst: [3][32] biases, [2][32] score vectors, [2] score constants (162 floats; zeros where the descriptor has none): the epilogue
// issues no vector memory loads.  Threads 0 .. 161 of the workgroup fill it; a barrier stands between this and the first epilogue.
__device__ __forceinline__ void msdil_fill_lconst(float* lconst, int tid, const egne_conv_desc& p, const float* score_w, const float* score_c) {
  if (tid < 160) {
    const int r = tid >> 5, c = tid & 31;
    lconst[tid] = r < 3 ? (p.bias ? p.bias[r * p.CoutP + c] : 0.f) : (score_w ? score_w[(r - 3) * 32 + c] : 0.f);
  } else if (tid < 162) {
    lconst[tid] = score_c ? score_c[tid - 160] : 0.f;
  }
}

// The running score sum this lane will finish: lane (l15, kg) ends head kg >> 1 of pixel block kg & 1, whose frame pixel is (y, x) of
// frame b (`ok`: inside the map).  The load is UNCONDITIONAL (lanes without a sum read the residual's first word): the kernels count
// their loads in flight by instruction.
__device__ __forceinline__ void msdil_score_prefetch(const egne_conv_desc& p, const float* score_w, float* s0, float* s1, int kg, int b, int y,
                                                     int x, bool ok, float*& sdst, float& sprev) {
  const int h = kg >> 1;
  sdst = (score_w && ok) ? (h ? s1 : s0) + ((long long)b * p.H + y) * p.W + x : nullptr;
  sprev = *(sdst ? (const volatile float*)sdst : (const volatile float*)p.residual);
}

// Epilogue of a tile row.  NPH: pixel blocks of the row (block 1 of msdil3_kernel can be empty); LO: the residual has a lo plane.
//   acc[g][ph][nh]   accumulators of dilation g;  resh / resl[ph]: the centre tap's operands = the lane's 8 channels of o * a_scale
//                    (positions 8 kg .. 8 kg + 7 of either plane = channels {4 kg ..} and {16 + 4 kg ..}, engine.SPLIT_PAIR_PERM)
//   pix / okp[ph]    index of the block's pixel inside its frame, and whether it lies inside the map;  rout: the frame of p.out
//   sdst / sprev     from msdil_score_prefetch
// bias + ReLU per dilation, o + o1 + o2 + o3 (bdcn_new.py:54), 16-byte stores, the block's share of the stage's two score maps.
template <int NPH, bool LO>
__device__ __forceinline__ void msdil_epilogue(const egne_conv_desc& p, const float* lconst, const f32x4 (&acc)[3][2][2], const h8 (&resh)[2],
                                               const h8 (&resl)[2], const int (&pix)[2], const bool (&okp)[2], __amdgpu_buffer_rsrc_t rout,
                                               float inv_a, float out_scale, int kg, const float* score_w, float* sdst, float sprev,
                                               int accumulate, bool& ovf_bad) {
  f32x4 bq[3][2], cwq[2][2];
#pragma unroll
  for (int nh = 0; nh < 2; ++nh) {
    const int n = nh * 16 + 4 * kg;
#pragma unroll
    for (int g = 0; g < 3; ++g) bq[g][nh] = *(const f32x4*)&lconst[g * 32 + n];
#pragma unroll
    for (int h = 0; h < 2; ++h) cwq[h][nh] = *(const f32x4*)&lconst[(3 + h) * 32 + n];
  }
  float sc[2][2];                                      // [head][ph]
  sc[0][1] = sc[1][1] = 0.f;
#pragma unroll
  for (int ph = 0; ph < NPH; ++ph) {
    sc[0][ph] = sc[1][ph] = 0.f;
#pragma unroll
    for (int nh = 0; nh < 2; ++nh) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // (plain f16 operands: the residual is the hi half alone; the + 0.f keeps the rounding steps of the two-plane form)
        const float o = ((float)resh[ph][nh * 4 + e] + (LO ? (float)resl[ph][nh * 4 + e] : 0.f)) * inv_a;
        v[e] = fmaxf(acc[0][ph][nh][e] * out_scale + bq[0][nh][e], 0.f) + fmaxf(acc[1][ph][nh][e] * out_scale + bq[1][nh][e], 0.f) +
               fmaxf(acc[2][ph][nh][e] * out_scale + bq[2][nh][e], 0.f) + o;
        sc[0][ph] += v[e] * cwq[0][nh][e];
        sc[1][ph] += v[e] * cwq[1][nh][e];
        // (fmaxf(x, 0) swallows NaN and -inf: the overflow test takes the accumulators themselves; lane = pixel: one channel per
        //  pixel, common.h)
        if (nh == 0 && e == 0) ovf_bad |= egne_nonfinite(acc[0][ph][nh][e] + acc[1][ph][nh][e] + acc[2][ph][nh][e] + o);
      }
      if (p.out) {
        const int n = nh * 16 + 4 * kg;
        const int oo = (okp[ph] && n < p.Cout_store) ? (pix[ph] * (int)p.out_pix_stride + p.out_ch_off + n) * 4 : (int)OOB;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rout, oo, 0, 0);
      }
    }
  }
  if (score_w) {
    // bdcn_new.py:118-166 is linear behind the block: per block and head ONE 32-vector.  8 channels were summed in the lane, the other
    // 24 sit in lanes l15 + 16, + 32, + 48 -- two exchanges, fixed order
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int ph = 0; ph < NPH; ++ph) {
        float t = sc[h][ph];
        t += __shfl_xor(t, 16);
        t += __shfl_xor(t, 32);
        sc[h][ph] = t;
      }
    const int h = kg >> 1, ph = kg & 1;
    const float v = h ? (ph ? sc[1][1] : sc[1][0]) : (ph ? sc[0][1] : sc[0][0]);
    if (sdst) *sdst = v + (accumulate ? sprev : lconst[160 + h]);
  }
}

namespace egne {

// ---- host side ----------------------------------------------------------------------------------------------------------------
// The launchers egne_msblock_dil_scores_f16_fwd (msblock_dil_f16.hip) chooses between for a split-pair input, in its order; *_wanted:
// the form takes this descriptor (and its switch EGNE_MSDIL1 / EGNE_MSDIL3, read at every launch, does not say 0).
bool msdil1_wanted(const egne_conv_desc& d);      // msblock_dil1_f16.hip: plain f16 operands, ring of rows
int msdil1_launch(const egne_conv_desc& d, const void* fhi, float a_scale, float w_scale, const float* score_w, const float* score_c,
                  float* s0, float* s1, int accumulate, hipStream_t st);
bool msdil3_wanted(const egne_conv_desc& d);      // msblock_dil3_f16.hip: three products, ring of phase-plane rows
int msdil3_launch(const egne_conv_desc& d, const void* fhi, const void* flo, float a_scale, float w_scale, const float* score_w,
                  const float* score_c, float* s0, float* s1, int accumulate, hipStream_t st);
int msdil_ps_launch(const egne_conv_desc& d, const void* fhi, const void* flo, float a_scale, float w_scale, const float* score_w,
                    const float* score_c, float* s0, float* s1, int accumulate, hipStream_t st);   // msblock_dil_ps_f16.hip: strips

struct msdil_scales { float os, inv_a; };      // accumulator -> output, f16 operand -> o
inline msdil_scales msdil_scales_of(float a_scale, float w_scale) { return {1.0f / (a_scale * w_scale), 1.0f / a_scale}; }

// Vertical segments of the ring kernels' work items.  A workgroup walks a column of `extent` rows down in steps of 8 rows; a column is
// cut into up to four segments where whole columns would leave compute units without work.  per_seg: work items per segment of a
// column (frames x columns [x phases]); warmup: what filling the ring costs a segment, in steps; force = 1 .. 4 takes that count
// where it leaves no segment empty.  Cost model: rounds of 256 workgroups x (steps + warm-up) of a segment.
struct msdil_segs { int nseg, seg_rows; };
inline msdil_segs msdil_segments(int extent, long long per_seg, double warmup, int force) {
  int best = 1;
  double best_t = 1e30;
  for (int ns = 1; ns <= 4; ++ns) {
    const int rows = ((extent + ns - 1) / ns + 7) / 8 * 8;
    if (ns > 1 && rows * (ns - 1) >= extent) continue;          // an empty last segment
    const long long items = per_seg * ns;
    const double t = (double)((items + 255) / 256) * (rows / 8 + warmup);
    if (force == ns) { best = ns; break; }
    if (t < best_t) { best_t = t; best = ns; }
  }
  return {best, ((extent + best - 1) / best + 7) / 8 * 8};
}

}  // namespace egne
