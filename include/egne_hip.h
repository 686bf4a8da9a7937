/*
 * egne_hip.h -- C-ABI of the MI355X (gfx950) hot path of edge-guided near-eye segmentation.
 *
 * The reference (zhaoyuhsin/Edge-Guided-Near-Eye-Image-Analysis-for-Head-Mounted-Displays) has no
 * FFI layer of its own: its hot path is a chain of PyTorch ATen calls made from Python
 * (SURVEY.md section 2.3).  Each entry point below therefore names the reference call site(s)
 * whose ATen op(s) it replaces (file:line under /root/reference).  The Python host in
 * edge-guided-near-eye-image-analysis-for-head-mounted-displays_amd/ binds these with ctypes
 * (_lib.py); INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative egne_status otherwise; egne_last_error()
 *     returns a message for the calling thread;
 *   - all pointers are DEVICE pointers owned by the caller, nothing is allocated or freed here;
 *   - activations are fp32 NHWC; a tensor is addressed as (base pointer, floats per pixel,
 *     first channel, channel count) so that torch.cat never has to materialise: producers write
 *     into channel slices of a shared buffer and consumers read up to EGNE_MAXSEG slices;
 *   - channel counts of slices are padded to a multiple of 8 with zero weights / zero data;
 *   - `stream` is a hipStream_t passed as void*; kernels are asynchronous on it.
 */
#ifndef EGNE_HIP_H
#define EGNE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EGNE_MAXSEG 8
#define EGNE_MAXGROUP 3

typedef enum {
  EGNE_OK = 0,
  EGNE_ERR_ARG = -1,     /* shape / alignment / range check failed on the host side */
  EGNE_ERR_LAUNCH = -2,  /* hipLaunchKernel or a runtime call failed */
  EGNE_ERR_NODEVICE = -3
} egne_status;

typedef enum { EGNE_ACT_NONE = 0, EGNE_ACT_RELU = 1, EGNE_ACT_LEAKY = 2 } egne_act;

/* One input slice of a convolution (a piece of a would-be torch.cat). */
typedef struct {
  const float* ptr;     /* NHWC base of the buffer that holds the slice */
  int64_t pix_stride;   /* floats per pixel of that buffer */
  int32_t ch_off;       /* first channel of the slice (multiple of 4) */
  int32_t Cp;           /* padded channel count of the slice (multiple of 8) */
  const float* scale;   /* optional per-(n,c) affine applied while loading: x*scale+shift  */
  const float* shift;   /*   ([B][Cp], used to fuse InstanceNorm / BatchNorm into the consumer) */
  int32_t act_in;       /* egne_act applied after the affine (LeakyReLU of Transition_down) */
  int32_t presplit;     /* 1: the slice is held in SPLIT-PAIR storage (see egne_conv_desc.out_split), written with the scale that is
                         * passed as this launch's a_scale; honoured by egne_msblock_dil(_scores)_f16_fwd only, 0 everywhere else.
                         * 2: the slice is held as F16 (out_split = 2 of its producer; ptr at halfs, pix_stride / ch_off in halfs, multiples
                         * of 8), written with this launch's a_scale: egne_conv3x3_rw_f16_fwd with f16_products = 1 only.
                         * 3: the slice is held in split-pair storage in CHANNEL order (out_split = 3 of its producer), written with this launch's
                         * a_scale: egne_conv2d_f16x3_big_fwd, egne_conv2d_f16x3_fwd (128-wide layers), egne_conv3x3_halo_f16_fwd (32 outputs,
                         * dilation 1).  Every other split-f16 entry point rejects the value. */
} egne_seg;

/*
 * Implicit-GEMM convolution, fp32 in / fp32 accumulate on v_mfma_f32_32x32x2_f32.
 * Replaces F.conv2d at: vgg16_c.py:66-78 (3x3, dilation 1/2), bdcn_new.py:50-53 (3x3 + three
 * dilated 3x3 of MSBlock, fused as `ngroups`=3 with the 4-way sum of :54 as `residual`),
 * utils.py:1047-1048 (convBlock), models/RITnet_v2.py:57-62,41 (down block 3x3 / concat-free
 * 1x1 / Transition_down), :85-87 (up block), utils.py:1016-1019 (regressionModule convs),
 * utils.py:1020-1021 (its Linear layers, as 1x1 convs), models/RITnet_v2.py:91-121 (StyleEncoder
 * with reflect padding, MLP).
 */
typedef struct {
  int32_t B, H, W;            /* input batch / height / width */
  int32_t Ho, Wo;             /* output height / width */
  int32_t kh, kw, stride;
  int32_t pad_h, pad_w;       /* padding for dilation 1; group g pads by pad*dil[g] */
  int32_t pad_mode;           /* 0 zero, 1 reflect */
  int32_t ngroups;            /* 1, or 3 for the fused MSBlock dilated branch */
  int32_t dil[EGNE_MAXGROUP];
  int32_t nseg;
  egne_seg seg[EGNE_MAXSEG];
  int32_t Ktot;               /* sum of seg[i].Cp */
  int32_t CoutP;              /* rows of the packed weight, multiple of 32 */
  const float* w;             /* packed [group][tap][CoutP][Ktot], zero padded */
  const float* bias;          /* [group][CoutP], zero padded (may be NULL) */
  int32_t act;                /* egne_act applied to (acc + bias) of every group */
  const float* post_scale;    /* optional per-channel affine after act (eval BatchNorm) [CoutP] */
  const float* post_shift;
  const float* residual;      /* optional tensor added last (same pixels as the output) */
  int64_t res_pix_stride;
  int32_t res_ch_off;
  float* out;
  int64_t out_pix_stride;
  int32_t out_ch_off;
  int32_t Cout_store;         /* channels written (logical Cout rounded up to the slice's padding) */
  /* Optional (egne_conv3x3_halo_f16_fwd, egne_conv1x1_3x3_fused_f16_fwd; round 5: egne_conv3x3_bf16_fwd): per-(frame, chunk, channel) partial sums of the
   * STORED output values, [B][stats_nchunk][Cout_store][2] doubles (sum, sum of squares), for a following
   * egne_norm_stats_finish -- the InstanceNorm statistics of the consumer (models/RITnet_v2.py:40,57) without another
   * pass over the tensor.  A chunk is one wave's rows of one tile: stats_nchunk = ceil(W/32) * ceil(H/8) * 4. */
  double* stats_ws;
  int32_t stats_nchunk;
  /* Optional (egne_conv3x3_rs_f16_fwd, shapes whose consumer waves own two tile rows): second output = the 2x2 / stride 2 /
   * ceil-mode max pooling of the stored result (vgg16_c.py:70 pool1 behind conv1_2), [B][ceil(H/2)][ceil(W/2)] pixels of
   * pool_pix_stride floats, Cout_store channels from pool_ch_off; needs a monotonic activation and no post affine. */
  float* pool_out;
  int64_t pool_pix_stride;
  int32_t pool_ch_off;
  /* Optional (egne_conv3x3_halo_f16_fwd, egne_conv3x3_rs_f16_fwd, egne_conv3x3_rw_f16_fwd, egne_conv2d_f16x3_fwd): the
   * activation pre-scale of the split taken ON THE DEVICE from this word = bit pattern of max |x| of the input (written by
   * egne_absmax on the same stream): a_scale = the power of two that puts it in [1024, 2048); the a_scale argument is then
   * ignored (pass 1).  Training plans use it: their weights move every step, so a host-side calibration would cost a
   * synchronisation per launch and step.  Zero / denormal maxima leave a_scale = 1. */
  const uint32_t* dyn_scale;
  /* Optional (egne_conv2d_fwd, the exact-fp32 implicit GEMM): atomic max of the bit patterns of |stored value| into this word
   * (cleared by the caller) -- the dyn_scale word of the split-f16 launch that reads this output next, without another pass
   * over the tensor. */
  uint32_t* absmax_out;
  /* Storage type of the ACTIVATION tensors of this call: 0 = fp32 (everything above as declared), 1 = bf16 -- seg[i].ptr, out,
   * residual and pool_out (and the gz argument of the weight-gradient entry points) then point at bf16 elements; strides and
   * offsets stay in ELEMENTS, slices must start on multiples of 4 elements.  Weights, bias, affine tables and statistics stay
   * fp32, accumulation is fp32 (training plans with bf16 activation storage: BASELINE.json configs[2..4]).  Honoured by
   * egne_conv2d_fwd, egne_conv3x3_smallcin_fwd, egne_conv2d_wgrad, egne_conv3x3_bf16_fwd; every other convolution entry
   * point requires 0. */
  int32_t dtype;
  /* Optional (egne_conv3x3_rw_f16_fwd): SPLIT-PAIR storage of the output.  The split-f16 kernels multiply every fp32 element by a
   * power of two s and split it into hi = f16(x s), lo = f16(x s - hi) while staging it; a tensor whose ONLY consumer stages each
   * element many times (bdcn_new.py:50-54: `o` of an MSBlock feeds three dilated 3x3 convolutions, 13.5 stagings per element)
   * is written in that form once, by its producer: per pixel and 32-channel block 128 bytes = [hi x 32 | lo x 32] halves instead
   * of 32 floats (same bytes, same strides / offsets in units of 4 bytes; out_ch_off and Cout_store whole blocks); position p of
   * either plane holds channel 16 * ((p >> 2) & 1) + 4 * (p >> 3) + (p & 3) of the block (the order the producer's lanes end
   * with, so that a lane stores 16 contiguous bytes per plane) and the consumer's weights are packed in that order.  The consumer
   * (seg.presplit = 1) copies 16-byte pieces straight into its LDS operand image and recovers x = (hi + lo) / s where it needs
   * the value itself (the 4-way sum of bdcn_new.py:54), exact to 2^-22 |x|.
   * out_split = 2 (egne_conv3x3_rw_f16_fwd and egne_conv3x3_smallcin_f16_fwd with f16_products = 1; round 6): F16 storage -- the output
   * (and egne_conv3x3_rw_f16_fwd's pooled second output) is written as f16(v s), one half per element in CHANNEL order; `out` /
   * `pool_out` then point at halfs, strides and offsets count halfs (slices on multiples of 8).  A plain-f16 consumer rounds its operand to
   * exactly this value while staging it (f16(x a_scale), a_scale = s), so the stored tensor carries everything the consumer would have
   * kept at half the bytes: conv1_1 / conv1_2 / pool1 of the frozen edge network next to a bf16-storage training plan
   * (vgg16_c.py:66-70 under utils.py:646).  Consumers read it through seg.presplit = 2 with a_scale = s.
   * out_split = 3 (egne_conv2d_f16x3_big_fwd, egne_conv2d_f16x3_fwd on 128-wide layers; three products): split-pair storage with both planes in
   * CHANNEL order -- position p of either plane holds channel p of the block (the deep trunk kernel's lanes trade halves so that each stores 16 bytes per plane).  The wide trunk tensors
   * conv3_1 .. conv5_3, pool3, pool4 of the calibrated inference plan of the edge network (vgg16_c.py:72-88): their readers stage an element 9-18
   * times and would derive the same pair every time; with this storage they copy it (the deep trunk kernel by LDS-DMA) and multiply the same
   * operands in the same order as over the fp32 tensor, so the results are bit-identical.  s is the pre-scale the readers would use:
   * the power of two that puts max |x| of the tensor in [1024, 2048).  Read through seg.presplit = 3 with a_scale = s; pooled by
   * egne_maxpool2_split. */
  int32_t out_split;
  float out_split_scale;      /* s > 0, a power of two */
  /* Optional (every split-f16 entry point): sticky overflow word.  The kernel sets bit 0 when a value it stores is not finite --
   * the trace of an operand that left the f16 range under the launch's calibrated pre-scale (or of non-finite input).  The
   * caller clears it, reads it behind the launches it covers and answers by re-calibrating (engine.Plan.check_overflow). */
  uint32_t* ovf_flag;
  /* Optional (egne_conv2d_f16x3_big_fwd, egne_msblock_dil(_scores)_f16_fwd on split-pair input, egne_conv3x3_rw_f16_fwd): products per
   * multiply of the split-f16 arithmetic.  0 / 3: a b ~= hi hi + hi lo + lo hi (22-bit significand, the inference plans and every
   * fp32-storage plan).  1: hi hi only -- plain f16 operands (11-bit significand), fp32 accumulation: the frozen edge network next
   * to a training plan with BF16 activation storage (BASELINE.json configs[2..4]), whose input the edge map is rounded to bf16
   * (8-bit significand) anyway.  Entry points that do not know the field compute all three products. */
  int32_t f16_products;
  /* Optional (egne_conv3x3_bf16_fwd used as a DATA GRADIENT, round 5): the launch is the last writer of a gradient slice and applies the
   * activation mask of the layer whose OUTPUT the slice is the gradient of -- stored value = v * act'(y), y = that layer's activated
   * output (bf16, same pixels and channels; mask_act = its egne_act) -- and leaves the channel sums of what it stored for that layer's
   * bias gradient: mask_sums [egne_conv3x3_bf16_sum_rows()][Cout_store] floats, one row per consumer wave (zero-initialised by the caller:
   * a wave writes the 32 channels of its output block only), added by egne_group_sums_reduce in a fixed order.  Replaces an
   * egne_act_bwd_bias pass (read g, read y, write g) over the slice. */
  const void* mask_y; int64_t mask_pix_stride; int32_t mask_ch_off; int32_t mask_act;
  float* mask_sums;
} egne_conv_desc;

int egne_conv2d_fwd(const egne_conv_desc* d, void* stream);
int egne_conv3x3_bf16_sum_rows(void);      /* rows of egne_conv_desc.mask_sums a launch of egne_conv3x3_bf16_fwd writes */

/*
 * Fast path for the 3x3 / stride 1 / "same" / dilation<=2 / single-slice convolutions (most of
 * vgg16_c.py:66-78, utils.py:1047-1048 and the 3x3s of models/RITnet_v2.py:57-62,85-87): the input halo
 * tile is staged once per 32 channels in LDS and all 9 taps run from it.  Same descriptor as
 * egne_conv2d_fwd, except that `w` must be the FRAGMENT-order pack of egne_pack_conv_weight_frag
 * ([tap][Ktot/8][CoutP/32][lane][4], each wave's B fragment is one coalesced 1-KiB load).
 */
int egne_conv3x3_halo_supported(const egne_conv_desc* d);
int egne_conv3x3_halo_fwd(const egne_conv_desc* d, void* stream);
int egne_pack_conv_weight_frag(const float* w_oihw, int Cout, int Cin, int kh, int kw,
                               const int32_t* kinv, int CoutP, int Ktot, float* w_packed, void* stream);

/*
 * Split-precision convolution for the FROZEN edge extractor (vgg16_c.py:66-78, bdcn_new.py:50): fp32 tensors,
 * every operand split into two f16 halves (22-bit significand), three v_mfma_f32_32x32x16_f16 per product,
 * fp32 accumulation -- 5.3x the matrix rate of the exact-fp32 MFMA.  Same descriptor as egne_conv2d_fwd
 * (`w` unused; CoutP = row count of the f16 pack, Ktot = slice width rounded up to 32).  One input slice
 * (fused affine allowed), stride 1, zero padding; ngroups = 3 fuses the MSBlock dilated branch.  a_scale / w_scale: exact power-of-two pre-scales that keep
 * the low halves in the f16 normal range (w_scale is baked into the pack).
 */
int egne_pack_conv_weight_f16x2(const float* w_oihw, int Cout, int Cin, int kh, int kw, int CoutP, int Ktot,
                                float wscale, void* whi, void* wlo, void* stream);
int egne_conv2d_f16x3_fwd(const egne_conv_desc* d, const void* whi, const void* wlo, float a_scale,
                          float w_scale, void* stream);
/* The same convolution for SMALL problems (one or two frames at the 30x40 / 15x20 levels: evaluate.py:235-249 feeds one eye per call):
 * few output tiles and a long K loop would leave most compute units idle, so the launch uses 64 x 64 (or 128 x 32) tiles and splits the K
 * range over gridDim.z workgroups; their partial sums go through `ws` ([Z][B*Ho*Wo][CoutP] floats) and a second launch applies bias /
 * activation / post affine / residual.  egne_conv2d_f16x3_small_workspace_floats: floats of workspace this descriptor needs (0: small tiles,
 * no split), or -1 if the problem is not small -- egne_conv2d_f16x3_small_fwd then runs exactly egne_conv2d_f16x3_fwd.  ngroups = 1 only. */
int64_t egne_conv2d_f16x3_small_workspace_floats(const egne_conv_desc* d);
int egne_conv2d_f16x3_small_fwd(const egne_conv_desc* d, const void* whi, const void* wlo, float a_scale, float w_scale,
                                float* ws, int64_t ws_floats, void* stream);

/* Deep variant of egne_conv2d_f16x3_fwd for the wide trunk layers (vgg16_c.py:70-78): 256 x 256 (or 256 x 128) tile, 8 waves,
 * two LDS stages, one barrier per K step; weights as ready-made LDS images staged by LDS-DMA
 * ([Cout tile][step = chunk*taps + tap][BN rows][128 B], hi | lo granules, swizzled; BN = 256 if Cout % 256 == 0 else 128),
 * fp32 activations converted while staging.  One input slice without fused affine, Cp % 32 == 0, stride 1, zero padding. */
int egne_pack_conv_weight_f16img(const float* w_oihw, int Cout, int Cin, int kh, int kw, int BN, int Ktot, float wscale,
                                 void* wimg, void* stream);
int egne_conv2d_f16x3_big_fwd(const egne_conv_desc* d, const void* wimg, float a_scale, float w_scale, void* stream);
/* The deep variant on PLAIN f16 operands (d->f16_products = 1: the frozen edge network next to a bf16-storage training plan; vgg16_c.py:70-78
 * under utils.py:646): same tile, same accumulation order (bit-identical to egne_conv2d_f16x3_big_fwd with f16_products = 1), but 64-byte LDS
 * rows (hi halves only) in a FOUR-stage ring: activations written two K steps ahead, weight images requested three ahead, the next step's
 * fragments read during the current one.  Needs an even number of K steps (Cp / 32 * kh * kw: egne_conv2d_f16_big1_supported) and weight
 * images without lo granules ([Cout tile][step][BN rows][64 B], egne_pack_conv_weight_f16img1: half the bytes of the f16img pack). */
int egne_pack_conv_weight_f16img1(const float* w_oihw, int Cout, int Cin, int kh, int kw, int BN, int Ktot, float wscale,
                                  void* wimg, void* stream);
int egne_conv2d_f16_big1_supported(const egne_conv_desc* d);
int egne_conv2d_f16_big1_fwd(const egne_conv_desc* d, const void* wimg, float a_scale, float w_scale, void* stream);

/* Split-f16 variant of the LDS-halo 3x3 kernel (narrow full-resolution layers: Cout 32 / 64, dilation <= 2, one
 * input slice, fused affine allowed).  Weights: hi / lo f16 in MFMA-fragment order
 * [tap][Ktot/16][CoutP/32][lane][8], Ktot = slice width rounded up to 32. */
int egne_pack_conv_weight_f16frag(const float* w_oihw, int Cout, int Cin, int kh, int kw, int CoutP, int Ktot,
                                  float wscale, void* fhi, void* flo, void* stream);
int egne_conv3x3_halo_f16_fwd(const egne_conv_desc* d, const void* fhi, const void* flo, float a_scale,
                              float w_scale, void* stream);

/* The dilated branch of a BDCN MSBlock in ONE launch (bdcn_new.py:51-54): out = o + sum_g relu(conv3x3_{dil g}(o) + b_g),
 * 32 -> 32 channels, dilations {4, 8, 12}.  Same descriptor as the grouped form of egne_conv2d_f16x3_fwd (ngroups = 3,
 * one raw 32-channel slice, CoutP = Ktot = 32, bias [3][32], act = ReLU, residual = the input slice); weights: three
 * consecutive egne_pack_conv_weight_f16frag packs.  A workgroup keeps the 4-way sum of its 8 x 32 tile in registers, so o
 * is read once and out written once (round 1: three launches accumulating through HBM). */
int egne_msblock_dil_f16_fwd(const egne_conv_desc* d, const void* fhi, const void* flo, float a_scale, float w_scale,
                             void* stream);
/* ... with the stage's score heads in the epilogue (bdcn_new.py:118-166: conv*_down 32 -> 21 summed over the stage's blocks,
 * then score_dsn* / score_dsn*_1 21 -> 1; linear, so per block and head one 32-vector): s0[p] (+)= score_w[0] . out[p],
 * s1[p] (+)= score_w[1] . out[p]; the first block of a stage (accumulate = 0) also adds the constants score_c[2].  With
 * d->out == NULL the 32-channel block output is not stored at all (nothing else reads it). */
int egne_msblock_dil_scores_f16_fwd(const egne_conv_desc* d, const void* fhi, const void* flo, float a_scale, float w_scale,
                                    const float* score_w, const float* score_c, float* s0, float* s1, int accumulate,
                                    void* stream);

/* Transition_down of an inference plan in one pass (models/RITnet_v2.py:32-44: avg_pool2d(conv1x1(leaky(IN(cat(out, x)))), 2) --
 * pooling and 1x1 are linear, the 2x2 average moves in front): the 1x1's operand is the window average of
 * act_in(x * scale + shift).  d: kh = kw = 1, H / W = input size, Ho / Wo = H / 2, W / 2, every slice with scale / shift
 * [B][Cp]; weights as for egne_conv1x1_f16x3_fwd. */
int egne_conv1x1_pool2_f16x3_fwd(const egne_conv_desc* d, const void* fhi, const void* flo, float a_scale, float w_scale,
                                 void* stream);

/* Role-split variant of egne_conv3x3_halo_f16_fwd for narrow inputs (one slice of <= 64 channels: vgg16_c.py:66-69 conv1_2 /
 * conv2_1, bdcn_new.py:50 stage-1 MSBlock convs, models/RITnet_v2.py:57 down-block conv1, utils.py:1047-1048 decoder convBlock):
 * 4 producer waves stage the halo (gather, fused affine, fp32 -> hi / lo) while 4 consumer waves do nothing but LDS reads and
 * MFMAs.  Same descriptor and weight pack; dilation 1, Ktot 32 or 64, CoutP 32 / 64 / 128; stats_ws allowed. */
int egne_conv3x3_rs_f16_fwd(const egne_conv_desc* d, const void* fhi, const void* flo, float a_scale, float w_scale,
                            void* stream);

/* The same convolution with the workgroup's weights RESIDENT in LDS (one 32-channel output block per workgroup, the input staged
 * once per block): the consumer waves issue no vector loads, so their stores are never waited for (loads and stores retire through
 * one in-order counter).  Same descriptor and pack; Cout_store % 8 == 0, 16-byte aligned slices, no statistics; optional pooled
 * second output (pool_out). */
int egne_conv3x3_rw_f16_fwd(const egne_conv_desc* d, const void* fhi, const void* flo, float a_scale, float w_scale,
                            void* stream);

/* Streaming 1x1 convolution over a concatenation of raw NHWC slices (models/RITnet_v2.py:59,61,84,86 conv21 / conv31 /
 * conv11, :38 Transition_down in eval plans) on the split-f16 path: no staging, every lane loads its MFMA operand
 * straight from HBM, weight fragments stay in LDS.  Same descriptor as egne_conv2d_fwd (`w` unused; no fused affine,
 * residual or post affine; CoutP 32 or a multiple of 64).  Weights: hi / lo f16 fragments [G][CoutP/32][lane][8] where
 * G = sum over slices of ceil(Cp/16) and kmap[g*16 + h*8 + j] (device int32) names the logical input channel in K
 * slot (half h, j) of group g (-1 = padding); the kernel's slot order is channel 16g + (j<4 ? 4h+j : 8+4h+j-4).
 * Up-sampled addend: with d->residual set and Ho * 2 == H, Wo * 2 == W (instead of Ho == H, Wo == W) the residual is a
 * HALF-resolution tensor [B][Ho][Wo] (res_pix_stride / res_ch_off, 16-byte aligned channel vectors) whose bilinear x2
 * up-sampling (F.interpolate, scale 2, align_corners False) is added to the activation-free result:
 * conv11(cat(up(x), skip)) = up(W_up x) + W_skip skip of an up block (models/RITnet_v2.py:84-86) without the up-sampled
 * tensor. */
int egne_pack_conv1x1_weight_f16(const float* w_oihw, int Cout, int Cin, const int32_t* kmap, int G, int CoutP,
                                 float wscale, void* fhi, void* flo, void* stream);
int egne_conv1x1_f16x3_fwd(const egne_conv_desc* d, const void* fhi, const void* flo, float a_scale,
                           float w_scale, void* stream);

/* A 1x1 convolution over raw slices FUSED with the 3x3 / pad 1 convolution that is its only consumer
 * (models/RITnet_v2.py:59-62 conv22(conv21(.)), conv32(conv31(.)); :84-87 conv12(conv11(.)), conv22(conv21(.))): the 1x1 is
 * evaluated on each tile's halo and kept in LDS as hi / lo halves, the 3x3 runs from there -- its input is never stored.
 * d1 = the 1x1 (slices as for egne_conv1x1_f16x3_fwd; CoutP 32 or 64; no activation; output fields ignored),
 * d2 = the 3x3 (Ktot = d1->CoutP, CoutP 32 or 64, bias / act / post affine / residual / output as for
 * egne_conv3x3_halo_f16_fwd; seg[] ignored).  w1hi / w1lo: egne_pack_conv1x1_weight_f16, f2hi / f2lo:
 * egne_pack_conv_weight_f16frag.  a1 pre-scales the slices, a2 the 1x1 result (powers of two). */
int egne_conv1x1_3x3_fused_f16_fwd(const egne_conv_desc* d1, const egne_conv_desc* d2, const void* w1hi, const void* w1lo,
                                   float a1, float w1_scale, const void* f2hi, const void* f2lo, float a2, float w2_scale,
                                   void* stream);

/* The same with a 3x3 / pad 1 convolution on <= 4 input channels in front (utils.py:1047-1048 convBlock: conv1 -> LeakyReLU ->
 * conv2 -> LeakyReLU [-> eval BatchNorm = d2's post affine]): d1 = that convolution (one slice with >= 4 padded channels,
 * CoutP = 32; its activation is applied before the 3x3), c4hi / c4lo = egne_pack_conv3x3_c4_weight_f16 (CoutP 32).
 * A one-channel input may be given in place as [B][H][W] floats (= NCHW with C = 1): seg[0].pix_stride = 1, ch_off = 0. */
int egne_conv3x3c4_3x3_fused_f16_fwd(const egne_conv_desc* d1, const egne_conv_desc* d2, const void* c4hi, const void* c4lo,
                                     float a1, float w1_scale, const void* f2hi, const void* f2lo, float a2, float w2_scale,
                                     void* stream);

/* LDS-staged variant of the split-f16 1x1 convolution over raw slices, for the layers whose K or Cout exceed what the
 * streaming kernel keeps in LDS (decoder conv11 / conv21 at 30x40 and 60x80, models/RITnet_v2.py:84,86; dense block 3):
 * 128x128 (CoutP % 128 == 0) or 256x64 tiles.  d->Ktot = sum of the slice widths rounded up to 32 each; weights: hi / lo
 * f16 [CoutP][Ktot] with kmap[k] (device int32) naming the logical input channel of K column k (-1 = padding). */
int egne_pack_conv1x1_weight_f16x2_map(const float* w_oihw, int Cout, int Cin, const int32_t* kmap, int CoutP, int Ktot,
                                       float wscale, void* whi, void* wlo, void* stream);
int egne_conv1x1_ms_f16x3_fwd(const egne_conv_desc* d, const void* whi, const void* wlo, float a_scale,
                              float w_scale, void* stream);

/* First layers (vgg16_c.py:66 conv1_1 on 3 channels, utils.py:1047 convBlock conv1 on 1-2 channels):
 * 3x3 / stride 1 / pad 1, logical Cin <= 4, Cout <= 64.  The 9 taps are folded into K (one 40-wide K step,
 * exact fp32 MFMA), so the layer is a pure store stream.  w40: [32 or 64][40] fp32, column tap*4 + c. */
int egne_conv3x3_smallcin_fwd(const egne_conv_desc* d, const float* w40, void* stream);

/* Split-f16, streaming form of egne_conv3x3_smallcin_fwd for frozen / inference plans: the 9 taps folded into K = 48 (three
 * K=16 steps), nothing staged -- a lane's operand for one step is the 4-channel vectors of two taps of its pixel (two 16-byte
 * buffer loads), weight fragments in registers, 16-byte stores.  Weights: hi / lo f16 [3][CoutP/32][lane][8], K slot
 * (step s, half h, j) = tap 4s + 2h + (j>>2), channel j&3; d->CoutP = 32 or 64. */
int egne_pack_conv3x3_c4_weight_f16(const float* w_oihw, int Cout, int Cin, int CoutP, float wscale, void* fhi, void* flo,
                                    void* stream);
int egne_conv3x3_smallcin_f16_fwd(const egne_conv_desc* d, const void* fhi, const void* flo, float a_scale,
                                  float w_scale, void* stream);

/* OIHW (torch layout) -> packed [tap][CoutP][Ktot].  kinv[k] (device int32, k < Ktot) names the
 * input channel stored at padded K position k, or -1 for a padding column; rows Cout..CoutP-1 are
 * zero.  Used at load_state_dict / after optimizer steps. */
int egne_pack_conv_weight(const float* w_oihw, int Cout, int Cin, int kh, int kw,
                          const int32_t* kinv, int CoutP, int Ktot, float* w_packed, void* stream);

/* max |x| over the channel slice [ch_off, ch_off+Cp) of npix NHWC pixels, written as the float's bit pattern with an
 * integer atomic max into *out_bits (zero it first; a NaN input gives a pattern above +inf).  Used once per plan to
 * choose the power-of-two pre-scale of the split-f16 kernels (a_scale): |x| * a_scale must stay below the f16 range,
 * which the fixed scale of round 1 did not guarantee for arbitrary checkpoints. */
int egne_absmax(const float* x, int64_t pix_stride, int ch_off, int Cp, int64_t npix, void* out_bits, void* stream);
/* The same over a slice held as F16 (egne_conv_desc.out_split = 2; pix_stride / ch_off in halfs, multiples of 8): the word receives the
 * bit pattern of max |x| as a FLOAT, so the host derives scales from either measurement alike. */
int egne_absmax_f16(const void* x, int64_t pix_stride, int ch_off, int Cp, int64_t npix, void* out_bits, void* stream);

/* Per-(n,c) mean / inverse std over H*W of an NHWC slice -> scale = rstd, shift = -mean*rstd
 * ([B][Cp]).  F.instance_norm at models/RITnet_v2.py:40,57 (eps 1e-5, biased variance).  With
 * per_sample=0 the statistics run over (B,H,W): training-mode BatchNorm2d of utils.py:1049 and
 * the result is [1][Cp]; mean/var (biased) are also written when the pointers are non-NULL.
 * Two deterministic stages with fp64 partial sums in `ws` (egne_norm_stats_workspace_bytes; 16-byte aligned, as for egne_norm_bwd). */
int64_t egne_norm_stats_workspace_bytes(int B, int HW, int Cp, int per_sample);
int egne_norm_stats(const float* x, int64_t pix_stride, int ch_off, int Cp, int B, int HW,
                    int per_sample, float eps, float* scale, float* shift,
                    float* mean_out, float* var_out, void* ws, void* stream);

/* Second stage of egne_norm_stats on partial sums that a convolution wrote from its epilogue (egne_conv_desc.stats_ws):
 * ws [B][nchunk][Cp][2] doubles -> scale = rstd, shift = -mean*rstd ([B][Cp]); fixed summation order (deterministic). */
int egne_norm_stats_finish(const void* ws, int Cp, int B, int nchunk, int HW, float eps, float* scale, float* shift,
                           void* stream);
/* The same with mean / biased variance written too ([B][Cp]): batch statistics of a training-mode BatchNorm (utils.py:1049) from a
 * convolution's epilogue (round 5) -- the B samples of the batch as ONE sample of B * nchunk chunks and B * HW pixels. */
int egne_norm_stats_finish_moments(const void* ws, int Cp, int B, int nchunk, int HW, float eps, float* scale, float* shift,
                                   float* mean_out, float* var_out, void* stream);

/* y = x*scale[c] + shift[c] in place over an NHWC slice (training-mode BatchNorm apply). */
int egne_affine_inplace(float* x, int64_t pix_stride, int ch_off, int Cp, int64_t npix,
                        const float* scale, const float* shift, void* stream);

/* y = x*scale[c] + shift[c], out of place (training-mode BatchNorm keeps its input for backward). */
int egne_affine(const float* x, int64_t xs, int xo, float* y, int64_t ys, int yo, int Cp, int64_t npix,
                const float* scale, const float* shift, void* stream);

/* nn.AvgPool2d(2) (models/RITnet_v2.py:36,43; utils.py:1017) on an NHWC slice. */
int egne_avgpool2(const float* x, int64_t xs, int xo, float* y, int64_t ys, int yo,
                  int B, int H, int W, int Cp, void* stream);

/* avgpool2(act(x*scale[n][c] + shift[n][c])): Transition_down (models/RITnet_v2.py:32-44) with the
 * AvgPool2d commuted in front of its 1x1 conv (both linear; rounding-level difference only). */
int egne_norm_act_pool2(const float* x, int64_t xs, int xo, const float* scale, const float* shift, int act,
                        float* y, int64_t ys, int yo, int B, int H, int W, int Cp, void* stream);

/* nn.MaxPool2d(2, stride, ceil_mode=True) (vgg16_c.py:15,20,27,34) on an NHWC slice. */
int egne_maxpool2(const float* x, int64_t xs, int xo, float* y, int64_t ys, int yo,
                  int B, int H, int W, int Ho, int Wo, int stride, int Cp, void* stream);
/* The same pooling over a slice held as F16 (egne_conv_desc.out_split = 2; strides / offsets in halfs, multiples of 8): the maximum commutes with
 * the storage scale, so the output is held under the input's scale (pool3 / pool4 of vgg16_c.py:76-82 in a plain-f16 plan). */
int egne_maxpool2_f16(const void* x, int64_t xs, int xo, void* y, int64_t ys, int yo, int B, int H, int W, int Ho, int Wo, int stride,
                      int Cp, void* stream);

/* The same pooling over a slice in channel-order split-pair storage (egne_conv_desc.out_split = 3; strides / offsets in units of 4 bytes, whole
 * 32-channel blocks): the window is compared on hi + lo (exact in fp32), the winner's pair is written, on equal sums the pair with the larger hi --
 * bit-equal to the split of the pooled fp32 tensor under the same scale (pool3 / pool4 of vgg16_c.py:76-82 in the calibrated inference plan). */
int egne_maxpool2_split(const void* x, int64_t xs, int xo, void* y, int64_t ys, int yo, int B, int H, int W, int Ho, int Wo, int stride,
                        int Cp, void* stream);

/* F.interpolate(bilinear, scale_factor=2, align_corners=False) (models/RITnet_v2.py:80-83). */
int egne_upsample2x(const float* x, int64_t xs, int xo, float* y, int64_t ys, int yo,
                    int B, int H, int W, int Cp, void* stream);

/* NCHW [B,C,H,W] -> NHWC slice (zero fills channels C..Cp-1) and back. */
int egne_nchw_to_nhwc(const float* x, int B, int C, int H, int W, float* y, int64_t ys, int yo,
                      int Cp, void* stream);
int egne_nhwc_to_nchw(const float* x, int64_t xs, int xo, int B, int C, int H, int W, float* y,
                      void* stream);

/*
 * BDCN side outputs of one stage (bdcn_new.py:118-164): the 1x1 `convK_j_down` (32->21) of every
 * MSBlock output of the stage are summed and the two 1x1 score heads (21->1) applied; writes the two
 * low-resolution score maps s (score_dsnK) and s1 (score_dsnK_1), each [B,h,w].
 * ms is a HOST array of nblk device pointers to NHWC 32-channel tensors; wd [nblk][21][32], bd [nblk][21]; ws/ws1 [21], bs/bs1 scalars
 * passed by pointer (device).
 */
int egne_bdcn_stage_scores(const float* const* ms, int nblk, int64_t ms_pix_stride, int64_t npix,
                           const float* wd, const float* bd, const float* ws, const float* bs,
                           const float* ws1, const float* bs1, float* s, float* s1, void* stream);

/*
 * BDCN tail (bdcn_new.py:127-191): ConvTranspose2d upsampling (k=2*stride, weights from the
 * checkpoint) + crop of stages 2..5, the two deep-supervision cascades, the 1x1 fuse over the 10
 * maps and the sigmoids.  s[k]/s1[k] are the stage score maps [B,h_k,w_k]; up[k] the k_k x k_k
 * upsampling kernels (up[0] unused).  out[0..10] are [B,1,H,W] maps (any may be NULL to skip it;
 * calc_edge only needs out[10], the fused edge map).
 */
typedef struct {
  int32_t B, H, W;
  const float* s[5];
  const float* s1[5];
  int32_t h[5], w[5];
  int32_t stride[5], crop[5];
  const float* up[5];
  const float* fuse_w;   /* [10] */
  const float* fuse_b;   /* [1]  */
  float* out[11];
  int32_t edge_thres;    /* utils.py:653-655: out[10] >= 0.1 -> 1 */
} egne_bdcn_tail_desc;
int egne_bdcn_tail(const egne_bdcn_tail_desc* d, void* stream);

/*
 * Loss head (models/RITnet_v2.py:372-432, loss.py:16-137) in two launches and no host sync.
 * Pass 1 reads the logits once (NHWC slice, 3 classes) and writes per-block partial sums;
 * pass 2 (one block per sample + one finishing block) reduces them to
 *   out_terms[0..7] = total, l_seg2pt, l_seg, l_pt, l_ellipse, n_mask_present, bad_sample_flag, 0
 *   pred_c[B][2][2] = (iris, pupil) soft-argmax centres (iris = elOut[:,5:7] when no mask in batch)
 *   mask[B][H][W]   = argmax over the 3 classes (int64, first max on ties; utils.py:65-81), optional
 *   op_nchw         = logits transposed to [B,3,H,W], optional
 */
typedef struct {
  int32_t B, H, W;
  const float* logits; int64_t pix_stride; int32_t ch_off;
  const int64_t* target;       /* [B,H,W] */
  const float* spatWts;        /* [B,H,W] */
  const float* distMap;        /* [B,3,H,W] */
  const float* cond;           /* [B,4], 0 = annotation present */
  const float* pupil_center;   /* [B,2] pixels */
  const float* elNorm;         /* [B,2,5] */
  const float* elOut;          /* [B,10] */
  float alpha;
  const float* grid_x;         /* optional [W] / [H] mesh axes (torch.linspace(-1,1,.)); NULL = closed form */
  const float* grid_y;
  float* partials;             /* workspace, egne_loss_workspace_floats(B,H,W) floats */
  float* out_terms;            /* [8] */
  float* pred_c;               /* [B,2,2] */
  float* elPred;               /* [B,10] = (c_iris, elOut[2:5], c_pupil, elOut[7:10]) */
  int64_t* mask;               /* optional */
  float* op_nchw;              /* optional */
  float* coef;                 /* optional [B][32]: per-sample state kept for egne_loss_bwd */
  int32_t dtype;               /* storage of `logits`: 0 fp32, 1 bf16 (pix_stride / ch_off in elements); everything else stays fp32 */
  /* egne_loss_bwd only, all optional (round 5): gradients a caller back-propagates through the OUTPUTS next to the loss
   * (models/RITnet_v2.py:334-354 returns op, elPred, elOut with grad): added to what the loss terms themselves give. */
  const float* g_op_nchw;      /* [B,3,H,W] upstream gradient w.r.t. the logits */
  const float* g_pred_c;       /* [B,2,2] upstream gradient w.r.t. pred_c (iris, pupil soft-argmax centres; when no sample of the batch
                                  has a mask pred_c's iris row is a copy of elOut[:,5:7], RITnet_v2.py:404: its gradient is then added
                                  to g_elOut[:,5:7] instead of the logits) */
  const float* g_elOut_up;     /* [B,10] upstream gradient w.r.t. elOut */
} egne_loss_desc;
int64_t egne_loss_workspace_floats(int B, int H, int W);
int egne_loss_fwd(const egne_loss_desc* d, void* stream);

/* Self-consistency term (loss.py:187-219 get_selfConsistency; models/RITnet_v2.py:339-341, RITnet_v1.py:286-287), csrc/selfcorr.hip.
 * With q_e(x, y) = (X/a)^2 + (Y/b)^2 in the frame of ellipse e = (cx, cy, a, b, theta) over the mesh grid_x x grid_y (both required),
 *   t_pup = sigmoid(64 (1 - q_pupil)),  t_bg = sigmoid(64 (q_iris - 1)),  kl(t, lp) = t (log t - lp),  lp = log_softmax(logits),
 *   term  = sum_b ok_b (mean_pix kl(t_pup, lp[2]) + mean_pix kl(t_bg, lp[0])) / n_ok,  ok_b = 1 - cond[b][1],  n_ok = sum_b ok_b,
 * 0 when n_ok == 0.  The iris ellipse is d->elPred[b][0:5], the pupil ellipse d->elPred[b][5:10] (axes non-zero): the call runs behind
 * egne_loss_fwd with the same descriptor and in front of egne_conf_loss.  Reads logits (either storage), cond, elPred and the mesh.
 *   sc_terms[4] = term, n_ok, weight * term, 0;   d->out_terms[0] += weight * term (the reference's weight is 10).
 * ws: egne_selfcorr_workspace_floats(B, H, W) floats, kept for the backward.  Two launches (per-(sample, block) partial sums, one
 * combining block), no atomics. */
int64_t egne_selfcorr_workspace_floats(int B, int H, int W);
int egne_selfcorr_fwd(const egne_loss_desc* d, float weight, float* ws, float* sc_terms, void* stream);
/* Its backward, gscale[0] * weight * d term / d ., ADDED to the three tensors egne_loss_bwd reads as upstream gradients (one launch, every
 * element has one writer):
 *   g_op_nchw [B,3,H,W] += w (t_pup (p_k - [k == 2]) + t_bg (p_k - [k == 0])),  w = weight * gscale * ok_b / (H W n_ok), p = softmax;
 *   g_pred_c  [B,2,2]   += d / d (iris centre, pupil centre), the entries 0:2 and 5:7 of elPred;
 *   g_elOut_up[B,10]    += entries 2:5 and 7:10 only (axes and angle of both ellipses), 0:2 and 5:7 are not touched.
 * d kl / d z = t (1 - t) (log t - lp + 1) is taken as its limit 0 where t or 1 - t underflows (the reference's autograd gives NaN
 * there): finite for finite inputs.  A sample with ok_b == 0, or a batch with n_ok == 0, adds nothing (the destinations keep their bits). */
int egne_selfcorr_bwd(const egne_loss_desc* d, float weight, const float* ws, const float* gscale /* device, 1 float */,
                      float* g_op_nchw, float* g_pred_c, float* g_elOut_up, void* stream);

/* Loss of the DeepVOG comparator (models/deepvog_pytorch.py:148-167 get_allLoss), forward only: 10 * cross_entropy(softmax(op), label == 2)
 * averaged per frame and over the frames with cond[:,1] == 0, plus the mean L1 distance between the soft-argmax centre of channel 1
 * (loss.py:16-46, temperature 4) and utils.normPts(pupil_center).  logits: two channels of an NHWC fp32 slice.  Also writes the NCHW logits
 * [B,2,H,W], the argmax mask [B,H,W] int64 and pred_c [B,2]; out_terms[0] = loss, [1] = segmentation term, [2] = centre term. */
int64_t egne_deepvog_loss_workspace_floats(int B, int H, int W);
int egne_deepvog_loss_fwd(const float* logits, int64_t pix_stride, int ch_off, const int64_t* target, const float* pupil_center,
                          const float* cond, int B, int H, int W, float* partials, float* out_terms, float* pred_c,
                          float* op_nchw, int64_t* mask, void* stream);
/* Its backward (loss.backward() of train.py:286 for this comparator): g_logits[b][y][x][go .. go+2) = gscale[0] * d loss / d logits, from the
 * forward's `partials` and `pred_c` (the launch stores, it does not accumulate). */
int egne_deepvog_loss_bwd(const float* logits, int64_t pix_stride, int ch_off, const int64_t* target, const float* pupil_center,
                          const float* cond, int B, int H, int W, const float* partials, const float* pred_c, const float* gscale /* device */,
                          float* g_logits, int64_t gs, int go, void* stream);
/* y = act(x * scale[c] + shift[c]) over an NHWC fp32 slice: BatchNorm (scale / shift from its statistics) followed by its activation,
 * the order of models/deepvog_pytorch.py:36-41 (conv -> bn -> relu). */
int egne_affine_act(const float* x, int64_t xs, int xo, float* y, int64_t ys, int yo, int Cp, int64_t npix, const float* scale,
                    const float* shift, int act, void* stream);

/* Nearest-neighbour x2 up-sampling of an NHWC slice and its transpose (gx += the four copies): F.interpolate(scale_factor=2,
 * mode='nearest') of the comparator model models/RITnet_v1.py:89 (H, W = INPUT size).  bf16 twins: *_bf16. */
int egne_upsample2x_nearest(const float* x, int64_t xs, int xo, float* y, int64_t ys, int yo, int B, int H, int W, int Cp, void* stream);
int egne_upsample2x_nearest_bwd(const float* gy, int64_t gs, int go, float* gx, int64_t xs, int xo, int B, int H, int W, int Cp, void* stream);
int egne_upsample2x_nearest_bf16(const void* x, int64_t xs, int xo, void* y, int64_t ys, int yo, int B, int H, int W, int Cp, void* stream);
int egne_upsample2x_nearest_bwd_bf16(const void* gy, int64_t gs, int go, void* gx, int64_t xs, int xo, int B, int H, int W, int Cp, void* stream);

/* regressionModule output activations (utils.py:1023-1036): tanh / sigmoid / identity split of the
 * 10 raw outputs, in place over [B,10] (row stride `ld`). */
int egne_ellipse_head_act(float* x, int B, int ld, void* stream);
/* torch.selu in place over n floats (utils.py:1021). */
int egne_selu_inplace(float* x, int64_t n, void* stream);
/* latent = mean over H*W of an NHWC slice -> [B][C] (models/RITnet_v2.py:282). */
int egne_spatial_mean(const float* x, int64_t pix_stride, int ch_off, int C, int B, int HW,
                      float* out, void* stream);

/* AdaIN fusion path (models/RITnet_v2.py:289-308).  egne_softmax3: nn.Softmax(dim=1) over the 3 logits
 * of every pixel into an NHWC slice of Cp_out channels (zero padded) that feeds the StyleEncoder.
 * egne_adain: calc_mean_std (:251-259, UNBIASED variance + eps) and
 * x' = (x-mean)/std * gamma[n][c] + beta[n][c]; gamma/beta are rows of the MLP output
 * (element [n*gb_stride + gb_off + c]). */
int egne_softmax3(const float* x, int64_t xs, int xo, float* y, int64_t ys, int yo, int Cp_out,
                  int64_t npix, void* stream);
int egne_adain(const float* x, int64_t xs, int xo, int C, const float* gamma, const float* beta,
               int64_t gb_stride, int gb_off, float* y, int64_t ys, int yo, int B, int HW, float eps,
               void* stream);

/* conf_Loss (loss.py:139-157) on pred [B,C] (row stride ld).  flag=1: conf = mean|softmax - 1/C| and
 * terms[0] += weight*conf (RITnet_v2.py:345-347); flag=0: conf = cross-entropy(pred, gt) and
 * terms[0] = conf (:348-350).  terms[7] = conf.  Runs after egne_loss_fwd on the same stream. */
int egne_conf_loss(const float* pred, int ld, const int64_t* gt, int B, int C, int flag, float weight,
                   float* terms, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Backward of ESF-Net (loss.backward() of train.py:286; BDCN is frozen and has no backward).
 * Data gradients of convolutions are forward convolutions with the weight pack of
 * egne_pack_conv_weight_dgrad (flipped taps, in/out channels swapped, restricted to one input slice),
 * accumulated into the slice's gradient through `residual`.
 * ------------------------------------------------------------------------------------------------ */

/* d total_loss * gscale / d logits (written to an NHWC slice, 3 channels) and / d elOut [B,10].
 * Needs the descriptor of the matching egne_loss_fwd call with `coef`, `grid_x`, `grid_y` set. */
int egne_loss_bwd(const egne_loss_desc* d, const float* gscale /* device, 1 float */, float* g_logits,
                  int64_t gs, int go, float* g_elOut, void* stream);

/* In place g <- g * act'(y) over an NHWC slice (y = forward output of the conv) and the bias gradient
 * dbias[c] (+)= sum over pixels of the masked g, c < C. */
int64_t egne_act_bwd_bias_workspace_bytes(int64_t npix, int Cp);
/* egne_act_bwd_bias_absmax: the same, plus the atomic max of the bit patterns of |gz| into *absmax_bits (the dyn_scale word
 * of the split-f16 data-gradient launches that read gz next). */
int egne_act_bwd_bias_absmax(float* g, int64_t gs, int go, const float* y, int64_t ys, int yo, int act, int Cp,
                             int64_t npix, float* dbias, int C, int accumulate, void* ws, uint32_t* absmax_bits, void* stream);
int egne_act_bwd_bias(float* g, int64_t gs, int go, const float* y, int64_t ys, int yo, int act, int Cp,
                      int64_t npix, float* dbias, int C, int accumulate, void* ws, void* stream);
/* Zero a list of device buffers in one launch (a backward plan's gradient twins before each pass; the reference's autograd
 * allocates fresh gradients instead).  table: device array of nseg x {uint64 address, uint64 bytes, uint64 first_block}, addresses
 * 16-byte aligned, bytes a multiple of 16, first_block = the running sum of ceil(bytes / 65536); nblocks = that sum over all. */
int egne_zero_many(const void* table, int nseg, int64_t nblocks, void* stream);
/* Bias gradient of an activation-free 1x1 that feeds a 3x3 (stride 1, zero pad 1) -- the 'a' layer of the reference's dense-block
 * pairs (RITnet_v2.py:145-156 conv1x1 -> conv3x3) -- without a pass over the 3x3's data gradient g_tmp: sum_q g_tmp[q][ca] =
 * sum_{co,tap} w[co][ca][tap] * S_tap[co], S_tap = the 3x3's per-channel gradient total minus the border row / column the tap
 * cannot reach.  g: the 3x3's masked output gradient after egne_act_bwd_bias(..., dbias = NULL, ws = act_ws) over the same
 * B*H*W pixels and Cp channels (its chunk sums are read from act_ws); w: fp32 OIHW [Cout][Ca][3][3]; db_b (may be NULL) += the
 * 3x3's bias gradient, db_a += the 1x1's.  ws: egne_pair_bias_bwd_workspace_bytes(B, Cp) bytes, 8-byte aligned.  Cp, Ca <= 256. */
int64_t egne_pair_bias_bwd_workspace_bytes(int B, int Cp);
int egne_pair_bias_bwd(const float* g, int64_t gs, int go, int Cp, int B, int H, int W, const void* act_ws, const float* w,
                       int Cout, int Ca, float* db_b, float* db_a, void* ws, void* stream);

/* Backward of the normalisation that the forward fused into a conv's load (InstanceNorm, per_sample=1)
 * or of training-mode BatchNorm (per_sample=0, gamma/dgamma/dbeta given): xh = x*scale+shift,
 * g = gy*act_in'(xh), gx += scale*gamma*(g - mean(g) - xh*mean(g*xh)).  sums: [Bn][Cp][2] scratch. */
int64_t egne_norm_bwd_workspace_bytes(int B, int HW, int Cp, int per_sample);
int egne_norm_bwd(const float* x, int64_t xs, int xo, const float* scale, const float* shift,
                  const float* gamma, const float* gy, int64_t gs, int go, int act_in, int Cp, int B, int HW,
                  int per_sample, float* gx, int64_t gxs, int gxo, float* sums, float* dgamma, float* dbeta,
                  int C, void* ws, void* stream);

/* Backward of egne_norm_act_pool2 (training-mode Transition_down with the pooling in front of the 1x1, models/RITnet_v2.py:32-44):
 * egne_norm_bwd (per-sample statistics) whose gy is a quarter of the pooled cell's gradient gzp [B][H/2][W/2]; H, W even;
 * accumulate = 0 stores gx instead of adding to it; workspace as egne_norm_bwd_workspace_bytes(B, H*W, Cp, 1). */
int egne_norm_pool2_bwd(const float* x, int64_t xs, int xo, const float* scale, const float* shift,
                        const float* gzp, int64_t gs, int go, int act_in, int Cp, int B, int H, int W,
                        float* gx, int64_t gxs, int gxo, int accumulate, float* sums, void* ws, void* stream);
/* egne_norm_bwd_store: egne_norm_bwd with gx stored (=) instead of accumulated (+=): the first writer of a gradient slice. */
int egne_norm_bwd_store(const float* x, int64_t xs, int xo, const float* scale, const float* shift,
                        const float* gamma, const float* gy, int64_t gs, int go, int act_in, int Cp, int B, int HW,
                        int per_sample, float* gx, int64_t gxs, int gxo, float* sums, float* dgamma, float* dbeta,
                        int C, void* ws, void* stream);
int egne_avgpool2_bwd(const float* gy, int64_t gs, int go, float* gx, int64_t xs, int xo,
                      int B, int H, int W, int Cp, void* stream);       /* gx += ; H,W = input size */
int egne_upsample2x_bwd(const float* gy, int64_t gs, int go, float* gx, int64_t xs, int xo,
                        int B, int H, int W, int Cp, void* stream);     /* gx += ; H,W = input size */
int egne_ellipse_head_act_bwd(float* g, const float* y, int B, int ld, void* stream);
int egne_selu_bwd(float* g, const float* y, int64_t n, void* stream);
/* Backward of the AdaIN fusion path (models/RITnet_v2.py:289-308); every output is ACCUMULATED (+=).
 * egne_softmax3_bwd: gx[c] += y[c]*(gy[c] - sum_k gy[k]y[k]) over the 3 logits of a pixel.
 * egne_adain_bwd: gradients of x' = gamma*(x-mean)/sqrt(var_unbiased+eps) + beta w.r.t. x (gx), gamma and beta
 *   (rows of the MLP output gradient: element [n*gg_stride + gg_off + c]).
 * egne_reflect_pad_bwd: backward of nn.ReflectionPad2d(P) in front of a Conv2dBlock (utils.py:1099-1100,1144):
 *   gx += fold of the padded-input gradient; phase=1 reads the phase-packed [B,(H+2P)/2,(W+2P)/2,4*Cp] output of the
 *   stride-2 transposed convolution (channel block (py&1)*2+(px&1)). */
int egne_softmax3_bwd(const float* y, int64_t ys, int yo, const float* gy, int64_t gs, int go, float* gx,
                      int64_t xs, int xo, int64_t npix, void* stream);
int egne_adain_bwd(const float* x, int64_t xs, int xo, int C, const float* gamma, int64_t gb_stride, int gb_off,
                   const float* gy, int64_t gys, int gyo, float* gx, int64_t gxs, int gxo, float* ggamma,
                   float* gbeta, int64_t gg_stride, int gg_off, int B, int HW, float eps, void* stream);
int egne_reflect_pad_bwd(const float* gpad, int64_t gs, int go, int phase, int Cp, float* gx, int64_t xs, int xo,
                         int B, int H, int W, int P, void* stream);
int egne_spatial_mean_bwd(const float* g, int gld, float* gx, int64_t xs, int xo, int C, int B, int HW,
                          void* stream);
int egne_conf_loss_bwd(const float* pred, int ld, const int64_t* gt, int B, int C, int flag,
                       const float* gscale /* device, 1 float */, float* gpred, int gld, void* stream);

/* Fused backward of a tensor x that was InstanceNorm-ed once (scale / shift per sample, egne_norm_stats) for up to two consumers
 * (round 5; models/RITnet_v2.py:57: conv1 behind IN(x); :40-44: Transition_down behind avg_pool2d(leaky(IN(.)))): the
 * normalisation's backward is linear in its upstream gradient G = a1 + act_q'(xh) up(gq) / 4 (a1: full-resolution addend, gq: the
 * gradient of the 2x2-pooled tensor; either may be NULL), and its result joins the gradient of x where the layer that PRODUCED x
 * masks it: g <- act'(x) (g + rstd (G - mean G - xh mean(G xh))) in place, with that layer's bias sums (dbias += ..., and the chunk
 * sums in ws_bias as egne_act_bwd_bias leaves them for egne_pair_bias_bwd).  Replaces egne_norm_bwd + egne_norm_pool2_bwd +
 * egne_act_bwd_bias: five passes over full-resolution tensors less.  B samples of H x W pixels (even for a pooled addend).
 * sums: [B][Cp][2] floats (scratch); ws_norm: egne_norm_bwd_workspace_bytes(B, H*W, Cp, 1); ws_bias:
 * egne_act_bwd_bias_workspace_bytes(B*H*W, Cp).  acc_samples: g of the first acc_samples samples is read (accumulated onto), the
 * rest of g is written only (no earlier writer; B: plain read-modify-write of all of g). */
int egne_act_norm_bwd(float* g, int64_t gs, int go, const float* x, int64_t xs, int xo, int act, const float* scale, const float* shift,
                      const float* a1, int64_t a1s, int a1o, const float* gq, int64_t gqs, int gqo, int act_q, int Cp, int B, int H, int W,
                      float* sums, void* ws_norm, float* dbias /* may be NULL */, int C, void* ws_bias, int acc_samples, void* stream);
int egne_act_norm_bwd_bf16(void* g, int64_t gs, int go, const void* x, int64_t xs, int xo, int act, const float* scale, const float* shift,
                           const void* a1, int64_t a1s, int a1o, const void* gq, int64_t gqs, int gqo, int act_q, int Cp, int B, int H, int W,
                           float* sums, void* ws_norm, float* dbias, int C, void* ws_bias, int acc_samples, void* stream);

/* Training-mode BatchNorm backward (batch statistics over B samples, utils.py:1049) together with the masking pass of the layer in
 * front of it (round 5): x = that layer's activated output = the BatchNorm's input, scale / shift = rstd / -mean rstd ([Cp], one row:
 * egne_norm_stats with per_sample = 0), gamma [Cp], gy = gradient of the BatchNorm's output;
 *   gx <- act'(x) rstd gamma (gy - mean gy - xh mean(gy xh))      (stored: the BatchNorm is the only reader of x)
 *   dgamma += sum gy xh, dbeta += sum gy (first Cn channels), dbias += sum gx (first C channels; may be NULL), chunk sums of gx in
 * ws_bias as egne_act_bwd_bias leaves them.  Replaces egne_norm_bwd + egne_act_bwd_bias: one statistics pass (reads gy, x) and one
 * apply pass (reads gy, x, writes gx) instead of those two and a read-modify-write of gx.  sums: [Cp][2] floats (scratch); ws_norm:
 * egne_norm_bwd_workspace_bytes(B, H*W, Cp, 1); ws_bias: egne_act_bwd_bias_workspace_bytes(B*H*W, Cp). */
int egne_bn_act_bwd(const float* x, int64_t xs, int xo, int act, const float* scale, const float* shift, const float* gamma, const float* gy,
                    int64_t gys, int gyo, int Cp, int B, int H, int W, float* gx, int64_t gxs, int gxo, float* sums, void* ws_norm,
                    float* dgamma, float* dbeta, int Cn, float* dbias /* may be NULL */, int C, void* ws_bias, void* stream);
int egne_bn_act_bwd_bf16(const void* x, int64_t xs, int xo, int act, const float* scale, const float* shift, const float* gamma, const void* gy,
                         int64_t gys, int gyo, int Cp, int B, int H, int W, void* gx, int64_t gxs, int gxo, float* sums, void* ws_norm,
                         float* dgamma, float* dbeta, int Cn, float* dbias, int C, void* ws_bias, void* stream);

/* Weight gradient of the convolution described by `d` (same descriptor as the forward call):
 * gw[g][co][ci][kh][kw] += sum_pixels gz[pixel][co] * input[pixel + tap][ci], gz = gradient w.r.t. the
 * pre-activation output.  gw is a HOST array of ngroups device pointers (OIHW, torch layout).
 * ws: egne_conv2d_wgrad_workspace_bytes(d) bytes of split partial sums, ZERO-FILLED by the caller before its first use and kept for
 * calls with the same descriptor shape: the forms that do not write every partial (1x1 over slices, the generic implicit GEMM)
 * rely on the zeros, and their reduction clears what it reads, so the workspace is zero-filled again when the call returns (round 4:
 * this replaced a fill in front of every such launch).  Every argument is validated before the first launch (a rejected call queues
 * nothing and leaves ws as it was); a call whose launches fail clears ws itself before it returns the error (round 5). */
int egne_conv2d_wgrad_splits(const egne_conv_desc* d);
int64_t egne_conv2d_wgrad_workspace_bytes(const egne_conv_desc* d);
int egne_conv2d_wgrad(const egne_conv_desc* d, const float* gz, int64_t gzs, int gzo, int Cout, int Cin,
                      const int32_t* kinv, float* const* gw, void* ws, void* stream);
/* egne_conv2d_wgrad_f16: the same with split-f16 products (3 x v_mfma_f32_32x32x16_f16, fp32 accumulation) for the 3x3 / stride 1 /
 * pad 1 single-slice shapes when gz_absmax_bits (device word: bit pattern of max|gz|, written by egne_act_bwd_bias_absmax) is given
 * and the input carries a pre-scale (normalised on load, or d->dyn_scale from the forward launch); exact fp32 otherwise. */
int egne_conv2d_wgrad_f16(const egne_conv_desc* d, const float* gz, int64_t gzs, int gzo, const uint32_t* gz_absmax_bits,
                          int Cout, int Cin, const int32_t* kinv, float* const* gw, void* ws, void* stream);
int egne_pack_conv_weight_dgrad(const float* w_oihw, int Cout, int Cin, int kh, int kw, int ci0, int Cpiece,
                                int CoutPp, int Ktotp, int frag, float* out, void* stream);

/*
 * Ellipse fit of evaluate.py (utils.py:450-486 search_proper_parameter_iou_for_our_data with
 * calc_ell_iou utils.py:176-204 and the conic algebra of helperfunctions.py:13-63,102-129):
 * one workgroup per (frame, class) runs the whole coordinate search on the device.
 * mask [frames][H][W] int64 class maps, frame_of[n] / cls[n] the frame and class id of each fit,
 * xs[W] / ys[H] the float32 mesh axes exactly as torch.linspace(-1,1,.) produces them (utils.py:27-60
 * create_meshgrid; passed in because ATen's vectorised linspace is not a closed formula),
 * init [n][5] (cx,cy,a,b,theta) pixels, out [n][5] doubles, evals[n] IoU evaluation count (optional).
 * nframes = number of class maps in `mask`; a fit whose frame_of is outside [0, nframes) reads nothing and
 * reports NaN.  Each IoU evaluation scans the ellipse's bounding box only (pixels outside it cannot be inside
 * the ellipse, so the counts -- and therefore the search -- are unchanged).  The two candidates of a coordinate step are scored at the
 * same time by different waves and a sweep's closing score is looked up when its parameters were scored before; decisions are taken in the
 * reference's order and evals[] counts the evaluations the reference's sequential search performs (csrc/fit.hip).
 *
 * egne_ellipse_init_from_pred: the seeds of that search straight from the network's regression output on the
 * device (evaluate.py:135-151 does this per frame on the host): elPred [nframes][10] float32 normalised
 * ellipses -> init [2*nframes][5] float64 pixel ellipses via my_ellipse(p).transform(H)
 * (helperfunctions.py:124-129), fit 2f = iris / class 1 from elPred[f][0:5], fit 2f+1 = pupil / class 2 from
 * elPred[f][5:10]; also fills frame_of / cls [2*nframes].
 *
 * egne_ellipse_iou_counts: ONE evaluation of that search per ellipse, through the same device functions the search
 * kernel calls (mask packing and the row-interval evaluation), for tests that compare every count with the
 * reference instead of the search's final result only.  ell [n][5] = (cx, cy, a, b) in pixels and the angle in
 * DEGREES -- what one evaluation of the search is handed; counts [n][3] = pixels of class cls[i] in frame
 * frame_of[i], pixels inside the ellipse, pixels in both (utils.py:176-204 before the division).  roww = 1: one
 * wave, 64 rows per pass; roww = 4: four waves, 256 rows per pass, partial sums added across the waves (the two
 * row splits of the search's launch forms).  A frame_of outside [0, nframes) writes 0xffffffff three times and
 * reads nothing.
 */
int egne_ellipse_fit(const int64_t* mask, int nframes, const int32_t* frame_of, const int32_t* cls, int n,
                     int H, int W, const float* xs, const float* ys, const double* init, double* out,
                     int32_t* evals, void* stream);
int egne_ellipse_init_from_pred(const float* elPred, int nframes, int H, int W, double* init,
                                int32_t* frame_of, int32_t* cls, void* stream);
int egne_ellipse_iou_counts(const int64_t* mask, int nframes, const int32_t* frame_of, const int32_t* cls, int n,
                            int H, int W, const float* xs, const float* ys, const double* ell, uint32_t* counts,
                            int roww, void* stream);

/*
 * Ellipse seeds from the class map (evaluate.py --ellipse_seed mask; csrc/mask_seed.hip; not in the reference): the seed of the
 * search above from the segmentation itself instead of the regression head.  mask [nframes][H][W] int64 class ids; row i < n
 * names a frame (frame_of[i]), a region (class_bits[i]: a pixel belongs iff bit mask[p] is set, ids outside 0..31 never belong)
 * and the class the search is to score against (search_cls[i]).  Per row: label the 8-connected components of the region
 * (multi-launch union-find, the launch boundary is the only synchronisation), choose the one with the most pixels (tie: the one
 * whose first pixel in raster order comes first), accumulate N, Sx, Sy, Sxx, Sxy, Syy over it (x = column, y = row; 64-bit integer
 * adds only, so order-independent) and finalise in float64 (unit-pixel term N*N/12, axes scaled by W/(W-1), H/(H-1): the
 * search's mesh is linspace(-1,1,W) while its pixel map is 2p/W - 1): init [n][5] = (cx, cy, a, b, theta), a the semi-axis along
 * theta.  out_frame_of[i] = frame_of[i], out_cls[i] = search_cls[i], stats [n][8] int64 = (N, Sx, Sy, Sxx, Sxy, Syy, number of
 * components, pixels in the region).  Absent region (class_bits 0, no pixel, N < min_area, frame_of outside [0, nframes)): init
 * -1 five times, out_frame_of -1 (egne_ellipse_fit reads nothing for it), zeros for the six sums.  Every find / union loop stops
 * after 4*H*W + 64 steps: such a row sets bit 0 of the device word `status` (zeroed by the call) and is reported absent.
 * Refused (nothing written): H < 2, W < 2, max(H, W) > 1024, H*W > 2^20.  ws: egne_mask_seed_workspace_bytes(n, H, W) bytes
 * (-1 for a refused shape), aligned to 8.  Seven launches on `stream`, fixed sequence (capturable), no host synchronisation.
 */
int64_t egne_mask_seed_workspace_bytes(int n, int H, int W);
int egne_ellipse_init_from_mask(const int64_t* mask, int nframes, const int32_t* frame_of, const int32_t* class_bits,
                                const int32_t* search_cls, int n, int H, int W, int min_area, double* init,
                                int32_t* out_frame_of, int32_t* out_cls, int64_t* stats, int32_t* status, void* ws,
                                void* stream);

/*
 * Class-map clean-up (evaluate.py --clean_mask 1; csrc/cleanup.hip): which pixels count, decided before any ellipse is
 * fitted.  The first step restates the reference's helperfunctions.clean_mask (:378-392, called by none of its scripts); keeping the
 * largest blob and filling its holes is not in the reference.  Integer-exact.
 * mask [nframes][H][W] int64 class ids; row i < n = (frame_of[i], class_bits[i], paint_cls[i], flags[i]); open3 0 or 1; min_area >= 1.
 * Step 1, opening (open3 = 1), per class id c in 0..31 that a row names: S_c = {p : mask[p] == c}; E_c = the pixels of S_c whose
 * 4-neighbours inside the frame are all in S_c (neighbours outside the frame do not constrain: cv2.erode's default border); O_c = E_c
 * and the 4-neighbours of E_c inside the frame (cv2.dilate, border = background); O_c is a subset of S_c.  A pixel is eligible iff it
 * lies in the O of its own class; with open3 = 0 every pixel with an id in 0..31 is.  Ids outside 0..31 are never eligible.  The
 * element is the cross of cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (3, 3)), restated from OpenCV's documented behaviour.
 * Step 2, per row: R = the eligible pixels of frame frame_of[i] whose bit mask[p] is set in class_bits[i].  flags & 1: K = the
 * 8-connected component of R with the most pixels (tie: the one whose first pixel comes first in raster order, the rule of
 * egne_ellipse_init_from_mask); otherwise K = R.  Fewer than min_area pixels in K: the row paints nothing.  flags & 2: every
 * 4-connected component of frame \ K without a pixel of the first or last row or column is added to K
 * (scipy.ndimage.binary_fill_holes; dropped components of R inside such a hole are filled with it).
 * Step 3: out[f] = fill_cls everywhere, then the rows of frame f paint paint_cls[i] over their K in row order.  A row whose frame_of
 * is outside [0, nframes) paints nothing; a frame no row names is all fill_cls.  Every pixel of out is written exactly once.
 * stats [n][4] int64 = (pixels of R, components of R, pixels of K before filling, pixels added by filling).  Every find / union loop
 * stops after 4*H*W + 64 steps: such a row sets bit 0 of the device word `status` (zeroed by the call) and paints nothing.
 * Refused (nothing written): H < 2, W < 2, max(H, W) > 1024, H*W > 2^20; out overlapping mask.  ws:
 * egne_class_map_cleanup_workspace_bytes(n, H, W) bytes (-1 for a refused shape), aligned to 8: all scratch lives there.  Eleven
 * launches on `stream`, fixed sequence (capturable), no host synchronisation; the launch boundary is the only synchronisation
 * between workgroups.
 */
int64_t egne_class_map_cleanup_workspace_bytes(int n, int H, int W);
int egne_class_map_cleanup(const int64_t* mask, int nframes, const int32_t* frame_of, const int32_t* class_bits,
                           const int32_t* paint_cls, const int32_t* flags, int n, int H, int W, int open3, int min_area,
                           int64_t fill_cls, int64_t* out, int64_t* stats, int32_t* status, void* ws, void* stream);

/*
 * Ellipses from class-map boundaries (csrc/ellifit.hip): the reference's helperfunctions.ElliFit (:209-276) under
 * helperfunctions.ransac (:278-310), the estimator behind its dataset_generation/Extract*.py "Fits", per (frame, region) row on the
 * device -- it replaces ransac(pts, ElliFit, n_min, iters, thres, n_good).loop() and my_ellipse(model).verify(pts) on the host.
 * Rows as for egne_ellipse_init_from_mask plus exclude_bits[i].  Boundary point: in the region, at least one 4-neighbour inside
 * the image outside the region, no pixel of its 3x3 neighbourhood inside the image with its bit set in exclude_bits (class ids
 * outside 0..31 neither belong nor exclude); (x, y) = (column, row) in raster order, at most max_pts (even, <= 16384) of them --
 * a row with more is absent and sets bit 1 of `status`.  Fit(S): float64, centred on S's mean, normal equations of
 * X = [x^2, 2xy, -2x, -2y, -1], Y = -y^2 by Cholesky, model = lines :249-257; a singular system or a non-finite entry makes the
 * model invalid, its error +inf.  Candidate -1 = Fit(all); for N > n_min iterations i = 0..iters: S_i (n_min distinct indices),
 * I = S_i u {p : fit_error(Fit(S_i), p) < thres}, candidate i = Fit(I) iff |I| > max(n_good, n_min), error = mean fit_error over
 * I; result = smallest (error, i).  iters = -1: candidate -1 only.  Fewer than 7 points: absent.
 * draws: int32 [n][iters+1][n_min] indices into the row's point list (an index outside [0, N) or a repeated one sets bit 0 of
 * `status` and makes the row absent), or NULL: generated from `seed` -- attempt t of iteration i of row r is
 * mulhi(hash(seed, r % draw_period, i, t), N), indices already taken are skipped, at most 256 attempts (then bit 0); with
 * draw_period = rows per frame a frame's ellipses do not depend on where in a batch, or in how large a batch, the frame sits
 * (draw_period = n: every row its own stream).  draws_out (may be NULL) receives them, -1 where a row ran no iteration or an
 * iteration's attempts ran out.
 * Outputs per row: raw [n][5] the reference's (cx, cy, a, b, theta); init [n][5] the same ellipse as the search reads it (centre
 * and second-moment form scaled by W/(W-1), H/(H-1), a the semi-axis along theta); out_frame_of / out_cls as the mask seeds (-1
 * and five times -1 where absent); stats_i [n][4] = (N, best iteration, |I| of the best, candidates including -1); stats_f [n][2]
 * = (best error, mean of p^T M p over all points, M = my_ellipse(raw).mat); points_out (may be NULL) int16 [n][max_pts][2], only
 * the first N entries of a row are written.  ws: egne_ellipse_ransac_workspace_bytes(n, H, W, max_pts) bytes (negative for
 * refused sizes: H, W outside 2..1024, max_pts outside 1..16384), aligned to 8.  Five launches on `stream`, fixed sequence
 * (capturable): ballot words, their prefix, the point list, one workgroup of four waves per row for the fits (max_pts*4 + 1552
 * bytes of LDS), one thread per row for the outputs; no host synchronisation, no allocation.
 */
int64_t egne_ellipse_ransac_workspace_bytes(int n, int H, int W, int max_pts);
int egne_ellipse_ransac_from_mask(const int64_t* mask, int nframes, const int32_t* frame_of, const int32_t* class_bits,
                                  const int32_t* search_cls, const int32_t* exclude_bits, int n, int H, int W, int max_pts,
                                  int n_min, int iters, double thres, int n_good, const int32_t* draws, uint32_t seed,
                                  int draw_period, int32_t* draws_out, double* raw, double* init, int32_t* out_frame_of, int32_t* out_cls,
                                  int32_t* stats_i, double* stats_f, int16_t* points_out, int32_t* status, void* ws,
                                  void* stream);

/* Device-side batch preparation (the reference does this per sample on the host in its Dataset).
 * egne_dist_maps: out[b][c] = helperfunctions.one_hot2dist(label[b] == c) (helperfunctions.py:356-371, called from
 *   CurriculumLib.py:131-136): signed exact Euclidean distance transform normalised by the image diagonal, 0 for an absent
 *   class; label int64 [B,H,W], out float32 [B,ncls,H,W] (the float32 cast of the reference's float64 result, bit-identical).
 * egne_zscore: (img - img.mean()) / img.std() per image (CurriculumLib.py:139), statistics in double. */
int64_t egne_dist_maps_workspace_bytes(int B, int H, int W, int ncls);
int egne_dist_maps(const int64_t* label, int B, int H, int W, int ncls, float* out, void* ws, void* stream);
int egne_zscore(const float* x, float* y, int B, int n, void* stream);
/* egne_spatial_weights: 1 + 20 * cv2.dilate(cv2.Canny(label, 0, 1) / 255, (3, 3)) per frame (CurriculumLib.py:128-129); label int64
 *   [B,H,W] (class indices), out float32 [B,H,W].  PARITY UNPINNED: neither OpenCV nor a fixture of this function exists in the
 *   build container; the kernel is bit-identical to the restatement of OpenCV's published algorithm in oracle/dataprep.py. */
int egne_spatial_weights(const int64_t* label, int B, int H, int W, float* out, void* stream);
/* egne_augment: the NumPy branches of data_augment.augment (data_augment.py:12-130; called per sample from CurriculumLib.py:114-120)
 *   over a batch: choice[b] = 0 flip left-right (image and label), 2 gamma = lut[b][pixel] (256-entry uint8 table per frame, built on
 *   the host as the reference builds it), 3 exposure pixel + param[b], 4 noise pixel + param[b] * noise[b][y][x] (standard-normal
 *   draws, double), >= 7 copy; double arithmetic, clip to [0,255], truncation.  The cv2 branches (1 blur, 5 lines, 6 rotate) are not
 *   implemented: the host wrapper rejects them.  img / out_img uint8 [B,H,W], label / out_label int64 [B,H,W]; not in place. */
int egne_augment(const uint8_t* img, const int64_t* label, const int32_t* choice, const double* param, const uint8_t* lut,
                 const double* noise, uint8_t* out_img, int64_t* out_label, int B, int H, int W, void* stream);
/* egne_augment_cv: the OpenCV branches of data_augment.augment (data_augment.py:38-42 cv2.GaussianBlur, :67-79 cv2.line, :99-120
 *   cv2.getRotationMatrix2D + cv2.warpAffine) over the same batch (csrc/augment_cv.hip; egne_amd.data_augment
 *   .augment_batch(on_cv2="device") calls it behind egne_augment, in place of the NotImplementedError of the default mode).  out_img /
 *   out_label must already hold egne_augment's result (a copy for these frames); frames of any other choice are not touched.
 *   frame int32 [B][3] on the device = {choice, sigma, number of kept segments} per frame, frame_host the same array in HOST memory
 *   (validated here: sigma 2..6 for choice 1, at most 9 segments for choice 5; H, W >= 4 when a frame is blurred).
 *   1 cv2.GaussianBlur(img, (7,7), sigma): separable, BORDER_REFLECT_101, taps q8[sigma-2][7] (int32 [5][7], 8-bit fixed point, each
 *     row sums to 256): r = sum q*src, s = sum q*r, out = (s + 32768) >> 16; label unchanged.
 *   5 cv2.line(.., 255, thickness 4) for segs[b][j] = (x1, y1, x2, y2), j < kept (float64 [B][9][4], clipped by the host to
 *     [-4, W+3] x [-4, H+3]): a pixel becomes 255 iff its squared distance to a segment is <= 4.0 (float64, t = clamp(dot / len2, 0, 1),
 *     a zero-length segment is a disc); label unchanged.
 *   6 cv2.warpAffine(.., M, flags=INTER_LANCZOS4 / INTER_NEAREST), BORDER_CONSTANT 0: rot[b] = i00 i01 i02 i10 i11 i12 (float64 [B][6])
 *     is the INVERSE of M; X = ((i00*x) + (i01*y)) + i02, Y likewise.  Image: ix = floor(32*X + 0.5), first tap (ix >> 5) - 3, weights
 *     phase[ix & 31][8] (float64 [32][8], Lanczos a = 4, normalised), same in y; t[ky] = sum_kx wx*src from 0.0 left to right,
 *     v = sum_ky wy*t, out = clip(rint(v), 0, 255).  Label: label[floor(Y + 0.5)][floor(X + 0.5)], 0 outside.
 *   PIXEL PARITY WITH OPENCV UNPINNED (tap rounding of the blur, boundary pixels of the thick line, 15-bit Lanczos weights); the
 *   kernels are byte-identical to the restatement in tests/augment_cv2_refs.py.  Not in place. */
int egne_augment_cv(const uint8_t* img, const int64_t* label, const int32_t* frame, const int32_t* frame_host, const double* segs,
                    const double* rot, const int32_t* q8, const double* phase, uint8_t* out_img, int64_t* out_label, int B, int H,
                    int W, void* stream);
/* Device-side training loader (csrc/loader.hip; egne_amd.loader.device_batch): the stages of the reference's item path
 * (CurriculumLib.py:94-166) in front of and behind the augmentation, for a batch of raw frames.
 * egne_loader_stage: pad2Size (helperfunctions.py:406-428) and, with tap tables, scaleFn (CurriculumLib.py:78-89).  img uint8 and
 *   label int8 [B,Rmax,Cmax]: frame b holds src_hw[b] = (rows, columns) valid pixels (int32 [B,2], device), the rest is ignored.
 *   Every frame is centred in the H x W canvas ((H - rows) / 2 zero rows above, (W - columns) / 2 zero columns left); the caller
 *   refuses odd or negative differences as the reference asserts (whatever src_hw holds, nothing outside a frame's valid pixels,
 *   clamped to the buffer, is read).  Without tables Hs = H, Ws = W and the canvas is the output.  With them the image is the 8-tap
 *   Lanczos resampling of the CANVAS to Hs x Ws: row_idx / row_w [Hs][8], col_idx / col_w [Ws][8] as for egne_eval_prep
 *   (evaluate.lanczos4_table; a NULL pair skips that pass), the same device code, byte-identical to evaluate.resize_lanczos4 (whose
 *   parity with OpenCV is unpinned); the label is canvas[near_row[y]][near_col[x]] (int32 [Hs], [Ws]: evaluate.resize_nearest's
 *   indices).  out_img uint8, out_label int64 [B,Hs,Ws]: what egne_augment takes.  One launch.
 * egne_loader_finish: after the augmentation.  out_label = label with 1 -> 0, 2 -> 1, 3 -> 2 and every other value (-1 too) kept
 *   (CurriculumLib.py:123-125); out_img float32 [B,n] = the z-score of the uint8 image with egne_zscore's float64 statistics and
 *   order of additions, bit-identical to egne_zscore on the float of the same pixels (a constant image: whatever 0 / 0 gives
 *   there).  n = H*W pixels per frame.  One launch: one workgroup per frame for the z-score next to the remap's. */
int egne_loader_stage(const uint8_t* img, const int8_t* label, const int32_t* src_hw, int B, int Rmax, int Cmax, int H, int W,
                      int Hs, int Ws, const int32_t* row_idx, const double* row_w, const int32_t* col_idx, const double* col_w,
                      const int32_t* near_row, const int32_t* near_col, uint8_t* out_img, int64_t* out_label, void* stream);
int egne_loader_finish(const uint8_t* img, const int64_t* label, float* out_img, int64_t* out_label, int B, int n, void* stream);

/* Device-side front and back end of evaluate.py (--device_io 1; csrc/evalio.hip), pinned bit for bit against the host functions there.
 * egne_eval_prep: preprocess_frame(grey, (Ho, Wo), align_width=True) for every eye of a batch of video frames.  src uint8 [N,Hs,Ws];
 *   eye e of frame n is columns [e*We, (e+1)*We) (eyes*We <= Ws); out float32 [N*eyes,1,Ho,Wo], frame-major then eye.
 *   (Hr, Wr) = shape of an eye after the Lanczos resize (int(Hs*sc), int(We*sc), sc = Wo/We; Wr must equal Wo; Hr = Hs, Wr = We
 *   when nothing is resized).  row_idx / row_w [Hr][8] and col_idx / col_w [Wr][8]: the 8 source indices (already clamped to the
 *   border) and normalised float64 weights of every output row / column, exactly as evaluate.resize_lanczos4 builds them
 *   (evaluate.lanczos4_table); a NULL pair skips that pass (its source and resized extent must then agree).  Rows first (sequential
 *   float64 sum), then columns (pairwise float64 sum) with no rounding in between, clip(rint(.), 0, 255).  Rows: zero-padded
 *   (Ho-Hr)/2 above when Hr < Ho, centre-cropped from (Hr-Ho)/2 when Hr > Ho.  z-score from exact 64-bit integer sums S, Q over the
 *   padded image of n = Ho*Wo pixels: mean = S/n, std = sqrt(n*Q - S*S)/n in float64, out = float((x - mean) / std); a constant
 *   image gives NaN as on the host.  u8_out (optional, may be NULL) uint8 [N*eyes,Ho,Wo]: the resized, padded image before the
 *   z-score.  ws: egne_eval_prep_workspace_bytes(N, eyes, Hr, Wr, resize) bytes, resize = 1 when either tap table is given.
 * egne_eval_render: the two uint8 BGR frames of evaluate.py's draw() and the ellipses at source geometry.  src as above; seg int64
 *   [N*eyes,Ho,Wo] class maps, edge float32 [N*eyes,Ho,Wo], fit float64 [N*eyes,2,5] (iris, pupil) x (cx,cy,a,b,theta) at network
 *   geometry; inv_scale = 1 / scale and shift = rows added (+) or removed (-) by the front end (its scale_shift); cos_sin float64
 *   [2][720] = cos(t), sin(t) of t = linspace(0, 2 pi, 720, endpoint=False).  ell_out float64 [N*eyes,2,5]: rescale_to_original
 *   (e[1] -= shift // 2, e[:4] *= inv_scale).  overlay / edge_frame uint8 [N,Hs,Ws,3]: class and edge maps un-padded / zero
 *   re-padded and nearest-resized (floor(dst * n1 / n2), clamped) to (Hs, We) per eye; overlay = grey, class 1 (120,183,53), class 2
 *   (36,231,253), iris outline (255,0,0), pupil outline (0,0,255), outlines as evaluate._draw_ellipse (skipped when all -1 or
 *   non-finite, truncated centre / axes, 720 samples, rint, clipped to the eye); edge_frame = clip(255 - 255*edge, 0, 255) truncated,
 *   formed in float32 at network geometry (re-padded rows are 0); columns beyond eyes*We are copied from src in both frames. */
int64_t egne_eval_prep_workspace_bytes(int N, int eyes, int Hr, int Wr, int resize);
int egne_eval_prep(const uint8_t* src, int N, int Hs, int Ws, int eyes, int We, int Hr, int Wr, const int32_t* row_idx,
                   const double* row_w, const int32_t* col_idx, const double* col_w, int Ho, int Wo, float* out,
                   uint8_t* u8_out, void* ws, void* stream);
int egne_eval_render(const uint8_t* src, int N, int Hs, int Ws, int eyes, int We, const int64_t* seg, const float* edge,
                     const double* fit, int Ho, int Wo, double inv_scale, int shift, const double* cos_sin,
                     uint8_t* overlay, uint8_t* edge_frame, double* ell_out, void* stream);

/* Device-side Motion-JPEG encoder and frame-number stamp of evaluate.py (--device_jpeg 1; csrc/jpeg.hip), pinned byte for byte against
 * the restatement in tests/jpeg_refs.py.  Integer arithmetic throughout: the output is one defined byte string.
 * egne_jpeg_encode: bgr uint8 [N,H,W,3] (any H, W >= 1) -> frame n's complete baseline JPEG file (T.81, JFIF, 4:2:0) at out + n*cap:
 *   `header` copied as given (SOI, APP0, two DQT, SOF0 with sampling 2x2 / 1x1 / 1x1, four DHT, DRI = restart_mcus, SOS), the
 *   entropy-coded scan with RSTm (m cycling 0..7) between restart intervals of restart_mcus (1..8) MCUs, EOI.  lengths[n] = the file's
 *   size, flags[n] = 0; a file that does not fit `cap` bytes gives lengths[n] = 0, flags[n] = 1 and nothing is written for that frame;
 *   no byte is ever written outside [out + n*cap, out + n*cap + lengths[n]).
 *   The frame is extended to multiples of 16 by repeating its last column / row.  Per pixel Y = (19595 R + 38470 G + 7471 B + 32768)
 *   >> 16, Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16, Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16;
 *   chroma = (a + b + c + d + 2) >> 2 of every 2 x 2 group.  F = T s T^t of s = plane - 128 in exact integers, dct = T int32 [8][8],
 *   T[u][x] = rint(8192 a(u) cos((2x+1) u pi / 16)).  qt uint8 [2][64]: luminance / chrominance divisors q in zigzag order;
 *   v = sign(F) * ((|F| + (q << 25)) / (q << 26)).  Entropy coding as T.81 F.1.2: MCU = Y00 Y01 Y10 Y11 Cb Cr, DC predictors 0 at
 *   every interval, ZRL, EOB unless coefficient 63 is non-zero, MSB first, 0x00 behind every 0xFF, last byte filled with 1-bits.
 *   huff uint32 [544]: entry = (code length << 16) | code; [0,16) DC luminance by category, [16,32) DC chrominance, [32,288) AC
 *   luminance by (run << 4 | category), [288,544) AC chrominance; unused entries 0.  The tables live on the device and are not
 *   checked: a code longer than 16 bits gives an undefined stream (never a write outside the slot).  ws: egne_jpeg_workspace_bytes(N, H, W) bytes,
 *   16-byte aligned.  Bit-identical from run to run.
 * egne_stamp_mask: blends the grey patch mask[n] (uint8 [N,ph,pw]) at origin (x0, y0), clipped to the frame, into bgr [N,H,W,3] in
 *   place, as PIL's ImageDraw.text does: per channel t = src*(255 - a) + ink*a + 128, dst = ((t >> 8) + t) >> 8. */
int64_t egne_jpeg_workspace_bytes(int N, int H, int W);
int egne_jpeg_encode(const uint8_t* bgr, int N, int H, int W, const uint8_t* qt, const void* huff, const int32_t* dct,
                     const uint8_t* header, int header_len, int restart_mcus, uint8_t* out, int64_t cap, int32_t* lengths,
                     int32_t* flags, void* ws, void* stream);
int egne_stamp_mask(uint8_t* bgr, int N, int H, int W, const uint8_t* mask, int ph, int pw, int x0, int y0, int b, int g, int r,
                    void* stream);

/* Device-side Motion-JPEG decoder of evaluate.py (--device_decode 1; csrc/jpeg_decode.hip, csrc/jpeg_decode_core.h): the scans of N
 * baseline JPEG files (T.81 SOF0, 8 bit, one scan, Huffman) -> grey frames, byte for byte what libjpeg-turbo's default decode path
 * (jidctint "islow", fancy upsampling) followed by PIL's convert('L') gives; pinned against the restatement in
 * tests/jpeg_decode_refs.py, which tests/test_host_jpeg_decode.py holds against PIL.  Integer arithmetic with arithmetic shifts
 * throughout.  The host parses the marker segments (evaluate.jpeg_parse) and does nothing per Huffman symbol.
 * egne_jpeg_decode: streams = the entropy-coded scans (everything between SOS and EOI: 0x00 stuffing and RSTm still inside) of all
 *   frames in one buffer of stream_bytes bytes (a multiple of 4), every scan at a multiple of 4, the scans disjoint and in the frames'
 *   order (scan_off + scan_len of frame n <= scan_off of frame n+1: the per-frame slots of the workspace are placed by scan_off, and
 *   only each record alone is checked on the device -- records that overlap or run backwards stay in bounds but decode wrongly);
 *   all frames share H, W and `sampling`:
 *   0 grey (one component, MCU = one block), 1 = 4:4:4, 2 = 4:2:2 (Y 2x1), 3 = 4:2:0 (Y 2x2); chroma components 1x1, MCU = the Y blocks
 *   in raster order, Cb, Cr.  desc: one record of 1408 bytes per frame --
 *     int32 [8]: scan_off, scan_len (bytes), restart interval in MCUs (0 = none), tq, td, ta (byte c of each = the quantisation / DC /
 *       AC table of component c), 0, 0;
 *     uint8 [4][64] from byte 32: the quantisation tables 0..3 in file (zigzag) order;
 *     uint8 [4][272] from byte 288: the code tables DC 0, DC 1, AC 0, AC 1, each 16 counts (codes of length 1..16) + 256 symbols.
 *   A record is checked on the device (range of the scan, alignment, restart interval); a bad one only flags its frame.
 *   Stages: (a) per frame, the byte behind every 0xFF is dropped (and the 0xFF too where that byte is RSTm: a segment starts there; a
 *   frame without restart interval is one segment, whose start state is known: byte-aligned, DC predictors 0, first block of an MCU);
 *   (b) entropy decode, T.81 F.2.2: mode 0 = one lane walks one segment from start to end -- the form this contract is stated in;
 *   mode 1 = every segment is cut into subsequences of sub_bits bits (a multiple of 32 in 128..4096) that lanes decode from guessed
 *   states and re-decode from their left neighbour's exit state until a workgroup-wide vote finds nothing changed (at most one round
 *   per subsequence; one workgroup per frame, 256 subsequences at a time, no waiting between workgroups): the result is exactly mode
 *   0's for every stream, valid or not in its bits.  Bits beyond the end of the frame's scan read as 1.  (c) coefficient k of a block
 *   times q[k], IDCT islow (CONST_BITS 13, PASS1_BITS 2: columns descaled by 11, rows by 18, DESCALE(x, n) = (x + (1 << (n-1))) >> n)
 *   in 64 bits, clip(x + 128); chroma planes cropped to ceil(H/v) x ceil(W/h) and upsampled with replicated edges -- 4:2:0: s = 3 *
 *   nearer row + the row above (even output rows) / below (odd), out[2i] = (3 s[i] + s[i-1] + 8) >> 4, out[2i+1] = (3 s[i] + s[i+1] +
 *   7) >> 4; 4:2:2: out[2i] = (3 c[i] + c[i-1] + 1) >> 2, out[2i+1] = (3 c[i] + c[i+1] + 2) >> 2 --; with cb, cr centred on 0: R =
 *   clip(Y + ((91881 cr + 32768) >> 16)), G = clip(Y + ((-22554 cb + 32768 - 46802 cr) >> 16)), B = clip(Y + ((116130 cb + 32768) >>
 *   16)), L = (19595 R + 38470 G + 7471 B + 32768) >> 16; grey streams: L = Y.  (libjpeg replicates instead of interpolating chroma
 *   planes of one or two columns: evaluate.jpeg_parse leaves such files to the host.)
 *   grey_out uint8 [N,H,W].  flags int32 [N]: 0, or 1 for a frame with a bad record, a code no table holds, a DC category above 11 or
 *   AC category above 10, a run that is neither ZRL nor EOB with category 0, a zigzag index past 63, a symbol that ends behind its
 *   segment, a segment with fewer blocks than it must hold or with more than 7 bits behind its last block, or a count of RSTm that
 *   is not the segments' minus one; such a frame's row of grey_out (and of coef_out) is unspecified, and nothing outside frame n's
 *   rows is ever written for frame n.  coef_out (optional, may be NULL; for the tests) int16 [N, blocks, 64]: the quantised
 *   coefficients in zigzag order after DC prediction, blocks in MCU order.  stats (optional, may be NULL; for the tests) int32 [N,2]:
 *   (synchronisation rounds of the frame's deepest window -- 0 in mode 0 --, subsequences; mode 0: segments).  ws:
 *   egne_jpeg_decode_workspace_bytes(N, H, W, sampling, stream_bytes, sub_bits, coef_out == NULL) bytes, 16-byte aligned.  Bit-identical
 *   from run to run and between the modes and all values of sub_bits. */
int64_t egne_jpeg_decode_workspace_bytes(int N, int H, int W, int sampling, int64_t stream_bytes, int sub_bits, int own_coef);
int egne_jpeg_decode(const uint8_t* streams, int64_t stream_bytes, const uint8_t* desc, int N, int H, int W, int sampling,
                     int sub_bits, int mode, uint8_t* grey_out, int16_t* coef_out, int32_t* flags, int32_t* stats, void* ws,
                     void* stream);

/*
 * ---- bf16 activation storage (training plans; BASELINE.json configs[2..4], reference loop train.py:262-287, --prec args.py:17-28) ----
 * Twins of the entry points above for plans that keep activations and activation gradients in HBM as bf16 (NHWC, strides and
 * offsets in ELEMENTS, slices on multiples of 4 elements): same arguments, every activation / gradient pointer addresses bf16
 * elements, all arithmetic and every statistic / table / parameter gradient stays fp32 (fp64 partial sums as in the fp32 forms),
 * stores round to nearest even.  Descriptor-based convolutions (egne_conv2d_fwd, egne_conv3x3_smallcin_fwd, egne_conv2d_wgrad)
 * and the loss head take the storage type from egne_conv_desc.dtype / egne_loss_desc.dtype instead of a twin.
 */
int egne_norm_stats_bf16(const void* x, int64_t pix_stride, int ch_off, int Cp, int B, int HW, int per_sample, float eps,
                         float* scale, float* shift, float* mean_out, float* var_out, void* ws, void* stream);
int egne_affine_bf16(const void* x, int64_t xs, int xo, void* y, int64_t ys, int yo, int Cp, int64_t npix, const float* scale,
                     const float* shift, void* stream);
int egne_avgpool2_bf16(const void* x, int64_t xs, int xo, void* y, int64_t ys, int yo, int B, int H, int W, int Cp, void* stream);
int egne_norm_act_pool2_bf16(const void* x, int64_t xs, int xo, const float* scale, const float* shift, int act, void* y,
                             int64_t ys, int yo, int B, int H, int W, int Cp, void* stream);
int egne_upsample2x_bf16(const void* x, int64_t xs, int xo, void* y, int64_t ys, int yo, int B, int H, int W, int Cp, void* stream);
int egne_nchw_to_nhwc_bf16(const float* x, int B, int C, int H, int W, void* y, int64_t ys, int yo, int Cp, void* stream); /* fp32 in */
int egne_ellipse_head_act_bf16(void* x, int B, int ld, void* stream);
int egne_selu_inplace_bf16(void* x, int64_t n, void* stream);
int egne_spatial_mean_bf16(const void* x, int64_t pix_stride, int ch_off, int C, int B, int HW, void* out, void* stream); /* bf16 out */
int egne_softmax3_bf16(const void* x, int64_t xs, int xo, void* y, int64_t ys, int yo, int Cp_out, int64_t npix, void* stream);
int egne_adain_bf16(const void* x, int64_t xs, int xo, int C, const void* gamma, const void* beta, int64_t gb_stride, int gb_off,
                    void* y, int64_t ys, int yo, int B, int HW, float eps, void* stream);
int egne_conf_loss_bf16(const void* pred, int ld, const int64_t* gt, int B, int C, int flag, float weight, float* terms, void* stream);
int egne_loss_bwd_bf16(const egne_loss_desc* d, const float* gscale, void* g_logits, int64_t gs, int go, float* g_elOut, void* stream);
int egne_act_bwd_bias_bf16(void* g, int64_t gs, int go, const void* y, int64_t ys, int yo, int act, int Cp, int64_t npix,
                           float* dbias, int C, int accumulate, void* ws, void* stream);
int egne_pair_bias_bwd_bf16(const void* g, int64_t gs, int go, int Cp, int B, int H, int W, const void* act_ws, const float* w,
                            int Cout, int Ca, float* db_b, float* db_a, void* ws, void* stream);
int egne_norm_bwd_bf16(const void* x, int64_t xs, int xo, const float* scale, const float* shift, const float* gamma,
                       const void* gy, int64_t gs, int go, int act_in, int Cp, int B, int HW, int per_sample, void* gx,
                       int64_t gxs, int gxo, float* sums, float* dgamma, float* dbeta, int C, void* ws, void* stream);
int egne_norm_bwd_store_bf16(const void* x, int64_t xs, int xo, const float* scale, const float* shift, const float* gamma,
                             const void* gy, int64_t gs, int go, int act_in, int Cp, int B, int HW, int per_sample, void* gx,
                             int64_t gxs, int gxo, float* sums, float* dgamma, float* dbeta, int C, void* ws, void* stream);
int egne_norm_pool2_bwd_bf16(const void* x, int64_t xs, int xo, const float* scale, const float* shift, const void* gzp,
                             int64_t gs, int go, int act_in, int Cp, int B, int H, int W, void* gx, int64_t gxs, int gxo,
                             int accumulate, float* sums, void* ws, void* stream);
int egne_avgpool2_bwd_bf16(const void* gy, int64_t gs, int go, void* gx, int64_t xs, int xo, int B, int H, int W, int Cp, void* stream);
int egne_upsample2x_bwd_bf16(const void* gy, int64_t gs, int go, void* gx, int64_t xs, int xo, int B, int H, int W, int Cp, void* stream);
/* egne_upsample2x_bwd with gx STORED instead of accumulated onto (round 5: the first writer of a gradient slice) */
int egne_upsample2x_bwd_store(const float* gy, int64_t gs, int go, float* gx, int64_t xs, int xo, int B, int H, int W, int Cp, void* stream);
int egne_upsample2x_bwd_store_bf16(const void* gy, int64_t gs, int go, void* gx, int64_t xs, int xo, int B, int H, int W, int Cp, void* stream);
int egne_ellipse_head_act_bwd_bf16(void* g, const void* y, int B, int ld, void* stream);
int egne_selu_bwd_bf16(void* g, const void* y, int64_t n, void* stream);
int egne_softmax3_bwd_bf16(const void* y, int64_t ys, int yo, const void* gy, int64_t gs, int go, void* gx, int64_t xs, int xo,
                           int64_t npix, void* stream);
int egne_adain_bwd_bf16(const void* x, int64_t xs, int xo, int C, const void* gamma, int64_t gb_stride, int gb_off, const void* gy,
                        int64_t gys, int gyo, void* gx, int64_t gxs, int gxo, void* ggamma, void* gbeta, int64_t gg_stride,
                        int gg_off, int B, int HW, float eps, void* stream);
int egne_reflect_pad_bwd_bf16(const void* gpad, int64_t gs, int go, int phase, int Cp, void* gx, int64_t xs, int xo, int B, int H,
                              int W, int P, void* stream);
int egne_spatial_mean_bwd_bf16(const void* g, int gld, void* gx, int64_t xs, int xo, int C, int B, int HW, void* stream);
int egne_conf_loss_bwd_bf16(const void* pred, int ld, const int64_t* gt, int B, int C, int flag, const float* gscale, void* gpred,
                            int gld, void* stream);

/*
 * 3x3 / stride 1 / pad 1 / dilation 1 convolution over ONE bf16 input slice on v_mfma_f32_16x16x32_bf16 (fp32 accumulate): the
 * 3x3 convolutions of models/RITnet_v2.py:57-62,85-87 and utils.py:1047-1048 and their data gradients (a 3x3 over gz with
 * flipped / transposed weights) in training plans with bf16 storage (egne_conv_desc.dtype must be 1).  Descriptor as for
 * egne_conv3x3_rw_f16_fwd: optional fused per-(n,c) affine + activation on load, bias, activation, residual (bf16, accumulated
 * onto in fp32), Ktot = slice width rounded up to 32, CoutP a multiple of 32 (<= 256), Cout_store a multiple of 8.  wfrag: the
 * weights rounded to bf16 in MFMA-fragment order [tap][Ktot/16][CoutP/32][lane][8] (egne_pack_conv_weight_bf16frag; fp32 master
 * weights stay with the caller).
 */
int egne_pack_conv_weight_bf16frag(const float* w_oihw, int Cout, int Cin, int kh, int kw, int CoutP, int Ktot, void* wfrag,
                                   void* stream);
/* ... and the fragments of its DATA GRADIENT w.r.t. input channels [c0, c0 + cn) of the forward weight w_oihw [Cout][Cin][kh][kw]: an
 * ordinary convolution over gz with W'[ci][co][j][i] = w[co][c0 + ci][kh-1-j][kw-1-i] (CoutP >= cn rows, Ktot >= Cout columns). */
int egne_pack_conv_weight_bf16frag_dgrad(const float* w_oihw, int Cout, int Cin, int kh, int kw, int c0, int cn, int CoutP, int Ktot,
                                         void* wfrag, void* stream);
int egne_conv3x3_bf16_fwd(const egne_conv_desc* d, const void* wfrag, void* stream);

/*
 * k x k (k = 3, 5, 7) / stride 1 / zero-padded convolution with a NARROW output (Cout_store <= 8) over ONE bf16 slice of 32 or 64
 * channels, LDS-resident halo, v_mfma_f32_16x16x32_bf16 (egne_conv_desc.dtype must be 1; d.w = the fp32 flat pack
 * [tap][CoutP][Ktot] of egne_pack_conv_weight, rounded to bf16 inside).  Replaces egne_conv2d_fwd for the data gradient of the
 * StyleEncoder's reflect-padded 7x7 (models/RITnet_v2.py:95 under train.py:285-286: 64 channels back to the 3 softmax channels
 * over 49 taps), which the implicit GEMM ran at 22 TFLOP/s.  egne_conv_narrow_bf16_supported tells whether a descriptor qualifies.
 */
int egne_conv_narrow_bf16_supported(const egne_conv_desc* d);
int egne_conv_narrow_bf16_fwd(const egne_conv_desc* d, void* stream);

/*
 * 3x3 / stride 1 / pad 1 convolution with a NARROW output (<= 4 channels; Cout_store <= 8, stored channels past the fourth are
 * written as zeros: the padding of an 8-channel slice) over ONE raw fp32 slice of 4..64 channels, EXACT fp32 on
 * the vector ALU (one rounding per fused multiply-add, accumulation tap-major then channel; bias, optional ReLU / LeakyReLU, post affine): the
 * logits layer of ESF-Net (models/RITnet_v2.py:249 `final` / utils.py:1047 convBlock conv2: 32 -> 3 classes at 240x320), which the
 * matrix kernels ran as a 32-wide output block.  d.w = [9 taps][CP][4 outputs] fp32 from egne_pack_conv3x3_narrow_weight (CP = the
 * slice's channels rounded up to 32; 64-byte aligned; read through the scalar cache; d.Ktot / d.CoutP are ignored).  Post affine
 * allowed; no residual / statistics / fused input affine; egne_conv3x3_narrow_supported tells whether a descriptor qualifies.
 * Replaces egne_conv3x3_rw_f16_fwd for that layer in inference plans (egne_conv2d_fwd semantics).
 */
int egne_pack_conv3x3_narrow_weight(const float* w_oihw, int Cout, int Cin, float* out, void* stream);
int egne_conv3x3_narrow_supported(const egne_conv_desc* d);
int egne_conv3x3_narrow_fwd(const egne_conv_desc* d, void* stream);

/*
 * 1x1 convolution over up to EGNE_MAXSEG RAW bf16 slices on v_mfma_f32_32x32x16_bf16 (fp32 accumulate, bf16 output): conv21 / conv31
 * of the dense blocks, Transition_down behind its pooling, conv11 / conv21 of the up blocks (models/RITnet_v2.py:38-41,59-61,85-86)
 * and their merged data gradients in training plans with bf16 storage (dtype 1).  Streaming: a lane's operand of a 16-channel
 * k-step is one 16-byte load of 8 channels of its pixel, the weights (bf16 fragments [k-step][CoutP/32][lane][8], every slice
 * padded to whole k-steps; egne_pack_conv1x1_bf16 builds them from the fp32 pack [CoutP][Ktot] of the same descriptor) stay in
 * LDS.  Bias, activation and an accumulated bf16 residual as for egne_conv2d_fwd; no fused affine, no post affine.
 * egne_conv1x1_bf16_pack_elems: bf16 elements of the fragment pack (-1: too many k-steps).
 */
int64_t egne_conv1x1_bf16_pack_elems(const egne_conv_desc* d);
int egne_pack_conv1x1_bf16(const egne_conv_desc* d, const float* wflat, const int32_t* seginfo, void* wfrag, void* stream);
/* Several 1x1 convolutions over the SAME bf16 input slices in one launch (round 5): the per-member data gradients of a 1x1 over a
 * would-be torch.cat (models/RITnet_v2.py:59-61,85-86; replaces one egne_conv1x1_bf16_fwd per member, each re-reading gz).
 * A destination may be the LAST writer of its gradient slice: then it applies the activation mask of the layer whose output the
 * slice is the gradient of (mask_y, act: gz = g * act'(y), the pass egne_act_bwd_bias would make); ONE destination per launch (at most
 * 128 channels) may also leave the channel sums of its stored values for that layer's bias gradient (sums: one row [C] per wave,
 * egne_conv1x1_bf16_multi_waves rows, added by egne_group_sums_reduce in a fixed order). */
#define EGNE_MAXDST 6
typedef struct {
  void* out; int64_t out_pix_stride; int32_t out_ch_off;
  int32_t C;                    /* channels stored (multiple of 8) */
  int32_t CoutP;                /* rows of this destination's weight pack (multiple of 32) */
  const void* wfrag;            /* egne_pack_conv1x1_bf16 fragments for (the input slices, CoutP) */
  const void* residual; int64_t res_pix_stride; int32_t res_ch_off;      /* optional accumulated tensor (bf16) */
  const void* mask_y; int64_t mask_pix_stride; int32_t mask_ch_off;      /* optional: activated output whose sign masks the result */
  int32_t act;                  /* egne_act of that layer */
  float* sums;                  /* optional [egne_conv1x1_bf16_multi_waves][C] */
  int64_t res_pixels;           /* 0: the residual covers every pixel; k > 0: only the first k pixels accumulate (the rest of the slice has
                                 * no earlier writer: the decoder's skip gradients reach the image half of the encoder's batch only) */
} egne_dst;
int egne_conv1x1_bf16_multi_supported(const egne_conv_desc* d, int ndst, const egne_dst* dsts);
int egne_conv1x1_bf16_multi_fwd(const egne_conv_desc* d, int ndst, const egne_dst* dsts, void* stream);
int64_t egne_conv1x1_bf16_multi_waves(const egne_conv_desc* d, int ndst, const egne_dst* dsts);   /* rows of egne_dst.sums the launch writes */
int egne_group_sums_reduce(const float* sums, int64_t nrows, int ld, int C, float* out /* [C], may be NULL */, double* total /* [C], may be NULL */,
                           int accumulate, void* stream);
int egne_conv1x1_bf16_fwd(const egne_conv_desc* d, const void* wfrag, void* stream);

/* ----------------------------------------------------------------------------------------------------------------------------
 * Which forward entry point serves a convolution (round 6, csrc/dispatch.hip).  The reference leaves the choice of a kernel to ATen
 * (F.conv2d at models/RITnet_v2.py:57-62,85-87, bdcn_new.py:49-55, vgg16_c.py:65-88); here the engine's planner makes it
 * (engine.Plan._conv_impl / _conv_bf16) and this function restates its predicates, in its order, with its default thresholds, for
 * callers that bind this header directly: describe the layer, get the entry point (egne_conv_kind + the `kind` string the planner
 * records in Plan.meta) and what its epilogue takes along (statistics, pooled output, frames handed to the flat kernel behind the
 * deep trunk kernel, workspace of the small-problem form).  The planner checks every convolution it plans against this function
 * under EGNE_CHECK_DISPATCH=1.  Pair fusions (1x1 into the 3x3 that consumes it, Transition_down with its pooling) are decided
 * by the plan builder before a layer gets here. */
typedef enum {
  EGNE_KIND_IGEMM = 0,            /* egne_conv2d_fwd (exact fp32 implicit GEMM; bf16 tensors too) */
  EGNE_KIND_HALO_F32 = 1,         /* egne_conv3x3_halo_fwd */
  EGNE_KIND_SMALLCIN = 2,         /* egne_conv3x3_smallcin_fwd */
  EGNE_KIND_NARROW_F32 = 3,       /* egne_conv3x3_narrow_fwd */
  EGNE_KIND_F16X3_FLAT = 4,       /* egne_conv2d_f16x3_fwd */
  EGNE_KIND_F16X3_SMALL = 5,      /* egne_conv2d_f16x3_small_fwd */
  EGNE_KIND_F16X3_BIG = 6,        /* egne_conv2d_f16x3_big_fwd (+ egne_conv2d_f16x3_fwd for tail_frames); with f16_products = 1 and egne_conv2d_f16_big1_supported(): egne_conv2d_f16_big1_fwd */
  EGNE_KIND_F16X3_HALO = 7,       /* egne_conv3x3_halo_f16_fwd */
  EGNE_KIND_F16X3_RS = 8,         /* egne_conv3x3_rs_f16_fwd */
  EGNE_KIND_F16X3_RW = 9,         /* egne_conv3x3_rw_f16_fwd */
  EGNE_KIND_F16X3_LATTICE = 10,   /* three egne_conv3x3_halo_f16_fwd launches on dilation lattices */
  EGNE_KIND_F16X3_MSDIL = 11,     /* egne_msblock_dil(_scores)_f16_fwd */
  EGNE_KIND_F16X3_STREAM1X1 = 12, /* egne_conv1x1_f16x3_fwd */
  EGNE_KIND_F16X3_GEMM1X1 = 13,   /* egne_conv1x1_ms_f16x3_fwd */
  EGNE_KIND_F16X3_FIRST = 14,     /* egne_conv3x3_smallcin_f16_fwd */
  EGNE_KIND_BF16_3X3 = 15,        /* egne_conv3x3_bf16_fwd */
  EGNE_KIND_BF16_1X1 = 16,        /* egne_conv1x1_bf16_fwd */
  EGNE_KIND_BF16_NARROW = 17      /* egne_conv_narrow_bf16_fwd */
} egne_conv_kind;

typedef struct {
  int32_t dtype;                  /* storage of the activation tensors: 0 fp32, 1 bf16 (egne_conv_desc.dtype) */
  int32_t B, H, W;                /* frames and INPUT map */
  int32_t kh, kw, stride, pad_h, pad_w, pad_mode, ngroups;     /* padding in TAPS, as in egne_conv_desc (a dilated "same" 3x3: 1) */
  int32_t dil[EGNE_MAXGROUP];
  int32_t nseg;                   /* input slices in concat order */
  int32_t seg_C[EGNE_MAXSEG];     /* logical channels */
  int32_t seg_Cp[EGNE_MAXSEG];    /* stored channels (padded to 8) */
  int32_t seg_ch_off[EGNE_MAXSEG];
  int64_t seg_pix_stride[EGNE_MAXSEG];
  int32_t seg_affine[EGNE_MAXSEG];/* 1: per-(n, c) affine (+ activation) applied on load (egne_seg.scale) */
  int32_t seg_planar;             /* the one slice is an NCHW tensor read in place (first layer) */
  int32_t seg_presplit;           /* the one slice is in split-pair storage: the value of egne_seg.presplit (1, or 3 = channel order; 3 changes no choice:
                                   * the deep trunk, flat and halo kernels read it in place of the fp32 tensor) */
  int32_t Cout;                   /* logical output channels of ONE group */
  int32_t Cout_store;             /* channels the layer stores (0: Cout rounded up to 8) */
  int32_t dst_Cp, dst_ch_off; int64_t dst_pix_stride;
  int32_t act, has_post, has_residual; int64_t res_pix_stride; int32_t res_ch_off;
  int32_t split;                  /* k x k products may be split-f16 (22-bit significand; ConvLayer.split) */
  int32_t split1;                 /* the same for a 1x1 over raw slices (ConvLayer.split1) */
  int32_t split_c4;               /* ... for a first layer on <= 4 channels (ConvLayer.split_c4) */
  int32_t train;                  /* the plan records a backward pass */
  int32_t dyn_scales;             /* split-f16 pre-scales are taken on the device (training plans with fp32 storage) */
  int32_t is_dgrad;               /* the layer is a data gradient (derived weights) */
  int32_t want_stats;             /* the consumer needs InstanceNorm statistics of the output */
  int32_t want_pool; int32_t pool_Cp; int64_t pool_pix_stride;   /* a 2x2 ceil-mode max pooling of the result is wanted */
  int32_t want_scores;            /* MSBlock: the block's share of the stage's score maps instead of its output */
  int32_t up_add;                 /* a half-resolution addend is up-sampled into the result (streaming 1x1) */
  int32_t narrow_bf16_ok;         /* dtype 1: egne_conv_narrow_bf16_supported said yes on the finished descriptor */
  int32_t f16_products;           /* egne_conv_desc.f16_products of the plan's split-f16 launches (1: plain f16 operands -- the role-split / streamed-weights
                                   * 3x3 forms then take maps from 30 pixels of width on) */
  int32_t f16_storage;            /* the input slice or the destination is held as f16 (egne_seg.presplit = 2 / egne_conv_desc.out_split = 2) */
} egne_conv_query;

typedef struct {
  int32_t kind;                   /* egne_conv_kind */
  char name[32];                  /* the planner's name for it ("conv_f16x3:rw", "conv_bf16:3x3", ...) */
  int32_t tail_frames;            /* EGNE_KIND_F16X3_BIG: trailing frames that go to egne_conv2d_f16x3_fwd (whole rounds of 256 workgroups for the rest) */
  int32_t fused_stats;            /* the launch writes the statistics partial sums (egne_conv_desc.stats_ws) */
  int32_t fused_pool;             /* ... and the pooled output (egne_conv_desc.pool_out) */
  int64_t small_ws_floats;        /* EGNE_KIND_F16X3_SMALL: workspace of egne_conv2d_f16x3_small_fwd */
} egne_conv_choice;

int egne_conv2d_auto_kind(const egne_conv_query* q, egne_conv_choice* out);

/* ---- score tracking of train.py / test.py on the device (csrc/scores.hip, egne_amd.scores) -----------------------------------
 * What the reference computes per batch on host copies of the class map and the labels -- utils.py:120-170 (getSeg_metrics,
 * getPoint_metric, getAng_metric) and the loop body train.py:289-338 -- from tensors that are on the device already.  Both calls
 * queue work on `stream` and synchronise nothing.
 *
 * egne_seg_confusion_counts: y_true, y_pred int64 [B,H,W] (contiguous, 8-byte aligned; 16-byte loads are used when both pointers
 *   agree modulo 16, frames of odd size included); counts uint32 [B, ncls, 3] = (n_true, n_pred, n_both) per frame and class,
 *   zeroed by the call itself.  ncls is 2 or 3; values outside [0, ncls) count for no class.  H * W < 2^31, B <= 65535.
 *   A workgroup takes EGNE_SCORES_CHUNK pixels of one frame (grid: chunks x frames) and adds its sums with integer atomics:
 *   the result does not depend on the order.
 *
 * egne_score_rows: one row of EGNE_SCORE_FIELDS float64 per sample, written at ledger[row_offset + i].  All vectors float32:
 *   elOut, elPred [B,10]; pupil_center, iris_center [B,2] in pixels; elNorm [B,2,5]; cond [B,ncond] (non-zero = set, ncond >= 2);
 *   loss_terms: one float32 read on the device (element 0), or NULL (the field is NaN).  Fields:
 *     IOU + c            NaN if cond[:,1] is set or class c is absent from the truth, else n_both / (n_true + n_pred - n_both)
 *     DIST_*             raw (unflagged) centre distances in pixels, float32 arithmetic as utils.unnormPts + getPoint_metric, widened:
 *                        pupil: pupil_center against elOut[:,5:7] (latent) / elPred[:,5:7] (seg); iris: iris_center against [:,0:2]
 *     ANG_IRIS / _PUPIL  float32 |elNorm[:,k,4] - elOut[:,4 or 9]| widened, times 180 / pi in float64 (np.rad2deg)
 *     SCALE_IRIS/_PUPIL  float32 sqrt((a_gt^2 + b_gt^2) / (a_pred^2 + b_pred^2)) from elNorm[:,k,2:4] and elOut[:,2:4 or 7:9], widened
 *     COND0, COND1       0 or 1
 *     LOSS, BATCH        loss_terms[0] widened; batch_no as passed
 *     SAMPLE             index of the sample in its batch */
#define EGNE_SCORES_CHUNK 2048
#define EGNE_SCORE_IOU 0
#define EGNE_SCORE_DIST_PUPIL_LATENT 3
#define EGNE_SCORE_DIST_PUPIL_SEG 4
#define EGNE_SCORE_DIST_IRIS_LATENT 5
#define EGNE_SCORE_DIST_IRIS_SEG 6
#define EGNE_SCORE_ANG_IRIS 7
#define EGNE_SCORE_ANG_PUPIL 8
#define EGNE_SCORE_SCALE_IRIS 9
#define EGNE_SCORE_SCALE_PUPIL 10
#define EGNE_SCORE_COND0 11
#define EGNE_SCORE_COND1 12
#define EGNE_SCORE_LOSS 13
#define EGNE_SCORE_BATCH 14
#define EGNE_SCORE_SAMPLE 15
#define EGNE_SCORE_FIELDS 16
int egne_seg_confusion_counts(const void* y_true, const void* y_pred, int B, int H, int W, int ncls, void* counts, void* stream);
int egne_score_rows(const void* counts, int B, int ncls, const void* elOut, const void* elPred, const void* pupil_center,
                    const void* iris_center, const void* elNorm, const void* cond, int ncond, const void* loss_terms, int H, int W,
                    int batch_no, void* ledger, int64_t row_offset, int64_t capacity_rows, void* stream);

/* ---- ellipse scores of test.py against ground truth (csrc/ellipse_scores.hip, egne_amd.scores.EllipseLedger) ------------------
 * The block the reference keeps behind bbox_iou_flag (test.py:108-155): per sample and region (0 iris, 1 pupil) the IoU of the
 * rotated bounding boxes of the scored and the ground-truth ellipse (calc_box_iou.py:13-54) and the absolute differences of their
 * parameters; also the IoU of the two ellipses themselves and of either against the class map.  All calls queue work on `stream`,
 * synchronise nothing, use no atomics and give the same bits on every run.
 *
 * egne_ellipse_pair_scores: one row of EGNE_ELLSCORE_FIELDS float64 per sample at ledger[row_offset + i]; one workgroup per (sample,
 *   region).  elNorm [B,2,5] float32, the ground truth on the normalised mesh; pred_px [B,2,5] float64, the scored ellipses in
 *   pixels (cx, cy, a, b, theta) -- from egne_ellipse_init_from_pred, from egne_ellipse_fit or from anywhere else; mask [B,H,W]
 *   int64 class map; cond [B,ncond] float32 (non-zero = set, ncond >= 2); cls_iris / cls_pupil: the class of the map each region
 *   is held against, negative = the region is not scored and its fields are NaN; xs[W] / ys[H]: the mesh axes as egne_ellipse_fit
 *   takes them.  H, W from 2 up to the limit of egne_ellipse_fit.  The ground-truth pixel ellipse is the transform of
 *   egne_ellipse_init_from_pred (the same device function).  Fields of a region, at r * EGNE_ELLSCORE_REGION_FIELDS:
 *     ELL_PRED, ELL_GT     5 each: the two pixel ellipses
 *     CORNERS_PRED, _GT    8 each: (x0, y0, ..., x3, y3) of calc_bbox in float64 -- centre rotated by -theta, corners (-a,-b), (-a,+b),
 *                          (+a,+b), (+a,-b) around it, each rotated by theta -- converted to int32 as NumPy converts (truncation toward
 *                          zero; NaN and values outside int32 give INT_MIN)
 *     BOX_IOU, _AND, _OR   n_and / n_or in float64 (NaN for 0 / 0) and the two counts over the H x W canvas.  A pixel (x, y), 0 <= x < W,
 *                          0 <= y < H, belongs to a box iff for each of its four edges k -> k+1 the cross product
 *                          (x[k+1]-x[k]) (y-y[k]) - (y[k+1]-y[k]) (x-x[k]), in exact integers, has the sign of the box's signed area or
 *                          is zero; a box without area holds the pixels exactly on its four segments.  (cv2.fillPoly agrees away
 *                          from the edges; which edge pixels it sets is not restated.)
 *     PARA                 5: |ELL_PRED - ELL_GT|, the angle in radians
 *     AREA                 3: pixels inside the scored ellipse, inside the ground-truth ellipse, inside both -- the membership rule of
 *                          calc_ell_iou (utils.py:185-196) through the device functions of egne_ellipse_fit
 *     MAP_PRED, MAP_GT     3 each: (pixels of the class, pixels of the ellipse, pixels of both) as egne_ellipse_iou_counts counts them
 *   and per row COND0, COND1 (0 or 1), BATCH (batch_no as passed), SAMPLE (index in the batch).
 *
 * egne_ellipse_box_corners: ell_px [n,5] float64 -> corners [n,8] int32.  egne_box_iou_counts: corners_a, corners_b [n,8] int32 ->
 *   out [n,3] float64 (IoU, n_and, n_or) on an H x W canvas (H * W < 2^31).  The device functions of the call above, for tests and
 *   for boxes from elsewhere. */
#define EGNE_ELLSCORE_ELL_PRED 0
#define EGNE_ELLSCORE_ELL_GT 5
#define EGNE_ELLSCORE_CORNERS_PRED 10
#define EGNE_ELLSCORE_CORNERS_GT 18
#define EGNE_ELLSCORE_BOX_IOU 26
#define EGNE_ELLSCORE_BOX_AND 27
#define EGNE_ELLSCORE_BOX_OR 28
#define EGNE_ELLSCORE_PARA 29
#define EGNE_ELLSCORE_AREA 34
#define EGNE_ELLSCORE_MAP_PRED 37
#define EGNE_ELLSCORE_MAP_GT 40
#define EGNE_ELLSCORE_REGION_FIELDS 43
#define EGNE_ELLSCORE_COND0 86
#define EGNE_ELLSCORE_COND1 87
#define EGNE_ELLSCORE_BATCH 88
#define EGNE_ELLSCORE_SAMPLE 89
#define EGNE_ELLSCORE_FIELDS 90
int egne_ellipse_pair_scores(const void* elNorm, const void* pred_px, const void* mask, const void* cond, int ncond, int B, int H, int W,
                             int cls_iris, int cls_pupil, const void* xs, const void* ys, int batch_no, void* ledger,
                             int64_t row_offset, int64_t capacity_rows, void* stream);
int egne_ellipse_box_corners(const void* ell_px, int n, void* corners, void* stream);
int egne_box_iou_counts(const void* corners_a, const void* corners_b, int n, int H, int W, void* out, void* stream);

/* ---- prediction overlay grid of train.py / test.py --disp 1 (csrc/dispgrid.hip, egne_amd.dispgrid.image_grid) -------------------
 * The reference's generateImageGrid (utils.py:206-399): the first n = min(count, B) frames of a batch, histogram-equalised, the
 * predicted classes painted in, the predicted ellipses outlined, tiled as torchvision.utils.make_grid(nrow, padding=2) tiles them.
 * The call queues on `stream`, synchronises nothing and can be captured in a graph; only integer atomics: the same bits on every run.
 *
 * img [B,H,W] float32; mask [B,H,W] int64 class map; el, el_gt [B,2,5] float32 normalised (iris, pupil) ellipses (el_gt may be null
 * unless draw_gt); cond [B,ncond] float32 or null (ncond >= 2); cos_sin float64 [2,720]: cos t then sin t of
 * t = linspace(0, 2 pi, 720, endpoint=False), made by the host; grid float32 [3,Hg,Wg]; bgr_u8 uint8 [Hg,Wg,3] or null; status
 * int32 [n]; workspace: egne_disp_grid_workspace_bytes(n) bytes.  H, W >= 6, H * W <= 2^30, n <= 65535.
 *
 * Per frame i < n (the reference's order of operations, utils.py:269-350), pinned by the reference:
 *   mn = min, mx = max of the frame in float32; u = trunc_to_u8(fl32(fl32(255 * fl32(x - mn)) / fl32(mx - mn))), IEEE float32 with a
 *   correctly rounded division; e = equalizeHist(u); e = e - min(e) in uint8; v = float32(double(e) / double(max(e))); all three
 *   channels start at v.  The frame is painted iff override != 0, or cond is given and cond[i,1] == 0: class 1 pixels become
 *   (0, 255, 0), class 2 pixels (255, 255, 0) -- 255 in an image whose grey lies in [0, 1], as the reference writes it --, then with
 *   draw_gt the two ground-truth outlines in (0, 102, 255) (the reference's commented-out lines), then the iris outline in
 *   (0, 0, 255), then the pupil outline in (255, 0, 0): later paints win.  Outline rows are clipped, not dropped:
 *   row = min(max(row, 6), H - 6), col = min(max(col, 6), W - 6) (ndarray.clip taken literally, also where H - 6 < 6).
 * This project's rules (the reference calls OpenCV, scikit-image and torchvision there):
 *   equalizeHist by OpenCV's published rule: 256-bin histogram of u, i0 its first occupied bin; if bin i0 holds every pixel the output
 *     is i0 everywhere; otherwise scale = 255.f / float(total - hist[i0]), lut[i0] = 0 and, for k > i0,
 *     lut[k] = round_half_even(float(sum_{i0 < j <= k} hist[j]) * scale) saturated to 0..255; e = lut[u].
 *   outline pixels: the pixel ellipse is the transform of egne_ellipse_init_from_pred (the same device function) of the widened
 *     float32 parameters; centre and axes are truncated toward zero, the angle is kept; 720 samples
 *     x = cx + a cos t cos th - b sin t sin th, y = cy + a cos t sin th + b sin t cos th in float64 (evaluate._draw_ellipse), each
 *     rounded to the nearest integer, ties to even, then clipped as above.  An ellipse whose pixel parameters are not finite or
 *     whose truncated axes are below 1 is not drawn; its status bit is set.
 *   layout: n == 1: the frame itself, [3,H,W].  Otherwise xm = min(nrow, n), ym = ceil(n / xm), grid [3, ym (H+2) + 2, xm (W+2) + 2],
 *     zero everywhere, frame k at row (k / xm) (H+2) + 2, column (k % xm) (W+2) + 2.
 *   bgr_u8 = rint(255 * min(max(g, 0), 1)) in float32, channels reversed: how an imshow of the grid looks.
 * status[i]: bit 0: the frame is constant (mx == mn; the reference divides by zero): grey 0.  Bit 1: the frame holds a non-finite
 *   pixel; its pixels are then unspecified (but the same on every run).  Bits 2, 3: the iris / pupil outline was skipped; bits 4, 5: the
 *   ground-truth iris / pupil outline was skipped (only outlines that were asked for set a bit). */
#define EGNE_DISPGRID_CONSTANT 1
#define EGNE_DISPGRID_NONFINITE 2
#define EGNE_DISPGRID_SKIP_IRIS 4
#define EGNE_DISPGRID_SKIP_PUPIL 8
#define EGNE_DISPGRID_SKIP_GT_IRIS 16
#define EGNE_DISPGRID_SKIP_GT_PUPIL 32
int64_t egne_disp_grid_workspace_bytes(int frames);
int egne_disp_grid(const void* img, const void* mask, const void* el, const void* el_gt, const void* cond, int ncond, int B, int H, int W,
                   int override_, int draw_gt, int count, int nrow, const void* cos_sin, void* grid, void* bgr_u8, void* status,
                   void* workspace, void* stream);

/* ---- label maps from TEyeD annotations (csrc/annot.hip, egne_amd.dataprep.labels_from_annotations) -----------------------------
 * What the reference's dataset_generation/Extract_TEyeD_*_histo.py scripts draw per kept frame: Masks_noSkin = zeros, cv2.circle
 * (eyeball) -> 1, cv2.ellipse (iris) -> 2, cv2.ellipse (pupil) -> 3; Masks = the same map, zeroed outside cv2.fillPoly of the 34
 * eyelid landmarks.  The ARGUMENTS handed to OpenCV are pinned by the reference (tests/golden/annot.npz) and applied on the host
 * by dataprep.pack_annotations; the PIXELS are this project's rules below, not OpenCV's (its boundary pixels are unpinned).  The call
 * queues three launches on `stream`, synchronises nothing and can be captured in a graph; its only atomic is an integer atomicOr
 * on the status word.
 *
 * records: B records of EGNE_ANNOT_RECORD_WORDS 32-bit words, 8-byte aligned (csrc/annot_core.h):
 *   word 0 flags (EGNE_ANNOT_HAS_*: an absent shape is skipped); word 1 n, the lid's vertices, 0 .. 64; words 2..4 ball bx, by, br;
 *   word 5 zero; words 6..9 iris ex, ey, A, B, words 10..13 its c, s as two float64 (cos and sin of the angle, made by the host: the
 *   device calls no trigonometry); words 14..21 the pupil likewise; words 22.. the lid's x, y pairs.  Every integer is at most 2^20
 *   in magnitude (pack_annotations refuses more), so that no int64 product overflows.
 * src_hw int32 [B,2] or null: the frame's own (rows, columns) inside the canvas, clamped to it; pixels at or beyond them stay 0 (the
 *   RawBatch layout).  noskin, skin (or null): int8 [B,R,C]; status int32 [B].  B <= 65535; R, C <= 2^20.
 *
 * Pixel (x, y), x the column:
 *   circle: dx * dx + dy * dy <= br * br in int64 (dx = x - bx, dy = y - by); br == 0 is the centre pixel.
 *   ellipse: X = dx * c + dy * s, Y = dy * c - dx * s (cv2.ellipse's convention: the first axis along (c, s), y down); the pixel
 *     belongs iff (X * B) * (X * B) + (Y * A) * (Y * A) <= (A * B) * (A * B) in float64, every operation rounded on its own in this
 *     order (no contraction).  Evaluated inside |dx|, |dy| <= max(A, B) + 1 only; with c * c + s * s = 1 to within rounding no pixel
 *     outside that square satisfies it.  A half-axis of zero (or below) paints nothing and sets a status bit -- OpenCV would draw a
 *     line segment there.
 *   polygon (closed, n vertices): even-odd with the boundary included.  Every edge with y0 != y1, oriented so that y0 < y1, toggles
 *     the parity of a pixel with y0 <= y < y1 and (x - x0) * (y1 - y0) - (x1 - x0) * (y - y0) < 0 in int64; a pixel with a zero cross
 *     product inside an edge's bounding box belongs regardless of parity (horizontal edges, zero-area polygons).  Self-intersections
 *     and repeated vertices need no special case.
 *   noskin = 0, then ball -> 1, iris -> 2, pupil -> 3; skin = noskin where the lid polygon holds, else 0; without the lid skin = noskin.
 * status[b]: EGNE_ANNOT_IRIS_ZERO_AXIS / EGNE_ANNOT_PUPIL_ZERO_AXIS: that ellipse is present with a half-axis <= 0;
 *   EGNE_ANNOT_EMPTY: no pixel of the frame's noskin map carries a class (readImage's "mask all 0", cond[1] of the batch). */
#define EGNE_ANNOT_RECORD_WORDS 150
#define EGNE_ANNOT_HAS_BALL 1
#define EGNE_ANNOT_HAS_IRIS 2
#define EGNE_ANNOT_HAS_PUPIL 4
#define EGNE_ANNOT_HAS_LID 8
#define EGNE_ANNOT_IRIS_ZERO_AXIS 1
#define EGNE_ANNOT_PUPIL_ZERO_AXIS 2
#define EGNE_ANNOT_EMPTY 4
int egne_labels_from_annotations(const void* records, const int* src_hw, int B, int R, int C, int8_t* noskin, int8_t* skin, int* status,
                                 void* stream);

const char* egne_last_error(void);
int egne_version(void);
int egne_sizeof(int which);   /* 0 egne_conv_desc, 1 egne_loss_desc, 2 egne_bdcn_tail_desc, 3 egne_dst, 4 egne_conv_query, 5 egne_conv_choice */

#ifdef __cplusplus
}
#endif
#endif
