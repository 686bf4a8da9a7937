// Self-consistency term of the loss head (loss.py:187-219 get_selfConsistency; models/RITnet_v2.py:339-341, RITnet_v1.py:286-287),
// forward and backward, without host syncs.
//
// The pupil ellipse of elPred is rasterised into the soft mask t = sigmoid(64 (1 - q)) and the background of the iris ellipse into
// t = sigmoid(64 (q - 1)), q = (X/a)^2 + (Y/b)^2 in the ellipse's frame; the term is the mean over pixels of kl(t, log_softmax(op)[c])
// (c = 2 for the pupil mask, 0 for the background), averaged over the samples whose mask is present.
//
// Forward: one pass over the logits writes per-(sample, block) partial sums -- the two KL sums and, per ellipse, the five moments of
// u = d kl / d q that the gradient w.r.t. its parameters needs -- then one block combines them per sample and over the batch.
// Backward: one pass adds the gradient w.r.t. the logits into an NCHW fp32 tensor, and ten threads per sample add the parameter
// gradients.  Every element has one writer and every sum a fixed order: no atomics, results are deterministic.
//
// Where sigmoid underflows to 0 the reference's autograd forms 0 * log 0 = NaN (kl_div's target gradient); the derivative there is the
// limit, 0, and that is what these kernels return: a pixel whose t, or t (1 - t), is 0 contributes nothing.
#include "common.h"
#include "kernel_util.h"

namespace {

constexpr int SC_PIX = 2048;   // pixels per block
constexpr int SC_NPART = 12;   // floats per (sample, block) record
constexpr int SC_HEAD = 4;     // ws[0..3] = term, n_ok, weight * term, 0
// ws layout: head | [B][10] d (sum_pix kl_pup + kl_bg) / d elPred[b][j] | [B][nblk][SC_NPART] records
// record: [0] sum kl_pup, [1] sum kl_bg, [2..6] iris ellipse: sum u xa, u yb, u xa^2, u yb^2, u xa yb (xa = X/a, yb = Y/b), [7..11] pupil

inline int sc_nblk(int H, int W) { return (H * W + SC_PIX - 1) / SC_PIX; }

struct Ell { float cx, cy, a, b, c, s; };

__device__ __forceinline__ Ell load_ell(const float* e) {
  Ell r = {e[0], e[1], e[2], e[3], cosf(e[4]), sinf(e[4])};
  return r;
}

// q of get_mask (loss.py:211-216) with its two quotients
__device__ __forceinline__ float ell_q(const Ell& e, float gx, float gy, float& xa, float& yb) {
  const float dx = gx - e.cx, dy = gy - e.cy;
  const float X = dx * e.c + dy * e.s, Y = -dx * e.s + dy * e.c;
  xa = X / e.a; yb = Y / e.b;
  return xa * xa + yb * yb;
}

// t = sigmoid(z), log t = -softplus(-z), tt = t (1 - t): all from e = exp(-|z|), none of them through a difference of near-equal values
__device__ __forceinline__ void soft_mask(float z, float& t, float& logt, float& tt) {
  const float e = expf(-fabsf(z));
  const float inv = 1.f / (1.f + e);
  t = z >= 0.f ? inv : e * inv;
  logt = fminf(z, 0.f) - log1pf(e);
  tt = e * inv * inv;
}

struct Pix { float lp0, lp2, p0, p1, p2; };

template <typename T>
__device__ __forceinline__ Pix load_pix(const egne_loss_desc& d, long long pix) {
  const T* lp = (const T*)d.logits + pix * d.pix_stride + d.ch_off;
  const float l0 = ld1(lp), l1 = ld1(lp + 1), l2 = ld1(lp + 2);
  const float mx = fmaxf(l0, fmaxf(l1, l2));
  const float e0 = expf(l0 - mx), e1 = expf(l1 - mx), e2 = expf(l2 - mx);
  const float se = e0 + e1 + e2, inv = 1.f / se, lse = mx + logf(se);
  Pix r = {l0 - lse, l2 - lse, e0 * inv, e1 * inv, e2 * inv};
  return r;
}

template <typename T>
__global__ __launch_bounds__(256) void selfcorr_partial_k(const egne_loss_desc d, float* __restrict__ ws, int nblk) {
  const int b = blockIdx.y, blk = blockIdx.x;
  const int HW = d.H * d.W;
  float* out = ws + SC_HEAD + (long long)d.B * 10 + ((long long)b * nblk + blk) * SC_NPART;
  const float ok = 1.f - d.cond[b * 4 + 1];
  if (ok == 0.f) {   // the sample does not enter the term: its ellipses are not even read
    if (threadIdx.x < SC_NPART) out[threadIdx.x] = 0.f;
    return;
  }
  const Ell iri = load_ell(d.elPred + b * 10), pup = load_ell(d.elPred + b * 10 + 5);
  const int p0 = blk * SC_PIX, p1 = min(p0 + SC_PIX, HW);
  const long long base = (long long)b * HW;
  float acc[SC_NPART];
#pragma unroll
  for (int i = 0; i < SC_NPART; ++i) acc[i] = 0.f;
  for (int p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
    const Pix px = load_pix<T>(d, base + p);
    const int y = p / d.W, x = p - y * d.W;
    const float gx = d.grid_x[x], gy = d.grid_y[y];
    float xa, yb, t, logt, tt;
    // background of the iris ellipse against class 0: z = 64 (q - 1), d z / d q = 64
    float q = ell_q(iri, gx, gy, xa, yb);
    soft_mask(64.f * (q - 1.f), t, logt, tt);
    if (t > 0.f) acc[1] += t * (logt - px.lp0);
    if (tt > 0.f) {
      const float u = 64.f * tt * (logt - px.lp0 + 1.f);
      acc[2] += u * xa; acc[3] += u * yb; acc[4] += u * xa * xa; acc[5] += u * yb * yb; acc[6] += u * xa * yb;
    }
    // pupil ellipse against class 2: z = 64 (1 - q), d z / d q = -64
    q = ell_q(pup, gx, gy, xa, yb);
    soft_mask(64.f * (1.f - q), t, logt, tt);
    if (t > 0.f) acc[0] += t * (logt - px.lp2);
    if (tt > 0.f) {
      const float u = -64.f * tt * (logt - px.lp2 + 1.f);
      acc[7] += u * xa; acc[8] += u * yb; acc[9] += u * xa * xa; acc[10] += u * yb * yb; acc[11] += u * xa * yb;
    }
  }
  // at most SC_PIX / 256 = 8 terms per thread in fp32; the block's 256 sums are combined in float64
  double s[SC_NPART];
#pragma unroll
  for (int i = 0; i < SC_NPART; ++i) s[i] = (double)acc[i];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
    for (int i = 0; i < SC_NPART; ++i) s[i] += __shfl_xor(s[i], o);
  }
  __shared__ double sh[4][SC_NPART];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < SC_NPART; ++i) sh[wave][i] = s[i];
  }
  __syncthreads();
  if (threadIdx.x < SC_NPART) {
    const int i = threadIdx.x;
    out[i] = (float)((sh[0][i] + sh[1][i]) + (sh[2][i] + sh[3][i]));
  }
}

// d q / d (cx, cy, a, b, theta) summed with u: from the five moments of one ellipse
__device__ __forceinline__ void ell_param_grad(const float* e, const double* m, float* g) {
  const double a = e[2], b = e[3], c = cos((double)e[4]), s = sin((double)e[4]);
  g[0] = (float)(2.0 * (-c * m[0] / a + s * m[1] / b));
  g[1] = (float)(2.0 * (-s * m[0] / a - c * m[1] / b));
  g[2] = (float)(-2.0 * m[2] / a);
  g[3] = (float)(-2.0 * m[3] / b);
  g[4] = (float)(2.0 * m[4] * (b / a - a / b));
}

// one block; thread i handles samples i, i + blockDim, ...; then a block reduction over the batch (the shape of loss_final_k)
__global__ __launch_bounds__(256) void selfcorr_final_k(const egne_loss_desc d, float weight, float* __restrict__ ws,
                                                        float* __restrict__ sc_terms, int nblk) {
  const double fHW = (double)d.H * (double)d.W;
  double bt[2] = {0.0, 0.0};   // sum ok_b * (mean kl_pup + mean kl_bg), n_ok
  for (int b = threadIdx.x; b < d.B; b += blockDim.x) {
    const float ok = 1.f - d.cond[b * 4 + 1];
    float* pg = ws + SC_HEAD + (long long)b * 10;
    if (ok == 0.f) {
      for (int j = 0; j < 10; ++j) pg[j] = 0.f;
      continue;
    }
    double a[SC_NPART];
    for (int i = 0; i < SC_NPART; ++i) a[i] = 0.0;
    const float* r = ws + SC_HEAD + (long long)d.B * 10 + (long long)b * nblk * SC_NPART;
    for (int k = 0; k < nblk; ++k)
      for (int i = 0; i < SC_NPART; ++i) a[i] += (double)r[k * SC_NPART + i];
    bt[0] += (double)ok * (a[0] / fHW + a[1] / fHW);
    bt[1] += (double)ok;
    ell_param_grad(d.elPred + b * 10, a + 2, pg);
    ell_param_grad(d.elPred + b * 10 + 5, a + 7, pg + 5);
  }
  __shared__ double sh[256][2];
  sh[threadIdx.x][0] = bt[0]; sh[threadIdx.x][1] = bt[1];
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (threadIdx.x < s) { sh[threadIdx.x][0] += sh[threadIdx.x + s][0]; sh[threadIdx.x][1] += sh[threadIdx.x + s][1]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float n_ok = (float)sh[0][1];
    const float term = n_ok > 0.f ? (float)(sh[0][0] / sh[0][1]) : 0.f;
    const float add = weight * term;
    ws[0] = term; ws[1] = n_ok; ws[2] = add; ws[3] = 0.f;
    sc_terms[0] = term; sc_terms[1] = n_ok; sc_terms[2] = add; sc_terms[3] = 0.f;
    d.out_terms[0] += add;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void selfcorr_bwd_k(const egne_loss_desc d, float weight, const float* __restrict__ ws,
                                                      const float* __restrict__ gscale_p, float* __restrict__ g_op,
                                                      float* __restrict__ g_pred_c, float* __restrict__ g_elOut_up) {
  const int b = blockIdx.y, blk = blockIdx.x;
  const int HW = d.H * d.W;
  const float n_ok = ws[1];
  const float ok = 1.f - d.cond[b * 4 + 1];
  if (!(n_ok > 0.f) || ok == 0.f) return;   // nothing is added: the destinations keep their bits
  const float w = weight * gscale_p[0] * ok / ((float)HW * n_ok);
  if (blk == 0 && threadIdx.x < 10) {
    const int j = threadIdx.x;
    const float g = w * ws[SC_HEAD + (long long)b * 10 + j];
    // elPred = (iris centre, elOut[2:5], pupil centre, elOut[7:10]): the centres are the soft-argmax rows of pred_c
    if (j < 2) g_pred_c[b * 4 + j] += g;
    else if (j == 5 || j == 6) g_pred_c[b * 4 + 2 + (j - 5)] += g;
    else g_elOut_up[b * 10 + j] += g;
  }
  const Ell iri = load_ell(d.elPred + b * 10), pup = load_ell(d.elPred + b * 10 + 5);
  const int p0 = blk * SC_PIX, p1 = min(p0 + SC_PIX, HW);
  const long long base = (long long)b * HW;
  for (int p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
    const Pix px = load_pix<T>(d, base + p);
    const int y = p / d.W, x = p - y * d.W;
    const float gx = d.grid_x[x], gy = d.grid_y[y];
    float xa, yb, tb, tp, logt, tt;
    soft_mask(64.f * (ell_q(iri, gx, gy, xa, yb) - 1.f), tb, logt, tt);
    soft_mask(64.f * (1.f - ell_q(pup, gx, gy, xa, yb)), tp, logt, tt);
    // d kl(t, lp_c) / d l_k = t (p_k - [k == c])
    float* o = g_op + (long long)b * 3 * HW + p;
    o[0] += w * (tp * px.p0 + tb * (px.p0 - 1.f));
    o[HW] += w * ((tp + tb) * px.p1);
    o[2 * (long long)HW] += w * (tp * (px.p2 - 1.f) + tb * px.p2);
  }
}

int sc_check(const egne_loss_desc* dp, const char* what) {
  EGNE_REQUIRE(dp, "%s: null descriptor", what);
  const egne_loss_desc& d = *dp;
  EGNE_REQUIRE(d.B > 0 && d.H > 1 && d.W > 1, "%s: bad shape", what);
  EGNE_REQUIRE(d.logits && d.ch_off >= 0 && d.ch_off + 3 <= d.pix_stride, "%s: bad logits slice", what);
  EGNE_REQUIRE(d.dtype == 0 || d.dtype == 1, "%s: dtype %d", what, d.dtype);
  EGNE_REQUIRE(d.cond && d.elPred && d.grid_x && d.grid_y && d.out_terms, "%s: cond / elPred / grid / out_terms missing", what);
  return 0;
}

}  // namespace

extern "C" int64_t egne_selfcorr_workspace_floats(int B, int H, int W) {
  return SC_HEAD + (int64_t)B * 10 + (int64_t)B * sc_nblk(H, W) * SC_NPART;
}

extern "C" int egne_selfcorr_fwd(const egne_loss_desc* dp, float weight, float* ws, float* sc_terms, void* stream) {
  if (int rc = sc_check(dp, "selfcorr_fwd")) return rc;
  EGNE_REQUIRE(ws && sc_terms, "selfcorr_fwd: null workspace / output");
  const egne_loss_desc& d = *dp;
  const int nblk = sc_nblk(d.H, d.W);
  hipStream_t st = (hipStream_t)stream;
  if (d.dtype == 1) hipLaunchKernelGGL(selfcorr_partial_k<egne_bf16>, dim3(nblk, d.B), dim3(256), 0, st, d, ws, nblk);
  else hipLaunchKernelGGL(selfcorr_partial_k<float>, dim3(nblk, d.B), dim3(256), 0, st, d, ws, nblk);
  hipLaunchKernelGGL(selfcorr_final_k, dim3(1), dim3(256), 0, st, d, weight, ws, sc_terms, nblk);
  return egne::check_launch("egne_selfcorr_fwd");
}

extern "C" int egne_selfcorr_bwd(const egne_loss_desc* dp, float weight, const float* ws, const float* gscale, float* g_op_nchw,
                                 float* g_pred_c, float* g_elOut_up, void* stream) {
  if (int rc = sc_check(dp, "selfcorr_bwd")) return rc;
  EGNE_REQUIRE(ws && gscale && g_op_nchw && g_pred_c && g_elOut_up, "selfcorr_bwd: null pointer");
  const egne_loss_desc& d = *dp;
  const int nblk = sc_nblk(d.H, d.W);
  hipStream_t st = (hipStream_t)stream;
  if (d.dtype == 1) hipLaunchKernelGGL(selfcorr_bwd_k<egne_bf16>, dim3(nblk, d.B), dim3(256), 0, st, d, weight, ws, gscale, g_op_nchw, g_pred_c, g_elOut_up);
  else hipLaunchKernelGGL(selfcorr_bwd_k<float>, dim3(nblk, d.B), dim3(256), 0, st, d, weight, ws, gscale, g_op_nchw, g_pred_c, g_elOut_up);
  return egne::check_launch("egne_selfcorr_bwd");
}
