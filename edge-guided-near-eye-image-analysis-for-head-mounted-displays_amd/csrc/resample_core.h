// The 8-tap Lanczos resampling of evaluate.resize_lanczos4 for one output row, shared by the front end of evaluate.py
// (csrc/evalio.hip, egne_eval_prep) and the training loader (csrc/loader.hip, egne_loader_stage).  Both files are compiled without
// FMA contraction (Makefile): every product and sum below is rounded on its own, as NumPy rounds them.
#pragma once
#include <cstdint>

namespace egne {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One workgroup of 256 threads, output row y.  px(row, x) is the uint8 source pixel (rows 0..Hs-1, columns 0..We-1).
// Row pass: the 8 source rows ridx[y][8] weighted by rw[y][8] in float64 into rowbuf[We] (LDS; sequential sum, as NumPy reduces a
// middle axis), or a plain copy of row y when ridx is NULL.  Column pass out of rowbuf: cidx[x][8] / cw[x][8] (pairwise sum, as
// NumPy reduces a contiguous axis of 8), or a copy when cidx is NULL.  rint, clip to [0, 255], out[Wr].  Indices are clamped again
// here, so a bad table cannot read outside the source.
template <class Px>
__device__ __forceinline__ void lanczos4_row(Px px, int Hs, int We, int Wr, int y, const int* __restrict__ ridx,
                                             const double* __restrict__ rw, const int* __restrict__ cidx,
                                             const double* __restrict__ cw, double* rowbuf, uint8_t* __restrict__ out) {
  if (ridx) {
    int ri[8];
    double w[8];
    for (int k = 0; k < 8; ++k) { ri[k] = clampi(ridx[y * 8 + k], 0, Hs - 1); w[k] = rw[y * 8 + k]; }
    for (int x = threadIdx.x; x < We; x += 256) {
      double acc = (double)px(ri[0], x) * w[0];
      for (int k = 1; k < 8; ++k) acc = acc + (double)px(ri[k], x) * w[k];
      rowbuf[x] = acc;
    }
  } else {
    for (int x = threadIdx.x; x < We; x += 256) rowbuf[x] = (double)px(y, x);
  }
  __syncthreads();
  for (int x = threadIdx.x; x < Wr; x += 256) {
    double v;
    if (cidx) {
      double p[8];
      for (int k = 0; k < 8; ++k) p[k] = rowbuf[clampi(cidx[x * 8 + k], 0, We - 1)] * cw[x * 8 + k];
      v = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
    } else {
      v = rowbuf[x];
    }
    v = rint(v);
    v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
    out[x] = (uint8_t)(int)v;
  }
}

}  // namespace egne
