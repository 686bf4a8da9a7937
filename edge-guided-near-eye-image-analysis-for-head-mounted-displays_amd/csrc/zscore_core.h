// The float64 statistics of the per-image z-score (CurriculumLib.py:139), shared by egne_zscore (csrc/dataprep.hip) and
// egne_loader_finish (csrc/loader.hip) so that both produce the same bits: the order of the additions is part of the result.
#pragma once

namespace egne {

// One workgroup of 256 threads over the n pixels x(0..n-1) of an image (x returns float): thread t accumulates pixels t, t + 256, ...
// in double, a binary tree over sh[256] adds the partial sums.  mean = sum / n, then sd = sqrt(sum((x - mean)^2) / n) the same way
// (population standard deviation, the squares fused into the sum: contraction is pinned here, whatever the file is compiled with).
template <class X>
__device__ __forceinline__ void zscore_stats(X x, int n, double* sh, double& mean, double& sd) {
#pragma clang fp contract(on)
  double s = 0;
  for (int i = threadIdx.x; i < n; i += 256) s += x(i);
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k >= 1; k >>= 1) { if ((int)threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k]; __syncthreads(); }
  mean = sh[0] / n;
  __syncthreads();
  double q = 0;
  for (int i = threadIdx.x; i < n; i += 256) { const double d = x(i) - mean; q += d * d; }
  sh[threadIdx.x] = q;
  __syncthreads();
  for (int k = 128; k >= 1; k >>= 1) { if ((int)threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k]; __syncthreads(); }
  sd = sqrt(sh[0] / n);
}

}  // namespace egne
