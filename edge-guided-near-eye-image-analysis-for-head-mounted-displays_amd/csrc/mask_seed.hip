// Ellipse seeds from the class map (evaluate.py --ellipse_seed mask): per (frame, region) the largest 8-connected component of the
// region and the ellipse of its second moments.  Not in the reference (its ElliFit route goes through cv2.Canny); the float64 block of
// seed_final_k is restated line for line in tests/mask_seed_refs.py.
//
// Multi-launch union-find; the launch boundary is the only synchronisation between workgroups (no flag is waited for, no "last block"):
//   seed_zero_k   the per-row accumulators and the status word
//   seed_pack_k   region membership -> one 64-bit word per 64 columns (a wave's ballot); a NODE is the first pixel of a run of ones inside
//                 a word, label[node] = node, area[node] = 0.  Pixels that are not nodes never own a label: their node is found from the word.
//   seed_merge_k  unions between nodes: across a word boundary inside a row, and to the row above (N; NW / NE only where N is absent, and each
//                 only where the horizontal neighbour does not already carry it -- see the rules there).  atomicMin on the larger root; every
//                 label read in this pass is a relaxed agent-scope atomic load.
//   seed_count_k  every node finds its root, stores it (flatten) and adds its run length to area[root]
//   seed_pick_k   roots: components += 1, region pixels += area, best = max over (area, first pixel earliest) as one 64-bit key
//   seed_sums_k   nodes of the chosen root add the closed-form integer sums of their run (N, Sx, Sy, Sxx, Sxy, Syy): wave reduction, then
//                 64-bit integer atomics -- order-independent, so reproducible run to run
//   seed_final_k  one thread per row: float64 moments -> (cx, cy, a, b, theta) in the coordinate convention of the search
// Labels only ever decrease and label[x] <= x, so a find walks at most H*W links; find and union still carry the static bound
// 4*H*W + 64 steps: a row that reaches it sets bit 0 of `status`, is reported absent, and never keeps looping.
// The launches up to and including seed_pick_k live in mask_cc_common.h, which csrc/cleanup.hip includes too.
#include "common.h"

namespace {

#include "mask_cc_common.h"

__global__ __launch_bounds__(256) void seed_sums_k(int H, int W, int wpr, int bpr, char* ws) {
  int i, y, c;
  if (!locate(H, wpr, bpr, i, y, c)) return;
  const int l = threadIdx.x & 63;
  const RowWs r = row_ws(ws, i, H, W);
  const u64 cur = r.bits[(size_t)y * wpr + c];
  const u64 best = r.acc[0];
  if (cur == 0ull || best == 0ull) return;
  const int root = (int)(0xffffffffu - (unsigned)(best & 0xffffffffull));
  const int p = y * W + c * 64 + l;
  u64 s[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
  if (is_node(cur, l) && r.label[p] == root) {
    // the run x0 .. x1 of image row y: sums of 1, x, y, x^2, x y, y^2 in closed form
    const u64 len = (u64)run_len(cur, l), x0 = (u64)(c * 64 + l), x1 = x0 + len - 1ull, yy = (u64)y;
    auto sq = [](u64 m) -> u64 { return m * (m + 1ull) * (2ull * m + 1ull) / 6ull; };      // 0^2 + .. + m^2
    s[0] = len;
    s[1] = (x0 + x1) * len / 2ull;
    s[2] = yy * len;
    s[3] = sq(x1) - (x0 ? sq(x0 - 1ull) : 0ull);
    s[4] = yy * s[1];
    s[5] = yy * yy * len;
  }
  const bool any = wave_sum(s[0]) != 0ull;
  if (!any) return;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const u64 t = wave_sum(s[k]);
    if (l == 0) atomicAdd((unsigned long long*)(r.acc + 3 + k), t);
  }
}

__global__ void seed_final_k(const int* __restrict__ frame_of, const int* __restrict__ class_bits, const int* __restrict__ search_cls,
                             int nframes, int n, int H, int W, int min_area, char* ws, double* __restrict__ init,
                             int* __restrict__ out_frame_of, int* __restrict__ out_cls, long long* __restrict__ stats) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u64* acc = row_ws(ws, i, H, W).acc;
  const long long N = (long long)acc[3], Sx = (long long)acc[4], Sy = (long long)acc[5], Sxx = (long long)acc[6],
                  Sxy = (long long)acc[7], Syy = (long long)acc[8];
  const int fr = frame_of[i];
  const bool present = fr >= 0 && fr < nframes && class_bits[i] != 0 && acc[9] == 0ull && N > 0 && N >= (long long)min_area;
  long long* st = stats + (size_t)i * 8;
  st[6] = (long long)acc[1];
  st[7] = (long long)acc[2];
  out_cls[i] = search_cls[i];
  if (!present) {
    for (int k = 0; k < 6; ++k) st[k] = 0;
    for (int k = 0; k < 5; ++k) init[i * 5 + k] = -1.0;
    out_frame_of[i] = -1;
    return;
  }
  st[0] = N; st[1] = Sx; st[2] = Sy; st[3] = Sxx; st[4] = Sxy; st[5] = Syy;
  out_frame_of[i] = fr;
  const long long Ixx = N * Sxx - Sx * Sx, Iyy = N * Syy - Sy * Sy, Ixy = N * Sxy - Sx * Sy;
  const long long Jxx = 12 * Ixx + N * N, Jyy = 12 * Iyy + N * N, Jxy = 12 * Ixy;      // N*N: the 1/12 of a unit pixel
  const double nn = (double)N, d12 = 12.0 * nn * nn, sx = (double)W / (W - 1), sy = (double)H / (H - 1);
  const double mxx = ((double)Jxx / d12) * (sx * sx), myy = ((double)Jyy / d12) * (sy * sy), mxy = ((double)Jxy / d12) * (sx * sy);
  const double cx = ((double)Sx / nn) * sx, cy = ((double)Sy / nn) * sy;
  const double d = mxx - myy, rr = sqrt(d * d + 4.0 * mxy * mxy);
  init[i * 5 + 0] = cx;
  init[i * 5 + 1] = cy;
  init[i * 5 + 2] = 2.0 * sqrt((mxx + myy + rr) / 2.0);
  init[i * 5 + 3] = 2.0 * sqrt(fmax((mxx + myy - rr) / 2.0, 0.0));
  init[i * 5 + 4] = 0.5 * atan2(2.0 * mxy, d);
}

}  // namespace

extern "C" int64_t egne_mask_seed_workspace_bytes(int n, int H, int W) {
  if (n < 1 || !seed_shape_ok(H, W)) return -1;
  return (int64_t)((size_t)n * seed_row_bytes(H, W));
}

extern "C" int egne_ellipse_init_from_mask(const int64_t* mask, int nframes, const int32_t* frame_of, const int32_t* class_bits,
                                           const int32_t* search_cls, int n, int H, int W, int min_area, double* init,
                                           int32_t* out_frame_of, int32_t* out_cls, int64_t* stats, int32_t* status, void* ws,
                                           void* stream) {
  EGNE_REQUIRE(mask && frame_of && class_bits && search_cls && init && out_frame_of && out_cls && stats && status && ws,
               "ellipse_init_from_mask: null pointer");
  EGNE_REQUIRE(n > 0 && nframes > 0, "ellipse_init_from_mask: bad counts");
  EGNE_REQUIRE(seed_shape_ok(H, W), "ellipse_init_from_mask: %dx%d masks (2..1024 rows and columns, at most 2^20 pixels)", H, W);
  EGNE_REQUIRE(((uintptr_t)ws & 7) == 0, "ellipse_init_from_mask: workspace not aligned to 8 bytes");
  const int wpr = (W + 63) / 64, bpr = (H * wpr + 3) / 4;
  EGNE_REQUIRE((long long)n * bpr < (1ll << 31), "ellipse_init_from_mask: %d rows of %dx%d exceed one grid", n, H, W);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(n * bpr)), block(256);
  char* w = (char*)ws;
  hipLaunchKernelGGL(seed_zero_k, dim3((unsigned)((n * 16 + 255) / 256)), block, 0, st, w, n, H, W, status);
  hipLaunchKernelGGL(seed_pack_k, grid, block, 0, st, (const long long*)mask, nframes, frame_of, class_bits, H, W, wpr, bpr, w);
  hipLaunchKernelGGL(seed_merge_k, grid, block, 0, st, H, W, wpr, bpr, w, status);
  hipLaunchKernelGGL(seed_count_k, grid, block, 0, st, H, W, wpr, bpr, w, status);
  hipLaunchKernelGGL(seed_pick_k, grid, block, 0, st, H, W, wpr, bpr, w);
  hipLaunchKernelGGL(seed_sums_k, grid, block, 0, st, H, W, wpr, bpr, w);
  hipLaunchKernelGGL(seed_final_k, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, frame_of, class_bits, search_cls, nframes, n, H, W,
                     min_area, w, init, out_frame_of, out_cls, (long long*)stats);
  return egne::check_launch("egne_ellipse_init_from_mask");
}
