// Class-map clean-up (evaluate.py --clean_mask 1; utils.clean_class_maps): per-class 3x3 opening, per row the largest
// 8-connected component with its holes filled, composed into a cleaned class map.  The contract is in include/egne_hip.h; the NumPy
// restatement is tests/cleanup_refs.py.  Integer-exact: every output is a function of the input alone, whatever the order of the atomics.
//
// A fixed sequence of launches; the launch boundary is the only synchronisation between workgroups (no flag is waited for, no "last
// block").  Rows 0 .. n-1 of the workspace hold the region R of each row, rows n .. 2n-1 the complement of its K, both in the layout
// of mask_cc_common.h; behind them one bitmap [H][wpr] per row, first K, then K with its holes (P):
//   seed_zero_k      (shared) the accumulators of all 2n workspace rows and the status word
//   seed_pack_k      (shared; open3 = 0) R -> row words and nodes
//   clean_open_k     (open3 = 1, instead) the same from the opened class sets: per class of the row's class_bits the ballots of the
//                    diamond of 11 words around this one, cleanup_core.h's open3_word, ORed
//   seed_merge_k, seed_count_k, seed_pick_k   (shared) components of R, areas, the largest one
//   clean_kbits_k    K's bitmap (the runs whose root is the chosen one; all of R without flag 1; nothing below min_area) and, for flag 2,
//                    the complement of K packed into words and nodes
//   clean_merge4_k   complement, 4-connected: a node joins its run's continuation across the word boundary and the runs of the row
//                    above that share a column with its run.  No diagonals
//   clean_border_k   every node finds its root, stores it, and marks the root when its run touches the frame border
//   clean_fill_k     P = K | the complement runs whose root is unmarked; their pixels are counted
//   clean_final_k    one thread per row: the four statistics
//   clean_paint_k    one thread per pixel of `out`, written exactly once: paint_cls of the last row of its frame whose P covers it,
//                    else fill_cls
// find / union carry the static bound 4*H*W + 64 of the seed stage; a row that reaches it sets bit 0 of `status` and paints nothing.
#include "common.h"
#include "cleanup_core.h"

namespace {

#include "mask_cc_common.h"

namespace cl = egne_cleanup;

__device__ __forceinline__ u64* row_bitmap(char* ws, int n, int i, int H, int W) {
  const size_t wpr = (size_t)(W + 63) / 64;
  return (u64*)(ws + (size_t)2 * n * seed_row_bytes(H, W) + (size_t)i * H * wpr * 8);
}

__global__ __launch_bounds__(256) void clean_open_k(const long long* __restrict__ mask, int nframes, const int* __restrict__ frame_of,
                                                    const int* __restrict__ class_bits, int H, int W, int wpr, int bpr, char* ws) {
  int i, y, c;
  if (!locate(H, wpr, bpr, i, y, c)) return;
  const int l = threadIdx.x & 63, x = c * 64 + l;
  const RowWs r = row_ws(ws, i, H, W);
  const int fr = frame_of[i];
  const unsigned cb = (unsigned)class_bits[i];
  u64 w = 0ull;
  if (fr >= 0 && fr < nframes && cb != 0u) {                // (uniform over the wave: the ballots below see all 64 lanes)
    // this lane's pixel of the 15 words around: its class id, -1 for an id outside 0..31, -2 outside the frame
    int kk[5][3];
#pragma unroll
    for (int dy = 0; dy < 5; ++dy)
#pragma unroll
      for (int dc = 0; dc < 3; ++dc) {
        const int yy = y + dy - 2, xx = x + (dc - 1) * 64;
        int v = -2;
        if (!((dy == 0 || dy == 4) && dc != 1) && yy >= 0 && yy < H && xx >= 0 && xx < W) {
          const long long k = mask[((size_t)fr * H + yy) * W + xx];
          v = (k >= 0 && k < 32) ? (int)k : -1;
        }
        kk[dy][dc] = v;
      }
    unsigned rest = cb;
    for (int t = 0; t < 32 && rest; ++t) {
      const int cls = __ffs((int)rest) - 1;
      rest &= rest - 1u;
      cl::word_t s[5][3];
#pragma unroll
      for (int dy = 0; dy < 5; ++dy)
#pragma unroll
        for (int dc = 0; dc < 3; ++dc) s[dy][dc] = __ballot(kk[dy][dc] == -2 || kk[dy][dc] == cls);
      w |= cl::open3_word(s, y, c, H, W);
    }
  }
  if (l == 0) r.bits[(size_t)y * wpr + c] = w;
  if (is_node(w, l)) {
    const int p = y * W + x;
    r.label[p] = p;
    r.area[p] = 0u;
  }
}

// pixels of K before filling, from the accumulators of R's row
__device__ __forceinline__ long long k_pixels(const u64* acc, int fl) { return (fl & 1) ? (long long)(acc[0] >> 32) : (long long)acc[2]; }

__global__ __launch_bounds__(256) void clean_kbits_k(const int* __restrict__ flags, int n, int min_area, int H, int W, int wpr, int bpr,
                                                     char* ws) {
  int i, y, c;
  if (!locate(H, wpr, bpr, i, y, c)) return;
  const int l = threadIdx.x & 63, x = c * 64 + l;
  const RowWs r = row_ws(ws, i, H, W), q = row_ws(ws, n + i, H, W);
  const size_t at = (size_t)y * wpr + c;
  const u64 cur = r.bits[at], best = r.acc[0];
  const int fl = flags[i];
  const long long kpx = k_pixels(r.acc, fl);
  const bool ok = r.acc[9] == 0ull && kpx > 0 && kpx >= (long long)min_area;
  bool in = ok && ((cur >> l) & 1ull);
  if (in && (fl & 1)) {
    const int root = (int)(0xffffffffu - (unsigned)(best & 0xffffffffull));
    in = r.label[y * W + c * 64 + run_start(cur, l)] == root;
  }
  const u64 kw = __ballot(in);
  const u64 cw = (ok && (fl & 2)) ? ~kw & cl::row_mask(W, c) : 0ull;
  if (l == 0) {
    row_bitmap(ws, n, i, H, W)[at] = kw;
    q.bits[at] = cw;
  }
  if (is_node(cw, l)) {
    const int p = y * W + x;
    q.label[p] = p;
    q.area[p] = 0u;
  }
}

__global__ __launch_bounds__(256) void clean_merge4_k(int H, int W, int wpr, int bpr, char* wsc, int* status) {
  int i, y, c;
  if (!locate(H, wpr, bpr, i, y, c)) return;
  const int l = threadIdx.x & 63;
  const RowWs q = row_ws(wsc, i, H, W);
  const u64* brow = q.bits + (size_t)y * wpr;
  const u64 cur = brow[c];
  if (!is_node(cur, l)) return;
  const int bound = 4 * H * W + 64;
  const int me = y * W + c * 64 + l;
  bool ok = true;
  // a run that goes on across the word boundary: two nodes, one run
  if (l == 0 && c > 0 && (brow[c - 1] >> 63)) ok &= unite(q.label, me, y * W + (c - 1) * 64 + run_start(brow[c - 1], 63), bound);
  if (y > 0) {
    const int up = (y - 1) * W + c * 64;
    cl::for_each_overlap4(cl::run_bits(cur, l), brow[c - wpr], [&](int first) { ok &= unite(q.label, me, up + first, bound); });
  }
  if (!ok) {
    atomicOr(status, 1);
    atomicOr((unsigned long long*)(q.acc + 9), 1ull);
  }
}

__global__ __launch_bounds__(256) void clean_border_k(int H, int W, int wpr, int bpr, char* wsc, int* status) {
  int i, y, c;
  if (!locate(H, wpr, bpr, i, y, c)) return;
  const int l = threadIdx.x & 63;
  const RowWs q = row_ws(wsc, i, H, W);
  const u64 cur = q.bits[(size_t)y * wpr + c];
  if (!is_node(cur, l)) return;
  const int p = y * W + c * 64 + l;
  int budget = 4 * H * W + 64;
  const int root = find(q.label, p, budget);
  if (root < 0) {
    atomicOr(status, 1);
    atomicOr((unsigned long long*)(q.acc + 9), 1ull);
    return;
  }
  __hip_atomic_store(q.label + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int x0 = c * 64 + l, x1 = x0 + run_len(cur, l) - 1;
  if (y == 0 || y == H - 1 || x0 == 0 || x1 == W - 1) atomicOr(q.area + root, 1u);
}

__global__ __launch_bounds__(256) void clean_fill_k(int n, int H, int W, int wpr, int bpr, char* ws) {
  int i, y, c;
  if (!locate(H, wpr, bpr, i, y, c)) return;
  const int l = threadIdx.x & 63;
  const RowWs q = row_ws(ws, n + i, H, W);
  const size_t at = (size_t)y * wpr + c;
  const u64 cur = q.bits[at];
  if (cur == 0ull) return;                                  // (whole waves leave)
  bool hole = false;
  if ((cur >> l) & 1ull) hole = q.area[q.label[y * W + c * 64 + run_start(cur, l)]] == 0u;
  const u64 hw = __ballot(hole);
  if (l == 0 && hw) {
    row_bitmap(ws, n, i, H, W)[at] |= hw;
    atomicAdd((unsigned long long*)(q.acc + 10), (unsigned long long)__popcll(hw));
  }
}

__global__ void clean_final_k(const int* __restrict__ flags, int n, int min_area, int H, int W, char* ws, long long* __restrict__ stats) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u64 *ra = row_ws(ws, i, H, W).acc, *qa = row_ws(ws, n + i, H, W).acc;
  const long long kpx = k_pixels(ra, flags[i]);
  const bool ok = ra[9] == 0ull && qa[9] == 0ull && kpx > 0 && kpx >= (long long)min_area;
  long long* st = stats + (size_t)i * 4;
  st[0] = (long long)ra[2];
  st[1] = (long long)ra[1];
  st[2] = kpx;
  st[3] = ok ? (long long)qa[10] : 0;
}

__global__ __launch_bounds__(256) void clean_paint_k(long long* __restrict__ out, int nframes, const int* __restrict__ frame_of,
                                                     const int* __restrict__ paint_cls, int n, long long fill_cls, int H, int W, int wpr,
                                                     int bpr, char* ws) {
  const int f = blockIdx.x / bpr;
  const int word = (blockIdx.x % bpr) * 4 + (threadIdx.x >> 6);
  if (word >= H * wpr) return;                              // (whole waves leave)
  const int y = word / wpr, c = word % wpr, l = threadIdx.x & 63, x = c * 64 + l;
  const size_t at = (size_t)y * wpr + c;
  long long v = fill_cls;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int ii = i0 + l;
    u64 m = __ballot(ii < n && frame_of[ii] == f);
    for (int t = 0; t < 64 && m; ++t) {                     // the rows of this frame, in row order: a later one paints over an earlier one
      const int i = i0 + __ffsll((long long)m) - 1;
      m &= m - 1ull;
      if (row_ws(ws, i, H, W).acc[9] | row_ws(ws, n + i, H, W).acc[9]) continue;
      if ((row_bitmap(ws, n, i, H, W)[at] >> l) & 1ull) v = (long long)paint_cls[i];
    }
  }
  if (x < W) out[((size_t)f * H + y) * W + x] = v;
}

}  // namespace

extern "C" int64_t egne_class_map_cleanup_workspace_bytes(int n, int H, int W) {
  if (n < 1 || !seed_shape_ok(H, W)) return -1;
  const size_t wpr = (size_t)(W + 63) / 64;
  return (int64_t)((size_t)n * (2 * seed_row_bytes(H, W) + (size_t)H * wpr * 8));
}

extern "C" int egne_class_map_cleanup(const int64_t* mask, int nframes, const int32_t* frame_of, const int32_t* class_bits,
                                      const int32_t* paint_cls, const int32_t* flags, int n, int H, int W, int open3, int min_area,
                                      int64_t fill_cls, int64_t* out, int64_t* stats, int32_t* status, void* ws, void* stream) {
  EGNE_REQUIRE(mask && frame_of && class_bits && paint_cls && flags && out && stats && status && ws, "class_map_cleanup: null pointer");
  EGNE_REQUIRE(n > 0 && nframes > 0, "class_map_cleanup: bad counts");
  EGNE_REQUIRE((open3 == 0 || open3 == 1) && min_area >= 1, "class_map_cleanup: open3 %d (0 or 1), min_area %d (at least 1)", open3, min_area);
  EGNE_REQUIRE(seed_shape_ok(H, W), "class_map_cleanup: %dx%d masks (2..1024 rows and columns, at most 2^20 pixels)", H, W);
  EGNE_REQUIRE(((uintptr_t)ws & 7) == 0, "class_map_cleanup: workspace not aligned to 8 bytes");
  const uintptr_t bytes = (uintptr_t)nframes * H * W * 8, m0 = (uintptr_t)mask, o0 = (uintptr_t)out;
  EGNE_REQUIRE(m0 + bytes <= o0 || o0 + bytes <= m0, "class_map_cleanup: out overlaps mask");
  const int wpr = (W + 63) / 64, bpr = (H * wpr + 3) / 4;
  EGNE_REQUIRE((long long)n * bpr < (1ll << 31) && (long long)nframes * bpr < (1ll << 31) && (long long)n * 32 < (1ll << 31),
               "class_map_cleanup: %d rows / %d frames of %dx%d exceed one grid", n, nframes, H, W);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(n * bpr)), block(256);
  char* w = (char*)ws;
  char* wc = w + (size_t)n * seed_row_bytes(H, W);          // the complements' workspace rows
  hipLaunchKernelGGL(seed_zero_k, dim3((unsigned)((2 * n * 16 + 255) / 256)), block, 0, st, w, 2 * n, H, W, status);
  if (open3)
    hipLaunchKernelGGL(clean_open_k, grid, block, 0, st, (const long long*)mask, nframes, frame_of, class_bits, H, W, wpr, bpr, w);
  else
    hipLaunchKernelGGL(seed_pack_k, grid, block, 0, st, (const long long*)mask, nframes, frame_of, class_bits, H, W, wpr, bpr, w);
  hipLaunchKernelGGL(seed_merge_k, grid, block, 0, st, H, W, wpr, bpr, w, status);
  hipLaunchKernelGGL(seed_count_k, grid, block, 0, st, H, W, wpr, bpr, w, status);
  hipLaunchKernelGGL(seed_pick_k, grid, block, 0, st, H, W, wpr, bpr, w);
  hipLaunchKernelGGL(clean_kbits_k, grid, block, 0, st, flags, n, min_area, H, W, wpr, bpr, w);
  hipLaunchKernelGGL(clean_merge4_k, grid, block, 0, st, H, W, wpr, bpr, wc, status);
  hipLaunchKernelGGL(clean_border_k, grid, block, 0, st, H, W, wpr, bpr, wc, status);
  hipLaunchKernelGGL(clean_fill_k, grid, block, 0, st, n, H, W, wpr, bpr, w);
  hipLaunchKernelGGL(clean_final_k, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, flags, n, min_area, H, W, w, (long long*)stats);
  hipLaunchKernelGGL(clean_paint_k, dim3((unsigned)(nframes * bpr)), block, 0, st, (long long*)out, nframes, frame_of, paint_cls, n,
                     (long long)fill_cls, H, W, wpr, bpr, w);
  return egne::check_launch("egne_class_map_cleanup");
}
