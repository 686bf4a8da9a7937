// Host program of tests/test_host_cleanup.py: the class-map clean-up on one frame with the bit arithmetic of csrc/cleanup_core.h -- the
// opening of row words, run enumeration and the vertical 4-overlap are the kernels' own text; the union-find around them is sequential.
// Built with -fsanitize=address,undefined.
//   cleanup_host <in> <out>
// <in>:  int32 cases; per case int32 H, W, n, open3, min_area, fill_cls, then n x (class_bits, paint_cls, flags) int32, then int64 [H][W]
// <out>: per case int64 [H][W] cleaned map, then int64 [n][4] statistics
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cleanup_core.h"

namespace cl = egne_cleanup;
typedef cl::word_t u64;

static int find(std::vector<int>& lab, int x) {
  while (lab[x] != x) {
    lab[x] = lab[lab[x]];
    x = lab[x];
  }
  return x;
}
static void unite(std::vector<int>& lab, int a, int b) {
  a = find(lab, a);
  b = find(lab, b);
  if (a == b) return;
  if (a < b) lab[b] = a; else lab[a] = b;                  // the smaller index stays the root: a component's root is its first pixel
}

struct Frame {
  int H, W, wpr;
  const long long* m;
  // membership of class `cls` in word c of row y, everything outside the frame SET (the erosion's border)
  u64 member_or_outside(int cls, int y, int c) const {
    if (y < 0 || y >= H || c < 0 || c >= wpr) return ~0ull;
    u64 w = ~cl::row_mask(W, c);
    for (int l = 0; l < 64 && c * 64 + l < W; ++l)
      if (m[(size_t)y * W + c * 64 + l] == cls) w |= 1ull << l;
    return w;
  }
};

static void one_case(FILE* in, FILE* out) {
  int hdr[6];
  if (fread(hdr, 4, 6, in) != 6) exit(2);
  const int H = hdr[0], W = hdr[1], n = hdr[2], open3 = hdr[3], min_area = hdr[4];
  const long long fill_cls = hdr[5];
  std::vector<int> rows((size_t)n * 3);
  std::vector<long long> mask((size_t)H * W), res((size_t)H * W, fill_cls), stats((size_t)n * 4, 0);
  if (n && fread(rows.data(), 4, rows.size(), in) != rows.size()) exit(2);
  if (fread(mask.data(), 8, mask.size(), in) != mask.size()) exit(2);
  const int wpr = (W + 63) / 64;
  const Frame fr = {H, W, wpr, mask.data()};
  for (int i = 0; i < n; ++i) {
    const unsigned cb = (unsigned)rows[i * 3];
    const int paint = rows[i * 3 + 1], fl = rows[i * 3 + 2];
    // R as row words
    std::vector<u64> R((size_t)H * wpr, 0ull);
    for (int cls = 0; cls < 32; ++cls) {
      if (!((cb >> cls) & 1u)) continue;
      for (int y = 0; y < H; ++y)
        for (int c = 0; c < wpr; ++c) {
          if (open3) {
            u64 s[5][3];
            for (int dy = 0; dy < 5; ++dy)
              for (int dc = 0; dc < 3; ++dc) s[dy][dc] = fr.member_or_outside(cls, y + dy - 2, c + dc - 1);
            R[(size_t)y * wpr + c] |= cl::open3_word(s, y, c, H, W);
          } else {
            R[(size_t)y * wpr + c] |= fr.member_or_outside(cls, y, c) & cl::row_mask(W, c);
          }
        }
    }
    auto bit = [&](const std::vector<u64>& b, int y, int x) -> bool {
      return y >= 0 && y < H && x >= 0 && x < W && ((b[(size_t)y * wpr + (x >> 6)] >> (x & 63)) & 1ull);
    };
    // 8-connected components of R, pixel by pixel
    std::vector<int> lab((size_t)H * W);
    for (int p = 0; p < H * W; ++p) lab[p] = p;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        if (!bit(R, y, x)) continue;
        const int p = y * W + x;
        if (bit(R, y, x - 1)) unite(lab, p, p - 1);
        for (int dx = -1; dx <= 1; ++dx)
          if (bit(R, y - 1, x + dx)) unite(lab, p, p - W + dx);
      }
    std::vector<int> area((size_t)H * W, 0);
    long long rpx = 0, comps = 0, best_area = 0;
    int best = -1;
    for (int p = 0; p < H * W; ++p)
      if (bit(R, p / W, p % W)) { ++area[find(lab, p)]; ++rpx; }
    for (int p = 0; p < H * W; ++p)
      if (area[p] > 0) {
        ++comps;
        if (area[p] > best_area) { best_area = area[p]; best = p; }      // ascending p: the first of equal areas stays
      }
    const long long kpx = (fl & 1) ? best_area : rpx;
    stats[(size_t)i * 4 + 0] = rpx;
    stats[(size_t)i * 4 + 1] = comps;
    stats[(size_t)i * 4 + 2] = kpx;
    if (kpx < min_area || kpx == 0) continue;
    std::vector<u64> K((size_t)H * wpr, 0ull);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x)
        if (bit(R, y, x) && (!(fl & 1) || find(lab, y * W + x) == best)) K[(size_t)y * wpr + (x >> 6)] |= 1ull << (x & 63);
    std::vector<u64> P = K;
    if (fl & 2) {
      // the complement's runs, 4-connected: nodes are run starts inside a word
      std::vector<u64> C((size_t)H * wpr);
      for (int y = 0; y < H; ++y)
        for (int c = 0; c < wpr; ++c) C[(size_t)y * wpr + c] = ~K[(size_t)y * wpr + c] & cl::row_mask(W, c);
      for (int p = 0; p < H * W; ++p) lab[p] = p;
      for (int y = 0; y < H; ++y)
        for (int c = 0; c < wpr; ++c) {
          const u64 cur = C[(size_t)y * wpr + c];
          for (int l = 0; l < 64; ++l) {
            if (!cl::run_begins(cur, l)) continue;
            const int me = y * W + c * 64 + l;
            if (l == 0 && c > 0 && (C[(size_t)y * wpr + c - 1] >> 63))
              unite(lab, me, y * W + (c - 1) * 64 + cl::run_first(C[(size_t)y * wpr + c - 1], 63));
            if (y > 0)
              cl::for_each_overlap4(cl::run_bits(cur, l), C[(size_t)(y - 1) * wpr + c],
                                    [&](int first) { unite(lab, me, (y - 1) * W + c * 64 + first); });
          }
        }
      std::vector<char> open_root((size_t)H * W, 0);
      for (int pass = 0; pass < 2; ++pass)
        for (int y = 0; y < H; ++y)
          for (int c = 0; c < wpr; ++c) {
            const u64 cur = C[(size_t)y * wpr + c];
            for (int l = 0; l < 64; ++l) {
              if (!cl::run_begins(cur, l)) continue;
              const int x0 = c * 64 + l, x1 = x0 + cl::run_length(cur, l) - 1, root = find(lab, y * W + x0);
              if (pass == 0) {
                if (y == 0 || y == H - 1 || x0 == 0 || x1 == W - 1) open_root[root] = 1;
              } else if (!open_root[root]) {
                P[(size_t)y * wpr + c] |= cl::run_bits(cur, l);
                stats[(size_t)i * 4 + 3] += x1 - x0 + 1;
              }
            }
          }
    }
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x)
        if (bit(P, y, x)) res[(size_t)y * W + x] = paint;
  }
  fwrite(res.data(), 8, res.size(), out);
  fwrite(stats.data(), 8, stats.size(), out);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int cases = 0;
  if (fread(&cases, 4, 1, in) != 1) return 2;
  for (int k = 0; k < cases; ++k) one_case(in, out);
  fclose(in);
  fclose(out);
  printf("cases %d\n", cases);
  return 0;
}
