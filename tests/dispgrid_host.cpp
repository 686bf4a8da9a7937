// Host program of tests/test_host_dispgrid.py: the arithmetic of the overlay grid kernels (csrc/dispgrid_core.h, the kernels' own text)
// on a host -- the order-preserving keys, the uint8 conversion, the equalisation and grey tables, the uint8 form of a grid value, the
// outline samples with their clip, and the grid offsets.  Built with -fsanitize=address,undefined and without FMA contraction.
//   dispgrid_host <in> <out>
// <in>:  float64 cos t [720], sin t [720]; int32 nf, then nf float32 grid values; int32 nh, then nh x int32 [256] histograms;
//        int32 cases; per case int32 H, W, n, nrow, nel, then float32 [n][H][W] frames, then nel x float64 [7]
//        (pixel ellipse cx, cy, a, b, theta, then cos theta, sin theta)
// <out>: uint8 [nf]; per histogram uint8 lut[256], float32 grey[256]; per case: per frame float32 mn, float32 d, uint8 u[H][W],
//        uint8 lut[256], float32 grey[256]; int32 Hg, Wg, then n x int32 (row, col); per ellipse int32 drawn, rows[720], cols[720]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dispgrid_core.h"

namespace dg = egne_dispgrid;

template <class T>
static void rd(FILE* f, T* p, size_t n) {
  if (n && fread(p, sizeof(T), n, f) != n) exit(2);
}
template <class T>
static void wr(FILE* f, const T* p, size_t n) {
  if (n && fwrite(p, sizeof(T), n, f) != n) exit(3);
}

static void tables(FILE* out, const int* hist, int total) {
  uint8_t lut[256];
  float grey[256];
  dg::build_tables(hist, total, lut, grey);
  wr(out, lut, 256);
  wr(out, grey, 256);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  std::vector<double> cs(1440);
  rd(in, cs.data(), 1440);
  int nf = 0, nh = 0, cases = 0;
  rd(in, &nf, 1);
  std::vector<float> gv(nf);
  rd(in, gv.data(), gv.size());
  std::vector<uint8_t> g8(nf);
  for (int k = 0; k < nf; ++k) g8[k] = dg::u8_of_grid(gv[k]);
  wr(out, g8.data(), g8.size());
  rd(in, &nh, 1);
  for (int k = 0; k < nh; ++k) {
    int hist[256];
    long long total = 0;
    rd(in, hist, 256);
    for (int j = 0; j < 256; ++j) total += hist[j];
    tables(out, hist, (int)total);
  }
  rd(in, &cases, 1);
  for (int c = 0; c < cases; ++c) {
    int hdr[5];
    rd(in, hdr, 5);
    const int H = hdr[0], W = hdr[1], n = hdr[2], nrow = hdr[3], nel = hdr[4];
    std::vector<float> frame((size_t)H * W);
    std::vector<uint8_t> u((size_t)H * W);
    for (int i = 0; i < n; ++i) {
      rd(in, frame.data(), frame.size());
      // the kernels' reduction: integer maxima of the keys, the minimum as the complement of its key; non-finite pixels are left out
      uint32_t kmax = 0u, kmin = 0u;
      for (float x : frame)
        if (dg::finite_f32(x)) {
          const uint32_t k = dg::order_key(x);
          kmax = k > kmax ? k : kmax;
          kmin = ~k > kmin ? ~k : kmin;
        }
      const float mx = dg::key_value(kmax), mn = dg::key_value(~kmin), d = mx - mn;
      int hist[256] = {0};
      for (size_t p = 0; p < frame.size(); ++p) {
        u[p] = dg::to_u8(frame[p], mn, d);
        ++hist[u[p]];
      }
      wr(out, &mn, 1);
      wr(out, &d, 1);
      wr(out, u.data(), u.size());
      tables(out, hist, H * W);
    }
    const dg::Layout lay = dg::grid_layout(n, nrow, H, W);
    wr(out, &lay.Hg, 1);
    wr(out, &lay.Wg, 1);
    for (int i = 0; i < n; ++i) {
      int rc[2];
      dg::grid_origin(i, n, lay, H, W, &rc[0], &rc[1]);
      wr(out, rc, 2);
    }
    for (int e = 0; e < nel; ++e) {
      double el[7];
      rd(in, el, 7);
      const int drawn = dg::ellipse_drawn(el) ? 1 : 0;
      std::vector<int> rows(720, -1), cols(720, -1);
      if (drawn)
        for (int s = 0; s < 720; ++s)
          dg::outline_px(trunc(el[0]), trunc(el[1]), trunc(el[2]), trunc(el[3]), el[5], el[6], cs[s], cs[720 + s], H, W, &rows[s], &cols[s]);
      wr(out, &drawn, 1);
      wr(out, rows.data(), 720);
      wr(out, cols.data(), 720);
    }
  }
  fclose(in);
  fclose(out);
  printf("cases %d\n", cases);
  return 0;
}
