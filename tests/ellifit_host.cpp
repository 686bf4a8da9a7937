// Stand-alone host program over csrc/ellifit_core.h (tests/test_host_ellifit.py builds it with -fsanitize=address,undefined).
//   ellifit_host layout                 the launcher's offset and size arithmetic over the accepted sizes: every region of every row
//                                       of a workspace of exactly egne_ellipse_ransac_workspace_bytes is written end to end (the
//                                       sanitizer sees any byte outside), regions are aligned and do not overlap, refused sizes are
//                                       negative, the LDS size holds the kernel's carve-up
//   ellifit_host fit IN OUT             IN: int32 count of sets, then per set int32 n and n x (int32 x, int32 y); OUT per set 12
//                                       doubles: Phi[5], model[5], valid, mean residual -- the device's Fit with the sums taken
//                                       in list order
//   ellifit_host draws SEED ROW N NMIN ITERS   the generated draws, one line per iteration (empty line: attempts exhausted)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ellifit_core.h"

static int fail(const char* what, long a, long b, long c) {
  std::fprintf(stderr, "FAIL %s (%ld %ld %ld)\n", what, a, b, c);
  return 1;
}

static int run_layout() {
  const int sizes[] = {2, 3, 24, 40, 63, 64, 65, 70, 127, 128, 129, 130, 240, 320, 1000, 1023, 1024};
  const int caps[] = {2, 256, 4096, 16384};
  long checked = 0;
  for (int H : sizes)
    for (int W : sizes)
      for (int mp : caps)
        for (int n : {1, 3}) {
          const int64_t bytes = ef_workspace_bytes(n, H, W, mp);
          if (bytes <= 0) return fail("accepted size refused", H, W, mp);
          const EfLayout l = ef_layout(H, W, mp);
          if ((size_t)bytes != (size_t)n * l.row_bytes) return fail("bytes", H, W, mp);
          if (l.off_bits < 128 || l.off_bits % 8 || l.off_offs % 8 || l.off_pts % 8 || l.row_bytes % 8) return fail("alignment", H, W, mp);
          if (l.off_offs != l.off_bits + l.nwords * 8 || l.off_pts < l.off_offs + l.nwords * 4 || l.row_bytes < l.off_pts + (size_t)mp * 4)
            return fail("overlap", H, W, mp);
          if (l.nwords != (size_t)H * ((W + 63) / 64) || (l.nwords + 255) / 256 > 64) return fail("words", H, W, mp);
          std::vector<unsigned char>* ws = new std::vector<unsigned char>((size_t)bytes);      // heap: red zones on both sides
          unsigned char* p = ws->data();
          for (int i = 0; i < n; ++i) {
            unsigned char* row = p + (size_t)i * l.row_bytes;
            std::memset(row, 1, 128);                                    // header
            std::memset(row + l.off_bits, 2, l.nwords * 8);              // one word per 64 columns
            std::memset(row + l.off_offs, 3, l.nwords * 4);              // their prefix
            std::memset(row + l.off_pts, 4, (size_t)mp * 4);             // the point list
          }
          // the last word / point the kernels can address
          const size_t last_word = (size_t)(H - 1) * l.wpr + (size_t)(W - 1) / 64;
          if (last_word != l.nwords - 1) return fail("last word", H, W, mp);
          if (p[(size_t)(n - 1) * l.row_bytes + l.off_pts + (size_t)(mp - 1) * 4 + 3] != 4) return fail("last point", H, W, mp);
          delete ws;
          if (ef_lds_bytes(mp) < (size_t)mp * 4 + 4 * EF_MAX_NMIN * 4 + 4 * 9 * 8 + 4) return fail("lds", mp, 0, 0);
          ++checked;
        }
  const int bad[][4] = {{1, 1, 64, 256}, {1, 64, 1, 256}, {1, 1025, 64, 256}, {1, 64, 1025, 256}, {0, 64, 64, 256},
                        {1, 64, 64, 0},  {1, 64, 64, 16385}, {1, -5, 64, 256}, {-1, 64, 64, 256}};
  for (const auto& b : bad)
    if (ef_workspace_bytes(b[0], b[1], b[2], b[3]) >= 0) return fail("refused size accepted", b[1], b[2], b[3]);
  std::printf("layout ok: %ld combinations\n", checked);
  return 0;
}

static int run_fit(const char* in, const char* out) {
  FILE* f = std::fopen(in, "rb");
  FILE* g = std::fopen(out, "wb");
  if (!f || !g) return fail("open", 0, 0, 0);
  int32_t sets = 0;
  if (std::fread(&sets, 4, 1, f) != 1) return fail("read", 0, 0, 0);
  for (int s = 0; s < sets; ++s) {
    int32_t n = 0;
    if (std::fread(&n, 4, 1, f) != 1 || n < 0 || n > EF_MAX_PTS) return fail("read n", s, n, 0);
    std::vector<int32_t> xy((size_t)n * 2);
    if (n && std::fread(xy.data(), 8, (size_t)n, f) != (size_t)n) return fail("read points", s, n, 0);
    double res[12];
    for (double& v : res) v = -1.0;
    res[10] = 0.0;
    if (n >= 7) {
      long long sx = 0, sy = 0;
      for (int i = 0; i < n; ++i) { sx += xy[2 * i]; sy += xy[2 * i + 1]; }
      const double xm = (double)sx / (double)n, ym = (double)sy / (double)n;
      double mom[EF_NMOM] = {0};
      for (int i = 0; i < n; ++i) ef_accum(mom, (double)xy[2 * i] - xm, (double)xy[2 * i + 1] - ym);
      bool ok = ef_solve(mom, (double)n, res);
      ok = ok && ef_model(res, xm, ym, res + 5);
      res[10] = ok ? 1.0 : 0.0;
      if (ok) {
        const EfErr e = ef_err_prep(res + 5);
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc += ef_err(e, (double)xy[2 * i], (double)xy[2 * i + 1]);
        res[11] = acc / (double)n;
      }
    }
    std::fwrite(res, 8, 12, g);
  }
  std::fclose(f);
  std::fclose(g);
  return 0;
}

static int run_draws(unsigned seed, unsigned row, int N, int n_min, int iters) {
  if (N < 1 || n_min < 1 || n_min > EF_MAX_NMIN || iters < 0 || iters >= EF_MAX_ITERS) return fail("draws arguments", N, n_min, iters);
  for (int it = 0; it <= iters; ++it) {
    int got[EF_MAX_NMIN], have = 0;
    for (int t = 0; t < 64 * EF_DRAW_ROUNDS && have < n_min; ++t) {
      const int idx = ef_draw_index(ef_hash(seed, row, (unsigned)it, (unsigned)t), N);
      bool fresh = true;
      for (int q = 0; q < have; ++q) fresh = fresh && got[q] != idx;
      if (fresh) got[have++] = idx;
    }
    if (have == n_min)
      for (int q = 0; q < n_min; ++q) std::printf("%d ", got[q]);
    std::printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "layout")) return run_layout();
  if (argc == 4 && !std::strcmp(argv[1], "fit")) return run_fit(argv[2], argv[3]);
  if (argc == 7 && !std::strcmp(argv[1], "draws"))
    return run_draws((unsigned)std::strtoul(argv[2], nullptr, 10), (unsigned)std::strtoul(argv[3], nullptr, 10), std::atoi(argv[4]),
                     std::atoi(argv[5]), std::atoi(argv[6]));
  std::fprintf(stderr, "usage: ellifit_host layout | fit IN OUT | draws SEED ROW N NMIN ITERS\n");
  return 2;
}
