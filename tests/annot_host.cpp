// Host program of tests/test_host_annot.py: the rules of the label maps from TEyeD annotations (csrc/annot_core.h, the kernel's own
// text) on a host.  It paints every frame the way the kernel does -- the shapes pixel by pixel, the lid through the per-row crossings
// of edge_row -- and checks the row form against the per-pixel definition (in_polygon) on every pixel.  Built with
// -fsanitize=address,undefined and without FMA contraction; never loaded into Python.
//   annot_host <in> <out>
// <in>:  int32 cases; per case int32 B, R, C, has_hw, with_skin; int32 records [B][150]; int32 src_hw [B][2] if has_hw
// <out>: per case int8 noskin [B][R][C]; int8 skin [B][R][C] if with_skin; int32 status [B]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "annot_core.h"

namespace an = egne_annot;

template <class T>
static void rd(FILE* f, T* p, size_t n) {
  if (n && fread(p, sizeof(T), n, f) != n) exit(2);
}
template <class T>
static void wr(FILE* f, const T* p, size_t n) {
  if (n && fwrite(p, sizeof(T), n, f) != n) exit(3);
}
static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int cases = 0;
  rd(in, &cases, 1);
  for (int cs = 0; cs < cases; ++cs) {
    int hdr[5];
    rd(in, hdr, 5);
    const int B = hdr[0], R = hdr[1], C = hdr[2], has_hw = hdr[3], with_skin = hdr[4];
    std::vector<int32_t> recs((size_t)B * an::kRecordWords);
    std::vector<int> hw((size_t)B * 2);
    rd(in, recs.data(), recs.size());
    if (has_hw) rd(in, hw.data(), hw.size());
    std::vector<int8_t> noskin((size_t)B * R * C, 0), skin((size_t)B * R * C, 0);
    std::vector<int> status(B, 0);
    for (int b = 0; b < B; ++b) {
      // (a copy of exactly one record: a read past its end is a sanitizer finding)
      std::vector<int32_t> rec(recs.begin() + (size_t)b * an::kRecordWords, recs.begin() + (size_t)(b + 1) * an::kRecordWords);
      const int r = has_hw ? clampi(hw[2 * b], 0, R) : R, c = has_hw ? clampi(hw[2 * b + 1], 0, C) : C;
      const int n = an::lid_count(rec.data());
      const bool lid = (rec[0] & an::HAS_LID) != 0;
      const int32_t* v = rec.data() + an::kLidWord;
      int st = an::record_status(rec.data());
      bool painted = false;
      for (int y = 0; y < r; ++y) {
        std::vector<int> xc, bl, bh;
        for (int i = 0; i < n; ++i) {
          const int j = i + 1 == n ? 0 : i + 1;
          const an::EdgeRow e = an::edge_row(v[2 * i], v[2 * i + 1], v[2 * j], v[2 * j + 1], y);
          if (e.toggles) xc.push_back(e.xc);
          if (e.bl <= e.bh) { bl.push_back(e.bl); bh.push_back(e.bh); }
        }
        for (int x = 0; x < c; ++x) {
          const int8_t m = an::noskin_at(rec.data(), x, y);
          painted = painted || m != 0;
          bool hold = false;
          for (int t : xc) hold ^= x < t;
          for (size_t t = 0; t < bl.size(); ++t) hold = hold || (x >= bl[t] && x <= bh[t]);
          if (hold != an::in_polygon(x, y, v, n)) {
            fprintf(stderr, "case %d frame %d pixel (%d, %d): the row form and the definition disagree\n", cs, b, x, y);
            return 4;
          }
          const size_t o = ((size_t)b * R + y) * C + x;
          noskin[o] = m;
          skin[o] = (!lid || hold) ? m : (int8_t)0;
        }
      }
      status[b] = st | (painted ? 0 : (int)an::ST_EMPTY);
    }
    wr(out, noskin.data(), noskin.size());
    if (with_skin) wr(out, skin.data(), skin.size());
    wr(out, status.data(), status.size());
  }
  fclose(in);
  fclose(out);
  printf("cases %d\n", cases);
  return 0;
}
