// Class-map clean-up (csrc/cleanup.hip): the bit arithmetic on 64-bit row words -- bit l of word c of an image row is
// column 64 c + l.  The 3x3-cross opening of a word from its neighbours, the runs of ones of a word, and which runs of the row above
// a run touches vertically (4-connectivity).  Plain integer C++: the kernels include it, and tests/cleanup_host.cpp compiles the very
// same text with a host compiler under -fsanitize=address,undefined.  No HIP type appears here.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EGNE_CL_HD __host__ __device__ inline
#else
#define EGNE_CL_HD inline
#endif

namespace egne_cleanup {

typedef unsigned long long word_t;

// the columns of word c that lie inside a row of W pixels (c may be -1 or past the last word: 0)
EGNE_CL_HD word_t row_mask(int W, int c) {
  if (c < 0 || (long long)c * 64 >= W) return 0ull;
  const int left = W - c * 64;
  return left >= 64 ? ~0ull : (1ull << left) - 1ull;
}

// cv2.erode with the 3x3 cross, one word: a pixel survives iff it and its four neighbours are set.  up / dn: the same word of the rows
// above / below; lbit / rbit: column -1 / 64 of this word (bit 63 of the word to the left, bit 0 of the word to the right).  What
// lies outside the frame does not constrain: the caller hands it over as ones.
EGNE_CL_HD word_t erode_word(word_t up, word_t cur, word_t dn, word_t lbit, word_t rbit) {
  return cur & up & dn & ((cur << 1) | (lbit & 1ull)) & ((cur >> 1) | ((rbit & 1ull) << 63));
}

// cv2.dilate with the 3x3 cross, one word.  What lies outside the frame is background: the caller hands it over as zeros.
EGNE_CL_HD word_t dilate_word(word_t up, word_t cur, word_t dn, word_t lbit, word_t rbit) {
  return cur | up | dn | (cur << 1) | (lbit & 1ull) | (cur >> 1) | ((rbit & 1ull) << 63);
}

// The opening of word c of image row y.  s[dy + 2][dc + 1]: membership of rows y-2 .. y+2, words c-1 .. c+1, with EVERY bit outside
// the frame set (rows above 0 and below H-1, words left of 0 and right of the last one, the columns beyond W-1 of the last word);
// s[0][0], s[0][2], s[4][0], s[4][2] are not read.  The erosion of the three rows y-1 .. y+1 of this word and of the two edge bits
// next to it in row y, then the dilation; erosion values outside the frame are zeros, and so are the result's bits beyond W-1.
EGNE_CL_HD word_t open3_word(const word_t s[5][3], int y, int c, int H, int W) {
  const word_t ml = row_mask(W, c - 1), mc = row_mask(W, c), mr = row_mask(W, c + 1);
  word_t e[3];
  for (int k = 0; k < 3; ++k) {
    const int yy = y + k - 1;
    e[k] = (yy < 0 || yy >= H) ? 0ull : erode_word(s[k][1], s[k + 1][1], s[k + 2][1], s[k + 1][0] >> 63, s[k + 1][2]) & mc;
  }
  // the left word's bit 63 (its own left neighbour is its bit 62) and the right word's bit 0 (its right neighbour is its bit 1)
  const word_t el = (erode_word(s[1][0], s[2][0], s[3][0], 1ull, s[2][1]) & ml) >> 63;
  const word_t er = erode_word(s[1][2], s[2][2], s[3][2], s[2][1] >> 63, 1ull) & mr & 1ull;
  return dilate_word(e[0], e[1], e[2], el, er) & mc;
}

// runs of ones inside a word -----------------------------------------------------------------------------------------------------------
EGNE_CL_HD bool run_begins(word_t w, int l) { return ((w >> l) & 1ull) && (l == 0 || !((w >> (l - 1)) & 1ull)); }

// first bit of the run that holds bit l (bit l set)
EGNE_CL_HD int run_first(word_t w, int l) {
  const word_t below = ~w & ((1ull << l) - 1ull);
  return below ? 64 - __builtin_clzll(below) : 0;
}

// ones from bit l upwards (bit l set)
EGNE_CL_HD int run_length(word_t w, int l) {
  const word_t inv = ~(w >> l);
  return inv ? __builtin_ctzll(inv) : 64;
}

// the bits of the run that begins at bit l
EGNE_CL_HD word_t run_bits(word_t w, int l) {
  const int n = run_length(w, l);
  return (n >= 64 ? ~0ull : (1ull << n) - 1ull) << l;
}

// Vertical 4-overlap: calls f(first bit) for every run of `above` (the same word of the row above) that shares a column with the run
// `mine` (bits of one run of this row's word).  No diagonals.  At most 32 runs fit a word: the loop is bounded by that.
template <class F>
EGNE_CL_HD void for_each_overlap4(word_t mine, word_t above, F f) {
  word_t ov = mine & above;
  for (int k = 0; k < 32 && ov; ++k) {
    const int b = __builtin_ctzll(ov);
    const int first = run_first(above, b);
    f(first);
    ov &= ~run_bits(above, first);
  }
}

}  // namespace egne_cleanup
