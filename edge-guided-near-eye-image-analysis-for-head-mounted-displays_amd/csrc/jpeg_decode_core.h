// The per-lane entropy-decoding step of the device Motion-JPEG decoder (csrc/jpeg_decode.hip; definition: include/egne_hip.h, DESIGN.md
// 6f): bit reader, symbol decode, state advance and the bounds rules, as inline functions that compile for the device AND for the host,
// so that a stand-alone host program (tests/jpeg_decode_host.cpp, built with the address / undefined-behaviour sanitizers) runs the very
// code the kernels run.  Nothing here touches memory outside the arrays it is handed:
//   * every stream read is clamped to the frame's unstuffed scan: bits beyond its end read as 1;
//   * a table index is masked to the table; a coefficient is written only at block < the segment's expected count and index <= 63;
//   * an invalid code, a category the baseline process does not have, a zigzag index past 63 or a symbol that ends past the segment
//     stops the walk: in the guessing / synchronisation passes (WRITE = false) with an invalid state and nothing more, in the final
//     pass (WRITE = true) with the return value 1 (the frame's flag).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JD_HD __host__ __device__ __forceinline__
#else
#define JD_HD inline
#endif

namespace jd {

// ---- the descriptor of one frame (egne_hip.h): 8 int32 words, 4 x 64 divisors, 4 x (16 counts + 256 symbols) -------------------------
constexpr int DESC_BYTES = 1408, DESC_QT = 32, DESC_HUFF = 288, HUFF_BYTES = 272;
enum { D_SCAN_OFF = 0, D_SCAN_LEN = 1, D_RESTART = 2, D_TQ = 3, D_TD = 4, D_TA = 5 };
enum { GREY = 0, S444 = 1, S422 = 2, S420 = 3 };

struct Geom {
  int hs, vs;        // luminance blocks per MCU, horizontally / vertically
  int bpm, nlum;     // blocks per MCU, of which luminance
  int mw, mh, nmcu;  // MCUs per row / column / frame
};

JD_HD Geom geometry(int H, int W, int sampling) {
  Geom g;
  g.hs = (sampling == S422 || sampling == S420) ? 2 : 1;
  g.vs = sampling == S420 ? 2 : 1;
  g.nlum = g.hs * g.vs;
  g.bpm = sampling == GREY ? 1 : g.nlum + 2;
  g.mw = (W + 8 * g.hs - 1) / (8 * g.hs);
  g.mh = (H + 8 * g.vs - 1) / (8 * g.vs);
  g.nmcu = g.mw * g.mh;
  return g;
}

// ---- code tables: a direct table for codes of up to 8 bits, the canonical walk of T.81 F.2.2.3 for longer ones -----------------------
struct Tables {                // table 0, 1: DC; 2, 3: AC
  uint16_t look[4][256];       // by the next 8 bits: (length << 8) | symbol, 0 = no code of up to 8 bits
  int32_t maxcode[4][17];      // by length 1..16: the largest code of that length, -1 = none
  int32_t valoff[4][17];       // by length: index of its first symbol minus its first code
  uint8_t sym[4][256];
};

// one lane per table: the limits of every code length.  huff = 16 counts, 256 symbols
JD_HD void build_limits(Tables& T, int t, const uint8_t* huff) {
  int code = 0, k = 0;
  T.maxcode[t][0] = -1;
  T.valoff[t][0] = 0;
  for (int l = 1; l <= 16; ++l) {
    const int n = huff[l - 1];
    T.valoff[t][l] = k - code;
    T.maxcode[t][l] = n ? code + n - 1 : -1;
    k += n;
    code = (code + n) << 1;
  }
}

// one lane per (table, index): after build_limits
JD_HD void build_entry(Tables& T, int t, int i, const uint8_t* huff) {
  T.sym[t][i] = huff[16 + i];
  unsigned e = 0;
  for (int l = 1; l <= 8; ++l) {
    const int c = i >> (8 - l);
    if (c <= T.maxcode[t][l]) {
      e = (unsigned)(l << 8) | huff[16 + ((T.valoff[t][l] + c) & 255)];
      break;
    }
  }
  T.look[t][i] = (uint16_t)e;
}

// the symbol whose code starts the 16 bits `peek`; -1 = no code
JD_HD int decode_symbol(const Tables& T, int t, unsigned peek, int& len) {
  const unsigned e = T.look[t][peek >> 8];
  if (e) {
    len = (int)(e >> 8);
    return (int)(e & 255u);
  }
  for (int l = 9; l <= 16; ++l) {
    const int c = (int)(peek >> (16 - l));
    if (c <= T.maxcode[t][l]) {
      len = l;
      return T.sym[t][(T.valoff[t][l] + c) & 255];
    }
  }
  return -1;
}

// ---- bit reader over the frame's unstuffed scan (words: 4-byte aligned, ulen bytes; whatever lies beyond reads as 1-bits) -------------
struct Reader {
  const uint32_t* words;
  int ulen, next;
  uint64_t win;      // the next `avail` bits, left-aligned
  int avail;

  JD_HD uint32_t word(int w) const {
    const long long at = 4LL * w;
    if (w < 0 || at >= ulen) return 0xffffffffu;
    uint32_t v = __builtin_bswap32(words[w]);
    if (at + 4 > ulen) v |= 0xffffffffu >> (8 * (int)(ulen - at));
    return v;
  }
  JD_HD void init(const uint32_t* words_, int ulen_, long long bit) {
    words = words_;
    ulen = ulen_;
    const int w = (int)(bit >> 5), o = (int)(bit & 31);
    win = ((uint64_t)word(w) << 32 | word(w + 1)) << o;
    avail = 64 - o;
    next = w + 2;
    refill();
  }
  JD_HD void refill() {
    if (avail <= 32) {
      win |= (uint64_t)word(next++) << (32 - avail);
      avail += 32;
    }
  }
  JD_HD unsigned peek16() const { return (unsigned)(win >> 48); }
  JD_HD void skip(int n) {           // n <= 16
    win <<= n;
    avail -= n;
    refill();
  }
  JD_HD int receive_extend(int s) {  // T.81 F.2.2.1 / F.2.2.4: s <= 11 value bits -> the signed value
    if (s == 0) return 0;
    const int v = (int)(win >> (64 - s));
    skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
  }
};

// ---- a lane's state at a subsequence boundary ------------------------------------------------------------------------------------------
struct State {
  int32_t p;        // bit position inside the segment of the next symbol; < 0 = invalid
  int32_t bz;       // (block index within the MCU << 8) | zigzag index of the next coefficient (0 = the block's DC symbol comes next)
};
JD_HD bool same(const State& a, const State& b) { return a.p == b.p && a.bz == b.bz; }

// Decodes the symbols of one segment that START in [s.p, end_bit) from the entry state s, leaves the exit state in s and the number of
// blocks completed in `completed`.  seg_byte0 / seg_bits: the segment inside the frame's unstuffed scan.  tsel: bit 2c = DC table, bit
// 2c+1 = AC table of component c.  WRITE: coef = the segment's first block (int16 [.][64], zigzag order, zeroed beforehand; the DC entry
// receives the DIFFERENCE), blk = index inside the segment of the block the entry state is in, nblk = blocks the segment must hold, last
// = the range ends the segment.  The walk stops where block nblk - 1 ends.  Returns 1 (WRITE only) for: an error met before that, more
// than 7 bits left behind the last block, fewer than nblk blocks at the end of the segment.  An invalid entry state, or an entry at or
// beyond block nblk, returns 0: the lane that met the error has reported it, or the segment was complete before this range.
template <bool WRITE>
JD_HD int decode_range(const Tables& T, const uint32_t* words, int ulen, int seg_byte0, int seg_bits, int end_bit, State& s,
                       int& completed, unsigned tsel, int bpm, int nlum, int16_t* coef, int blk, int nblk, bool last) {
  completed = 0;
  if (s.p < 0) return 0;
  if (WRITE && blk >= nblk) return 0;
  int p = s.p, b = s.bz >> 8, z = s.bz & 255;
  if (b < 0 || b >= bpm || z > 63) {
    s.p = -1;
    return WRITE ? 1 : 0;
  }
  Reader r;
  r.init(words, ulen, 8LL * seg_byte0 + p);
  bool bad = false, done = false;
  while (p < end_bit) {
    const int comp = b < nlum ? 0 : b - nlum + 1;
    int len = 0;
    bool ends = false;
    if (z == 0) {
      const int cat = decode_symbol(T, (int)((tsel >> (2 * comp)) & 1u), r.peek16(), len);
      if (cat < 0 || cat > 11 || p + len + cat > seg_bits) { bad = true; break; }
      r.skip(len);
      const int v = r.receive_extend(cat);
      if (WRITE) coef[(long long)blk * 64] = (int16_t)v;
      p += len + cat;
      z = 1;
    } else {
      const int rs = decode_symbol(T, 2 + (int)((tsel >> (2 * comp + 1)) & 1u), r.peek16(), len);
      if (rs < 0) { bad = true; break; }
      const int run = rs >> 4, cat = rs & 15;
      if (cat == 0) {
        if (run == 15) z += 16;               // ZRL
        else if (run == 0) ends = true;       // EOB
        else { bad = true; break; }
        if (z > 63 || p + len > seg_bits) { bad = true; break; }
        r.skip(len);
        p += len;
      } else {
        z += run;
        if (cat > 10 || z > 63 || p + len + cat > seg_bits) { bad = true; break; }
        r.skip(len);
        const int v = r.receive_extend(cat);
        if (WRITE) coef[(long long)blk * 64 + z] = (int16_t)v;
        p += len + cat;
        ends = ++z == 64;
      }
    }
    if (ends) {
      z = 0;
      b = b + 1 == bpm ? 0 : b + 1;
      ++completed;
      if (WRITE && ++blk == nblk) { done = true; break; }
    }
  }
  if (bad) {
    s.p = -1;
    return WRITE ? 1 : 0;
  }
  s.p = p;
  s.bz = b << 8 | z;
  if (WRITE && done) return seg_bits - p >= 8 ? 1 : 0;
  return (WRITE && last) ? 1 : 0;
}

}  // namespace jd
