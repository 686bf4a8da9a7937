// 8-connected components of a region on 64-bit row words: the per-row workspace, the bit helpers, find / union and the launches
// seed_zero_k .. seed_pick_k, shared by csrc/mask_seed.hip (ellipse seeds from the class map) and csrc/cleanup.hip (class-map
// clean-up).  Device code; include it inside the including file's anonymous namespace, after common.h.  The launches and their rules
// are described at the top of mask_seed.hip; nothing here differs between the two users, so a shared launch gives both the same bits.
#pragma once

typedef unsigned long long u64;

struct RowWs {
  u64* bits;       // [H][wpr]
  int* label;      // [H*W], nodes only
  unsigned* area;  // [H*W], roots only
  u64* acc;        // [16]: 0 best key, 1 components, 2 region pixels, 3..8 sums, 9 failed (10..15: csrc/cleanup.hip)
};

__host__ __device__ inline size_t seed_row_bytes(int H, int W) {
  const size_t wpr = (size_t)(W + 63) / 64;
  return (size_t)H * wpr * 8 + (size_t)H * W * 8 + 128;
}

__device__ __forceinline__ RowWs row_ws(char* ws, int i, int H, int W) {
  const size_t wpr = (size_t)(W + 63) / 64;
  char* p = ws + (size_t)i * seed_row_bytes(H, W);
  RowWs r;
  r.acc = (u64*)p;
  r.bits = (u64*)(p + 128);
  r.label = (int*)(p + 128 + (size_t)H * wpr * 8);
  r.area = (unsigned*)(p + 128 + (size_t)H * wpr * 8 + (size_t)H * W * 4);
  return r;
}

// which (row, image row, word) this wave works on; false past the end.  bpr = workgroups (four waves = four words) per row
__device__ __forceinline__ bool locate(int H, int wpr, int bpr, int& i, int& y, int& c) {
  i = blockIdx.x / bpr;
  const int word = (blockIdx.x % bpr) * 4 + (threadIdx.x >> 6);
  y = word / wpr;
  c = word % wpr;
  return word < H * wpr;
}

__device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// first pixel of the run of ones that holds bit l of word w (bit l set): column offset inside the word
__device__ __forceinline__ int run_start(u64 w, int l) {
  const u64 below = ~w & ((1ull << l) - 1ull);
  return below ? 64 - __clzll((long long)below) : 0;
}
__device__ __forceinline__ bool is_node(u64 w, int l) { return ((w >> l) & 1ull) && (l == 0 || !((w >> (l - 1)) & 1ull)); }
__device__ __forceinline__ int run_len(u64 w, int l) {   // ones from bit l upwards
  const u64 inv = ~(w >> l);
  return inv ? __ffsll((long long)inv) - 1 : 64;          // (w >> l has zeros above bit 63 - l, so inv is 0 only for l = 0, w all ones)
}

__device__ __forceinline__ int find(const int* label, int x, int& budget) {
  while (budget > 0) {
    const int p = ld(label + x);
    if (p == x) return x;
    x = p;
    --budget;
  }
  return -1;
}

// false when the step bound was reached
__device__ __forceinline__ bool unite(int* label, int a, int b, int budget) {
  while (budget > 0) {
    a = find(label, a, budget);
    if (a < 0) return false;
    b = find(label, b, budget);
    if (b < 0) return false;
    if (a == b) return true;
    if (a < b) { const int t = a; a = b; b = t; }        // a > b: hang the larger root under the smaller
    const int old = atomicMin(label + a, b);
    if (old == a) return true;
    a = old;                                             // somebody moved it first: go on from where it points now
    --budget;
  }
  return false;
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ u64 wave_max(u64 v) {
  for (int o = 32; o > 0; o >>= 1) { const u64 t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
  return v;
}

__global__ void seed_zero_k(char* ws, int n, int H, int W, int* status) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) *status = 0;
  if (t < n * 16) row_ws(ws, t >> 4, H, W).acc[t & 15] = 0ull;
}

__global__ __launch_bounds__(256) void seed_pack_k(const long long* __restrict__ mask, int nframes, const int* __restrict__ frame_of,
                                                   const int* __restrict__ class_bits, int H, int W, int wpr, int bpr, char* ws) {
  int i, y, c;
  if (!locate(H, wpr, bpr, i, y, c)) return;
  const int l = threadIdx.x & 63, x = c * 64 + l;
  const RowWs r = row_ws(ws, i, H, W);
  const int fr = frame_of[i];
  const unsigned cb = (unsigned)class_bits[i];
  bool in = false;
  if (fr >= 0 && fr < nframes && cb != 0u && x < W) {     // a frame the mask tensor does not hold: read nothing
    const long long k = mask[((size_t)fr * H + y) * W + x];
    in = k >= 0 && k < 32 && ((cb >> (int)k) & 1u);
  }
  const u64 w = __ballot(in);
  if (l == 0) r.bits[(size_t)y * wpr + c] = w;
  if (in && is_node(w, l)) {
    const int p = y * W + x;
    r.label[p] = p;
    r.area[p] = 0u;
  }
}

__global__ __launch_bounds__(256) void seed_merge_k(int H, int W, int wpr, int bpr, char* ws, int* status) {
  int i, y, c;
  if (!locate(H, wpr, bpr, i, y, c)) return;
  const int l = threadIdx.x & 63, x = c * 64 + l;
  const RowWs r = row_ws(ws, i, H, W);
  const u64* brow = r.bits + (size_t)y * wpr;
  const u64 cur = brow[c];
  if (!((cur >> l) & 1ull)) return;
  const int bound = 4 * H * W + 64;
  const int me = y * W + c * 64 + run_start(cur, l);
  bool ok = true;
  // the pixel of column xx in image row yy: member?  and its node
  auto member = [&](int yy, int xx) -> bool {
    if (xx < 0 || xx >= W || yy < 0) return false;
    return (r.bits[(size_t)yy * wpr + (xx >> 6)] >> (xx & 63)) & 1ull;
  };
  auto node_of = [&](int yy, int xx) -> int {
    const u64 w = r.bits[(size_t)yy * wpr + (xx >> 6)];
    return yy * W + (xx & ~63) + run_start(w, xx & 63);
  };
  const bool Wm = member(y, x - 1);
  // a run that goes on across the word boundary: two nodes, one run
  if (l == 0 && Wm) ok &= unite(r.label, me, node_of(y, x - 1), bound);
  if (y > 0) {
    const bool Nm = member(y - 1, x), NWm = member(y - 1, x - 1);
    if (Nm) {
      // W and NW both present: W is joined to NW (its own N, by this rule applied to it), NW to N and W to this pixel along their rows
      if (!(Wm && NWm)) ok &= unite(r.label, me, node_of(y - 1, x), bound);
    } else {
      // (with N present NW and NE hang on N along its row.)  NW: W, if present, carries it as its N.  NE: E, if present, carries it as its N
      if (NWm && !Wm) ok &= unite(r.label, me, node_of(y - 1, x - 1), bound);
      if (member(y - 1, x + 1) && !member(y, x + 1)) ok &= unite(r.label, me, node_of(y - 1, x + 1), bound);
    }
  }
  if (!ok) {
    atomicOr(status, 1);
    atomicOr((unsigned long long*)(r.acc + 9), 1ull);
  }
}

__global__ __launch_bounds__(256) void seed_count_k(int H, int W, int wpr, int bpr, char* ws, int* status) {
  int i, y, c;
  if (!locate(H, wpr, bpr, i, y, c)) return;
  const int l = threadIdx.x & 63;
  const RowWs r = row_ws(ws, i, H, W);
  const u64 cur = r.bits[(size_t)y * wpr + c];
  if (!is_node(cur, l)) return;
  const int p = y * W + c * 64 + l;
  int budget = 4 * H * W + 64;
  const int root = find(r.label, p, budget);
  if (root < 0) {
    atomicOr(status, 1);
    atomicOr((unsigned long long*)(r.acc + 9), 1ull);
    return;
  }
  // (other nodes walk through label[p] meanwhile: old and new value both lead to the root)
  __hip_atomic_store(r.label + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  atomicAdd(r.area + root, (unsigned)run_len(cur, l));
}

__global__ __launch_bounds__(256) void seed_pick_k(int H, int W, int wpr, int bpr, char* ws) {
  int i, y, c;
  if (!locate(H, wpr, bpr, i, y, c)) return;     // (whole waves leave: the shuffles below see all 64 lanes)
  const int l = threadIdx.x & 63;
  const RowWs r = row_ws(ws, i, H, W);
  const u64 cur = r.bits[(size_t)y * wpr + c];
  if (cur == 0ull) return;
  const int p = y * W + c * 64 + l;
  u64 key = 0ull, comps = 0ull, px = 0ull;
  if (is_node(cur, l) && r.label[p] == p) {
    const unsigned a = r.area[p];
    key = ((u64)a << 32) | (u64)(0xffffffffu - (unsigned)p);      // most pixels; on a tie the earliest first pixel
    comps = 1ull;
    px = a;
  }
  key = wave_max(key); comps = wave_sum(comps); px = wave_sum(px);
  if (l == 0 && comps) {
    atomicMax((unsigned long long*)(r.acc + 0), key);
    atomicAdd((unsigned long long*)(r.acc + 1), comps);
    atomicAdd((unsigned long long*)(r.acc + 2), px);
  }
}

inline bool seed_shape_ok(int H, int W) {
  return H >= 2 && W >= 2 && H <= 1024 && W <= 1024 && (long long)H * W <= (1ll << 20);
}
