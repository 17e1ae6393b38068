// Instance labelling of predicted masks (gfx950): connected components of a
// uint8 mask with scipy.ndimage.label's numbering, optional hole filling
// (scipy.ndimage.binary_fill_holes), a minimum area and per-instance
// statistics.  No reference counterpart; the definitions are scipy.ndimage's
// (tests/instances_ref.py).
//
// Union-find with "the smaller flat index wins" over a per-frame int32 parent
// array, in ordinary launches on the caller's stream.  Tiles are kInstTH x
// kInstTW = 32 x 64 pixels (one wave = one tile row), one 256-thread block per
// tile, frames on grid.y.  All indices are per-frame int32 (H W < 2^31).
//
// Parent entry of pixel p after pass (a):
//   -1            background
//   -(l) - 2      foreground, not the root of its tile-local component; l is the
//                 tile-local raster index (ly * 64 + lx) of that root.  Written
//                 once, never changed again.
//   q >= 0        p is a tile root (the minimum raster index of its component
//                 within the tile); q <= p is its parent among the tile roots of
//                 the frame, q == p while it is a root.
// Only tile-root entries take part in the global union-find, so the later
// passes still know every pixel's tile-local component and can reduce per tile.
//
//   (a) inst_tile_kernel     tile-local labelling in LDS: row runs from the
//                            wave's ballot, then LDS atomicMin unions with the row
//                            above, then every pixel finds its local root.
//   (b) inst_merge_kernel    one thread per pixel pair position on a tile edge:
//                            union of the two tile roots with atomicMin on the
//                            global parent array; monotone path compression.
//   (c)+(d) inst_resolve_kernel  every tile root resolves its frame root and
//                            stores it (flatten: a pixel then reaches its root in
//                            two hops, tile root -> root); pixel counts per tile
//                            root in LDS, one global atomicAdd per tile root into
//                            area[root].
//   (e) inst_rank_*          exclusive prefix sum of "root and area >= min_area"
//                            in raster order: block counts, scan of the block
//                            counts per frame, ranks.  Ballots and shuffles only.
//   (f) inst_relabel_kernel  labels[p] = rank of p's root; statistics reduced per
//                            tile root in LDS, then 7 global 64-bit atomics per
//                            tile root of an instance below the cap.
// fill_holes runs (a), (b) on the complement with 4-connectivity, flags the
// roots that own a frame-edge pixel (inst_edge_kernel) and writes mask | unflagged
// complement (inst_fill_kernel); the filled mask is then labelled as above.
//
// No block waits for another block anywhere: every find / union loop either
// returns or moves to a strictly smaller index, and kernel boundaries are the
// only ordering between passes.  During (b) other CUs rewrite the parent array,
// so it is read only with relaxed agent-scope atomic loads (global_load_dword
// sc1: served by L2, never by a CU's L1, which another CU's stores do not
// refresh) and written only with atomicMin.  A stale "is a root" answer is
// harmless: the atomicMin returns the true old value and the loop goes on from
// there.  After (b) the root of a component is its minimum flat index whatever
// the arrival order, so every output is bit-reproducible.
#include "../../include/unet_hip.h"
#include "common.h"
#include "kernels.h"

namespace unet {

namespace {

static_assert(kInstTH == UNET_INSTANCE_TILE_H && kInstTW == UNET_INSTANCE_TILE_W, "tile geometry of the header");

constexpr int TH = kInstTH, TW = kInstTW, TP = TH * TW;  // 32 x 64 = 2048 pixels per tile
constexpr int NT = 256;                                  // threads per block: 4 waves, 8 rounds over the tile
constexpr int RB = kInstRankBlock;                       // elements per block of the ranking passes
static_assert(TW == 64 && TP % NT == 0 && RB % NT == 0, "one wave per tile row");

__device__ __forceinline__ int ld_agent(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int ld_wg(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ---- (a) tile-local labelling ----------------------------------------------

__device__ __forceinline__ int lds_find(const int* L, int i) {
  for (;;) {
    const int v = ld_wg(L + i);
    if (v == i) return i;
    i = v;  // v < i: parents only decrease
  }
}
// every iteration returns or lowers max(a, b)
__device__ __forceinline__ void lds_unite(int* L, int a, int b) {
  a = lds_find(L, a);
  b = lds_find(L, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(L + a, b);
    if (old == a) break;
    a = old;
  }
}

struct TilePos {
  int n, y0, x0;
  size_t base;  // n * H * W
};
__device__ __forceinline__ TilePos tile_pos(int H, int W, int ntx) {
  TilePos t;
  t.n = blockIdx.y;
  t.y0 = (int)(blockIdx.x / (unsigned)ntx) * TH;
  t.x0 = (int)(blockIdx.x % (unsigned)ntx) * TW;
  t.base = (size_t)t.n * (size_t)H * (size_t)W;
  return t;
}

template <int CONN>
__global__ void __launch_bounds__(NT) inst_tile_kernel(const uint8_t* __restrict__ src, int H, int W, int ntx,
                                                       int fgv, int invert, int* __restrict__ parent) {
  __shared__ int L[TP];
  __shared__ unsigned long long rowbits[TH];
  const TilePos t = tile_pos(H, W, ntx);
  const int lane = threadIdx.x & 63;
  const int x = t.x0 + lane;
  // row runs: a foreground pixel starts at the first pixel of its horizontal run
  for (int l = threadIdx.x; l < TP; l += NT) {
    const int ly = l >> 6, y = t.y0 + ly;
    bool fg = false;
    if (y < H && x < W) {
      const int v = src[t.base + (size_t)y * W + x];
      fg = (fgv < 0 ? v != 0 : v == fgv) != (invert != 0);
    }
    const unsigned long long m = __ballot(fg);
    const unsigned long long gaps = ~m & ((1ull << lane) - 1ull);
    const int start = gaps ? 64 - __clzll((long long)gaps) : 0;
    L[l] = fg ? (ly << 6) + start : -1;
    if (lane == 0) rowbits[ly] = m;
  }
  __syncthreads();
  // unions with the row above; a union that the left neighbour already makes is skipped
  for (int l = threadIdx.x; l < TP; l += NT) {
    const int ly = l >> 6;
    if (ly == 0) continue;
    const unsigned long long m = rowbits[ly], up = rowbits[ly - 1];
    if (!((m >> lane) & 1)) continue;
    const bool left = lane > 0 && ((m >> (lane - 1)) & 1);
    const bool u = (up >> lane) & 1;
    const bool ul = lane > 0 && ((up >> (lane - 1)) & 1);
    if (CONN == 1) {
      if (u && !(left && ul)) lds_unite(L, l, l - TW);
    } else {
      const bool ur = lane < 63 && ((up >> (lane + 1)) & 1);
      if (u) {
        if (!(left && ul)) lds_unite(L, l, l - TW);
      } else {
        if (ul && !left) lds_unite(L, l, l - TW - 1);
        if (ur) lds_unite(L, l, l - TW + 1);
      }
    }
  }
  __syncthreads();
  for (int l = threadIdx.x; l < TP; l += NT) {
    const int ly = l >> 6, y = t.y0 + ly;
    if (y >= H || x >= W) continue;
    int out = -1;
    if ((rowbits[ly] >> lane) & 1) {
      const int r = lds_find(L, l);
      out = r == l ? y * W + x : -r - 2;
    }
    parent[t.base + (size_t)y * W + x] = out;
  }
}

// ---- (b) border merge ------------------------------------------------------

// frame index of the tile root of foreground pixel (y, x) with parent entry v != -1
__device__ __forceinline__ int tile_root_of(int v, int y, int x, int W) {
  if (v >= 0) return y * W + x;
  const int l = -v - 2;
  return ((y & ~(TH - 1)) + (l >> 6)) * W + (x & ~(TW - 1)) + (l & 63);
}
// r is a tile root; its chain holds tile roots only and strictly decreases
__device__ __forceinline__ int find_root(const int* par, int r) {
  for (;;) {
    const int v = ld_agent(par + r);
    if (v == r) return r;
    r = v;
  }
}
// Pixels (ya, xa) and (yb, xb) of one frame, both inside it where `valid`.  Called
// by every lane of the wave.  A run of positions along a tile edge joins the same
// two tile roots: only the first lane of such a run makes the union.
__device__ __forceinline__ void unite_pixels(int* par, int W, bool valid, int ya, int xa, int yb, int xb) {
  int ta = -1, tb = -1;
  if (valid) {
    const int va = ld_agent(par + ya * W + xa);
    const int vb = va == -1 ? -1 : ld_agent(par + yb * W + xb);
    if (vb != -1) {
      ta = tile_root_of(va, ya, xa, W);
      tb = tile_root_of(vb, yb, xb, W);
    }
  }
  const int pa = __shfl_up(ta, 1, 64), pb = __shfl_up(tb, 1, 64);
  if (ta < 0 || ((threadIdx.x & 63) != 0 && pa == ta && pb == tb)) return;
  int a = find_root(par, ta), b = find_root(par, tb);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(par + a, b);
    if (old == a) { a = b; break; }
    a = old;  // old < a: every iteration returns or lowers max(a, b)
  }
  // monotone path compression: a is an ancestor of both tile roots
  if (ta != a) atomicMin(par + ta, a);
  if (tb != a) atomicMin(par + tb, a);
}

struct EdgePair {
  int ya, xa, yb, xb;
  bool ok;
};

// grid.x covers the (nty - 1) * W positions on horizontal tile edges, then the
// (ntx - 1) * H positions on vertical ones.  4-connectivity: the pair across the
// edge; 8-connectivity: also the two diagonal pairs across it.
__global__ void __launch_bounds__(NT) inst_merge_kernel(int* __restrict__ parent, int H, int W, int ntx, int nty,
                                                        int conn) {
  int* par = parent + (size_t)blockIdx.y * (size_t)H * (size_t)W;
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  const long long nh = (long long)(nty - 1) * W;
  const long long j = i - nh;
  // every lane makes the same calls (unite_pixels shuffles); a position off the grid has no pair
  EdgePair p0 = {0, 0, 0, 0, false}, p1 = p0, p2 = p0;
  if (i < nh) {
    const int e = (int)(i / W), x = (int)(i % W);
    const int yt = e * TH + TH - 1, yb = yt + 1;  // yb <= (nty - 1) * TH < H
    p0 = {yt, x, yb, x, true};
    p1 = {yt, x, yb, x - 1, x > 0};
    p2 = {yt, x, yb, x + 1, x + 1 < W};
  } else if (j < (long long)(ntx - 1) * H) {
    const int e = (int)(j / H), y = (int)(j % H);
    const int xl = e * TW + TW - 1, xr = xl + 1;  // xr <= (ntx - 1) * TW < W
    p0 = {y, xl, y, xr, true};
    p1 = {y, xl, y + 1, xr, y + 1 < H};
    p2 = {y, xr, y + 1, xl, y + 1 < H};
  }
  unite_pixels(par, W, p0.ok, p0.ya, p0.xa, p0.yb, p0.xb);
  if (conn == 2) {
    unite_pixels(par, W, p1.ok, p1.ya, p1.xa, p1.yb, p1.xb);
    unite_pixels(par, W, p2.ok, p2.ya, p2.xa, p2.yb, p2.xb);
  }
}

// ---- (c) + (d) flatten the tile roots, per-component area --------------------

// tile-local index of the tile root of the pixel at tile-local l with entry v != -1
__device__ __forceinline__ int local_root(int v, int l) { return v >= 0 ? l : -v - 2; }

__global__ void __launch_bounds__(NT) inst_resolve_kernel(int* __restrict__ parent, int H, int W, int ntx,
                                                          int* __restrict__ area) {
  __shared__ int cnt[TP];
  const TilePos t = tile_pos(H, W, ntx);
  int* par = parent + t.base;
  const int lane = threadIdx.x & 63;
  const int x = t.x0 + lane;
  for (int l = threadIdx.x; l < TP; l += NT) cnt[l] = 0;
  __syncthreads();
  for (int l = threadIdx.x; l < TP; l += NT) {
    const int y = t.y0 + (l >> 6);
    int v = -1;
    if (y < H && x < W) v = par[y * W + x];
    const bool fg = v != -1;
    const int r = fg ? local_root(v, l) : 0;
    // one LDS add per wave where the whole row segment is one component
    const unsigned long long m = __ballot(fg);
    if (m) {
      const int first = __ffsll((long long)m) - 1;
      const int r0 = __shfl(r, first, 64);
      if (__all(!fg || r == r0)) {
        if (lane == first) atomicAdd(&cnt[r0], (int)__popcll(m));
      } else if (fg) {
        atomicAdd(&cnt[r], 1);
      }
    }
  }
  __syncthreads();
  for (int l = threadIdx.x; l < TP; l += NT) {
    const int c = cnt[l];
    if (c == 0) continue;  // c > 0: l is a tile root inside the frame
    const int p = (t.y0 + (l >> 6)) * W + x;
    const int g = find_root(par, p);
    // other blocks may read this entry in their own find: old and new value are both ancestors of p
    if (g != p) __hip_atomic_store(par + p, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicAdd(area + t.base + g, c);
  }
}

// ---- (e) ranking -----------------------------------------------------------

// area is non-zero exactly at the roots (zeroed, then one add per tile root into area[root])
__device__ __forceinline__ bool rank_flag(const int* area, int i, int min_area) {
  return area[i] >= (min_area > 1 ? min_area : 1);
}

// cnt[n][b] = number of kept roots in block b of frame n
__global__ void __launch_bounds__(NT) inst_rank_count_kernel(const int* __restrict__ area, int HW, int nb,
                                                             int min_area, int* __restrict__ part) {
  __shared__ int wsum[NT / 64];
  const size_t base = (size_t)blockIdx.y * (size_t)HW;
  const int i0 = blockIdx.x * RB;  // < HW < 2^31
  int c = 0;
  for (int k = 0; k < RB / NT; ++k) {
    const long long i = (long long)i0 + k * NT + threadIdx.x;
    const bool f = i < HW && rank_flag(area + base, (int)i, min_area);
    c += (int)__popcll(__ballot(f));  // wave-uniform
  }
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < NT / 64; ++w) s += wsum[w];
    part[(size_t)blockIdx.y * nb + blockIdx.x] = s;
  }
}

// one block per frame: part[n][*] -> exclusive prefix sums in place, counts[n] = total
__global__ void __launch_bounds__(NT) inst_rank_scan_kernel(int* __restrict__ part, int nb,
                                                            int* __restrict__ counts) {
  __shared__ int wsum[NT / 64];
  int* p = part + (size_t)blockIdx.x * nb;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int running = 0;
  for (int c0 = 0; c0 < nb; c0 += NT) {
    const int i = c0 + threadIdx.x;
    const int v = i < nb ? p[i] : 0;
    int s = v;  // inclusive scan within the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(s, o, 64);
      if (lane >= o) s += u;
    }
    if (lane == 63) wsum[w] = s;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) {
      const int ws = wsum[k];
      if (k < w) before += ws;
      total += ws;
    }
    if (i < nb) p[i] = running + before + s - v;
    running += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = running;
}

// area[i] <- rank (1-based id) of a kept root, 0 for everything else
__global__ void __launch_bounds__(NT) inst_rank_write_kernel(int* __restrict__ area, int HW, int nb, int min_area,
                                                             const int* __restrict__ part) {
  constexpr int R = RB / NT, NW = NT / 64;
  __shared__ int wsum[R * NW];
  const size_t base = (size_t)blockIdx.y * (size_t)HW;
  const int i0 = blockIdx.x * RB;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int within[R];
  bool flag[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const long long i = (long long)i0 + k * NT + threadIdx.x;
    flag[k] = i < HW && rank_flag(area + base, (int)i, min_area);
    const unsigned long long m = __ballot(flag[k]);
    within[k] = (int)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[k * NW + w] = (int)__popcll(m);
  }
  __syncthreads();
  const int off = part[(size_t)blockIdx.y * nb + blockIdx.x];
  int before = 0;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const long long i = (long long)i0 + k * NT + threadIdx.x;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) {
      if (ww == w && i < HW) area[base + i] = flag[k] ? off + before + within[k] + 1 : 0;
      before += wsum[k * NW + ww];
    }
  }
}

// ---- (f) relabel and statistics --------------------------------------------

// rows k < min(counts[n], max_inst): {0, 0, 0, H, W, 0, 0} (the neutral elements
// of add / min / max); every other row zero
__global__ void __launch_bounds__(NT) inst_stats_init_kernel(long long* __restrict__ stats,
                                                             const int* __restrict__ counts, int max_inst, int H,
                                                             int W) {
  const int k = blockIdx.x * NT + threadIdx.x;
  if (k >= max_inst) return;
  const int n = blockIdx.y;
  long long* row = stats + ((size_t)n * max_inst + k) * UNET_INSTANCE_STATS;
  const bool live = k < counts[n];
  row[0] = 0; row[1] = 0; row[2] = 0;
  row[3] = live ? H : 0;
  row[4] = live ? W : 0;
  row[5] = 0; row[6] = 0;
}

// sum of the positions of the set bits
__device__ __forceinline__ unsigned long long bit_position_sum(unsigned long long m) {
  return (unsigned long long)(__popcll(m & 0xAAAAAAAAAAAAAAAAull) + 2 * __popcll(m & 0xCCCCCCCCCCCCCCCCull) +
                              4 * __popcll(m & 0xF0F0F0F0F0F0F0F0ull) + 8 * __popcll(m & 0xFF00FF00FF00FF00ull) +
                              16 * __popcll(m & 0xFFFF0000FFFF0000ull) + 32 * __popcll(m & 0xFFFFFFFF00000000ull));
}

template <bool STATS>
__global__ void __launch_bounds__(NT) inst_relabel_kernel(const int* __restrict__ parent,
                                                          const int* __restrict__ rank, int H, int W, int ntx,
                                                          int max_inst, int* __restrict__ labels,
                                                          long long* __restrict__ stats) {
  constexpr int SN = STATS ? TP : 1;
  __shared__ int lid[TP];                  // instance id of the tile root at l
  __shared__ unsigned long long sums[SN];  // count << 40 | sum ly << 20 | sum lx (12 + 16 + 17 bits used)
  __shared__ unsigned long long cols[SN];  // occupied tile columns
  __shared__ unsigned rows[SN];            // occupied tile rows
  const TilePos t = tile_pos(H, W, ntx);
  const int* par = parent + t.base;
  const int* rk = rank + t.base;
  const int lane = threadIdx.x & 63;
  const int x = t.x0 + lane;
  int v[TP / NT];
#pragma unroll
  for (int k = 0; k < TP / NT; ++k) {
    const int l = k * NT + threadIdx.x;
    const int y = t.y0 + (l >> 6);
    v[k] = (y < H && x < W) ? par[y * W + x] : -1;
    lid[l] = v[k] >= 0 ? rk[v[k]] : 0;  // a tile root's entry is its frame root after (c)
    if (STATS) { sums[l] = 0; cols[l] = 0; rows[l] = 0; }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < TP / NT; ++k) {
    const int l = k * NT + threadIdx.x;
    const int ly = l >> 6, y = t.y0 + ly;  // wave-uniform: one wave per tile row
    const bool in = y < H && x < W;
    const bool fg = in && v[k] != -1;
    const int r = fg ? local_root(v[k], l) : 0;
    const int id = fg ? lid[r] : 0;
    if (STATS) {
      const bool st = id > 0 && id <= max_inst;
      const unsigned long long m = __ballot(st);
      if (m) {
        const int first = __ffsll((long long)m) - 1;
        const int r0 = __shfl(r, first, 64);
        if (__all(!st || r == r0)) {  // the row segment is one component: one lane adds for the wave
          if (lane == first) {
            const unsigned long long c = (unsigned long long)__popcll(m);
            atomicAdd(&sums[r0], (c << 40) | ((c * (unsigned long long)ly) << 20) | bit_position_sum(m));
            atomicOr(&cols[r0], m);
            atomicOr(&rows[r0], 1u << ly);
          }
        } else if (st) {
          atomicAdd(&sums[r], (1ull << 40) | ((unsigned long long)ly << 20) | (unsigned long long)lane);
          atomicOr(&cols[r], 1ull << lane);
          atomicOr(&rows[r], 1u << ly);
        }
      }
    }
    if (in) labels[t.base + (size_t)y * W + x] = id;
  }
  if (!STATS) return;
  __syncthreads();
  for (int l = threadIdx.x; l < TP; l += NT) {
    const unsigned long long s = sums[l];
    if (s == 0) continue;  // s != 0: l is a tile root of an instance below the cap
    const unsigned long long c = s >> 40, sy = (s >> 20) & 0xFFFFFull, sx = s & 0xFFFFFull;
    const unsigned long long cm = cols[l];
    const unsigned rm = rows[l];
    unsigned long long* row = reinterpret_cast<unsigned long long*>(stats) +
                              ((size_t)t.n * max_inst + (lid[l] - 1)) * UNET_INSTANCE_STATS;
    atomicAdd(row + 0, c);
    atomicAdd(row + 1, sy + c * (unsigned long long)t.y0);
    atomicAdd(row + 2, sx + c * (unsigned long long)t.x0);
    atomicMin(row + 3, (unsigned long long)(t.y0 + __ffs((int)rm) - 1));
    atomicMin(row + 4, (unsigned long long)(t.x0 + __ffsll((long long)cm) - 1));
    atomicMax(row + 5, (unsigned long long)(t.y0 + 32 - __clz((int)rm)));
    atomicMax(row + 6, (unsigned long long)(t.x0 + 64 - __clzll((long long)cm)));
  }
}

// ---- fill_holes --------------------------------------------------------------

// parent: (a), (b) of the complement.  One thread per frame-edge position (top
// row, bottom row, left column, right column); flag[root] = 1 where the
// complement component owns such a pixel.  A plain store of 1: a same-value race.
__global__ void __launch_bounds__(NT) inst_edge_kernel(const int* __restrict__ parent, int H, int W,
                                                       int* __restrict__ flag) {
  const size_t base = (size_t)blockIdx.y * (size_t)H * (size_t)W;
  const int* par = parent + base;
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= 2ll * W + 2ll * H) return;
  int y, x;
  if (i < W) { y = 0; x = (int)i; }
  else if (i < 2ll * W) { y = H - 1; x = (int)(i - W); }
  else if (i < 2ll * W + H) { y = (int)(i - 2ll * W); x = 0; }
  else { y = (int)(i - 2ll * W - H); x = W - 1; }
  const int v = par[y * W + x];
  if (v == -1) return;
  flag[base + find_root(par, tile_root_of(v, y, x, W))] = 1;
}

// filled = 1 where the mask is foreground (entry -1 of the complement's parent
// array) or the complement component touches no frame edge, else 0
__global__ void __launch_bounds__(NT) inst_fill_kernel(const int* __restrict__ parent, const int* __restrict__ flag,
                                                       int H, int W, int ntx, uint8_t* __restrict__ filled) {
  __shared__ int open[TP];  // per tile root: its component reaches the frame edge
  const TilePos t = tile_pos(H, W, ntx);
  const int* par = parent + t.base;
  const int lane = threadIdx.x & 63;
  const int x = t.x0 + lane;
  int v[TP / NT];
#pragma unroll
  for (int k = 0; k < TP / NT; ++k) {
    const int l = k * NT + threadIdx.x;
    const int y = t.y0 + (l >> 6);
    v[k] = (y < H && x < W) ? par[y * W + x] : -1;
    open[l] = v[k] >= 0 ? flag[t.base + find_root(par, v[k])] : 0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < TP / NT; ++k) {
    const int l = k * NT + threadIdx.x;
    const int y = t.y0 + (l >> 6);
    if (y >= H || x >= W) continue;
    filled[t.base + (size_t)y * W + x] = (v[k] == -1 || !open[local_root(v[k], l)]) ? 1 : 0;
  }
}

inline size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

int64_t instances_workspace_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0 || (int64_t)H * W >= kInstMaxHW) return 0;
  const size_t P = (size_t)N * H * W;
  const size_t nb = ((size_t)H * W + RB - 1) / RB;
  return (int64_t)(2 * a256(4 * P) + a256(4 * (size_t)N * nb) + a256(P));
}

hipError_t launch_label_instances(const InstArgs& a, hipStream_t st) {
  if (!a.mask || !a.labels || !a.counts || !a.workspace || a.N <= 0 || a.H <= 0 || a.W <= 0 ||
      (int64_t)a.H * a.W >= kInstMaxHW || a.fg_value < -1 || a.fg_value > 255 || (a.conn != 1 && a.conn != 2) ||
      a.min_area < 0 || a.max_inst < 1 || a.workspace_bytes < instances_workspace_bytes(a.N, a.H, a.W))
    return hipErrorInvalidValue;
  const int H = a.H, W = a.W, HW = H * W;
  const int ntx = (W + TW - 1) / TW, nty = (H + TH - 1) / TH;
  const int nb = (HW + RB - 1) / RB;
  const size_t P = (size_t)a.N * HW;
  char* ws = static_cast<char*>(a.workspace);
  int* parent = reinterpret_cast<int*>(ws);
  int* area = reinterpret_cast<int*>(ws + a256(4 * P));
  int* part = reinterpret_cast<int*>(ws + 2 * a256(4 * P));
  uint8_t* wfilled = reinterpret_cast<uint8_t*>(ws + 2 * a256(4 * P) + a256(4 * (size_t)a.N * nb));
  const long long edges = (long long)(nty - 1) * W + (long long)(ntx - 1) * H;
  hipError_t e;
  // frames go on grid.y (<= 65535 per launch)
  for (int n0 = 0; n0 < a.N; n0 += 65535) {
    const unsigned nn = (unsigned)(a.N - n0 < 65535 ? a.N - n0 : 65535);
    const size_t off = (size_t)n0 * HW;
    const dim3 tiles((unsigned)(ntx * nty), nn), blk(NT);
    const dim3 mgrid((unsigned)((edges + NT - 1) / NT), nn);
    const uint8_t* src = a.mask + off;
    int fgv = a.fg_value;
    if (a.fill_holes) {
      uint8_t* filled = (a.filled ? a.filled : wfilled) + off;
      inst_tile_kernel<1><<<tiles, blk, 0, st>>>(src, H, W, ntx, fgv, 1, parent + off);
      if (edges > 0) inst_merge_kernel<<<mgrid, blk, 0, st>>>(parent + off, H, W, ntx, nty, 1);
      if ((e = hipMemsetAsync(area + off, 0, (size_t)nn * HW * 4, st)) != hipSuccess) return e;
      inst_edge_kernel<<<dim3((unsigned)((2ll * W + 2ll * H + NT - 1) / NT), nn), blk, 0, st>>>(parent + off, H, W,
                                                                                                 area + off);
      inst_fill_kernel<<<tiles, blk, 0, st>>>(parent + off, area + off, H, W, ntx, filled);
      src = filled;
      fgv = -1;
    }
    if (a.conn == 1) inst_tile_kernel<1><<<tiles, blk, 0, st>>>(src, H, W, ntx, fgv, 0, parent + off);
    else inst_tile_kernel<2><<<tiles, blk, 0, st>>>(src, H, W, ntx, fgv, 0, parent + off);
    if (edges > 0) inst_merge_kernel<<<mgrid, blk, 0, st>>>(parent + off, H, W, ntx, nty, a.conn);
    if ((e = hipMemsetAsync(area + off, 0, (size_t)nn * HW * 4, st)) != hipSuccess) return e;
    inst_resolve_kernel<<<tiles, blk, 0, st>>>(parent + off, H, W, ntx, area + off);
    int* pt = part + (size_t)n0 * nb;
    inst_rank_count_kernel<<<dim3((unsigned)nb, nn), blk, 0, st>>>(area + off, HW, nb, a.min_area, pt);
    inst_rank_scan_kernel<<<dim3(nn), blk, 0, st>>>(pt, nb, a.counts + n0);
    inst_rank_write_kernel<<<dim3((unsigned)nb, nn), blk, 0, st>>>(area + off, HW, nb, a.min_area, pt);
    if (a.stats) {
      long long* stats = a.stats + (size_t)n0 * a.max_inst * UNET_INSTANCE_STATS;
      inst_stats_init_kernel<<<dim3((unsigned)((a.max_inst + NT - 1) / NT), nn), blk, 0, st>>>(
          stats, a.counts + n0, a.max_inst, H, W);
      inst_relabel_kernel<true><<<tiles, blk, 0, st>>>(parent + off, area + off, H, W, ntx, a.max_inst,
                                                        a.labels + off, stats);
    } else {
      inst_relabel_kernel<false><<<tiles, blk, 0, st>>>(parent + off, area + off, H, W, ntx, a.max_inst,
                                                         a.labels + off, nullptr);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace unet
