// Matching of two instance label maps (gfx950): the pair histogram of a ground
// truth and a predicted int32 label map, the area of every instance, the partner
// of highest IoU of every instance on both sides and, optionally, the list of
// overlapping pairs.  No reference counterpart; tests/match_ref.py builds the same
// tables from a dense numpy bincount.  The scores on top (DSB average precision,
// F1, panoptic quality, aggregated Jaccard index) are host arithmetic on these
// tables (match.py: instance_metrics).
//
// Ids are 0 (background) or 1..max_gt / 1..max_pred, both caps <= 65535; the key of
// a pixel is g << 16 | p, key 0 (background on both sides) is never stored and so
// marks an empty slot.  Tiles are kInstTH x kInstTW = 32 x 64 pixels (one wave =
// one tile row), one 256-thread block per tile, frames on grid.y, as in
// instances.hip.  All passes are ordinary launches on the caller's stream:
//
//   (0) match_init_kernel   the caller's workspace and status are uninitialised:
//                           pair table, areas, cursors and status <- 0, best-slot
//                           arrays <- -1.
//   (a) match_tile_kernel  keys of the tile; within a wave row only the first lane
//                           of a run of equal keys inserts, with the run length
//                           from the ballot of run heads.  Insert into an LDS table
//                           of kLdsSlots keys and counts (linear probing, atomicCAS
//                           claims a key, atomicAdd counts); a probe that has seen
//                           every LDS slot inserts into the global table instead.
//                           After the barrier one thread per occupied LDS slot
//                           inserts (key, count) into the frame's global table of
//                           `slots` entries (multiplicative hash, linear probing
//                           bounded by slots).  A probe that finds no room adds its
//                           count to status.dropped.
//   (b) match_area_kernel   one thread per global slot: integer atomicAdd of the
//                           count into gt_area[g] and pred_area[p] (the areas are
//                           the row and column sums of the histogram), and the
//                           number of slots with both ids nonzero into n_pairs.
//   (c) match_best_kernel   one thread per slot with both ids: raises best_of_gt[g]
//                           and best_of_pred[p] (slot indices, -1 = none) to this
//                           slot where its IoU is higher.  IoU c / u with u =
//                           area_g + area_p - c is compared as cA uB > cB uA in
//                           64 bits; equal IoU: the smaller partner id.
//   (d) match_write_kernel  one thread per id writes its row of the two tables and
//                           counts the present ids; with `pairs`, one thread per
//                           slot appends (g, p, c) through an atomic cursor and one
//                           thread per row from n_pairs on zeroes it.
//
// No block or thread waits for another.  The probes of (a) are bounded by the table
// sizes.  The loop of (c) retries only after its compare-and-swap lost against one
// that succeeded, and every successful one replaces the entry by a strictly better
// slot of a total order (IoU, then partner id; a slot is better than -1), so the
// entry can change at most as often as there are slots and ends as the maximum,
// whatever the timing.  `better` reads only what (a) and (b) finished before the
// launch.  Counts and areas are integer sums: every output is bit-reproducible
// (the order of the pairs rows aside, which match.py sorts).
//
// During (a) other CUs write the global keys, and during (c) the best-slot arrays:
// those are read with relaxed agent-scope atomic loads and written with atomics
// only, as the parent array of instances.hip.
#include "../../include/unet_hip.h"
#include "common.h"
#include "kernels.h"

namespace unet {

namespace {

constexpr int TH = kInstTH, TW = kInstTW, TP = TH * TW;  // 32 x 64 = 2048 pixels per tile
constexpr int NT = 256;                                  // threads per block: 4 waves, 8 rounds over the tile
constexpr int LS = kMatchLdsSlots;                       // slots of the LDS table of a tile
constexpr int LSB = 9;
static_assert(TW == 64 && TP % NT == 0, "one wave per tile row");
static_assert(LS == 1 << LSB && LS % NT == 0, "LDS table: a power of two, whole rounds of the block");
static_assert(UNET_MATCH_COLS == 4 && UNET_MATCH_STATUS == 5, "table layout of the header");

enum { ST_NGT = 0, ST_NPRED = 1, ST_NPAIRS = 2, ST_DROPPED = 3, ST_OOR = 4 };

__device__ __forceinline__ unsigned ld_agent(const unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int ld_agent(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned ld_wg(const unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Knuth's multiplicative hash: the top `bits` bits of key * 2^32 / phi
__device__ __forceinline__ unsigned hash_bits(unsigned key, int bits) { return (key * 2654435761u) >> (32 - bits); }

struct Table {
  unsigned* keys;  // [slots], 0 = empty
  int* counts;     // [slots]
  int slots, bits; // slots = 1 << bits
};

// At most `slots` probes.  false: no room, nothing added.
__device__ __forceinline__ bool global_insert(const Table& t, unsigned key, int c) {
  unsigned s = hash_bits(key, t.bits);
  for (int i = 0; i < t.slots; ++i) {
    unsigned old = ld_agent(t.keys + s);
    if (old == 0) old = atomicCAS(t.keys + s, 0u, key);
    if (old == 0 || old == key) {
      atomicAdd(t.counts + s, c);
      return true;
    }
    s = (s + 1) & (unsigned)(t.slots - 1);
  }
  return false;
}

__device__ __forceinline__ void global_insert_or_drop(const Table& t, unsigned key, int c,
                                                      unsigned long long* status) {
  if (!global_insert(t, key, c)) atomicAdd(status + ST_DROPPED, (unsigned long long)c);
}

// At most LS probes.  false: every LDS slot holds another key.
__device__ __forceinline__ bool lds_insert(unsigned* K, int* C, unsigned key, int c) {
  unsigned s = hash_bits(key, LSB);
  for (int i = 0; i < LS; ++i) {
    unsigned old = ld_wg(K + s);
    if (old == 0) old = atomicCAS(K + s, 0u, key);
    if (old == 0 || old == key) {
      atomicAdd(C + s, c);
      return true;
    }
    s = (s + 1) & (unsigned)(LS - 1);
  }
  return false;
}

// ---- initialisation ------------------------------------------------------------

// The caller's workspace and status are uninitialised.  32-bit words [0, nzero) of
// the workspace <- 0 (pair table, areas, cursors), [nzero, nall) <- -1 (best-slot
// arrays), status <- 0.  A kernel, not hipMemsetAsync: a captured call is then a
// chain of kernel nodes only.
__global__ void __launch_bounds__(NT) match_init_kernel(unsigned* __restrict__ ws, size_t nzero, size_t nall,
                                                        unsigned long long* __restrict__ status, size_t nstatus) {
  const size_t stride = (size_t)gridDim.x * NT;
  const size_t i0 = (size_t)blockIdx.x * NT + threadIdx.x;
  for (size_t i = i0; i < nall; i += stride) ws[i] = i < nzero ? 0u : 0xFFFFFFFFu;
  for (size_t i = i0; i < nstatus; i += stride) status[i] = 0;
}

// ---- (a) pair histogram ------------------------------------------------------

__global__ void __launch_bounds__(NT) match_tile_kernel(const int* __restrict__ gt, const int* __restrict__ pred,
                                                        int H, int W, int ntx, int max_gt, int max_pred,
                                                        unsigned* __restrict__ keys, int* __restrict__ counts,
                                                        int slots, int bits, unsigned long long* __restrict__ status) {
  __shared__ unsigned K[LS];
  __shared__ int C[LS];
  const int n = blockIdx.y;
  const int y0 = (int)(blockIdx.x / (unsigned)ntx) * TH;
  const int x0 = (int)(blockIdx.x % (unsigned)ntx) * TW;
  const size_t base = (size_t)n * (size_t)H * (size_t)W;
  const Table tab = {keys + (size_t)n * slots, counts + (size_t)n * slots, slots, bits};
  unsigned long long* st = status + (size_t)n * UNET_MATCH_STATUS;
  const int lane = threadIdx.x & 63;
  const int x = x0 + lane;
  for (int s = threadIdx.x; s < LS; s += NT) { K[s] = 0; C[s] = 0; }
  __syncthreads();
  for (int l = threadIdx.x; l < TP; l += NT) {
    const int y = y0 + (l >> 6);  // wave-uniform: one wave per tile row
    unsigned key = 0;
    bool bad = false;
    if (y < H && x < W) {
      const size_t i = base + (size_t)y * W + x;
      const int g = gt[i], p = pred[i];
      bad = g < 0 || g > max_gt || p < 0 || p > max_pred;
      if (!bad) key = ((unsigned)g << 16) | (unsigned)p;
    }
    const unsigned long long oor = __ballot(bad);
    if (oor && lane == 0) atomicAdd(st + ST_OOR, (unsigned long long)__popcll(oor));
    // a run of equal keys along the row: its first lane inserts for all of them
    const unsigned left = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || key != left;
    const unsigned long long heads = __ballot(head);
    if (head && key != 0) {
      const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
      const int len = after ? __ffsll((long long)after) : 64 - lane;
      if (!lds_insert(K, C, key, len)) global_insert_or_drop(tab, key, len, st);
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < LS; s += NT) {
    const unsigned key = K[s];
    if (key != 0) global_insert_or_drop(tab, key, C[s], st);
  }
}

// ---- (b) areas -----------------------------------------------------------------

__global__ void __launch_bounds__(NT) match_area_kernel(const unsigned* __restrict__ keys,
                                                        const int* __restrict__ counts, int slots, int gstride,
                                                        int pstride, unsigned* __restrict__ gt_area,
                                                        unsigned* __restrict__ pred_area,
                                                        unsigned long long* __restrict__ status) {
  __shared__ int wsum[NT / 64];
  const int n = blockIdx.y;
  const int s = blockIdx.x * NT + threadIdx.x;
  bool pair = false;
  if (s < slots) {
    const unsigned key = keys[(size_t)n * slots + s];
    if (key != 0) {
      const unsigned c = (unsigned)counts[(size_t)n * slots + s];
      const unsigned g = key >> 16, p = key & 0xFFFFu;
      if (g) atomicAdd(gt_area + (size_t)n * gstride + g, c);
      if (p) atomicAdd(pred_area + (size_t)n * pstride + p, c);
      pair = g && p;
    }
  }
  const unsigned long long m = __ballot(pair);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (int)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < NT / 64; ++w) t += wsum[w];
    if (t) atomicAdd(status + (size_t)n * UNET_MATCH_STATUS + ST_NPAIRS, (unsigned long long)t);
  }
}

// ---- (c) best partner ------------------------------------------------------------

struct Cand {
  unsigned long long c, u;  // intersection < 2^31, union < 2^32: c * u < 2^63
  unsigned partner;
};
// total order: higher IoU, then the smaller partner id
__device__ __forceinline__ bool better(const Cand& a, const Cand& b) {
  const unsigned long long l = a.c * b.u, r = b.c * a.u;
  return l > r || (l == r && a.partner < b.partner);
}

// best[id] <- the best of itself and `mine`; every successful compare-and-swap
// strictly raises the entry, so a retry follows progress by another thread
template <bool GT_SIDE>
__device__ __forceinline__ void raise_best(int* best, int mine, const Cand& cm, const unsigned* keys,
                                           const int* counts, const unsigned* gt_area, const unsigned* pred_area) {
  for (;;) {
    const int cur = ld_agent(best);
    if (cur >= 0) {
      const unsigned k = keys[cur];
      const unsigned g = k >> 16, p = k & 0xFFFFu;
      Cand cc;
      cc.c = (unsigned)counts[cur];
      cc.u = (unsigned long long)gt_area[g] + pred_area[p] - cc.c;
      cc.partner = GT_SIDE ? p : g;
      if (!better(cm, cc)) break;
    }
    if (atomicCAS(best, cur, mine) == cur) break;
  }
}

__global__ void __launch_bounds__(NT) match_best_kernel(const unsigned* __restrict__ keys,
                                                        const int* __restrict__ counts, int slots, int gstride,
                                                        int pstride, const unsigned* __restrict__ gt_area,
                                                        const unsigned* __restrict__ pred_area,
                                                        int* __restrict__ best_gt, int* __restrict__ best_pred) {
  const int n = blockIdx.y;
  const int s = blockIdx.x * NT + threadIdx.x;
  if (s >= slots) return;
  keys += (size_t)n * slots;
  counts += (size_t)n * slots;
  gt_area += (size_t)n * gstride;
  pred_area += (size_t)n * pstride;
  const unsigned key = keys[s];
  const unsigned g = key >> 16, p = key & 0xFFFFu;
  if (!g || !p) return;
  Cand cm;
  cm.c = (unsigned)counts[s];
  cm.u = (unsigned long long)gt_area[g] + pred_area[p] - cm.c;
  cm.partner = p;
  raise_best<true>(best_gt + (size_t)n * gstride + g, s, cm, keys, counts, gt_area, pred_area);
  cm.partner = g;
  raise_best<false>(best_pred + (size_t)n * pstride + p, s, cm, keys, counts, gt_area, pred_area);
}

// ---- (d) tables --------------------------------------------------------------------

// row id - 1 of a table: area, partner, intersection, partner_area
__device__ __forceinline__ bool write_row(long long* row, unsigned area, int best, bool gt_side,
                                          const unsigned* keys, const int* counts, const unsigned* other_area) {
  long long partner = 0, inter = 0, parea = 0;
  if (best >= 0) {
    const unsigned k = keys[best];
    const unsigned o = gt_side ? (k & 0xFFFFu) : (k >> 16);
    partner = o;
    inter = counts[best];
    parea = other_area[o];
  }
  row[0] = area;
  row[1] = partner;
  row[2] = inter;
  row[3] = parea;
  return area > 0;
}

__global__ void __launch_bounds__(NT) match_write_kernel(const unsigned* __restrict__ keys,
                                                         const int* __restrict__ counts, int slots, int max_gt,
                                                         int max_pred, int max_pairs,
                                                         const unsigned* __restrict__ gt_area,
                                                         const unsigned* __restrict__ pred_area,
                                                         const int* __restrict__ best_gt,
                                                         const int* __restrict__ best_pred, int* __restrict__ cursor,
                                                         long long* __restrict__ gt_table,
                                                         long long* __restrict__ pred_table,
                                                         unsigned long long* __restrict__ status,
                                                         long long* __restrict__ pairs) {
  const int n = blockIdx.y;
  const int i = blockIdx.x * NT + threadIdx.x;
  const int lane = threadIdx.x & 63;
  keys += (size_t)n * slots;
  counts += (size_t)n * slots;
  gt_area += (size_t)n * (max_gt + 1);
  pred_area += (size_t)n * (max_pred + 1);
  unsigned long long* st = status + (size_t)n * UNET_MATCH_STATUS;
  bool present = false;
  if (i < max_gt)
    present = write_row(gt_table + ((size_t)n * max_gt + i) * UNET_MATCH_COLS, gt_area[i + 1],
                        best_gt[(size_t)n * (max_gt + 1) + i + 1], true, keys, counts, pred_area);
  unsigned long long m = __ballot(present);
  if (m && lane == 0) atomicAdd(st + ST_NGT, (unsigned long long)__popcll(m));
  present = false;
  if (i < max_pred)
    present = write_row(pred_table + ((size_t)n * max_pred + i) * UNET_MATCH_COLS, pred_area[i + 1],
                        best_pred[(size_t)n * (max_pred + 1) + i + 1], false, keys, counts, gt_area);
  m = __ballot(present);
  if (m && lane == 0) atomicAdd(st + ST_NPRED, (unsigned long long)__popcll(m));
  // n_pairs is final since (b): the rows from there on are zero, the ones before it come from the cursor
  if (pairs && i < max_pairs && (unsigned long long)i >= st[ST_NPAIRS]) {
    long long* row = pairs + ((size_t)n * max_pairs + i) * 3;
    row[0] = 0;
    row[1] = 0;
    row[2] = 0;
  }
  if (pairs && i < slots) {
    const unsigned key = keys[i];
    const unsigned g = key >> 16, p = key & 0xFFFFu;
    if (g && p) {
      const int k = atomicAdd(cursor + n, 1);  // < slots
      if (k < max_pairs) {
        long long* row = pairs + ((size_t)n * max_pairs + k) * 3;
        row[0] = g;
        row[1] = p;
        row[2] = counts[i];
      }
    }
  }
}

inline size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }

// the smallest power of two >= 2 max_pairs, as slots = 1 << bits
inline int slot_bits(int max_pairs) {
  int bits = 1;
  while (((int64_t)1 << bits) < 2 * (int64_t)max_pairs) ++bits;
  return bits;
}

// Workspace: match_init_kernel zeroes [keys | counts | gt_area | pred_area | cursor]
// and sets [best_gt | best_pred] to -1.  The pair table comes first: uint32
// keys [N][slots], then int32 counts [N][slots] (include/unet_hip.h).
struct Layout {
  size_t keys, counts, gt_area, pred_area, cursor, best_gt, best_pred, total;
};
inline Layout layout(int N, int max_gt, int max_pred, int max_pairs) {
  const size_t slots = (size_t)1 << slot_bits(max_pairs);
  const size_t G = (size_t)N * (max_gt + 1), P = (size_t)N * (max_pred + 1);
  Layout l;
  l.keys = 0;
  l.counts = l.keys + 4 * (size_t)N * slots;  // a multiple of 8: no padding between keys and counts
  l.gt_area = a256(l.counts + 4 * (size_t)N * slots);
  l.pred_area = a256(l.gt_area + 4 * G);
  l.cursor = a256(l.pred_area + 4 * P);
  l.best_gt = a256(l.cursor + 4 * (size_t)N);
  l.best_pred = a256(l.best_gt + 4 * G);
  l.total = a256(l.best_pred + 4 * P);
  return l;
}

inline bool caps_ok(int N, int max_gt, int max_pred, int max_pairs) {
  return N > 0 && max_gt >= 1 && max_gt <= kMatchMaxId && max_pred >= 1 && max_pred <= kMatchMaxId &&
         max_pairs >= 1 && max_pairs <= kMatchMaxPairs;
}

}  // namespace

int64_t match_workspace_bytes(int N, int max_gt, int max_pred, int max_pairs) {
  if (!caps_ok(N, max_gt, max_pred, max_pairs)) return 0;
  return (int64_t)layout(N, max_gt, max_pred, max_pairs).total;
}

hipError_t launch_match_instances(const MatchArgs& a, hipStream_t st) {
  if (!a.gt || !a.pred || !a.gt_table || !a.pred_table || !a.status || !a.workspace ||
      !caps_ok(a.N, a.max_gt, a.max_pred, a.max_pairs) || a.H <= 0 || a.W <= 0 ||
      (int64_t)a.H * a.W >= kInstMaxHW ||
      a.workspace_bytes < match_workspace_bytes(a.N, a.max_gt, a.max_pred, a.max_pairs))
    return hipErrorInvalidValue;
  const int H = a.H, W = a.W;
  const size_t HW = (size_t)H * W;
  const int ntx = (W + TW - 1) / TW, nty = (H + TH - 1) / TH;
  const int bits = slot_bits(a.max_pairs), slots = 1 << bits;
  const int gs = a.max_gt + 1, ps = a.max_pred + 1;
  const Layout l = layout(a.N, a.max_gt, a.max_pred, a.max_pairs);
  char* ws = static_cast<char*>(a.workspace);
  unsigned* keys = reinterpret_cast<unsigned*>(ws + l.keys);
  int* counts = reinterpret_cast<int*>(ws + l.counts);
  unsigned* gt_area = reinterpret_cast<unsigned*>(ws + l.gt_area);
  unsigned* pred_area = reinterpret_cast<unsigned*>(ws + l.pred_area);
  int* cursor = reinterpret_cast<int*>(ws + l.cursor);
  int* best_gt = reinterpret_cast<int*>(ws + l.best_gt);
  int* best_pred = reinterpret_cast<int*>(ws + l.best_pred);
  unsigned long long* status = reinterpret_cast<unsigned long long*>(a.status);
  hipError_t e;
  {
    const size_t words = l.total / 4;
    const size_t blocks = (words + NT - 1) / NT;
    match_init_kernel<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(NT), 0, st>>>(
        reinterpret_cast<unsigned*>(ws), l.best_gt / 4, words, status, (size_t)a.N * UNET_MATCH_STATUS);
  }
  int ids = a.max_gt > a.max_pred ? a.max_gt : a.max_pred;
  if (a.pairs && slots > ids) ids = slots;  // slots >= 2 max_pairs: the rows of pairs are covered as well
  // frames go on grid.y (<= 65535 per launch)
  for (int n0 = 0; n0 < a.N; n0 += 65535) {
    const unsigned nn = (unsigned)(a.N - n0 < 65535 ? a.N - n0 : 65535);
    const dim3 blk(NT), sgrid((unsigned)((slots + NT - 1) / NT), nn);
    unsigned* k = keys + (size_t)n0 * slots;
    int* c = counts + (size_t)n0 * slots;
    unsigned* ga = gt_area + (size_t)n0 * gs;
    unsigned* pa = pred_area + (size_t)n0 * ps;
    int* bg = best_gt + (size_t)n0 * gs;
    int* bp = best_pred + (size_t)n0 * ps;
    unsigned long long* s = status + (size_t)n0 * UNET_MATCH_STATUS;
    match_tile_kernel<<<dim3((unsigned)(ntx * nty), nn), blk, 0, st>>>(a.gt + (size_t)n0 * HW, a.pred + (size_t)n0 * HW,
                                                                       H, W, ntx, a.max_gt, a.max_pred, k, c, slots,
                                                                       bits, s);
    match_area_kernel<<<sgrid, blk, 0, st>>>(k, c, slots, gs, ps, ga, pa, s);
    match_best_kernel<<<sgrid, blk, 0, st>>>(k, c, slots, gs, ps, ga, pa, bg, bp);
    match_write_kernel<<<dim3((unsigned)((ids + NT - 1) / NT), nn), blk, 0, st>>>(
        k, c, slots, a.max_gt, a.max_pred, a.max_pairs, ga, pa, bg, bp, cursor + n0,
        a.gt_table + (size_t)n0 * a.max_gt * UNET_MATCH_COLS, a.pred_table + (size_t)n0 * a.max_pred * UNET_MATCH_COLS,
        s, a.pairs ? a.pairs + (size_t)n0 * a.max_pairs * 3 : nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace unet
