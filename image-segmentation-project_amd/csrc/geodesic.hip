// Geodesic growth of a label map and marker watershed by levels (gfx950):
// multi-source shortest paths restricted to an allowed set.  No reference
// counterpart; the definitions are in include/unet_hip.h and tests/geodesic_ref.py.
//
// State: one 8-byte key per pixel in the workspace, cost << 32 | id, compared as
// one unsigned number, so that "least cost, then smallest id" is one minimum.
//   id              a labelled pixel: cost 0, never changes
//   cost, id        a free pixel that a path of that cost from that id has reached
//   kUnreached      a free pixel no path has reached yet (cost 2^31 - 1)
//   kBlocked        a pixel that is neither labelled nor allowed (all ones)
// Costs stay below 2^30 (H W <= 2^28, a step costs at most 4), so a key with a
// cost below 2^31 - 1 is a reached one.
//
//   geo_init_kernel   keys from the labels (first level) or from the keys of the
//                     level before (reached -> cost 0), and the allowed set: within
//                     and, for the watershed, relief <= level, evaluated here.
//                     Marks the tiles dirty in which a pixel has just become free.
//   geo_pass_kernel   one pass = one launch: one 256-thread block per 32 x 64 tile,
//                     frames on grid.y.  A tile that is not dirty returns after
//                     reading its flag.  Otherwise the tile and a 1-pixel halo are
//                     staged in LDS (34 x 66 keys), the block relaxes in gather
//                     form (own key <- min(own key, neighbour key + step)) until
//                     __syncthreads_or says that nothing changed, writes the
//                     changed keys back, marks the neighbouring tiles whose halo
//                     it changed dirty for the next pass and raises the pass's
//                     "changed" word.
//   geo_final_kernel  labels and costs from the keys.
//   geo_hist_kernel   256-bin histogram of the relief under the mask: the levels.
//
// Ordering.  Kernel boundaries are the only ordering between blocks; no block
// waits for another block and nothing relies on another block's store becoming
// visible within a launch.  Keys only decrease, and every stored key is the cost
// of a real path with the id at its start, so a block that reads a neighbour's
// border key from before or after that neighbour's store of the same pass is
// correct either way: it sees a valid, possibly older, upper bound, and the
// neighbour marks it dirty for the next pass whenever it lowers such a key.  A
// tile that is not dirty is at its fixed point for its present halo, so a pass
// that marks no tile has reached the fixed point of the whole frame, which is
// unique.  The halo keys are the only words read while another block may write
// them: they are read with relaxed agent-scope 8-byte atomic loads and every key
// is stored with a relaxed agent-scope 8-byte atomic store (chosen over ping-pong
// border rings: no second copy of the borders, no extra pass to exchange them; an
// 8-byte atomic access cannot tear, and such loads are served by L2, not by a
// CU's L1 that another CU's stores do not refresh).  The dirty flags are two
// arrays used in turn: a pass reads and clears its own flag in one and sets flags
// only in the other, with same-value stores of 1.
//
// Convergence is decided exactly: the host enqueues kGeoBatch passes, each with a
// "changed" word of its own, reads the words back on the caller's stream and
// stops when the last is 0 (the passes after a pass that changed nothing find no
// dirty tile and return at once).  These calls therefore synchronise with the
// host and cannot be captured into a graph.
//
// Integer arithmetic, one writer per key, a unique fixed point: the outputs are
// bit-reproducible.
#include "../../include/unet_hip.h"
#include "common.h"
#include "kernels.h"

namespace unet {

namespace {

typedef unsigned long long gkey_t;

constexpr int TH = kGeoTH, TW = kGeoTW, TP = TH * TW;  // 32 x 64 = 2048 pixels per tile
constexpr int NT = 256;                                // threads per block: 8 pixels each
constexpr int PW = TW + 2, PH = TH + 2;                // the tile with its halo
constexpr int HALO = 2 * PW + 2 * TH;                  // 196 halo cells
constexpr int PER = TP / NT;
static_assert(TW == 64 && TP % NT == 0 && HALO <= NT, "one wave per tile row, one thread per halo cell");

constexpr unsigned kInfCost = 0x7FFFFFFFu;
constexpr gkey_t kInfKey = (gkey_t)kInfCost << 32;  // keys below it are reached
constexpr gkey_t kUnreached = 0x7FFFFFFFFFFFFFFFull;
constexpr gkey_t kBlocked = ~0ull;

__device__ __forceinline__ gkey_t ld_agent(const gkey_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(gkey_t* p, gkey_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ gkey_t ld_wg(const gkey_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void st_wg(gkey_t* p, gkey_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ bool geo_allowed(const uint8_t* within, int wv, const uint8_t* relief, int level,
                                            size_t i) {
  if (within) {
    const int v = within[i];
    if (!(wv < 0 ? v != 0 : v == wv)) return false;
  }
  return !relief || (int)relief[i] <= level;
}

// FIRST: ids from the labels; otherwise from the keys of the level before
template <bool FIRST>
__global__ void __launch_bounds__(NT) geo_init_kernel(const int* __restrict__ labels,
                                                      const uint8_t* __restrict__ within, int wv,
                                                      const uint8_t* __restrict__ relief, int level, int H, int W,
                                                      int ntx, gkey_t* __restrict__ keys, int* __restrict__ dirty_cur,
                                                      int* __restrict__ dirty_next) {
  const int y0 = (int)(blockIdx.x / (unsigned)ntx) * TH, x0 = (int)(blockIdx.x % (unsigned)ntx) * TW;
  const size_t base = (size_t)blockIdx.y * (size_t)H * (size_t)W;
  const int x = x0 + (threadIdx.x & 63);
  // Only a tile with a pixel that has just become free can change before a neighbour does: a tile
  // without one has no free pixel at all (FIRST), or is at the fixed point of the level before, whose
  // reached keys merely drop to cost 0.  Its neighbours wake it when they lower a key on its halo.
  int wake = 0;
  for (int l = threadIdx.x; l < TP; l += NT) {
    const int y = y0 + (l >> 6);
    if (y >= H || x >= W) continue;
    const size_t i = base + (size_t)y * W + x;
    unsigned id;
    gkey_t old = kBlocked;
    if (FIRST) {
      id = (unsigned)labels[i];
    } else {
      old = keys[i];
      id = old < kInfKey ? (unsigned)old : 0u;
    }
    const gkey_t k = id ? (gkey_t)id : (geo_allowed(within, wv, relief, level, i) ? kUnreached : kBlocked);
    if (FIRST || k != old) keys[i] = k;
    wake |= k == kUnreached && old == kBlocked;
  }
  wake = __syncthreads_or(wake);
  if (threadIdx.x == 0) {
    const size_t ti = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    dirty_cur[ti] = wake;
    dirty_next[ti] = 0;
  }
}

// CHAMFER: 8 neighbours at 3 (axial) and 4 (diagonal); otherwise 4 neighbours at 1
template <bool CHAMFER>
__global__ void __launch_bounds__(NT) geo_pass_kernel(gkey_t* __restrict__ keys, int H, int W, int ntx, int nty,
                                                      unsigned limit, int* __restrict__ dirty_cur,
                                                      int* __restrict__ dirty_next, int* __restrict__ changed) {
  __shared__ gkey_t L[PH * PW];
  __shared__ int dirs;
  const size_t ti = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (dirty_cur[ti] == 0) return;  // block-uniform; cleared only behind the barriers below
  const int ty = (int)(blockIdx.x / (unsigned)ntx), tx = (int)(blockIdx.x % (unsigned)ntx);
  const int y0 = ty * TH, x0 = tx * TW;
  gkey_t* kp = keys + (size_t)blockIdx.y * (size_t)H * (size_t)W;  // per-frame indices are int: H W <= 2^28
  const int lx = threadIdx.x & 63, x = x0 + lx;
  gkey_t mine[PER], orig[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int ly = k * (NT / 64) + (threadIdx.x >> 6), y = y0 + ly;
    gkey_t v = kBlocked;
    if (y < H && x < W) v = kp[y * W + x];  // written by this tile's blocks only: ordered by kernel boundaries
    mine[k] = orig[k] = v;
    L[(ly + 1) * PW + lx + 1] = v;
  }
  if (threadIdx.x < HALO) {
    const int h = threadIdx.x;
    int r, c;
    if (h < PW) { r = -1; c = h - 1; }
    else if (h < 2 * PW) { r = TH; c = h - PW - 1; }
    else if (h < 2 * PW + TH) { r = h - 2 * PW; c = -1; }
    else { r = h - 2 * PW - TH; c = TW; }
    const int y = y0 + r, xx = x0 + c;
    gkey_t v = kBlocked;
    if (y >= 0 && y < H && xx >= 0 && xx < W) v = ld_agent(kp + y * W + xx);
    L[(r + 1) * PW + c + 1] = v;
  }
  if (threadIdx.x == 0) dirs = 0;
  __syncthreads();
  constexpr gkey_t A = (gkey_t)(CHAMFER ? 3 : 1) << 32, D = (gkey_t)4 << 32;
  // Every thread lowers only its own cells and reads its neighbours' as they are (8-byte
  // atomic accesses: old or new, never torn; both are costs of real paths).  A round in
  // which no thread lowered a key read the final state throughout: the tile's fixed point.
  for (;;) {
    int ch = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      if (mine[k] == kBlocked || (mine[k] >> 32) == 0) continue;  // blocked or labelled
      const int c = (k * (NT / 64) + (threadIdx.x >> 6) + 1) * PW + lx + 1;
      gkey_t best = mine[k], n;
      n = ld_wg(L + c - 1);  if (n < kInfKey && n + A < best) best = n + A;
      n = ld_wg(L + c + 1);  if (n < kInfKey && n + A < best) best = n + A;
      n = ld_wg(L + c - PW); if (n < kInfKey && n + A < best) best = n + A;
      n = ld_wg(L + c + PW); if (n < kInfKey && n + A < best) best = n + A;
      if (CHAMFER) {
        n = ld_wg(L + c - PW - 1); if (n < kInfKey && n + D < best) best = n + D;
        n = ld_wg(L + c - PW + 1); if (n < kInfKey && n + D < best) best = n + D;
        n = ld_wg(L + c + PW - 1); if (n < kInfKey && n + D < best) best = n + D;
        n = ld_wg(L + c + PW + 1); if (n < kInfKey && n + D < best) best = n + D;
      }
      // the least candidate has the least cost: beyond the limit, so is every other
      if (best < mine[k] && (unsigned)(best >> 32) <= limit) {
        mine[k] = best;
        st_wg(L + c, best);
        ch = 1;
      }
    }
    if (!__syncthreads_or(ch)) break;
  }
  // directions, bit j of: N, S, W, E, NW, NE, SW, SE
  int d = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (mine[k] == orig[k]) continue;
    const int ly = k * (NT / 64) + (threadIdx.x >> 6);
    st_agent(kp + (y0 + ly) * W + x, mine[k]);  // a changed key lies inside the frame
    const int n = ly == 0, s = ly == TH - 1, w = lx == 0, e = lx == TW - 1;
    d |= n | s << 1 | w << 2 | e << 3 | (n & w) << 4 | (n & e) << 5 | (s & w) << 6 | (s & e) << 7;
  }
  if (d) atomicOr(&dirs, d);
  __syncthreads();
  if (threadIdx.x == 0) dirty_cur[ti] = 0;
  if (threadIdx.x < 8 && ((dirs >> threadIdx.x) & 1)) {
    const int dy[8] = {-1, 1, 0, 0, -1, -1, 1, 1}, dx[8] = {0, 0, -1, 1, -1, 1, -1, 1};
    const int ny = ty + dy[threadIdx.x], nx = tx + dx[threadIdx.x];
    if (ny >= 0 && ny < nty && nx >= 0 && nx < ntx) {
      __hip_atomic_store(dirty_next + (size_t)blockIdx.y * gridDim.x + ny * ntx + nx, 1, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(changed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// labels: the id of a reached key, else 0; cost: its cost, else -1
__global__ void __launch_bounds__(NT) geo_final_kernel(const gkey_t* __restrict__ keys, size_t P,
                                                       int* __restrict__ labels, int* __restrict__ cost) {
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < P; i += (size_t)gridDim.x * NT) {
    const gkey_t k = keys[i];
    const bool reached = k < kInfKey;
    labels[i] = reached ? (int)(unsigned)k : 0;
    if (cost) cost[i] = reached ? (int)(k >> 32) : -1;
  }
}

// hist[v] += number of pixels under the mask with relief v (all frames together)
__global__ void __launch_bounds__(NT) geo_hist_kernel(const uint8_t* __restrict__ relief,
                                                      const uint8_t* __restrict__ mask, int mv, size_t P,
                                                      int* __restrict__ hist) {
  __shared__ int h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < P; i += (size_t)gridDim.x * NT)
    if (geo_allowed(mask, mv, nullptr, 0, i)) atomicOr(&h[relief[i]], 1);
  __syncthreads();
  if (h[threadIdx.x]) atomicOr(&hist[threadIdx.x], 1);
}
static_assert(NT == 256, "one thread per histogram bin");

inline size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }

thread_local GeoCounts g_counts = {0, 0, 0};

struct GeoPlan {
  int N, H, W, ntx, nty;
  gkey_t* keys;
  int* dirty[2];
  int* changed;  // kGeoBatch words
  int* hist;     // 256 words
  int cur;       // which dirty array the next pass reads
};

inline unsigned flat_blocks(size_t P) {
  const size_t b = (P + (size_t)NT * 8 - 1) / ((size_t)NT * 8);
  return (unsigned)(b < 16384 ? b : 16384);
}

hipError_t geo_init(GeoPlan& p, bool first, const int* labels, const uint8_t* within, int wv, const uint8_t* relief,
                    int level, hipStream_t st) {
  const size_t HW = (size_t)p.H * p.W, nt = (size_t)p.ntx * p.nty;
  for (int n0 = 0; n0 < p.N; n0 += 65535) {  // frames go on grid.y
    const unsigned nn = (unsigned)(p.N - n0 < 65535 ? p.N - n0 : 65535);
    const size_t off = (size_t)n0 * HW;
    const dim3 grid((unsigned)nt, nn), blk(NT);
    const uint8_t* w = within ? within + off : nullptr;
    const uint8_t* r = relief ? relief + off : nullptr;
    int* dc = p.dirty[p.cur] + n0 * nt;
    int* dn = p.dirty[p.cur ^ 1] + n0 * nt;
    if (first) geo_init_kernel<true><<<grid, blk, 0, st>>>(labels + off, w, wv, r, level, p.H, p.W, p.ntx, p.keys + off, dc, dn);
    else geo_init_kernel<false><<<grid, blk, 0, st>>>(nullptr, w, wv, r, level, p.H, p.W, p.ntx, p.keys + off, dc, dn);
  }
  return hipGetLastError();
}

// passes until one changes nothing; the only place that waits for the stream
hipError_t geo_converge(GeoPlan& p, int metric, unsigned limit, hipStream_t st) {
  const size_t HW = (size_t)p.H * p.W, nt = (size_t)p.ntx * p.nty;
  hipError_t e;
  int host[kGeoBatch];
  for (;;) {
    if ((e = hipMemsetAsync(p.changed, 0, sizeof(int) * kGeoBatch, st)) != hipSuccess) return e;
    for (int b = 0; b < kGeoBatch; ++b) {
      for (int n0 = 0; n0 < p.N; n0 += 65535) {
        const unsigned nn = (unsigned)(p.N - n0 < 65535 ? p.N - n0 : 65535);
        const dim3 grid((unsigned)nt, nn), blk(NT);
        gkey_t* k = p.keys + (size_t)n0 * HW;
        int* dc = p.dirty[p.cur] + n0 * nt;
        int* dn = p.dirty[p.cur ^ 1] + n0 * nt;
        if (metric) geo_pass_kernel<true><<<grid, blk, 0, st>>>(k, p.H, p.W, p.ntx, p.nty, limit, dc, dn, p.changed + b);
        else geo_pass_kernel<false><<<grid, blk, 0, st>>>(k, p.H, p.W, p.ntx, p.nty, limit, dc, dn, p.changed + b);
      }
      p.cur ^= 1;
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(host, p.changed, sizeof(int) * kGeoBatch, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    g_counts.readbacks += 1;
    g_counts.passes += kGeoBatch;
    for (int b = 0; b < kGeoBatch; ++b) g_counts.changing += host[b] != 0;
    if (host[kGeoBatch - 1] == 0) return hipSuccess;
  }
}

}  // namespace

int64_t geodesic_workspace_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0 || H > kGeoMaxDim || W > kGeoMaxDim || (int64_t)H * W > kGeoMaxHW) return 0;
  const size_t P = (size_t)N * H * W;
  const size_t nt = (size_t)N * ((H + TH - 1) / TH) * ((W + TW - 1) / TW);
  return (int64_t)(a256(8 * P) + 2 * a256(4 * nt) + a256(4 * (kGeoBatch + 256)));
}

GeoCounts geodesic_last_counts() { return g_counts; }

hipError_t launch_geodesic(const GeoArgs& a, hipStream_t st) {
  if (!a.labels || !a.out || a.out == a.labels || !a.workspace || (a.metric != 0 && a.metric != 1) ||
      a.within_value < -1 || a.within_value > 255 || (a.relief && a.cost) ||
      geodesic_workspace_bytes(a.N, a.H, a.W) == 0 || a.workspace_bytes < geodesic_workspace_bytes(a.N, a.H, a.W))
    return hipErrorInvalidValue;
  g_counts = {0, 0, 0};
  GeoPlan p;
  p.N = a.N; p.H = a.H; p.W = a.W;
  p.ntx = (a.W + TW - 1) / TW; p.nty = (a.H + TH - 1) / TH;
  const size_t P = (size_t)a.N * a.H * a.W, nt = (size_t)a.N * p.ntx * p.nty;
  char* ws = static_cast<char*>(a.workspace);
  p.keys = reinterpret_cast<gkey_t*>(ws);
  p.dirty[0] = reinterpret_cast<int*>(ws + a256(8 * P));
  p.dirty[1] = reinterpret_cast<int*>(ws + a256(8 * P) + a256(4 * nt));
  p.changed = reinterpret_cast<int*>(ws + a256(8 * P) + 2 * a256(4 * nt));
  p.hist = p.changed + kGeoBatch;
  p.cur = 0;
  // a cost never reaches 2^30: a larger limit is no limit
  const unsigned limit = a.max_cost < 0 || a.max_cost >= kInfCost ? kInfCost - 1 : (unsigned)a.max_cost;
  hipError_t e;
  if (!a.relief) {
    if ((e = geo_init(p, true, a.labels, a.within, a.within_value, nullptr, 0, st)) != hipSuccess) return e;
    if ((e = geo_converge(p, a.metric, limit, st)) != hipSuccess) return e;
  } else {
    int hist[256];
    if ((e = hipMemsetAsync(p.hist, 0, sizeof(hist), st)) != hipSuccess) return e;
    geo_hist_kernel<<<flat_blocks(P), NT, 0, st>>>(a.relief, a.within, a.within_value, P, p.hist);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(hist, p.hist, sizeof(hist), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    g_counts.readbacks += 1;
    bool first = true;
    for (int level = 0; level < 256; ++level) {
      if (!hist[level]) continue;  // growth into the same allowed set again changes nothing
      if ((e = geo_init(p, first, a.labels, a.within, a.within_value, a.relief, level, st)) != hipSuccess) return e;
      first = false;
      if ((e = geo_converge(p, a.metric, limit, st)) != hipSuccess) return e;
    }
    // nothing under the mask: the markers alone
    if (first && (e = geo_init(p, true, a.labels, a.within, a.within_value, a.relief, -1, st)) != hipSuccess) return e;
  }
  geo_final_kernel<<<flat_blocks(P), NT, 0, st>>>(p.keys, P, a.out, a.cost);
  return hipGetLastError();
}

}  // namespace unet
