// Measuring the instances of an int32 label map (gfx950): per instance the area,
// the coordinate sums up to second order, the bounding box, the crack-length
// perimeter with its part on the frame's border and its part in contact with
// another instance and, with an image, sum, sum of squares, minimum and maximum of
// up to four channels; and select_instances, which drops instances and renumbers
// the rest.  No reference counterpart; tests/measure_ref.py holds the definitions
// as numpy.
//
// Ids are 0 (background) or 1..max_inst (<= 65535); a pixel with another value
// belongs to no instance, is counted in status.out_of_range and is, as a
// neighbour, "another nonzero value".  Tiles are kInstTH x kInstTW = 32 x 64 pixels
// (a wave works on one tile row at a time), one 256-thread block per tile, frames
// on grid.y, as in instances.hip and match.hip.  All passes are ordinary launches
// on the caller's stream:
//
//   (0) measure_init_kernel    the caller's workspace and status are
//                              uninitialised: the accumulator rows [N][max_inst]
//                              [13 + 4 C] of 64-bit words in the workspace <- the
//                              neutral elements (0 for sums and maxima, H / W for
//                              the box's minima, all ones for the minima of the
//                              intensities), status <- 0.
//   (a) measure_tile_kernel    wave w of the block walks rows 8 w .. 8 w + 7 of the
//                              tile; it loads them, the rows above and below (10
//                              row loads for 8 rows), the two columns beside the
//                              tile and the image under its instances into
//                              registers before the first use.  Every lane counts the
//                              sides of its pixel that are edges, frame edges and
//                              contact edges; a segmented suffix reduction over the
//                              run of equal ids (shuffles, bounded by the ballot of
//                              run heads) brings the counts and the intensity sums,
//                              minima and maxima of the run to its first lane,
//                              which adds the closed forms of the coordinate sums
//                              and inserts: into the slot of its id in an LDS table
//                              of kMeasureLdsSlots keys (linear probing, atomicCAS
//                              claims a key, 64-bit LDS atomics on the columns),
//                              or, when the probe has seen every slot, straight
//                              into the accumulator row with global atomics.  After
//                              the barrier one thread per occupied slot and column
//                              issues the global 64-bit atomic.
//   (b) measure_finish_kernel  one thread per row: table and intensity rows from
//                              the accumulators (all zero where area == 0; the
//                              float minima and maxima back from their integer
//                              keys), n_present and max_id with one atomic per wave.
//
//   select_scan_kernel         one block per frame: exclusive prefix sum of keep
//                              (ballots within a wave, wave totals through LDS):
//                              new_ids and counts.
//   select_gather_kernel       per pixel new_ids[id - 1], 0 outside 1..M.
//
// No block or thread waits for another; the probes are bounded by the table size.
// Every integer output is a sum, minimum or maximum of integers through atomics
// and so independent of the order of arrival: bit-reproducible.  The minima and
// maxima of a float image go through a monotone integer key of the fp32 bits and
// are exact too; its sums are fp64 atomic adds and depend on the order in the last
// bits.  Per-frame indices are int32 (H W <= 2^28), every accumulator is 64-bit:
// sum_yy <= 2^28 * 2^30 and sum_sq of uint16 <= 2^28 * 2^32 stay below 2^63.
#include "../../include/unet_hip.h"
#include "common.h"
#include "kernels.h"

namespace unet {

namespace {

typedef unsigned long long u64;

constexpr int TH = kInstTH, TW = kInstTW;  // 32 x 64 pixels per tile
constexpr int NT = 256;                    // threads per block: 4 waves of 8 tile rows each
constexpr int RW = TH / (NT / 64);         // rows per wave
constexpr int LS = kMeasureLdsSlots, LSB = 6;
constexpr int MC = UNET_MEASURE_COLS, IC = UNET_MEASURE_ICOLS;
static_assert(TW == 64 && TH % (NT / 64) == 0, "a wave per tile row, whole rows per wave");
static_assert(LS == 1 << LSB, "LDS table: a power of two");
static_assert(MC == 13 && IC == 4 && UNET_MEASURE_STATUS == 3, "table layout of the header");
// C = 4: 64 slots * (13 + 16) columns * 8 bytes + keys = 14.8 KiB of LDS per block
static_assert(LS * ((MC + IC * kMeasureMaxChannels) * 8 + 4) * 2 <= 160 * 1024, "two blocks per CU");

enum { COL_AREA = 0, COL_SY, COL_SX, COL_Y0, COL_X0, COL_Y1, COL_X1, COL_SYY, COL_SXX, COL_SXY, COL_EDGES,
       COL_FRAME, COL_CONTACT };
enum { ST_PRESENT = 0, ST_MAXID = 1, ST_OOR = 2 };
enum { OP_ADD = 0, OP_MIN = 1, OP_MAX = 2, OP_FADD = 3 };

// what the accumulator column does with a contribution
template <bool FLT>
__device__ __forceinline__ int col_op(int col) {
  if (col < MC) return col == COL_Y0 || col == COL_X0 ? OP_MIN : (col == COL_Y1 || col == COL_X1 ? OP_MAX : OP_ADD);
  const int k = (col - MC) & 3;  // sum, sum_sq, min, max
  return k == 2 ? OP_MIN : (k == 3 ? OP_MAX : (FLT ? OP_FADD : OP_ADD));
}
__device__ __forceinline__ u64 col_neutral(int op, int col, int H, int W) {
  if (op != OP_MIN) return 0;  // +0.0 as a double as well
  return col == COL_Y0 ? (u64)H : (col == COL_X0 ? (u64)W : ~0ull);
}

// monotone key of a finite fp32: a < b <=> key(a) < key(b), with -0.0 below +0.0
__device__ __forceinline__ unsigned float_key(float v) {
  const unsigned b = __float_as_uint(v);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float key_float(unsigned k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

__device__ __forceinline__ int ld_wg(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the slot of `id` in the LDS table after at most LS probes; -1: every slot holds another id
__device__ __forceinline__ int lds_claim(int* K, int id) {
  unsigned s = ((unsigned)id * 2654435761u) >> (32 - LSB);
  for (int i = 0; i < LS; ++i) {
    int old = ld_wg(K + s);
    if (old == 0) old = atomicCAS(K + s, 0, id);
    if (old == 0 || old == id) return (int)s;
    s = (s + 1) & (unsigned)(LS - 1);
  }
  return -1;
}

// what a pixel of the image contributes: integers exactly, a float as fp64 and as its key
template <typename T>
struct Pix {
  typedef unsigned Sum;  // a run of 64 pixels: 64 * 65535 < 2^32
  typedef u64 Sq;
  static constexpr bool kFloat = false;
  static __device__ __forceinline__ Sum sum(T v) { return v; }
  static __device__ __forceinline__ Sq sq(T v) { return (u64)v * v; }
  static __device__ __forceinline__ unsigned key(T v) { return v; }
  static __device__ __forceinline__ u64 bits(Sum s) { return s; }
  static __device__ __forceinline__ u64 bits_sq(Sq s) { return s; }
};
template <>
struct Pix<float> {
  typedef double Sum;
  typedef double Sq;
  static constexpr bool kFloat = true;
  static __device__ __forceinline__ Sum sum(float v) { return (double)v; }
  static __device__ __forceinline__ Sq sq(float v) { return (double)v * (double)v; }  // exact: 48 bits
  static __device__ __forceinline__ unsigned key(float v) { return float_key(v); }
  static __device__ __forceinline__ u64 bits(Sum s) { return (u64)__double_as_longlong(s); }
  static __device__ __forceinline__ u64 bits_sq(Sq s) { return (u64)__double_as_longlong(s); }
};

// one contribution to one column; p is an LDS or a global address (the caller's
// branch decides, so each inlined copy has its own address space)
__device__ __forceinline__ void apply(u64* p, int op, u64 v) {
  if (op == OP_ADD) {
    if (v) atomicAdd(p, v);
  } else if (op == OP_MIN) {
    atomicMin(p, v);
  } else if (op == OP_MAX) {
    atomicMax(p, v);
  } else {
    const double d = __longlong_as_double((long long)v);
    if (d != 0.0) unsafeAtomicAdd(reinterpret_cast<double*>(p), d);
  }
}

// the run [x, x + c) of row y with its reduced edge counts (10-bit fields of e) and intensities
template <typename T, int C>
struct Run {
  int y, x, c;
  unsigned e;
  typename Pix<T>::Sum s[C > 0 ? C : 1];
  typename Pix<T>::Sq q[C > 0 ? C : 1];
  unsigned mn[C > 0 ? C : 1], mx[C > 0 ? C : 1];
};

template <typename T, int C>
__device__ __forceinline__ void insert_run(u64* row, const Run<T, C>& r) {
  const u64 c = (u64)r.c, x = (u64)r.x, y = (u64)r.y;
  const u64 tri = c * (c - 1) / 2;                      // 0 + 1 + ... + (c - 1)
  const u64 pyr = (c - 1) * c * (2 * c - 1) / 6;        // 0 + 1 + 4 + ... + (c - 1)^2
  const u64 sx = c * x + tri;
  apply(row + COL_AREA, OP_ADD, c);
  apply(row + COL_SY, OP_ADD, y * c);
  apply(row + COL_SX, OP_ADD, sx);
  apply(row + COL_Y0, OP_MIN, y);
  apply(row + COL_X0, OP_MIN, x);
  apply(row + COL_Y1, OP_MAX, y + 1);
  apply(row + COL_X1, OP_MAX, x + c);
  apply(row + COL_SYY, OP_ADD, y * y * c);
  apply(row + COL_SXX, OP_ADD, c * x * x + 2 * x * tri + pyr);
  apply(row + COL_SXY, OP_ADD, y * sx);
  apply(row + COL_EDGES, OP_ADD, r.e & 1023u);
  apply(row + COL_FRAME, OP_ADD, (r.e >> 10) & 1023u);
  apply(row + COL_CONTACT, OP_ADD, r.e >> 20);
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    u64* p = row + MC + IC * ch;
    apply(p + 0, Pix<T>::kFloat ? OP_FADD : OP_ADD, Pix<T>::bits(r.s[ch]));
    apply(p + 1, Pix<T>::kFloat ? OP_FADD : OP_ADD, Pix<T>::bits_sq(r.q[ch]));
    apply(p + 2, OP_MIN, r.mn[ch]);
    apply(p + 3, OP_MAX, r.mx[ch]);
  }
}

// ---- (0) initialisation ---------------------------------------------------------

__global__ void __launch_bounds__(NT) measure_init_kernel(u64* __restrict__ acc, size_t nwords, int NC, int H, int W,
                                                          u64* __restrict__ status, size_t nstatus) {
  const size_t stride = (size_t)gridDim.x * NT;
  const size_t i0 = (size_t)blockIdx.x * NT + threadIdx.x;
  for (size_t i = i0; i < nwords; i += stride) {
    const int col = (int)(i % (size_t)NC);
    acc[i] = col_neutral(col_op<false>(col), col, H, W);  // a float sum starts as +0.0: the same bits
  }
  for (size_t i = i0; i < nstatus; i += stride) status[i] = 0;
}

// ---- (a) the pixel pass -----------------------------------------------------------

template <typename T, int C>
__global__ void __launch_bounds__(NT) measure_tile_kernel(const int* __restrict__ labels, const T* __restrict__ image,
                                                          int H, int W, int ntx, int M, u64* __restrict__ acc,
                                                          u64* __restrict__ status) {
  constexpr int NC = MC + IC * C;
  constexpr bool FLT = Pix<T>::kFloat;
  __shared__ int K[LS];
  __shared__ u64 V[LS * NC];
  const int n = blockIdx.y;
  const int ty0 = (int)(blockIdx.x / (unsigned)ntx) * TH;
  const int x0 = (int)(blockIdx.x % (unsigned)ntx) * TW;
  const size_t HW = (size_t)H * (size_t)W;
  const int* L = labels + (size_t)n * HW;
  const T* I = C > 0 ? image + (size_t)n * C * HW : nullptr;
  u64* rows = acc + (size_t)n * M * NC;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int x = x0 + lane;
  for (int s = threadIdx.x; s < LS; s += NT) K[s] = 0;
  for (int i = threadIdx.x; i < LS * NC; i += NT) {
    const int col = i % NC;
    V[i] = col_neutral(col_op<false>(col), col, H, W);
  }
  __syncthreads();
  const int yb = ty0 + w * RW;
  const bool inx = x < W;
  // Every load of the wave before the first use, so that they are in flight together: its 8 rows with the
  // row above and the row below, the pixels beside the tile (lanes 0..7 hold x0 - 1 of the 8 rows, lanes
  // 8..15 hold x0 + 64) and the image under the valid pixels.  The loop below stays rolled and shifts
  // these registers by one row per turn: no index into them depends on r.
  int rv[RW + 2];
#pragma unroll
  for (int k = 0; k < RW + 2; ++k) {
    const int yy = yb + k - 1;
    rv[k] = (inx && yy >= 0 && yy < H) ? L[yy * W + x] : 0;
  }
  int sidev = 0;
  {
    const int yy = yb + (lane & (RW - 1)), xs = lane < RW ? x0 - 1 : x0 + TW;
    if (lane < 2 * RW && yy < H && xs >= 0 && xs < W) sidev = L[yy * W + xs];
  }
  T iv[RW][C > 0 ? C : 1];
#pragma unroll
  for (int k = 0; k < RW; ++k) {
    const bool ok = inx && yb + k < H && rv[k + 1] >= 1 && rv[k + 1] <= M;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) iv[k][ch] = ok ? I[(size_t)ch * HW + (size_t)((yb + k) * W + x)] : T(0);
  }
#pragma nounroll
  for (int r = 0; r < RW; ++r) {
    const int y = yb + r;  // wave-uniform
    if (y >= H) break;
    const int up = rv[0], cur = rv[1], down = rv[2];
    int left = __shfl_up(cur, 1, 64), right = __shfl_down(cur, 1, 64);
    const int lside = __shfl(sidev, r, 64), rside = __shfl(sidev, RW + r, 64);
    if (lane == 0) left = lside;
    if (lane == 63) right = rside;
    const bool valid = inx && cur >= 1 && cur <= M;
    const bool bad = inx && (cur < 0 || cur > M);
    const int key = valid ? cur : 0;
    const u64 oor = __ballot(bad);
    if (oor && lane == 0) atomicAdd(status + (size_t)n * UNET_MEASURE_STATUS + ST_OOR, (u64)__popcll(oor));
    // the four sides: outside the frame = edge + frame edge; another value = edge, nonzero = contact too
    unsigned e = 0;
    {
      const bool out4[4] = {y == 0, y == H - 1, x == 0, x == W - 1};
      const int nb4[4] = {up, down, left, right};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (out4[k]) e += 1u + (1u << 10);
        else if (nb4[k] != cur) e += 1u + (nb4[k] != 0 ? 1u << 20 : 0u);
      }
    }
    typename Pix<T>::Sum s[C > 0 ? C : 1];
    typename Pix<T>::Sq q[C > 0 ? C : 1];
    unsigned mn[C > 0 ? C : 1], mx[C > 0 ? C : 1];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      const T v = iv[0][ch];  // 0 under a pixel of no instance
      s[ch] = Pix<T>::sum(v);
      q[ch] = Pix<T>::sq(v);
      mn[ch] = mx[ch] = Pix<T>::key(v);
    }
    // runs of equal keys along the row; `last` is the last lane of this lane's run
    const int lkey = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || key != lkey;
    const u64 heads = __ballot(head);
    const u64 after = lane == 63 ? 0ull : heads >> (lane + 1);
    const int last = after ? lane + __ffsll((long long)after) - 1 : 63;
    // segmented suffix reduction: after the step of offset o a lane holds its run's lanes [lane, lane + 2 o)
    for (int o = 1; o < 64; o <<= 1) {
      const bool take = key != 0 && lane + o <= last;  // background reduces nothing
      if (!__any(take)) break;
      const unsigned te = __shfl_down(e, o, 64);
      if (take) e += te;
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        const typename Pix<T>::Sum ts = __shfl_down(s[ch], o, 64);
        const typename Pix<T>::Sq tq = __shfl_down(q[ch], o, 64);
        const unsigned tn = __shfl_down(mn[ch], o, 64), tx = __shfl_down(mx[ch], o, 64);
        if (take) {
          s[ch] += ts;
          q[ch] += tq;
          mn[ch] = tn < mn[ch] ? tn : mn[ch];
          mx[ch] = tx > mx[ch] ? tx : mx[ch];
        }
      }
    }
    if (head && key != 0) {
      Run<T, C> run;
      run.y = y;
      run.x = x;
      run.c = last - lane + 1;
      run.e = e;
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        run.s[ch] = s[ch];
        run.q[ch] = q[ch];
        run.mn[ch] = mn[ch];
        run.mx[ch] = mx[ch];
      }
      const int slot = lds_claim(K, key);
      if (slot >= 0) insert_run<T, C>(V + slot * NC, run);
      else insert_run<T, C>(rows + (size_t)(key - 1) * NC, run);  // the direct route
    }
#pragma unroll
    for (int k = 0; k < RW + 1; ++k) rv[k] = rv[k + 1];
#pragma unroll
    for (int k = 0; k + 1 < RW; ++k) {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) iv[k][ch] = iv[k + 1][ch];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < LS * NC; i += NT) {
    const int slot = i / NC, col = i % NC;
    const int id = K[slot];
    if (id != 0) apply(rows + (size_t)(id - 1) * NC + col, col_op<FLT>(col), V[i]);
  }
}

// ---- (b) tables -----------------------------------------------------------------

template <bool FLT>
__global__ void __launch_bounds__(NT) measure_finish_kernel(const u64* __restrict__ acc, int M, int C,
                                                            long long* __restrict__ table, void* __restrict__ intensity,
                                                            u64* __restrict__ status) {
  const int n = blockIdx.y;
  const int i = blockIdx.x * NT + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int NC = MC + IC * C;
  bool present = false;
  if (i < M) {
    const u64* a = acc + ((size_t)n * M + i) * NC;
    present = a[COL_AREA] != 0;
    long long* t = table + ((size_t)n * M + i) * MC;
    for (int col = 0; col < MC; ++col) t[col] = present ? (long long)a[col] : 0;
    for (int k = 0; k < IC * C; ++k) {
      const u64 v = a[MC + k];
      const size_t o = ((size_t)n * M + i) * (size_t)(IC * C) + k;
      if (FLT) {
        double d = 0.0;
        if (present) d = (k & 3) < 2 ? __longlong_as_double((long long)v) : (double)key_float((unsigned)v);
        static_cast<double*>(intensity)[o] = d;
      } else {
        static_cast<long long*>(intensity)[o] = present ? (long long)v : 0;
      }
    }
  }
  const u64 m = __ballot(present);
  if (m && lane == 0) {
    u64* st = status + (size_t)n * UNET_MEASURE_STATUS;
    atomicAdd(st + ST_PRESENT, (u64)__popcll(m));
    atomicMax(st + ST_MAXID, (u64)(i + 64 - __clzll((long long)m)));  // i is lane 0's row: the highest lane's id
  }
}

// ---- select_instances -------------------------------------------------------------

__global__ void __launch_bounds__(NT) select_scan_kernel(const uint8_t* __restrict__ keep, int M,
                                                         int* __restrict__ new_ids, int* __restrict__ counts) {
  __shared__ int wsum[NT / 64];
  const int n = blockIdx.x;
  const uint8_t* k = keep + (size_t)n * M;
  int* out = new_ids + (size_t)n * M;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int running = 0;
  for (int c0 = 0; c0 < M; c0 += NT) {
    const int i = c0 + threadIdx.x;
    const bool f = i < M && k[i] != 0;
    const u64 m = __ballot(f);
    const int within = (int)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[w] = (int)__popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int j = 0; j < NT / 64; ++j) {
      const int ws = wsum[j];
      if (j < w) before += ws;
      total += ws;
    }
    if (i < M) out[i] = f ? running + before + within + 1 : 0;
    running += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[n] = running;
}

// VEC: four pixels per thread as one 16-byte access (HW a multiple of 4, both maps 16-byte aligned)
template <bool VEC>
__global__ void __launch_bounds__(NT) select_gather_kernel(const int* __restrict__ labels, int HW, int M,
                                                           const int* __restrict__ new_ids, int* __restrict__ out) {
  const int n = blockIdx.y;
  const int* ids = new_ids + (size_t)n * M;
  const size_t base = (size_t)n * (size_t)HW;
  const int i = (blockIdx.x * NT + threadIdx.x) * (VEC ? 4 : 1);  // HW <= 2^28
  if (i >= HW) return;
  if (VEC) {
    const int4 v = *reinterpret_cast<const int4*>(labels + base + i);
    int4 o;
    o.x = (v.x >= 1 && v.x <= M) ? ids[v.x - 1] : 0;
    o.y = (v.y >= 1 && v.y <= M) ? ids[v.y - 1] : 0;
    o.z = (v.z >= 1 && v.z <= M) ? ids[v.z - 1] : 0;
    o.w = (v.w >= 1 && v.w <= M) ? ids[v.w - 1] : 0;
    *reinterpret_cast<int4*>(out + base + i) = o;
  } else {
    const int v = labels[base + i];
    out[base + i] = (v >= 1 && v <= M) ? ids[v - 1] : 0;
  }
}

inline size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }

inline bool shape_ok(int N, int H, int W) {
  return N > 0 && H > 0 && W > 0 && H <= kMeasureMaxDim && W <= kMeasureMaxDim && (int64_t)H * W <= kMeasureMaxHW;
}

template <typename T, int C>
void launch_tile(const MeasureArgs& a, int n0, unsigned nn, int ntx, int nty, u64* acc, u64* status, hipStream_t st) {
  const size_t HW = (size_t)a.H * a.W;
  constexpr int NC = MC + IC * C;
  measure_tile_kernel<T, C><<<dim3((unsigned)(ntx * nty), nn), dim3(NT), 0, st>>>(
      a.labels + (size_t)n0 * HW, C > 0 ? static_cast<const T*>(a.image) + (size_t)n0 * C * HW : nullptr, a.H, a.W, ntx,
      a.max_inst, acc + (size_t)n0 * a.max_inst * NC, status + (size_t)n0 * UNET_MEASURE_STATUS);
}

template <typename T>
void launch_tile_c(const MeasureArgs& a, int n0, unsigned nn, int ntx, int nty, u64* acc, u64* status,
                   hipStream_t st) {
  switch (a.channels) {
    case 1: launch_tile<T, 1>(a, n0, nn, ntx, nty, acc, status, st); break;
    case 2: launch_tile<T, 2>(a, n0, nn, ntx, nty, acc, status, st); break;
    case 3: launch_tile<T, 3>(a, n0, nn, ntx, nty, acc, status, st); break;
    default: launch_tile<T, 4>(a, n0, nn, ntx, nty, acc, status, st); break;
  }
}

}  // namespace

int64_t measure_workspace_bytes(int N, int H, int W, int max_inst, int channels) {
  if (!shape_ok(N, H, W) || max_inst < 1 || max_inst > kMeasureMaxId || channels < 0 ||
      channels > kMeasureMaxChannels)
    return 0;
  return (int64_t)a256((size_t)N * max_inst * (MC + IC * channels) * 8);
}

hipError_t launch_measure_instances(const MeasureArgs& a, hipStream_t st) {
  const int C = a.image ? a.channels : 0;
  if (!a.labels || !a.table || !a.status || !a.workspace || (a.image != nullptr) != (a.intensity != nullptr) ||
      (a.image && (a.channels < 1 || a.image_dtype < 0 || a.image_dtype > 2)) ||
      measure_workspace_bytes(a.N, a.H, a.W, a.max_inst, C) == 0 ||
      a.workspace_bytes < measure_workspace_bytes(a.N, a.H, a.W, a.max_inst, C))
    return hipErrorInvalidValue;
  const int NC = MC + IC * C;
  const bool flt = C > 0 && a.image_dtype == 2;
  const int ntx = (a.W + TW - 1) / TW, nty = (a.H + TH - 1) / TH;
  u64* acc = static_cast<u64*>(a.workspace);
  u64* status = reinterpret_cast<u64*>(a.status);
  hipError_t e;
  {
    const size_t words = (size_t)a.N * a.max_inst * NC;
    const size_t blocks = (words + NT - 1) / NT;
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096));
    measure_init_kernel<<<grid, dim3(NT), 0, st>>>(acc, words, NC, a.H, a.W, status,
                                                   (size_t)a.N * UNET_MEASURE_STATUS);
  }
  // frames go on grid.y (<= 65535 per launch)
  for (int n0 = 0; n0 < a.N; n0 += 65535) {
    const unsigned nn = (unsigned)(a.N - n0 < 65535 ? a.N - n0 : 65535);
    if (C == 0) launch_tile<uint8_t, 0>(a, n0, nn, ntx, nty, acc, status, st);
    else if (a.image_dtype == 0) launch_tile_c<uint8_t>(a, n0, nn, ntx, nty, acc, status, st);
    else if (a.image_dtype == 1) launch_tile_c<uint16_t>(a, n0, nn, ntx, nty, acc, status, st);
    else launch_tile_c<float>(a, n0, nn, ntx, nty, acc, status, st);
    const dim3 fgrid((unsigned)((a.max_inst + NT - 1) / NT), nn);
    const u64* ac = acc + (size_t)n0 * a.max_inst * NC;
    long long* tb = a.table + (size_t)n0 * a.max_inst * MC;
    u64* s = status + (size_t)n0 * UNET_MEASURE_STATUS;
    if (flt) measure_finish_kernel<true><<<fgrid, dim3(NT), 0, st>>>(
        ac, a.max_inst, C, tb, static_cast<double*>(a.intensity) + (size_t)n0 * a.max_inst * IC * C, s);
    else measure_finish_kernel<false><<<fgrid, dim3(NT), 0, st>>>(
        ac, a.max_inst, C, tb,
        C > 0 ? static_cast<long long*>(a.intensity) + (size_t)n0 * a.max_inst * IC * C : nullptr, s);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_select_instances(const SelectArgs& a, hipStream_t st) {
  if (!a.labels || !a.keep || !a.labels_out || !a.counts || !a.new_ids || !shape_ok(a.N, a.H, a.W) || a.M < 1 ||
      a.M > kMeasureMaxId)
    return hipErrorInvalidValue;
  const int HW = a.H * a.W;
  const bool vec = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(a.labels) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(a.labels_out) & 15) == 0;
  hipError_t e;
  for (int n0 = 0; n0 < a.N; n0 += 65535) {
    const unsigned nn = (unsigned)(a.N - n0 < 65535 ? a.N - n0 : 65535);
    int* ids = a.new_ids + (size_t)n0 * a.M;
    select_scan_kernel<<<dim3(nn), dim3(NT), 0, st>>>(a.keep + (size_t)n0 * a.M, a.M, ids, a.counts + n0);
    if (vec) select_gather_kernel<true><<<dim3((unsigned)((HW / 4 + NT - 1) / NT), nn), dim3(NT), 0, st>>>(
        a.labels + (size_t)n0 * HW, HW, a.M, ids, a.labels_out + (size_t)n0 * HW);
    else select_gather_kernel<false><<<dim3((unsigned)((HW + NT - 1) / NT), nn), dim3(NT), 0, st>>>(
        a.labels + (size_t)n0 * HW, HW, a.M, ids, a.labels_out + (size_t)n0 * HW);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace unet
