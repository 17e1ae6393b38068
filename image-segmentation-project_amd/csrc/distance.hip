// Exact Euclidean distance transform with nearest-site (feature) transform of
// label maps and masks, and nearest-label growth of instances on top of it
// (gfx950).  No reference counterpart; the definitions are in
// include/unet_hip.h and tests/distance_ref.py.
//
// A set of pixels of each frame are sites.  For every pixel p the result is the
// minimum over the sites s of the key (|p - s|^2, flat index of s), compared
// lexicographically: dist2 is its first part, nearest its second.  The key is
// separable:
//
//   (a) dist_col_kernel   one thread per column and segment of kDistColRows rows
//                         (lanes along x, so every row access is coalesced; what
//                         a segment needs from outside it, it scans for itself).
//                         A downward sweep stores minus
//                         the distance to the last site at or above each pixel,
//                         an upward sweep replaces it by plus the distance to the
//                         next site below where that is strictly nearer.  The
//                         int16 offset o (site row = y + o; -32768 when the
//                         column has no site) therefore names the column's
//                         nearest site and, on a tie, the upper one.  Within one
//                         column that is the minimum of the key: equal dy^2, and
//                         the upper site has the smaller flat index.
//   (b) dist_row_kernel   one block per row; the row's offsets are staged in LDS
//                         (2 W bytes <= 64 KiB).  Each thread owns pixels x, x +
//                         256, ... and takes the minimum of the key (o^2 + dx^2,
//                         (y + o) W + x') over the columns x' = x -+ dx.  A
//                         column's candidate for any pixel of the row is its own
//                         minimum key (dx^2 is a constant of the column), so the
//                         minimum over columns is the minimum over all sites.  A
//                         column can be left out once dx^2 > best dist2 (strictly:
//                         a column at dx^2 == best dist2 can still tie with a
//                         smaller flat index) or, when growing, dx^2 > max_dist2.
//                         The nearest kNear columns on either side are looked at
//                         one by one; if that does not settle the pixel, whole
//                         groups of G columns are skipped by the smallest
//                         |offset| of the group (row_scan).
// The row pass writes dist2 / nearest, or for unet_grow_instances directly
// out[p] = labels[p] != 0 ? labels[p] : labels[nearest] if allowed and in reach.
//
// Plain launches on the caller's stream; the only workspace is the int16 offset
// array (every entry is written by (a) before (b) reads it, so it need not be
// initialised).  No atomics, no block ever waits for another, kernel boundaries
// are the only ordering.  Integer arithmetic throughout: H, W <= 32768 and
// dy^2 + dx^2 <= 2 * 32767^2 < 2^31 - 1 = UNET_DISTANCE_NONE.
#include "../../include/unet_hip.h"
#include "common.h"
#include "kernels.h"

namespace unet {

namespace {

constexpr int CT = kDistColThreads;  // columns per block of the column pass (one wave)
constexpr int CS = kDistColRows;     // rows per thread of the column pass (a segment of a column)
constexpr int CB = kDistColBatch;    // rows loaded together by a column thread
constexpr int RT = kDistRowThreads;  // threads per block of the row pass
constexpr int G = kDistGroup;       // columns per group of the row pass
static_assert(G == 16, "a group is two 16-byte LDS reads");
constexpr int kNoSite = -32768;      // offset of a column without a site (|offsets| <= 32767)
constexpr int kNone = UNET_DISTANCE_NONE;
static_assert(kDistMaxDim == 32768 && kNone == 2147483647, "int16 offsets, int32 squared distances");


// ---- (a) columns -------------------------------------------------------------

template <typename T>
__device__ __forceinline__ bool is_site(T v, int fg_value, int sites) {
  return (fg_value < 0 ? v != 0 : (int)v == fg_value) == (sites != 0);
}

// One thread per column and segment of CS rows [ya, yb).  What the sweeps carry
// into the segment, the distance from its first row to the last site above and
// from its last row to the next site below, comes from a scan of the source
// outside the segment that stops at the first site it meets, so a segment
// depends on no other thread.  The CB loads of a batch are unconditional (row
// indices clamped into the range) so that they are all in flight together.
template <typename T>
__global__ void __launch_bounds__(CT) dist_col_kernel(const T* __restrict__ src, int H, int W, int fg_value,
                                                      int sites, short* __restrict__ off) {
  const int x = (int)blockIdx.x * CT + (int)threadIdx.x;
  if (x >= W) return;
  const int ya = (int)blockIdx.z * CS, yb = min(ya + CS, H);
  const size_t base = (size_t)blockIdx.y * (size_t)H * (size_t)W + (size_t)x;
  const T* s = src + base;
  short* o = off + base;
  int d = -1;  // rows since the last site above; -1: none yet
  for (int y1 = ya - 1; y1 >= 0 && d < 0; y1 -= CB) {
    T v[CB];
#pragma unroll
    for (int k = 0; k < CB; ++k)
      v[k] = s[(size_t)max(y1 - k, 0) * W];
#pragma unroll
    for (int k = 0; k < CB; ++k)
      if (y1 - k >= 0 && d < 0 && is_site(v[k], fg_value, sites)) d = ya - 1 - (y1 - k);
  }
  for (int y0 = ya; y0 < yb; y0 += CB) {
    T v[CB];
#pragma unroll
    for (int k = 0; k < CB; ++k)
      v[k] = s[(size_t)min(y0 + k, yb - 1) * W];
#pragma unroll
    for (int k = 0; k < CB; ++k)
      if (y0 + k < yb) {
        d = is_site(v[k], fg_value, sites) ? 0 : (d < 0 ? -1 : d + 1);
        o[(size_t)(y0 + k) * W] = (short)(d < 0 ? kNoSite : -d);
      }
  }
  d = -1;  // rows to the next site below
  for (int y0 = yb; y0 < H && d < 0; y0 += CB) {
    T v[CB];
#pragma unroll
    for (int k = 0; k < CB; ++k)
      v[k] = s[(size_t)min(y0 + k, H - 1) * W];
#pragma unroll
    for (int k = 0; k < CB; ++k)
      if (y0 + k < H && d < 0 && is_site(v[k], fg_value, sites)) d = y0 + k - yb;
  }
  for (int y1 = yb - 1; y1 >= ya; y1 -= CB) {
    short up[CB];  // this thread's own stores of the downward sweep
#pragma unroll
    for (int k = 0; k < CB; ++k)
      up[k] = o[(size_t)max(y1 - k, ya) * W];
#pragma unroll
    for (int k = 0; k < CB; ++k)
      if (y1 - k >= ya) {
        const int u = up[k];
        d = u == 0 ? 0 : (d < 0 ? -1 : d + 1);
        // strictly nearer only: on a tie the upper site (smaller flat index) stays
        if (d > 0 && (u == kNoSite || d < -u)) o[(size_t)(y1 - k) * W] = (short)d;
      }
  }
}

// ---- (b) rows ----------------------------------------------------------------

struct RowOut {
  int* dist2;            // [N][H][W] or null
  int* nearest;          // [N][H][W] or null
  const int* labels;     // grow: [N][H][W]
  const uint8_t* within; // grow: [N][H][W] or null
  int within_value;      // grow: -1 nonzero, 0..255 ==
  int max_d2;            // grow: reach (kNone: unlimited)
  int* out;              // grow: [N][H][W]
};

// The nearest site of pixel x of the staged row: squared distance d2 (kNone: no
// site), the offset o and the column c of its site (flat index (y + o) W + c).
struct Best {
  unsigned d2;
  int o, c;
};

// d2 of column c seen at squared column distance dx2; a column outside the row or without a site never wins
__device__ __forceinline__ unsigned cand(int o, unsigned dx2, bool inside) {
  return inside && o != kNoSite ? (unsigned)(o * o) + dx2 : 0xffffffffu;
}
// (d2, flat index) order: at equal d2 the upper site (smaller o), then the smaller column
__device__ __forceinline__ void take(Best& b, unsigned d2, int o, int c) {
  if (d2 < b.d2 || (d2 == b.d2 && (o < b.o || (o == b.o && c < b.c)))) b = Best{d2, o, c};
}

// The staged row: the offsets of its columns, padded with kNoSite to whole groups
// of G columns, and for the first ngc groups the smallest |offset| of the group
// (kGroupNone: no column of the group has a site).
struct Row {
  const short* L;
  const unsigned short* GM;
  int W, ng, ngc;
};
constexpr unsigned kGroupNone = 32768;
constexpr int kNear = 16;  // columns on either side that are scanned one by one before the groups

// the 16 columns of group g against the best so far
__device__ __forceinline__ void visit(const Row& R, int g, int x, Best& b) {
  const uint4* q = reinterpret_cast<const uint4*>(R.L + g * G);
  const uint4 q0 = q[0], q1 = q[1];
  const unsigned w[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
  for (int j = 0; j < G; ++j) {
    const int o = (short)(j & 1 ? w[j / 2] >> 16 : w[j / 2] & 0xffffu);
    const int c = g * G + j, dx = c - x;
    const unsigned d2 = cand(o, (unsigned)(dx * dx), true);
    if (d2 <= b.d2) take(b, d2, o, c);  // rare: most columns only confirm the best
  }
}

// Minimum key over the columns of the row seen from pixel x: first the kNear
// columns on either side, and if that does not settle it (kNear^2 is still
// within the best d2), by groups of G columns outwards from x's own group.  With m = the smallest |offset| of a
// group, every column of it has d2 >= m^2 + (its smallest dx)^2, and one of
// them has d2 <= m^2 + (its largest dx)^2.  A first walk over the groups takes
// the second as an upper bound ub of the result; the second walk opens only the
// groups whose lower bound is <= min(best d2, ub, reach) and stops a side once
// its smallest dx^2 is above that (strictly, so that every tie is still seen).
// Groups beyond ngc have no minimum and are always opened.
__device__ __forceinline__ Best row_scan(const Row& R, int x, unsigned reach) {
  Best b{(unsigned)kNone, 0, x};
  {
    const int o = R.L[x];
    if (o != kNoSite) b = Best{(unsigned)(o * o), o, x};
  }
  // the nearest kNear columns on either side one by one: most pixels of a mask end here
  {
    unsigned bound = min(b.d2, reach), dx2 = 1;
    int dx = 1;
    for (; dx <= kNear && dx2 <= bound; dx2 += 2u * dx + 1u, ++dx) {
      const int l = x - dx, r = x + dx;
      const int ol = R.L[max(l, 0)], orr = R.L[min(r, R.W - 1)];  // both reads in flight together
      const unsigned dl = cand(ol, dx2, l >= 0), dr = cand(orr, dx2, r < R.W);
      if (min(dl, dr) <= b.d2) {  // rare: most columns only confirm the best
        if (dl != 0xffffffffu) take(b, dl, ol, l);
        if (dr != 0xffffffffu) take(b, dr, orr, r);
        bound = min(b.d2, reach);
      }
    }
    if (dx2 > bound) return b;
  }
  const int g0 = x / G;
  unsigned ub = min(b.d2, reach);
  if (g0 < R.ngc && R.GM[g0] != kGroupNone) {
    const unsigned m = R.GM[g0], far = (unsigned)max(x - g0 * G, g0 * G + G - 1 - x);
    ub = min(ub, m * m + far * far);
  }
  for (int k = 1;; ++k) {
    const int gl = g0 - k, gr = g0 + k;
    const unsigned nl = (unsigned)(x - (gl * G + G - 1)), nr = (unsigned)(gr * G - x);  // smallest dx
    const bool inl = gl >= 0 && gl < R.ngc && nl * nl <= ub, inr = gr < R.ngc && nr * nr <= ub;
    if (!inl && !inr) break;
    if (inl && R.GM[gl] != kGroupNone) {
      const unsigned m = R.GM[gl], far = nl + G - 1;
      ub = min(ub, m * m + far * far);
    }
    if (inr && R.GM[gr] != kGroupNone) {
      const unsigned m = R.GM[gr], far = nr + G - 1;
      ub = min(ub, m * m + far * far);
    }
  }
  visit(R, g0, x, b);
  unsigned bound = min(b.d2, ub);
  for (int k = 1;; ++k) {
    const int gl = g0 - k, gr = g0 + k;
    const unsigned nl = (unsigned)(x - (gl * G + G - 1)), nr = (unsigned)(gr * G - x);
    const bool inl = gl >= 0 && nl * nl <= bound, inr = gr < R.ng && nr * nr <= bound;
    if (!inl && !inr) break;
    if (inl) {
      const unsigned m = gl < R.ngc ? R.GM[gl] : 0u;
      if (m != kGroupNone && m * m + nl * nl <= bound) visit(R, gl, x, b);
    }
    if (inr) {
      const unsigned m = gr < R.ngc ? R.GM[gr] : 0u;
      if (m != kGroupNone && m * m + nr * nr <= bound) visit(R, gr, x, b);
    }
    bound = min(b.d2, ub);
  }
  return b;
}

template <bool GROW>
__global__ void __launch_bounds__(RT) dist_row_kernel(const short* __restrict__ off, int H, int W, int ngc, RowOut r) {
  extern __shared__ __attribute__((aligned(16))) short L[];  // the row's offsets, then the group minima
  const int y = blockIdx.x;
  const size_t row = ((size_t)blockIdx.y * (size_t)H + (size_t)y) * (size_t)W;
  const size_t frame = (size_t)blockIdx.y * (size_t)H * (size_t)W;
  const int ng = (W + G - 1) / G;
  unsigned short* GM = reinterpret_cast<unsigned short*>(L + ng * G);
  for (int x = threadIdx.x; x < ng * G; x += RT) L[x] = x < W ? off[row + x] : (short)kNoSite;
  __syncthreads();
  for (int g = threadIdx.x; g < ngc; g += RT) {
    unsigned m = kGroupNone;
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int o = L[g * G + j];
      if (o != kNoSite) m = min(m, (unsigned)abs(o));
    }
    GM[g] = (unsigned short)m;
  }
  __syncthreads();
  const Row R{L, GM, W, ng, ngc};
  for (int x = threadIdx.x; x < W; x += RT) {
    if (GROW) {
      int lab = r.labels[row + x];
      if (lab == 0) {
        const bool allowed = !r.within || (r.within_value < 0 ? r.within[row + x] != 0
                                                               : (int)r.within[row + x] == r.within_value);
        if (allowed) {
          const Best b = row_scan(R, x, (unsigned)r.max_d2);
          if (b.d2 <= (unsigned)r.max_d2 && b.d2 != (unsigned)kNone)
            lab = r.labels[frame + (size_t)(y + b.o) * (size_t)W + (size_t)b.c];
        }
      }
      r.out[row + x] = lab;
    } else {
      const Best b = row_scan(R, x, (unsigned)kNone);
      const bool found = b.d2 != (unsigned)kNone;
      if (r.dist2) r.dist2[row + x] = (int)b.d2;
      if (r.nearest) r.nearest[row + x] = found ? (y + b.o) * W + b.c : -1;
    }
  }
}

inline size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }

inline bool shape_ok(int N, int H, int W) {
  return N > 0 && H > 0 && W > 0 && H <= kDistMaxDim && W <= kDistMaxDim && (int64_t)H * W < ((int64_t)1 << 31);
}

template <typename T>
void launch_cols(const void* src, size_t off_px, int H, int W, int fg_value, int sites, short* off, unsigned nn,
                 hipStream_t st) {
  dist_col_kernel<T><<<dim3((unsigned)((W + CT - 1) / CT), nn, (unsigned)((H + CS - 1) / CS)), dim3(CT), 0, st>>>(
      static_cast<const T*>(src) + off_px, H, W, fg_value, sites, off + off_px);
}

}  // namespace

int64_t distance_workspace_bytes(int N, int H, int W) {
  if (!shape_ok(N, H, W)) return 0;
  return (int64_t)a256(2 * (size_t)N * H * W);
}

hipError_t launch_distance(const DistArgs& a, hipStream_t st) {
  const bool grow = a.out != nullptr;
  if (!a.src || !a.workspace || !shape_ok(a.N, a.H, a.W) || (a.src_dtype != 0 && a.src_dtype != 1) ||
      a.fg_value < -1 || (a.src_dtype == 0 && a.fg_value > 255) || (a.sites != 0 && a.sites != 1) ||
      (!grow && !a.dist2 && !a.nearest) || (grow && (a.src_dtype != 1 || a.out == a.src)) ||
      a.within_value < -1 || a.within_value > 255 || a.workspace_bytes < distance_workspace_bytes(a.N, a.H, a.W))
    return hipErrorInvalidValue;
  const int H = a.H, W = a.W;
  const size_t HW = (size_t)H * W;
  short* off = static_cast<short*>(a.workspace);
  // LDS of the row pass: the padded row, then as many group minima as fit 64 KiB with it
  const int ng = (W + G - 1) / G;
  const int ngc = (int)min((size_t)ng, (kDistRowLds - (size_t)ng * G * sizeof(short)) / sizeof(short));
  const size_t lds = ((size_t)ng * G + (size_t)ngc) * sizeof(short);
  const int reach = a.max_dist2 < 0 || a.max_dist2 >= kNone ? kNone : (int)a.max_dist2;
  // frames go on grid.y (<= 65535 per launch)
  for (int n0 = 0; n0 < a.N; n0 += 65535) {
    const unsigned nn = (unsigned)(a.N - n0 < 65535 ? a.N - n0 : 65535);
    const size_t px = (size_t)n0 * HW;
    if (a.src_dtype == 0) launch_cols<uint8_t>(a.src, px, H, W, a.fg_value, a.sites, off, nn, st);
    else launch_cols<int>(a.src, px, H, W, a.fg_value, a.sites, off, nn, st);
    const dim3 rows((unsigned)H, nn), blk(RT);
    if (grow) {
      const RowOut r{nullptr, nullptr, static_cast<const int*>(a.src) + px, a.within ? a.within + px : nullptr,
                     a.within_value, reach, a.out + px};
      dist_row_kernel<true><<<rows, blk, lds, st>>>(off + px, H, W, ngc, r);
    } else {
      const RowOut r{a.dist2 ? a.dist2 + px : nullptr, a.nearest ? a.nearest + px : nullptr, nullptr, nullptr, -1,
                     kNone, nullptr};
      dist_row_kernel<false><<<rows, blk, lds, st>>>(off + px, H, W, ngc, r);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace unet
