// Training targets for touching cells (gfx950): the exact transform to the two
// nearest distinct instances of a label map, the U-Net border weight map as an
// epilogue of it, and the interior / boundary / background targets.  No reference
// counterpart; the definitions are in include/unet_hip.h and tests/weights_ref.py.
//
// Sites are the pixels with labels > 0.  For every pixel p the first site s1 is
// the minimum over the sites s of the key (|p - s|^2, flat index of s), compared
// lexicographically (distance.hip's key); the second site s2 is the minimum of
// the same key over the sites whose label differs from labels[s1].  The key is
// separable with two candidates per pixel and column:
//
//   (a) two_col_kernel   one thread per column and segment of kDistColRows rows,
//                        lanes along x.  A sweep carries "rows to the last site
//                        and its label, rows to the last site with another label
//                        and that label": when a site with a new label appears
//                        the old first becomes the second.  The downward sweep
//                        stores that state for the sites above, the upward sweep
//                        merges it with the same state for the sites below into
//                        c1 = the column's nearest site (the upper one on a tie)
//                        and c2 = the nearest site of the column whose label
//                        differs from c1's (the upper one on a tie).  Three int32
//                        planes: the two int16 row offsets packed, the label of
//                        c1, the label of c2.  What a segment needs from outside
//                        it, it scans for itself, so no thread waits for another.
//   (b) two_row_kernel   one block per row; the three planes of the row are
//                        staged in LDS (12 W bytes <= 48 KiB, and 2 B per group).  A thread owns
//                        pixels x, x + 256, ... and walks the columns x -+ dx
//                        outwards with two running minima: k1 over all candidates,
//                        k2 over the candidates whose label differs from k1's.
//                        When a candidate with another label beats k1, the old k1
//                        is the minimum of everything seen and becomes k2.  A
//                        column is left out once dx^2 > min(d2 of k2, reach)
//                        (strictly, so that every tie is still seen); beyond the
//                        nearest 8 columns whole groups of 16 columns are skipped
//                        by the smallest |offset| of the group (two_scan).
// The row pass writes dist2 / ids, or for unet_border_weights directly
// out[p] = base(p) + w0 exp(-(sqrt d1 + sqrt d2)^2 / (2 sigma^2)) (the square
// roots and the exponential in double, one rounding to float); labelled pixels
// skip the scan there.
//
// Plain launches on the caller's stream; the workspace is the three planes (every
// word is written by (a) before (a) or (b) reads it).  No atomics, no memset, no
// block ever waits for another, kernel boundaries are the only ordering.  Integer
// arithmetic up to the epilogue: H, W <= 4096 and dy^2 + dx^2 <= 2 * 4095^2.
#include "../../include/unet_hip.h"
#include "common.h"
#include "kernels.h"

namespace unet {

namespace {

constexpr int CT = kDistColThreads;  // columns per block of the column pass (one wave)
constexpr int CS = kDistColRows;     // rows per thread of the column pass (a segment of a column)
constexpr int CB = kDistColBatch;    // rows loaded together by a column thread
constexpr int RT = kDistRowThreads;  // threads per block of the row pass
constexpr int kNoSite = -32768;      // offset of a column without a (second) site (|offsets| <= 4095)
constexpr int kNone = UNET_DISTANCE_NONE;
constexpr unsigned kFar = 0xffffffffu;  // d2 of "no candidate yet"
static_assert(kTwoMaxDim <= 32767 && 2ll * (kTwoMaxDim - 1) * (kTwoMaxDim - 1) < kNone, "int16 offsets, int32 d2");
static_assert(12 * (size_t)kTwoMaxDim + 2 * (size_t)(kTwoMaxDim / 16) <= 65536,
              "a staged row and its group minima fit the default LDS limit of a block");

// ---- (a) columns -------------------------------------------------------------

// The sites on one side of a pixel of a column, the pixel included: d1 rows to the
// nearest site and its label l1, d2 rows to the nearest site whose label differs
// from l1 and its label l2; -1: none.
struct Side {
  int d1, l1, d2, l2;
};

// one row further along the sweep, onto a pixel of value v
__device__ __forceinline__ void step(Side& s, int v) {
  if (s.d1 >= 0) ++s.d1;
  if (s.d2 >= 0) ++s.d2;
  if (v > 0) {
    if (s.d1 >= 0 && v != s.l1) { s.d2 = s.d1; s.l2 = s.l1; }  // the old first is the nearest with another label
    s.l1 = v;
    s.d1 = 0;
  }
}

__device__ __forceinline__ int pack(int o1, int o2) { return (int)(((unsigned)o1 & 0xffffu) | ((unsigned)o2 << 16)); }
__device__ __forceinline__ int lo16(int p) { return (int)(short)(p & 0xffff); }
__device__ __forceinline__ int hi16(int p) { return p >> 16; }

// One thread per column and segment of CS rows [ya, yb).  The state the sweeps
// carry into the segment comes from a scan of the labels outside it that stops at
// the second distinct label it meets (or at the frame's edge), so a segment
// depends on no other thread.  The CB loads of a batch are unconditional (row
// indices clamped into the range) so that they are all in flight together.
__global__ void __launch_bounds__(CT) two_col_kernel(const int* __restrict__ src, int H, int W, size_t plane,
                                                     int* __restrict__ ws) {
  const int x = (int)blockIdx.x * CT + (int)threadIdx.x;
  if (x >= W) return;
  const int ya = (int)blockIdx.z * CS, yb = min(ya + CS, H);
  const size_t base = (size_t)blockIdx.y * (size_t)H * (size_t)W + (size_t)x;
  const int* s = src + base;
  int* po = ws + base;            // packed offsets
  int* p1 = ws + plane + base;    // label of c1
  int* p2 = ws + 2 * plane + base;  // label of c2
  Side a{-1, 0, -1, 0};  // as seen from row ya - 1
  for (int y1 = ya - 1; y1 >= 0 && a.d2 < 0; y1 -= CB) {
    int v[CB];
#pragma unroll
    for (int k = 0; k < CB; ++k)
      v[k] = s[(size_t)max(y1 - k, 0) * W];
#pragma unroll
    for (int k = 0; k < CB; ++k)
      if (y1 - k >= 0 && a.d2 < 0 && v[k] > 0) {
        if (a.d1 < 0) { a.d1 = ya - 1 - (y1 - k); a.l1 = v[k]; }
        else if (v[k] != a.l1) { a.d2 = ya - 1 - (y1 - k); a.l2 = v[k]; }
      }
  }
  for (int y0 = ya; y0 < yb; y0 += CB) {
    int v[CB];
#pragma unroll
    for (int k = 0; k < CB; ++k)
      v[k] = s[(size_t)min(y0 + k, yb - 1) * W];
#pragma unroll
    for (int k = 0; k < CB; ++k)
      if (y0 + k < yb) {
        step(a, v[k]);
        const size_t i = (size_t)(y0 + k) * W;
        po[i] = pack(a.d1 < 0 ? kNoSite : -a.d1, a.d2 < 0 ? kNoSite : -a.d2);
        p1[i] = a.l1;
        p2[i] = a.l2;
      }
  }
  Side b{-1, 0, -1, 0};  // as seen from row yb
  for (int y0 = yb; y0 < H && b.d2 < 0; y0 += CB) {
    int v[CB];
#pragma unroll
    for (int k = 0; k < CB; ++k)
      v[k] = s[(size_t)min(y0 + k, H - 1) * W];
#pragma unroll
    for (int k = 0; k < CB; ++k)
      if (y0 + k < H && b.d2 < 0 && v[k] > 0) {
        if (b.d1 < 0) { b.d1 = y0 + k - yb; b.l1 = v[k]; }
        else if (v[k] != b.l1) { b.d2 = y0 + k - yb; b.l2 = v[k]; }
      }
  }
  for (int y1 = yb - 1; y1 >= ya; y1 -= CB) {
    int uo[CB], u1[CB], u2[CB];  // this thread's own stores of the downward sweep
#pragma unroll
    for (int k = 0; k < CB; ++k) {
      const size_t i = (size_t)max(y1 - k, ya) * W;
      uo[k] = po[i];
      u1[k] = p1[i];
      u2[k] = p2[i];
    }
#pragma unroll
    for (int k = 0; k < CB; ++k)
      if (y1 - k >= ya) {
        const int ad1 = lo16(uo[k]) == kNoSite ? -1 : -lo16(uo[k]);
        const int ad2 = hi16(uo[k]) == kNoSite ? -1 : -hi16(uo[k]);
        const int al1 = u1[k], al2 = u2[k];
        step(b, ad1 == 0 ? al1 : 0);  // the pixel is a site exactly when the last site above is 0 rows away
        // c1: the nearer of the two firsts, the upper one on a tie
        const bool up1 = ad1 >= 0 && (b.d1 < 0 || ad1 <= b.d1);
        const int o1 = up1 ? -ad1 : (b.d1 >= 0 ? b.d1 : kNoSite);
        const int l1 = up1 ? al1 : (b.d1 >= 0 ? b.l1 : 0);
        // c2: on either side the nearest site whose label differs from l1 is the
        // side's first if its label differs, else the side's second
        const bool af = ad1 >= 0 && al1 != l1, bf = b.d1 >= 0 && b.l1 != l1;
        const int ud = af ? ad1 : ad2, ul = af ? al1 : al2;
        const int dd = bf ? b.d1 : b.d2, dl = bf ? b.l1 : b.l2;
        const bool none2 = o1 == kNoSite || (ud < 0 && dd < 0);
        const bool up2 = ud >= 0 && (dd < 0 || ud <= dd);
        const size_t i = (size_t)(y1 - k) * W;
        po[i] = pack(o1, none2 ? kNoSite : (up2 ? -ud : dd));
        p1[i] = l1;
        p2[i] = none2 ? 0 : (up2 ? ul : dl);
      }
  }
}

// ---- (b) rows ----------------------------------------------------------------

struct TwoOut {
  int* dist2;              // [N][2][H][W] or null
  int* ids;                // [N][2][H][W] or null
  // border weights (out != null)
  const int* labels;       // [N][H][W]
  const uint8_t* classes;  // [N][H][W] or null
  const float* cw;         // K class weights or null
  int K;
  float w0;
  double inv2s2;           // 1 / (2 sigma^2)
  float* out;              // [N][H][W]
};

// The key of a candidate site of the staged row: d2, then the row offset, then the
// column in one word, which orders as (d2, flat index) does: at equal d2 the upper
// site (smaller o), then the smaller column.
typedef unsigned long long Key;
static_assert(kTwoMaxDim <= 65536, "the column fits 16 bits of the key");
__device__ __forceinline__ Key key_of(unsigned d2, int o, int c) {
  return ((Key)d2 << 32) | ((Key)(unsigned)(o + 32768) << 16) | (unsigned)c;
}
__device__ __forceinline__ unsigned d2_of(Key k) { return (unsigned)(k >> 32); }
constexpr Key kNoKey = ~0ull;  // no candidate yet: d2_of() == kFar
// The two running minima of a pixel are four scalars (k1 / l1: the minimum key of
// all candidates fed and its label; k2 / l2: the minimum key of those whose label
// differs from l1, and its label), so that they stay in registers.
// When a candidate of another label beats k1, the old first was the minimum of
// everything seen, so of everything with another label than the newcomer: it
// becomes the second.  Selects, no branches.
__device__ __forceinline__ void feed(Key& k1, int& l1, Key& k2, int& l2, Key k, int l) {
  const bool first = k < k1, other = l != l1;
  const bool second = !first && other && k < k2;
  const bool demote = first && other;
  k2 = demote ? k1 : (second ? k : k2);
  l2 = demote ? l1 : (second ? l : l2);
  k1 = first ? k : k1;
  l1 = first ? l : l1;
}

// The staged row: the three planes and, per group of G columns, the smallest
// |offset of c1| of the group (kGroupNone: no column of the group has a site).
struct TwoRow {
  const int* O;   // packed offsets
  const int* L1;  // labels of c1
  const int* L2;  // labels of c2
  const unsigned short* GM;
  int W, ng;
};
constexpr int G = kDistGroup;        // columns per group of the row pass
constexpr unsigned kGroupNone = 65535;
constexpr int kNear = 8;             // columns on either side that are looked at one by one before the groups

// the two candidates of column c at squared column distance dx2 against the running minima
__device__ __forceinline__ void column(const TwoRow& R, int c, unsigned dx2, unsigned reach, Key& k1, int& l1, Key& k2, int& l2) {
  const int p = R.O[c];
  const int o1 = lo16(p);
  if (o1 == kNoSite) return;
  const unsigned lim = min(d2_of(k2), reach);
  const unsigned d1 = (unsigned)(o1 * o1) + dx2;
  if (d1 > lim) return;  // c2 is not nearer than c1
  feed(k1, l1, k2, l2, key_of(d1, o1, c), R.L1[c]);
  const int o2 = hi16(p);
  if (o2 == kNoSite) return;
  const unsigned d2 = (unsigned)(o2 * o2) + dx2;
  if (d2 <= min(d2_of(k2), reach)) feed(k1, l1, k2, l2, key_of(d2, o2, c), R.L2[c]);
}

// the columns of group g, whose smallest dx is n, if its lower bound allows a candidate
__device__ __forceinline__ void group(const TwoRow& R, int g, unsigned n, int x, unsigned reach, Key& k1, int& l1, Key& k2, int& l2) {
  const unsigned m = R.GM[g];
  if (m == kGroupNone || m * m + n * n > min(d2_of(k2), reach)) return;
  const int c1 = min(g * G + G, R.W);
  for (int c = g * G; c < c1; ++c) {
    const int dx = c - x;
    column(R, c, (unsigned)(dx * dx), reach, k1, l1, k2, l2);
  }
}

// Minimum keys over the columns of the row seen from pixel x.  A candidate beyond
// reach is never fed, so k1 / k2 are the minima within reach.  First the kNear
// columns on either side one by one, which settles most pixels between two cells;
// then whole groups of G columns outwards from x's own group.  With m the smallest
// |offset| of a group and n its smallest dx, every candidate of the group has d2 >=
// m^2 + n^2 (c2 is never nearer than c1), so a group is opened only when that is <=
// lim = min(d2_of(k2), reach), and a side ends once n^2 > lim (strictly, so that every
// tie is still seen).  Feeding a candidate twice changes nothing, so the groups may
// overlap the columns already looked at.
__device__ __forceinline__ void two_scan(const TwoRow& R, int x, unsigned reach, Key& k1, int& l1, Key& k2, int& l2) {
  k1 = k2 = kNoKey;
  l1 = l2 = 0;
  column(R, x, 0u, reach, k1, l1, k2, l2);
  unsigned dx2 = 1;
  for (int dx = 1; dx <= kNear; dx2 += 2u * dx + 1u, ++dx) {
    if (dx2 > min(d2_of(k2), reach)) return;
    const int l = x - dx, r = x + dx;
    if (l < 0 && r >= R.W) return;
    if (l >= 0) column(R, l, dx2, reach, k1, l1, k2, l2);
    if (r < R.W) column(R, r, dx2, reach, k1, l1, k2, l2);
  }
  const int g0 = x / G;
  for (int k = 0;; ++k) {
    const int gl = g0 - k, gr = g0 + k;
    const unsigned nl = k == 0 ? 0u : (unsigned)(x - (gl * G + G - 1)), nr = k == 0 ? 0u : (unsigned)(gr * G - x);
    const unsigned lim = min(d2_of(k2), reach);
    const bool inl = gl >= 0 && nl * nl <= lim, inr = k > 0 && gr < R.ng && nr * nr <= lim;
    if (!inl && !inr) break;
    if (inl) group(R, gl, nl, x, reach, k1, l1, k2, l2);
    if (inr) group(R, gr, nr, x, reach, k1, l1, k2, l2);
  }
}

template <bool BORDER>
__global__ void __launch_bounds__(RT) two_row_kernel(const int* __restrict__ ws, int H, int W, size_t plane,
                                                     unsigned reach, TwoOut r) {
  extern __shared__ __attribute__((aligned(16))) int S[];  // the row's three planes, then the group minima
  const int y = blockIdx.x;
  const size_t row = ((size_t)blockIdx.y * (size_t)H + (size_t)y) * (size_t)W;
  for (int x = threadIdx.x; x < W; x += RT) {
    S[x] = ws[row + x];
    S[W + x] = ws[plane + row + x];
    S[2 * W + x] = ws[2 * plane + row + x];
  }
  __syncthreads();
  const int ng = (W + G - 1) / G;
  unsigned short* GM = reinterpret_cast<unsigned short*>(S + 3 * W);
  for (int g = threadIdx.x; g < ng; g += RT) {
    unsigned m = kGroupNone;
    for (int c = g * G; c < min(g * G + G, W); ++c) {
      const int o = lo16(S[c]);
      if (o != kNoSite) m = min(m, (unsigned)abs(o));
    }
    GM[g] = (unsigned short)m;
  }
  __syncthreads();
  const TwoRow R{S, S + W, S + 2 * W, GM, W, ng};
  const size_t HW = (size_t)H * (size_t)W;
  for (int x = threadIdx.x; x < W; x += RT) {
    Key k1 = kNoKey, k2 = kNoKey;
    int l1 = 0, l2 = 0;
    if (BORDER) {
      double v = 1.0;
      if (r.classes) {
        const int c = r.classes[row + x];
        v = c < r.K ? (double)r.cw[c] : 0.0;
      }
      if (r.labels[row + x] <= 0 && r.w0 != 0.f) {
        two_scan(R, x, reach, k1, l1, k2, l2);
        if (d2_of(k2) != kFar) {
          const double s = sqrt((double)d2_of(k1)) + sqrt((double)d2_of(k2));
          v += (double)r.w0 * exp(-(s * s) * r.inv2s2);
        }
      }
      r.out[row + x] = (float)v;
    } else {
      two_scan(R, x, reach, k1, l1, k2, l2);
      const size_t i0 = ((size_t)blockIdx.y * 2 * (size_t)H + (size_t)y) * (size_t)W + (size_t)x, i1 = i0 + HW;
      if (r.dist2) {
        r.dist2[i0] = d2_of(k1) == kFar ? kNone : (int)d2_of(k1);
        r.dist2[i1] = d2_of(k2) == kFar ? kNone : (int)d2_of(k2);
      }
      if (r.ids) {
        r.ids[i0] = d2_of(k1) == kFar ? 0 : l1;
        r.ids[i1] = d2_of(k2) == kFar ? 0 : l2;
      }
    }
  }
}

// 0 background, 1 interior, 2 boundary: a labelled pixel with a neighbour inside
// the frame of another value (4 or 8 neighbours)
__global__ void __launch_bounds__(256) boundary_targets_kernel(const int* __restrict__ lab, int H, int W, int conn8,
                                                               uint8_t* __restrict__ cls) {
  const int x = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (x >= W) return;
  const int y = (int)(blockIdx.y % (unsigned)H);  // blockIdx.y walks the rows of all frames of the launch
  const size_t frame = (size_t)(blockIdx.y / (unsigned)H) * (size_t)H * (size_t)W;
  const int* f = lab + frame;
  const int v = f[(size_t)y * W + x];
  int c = 0;
  if (v > 0) {
    bool diff = false;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        if ((dy == 0 && dx == 0) || (!conn8 && dy != 0 && dx != 0)) continue;
        const int yy = y + dy, xx = x + dx;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W && f[(size_t)yy * W + xx] != v) diff = true;
      }
    c = diff ? 2 : 1;
  }
  cls[frame + (size_t)y * W + x] = (uint8_t)c;
}

inline size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }

inline bool shape_ok(int N, int H, int W) { return N > 0 && H > 0 && W > 0 && H <= kTwoMaxDim && W <= kTwoMaxDim; }

}  // namespace

int64_t two_nearest_workspace_bytes(int N, int H, int W) {
  if (!shape_ok(N, H, W)) return 0;
  return (int64_t)a256(12 * (size_t)N * H * W);
}

hipError_t launch_two_nearest(const TwoArgs& a, hipStream_t st) {
  const bool border = a.out != nullptr;
  if (!a.labels || !a.workspace || !shape_ok(a.N, a.H, a.W) || (!border && !a.dist2 && !a.ids) ||
      (border && (!(a.w0 >= 0.f) || !(a.sigma > 0.f) || (a.classes != nullptr) != (a.class_weights != nullptr) ||
                  (a.classes && a.K <= 0))) ||
      a.workspace_bytes < two_nearest_workspace_bytes(a.N, a.H, a.W))
    return hipErrorInvalidValue;
  const int H = a.H, W = a.W;
  const size_t HW = (size_t)H * W, plane = (size_t)a.N * HW;
  int* ws = static_cast<int*>(a.workspace);
  const size_t lds = 12 * (size_t)W + 2 * (size_t)((W + G - 1) / G);  // the three planes and the group minima
  const unsigned reach = a.max_dist2 < 0 || a.max_dist2 >= kNone ? (unsigned)kNone : (unsigned)a.max_dist2;
  const double inv2s2 = border ? 1.0 / (2.0 * (double)a.sigma * (double)a.sigma) : 0.0;
  // frames go on grid.y (<= 65535 per launch)
  for (int n0 = 0; n0 < a.N; n0 += 65535) {
    const unsigned nn = (unsigned)(a.N - n0 < 65535 ? a.N - n0 : 65535);
    const size_t px = (size_t)n0 * HW;
    two_col_kernel<<<dim3((unsigned)((W + CT - 1) / CT), nn, (unsigned)((H + CS - 1) / CS)), dim3(CT), 0, st>>>(
        a.labels + px, H, W, plane, ws + px);
    const dim3 rows((unsigned)H, nn), blk(RT);
    if (border) {
      const TwoOut r{nullptr, nullptr, a.labels + px, a.classes ? a.classes + px : nullptr, a.class_weights, a.K,
                     a.w0, inv2s2, a.out + px};
      two_row_kernel<true><<<rows, blk, lds, st>>>(ws + px, H, W, plane, reach, r);
    } else {
      const TwoOut r{a.dist2 ? a.dist2 + 2 * px : nullptr, a.ids ? a.ids + 2 * px : nullptr, nullptr, nullptr,
                     nullptr, 0, 0.f, 0.0, nullptr};
      two_row_kernel<false><<<rows, blk, lds, st>>>(ws + px, H, W, plane, reach, r);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_boundary_targets(const int* labels, int N, int H, int W, int connectivity, uint8_t* classes,
                                   hipStream_t st) {
  if (!labels || !classes || N <= 0 || H <= 0 || W <= 0 || H > kDistMaxDim || W > kDistMaxDim ||
      (int64_t)H * W >= ((int64_t)1 << 31) || (connectivity != 1 && connectivity != 2))
    return hipErrorInvalidValue;
  const size_t HW = (size_t)H * W;
  const int per = 65535 / H;  // whole frames per launch: their rows go on grid.y (<= 65535)
  for (int n0 = 0; n0 < N; n0 += per) {
    const int nn = N - n0 < per ? N - n0 : per;
    boundary_targets_kernel<<<dim3((unsigned)((W + 255) / 256), (unsigned)(nn * H)), dim3(256), 0, st>>>(
        labels + (size_t)n0 * HW, H, W, connectivity == 2, classes + (size_t)n0 * HW);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace unet
