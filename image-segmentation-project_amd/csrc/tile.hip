// Tiled whole-frame inference (gfx950): cut a frame of any size into T x T
// tiles for the tile-sized eval forward, and blend the tiles' logits back into
// the frame.  No reference counterpart (the reference predicts at the training
// size only).
//
// Geometry (one definition: tile_axis_count / tile_origin / tile_w1 of
// kernels.h, predict.tile_origins, tests/tile_ref.py).  Square tiles T x T,
// overlap O, stride S = T - O, 0 <= O <= T/2.  Per axis of length L:
//   L <= T: one tile at origin -((T - L) / 2) (centred; the footprint outside
//           the image is BORDER_REFLECT_101, reflect101 of common.h);
//   L >  T: n = ceil((L - T) / S) + 1 tiles at j S (j < n - 1) and L - T.
// With O <= T/2 at most 3 tiles cover a pixel per axis.  The blend weight of
// footprint position (u, v) is the integer w1(u) w1(v), w1(i) = min(i + 1,
// T - i, O + 1).  Test-time augmentation: dihedral transform d = k + 4 flip =
// "np.rot90(a, k), then [::-1] if flip" (rot90_vflip_kernel's convention) of
// the tile CONTENT, selected by the bits of `tta`; M = popcount(tta), m = the
// rank of d among the set bits.  Flat tile index t = ((n M + m) ny + jy) nx + jx.
//
// Both launch (64, 4) blocks over (lane group along x, row) and index in 32 bits.
//
//   tile_gather_kernel  image fp32 [N][H][W] -> tiles [count][T][T] for t in
//                       [first, first + count); slots t >= total are zeros.
//                       4 tile pixels (16 B) per lane where T % 4 == 0;
//                       identity-transform rows inside the image load 16 B when
//                       the source address is aligned, everything else scalar.
//   tile_blend_kernel   tile logits [total][K][T][T] -> per image pixel and
//                       class  (sum_t w_t v_t) / (float)(sum_t w_t)  over the
//                       covering tiles in ascending t (v_t read back through
//                       the inverse transform): fp32 multiply and add kept
//                       apart, from 0; int32 weight sum converted once;
//                       __fdiv_rn.  Gather form over output pixels: no atomics,
//                       bit-reproducible.  Optional outputs of the same pass:
//                       logits, the sigmoid mask (mask_positive), argmax labels
//                       (lowest class wins ties, as confusion_kernel).
//                       4 pixels along x per lane where W % 4 == 0 and the
//                       outputs are aligned; a tile row segment that holds all
//                       4 under a non-transposing transform is one 16-B load
//                       when aligned.
//
// Both are HBM-bound streams.  This file is built with -ffp-contract=off so
// the numpy restatement reproduces the blend bit for bit.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace unet {

// tile position (y, x) of transform d reads footprint position (sy, sx):
// tile = flip?(rot90(footprint, k))
__device__ __forceinline__ void dihedral_src(int d, int T, int y, int x, int& sy, int& sx) {
  if (d & 4) y = T - 1 - y;
  switch (d & 3) {
    case 0: sy = y; sx = x; break;
    case 1: sy = x; sx = T - 1 - y; break;
    case 2: sy = T - 1 - y; sx = T - 1 - x; break;
    default: sy = T - 1 - x; sx = y; break;
  }
}

// the inverse: footprint position (uy, ux) is held by tile position (ty, tx)
__device__ __forceinline__ void dihedral_dst(int d, int T, int uy, int ux, int& ty, int& tx) {
  switch (d & 3) {
    case 0: ty = uy; tx = ux; break;
    case 1: ty = T - 1 - ux; tx = uy; break;
    case 2: ty = T - 1 - uy; tx = T - 1 - ux; break;
    default: ty = ux; tx = T - 1 - uy; break;
  }
  if (d & 4) ty = T - 1 - ty;
}

// the m-th (ascending) set bit of tta
__device__ __forceinline__ int nth_transform(unsigned tta, int m) {
  int d = 0;
  for (; d < 8; ++d)
    if ((tta >> d) & 1u) {
      if (m == 0) break;
      --m;
    }
  return d;
}

template <int V>
__global__ void __launch_bounds__(256) tile_gather_kernel(const float* __restrict__ img, float* __restrict__ tiles,
                                                          TileGeom g, int64_t first, int count) {
  // block (64, 4): x = lane groups of a tile row (grid.y chunks), y = rows slot * T + y (grid.x)
  const int xg = blockIdx.y * blockDim.x + threadIdx.x;
  const unsigned r = blockIdx.x * blockDim.y + threadIdx.y;
  if (xg >= g.T / V || r >= (unsigned)count * (unsigned)g.T) return;
  const int x0 = xg * V, y = (int)(r % (unsigned)g.T);
  const int64_t slot = r / (unsigned)g.T;
  const int64_t t = first + slot;
  float v[V];
#pragma unroll
  for (int e = 0; e < V; ++e) v[e] = 0.f;
  if (t < g.total) {
    const unsigned tu = (unsigned)t;  // total < 2^31 (tile_geom)
    const int jx = (int)(tu % (unsigned)g.nx), jy = (int)((tu / (unsigned)g.nx) % (unsigned)g.ny);
    const unsigned nm = tu / (unsigned)(g.nx * g.ny);
    const int m = (int)(nm % (unsigned)g.M);
    const int64_t n = nm / (unsigned)g.M;
    const int d = nth_transform(g.tta, m);
    const int oy = tile_origin(jy, g.ny, g.H, g.T, g.S), ox = tile_origin(jx, g.nx, g.W, g.T, g.S);
    const float* src = img + n * (int64_t)g.H * g.W;
    bool done = false;
    if (V == 4 && d == 0 && ox + x0 >= 0 && ox + x0 + 3 < g.W) {  // an interior row of the identity transform
      const float* p = src + (int64_t)reflect101(oy + y, g.H) * g.W + ox + x0;
      if (((size_t)p & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1 % V] = q.y; v[2 % V] = q.z; v[3 % V] = q.w;
        done = true;
      }
    }
    if (!done) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        int sy, sx;
        dihedral_src(d, g.T, y, x0 + e, sy, sx);
        v[e] = src[(int64_t)reflect101(oy + sy, g.H) * g.W + reflect101(ox + sx, g.W)];
      }
    }
  }
  float* dst = tiles + (slot * g.T + y) * g.T + x0;
  if (V == 4) {
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1 % V], v[2 % V], v[3 % V]);
  } else {
    dst[0] = v[0];
  }
}

// tiles of an axis that cover pixels [p0, p1] (p1 - p0 < T): the regular ones
// jlo..jhi (origins j S, j < n - 1; empty when jlo > jhi) and, when `last`, the
// final tile n - 1 at L - T.  L <= T: the single tile.
__device__ __forceinline__ void covering(int p0, int p1, int n, int L, int T, int S, int& jlo, int& jhi, bool& last) {
  if (L <= T) {
    jlo = 0; jhi = -1; last = true;
    return;
  }
  jlo = p0 < T ? 0 : (p0 - T) / S + 1;
  jhi = min(p1 / S, n - 2);
  last = p1 >= L - T;
}

template <int V>
__global__ void __launch_bounds__(256) tile_blend_kernel(const float* __restrict__ tl, float* __restrict__ logits,
                                                         uint8_t* __restrict__ mask, uint8_t* __restrict__ labels,
                                                         TileGeom g, int N, int K) {
  // block (64, 4): x = lane groups of an image row (grid.y chunks), y = rows n * H + y (grid.x)
  const int xg = blockIdx.y * blockDim.x + threadIdx.x;
  const unsigned r = blockIdx.x * blockDim.y + threadIdx.y;
  if (xg >= (V == 4 ? g.W / 4 : g.W) || r >= (unsigned)N * (unsigned)g.H) return;
  const int x0 = xg * V, y = (int)(r % (unsigned)g.H);
  const int64_t n = r / (unsigned)g.H;
  const int T = g.T;
  const int64_t TT = (int64_t)T * T, HW = (int64_t)g.H * g.W;
  int ylo, yhi, xlo, xhi;
  bool ylast, xlast;
  covering(y, y, g.ny, g.H, T, g.S, ylo, yhi, ylast);
  covering(x0, x0 + V - 1, g.nx, g.W, T, g.S, xlo, xhi, xlast);
  const int ycnt = max(yhi - ylo + 1, 0) + (ylast ? 1 : 0), xcnt = max(xhi - xlo + 1, 0) + (xlast ? 1 : 0);
  float best[V];
  int arg[V];
#pragma unroll
  for (int e = 0; e < V; ++e) { best[e] = 0.f; arg[e] = 0; }
  for (int k = 0; k < K; ++k) {
    float acc[V];
    int ws[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { acc[e] = 0.f; ws[e] = 0; }
    for (int m = 0; m < g.M; ++m) {
      const int d = nth_transform(g.tta, m);
      for (int a = 0; a < ycnt; ++a) {
        const int jy = (ylast && a == ycnt - 1) ? g.ny - 1 : ylo + a;
        const int uy = y - tile_origin(jy, g.ny, g.H, T, g.S);
        const int wy = tile_w1(uy, T, g.O);
        for (int b = 0; b < xcnt; ++b) {
          const int jx = (xlast && b == xcnt - 1) ? g.nx - 1 : xlo + b;
          const int ux0 = x0 - tile_origin(jx, g.nx, g.W, T, g.S);
          const int64_t t = ((n * g.M + m) * g.ny + jy) * g.nx + jx;
          const float* tp = tl + (t * K + k) * TT;
          float v[V];
          bool cov[V];
#pragma unroll
          for (int e = 0; e < V; ++e) cov[e] = ux0 + e >= 0 && ux0 + e < T;
          bool done = false;
          if (V == 4 && !(d & 1) && ux0 >= 0 && ux0 + 3 < T) {  // the 4 pixels are one tile row segment
            int ty, tx0, tx3;
            dihedral_dst(d, T, uy, ux0, ty, tx0);
            dihedral_dst(d, T, uy, ux0 + 3, ty, tx3);
            const float* p = tp + (int64_t)ty * T + min(tx0, tx3);
            if (((size_t)p & 15) == 0) {
              const float4 q = *reinterpret_cast<const float4*>(p);
              const bool rev = tx3 < tx0;
              v[0] = rev ? q.w : q.x; v[1 % V] = rev ? q.z : q.y;
              v[2 % V] = rev ? q.y : q.z; v[3 % V] = rev ? q.x : q.w;
              done = true;
            }
          }
          if (!done) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
              v[e] = 0.f;
              if (cov[e]) {
                int ty, tx;
                dihedral_dst(d, T, uy, ux0 + e, ty, tx);
                v[e] = tp[(int64_t)ty * T + tx];
              }
            }
          }
#pragma unroll
          for (int e = 0; e < V; ++e) {
            if (cov[e]) {
              const int w = wy * tile_w1(ux0 + e, T, g.O);
              acc[e] = __fadd_rn(acc[e], __fmul_rn((float)w, v[e]));
              ws[e] += w;
            }
          }
        }
      }
    }
    float o[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      o[e] = __fdiv_rn(acc[e], (float)ws[e]);
      if (k == 0 || o[e] > best[e]) { best[e] = o[e]; arg[e] = k; }
    }
    const int64_t off = (n * K + k) * HW + (int64_t)y * g.W + x0;
    if (V == 4) {
      if (logits) *reinterpret_cast<float4*>(logits + off) = make_float4(o[0], o[1 % V], o[2 % V], o[3 % V]);
      if (mask)
        *reinterpret_cast<uchar4*>(mask + off) =
            make_uchar4(mask_positive(o[0]), mask_positive(o[1 % V]), mask_positive(o[2 % V]), mask_positive(o[3 % V]));
    } else {
      if (logits) logits[off] = o[0];
      if (mask) mask[off] = mask_positive(o[0]) ? 1 : 0;
    }
  }
  if (labels) {
    const int64_t off = n * HW + (int64_t)y * g.W + x0;
    if (V == 4) {
      *reinterpret_cast<uchar4*>(labels + off) =
          make_uchar4((uint8_t)arg[0], (uint8_t)arg[1 % V], (uint8_t)arg[2 % V], (uint8_t)arg[3 % V]);
    } else {
      labels[off] = (uint8_t)arg[0];
    }
  }
}

bool tile_geom(int H, int W, int T, int overlap, unsigned tta, int N, TileGeom* g) {
  if (H <= 0 || W <= 0 || T <= 0 || overlap < 0 || 2 * (int64_t)overlap > T || N <= 0 || tta == 0 || tta > 0xFFu)
    return false;
  g->H = H; g->W = W; g->T = T; g->O = overlap; g->S = T - overlap;
  g->ny = tile_axis_count(H, T, g->S);
  g->nx = tile_axis_count(W, T, g->S);
  g->tta = tta;
  g->M = __builtin_popcount(tta);
  g->total = (int64_t)N * g->M * g->ny * g->nx;
  // 32-bit row and tile indices in the kernels
  return g->total <= 0x7fffffffll && (int64_t)N * H <= 0x7fffffffll;
}

// grid of (64, 4) blocks over `cols` lane groups x `rows` rows: rows along grid.x (up to 2^31 - 1 blocks)
static bool grid_for(int64_t rows, int64_t cols, dim3* grid) {
  const int64_t gx = (rows + 3) / 4, gy = (cols + 63) / 64;
  if (rows <= 0 || cols <= 0 || rows > 0x7fffffffll || gx > 0x7fffffffll || gy > 65535) return false;
  *grid = dim3((unsigned)gx, (unsigned)gy);
  return true;
}

hipError_t launch_tile_gather(const float* image, float* tiles, const TileGeom& g, int64_t first, int64_t count,
                              hipStream_t st) {
  if (count <= 0) return count == 0 ? hipSuccess : hipErrorInvalidValue;
  const bool vec = g.T % 4 == 0 && ((size_t)tiles & 15) == 0;
  dim3 grid;
  if (count > 0x7fffffffll / g.T || !grid_for(count * g.T, vec ? g.T / 4 : g.T, &grid)) return hipErrorInvalidValue;
  if (vec)
    hipLaunchKernelGGL(tile_gather_kernel<4>, grid, dim3(64, 4), 0, st, image, tiles, g, first, (int)count);
  else
    hipLaunchKernelGGL(tile_gather_kernel<1>, grid, dim3(64, 4), 0, st, image, tiles, g, first, (int)count);
  return hipGetLastError();
}

hipError_t launch_tile_blend(const float* tile_logits, float* logits, uint8_t* mask, uint8_t* labels,
                             const TileGeom& g, int N, int K, hipStream_t st) {
  const bool vec = g.W % 4 == 0 && ((size_t)logits & 15) == 0 && ((size_t)mask & 3) == 0 && ((size_t)labels & 3) == 0;
  dim3 grid;
  if (!grid_for((int64_t)N * g.H, vec ? g.W / 4 : g.W, &grid)) return hipErrorInvalidValue;
  if (vec)
    hipLaunchKernelGGL(tile_blend_kernel<4>, grid, dim3(64, 4), 0, st, tile_logits, logits, mask, labels, g, N, K);
  else
    hipLaunchKernelGGL(tile_blend_kernel<1>, grid, dim3(64, 4), 0, st, tile_logits, logits, mask, labels, g, N, K);
  return hipGetLastError();
}

}  // namespace unet
