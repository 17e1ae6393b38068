// Softmax multi-class segmentation (gfx950): fused cross-entropy / multi-class
// Dice sums, their gradient wrt the logits, and the argmax confusion matrix.
//
// Logits are fp32 NCHW [N][K][HW] (head_fwd_mc_kernel's output), K = 2..16;
// labels are one integer per pixel [N][HW] in the caller's dtype (uint8 / int32
// / int64).  A thread owns whole pixels and holds their K values in registers,
// so every logit is read from HBM once and every wave load is one contiguous
// run of a channel plane: one pixel per lane in the sums kernel, 4 neighbouring
// pixels in the gradient and confusion kernels (one float4 per channel plane
// when the planes are 16-B aligned, 4 scalar loads otherwise; both forms give
// a thread the same pixels, so no result depends on the alignment).  K is a
// template parameter (the register arrays are statically indexed); blockIdx.y
// walks the images, so no index is divided.
//
// Per pixel, with m = max_k z_k first attained at kmax:
//   S'   = sum_{k != kmax} exp(z_k - m)
//   nll  = log1p(S') + (m - z_y)          (log1p with loss_accum's exact-rounding
//                                          correction: log(u) * S' / (u - 1), u = 1 + S')
//   p_k  = exp(z_k - m) / (1 + S')
// The plain log(sum exp) form rounds 1 + S' before the log and loses the
// confident-and-correct terms (S' ~ 1e-7 .. 1e-3) entirely.
#include "common.h"
#include "kernels.h"

namespace unet {
namespace {

// gradient / confusion kernels: float4 groups in flight per thread, K * U <= 16 loads of 16 B
constexpr int sm_unroll(int K) { return K <= 4 ? 4 : (K <= 8 ? 2 : 1); }

// exp(d), d <= 0, on v_exp_f32 with the rounding of d * log2(e) carried into a
// first-order correction: the bare product is off by up to |d| * 2^-24 * ln 2
// relative (1.2e-6 at d = -20), as large as the per-element bar of the BCE sums.
__device__ __forceinline__ float exp_neg(float d) {
  constexpr float kL2E = 1.44269502162933349609375f;  // fp32(log2 e)
  constexpr float kL2ELo = 1.92596299112661746e-8f;   // log2 e - fp32(log2 e)
  d = fmaxf(d, -104.f);  // exp2(-150) is already 0 in fp32; keeps d = -inf (a masked-out class) out of the fmaf below
  const float h = d * kL2E;
  const float l = fmaf(d, kL2E, -h) + d * kL2ELo;
  const float e = __builtin_amdgcn_exp2f(h);
  return fmaf(e, l * 0.693147182464599609375f, e);
}

// class index, or -1 for an ignored pixel, or -2 for any other label outside [0, K)
__device__ __forceinline__ int classify(int64_t lab, int K, int ign) {
  if (lab == (int64_t)ign) return -1;
  return (lab >= 0 && lab < (int64_t)K) ? (int)lab : -2;
}
// the class (classify) of pixel i
__device__ __forceinline__ int load_class(const void* p, int dt, int64_t i, int K, int ign) {
  if (dt == SM_LABEL_U8) return classify(reinterpret_cast<const uint8_t*>(p)[i], K, ign);
  if (dt == SM_LABEL_I32) return classify(reinterpret_cast<const int*>(p)[i], K, ign);
  return classify(reinterpret_cast<const long long*>(p)[i], K, ign);
}
// the classes of pixels i .. i + 3; vec: one packed load (i % 4 == 0 and the
// base aligned to 4 B for uint8, 16 B otherwise: sm_vec_ok)
__device__ __forceinline__ void load_classes4(const void* p, int dt, int64_t i, int K, int ign, int vec,
                                              int (&y)[4]) {
  int64_t l[4];
  if (!vec) {
#pragma unroll
    for (int c = 0; c < 4; ++c) y[c] = load_class(p, dt, i + c, K, ign);
    return;
  }
  if (dt == SM_LABEL_U8) {
    const uchar4 v = *reinterpret_cast<const uchar4*>(reinterpret_cast<const uint8_t*>(p) + i);
    l[0] = v.x; l[1] = v.y; l[2] = v.z; l[3] = v.w;
  } else if (dt == SM_LABEL_I32) {
    const int4 v = *reinterpret_cast<const int4*>(reinterpret_cast<const int*>(p) + i);
    l[0] = v.x; l[1] = v.y; l[2] = v.z; l[3] = v.w;
  } else {
    const longlong2* q = reinterpret_cast<const longlong2*>(reinterpret_cast<const long long*>(p) + i);
    const longlong2 a = q[0], b = q[1];
    l[0] = a.x; l[1] = a.y; l[2] = b.x; l[3] = b.y;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) y[c] = classify(l[c], K, ign);
}

// the K logits of pixels 4 j .. 4 j + 3 of one image: a float4 per channel
// plane (vec), or the same 4 values by scalar loads.  Both paths give every
// thread the same pixels in the same order, so the results do not depend on
// the alignment of the buffers.
template <int K>
__device__ __forceinline__ void load_quad(const float* __restrict__ xn, int64_t HW, int64_t j, int vec,
                                          float (&zv)[K][4]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float* p = xn + (size_t)k * HW + 4 * j;
    if (vec) {
      const float4 v = *reinterpret_cast<const float4*>(p);
      zv[k][0] = v.x; zv[k][1] = v.y; zv[k][2] = v.z; zv[k][3] = v.w;
    } else {
      zv[k][0] = p[0]; zv[k][1] = p[1]; zv[k][2] = p[2]; zv[k][3] = p[3];
    }
  }
}

// softmax of one pixel: p[], nll, kmax and S' (see the file comment)
template <int K>
__device__ __forceinline__ void softmax_px(const float (&z)[K], int y, float (&p)[K], float& nll, int& kmax,
                                           float& s_rest, float& ru_out) {
  float m = z[0];
  int km = 0;
#pragma unroll
  for (int k = 1; k < K; ++k)
    if (z[k] > m) { m = z[k]; km = k; }
  float e[K];
  float S = 0.f, zy = m;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    e[k] = k == km ? 0.f : exp_neg(z[k] - m);
    S += e[k];
    if (k == y) zy = z[k];
  }
  const float u = 1.f + S;
  const float ru = __builtin_amdgcn_rcpf(u);
  const float um1 = u - 1.f;
  const float l1p = um1 == 0.f ? S : __logf(u) * (S * __builtin_amdgcn_rcpf(um1));
  nll = l1p + (m - zy);
#pragma unroll
  for (int k = 0; k < K; ++k) p[k] = (k == km ? 1.f : e[k]) * ru;
  kmax = km;
  s_rest = S;
  ru_out = ru;
}

// per-thread fp32 partial sums, in the order of the block's scratch slot:
// ce_num, w_den, valid, invalid, I[K], P[K], Y[K]
template <int K>
struct SmAcc {
  float ce = 0.f, wden = 0.f, nvalid = 0.f, nbad = 0.f;
  float I[K], P[K], Y[K];
  __device__ __forceinline__ SmAcc() {
#pragma unroll
    for (int k = 0; k < K; ++k) I[k] = P[k] = Y[k] = 0.f;
  }
  // branch-free (selects, not products: a non-finite logit of an ignored pixel
  // must not reach the sums): divergent per-pixel branches cost more than the
  // softmax of the few ignored pixels
  // PW: the pixel's own weight pw multiplies the class weight (a compile-time
  // switch: the unweighted instance is the code it was)
  template <bool PW = false>
  __device__ __forceinline__ void add(const float (&z)[K], int y, const float* sw, float pw = 1.f) {
    const bool ok = y >= 0;
    float p[K], nll, S, ru;
    int km;
    softmax_px<K>(z, y, p, nll, km, S, ru);
    const float w = PW ? sw[ok ? y : 0] * pw : sw[ok ? y : 0];
    ce += ok ? w * nll : 0.f;
    wden += ok ? w : 0.f;
    nvalid += ok ? 1.f : 0.f;
    nbad += y == -2 ? 1.f : 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      P[k] += ok ? p[k] : 0.f;
      I[k] += k == y ? p[k] : 0.f;
      Y[k] += k == y ? 1.f : 0.f;
    }
  }
  __device__ __forceinline__ float get(int v) const {  // v is a compile-time constant after unrolling
    if (v == 0) return ce;
    if (v == 1) return wden;
    if (v == 2) return nvalid;
    if (v == 3) return nbad;
    v -= 4;
    return v < K ? I[v] : (v < 2 * K ? P[v - K] : Y[v - 2 * K]);
  }
};

// The NS = 4 + 3 K per-lane sums of a wave, added over its 64 lanes in fp64:
// lane l < NS returns the total of value l.  A butterfly per value would take
// 6 NS shuffle + add steps (312 for K = 16, as much as a thread's whole pixel
// loop); here each step also halves the values a lane carries (the lane keeps
// the half its bit selects and sends the other), W - 1 steps in all for W =
// NS rounded up to 16 / 32 / 64, then the plain butterfly over the remaining
// lane bits.  The order of the additions is fixed.
template <int K>
__device__ __forceinline__ double wave_sums_transposed(const SmAcc<K>& acc, int lane) {
  constexpr int NS = 4 + 3 * K;
  constexpr int W = NS <= 16 ? 16 : (NS <= 32 ? 32 : 64);
  double r[W / 2];
  {
    constexpr int h = W / 2;
    const bool hi = (lane & h) != 0;
#pragma unroll
    for (int i = 0; i < h; ++i) {
      const float a = i < NS ? acc.get(i) : 0.f;
      const float b = i + h < NS ? acc.get(i + h) : 0.f;
      const float keep = hi ? b : a, send = hi ? a : b;
      r[i] = (double)keep + (double)__shfl_xor(send, h, 64);
    }
  }
#pragma unroll
  for (int h = W / 4; h >= 1; h >>= 1) {
    const bool hi = (lane & h) != 0;
#pragma unroll
    for (int i = 0; i < h; ++i) {
      const double keep = hi ? r[i + h] : r[i], send = hi ? r[i] : r[i + h];
      r[i] = keep + __shfl_xor(send, h, 64);
    }
  }
  double t = r[0];  // the total of value lane % W over this group of W lanes
#pragma unroll
  for (int o = W; o < 64; o <<= 1) t += __shfl_xor(t, o, 64);
  return t;
}

// One pixel per lane and step: K dword loads, each wave load one 256-B run of a
// channel plane.  The pass is bound by VALU work and registers (3 K + 4
// partial sums live across the loop), not by load issue: walking 4-pixel
// groups with float4 loads as the other two kernels do needs 150 to 256
// registers and measured slower at every K (16 x K x 512 x 512, K = 2 / 4 / 8 /
// 16: 27.8 / 36.7 / 61.0 / 86.7 us, and 127 to 138 us once the K = 16 instance
// passes 256 registers, against 24.7 / 29.4 / 51.8 / 79.0 us).
template <int K, bool PW>
__global__ void __launch_bounds__(kSmNT) softmax_loss_sums_kernel(const float* __restrict__ x,
                                                                  const void* __restrict__ lab, int dt, int N,
                                                                  int64_t HW, const float* __restrict__ cw,
                                                                  const float* __restrict__ pw, int ign,
                                                                  double* __restrict__ part) {
  constexpr int NS = 4 + 3 * K;
  __shared__ float sw[K];
  __shared__ double red[kSmNT / 64][NS];
  if (threadIdx.x < K) sw[threadIdx.x] = cw ? cw[threadIdx.x] : 1.f;
  __syncthreads();
  SmAcc<K> acc;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const float* xn = x + (size_t)n * K * HW;
    const int64_t lbase = (int64_t)n * HW;
    for (int64_t i = tid; i < HW; i += stride) {
      float z[K];
#pragma unroll
      for (int k = 0; k < K; ++k) z[k] = xn[(size_t)k * HW + i];
      if (PW) acc.template add<true>(z, load_class(lab, dt, lbase + i, K, ign), sw, pw[lbase + i]);
      else acc.add(z, load_class(lab, dt, lbase + i, K, ign), sw);
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double s = wave_sums_transposed<K>(acc, lane);
  if (lane < NS) red[wave][lane] = s;
  __syncthreads();
  // this block's sums (fixed wave order) go to its own slot, value-major so the
  // reduce reads consecutive slots: part[v][slot]
  if (threadIdx.x < NS) {
    double s = 0.0;
    for (int w = 0; w < kSmNT / 64; ++w) s += red[w][threadIdx.x];
    part[(size_t)threadIdx.x * kSmSlots + blockIdx.y * gridDim.x + blockIdx.x] = s;
  }
}

// wave w owns values w, w + 16, ...: the nslot partials of a value are added in
// slot order (64 lanes striding, then a fixed butterfly).  sums[] keeps a fixed
// stride of 16 per class array whatever K is; unused entries are written as 0.
__global__ void __launch_bounds__(1024) softmax_loss_reduce_kernel(double* __restrict__ sums,
                                                                   const double* __restrict__ part, int nslot, int K,
                                                                   int kind, float alpha, float smooth,
                                                                   float* __restrict__ out) {
  __shared__ double tot[kSmSums];
  if (threadIdx.x < kSmSums) tot[threadIdx.x] = 0.0;
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int NS = 4 + 3 * K;
  for (int v = wave; v < NS; v += 16) {
    double a = 0.0;
    for (int b = lane; b < nslot; b += 64) a += part[(size_t)v * kSmSlots + b];
    a = wave_sum_d(a);
    if (lane == 0) tot[v < 4 ? v : 4 + 16 * ((v - 4) / K) + (v - 4) % K] = a;
  }
  __syncthreads();
  if (threadIdx.x < kSmSums) sums[threadIdx.x] = tot[threadIdx.x];
  if (threadIdx.x != 0) return;
  // no valid pixel: CE contributes 0 (torch: NaN)
  const double ce = tot[1] > 0.0 ? tot[0] / tot[1] : 0.0;
  double ratio = 0.0;
  for (int k = 0; k < K; ++k) {
    const double den = tot[20 + k] + tot[36 + k] + smooth;
    ratio += den != 0.0 ? (2.0 * tot[4 + k] + smooth) / den : 1.0;
  }
  const double dice = 1.0 - ratio / K;
  double r;
  if (kind == LOSS_BCE) r = ce;
  else if (kind == LOSS_DICE) r = dice;
  else r = alpha * ce + (1.0 - alpha) * dice;
  *out = (float)r;
}

// dL/dz_k = g (wb w_y (p_k - [y=k]) / w_den + wd p_k (a_k - sum_j p_j a_j)),
// a_j = c_j + [y=j] b_j with c_j = (2 I_j + s) / (K U_j^2), b_j = -2 / (K U_j).
// Both differences cancel for a confident pixel (p_kmax -> 1), so they are
// formed from the small terms: p_kmax - 1 = -S' / (1 + S'), and
// a_k - sum_j p_j a_j = (a_k - a_kmax) - sum_{j != kmax} p_j (a_j - a_kmax).
template <int K>
struct SmGrad {
  float c[K], b[K];  // already scaled by g * wd
  float gce;         // g * wb / w_den
  bool dice;
  template <bool PW = false>
  __device__ __forceinline__ void px(const float (&z)[K], int y, const float* sw, float (&d)[K],
                                     float pw = 1.f) const {
    const bool ok = y >= 0;  // branch-free as SmAcc::add; an ignored pixel's channels are selected to 0 at the end
    float p[K], nll, S, ru;
    int km;
    softmax_px<K>(z, y, p, nll, km, S, ru);
    const float wy = PW ? gce * (sw[ok ? y : 0] * pw) : gce * sw[ok ? y : 0];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float pm1 = k == km ? -S * ru : p[k] - 1.f;
      d[k] = wy * (k == y ? pm1 : p[k]);
    }
    if (dice) {  // uniform
      float a[K], am = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        a[k] = c[k] + (k == y ? b[k] : 0.f);
        if (k == km) am = a[k];
      }
      float dot = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) dot += k == km ? 0.f : p[k] * (a[k] - am);
#pragma unroll
      for (int k = 0; k < K; ++k) d[k] += p[k] * ((a[k] - am) - dot);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) d[k] = ok ? d[k] : 0.f;
  }
};

template <int K, bool PW>
__global__ void __launch_bounds__(kSmNT) softmax_loss_grad_kernel(const float* __restrict__ x,
                                                                  const void* __restrict__ lab, int dt, int N,
                                                                  int64_t HW, const float* __restrict__ cw,
                                                                  const float* __restrict__ pw, int ign,
                                                                  int vec, const double* __restrict__ s, int kind,
                                                                  float alpha, float smooth,
                                                                  const float* __restrict__ gscale,
                                                                  float* __restrict__ dl) {
  constexpr int U = sm_unroll(K);
  __shared__ float sw[K], sc[K], sb[K];
  const float g = gscale ? *gscale : 1.f;
  const float wb = kind == LOSS_BCE ? 1.f : (kind == LOSS_COMBO ? alpha : 0.f);
  const float wd = kind == LOSS_DICE ? 1.f : (kind == LOSS_COMBO ? 1.f - alpha : 0.f);
  if (threadIdx.x < K) {
    const int k = threadIdx.x;
    sw[k] = cw ? cw[k] : 1.f;
    const double Uk = s[20 + k] + s[36 + k] + smooth;
    sc[k] = Uk != 0.0 ? (float)((double)g * wd * (2.0 * s[4 + k] + smooth) / (Uk * Uk * K)) : 0.f;
    sb[k] = Uk != 0.0 ? (float)((double)g * wd * -2.0 / (Uk * K)) : 0.f;
  }
  __syncthreads();
  SmGrad<K> G;
#pragma unroll
  for (int k = 0; k < K; ++k) { G.c[k] = sc[k]; G.b[k] = sb[k]; }
  G.gce = s[1] > 0.0 ? (float)((double)g * wb / s[1]) : 0.f;  // w_den == 0: the CE gradient is 0
  G.dice = wd != 0.f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const float* xn = x + (size_t)n * K * HW;
    float* dn = dl + (size_t)n * K * HW;
    const int64_t lbase = (int64_t)n * HW;
    {
      const int64_t nq = HW >> 2;
      for (int64_t q = tid; q < nq; q += U * stride) {
        float zv[U][K][4];
        float wv[PW ? U : 1][4];  // the pixels' weights, loaded as the logits are
        int yc[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t j = q + u * stride;
          if (j < nq) {
            load_quad<K>(xn, HW, j, vec, zv[u]);
            load_classes4(lab, dt, lbase + 4 * j, K, ign, vec, yc[u]);
            if (PW) {
              const float* p = pw + lbase + 4 * j;
              if (vec) {
                const float4 v = *reinterpret_cast<const float4*>(p);
                wv[PW ? u : 0][0] = v.x; wv[PW ? u : 0][1] = v.y; wv[PW ? u : 0][2] = v.z; wv[PW ? u : 0][3] = v.w;
              } else {
                wv[PW ? u : 0][0] = p[0]; wv[PW ? u : 0][1] = p[1]; wv[PW ? u : 0][2] = p[2]; wv[PW ? u : 0][3] = p[3];
              }
            }
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t j = q + u * stride;
          if (j >= nq) break;
          float dv[K][4];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            float z[K], d[K];
#pragma unroll
            for (int k = 0; k < K; ++k) z[k] = zv[u][k][c];
            if (PW) G.template px<true>(z, yc[u][c], sw, d, wv[PW ? u : 0][c]);
            else G.px(z, yc[u][c], sw, d);
#pragma unroll
            for (int k = 0; k < K; ++k) dv[k][c] = d[k];
          }
#pragma unroll
          for (int k = 0; k < K; ++k) {
            float* o = dn + (size_t)k * HW + 4 * j;
            if (vec) {
              *reinterpret_cast<float4*>(o) = make_float4(dv[k][0], dv[k][1], dv[k][2], dv[k][3]);
            } else {
              o[0] = dv[k][0]; o[1] = dv[k][1]; o[2] = dv[k][2]; o[3] = dv[k][3];
            }
          }
        }
      }
    }
    for (int64_t i = (HW & ~(int64_t)3) + tid; i < HW; i += stride) {  // the HW % 4 last pixels
      float z[K], d[K];
#pragma unroll
      for (int k = 0; k < K; ++k) z[k] = xn[(size_t)k * HW + i];
      if (PW) G.template px<true>(z, load_class(lab, dt, lbase + i, K, ign), sw, d, pw[lbase + i]);
      else G.px(z, load_class(lab, dt, lbase + i, K, ign), sw, d);
#pragma unroll
      for (int k = 0; k < K; ++k) dn[(size_t)k * HW + i] = d[k];
    }
  }
}

// first index of the maximum logit
template <int K>
__device__ __forceinline__ int argmax_px(const float (&z)[K]) {
  float m = z[0];
  int km = 0;
#pragma unroll
  for (int k = 1; k < K; ++k)
    if (z[k] > m) { m = z[k]; km = k; }
  return km;
}

template <int K>
__global__ void __launch_bounds__(kCmNT) confusion_kernel(const float* __restrict__ x, const void* __restrict__ lab,
                                                          int dt, int N, int64_t HW, int ign, int vec,
                                                          unsigned* __restrict__ part) {
  constexpr int U = sm_unroll(K);
  __shared__ unsigned hist[K * K];
  for (int i = threadIdx.x; i < K * K; i += blockDim.x) hist[i] = 0u;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const float* xn = x + (size_t)n * K * HW;
    const int64_t lbase = (int64_t)n * HW;
    {
      const int64_t nq = HW >> 2;
      for (int64_t q = tid; q < nq; q += U * stride) {
        float zv[U][K][4];
        int yc[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t j = q + u * stride;
          if (j < nq) {
            load_quad<K>(xn, HW, j, vec, zv[u]);
            load_classes4(lab, dt, lbase + 4 * j, K, ign, vec, yc[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (q + u * stride >= nq) break;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int y = yc[u][c];
            float z[K];
#pragma unroll
            for (int k = 0; k < K; ++k) z[k] = zv[u][k][c];
            const int pred = argmax_px<K>(z);
            if (y >= 0) atomicAdd(&hist[y * K + pred], 1u);
          }
        }
      }
    }
    for (int64_t i = (HW & ~(int64_t)3) + tid; i < HW; i += stride) {  // the HW % 4 last pixels
      const int y = load_class(lab, dt, lbase + i, K, ign);
      if (y < 0) continue;
      float z[K];
#pragma unroll
      for (int k = 0; k < K; ++k) z[k] = xn[(size_t)k * HW + i];
      atomicAdd(&hist[y * K + argmax_px<K>(z)], 1u);
    }
  }
  __syncthreads();
  // cell-major: part[cell][slot]
  for (int i = threadIdx.x; i < K * K; i += blockDim.x)
    part[(size_t)i * kCmSlots + blockIdx.y * gridDim.x + blockIdx.x] = hist[i];
}

// one wave per cell of cm
__global__ void __launch_bounds__(64) confusion_reduce_kernel(long long* __restrict__ cm,
                                                              const unsigned* __restrict__ part, int nslot) {
  long long a = 0;
  for (int b = threadIdx.x; b < nslot; b += 64) a += (long long)part[(size_t)blockIdx.x * kCmSlots + b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if (threadIdx.x == 0) cm[blockIdx.x] = a;
}

// float4 / packed-label loads need HW % 4 == 0 (every plane then starts on a
// 16-B boundary when the base does) and aligned bases
bool sm_vec_ok(const SoftmaxArgs& a) {
  const uintptr_t lmask = a.label_dtype == SM_LABEL_U8 ? 3 : 15;
  return (a.HW & 3) == 0 && (reinterpret_cast<uintptr_t>(a.logits) & 15) == 0 &&
         (reinterpret_cast<uintptr_t>(a.labels) & lmask) == 0;
}

// grid (gx, gy): gy images in flight, gx blocks per image, gx * gy <= slots
dim3 sm_grid(const SoftmaxArgs& a, int threads, int slots) {
  const int gy = a.N < slots ? a.N : slots;
  const int64_t per_block = (int64_t)threads * 4 * 4;
  int64_t gx = (a.HW + per_block - 1) / per_block;
  const int cap = slots / gy;
  if (gx > cap) gx = cap;
  if (gx < 1) gx = 1;
  return dim3((unsigned)gx, (unsigned)gy);
}

bool sm_args_ok(const SoftmaxArgs& a) {
  return a.logits && a.labels && a.N > 0 && a.HW > 0 && a.K >= 2 && a.K <= kSmMaxK && a.label_dtype >= SM_LABEL_U8 &&
         a.label_dtype <= SM_LABEL_I64;
}

template <int K>
void run_sums(dim3 grid, hipStream_t st, const SoftmaxArgs& a, double* part) {
  if (a.pixel_weights)
    softmax_loss_sums_kernel<K, true><<<grid, dim3(kSmNT), 0, st>>>(a.logits, a.labels, a.label_dtype, a.N, a.HW,
                                                                    a.class_weights, a.pixel_weights,
                                                                    a.ignore_index, part);
  else
    softmax_loss_sums_kernel<K, false><<<grid, dim3(kSmNT), 0, st>>>(a.logits, a.labels, a.label_dtype, a.N, a.HW,
                                                                     a.class_weights, nullptr, a.ignore_index, part);
}
template <int K>
void run_grad(dim3 grid, hipStream_t st, const SoftmaxArgs& a, int vec, const double* sums, int kind, float alpha,
              float smooth, const float* gscale, float* dl) {
  if (a.pixel_weights)
    softmax_loss_grad_kernel<K, true><<<grid, dim3(kSmNT), 0, st>>>(a.logits, a.labels, a.label_dtype, a.N, a.HW,
                                                                    a.class_weights, a.pixel_weights,
                                                                    a.ignore_index, vec, sums, kind, alpha, smooth,
                                                                    gscale, dl);
  else
    softmax_loss_grad_kernel<K, false><<<grid, dim3(kSmNT), 0, st>>>(a.logits, a.labels, a.label_dtype, a.N, a.HW,
                                                                     a.class_weights, nullptr, a.ignore_index, vec,
                                                                     sums, kind, alpha, smooth, gscale, dl);
}
template <int K>
void run_confusion(dim3 grid, hipStream_t st, const SoftmaxArgs& a, int vec, unsigned* part) {
  confusion_kernel<K><<<grid, dim3(kCmNT), 0, st>>>(a.logits, a.labels, a.label_dtype, a.N, a.HW, a.ignore_index,
                                                    vec, part);
}

// FN<K>(...) for the run-time K (2..16: checked by sm_args_ok)
#define SM_CASE(KK, FN, ...) case KK: FN<KK>(__VA_ARGS__); break;
#define SM_DISPATCH(k, FN, ...)                                                                      \
  switch (k) {                                                                                       \
    SM_CASE(2, FN, __VA_ARGS__) SM_CASE(3, FN, __VA_ARGS__) SM_CASE(4, FN, __VA_ARGS__)              \
    SM_CASE(5, FN, __VA_ARGS__) SM_CASE(6, FN, __VA_ARGS__) SM_CASE(7, FN, __VA_ARGS__)              \
    SM_CASE(8, FN, __VA_ARGS__) SM_CASE(9, FN, __VA_ARGS__) SM_CASE(10, FN, __VA_ARGS__)             \
    SM_CASE(11, FN, __VA_ARGS__) SM_CASE(12, FN, __VA_ARGS__) SM_CASE(13, FN, __VA_ARGS__)           \
    SM_CASE(14, FN, __VA_ARGS__) SM_CASE(15, FN, __VA_ARGS__) SM_CASE(16, FN, __VA_ARGS__)           \
    default: return hipErrorInvalidValue;                                                            \
  }

}  // namespace

hipError_t launch_softmax_loss_sums(const SoftmaxArgs& a, int kind, float alpha, float smooth, double* sums,
                                    double* part, float* out, hipStream_t st) {
  if (!sm_args_ok(a) || !sums || !part || !out || (kind == LOSS_DICE && a.pixel_weights)) return hipErrorInvalidValue;
  const dim3 grid = sm_grid(a, kSmNT, kSmSlots);
  SM_DISPATCH(a.K, run_sums, grid, st, a, part)
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(softmax_loss_reduce_kernel, dim3(1), dim3(1024), 0, st, sums, part, (int)(grid.x * grid.y), a.K,
                     kind, alpha, smooth, out);
  return hipGetLastError();
}

hipError_t launch_softmax_loss_grad(const SoftmaxArgs& a, int kind, float alpha, float smooth, const double* sums,
                                    const float* gscale, float* dl, hipStream_t st) {
  if (!sm_args_ok(a) || !sums || !dl || (kind == LOSS_DICE && a.pixel_weights)) return hipErrorInvalidValue;
  const dim3 grid = sm_grid(a, kSmNT, 4096);
  const int vec = sm_vec_ok(a) && (reinterpret_cast<uintptr_t>(dl) & 15) == 0 &&
                          (reinterpret_cast<uintptr_t>(a.pixel_weights) & 15) == 0
                      ? 1
                      : 0;
  SM_DISPATCH(a.K, run_grad, grid, st, a, vec, sums, kind, alpha, smooth, gscale, dl)
  return hipGetLastError();
}

hipError_t launch_confusion(const SoftmaxArgs& a, long long* cm, unsigned* part, hipStream_t st) {
  if (!sm_args_ok(a) || !cm || !part) return hipErrorInvalidValue;
  const dim3 grid = sm_grid(a, kCmNT, kCmSlots);
  const int vec = sm_vec_ok(a) ? 1 : 0;
  SM_DISPATCH(a.K, run_confusion, grid, st, a, vec, part)
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(confusion_reduce_kernel, dim3(a.K * a.K), dim3(64), 0, st, cm, part, (int)(grid.x * grid.y));
  return hipGetLastError();
}

}  // namespace unet
