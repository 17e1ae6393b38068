// C ABI of the single ops (include/unet_hip.h): argument checks, the kernel
// argument block, then the launcher as the executor calls it.
#include <cstdarg>
#include <cstdio>

#include "plan.h"

namespace {

// set_err with a printf format; false, for `return errf(...)` in a check
__attribute__((format(printf, 1, 2))) bool errf(const char* fmt, ...) {
  char m[256];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(m, sizeof(m), fmt, ap);
  va_end(ap);
  set_err(m);
  return false;
}

// operands and geometry of a conv launch from the raw ABI arguments
ConvFwdArgs conv_args(const void* x, int ldx, const void* w, void* y, int ldy, int N, int H, int W, int C, int P,
                      int Q, int Cout, int R, int S, int stride, int pad) {
  ConvFwdArgs a = {};
  a.x = (const bf16_t*)x; a.ldx = ldx; a.w = (const bf16_t*)w; a.y = (bf16_t*)y; a.ldy = ldy;
  a.N = N; a.H = H; a.W = W; a.C = C; a.P = P; a.Q = Q; a.Cout = Cout;
  a.R = R; a.S = S; a.stride = stride; a.pad = pad;
  return a;
}

ConvWgradArgs wgrad_args(const void* dy, int lddy, const void* x, int ldx, float* dw, int N, int H, int W, int C,
                         int P, int Q, int Cout, int R, int S, int stride, int pad) {
  ConvWgradArgs a = {};
  a.dy = (const bf16_t*)dy; a.lddy = lddy; a.x = (const bf16_t*)x; a.ldx = ldx; a.dw = dw;
  a.N = N; a.H = H; a.W = W; a.C = C; a.P = P; a.Q = Q; a.Cout = Cout;
  a.R = R; a.S = S; a.stride = stride; a.pad = pad;
  return a;
}

// the fused BN(+ReLU) backward of a data-gradient epilogue: one BN, ...
BnBwdArgs bb_args(const void* act, int ldact, const void* yraw, int ldyraw, const float* mean, const float* invstd,
                  double* sums, int64_t npix, int C) {
  BnBwdArgs b = {};
  b.act = (const bf16_t*)act; b.ldact = ldact; b.y = (const bf16_t*)yraw; b.ldy = ldyraw;
  b.mean = mean; b.invstd = invstd; b.sums = sums;
  b.npix = npix; b.C = C; b.relu = 1;
  return b;
}
// ... and the second BN of out = relu(bn(y) + bn2(y2))
void bb_second(BnBwdArgs& b, const void* yraw2, int ldyraw2, const float* mean2, const float* invstd2,
               double* sums2) {
  b.y2 = (const bf16_t*)yraw2; b.ldy2 = ldyraw2; b.mean2 = mean2; b.invstd2 = invstd2; b.sums2 = sums2;
}

bool workspace_ok(const char* fn, const char* sizer_name, const void* workspace, int64_t bytes, int64_t need) {
  if (workspace && bytes >= need) return true;
  return errf("%s: workspace null or workspace_bytes %lld < %s (%lld)", fn, (long long)bytes, sizer_name,
              (long long)need);
}

}  // namespace

extern "C" {

static_assert(UNET_LOSS_SCRATCH_LEN == 8 * kLossBlocks, "loss partial slots");

static bool loss_bufs_ok(const char* fn, const double* sums8, const double* scratch, int64_t scratch_len) {
  if (sums8 && scratch && scratch_len >= UNET_LOSS_SCRATCH_LEN) return true;
  return errf("%s: sums8 / scratch null or scratch_len %lld < UNET_LOSS_SCRATCH_LEN (%d)", fn,
              (long long)scratch_len, UNET_LOSS_SCRATCH_LEN);
}

int unet_loss_forward(const float* logits, const float* target, int64_t n, int kind, float alpha, float smooth,
                      double* sums8, double* scratch, int64_t scratch_len, float* loss_out, hipStream_t stream) {
  if (!loss_bufs_ok("unet_loss_forward", sums8, scratch, scratch_len)) return 1;
  CK(launch_loss_sums(logits, target, n, sums8, scratch, 0, kind, alpha, smooth, loss_out, stream));
  return 0;
}

int unet_loss_backward(const float* logits, const float* target, int64_t n, int kind, float alpha, float smooth,
                       const double* sums8, const float* grad_scale, float* dlogits, hipStream_t stream) {
  CK(launch_loss_grad(logits, target, n, sums8, kind, alpha, smooth, grad_scale, dlogits, stream));
  return 0;
}

int unet_mask_metrics(const float* values, const float* target, int64_t n, int values_are_prob, double* sums8,
                      double* scratch, int64_t scratch_len, hipStream_t stream) {
  if (!loss_bufs_ok("unet_mask_metrics", sums8, scratch, scratch_len)) return 1;
  CK(launch_loss_sums(values, target, n, sums8, scratch, values_are_prob, 0, 0.f, 0.f, nullptr, stream));
  return 0;
}

static_assert(UNET_SOFTMAX_MAX_CLASSES == kSmMaxK && UNET_SOFTMAX_SUMS_LEN == kSmSums &&
                  UNET_SOFTMAX_MAX_BLOCKS == kSmSlots && UNET_SOFTMAX_THREADS == kSmNT,
              "softmax loss geometry");
static_assert((size_t)UNET_SOFTMAX_SCRATCH_LEN * sizeof(double) >=
                  (size_t)kSmMaxK * kSmMaxK * kCmSlots * sizeof(unsigned),
              "the confusion histograms fit the softmax scratch");

// the argument checks shared by the three softmax entry points
static bool softmax_args_ok(const char* fn, const void* logits, const void* labels, int label_dtype, int N, int K,
                            int64_t HW) {
  if (!logits || !labels) return errf("%s: logits / labels is null", fn);
  if (K < 2 || K > UNET_SOFTMAX_MAX_CLASSES)
    return errf("%s: K = %d is outside 2..%d", fn, K, UNET_SOFTMAX_MAX_CLASSES);
  if (label_dtype < 0 || label_dtype > 2)
    return errf("%s: label_dtype %d is not 0 (uint8), 1 (int32) or 2 (int64)", fn, label_dtype);
  // 2^38 pixels: the per-block uint32 histogram counts and the fp32 per-thread counts stay exact
  if (N <= 0 || HW <= 0 || HW > ((int64_t)1 << 38) / N)
    return errf("%s: N = %d, HW = %lld must be positive with N * HW <= 2^38", fn, N, (long long)HW);
  return true;
}

static bool softmax_kind_ok(const char* fn, int kind, const float* class_weights) {
  if (kind < LOSS_BCE || kind > LOSS_COMBO) return errf("%s: kind %d is not 0 (ce), 1 (dice) or 2 (combo)", fn, kind);
  if (kind == LOSS_DICE && class_weights)
    return errf("%s: class weights apply to the CE term; kind 1 (dice) takes none", fn);
  return true;
}

static bool softmax_scratch_ok(const char* fn, const void* scratch, int64_t scratch_len) {
  if (scratch && scratch_len >= UNET_SOFTMAX_SCRATCH_LEN) return true;
  return errf("%s: scratch null or scratch_len %lld < UNET_SOFTMAX_SCRATCH_LEN (%d)", fn, (long long)scratch_len,
              UNET_SOFTMAX_SCRATCH_LEN);
}

int unet_softmax_loss_forward(const float* logits, const void* labels, int label_dtype, int N, int K, int64_t HW,
                              const float* class_weights, int ignore_index, int kind, float alpha, float smooth,
                              double* sums, double* scratch, int64_t scratch_len, float* loss_out,
                              hipStream_t stream) {
  const char* fn = "unet_softmax_loss_forward";
  if (!softmax_args_ok(fn, logits, labels, label_dtype, N, K, HW) || !softmax_kind_ok(fn, kind, class_weights) ||
      !softmax_scratch_ok(fn, scratch, scratch_len))
    return 1;
  if (!sums || !loss_out) { set_err("unet_softmax_loss_forward: sums / loss_out is null"); return 1; }
  const SoftmaxArgs a{logits, labels, label_dtype, N, K, HW, class_weights, ignore_index};
  CK(launch_softmax_loss_sums(a, kind, alpha, smooth, sums, scratch, loss_out, stream));
  return 0;
}

int unet_softmax_loss_backward(const float* logits, const void* labels, int label_dtype, int N, int K, int64_t HW,
                               const float* class_weights, int ignore_index, int kind, float alpha, float smooth,
                               const double* sums, const float* grad_scale, float* dlogits, hipStream_t stream) {
  const char* fn = "unet_softmax_loss_backward";
  if (!softmax_args_ok(fn, logits, labels, label_dtype, N, K, HW) || !softmax_kind_ok(fn, kind, class_weights))
    return 1;
  if (!sums || !dlogits) { set_err("unet_softmax_loss_backward: sums / dlogits is null"); return 1; }
  const SoftmaxArgs a{logits, labels, label_dtype, N, K, HW, class_weights, ignore_index};
  CK(launch_softmax_loss_grad(a, kind, alpha, smooth, sums, grad_scale, dlogits, stream));
  return 0;
}

static bool softmax_pw_ok(const char* fn, int kind, const float* pixel_weights) {
  if (kind == LOSS_DICE && pixel_weights)
    return errf("%s: pixel weights apply to the CE term; kind 1 (dice) takes none", fn);
  return true;
}

int unet_softmax_loss_forward_pw(const float* logits, const void* labels, int label_dtype, int N, int K, int64_t HW,
                                 const float* class_weights, const float* pixel_weights, int ignore_index, int kind,
                                 float alpha, float smooth, double* sums, double* scratch, int64_t scratch_len,
                                 float* loss_out, hipStream_t stream) {
  const char* fn = "unet_softmax_loss_forward_pw";
  if (!softmax_args_ok(fn, logits, labels, label_dtype, N, K, HW) || !softmax_kind_ok(fn, kind, class_weights) ||
      !softmax_pw_ok(fn, kind, pixel_weights) || !softmax_scratch_ok(fn, scratch, scratch_len))
    return 1;
  if (!sums || !loss_out) { set_err("unet_softmax_loss_forward_pw: sums / loss_out is null"); return 1; }
  const SoftmaxArgs a{logits, labels, label_dtype, N, K, HW, class_weights, ignore_index, pixel_weights};
  CK(launch_softmax_loss_sums(a, kind, alpha, smooth, sums, scratch, loss_out, stream));
  return 0;
}

int unet_softmax_loss_backward_pw(const float* logits, const void* labels, int label_dtype, int N, int K, int64_t HW,
                                  const float* class_weights, const float* pixel_weights, int ignore_index, int kind,
                                  float alpha, float smooth, const double* sums, const float* grad_scale,
                                  float* dlogits, hipStream_t stream) {
  const char* fn = "unet_softmax_loss_backward_pw";
  if (!softmax_args_ok(fn, logits, labels, label_dtype, N, K, HW) || !softmax_kind_ok(fn, kind, class_weights) ||
      !softmax_pw_ok(fn, kind, pixel_weights))
    return 1;
  if (!sums || !dlogits) { set_err("unet_softmax_loss_backward_pw: sums / dlogits is null"); return 1; }
  const SoftmaxArgs a{logits, labels, label_dtype, N, K, HW, class_weights, ignore_index, pixel_weights};
  CK(launch_softmax_loss_grad(a, kind, alpha, smooth, sums, grad_scale, dlogits, stream));
  return 0;
}

int unet_confusion_matrix(const float* logits, const void* labels, int label_dtype, int N, int K, int64_t HW,
                          int ignore_index, long long* cm, double* scratch, int64_t scratch_len,
                          hipStream_t stream) {
  const char* fn = "unet_confusion_matrix";
  if (!softmax_args_ok(fn, logits, labels, label_dtype, N, K, HW) || !softmax_scratch_ok(fn, scratch, scratch_len))
    return 1;
  if (!cm) { set_err("unet_confusion_matrix: cm is null"); return 1; }
  const SoftmaxArgs a{logits, labels, label_dtype, N, K, HW, nullptr, ignore_index};
  CK(launch_confusion(a, cm, reinterpret_cast<unsigned*>(scratch), stream));
  return 0;
}

int unet_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* step_coef,
                   int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                   int advance_step, hipStream_t stream) {
  if (n < 0 || (n > 0 && (!params || !grads || !exp_avg || !exp_avg_sq)) || !step_coef) {
    set_err("unet_adam_step: null buffer or negative size");
    return 1;
  }
  CK(launch_adam(params, grads, exp_avg, exp_avg_sq, n, step_coef, lr, beta1, beta2, eps, weight_decay, advance_step, stream));
  return 0;
}

int unet_grad_to_bf16(const float* src, void* dst, int64_t n, hipStream_t stream) {
  if (n < 0 || (n > 0 && (!src || !dst))) {
    set_err("unet_grad_to_bf16: null buffer or negative size");
    return 1;
  }
  CK(launch_grad_to_bf16(src, (bf16_t*)dst, n, stream));
  return 0;
}

int unet_grad_from_bf16(const void* src, float* dst, int64_t n, float scale, hipStream_t stream) {
  if (n < 0 || (n > 0 && (!src || !dst))) {
    set_err("unet_grad_from_bf16: null buffer or negative size");
    return 1;
  }
  CK(launch_grad_from_bf16((const bf16_t*)src, dst, n, scale, stream));
  return 0;
}

// the stem kernels work on 64-channel output groups (unet_conv_fwd mode 2, unet_conv_wgrad* stem = 1)
static bool stem_width_ok(const char* fn, int Cout) {
  if (Cout > 0 && Cout % 64 == 0) return true;
  set_err(std::string(fn) + ": the stem needs Cout % 64 == 0");
  return false;
}

int unet_conv_fwd(const void* x, int ldx, const void* w, void* y, int ldy, const float* bias, const void* addend,
                  int ldadd, double* stats, int N, int H, int W, int C, int P, int Q, int Cout, int R, int S,
                  int stride, int pad, int mode, hipStream_t stream) {
  ConvFwdArgs a = conv_args(x, ldx, w, y, ldy, N, H, W, C, P, Q, Cout, R, S, stride, pad);
  a.bias = bias; a.add = (const bf16_t*)addend; a.ldadd = ldadd; a.stats = stats;
  if (mode < 0 || mode > 2) { set_err("bad mode"); return 1; }
  if (mode == MODE_STEM && !stem_width_ok("unet_conv_fwd", Cout)) return 1;
  CK(launch_conv_fwd(a, mode, stream));
  return 0;
}

int unet_convt2x2(const void* x, int ldx, const void* w, void* y, int ldy, const float* bias, const void* act,
                  int ldact, const void* yraw, int ldyraw, const float* mean, const float* invstd, double* bsums,
                  double* bias_acc, int N, int H, int W, int Ci, int Co, int mode, int grid, hipStream_t stream) {
  if (mode != 0 && mode != 1) { set_err("unet_convt2x2: mode must be 0 (forward) or 1 (data gradient)"); return 1; }
  if (mode == 0 && (bsums || bias_acc)) { set_err("unet_convt2x2: bsums / bias_acc belong to the data gradient"); return 1; }
  if (bsums && (!act || !yraw || !mean || !invstd)) {
    set_err("unet_convt2x2: fused BN backward needs act, yraw, mean, invstd");
    return 1;
  }
  ConvFwdArgs a = conv_args(x, ldx, w, y, ldy, N, H, W, Ci, 2 * H, 2 * W, Co, 2, 2, 2, 0);
  a.bias = mode == 0 ? bias : nullptr;
  a.grid_cap = grid;
  a.bias_acc = bias_acc;
  if (bsums) a.bb = bb_args(act, ldact, yraw, ldyraw, mean, invstd, bsums, (int64_t)N * H * W, Ci);
  const hipError_t e = launch_convt2x2(a, mode, stream);
  if (e == hipErrorNotSupported) {
    set_err("unet_convt2x2: shape / alignment not covered ((Ci, Co) in {(64,32),(64,64),(128,64)}, N*H*W % 32)");
    return 1;
  }
  CK(e);
  return 0;
}

int unet_conv3x3_fl(const void* x, int ldx, const void* wch, void* y, int ldy, const float* bias, const void* addend,
                    int ldadd, double* stats, const void* act, int ldact, const void* yraw, int ldyraw,
                    const float* mean, const float* invstd, const void* yraw2, int ldyraw2, const float* mean2,
                    const float* invstd2, double* bsums, double* bsums2, int N, int H, int W, int C, int Cout,
                    int mode, int grid, hipStream_t stream) {
  if (mode != 0 && mode != 1) { set_err("unet_conv3x3_fl: mode must be 0 (conv) or 1 (data gradient)"); return 1; }
  if (!conv3x3_fl_geom(C, Cout, H, W) || N <= 0) {
    set_err("unet_conv3x3_fl: needs C % 128 == 0, Cout % 64 == 0, H % 16 == 0, W % 16 == 0, N > 0");
    return 1;
  }
  if (mode == 0 && bsums) { set_err("unet_conv3x3_fl: the fused BN backward is a data-gradient epilogue"); return 1; }
  if (bsums && (!act || !yraw || !mean || !invstd || (yraw2 && (!mean2 || !invstd2 || !bsums2)))) {
    set_err("unet_conv3x3_fl: fused BN backward needs act, yraw, mean, invstd (and mean2, invstd2, bsums2 with yraw2)");
    return 1;
  }
  ConvFwdArgs a = conv_args(x, ldx, nullptr, y, ldy, N, H, W, C, H, W, Cout, 3, 3, 1, 1);
  a.wch = (const bf16_t*)wch;  // only conv3x3_fl_kernel reads this pack
  a.bias = bias; a.add = (const bf16_t*)addend; a.ldadd = ldadd; a.stats = mode == 0 ? stats : nullptr;
  a.grid_cap = grid;
  if (bsums) {
    a.bb = bb_args(act, ldact, yraw, ldyraw, mean, invstd, bsums, (int64_t)N * H * W, Cout);
    if (yraw2) bb_second(a.bb, yraw2, ldyraw2, mean2, invstd2, bsums2);
  }
  CK(launch_conv3x3_fl(a, mode, stream));
  return 0;
}

const char* unet_last_kernel_tag(void) { return unet::last_kernel_tag(); }

int unet_conv_ex(const unet_conv_ex_args* p, hipStream_t stream) {
  conv_kernel_tag("");  // a refused call leaves no stale instance name behind
  auto bad = [](const char* m) { set_err(std::string("unet_conv_ex: ") + m); return 1; };
  if (!p || p->size != (int)sizeof(unet_conv_ex_args)) return bad("null argument or size != sizeof(unet_conv_ex_args)");
  const unet_conv_ex_args& e = *p;
  if (e.mode != 0 && e.mode != 1) return bad("mode must be 0 (forward) or 1 (data gradient)");
  if (!e.x || !e.w || !e.y) return bad("x, w, y must be set");
  if (e.N <= 0 || e.H <= 0 || e.W <= 0 || e.C <= 0 || e.P <= 0 || e.Q <= 0 || e.Cout <= 0 || e.R <= 0 || e.S <= 0 ||
      e.stride <= 0 || e.pad < 0)
    return bad("N, H, W, C, P, Q, Cout, R, S, stride must be positive");
  if (e.C % 32 || e.Cout % 4) return bad("needs C % 32 == 0 and Cout % 4 == 0");
  if (e.grid_cap < 0) return bad("grid_cap must be >= 0");
  const bool fwd = e.mode == 0;
  const bool bbany = e.act || e.yraw || e.mean || e.invstd || e.yraw2 || e.mean2 || e.invstd2 || e.bsums || e.bsums2 ||
                     e.ldact || e.ldyraw || e.ldyraw2;
  const bool foldany = e.gamma || e.beta || e.running_mean || e.running_var || e.eps != 0.f || e.relu;
  const bool dsany = e.wds || e.yds || e.stats_ds || e.ldyds;
  const bool x2any = e.x2 || e.w2 || e.C2 || e.ldx2;
  const bool splitany = e.ysplit || e.ldysplit || e.csplit;
  if (fwd && (bbany || x2any || splitany))
    return bad("the fused BN backward, x2 / w2 and ysplit belong to the data gradient (mode 1)");
  if (!fwd && (e.bias || e.stats || foldany || dsany))
    return bad("bias, stats, the eval BN fold and wds / yds belong to the forward (mode 0)");
  if (e.ldx < e.C) return bad("ldx < C");
  if (e.ldy < (e.ysplit ? e.csplit : e.Cout)) return bad("ldy smaller than the channels stored to y");
  if ((e.addend != nullptr) != (e.ldadd != 0) || (e.addend && e.ldadd < e.Cout)) return bad("addend needs ldadd >= Cout");
  if (bbany) {
    if (!e.bsums || !e.act || !e.yraw || !e.mean || !e.invstd || e.ldact < e.Cout || e.ldyraw < e.Cout)
      return bad("the fused BN backward needs bsums, act, yraw, mean, invstd, ldact / ldyraw >= Cout");
    const bool two = e.yraw2 || e.mean2 || e.invstd2 || e.bsums2 || e.ldyraw2;
    if (two && (!e.yraw2 || !e.mean2 || !e.invstd2 || !e.bsums2 || e.ldyraw2 < e.Cout))
      return bad("the two-BN form needs yraw2, mean2, invstd2, bsums2, ldyraw2 >= Cout");
  }
  if (x2any && (!e.x2 || !e.w2 || e.C2 <= 0 || e.ldx2 < e.C2)) return bad("x2 needs w2, C2 > 0, ldx2 >= C2");
  if (splitany) {
    if (!e.ysplit || e.csplit <= 0 || e.csplit >= e.Cout || e.ldysplit < e.Cout - e.csplit)
      return bad("ysplit needs 0 < csplit < Cout and ldysplit >= Cout - csplit");
    if (e.addend || bbany) return bad("ysplit does not combine with addend or the fused BN backward");
  }
  if (foldany) {
    if (!e.gamma || !e.beta || !e.running_mean || !e.running_var || !(e.eps > 0.f))
      return bad("the eval BN fold needs gamma, beta, running_mean, running_var, eps > 0 (relu only with them)");
    if (e.stats) return bad("the eval BN fold does not combine with BN sums");
  }
  if (dsany && (!e.wds || !e.yds || e.ldyds < e.Cout)) return bad("wds needs yds, ldyds >= Cout");
  if (e.chunk_major && (x2any || splitany || dsany)) return bad("the chunk-major launch has no x2, ysplit or wds");

  ConvFwdArgs a = conv_args(e.x, e.ldx, e.w, e.y, e.ldy, e.N, e.H, e.W, e.C, e.P, e.Q, e.Cout, e.R, e.S, e.stride,
                            e.pad);
  a.bias = e.bias; a.add = (const bf16_t*)e.addend; a.ldadd = e.ldadd; a.stats = e.stats;
  a.grid_cap = e.grid_cap;
  if (bbany) {
    a.bb = bb_args(e.act, e.ldact, e.yraw, e.ldyraw, e.mean, e.invstd, e.bsums, (int64_t)e.N * e.P * e.Q, e.Cout);
    if (e.yraw2) bb_second(a.bb, e.yraw2, e.ldyraw2, e.mean2, e.invstd2, e.bsums2);
  }
  if (x2any) { a.x2 = (const bf16_t*)e.x2; a.ldx2 = e.ldx2; a.w2 = (const bf16_t*)e.w2; a.C2 = e.C2; }
  if (splitany) { a.ysplit = (bf16_t*)e.ysplit; a.ldysplit = e.ldysplit; a.csplit = e.csplit; }
  if (foldany) {
    a.fold.gamma = e.gamma; a.fold.beta = e.beta;
    a.fold.run_mean = const_cast<float*>(e.running_mean); a.fold.run_var = const_cast<float*>(e.running_var);
    a.fold.count = (double)e.N * e.P * e.Q; a.fold.C = e.Cout; a.fold.eps = e.eps; a.fold.training = 0;
    a.fold_on = 1; a.fold_relu = e.relu ? 1 : 0;
  }
  auto refused = [&](hipError_t err) {
    set_err(std::string("unet_conv_ex: the launcher refused this combination (") + hipGetErrorString(err) + ")");
    return (int)err;
  };
  if (e.chunk_major) {  // only conv3x3_fl_kernel reads this pack
    a.wch = a.w;
    a.w = nullptr;
    const hipError_t err = launch_conv3x3_fl(a, e.mode, stream);
    return err == hipSuccess ? 0 : refused(err);
  }
  if (dsany) {  // as conv_fwd: folded where launch_conv_fwd folds; the executor would launch the two separately
    a.wds = (const bf16_t*)e.wds; a.yds = (bf16_t*)e.yds; a.ldyds = e.ldyds; a.stats_ds = e.stats_ds;
    if (!conv_fwd_ds_ok(a)) return bad("the downsample fold does not cover this shape / epilogue");
    const hipError_t err = launch_conv_fwd(a, MODE_FWD, stream);
    return err == hipSuccess ? 0 : refused(err);
  }
  if (e.R == 1 && e.S == 1 && e.stride == 1 && (fwd || !bbany)) {  // weight-stationary 1x1 where covered
    const hipError_t err = launch_conv1x1(a, e.mode, stream);
    if (err != hipErrorNotSupported) return err == hipSuccess ? 0 : refused(err);
  }
  const hipError_t err = launch_conv_fwd(a, fwd ? MODE_FWD : MODE_TRANS, stream);
  return err == hipSuccess ? 0 : refused(err);
}

// ---- attention single ops: argument checks, then the launcher's pass as it is ----
namespace {
// the checks shared by unet_att_gate_op / unet_ch_att_op; the first failure is kept
struct OpCheck {
  const char* fn;
  bool ok = true;
  int fail(const std::string& m) {
    if (ok) set_err(std::string(fn) + ": " + m);
    ok = false;
    return 1;
  }
  void ptr(const void* q, const char* name, int pass) {
    if (ok && !q) fail(std::string(name) + " is null (pass " + std::to_string(pass) + " uses it)");
  }
  // a bf16 NHWC tensor read / written as 16-B chunks of 8 channels
  void act(const void* q, int ld, int width, const char* name, const char* ldname, int pass) {
    ptr(q, name, pass);
    if (ok && ((uintptr_t)q & 15)) fail(std::string(name) + " must be 16-byte aligned");
    if (ok && ld < width) fail(std::string(ldname) + " is smaller than the width " + std::to_string(width));
    if (ok && ld % 8) fail(std::string(ldname) + " must be a multiple of 8");
  }
};
}  // namespace

int unet_att_gate_op(const unet_att_gate_args* p, hipStream_t stream) {
  OpCheck k{"unet_att_gate_op"};
  if (!p || p->size != (int)sizeof(unet_att_gate_args)) return k.fail("null argument or size != sizeof(unet_att_gate_args)");
  const unet_att_gate_args& e = *p;
  const int ps = e.pass;
  if (ps < 0 || ps > 3) return k.fail("pass must be 0..3");
  if (e.training != 0 && e.training != 1) return k.fail("training must be 0 or 1");
  if (e.npix <= 0) return k.fail("npix must be positive");
  auto width_ok = [](int F) { return F >= 8 && F % 8 == 0 && 64 % (F / 8) == 0; };
  if (!width_ok(e.Fi)) return k.fail("Fi / 8 must divide 64 (Fi = 8, 16, 32, 64, 128, 256 or 512)");
  if (!width_ok(e.Fl)) return k.fail("Fl / 8 must divide 64 (Fl = 8, 16, 32, 64, 128, 256 or 512)");
  const bool bbany = e.yraw || e.yraw2 || e.mean || e.invstd || e.mean2 || e.invstd2 || e.bsums || e.bsums2 ||
                     e.ldyraw || e.ldyraw2;
  if (ps == 0) {
    k.act(e.s, e.lds, e.Fi, "s", "lds", ps);
    k.ptr(e.psi_w, "psi_w", ps); k.ptr(e.psi_b, "psi_b", ps); k.ptr(e.p, "p", ps);
    if (e.training) k.ptr(e.pst, "pst", ps);
  } else if (ps == 1) {
    k.ptr(e.p, "p", ps); k.ptr(e.psi, "psi", ps); k.ptr(e.gamma, "gamma", ps); k.ptr(e.beta, "beta", ps);
    k.ptr(e.run_mean, "run_mean", ps); k.ptr(e.run_var, "run_var", ps);
    if (e.training) { k.ptr(e.pst, "pst", ps); k.ptr(e.save, "save", ps); }
    k.act(e.x, e.ldx, e.Fl, "x", "ldx", ps);
    k.act(e.xatt, e.ldxatt, e.Fl, "xatt", "ldxatt", ps);
    if (k.ok && !(e.eps > 0.f)) k.fail("eps must be > 0");
  } else if (ps == 2) {
    k.ptr(e.save, "save", ps); k.ptr(e.psi, "psi", ps); k.ptr(e.p, "p", ps); k.ptr(e.dbnp, "dbnp", ps);
    k.ptr(e.pbs, "pbs", ps);
    k.act(e.x, e.ldx, e.Fl, "x", "ldx", ps);
    k.act(e.dxatt, e.lddxatt, e.Fl, "dxatt", "lddxatt", ps);
    k.act(e.dxpsi, e.lddxpsi, e.Fl, "dxpsi", "lddxpsi", ps);
  } else {
    k.ptr(e.save, "save", ps); k.ptr(e.pbs, "pbs", ps); k.ptr(e.gamma, "gamma", ps); k.ptr(e.psi_w, "psi_w", ps);
    k.ptr(e.p, "p", ps); k.ptr(e.dbnp, "dbnp", ps); k.ptr(e.gpsi_acc, "gpsi_acc", ps); k.ptr(e.gpsi_w, "gpsi_w", ps);
    k.ptr(e.ggamma, "ggamma", ps); k.ptr(e.gbeta, "gbeta", ps);
    k.act(e.s, e.lds, e.Fi, "s", "lds", ps);
    k.act(e.dS, e.lddS, e.Fi, "dS", "lddS", ps);
    if (k.ok && bbany) {
      if (!e.bsums || !e.bsums2 || !e.mean || !e.invstd || !e.mean2 || !e.invstd2 || !e.yraw || !e.yraw2)
        return k.fail("the fused BN backward (bb) needs all of yraw, yraw2, mean, invstd, mean2, invstd2, bsums, bsums2");
      k.act(e.yraw, e.ldyraw, e.Fi, "yraw", "ldyraw", ps);
      k.act(e.yraw2, e.ldyraw2, e.Fi, "yraw2", "ldyraw2", ps);
    }
  }
  if (!k.ok) return 1;

  AttGateArgs a = {};
  a.s = (const bf16_t*)e.s; a.lds = e.lds; a.psi_w = e.psi_w; a.psi_b = e.psi_b;
  a.p = e.p; a.psi = e.psi; a.dbnp = e.dbnp; a.pst = e.pst; a.pbs = e.pbs; a.save = e.save;
  a.gamma = e.gamma; a.beta = e.beta; a.run_mean = e.run_mean; a.run_var = e.run_var; a.nbt = e.nbt;
  a.count = (double)e.npix; a.eps = e.eps; a.momentum = e.momentum; a.training = e.training;
  a.x = (const bf16_t*)e.x; a.ldx = e.ldx; a.xatt = (bf16_t*)e.xatt; a.ldxatt = e.ldxatt;
  a.dxatt = (const bf16_t*)e.dxatt; a.lddxatt = e.lddxatt; a.dxpsi = (bf16_t*)e.dxpsi; a.lddxpsi = e.lddxpsi;
  a.dS = (bf16_t*)e.dS; a.lddS = e.lddS;
  a.gpsi_w = e.gpsi_w; a.ggamma = e.ggamma; a.gbeta = e.gbeta; a.gpsi_acc = e.gpsi_acc;
  if (ps == 3 && bbany) {
    a.bb = bb_args(a.s, a.lds, e.yraw, e.ldyraw, e.mean, e.invstd, e.bsums, e.npix, e.Fi);
    bb_second(a.bb, e.yraw2, e.ldyraw2, e.mean2, e.invstd2, e.bsums2);
  }
  a.npix = e.npix; a.Fi = e.Fi; a.Fl = e.Fl;
  const hipError_t err = launch_att_gate(a, ps, stream);
  if (err != hipSuccess) {
    set_err(std::string("unet_att_gate_op: launch_att_gate pass ") + std::to_string(ps) + " -> " + hipGetErrorString(err));
    return (int)err;
  }
  return 0;
}

int unet_ch_att_op(const unet_ch_att_args* p, hipStream_t stream) {
  OpCheck k{"unet_ch_att_op"};
  if (!p || p->size != (int)sizeof(unet_ch_att_args)) return k.fail("null argument or size != sizeof(unet_ch_att_args)");
  const unet_ch_att_args& e = *p;
  const int ps = e.pass;
  if (ps < 0 || ps > 5) return k.fail("pass must be 0..5");
  if (e.C < 8 || e.C % 8 || e.C / 8 > 256 || 256 % (e.C / 8))
    return k.fail("C / 8 must divide 256 (C = 8, 16, 32, 64, 128, 256, 512, 1024 or 2048)");
  if (e.Cr <= 0) return k.fail("Cr must be positive");
  if (e.N <= 0 || e.N > 65535) return k.fail("N must be 1..65535");
  if (e.HW <= 0 || e.HW > 0xFFFFFFFEll) return k.fail("HW must be 1..2^32-2 (the argmax key holds a 32-bit pixel index)");
  const bool bbany = e.act || e.yraw || e.mean || e.invstd || e.bsums || e.ldact || e.ldyraw;
  if (ps == 0) {
    k.act(e.y, e.ldy, e.C, "y", "ldy", ps);
    k.ptr(e.psum, "psum", ps); k.ptr(e.pkey, "pkey", ps);
  } else if (ps == 1) {
    k.ptr(e.psum, "psum", ps); k.ptr(e.pkey, "pkey", ps); k.ptr(e.w1, "w1", ps); k.ptr(e.w2, "w2", ps);
    k.ptr(e.am, "am", ps); k.ptr(e.h, "h", ps); k.ptr(e.gate, "gate", ps);
  } else if (ps == 2) {
    k.act(e.y, e.ldy, e.C, "y", "ldy", ps);
    k.ptr(e.gate, "gate", ps);
    k.act(e.out, e.ldo, e.C, "out", "ldo", ps);
  } else if (ps == 3) {
    k.act(e.dout2, e.lddo2, e.C, "dout2", "lddo2", ps);
    k.act(e.y, e.ldy, e.C, "y", "ldy", ps);
    k.ptr(e.dgate, "dgate", ps);
  } else if (ps == 4) {
    k.ptr(e.gate, "gate", ps); k.ptr(e.dgate, "dgate", ps); k.ptr(e.w1, "w1", ps); k.ptr(e.w2, "w2", ps);
    k.ptr(e.h, "h", ps); k.ptr(e.am, "am", ps); k.ptr(e.dam, "dam", ps); k.ptr(e.gw_acc, "gw_acc", ps);
    k.ptr(e.gw1, "gw1", ps); k.ptr(e.gw2, "gw2", ps);
  } else {
    k.ptr(e.gate, "gate", ps); k.ptr(e.dam, "dam", ps); k.ptr(e.pkey, "pkey", ps);
    k.act(e.dout2, e.lddo2, e.C, "dout2", "lddo2", ps);
    k.act(e.dout, e.lddo, e.C, "dout", "lddo", ps);
    if (k.ok && bbany) {
      if (!e.bsums || !e.act || !e.yraw || !e.mean || !e.invstd)
        return k.fail("the fused BN backward (bb) needs all of act, yraw, mean, invstd, bsums");
      k.act(e.act, e.ldact, e.C, "act", "ldact", ps);
      k.act(e.yraw, e.ldyraw, e.C, "yraw", "ldyraw", ps);
    }
  }
  if (!k.ok) return 1;

  ChAttArgs c = {};
  c.y = (const bf16_t*)e.y; c.ldy = e.ldy; c.out = (bf16_t*)e.out; c.ldo = e.ldo;
  c.psum = e.psum; c.pkey = e.pkey; c.w1 = e.w1; c.w2 = e.w2; c.am = e.am; c.h = e.h; c.gate = e.gate;
  c.dout2 = (const bf16_t*)e.dout2; c.lddo2 = e.lddo2; c.dgate = e.dgate; c.dam = e.dam;
  c.gw1 = e.gw1; c.gw2 = e.gw2; c.gw_acc = e.gw_acc;
  c.dout = (bf16_t*)e.dout; c.lddo = e.lddo;
  if (ps == 5 && bbany) c.bb = bb_args(e.act, e.ldact, e.yraw, e.ldyraw, e.mean, e.invstd, e.bsums, (int64_t)e.N * e.HW, e.C);
  c.HW = e.HW; c.inv_hw = 1.0f / (float)e.HW;  // as the executor's ch_args
  c.N = e.N; c.C = e.C; c.Cr = e.Cr;
  const hipError_t err = launch_ch_att(c, ps, stream);
  if (err != hipSuccess) {
    set_err(std::string("unet_ch_att_op: launch_ch_att pass ") + std::to_string(ps) + " -> " + hipGetErrorString(err));
    return (int)err;
  }
  return 0;
}

int unet_f8_quantize(const void* x, int ld, int C, int64_t npix, void* q, void* state, int calibrate,
                     hipStream_t stream) {
  CK(launch_f8_quant_act((const bf16_t*)x, ld, C, npix, (uint8_t*)q, (F8State*)state, calibrate, stream));
  return 0;
}

int unet_f8_pack_weight(const float* w, int Co, int Ci, int R, int S, void* dst, void* state, int calibrate,
                        hipStream_t stream) {
  CK(launch_f8_pack_w(w, Co, Ci, R, S, (uint8_t*)dst, (F8State*)state, calibrate, stream));
  return 0;
}

int unet_f8_roll(void* states, int n, hipStream_t stream) {
  CK(launch_f8_roll((F8State*)states, n, stream));
  return 0;
}

int unet_conv_fwd_f8(const void* xq, int ldx, const void* wq, const void* state_x, const void* state_w, void* y,
                     int ldy, const float* bias, const void* addend, int ldadd, double* stats, int N, int H, int W,
                     int C, int P, int Q, int Cout, int R, int S, int stride, int pad, hipStream_t stream) {
  ConvFwdArgs a = conv_args(xq, ldx, wq, y, ldy, N, H, W, C, P, Q, Cout, R, S, stride, pad);
  a.f8x = (const F8State*)state_x; a.f8w = (const F8State*)state_w;
  a.bias = bias; a.add = (const bf16_t*)addend; a.ldadd = ldadd; a.stats = stats;
  CK(launch_conv_fwd_f8(a, stream));
  return 0;
}

int unet_conv_wgrad(const void* dy, int lddy, const void* x, int ldx, float* dw_acc, int N, int H, int W, int C,
                    int P, int Q, int Cout, int R, int S, int stride, int pad, int stem, hipStream_t stream) {
  const ConvWgradArgs a = wgrad_args(dy, lddy, x, ldx, dw_acc, N, H, W, C, P, Q, Cout, R, S, stride, pad);
  if (stem && !stem_width_ok("unet_conv_wgrad", Cout)) return 1;
  CK(launch_conv_wgrad(a, stem, stream));
  return 0;
}

int unet_conv_wgrad_slab(const void* dy, int lddy, const void* x, int ldx, float* dw, void* slab,
                         int64_t slab_bytes, int N, int H, int W, int C, int P, int Q, int Cout, int R, int S,
                         int stride, int pad, int stem, hipStream_t stream) {
  if (!slab || slab_bytes <= 0 || ((uintptr_t)slab & 15)) { set_err("unet_conv_wgrad_slab: bad slab"); return 1; }
  ConvWgradArgs a = wgrad_args(dy, lddy, x, ldx, dw, N, H, W, C, P, Q, Cout, R, S, stride, pad);
  a.slab = (float*)slab; a.slab_bytes = (size_t)slab_bytes;
  if (stem && !stem_width_ok("unet_conv_wgrad_slab", Cout)) return 1;
  CK(launch_conv_wgrad(a, stem, stream));
  CK(launch_wgrad_finish(stream));
  return 0;
}

int unet_convt_wgrad_slab(const void* dy, int lddy, const void* x, int ldx, float* dw, void* slab,
                          int64_t slab_bytes, int N, int H, int W, int Ci, int Co, hipStream_t stream) {
  if (!slab || slab_bytes <= 0 || ((uintptr_t)slab & 15)) { set_err("unet_convt_wgrad_slab: bad slab"); return 1; }
  // as the executor: "dy" := X [N,H,W,Ci], "x" := dY [N,2H,2W,Co]
  ConvWgradArgs a = wgrad_args(x, ldx, dy, lddy, dw, N, 2 * H, 2 * W, 4 * Co, H, W, Ci, 2, 2, 2, 0);
  a.slab = (float*)slab; a.slab_bytes = (size_t)slab_bytes;
  CK(launch_convt_wgrad(a, stream));
  CK(launch_wgrad_finish(stream));
  return 0;
}

int unet_pack_weight(const float* src, void* dst, int kind, int Co, int Ci, int R, int S, hipStream_t stream) {
  if (kind < PK_CONV_FWD || kind > PK_CONV_DGRAD_CH) { set_err("unet_pack_weight: kind must be 0..6"); return 1; }
  if ((kind == PK_CONV_FWD_CH || kind == PK_CONV_DGRAD_CH) &&
      (R != 3 || S != 3 || Co % 32 || Ci % 32)) {
    set_err("unet_pack_weight: chunk-major packs are 3x3 with Co, Ci multiples of 32");
    return 1;
  }
  PackTable t;
  t.n = 1;
  t.e[0] = PackEntry{src, (bf16_t*)dst, kind, Co, Ci, R, S};
  CK(launch_pack(t, stream));
  return 0;
}

int unet_unpack_grad(const float* acc, float* dst, int kind, int Co, int Ci, int R, int S, hipStream_t stream) {
  UnpackTable t;
  t.n = 1;
  t.e[0] = UnpackEntry{acc, dst, kind, Co, Ci, R, S};
  CK(launch_unpack(t, stream));
  return 0;
}

int unet_bn_forward(const void* y, int ldy, void* out, int ldo, const void* res, int ldr, int res_mode,
                    const double* stats, const float* gamma, const float* beta, float* run_mean, float* run_var,
                    float* save, int64_t npix, int C, int relu, int training, hipStream_t stream) {
  if (res_mode < 0 || res_mode > 1) { set_err("res_mode must be 0 or 1"); return 1; }
  BnApplyArgs a = {};
  a.y = (const bf16_t*)y; a.ldy = ldy; a.out = (bf16_t*)out; a.ldo = ldo;
  a.res = (const bf16_t*)res; a.ldr = ldr; a.res_mode = res_mode; a.relu = relu;
  a.bn.stats = stats; a.bn.gamma = gamma; a.bn.beta = beta; a.bn.run_mean = run_mean; a.bn.run_var = run_var;
  a.bn.save_mean = save; a.bn.save_invstd = save + C; a.bn.count = (double)npix; a.bn.C = C;
  a.bn.eps = 1e-5f; a.bn.momentum = 0.1f; a.bn.training = training;
  a.npix = npix; a.C = C;
  CK(launch_bn_apply(a, stream));
  return 0;
}

int unet_bn_backward(const void* dout, int ldd, const void* out, int ldo, const void* y, int ldy, const float* save,
                     const float* gamma, double* sums, void* dy, int lddy, void* dres, float* dgamma, float* dbeta,
                     int64_t npix, int C, hipStream_t stream) {
  BnBwdArgs a = {};
  a.da = (const bf16_t*)dout; a.ldda = ldd; a.act = (const bf16_t*)out; a.ldact = ldo;
  a.y = (const bf16_t*)y; a.ldy = ldy; a.mean = save; a.invstd = save + C; a.gamma = gamma;
  a.sums = sums; a.dy = (bf16_t*)dy; a.lddy = lddy; a.dres = (bf16_t*)dres; a.lddres = C;
  a.dgamma = dgamma; a.dbeta = dbeta; a.npix = npix; a.C = C; a.relu = 1;
  CK(launch_bn_bwd_reduce(a, stream));
  CK(launch_bn_bwd_apply(a, stream));
  return 0;
}

int unet_resize_area_u8(const uint8_t* src, int N, int H, int W, uint8_t* dst, int oh, int ow, hipStream_t stream) {
  if (!src || !dst) { set_err("unet_resize_area_u8: null buffer"); return 1; }
  CK(launch_resize_area(src, dst, N, H, W, oh, ow, stream));
  return 0;
}

int unet_mask_prep(const uint8_t* src, int N, int H, int W, float* dst, int oh, int ow, hipStream_t stream) {
  if (!src || !dst) { set_err("unet_mask_prep: null buffer"); return 1; }
  CK(launch_mask_prep(src, dst, N, H, W, oh, ow, stream));
  return 0;
}

int unet_normalize_microscopy(const uint8_t* src, int N, int H, int W, float* dst, int normalize,
                              hipStream_t stream) {
  if (!src || !dst) { set_err("unet_normalize_microscopy: null buffer"); return 1; }
  CK(launch_normalize(src, dst, N, H, W, normalize, stream));
  return 0;
}

int unet_rot90_vflip_u8(const uint8_t* src, int N, int H, int W, const int* k, const int* vflip, uint8_t* dst,
                        hipStream_t stream) {
  if (!src || !dst || !k || !vflip) { set_err("unet_rot90_vflip_u8: null buffer"); return 1; }
  CK(launch_rot90_vflip(src, dst, N, H, W, k, vflip, stream));
  return 0;
}

int unet_warp_affine_u8(const uint8_t* src, int N, int H, int W, const double* minv, const int* active,
                        const int* vflip, int nearest, uint8_t* dst, hipStream_t stream) {
  if (!src || !dst || !minv || !active || !vflip) { set_err("unet_warp_affine_u8: null buffer"); return 1; }
  CK(launch_warp_affine(src, dst, N, H, W, minv, active, vflip, nearest, stream));
  return 0;
}

int unet_filter2d_u8(const uint8_t* src, int N, int H, int W, const float* kernels, const int* ksize, uint8_t* dst,
                     hipStream_t stream) {
  if (!src || !dst || !kernels || !ksize) { set_err("unet_filter2d_u8: null buffer"); return 1; }
  CK(launch_filter2d(src, dst, N, H, W, kernels, ksize, stream));
  return 0;
}

// ---- tiled whole-frame inference (tile.hip) ----
// the argument checks shared by the tile entry points; fills g
static bool tile_args_ok(const char* fn, int N, int H, int W, int T, int overlap, unsigned tta, TileGeom* g) {
  if (N <= 0 || H <= 0 || W <= 0) return errf("%s: N = %d, H = %d, W = %d must be positive", fn, N, H, W);
  if (T <= 0 || T > UNET_TILE_MAX) return errf("%s: T = %d is outside 1..%d", fn, T, UNET_TILE_MAX);
  if (overlap < 0 || 2 * overlap > T) return errf("%s: overlap = %d is outside [0, T/2] (T = %d)", fn, overlap, T);
  if (tta == 0 || tta > 0xFFu)
    return errf("%s: tta = 0x%X is not a non-empty mask of the 8 dihedral transforms", fn, tta);
  if (!tile_geom(H, W, T, overlap, tta, N, g)) return errf("%s: bad tile geometry", fn);
  return true;
}

int unet_tile_grid(int H, int W, int T, int overlap, int* ny, int* nx) {
  if (!ny || !nx) { set_err("unet_tile_grid: ny / nx is null"); return 1; }
  if (H <= 0 || W <= 0 || T <= 0 || overlap < 0 || 2 * (int64_t)overlap > T) {
    errf("unet_tile_grid: H = %d, W = %d, T = %d must be positive and overlap = %d in [0, T/2]", H, W, T, overlap);
    return 1;
  }
  *ny = tile_axis_count(H, T, T - overlap);
  *nx = tile_axis_count(W, T, T - overlap);
  return 0;
}

int unet_tile_gather(const float* image, int N, int H, int W, int T, int overlap, unsigned tta, int64_t first,
                     int64_t count, float* tiles, hipStream_t stream) {
  const char* fn = "unet_tile_gather";
  if (!image || !tiles) { set_err("unet_tile_gather: image / tiles is null"); return 1; }
  TileGeom g;
  if (!tile_args_ok(fn, N, H, W, T, overlap, tta, &g)) return 1;
  if (first < 0 || count < 0) { set_err("unet_tile_gather: first / count is negative"); return 1; }
  CK(launch_tile_gather(image, tiles, g, first, count, stream));
  return 0;
}

int unet_tile_blend(const float* tile_logits, int N, int K, int H, int W, int T, int overlap, unsigned tta,
                    float* logits, uint8_t* mask, uint8_t* labels, hipStream_t stream) {
  const char* fn = "unet_tile_blend";
  if (!tile_logits) { set_err("unet_tile_blend: tile_logits is null"); return 1; }
  if (!logits && !mask && !labels) { set_err("unet_tile_blend: logits, mask and labels are all null"); return 1; }
  if (K < 1 || K > UNET_TILE_MAX_CLASSES) {
    errf("unet_tile_blend: K = %d is outside 1..%d", K, UNET_TILE_MAX_CLASSES);
    return 1;
  }
  if (labels && K == 1) { set_err("unet_tile_blend: labels (argmax) need K >= 2"); return 1; }
  TileGeom g;
  if (!tile_args_ok(fn, N, H, W, T, overlap, tta, &g)) return 1;
  CK(launch_tile_blend(tile_logits, logits, mask, labels, g, N, K, stream));
  return 0;
}

// ---- instance labelling of masks (instances.hip) ----
static bool instances_shape_ok(const char* fn, int N, int H, int W) {
  if (N > 0 && H > 0 && W > 0 && (int64_t)H * W < kInstMaxHW) return true;
  return errf("%s: N = %d, H = %d, W = %d must be positive with H * W < 2^31", fn, N, H, W);
}

int64_t unet_instances_workspace_bytes(int N, int H, int W) {
  if (!instances_shape_ok("unet_instances_workspace_bytes", N, H, W)) return 0;
  return instances_workspace_bytes(N, H, W);
}

int unet_label_instances(const uint8_t* mask, int N, int H, int W, int fg_value, int connectivity, int fill_holes,
                         int min_area, int max_instances, int32_t* labels, int32_t* counts, int64_t* stats,
                         uint8_t* filled, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  const char* fn = "unet_label_instances";
  if (!mask || !labels || !counts) { set_err("unet_label_instances: mask / labels / counts is null"); return 1; }
  if (!instances_shape_ok(fn, N, H, W)) return 1;
  if (fg_value < -1 || fg_value > 255 || (connectivity != 1 && connectivity != 2) || min_area < 0 ||
      max_instances < 1) {
    errf("%s: fg_value = %d must be -1 or 0..255, connectivity = %d 1 or 2, min_area = %d >= 0, "
         "max_instances = %d >= 1", fn, fg_value, connectivity, min_area, max_instances);
    return 1;
  }
  if (!workspace_ok(fn, "unet_instances_workspace_bytes", workspace, workspace_bytes,
                    instances_workspace_bytes(N, H, W)))
    return 1;
  const InstArgs a{mask, N, H, W, fg_value, connectivity, fill_holes, min_area, max_instances, labels, counts,
                   reinterpret_cast<long long*>(stats), filled, workspace, workspace_bytes};
  CK(launch_label_instances(a, stream));
  return 0;
}

// ---- distance / nearest-site transform and growth of instances (distance.hip) ----
static_assert(kDistMaxDim == UNET_DISTANCE_MAX_DIM, "size limit of the header");

static bool distance_shape_ok(const char* fn, int N, int H, int W) {
  if (N > 0 && H > 0 && W > 0 && H <= kDistMaxDim && W <= kDistMaxDim && (int64_t)H * W < ((int64_t)1 << 31))
    return true;
  return errf("%s: N = %d, H = %d, W = %d must be positive with H, W <= %d and H * W < 2^31", fn, N, H, W,
              kDistMaxDim);
}

static bool distance_workspace_ok(const char* fn, int N, int H, int W, const void* workspace, int64_t bytes) {
  return workspace_ok(fn, "unet_distance_workspace_bytes", workspace, bytes, distance_workspace_bytes(N, H, W));
}

int64_t unet_distance_workspace_bytes(int N, int H, int W) {
  if (!distance_shape_ok("unet_distance_workspace_bytes", N, H, W)) return 0;
  return distance_workspace_bytes(N, H, W);
}

int unet_distance_transform(const void* src, int src_dtype, int N, int H, int W, int fg_value, int sites,
                            int32_t* dist2, int32_t* nearest, void* workspace, int64_t workspace_bytes,
                            hipStream_t stream) {
  const char* fn = "unet_distance_transform";
  if (!src) { set_err("unet_distance_transform: src is null"); return 1; }
  if (!dist2 && !nearest) { set_err("unet_distance_transform: dist2 and nearest are both null"); return 1; }
  if (!distance_shape_ok(fn, N, H, W)) return 1;
  if ((src_dtype != 0 && src_dtype != 1) || (sites != 0 && sites != 1) || fg_value < -1 ||
      (src_dtype == 0 && fg_value > 255)) {
    errf("%s: src_dtype = %d must be 0 (uint8) or 1 (int32), sites = %d 0 or 1, fg_value = %d -1 or >= 0 "
         "(<= 255 for uint8)", fn, src_dtype, sites, fg_value);
    return 1;
  }
  if (!distance_workspace_ok(fn, N, H, W, workspace, workspace_bytes)) return 1;
  const DistArgs a{src, src_dtype, N, H, W, fg_value, sites, dist2, nearest, -1, nullptr, -1, nullptr, workspace,
                   workspace_bytes};
  CK(launch_distance(a, stream));
  return 0;
}

int unet_grow_instances(const int32_t* labels, int N, int H, int W, int64_t max_dist2, const uint8_t* within,
                        int within_value, int32_t* out, void* workspace, int64_t workspace_bytes,
                        hipStream_t stream) {
  const char* fn = "unet_grow_instances";
  if (!labels || !out) { set_err("unet_grow_instances: labels / out is null"); return 1; }
  if (out == labels) { set_err("unet_grow_instances: out must not alias labels"); return 1; }
  if (!distance_shape_ok(fn, N, H, W)) return 1;
  if (within_value < -1 || within_value > 255) {
    errf("%s: within_value = %d must be -1 or 0..255", fn, within_value);
    return 1;
  }
  if (!distance_workspace_ok(fn, N, H, W, workspace, workspace_bytes)) return 1;
  const DistArgs a{labels, 1, N, H, W, -1, 1, nullptr, nullptr, max_dist2, within, within_value, out, workspace,
                   workspace_bytes};
  CK(launch_distance(a, stream));
  return 0;
}

// ---- geodesic growth and watershed by levels (geodesic.hip) ----
static_assert(kGeoMaxDim == UNET_DISTANCE_MAX_DIM && kGeoMaxHW == UNET_GEODESIC_MAX_HW, "size limits of the header");

static bool geodesic_shape_ok(const char* fn, int N, int H, int W) {
  if (N > 0 && H > 0 && W > 0 && H <= kGeoMaxDim && W <= kGeoMaxDim && (int64_t)H * W <= kGeoMaxHW) return true;
  return errf("%s: N = %d, H = %d, W = %d must be positive with H, W <= %d and H * W <= 2^28", fn, N, H, W,
              kGeoMaxDim);
}

// the arguments the two entries share, then "the stream is not capturing": these calls wait for the stream
static bool geodesic_args_ok(const char* fn, int N, int H, int W, int metric, int within_value, const void* workspace,
                             int64_t workspace_bytes, hipStream_t stream) {
  if (!geodesic_shape_ok(fn, N, H, W)) return false;
  if (metric != 0 && metric != 1) return errf("%s: metric = %d must be 0 (cityblock) or 1 (chamfer)", fn, metric);
  if (within_value < -1 || within_value > 255)
    return errf("%s: within_value = %d must be -1 or 0..255", fn, within_value);
  if (!workspace_ok(fn, "unet_geodesic_workspace_bytes", workspace, workspace_bytes,
                    geodesic_workspace_bytes(N, H, W)))
    return false;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  const hipError_t e = hipStreamIsCapturing(stream, &cs);
  if (e != hipSuccess || cs != hipStreamCaptureStatusNone) {
    (void)hipGetLastError();
    return errf("%s: the stream is capturing (%s); the call reads its convergence back on the host and cannot be "
                "captured into a graph", fn, e != hipSuccess ? hipGetErrorString(e) : "active");
  }
  return true;
}

int64_t unet_geodesic_workspace_bytes(int N, int H, int W) {
  if (!geodesic_shape_ok("unet_geodesic_workspace_bytes", N, H, W)) return 0;
  return geodesic_workspace_bytes(N, H, W);
}

int unet_geodesic_grow(const int32_t* labels, int N, int H, int W, int metric, int64_t max_cost,
                       const uint8_t* within, int within_value, int32_t* out, int32_t* cost, void* workspace,
                       int64_t workspace_bytes, hipStream_t stream) {
  const char* fn = "unet_geodesic_grow";
  if (!labels || !out) { set_err("unet_geodesic_grow: labels / out is null"); return 1; }
  if (out == labels || cost == labels || (cost && cost == out)) {
    set_err("unet_geodesic_grow: out / cost must not alias labels or each other");
    return 1;
  }
  if (!geodesic_args_ok(fn, N, H, W, metric, within_value, workspace, workspace_bytes, stream)) return 1;
  const GeoArgs a{labels, N, H, W, metric, max_cost, within, within_value, nullptr, out, cost, workspace,
                  workspace_bytes};
  CK(launch_geodesic(a, stream));
  return 0;
}

int unet_watershed(const uint8_t* relief, const int32_t* markers, int N, int H, int W, int metric,
                   const uint8_t* mask, int mask_value, int32_t* out, void* workspace, int64_t workspace_bytes,
                   hipStream_t stream) {
  const char* fn = "unet_watershed";
  if (!relief || !markers || !out) { set_err("unet_watershed: relief / markers / out is null"); return 1; }
  if (out == markers) { set_err("unet_watershed: out must not alias markers"); return 1; }
  if (!geodesic_args_ok(fn, N, H, W, metric, mask_value, workspace, workspace_bytes, stream)) return 1;
  const GeoArgs a{markers, N, H, W, metric, -1, mask, mask_value, relief, out, nullptr, workspace, workspace_bytes};
  CK(launch_geodesic(a, stream));
  return 0;
}

int unet_geodesic_last_counts(int* passes, int* changing_passes, int* readbacks) {
  const GeoCounts c = geodesic_last_counts();
  if (passes) *passes = c.passes;
  if (changing_passes) *changing_passes = c.changing;
  if (readbacks) *readbacks = c.readbacks;
  return 0;
}

// ---- two nearest distinct instances, border weights, boundary targets (weights.hip) ----
static_assert(kTwoMaxDim == UNET_TWO_NEAREST_MAX_DIM, "size limit of the header");

static bool two_shape_ok(const char* fn, int N, int H, int W) {
  if (N > 0 && H > 0 && W > 0 && H <= kTwoMaxDim && W <= kTwoMaxDim) return true;
  return errf("%s: N = %d, H = %d, W = %d must be positive with H, W <= %d", fn, N, H, W, kTwoMaxDim);
}

static bool two_workspace_ok(const char* fn, int N, int H, int W, const void* workspace, int64_t bytes) {
  return workspace_ok(fn, "unet_two_nearest_workspace_bytes", workspace, bytes, two_nearest_workspace_bytes(N, H, W));
}

int64_t unet_two_nearest_workspace_bytes(int N, int H, int W) {
  if (!two_shape_ok("unet_two_nearest_workspace_bytes", N, H, W)) return 0;
  return two_nearest_workspace_bytes(N, H, W);
}

int unet_two_nearest_instances(const int32_t* labels, int N, int H, int W, int64_t max_dist2, int32_t* dist2,
                               int32_t* ids, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  const char* fn = "unet_two_nearest_instances";
  if (!labels) { set_err("unet_two_nearest_instances: labels is null"); return 1; }
  if (!dist2 && !ids) { set_err("unet_two_nearest_instances: dist2 and ids are both null"); return 1; }
  if (!two_shape_ok(fn, N, H, W) || !two_workspace_ok(fn, N, H, W, workspace, workspace_bytes)) return 1;
  const TwoArgs a{labels, N, H, W, max_dist2, dist2, ids, 0.f, 0.f, nullptr, nullptr, 0, nullptr, workspace,
                  workspace_bytes};
  CK(launch_two_nearest(a, stream));
  return 0;
}

int unet_border_weights(const int32_t* labels, int N, int H, int W, float w0, float sigma, int64_t max_dist2,
                        const uint8_t* classes, const float* class_weights, int K, float* out, void* workspace,
                        int64_t workspace_bytes, hipStream_t stream) {
  const char* fn = "unet_border_weights";
  if (!labels || !out) { set_err("unet_border_weights: labels / out is null"); return 1; }
  if (!two_shape_ok(fn, N, H, W)) return 1;
  if (!(w0 >= 0.f) || !(sigma > 0.f)) {
    errf("%s: w0 = %g must be >= 0 and sigma = %g > 0", fn, (double)w0, (double)sigma);
    return 1;
  }
  if ((classes != nullptr) != (class_weights != nullptr) || (classes && K <= 0)) {
    errf("%s: classes and class_weights go together, with K = %d > 0", fn, K);
    return 1;
  }
  if (!two_workspace_ok(fn, N, H, W, workspace, workspace_bytes)) return 1;
  const TwoArgs a{labels, N, H, W, max_dist2, nullptr, nullptr, w0, sigma, classes, class_weights, K, out, workspace,
                  workspace_bytes};
  CK(launch_two_nearest(a, stream));
  return 0;
}

int unet_boundary_targets(const int32_t* labels, int N, int H, int W, int connectivity, uint8_t* classes,
                          hipStream_t stream) {
  const char* fn = "unet_boundary_targets";
  if (!labels || !classes) { set_err("unet_boundary_targets: labels / classes is null"); return 1; }
  if (!distance_shape_ok(fn, N, H, W)) return 1;
  if (connectivity != 1 && connectivity != 2) {
    errf("%s: connectivity = %d must be 1 (4 neighbours) or 2 (8)", fn, connectivity);
    return 1;
  }
  CK(launch_boundary_targets(labels, N, H, W, connectivity, classes, stream));
  return 0;
}

// ---- matching of two instance label maps (match.hip) ----
static bool match_caps_ok(const char* fn, int N, int max_gt, int max_pred, int max_pairs) {
  if (N > 0 && max_gt >= 1 && max_gt <= kMatchMaxId && max_pred >= 1 && max_pred <= kMatchMaxId && max_pairs >= 1 &&
      max_pairs <= kMatchMaxPairs)
    return true;
  return errf("%s: N = %d must be positive, max_gt = %d and max_pred = %d in 1..%d, max_pairs = %d in 1..%d", fn, N,
              max_gt, max_pred, kMatchMaxId, max_pairs, kMatchMaxPairs);
}

int64_t unet_match_workspace_bytes(int N, int max_gt, int max_pred, int max_pairs) {
  if (!match_caps_ok("unet_match_workspace_bytes", N, max_gt, max_pred, max_pairs)) return 0;
  return match_workspace_bytes(N, max_gt, max_pred, max_pairs);
}

int unet_match_instances(const int32_t* gt, const int32_t* pred, int N, int H, int W, int max_gt, int max_pred,
                         int max_pairs, int64_t* gt_table, int64_t* pred_table, int64_t* status, int64_t* pairs,
                         void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  const char* fn = "unet_match_instances";
  if (!gt || !pred || !gt_table || !pred_table || !status) {
    set_err("unet_match_instances: gt / pred / gt_table / pred_table / status is null");
    return 1;
  }
  if (!instances_shape_ok(fn, N, H, W)) return 1;
  if (!match_caps_ok(fn, N, max_gt, max_pred, max_pairs)) return 1;
  if (!workspace_ok(fn, "unet_match_workspace_bytes", workspace, workspace_bytes,
                    match_workspace_bytes(N, max_gt, max_pred, max_pairs)))
    return 1;
  const MatchArgs a{gt, pred, N, H, W, max_gt, max_pred, max_pairs, reinterpret_cast<long long*>(gt_table),
                    reinterpret_cast<long long*>(pred_table), reinterpret_cast<long long*>(status),
                    reinterpret_cast<long long*>(pairs), workspace, workspace_bytes};
  CK(launch_match_instances(a, stream));
  return 0;
}

// ---- measuring and selecting instances (measure.hip) ----
static_assert(kMeasureMaxDim == UNET_DISTANCE_MAX_DIM && kMeasureMaxHW == UNET_GEODESIC_MAX_HW,
              "size limits of the header");

static bool measure_shape_ok(const char* fn, int N, int H, int W) {
  if (N > 0 && H > 0 && W > 0 && H <= kMeasureMaxDim && W <= kMeasureMaxDim && (int64_t)H * W <= kMeasureMaxHW)
    return true;
  return errf("%s: N = %d, H = %d, W = %d must be positive with H, W <= %d and H * W <= 2^28", fn, N, H, W,
              kMeasureMaxDim);
}

static bool measure_caps_ok(const char* fn, int max_instances, int channels) {
  if (max_instances >= 1 && max_instances <= kMeasureMaxId && channels >= 0 && channels <= kMeasureMaxChannels)
    return true;
  return errf("%s: max_instances = %d must be in 1..%d and channels = %d in 0..%d", fn, max_instances, kMeasureMaxId,
              channels, kMeasureMaxChannels);
}

int64_t unet_measure_workspace_bytes(int N, int H, int W, int max_instances, int channels) {
  const char* fn = "unet_measure_workspace_bytes";
  if (!measure_shape_ok(fn, N, H, W) || !measure_caps_ok(fn, max_instances, channels)) return 0;
  return measure_workspace_bytes(N, H, W, max_instances, channels);
}

int unet_measure_instances(const int32_t* labels, const void* image, int image_dtype, int channels, int N, int H,
                           int W, int max_instances, int64_t* table, int64_t* status, void* intensity,
                           void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  const char* fn = "unet_measure_instances";
  if (!labels || !table || !status) { set_err("unet_measure_instances: labels / table / status is null"); return 1; }
  if ((image != nullptr) != (intensity != nullptr)) {
    set_err("unet_measure_instances: image and intensity go together, one of them is null");
    return 1;
  }
  if (!measure_shape_ok(fn, N, H, W) || !measure_caps_ok(fn, max_instances, channels)) return 1;
  if (image ? (channels < 1 || image_dtype < 0 || image_dtype > 2) : (channels != 0 || image_dtype != 0)) {
    errf("%s: with an image channels = %d must be in 1..%d and image_dtype = %d 0 (uint8), 1 (uint16) or 2 "
         "(float32); without one both must be 0", fn, channels, kMeasureMaxChannels, image_dtype);
    return 1;
  }
  if (!workspace_ok(fn, "unet_measure_workspace_bytes", workspace, workspace_bytes,
                    measure_workspace_bytes(N, H, W, max_instances, channels)))
    return 1;
  const MeasureArgs a{labels, image, image_dtype, channels, N, H, W, max_instances,
                      reinterpret_cast<long long*>(table), reinterpret_cast<long long*>(status), intensity, workspace,
                      workspace_bytes};
  CK(launch_measure_instances(a, stream));
  return 0;
}

int unet_select_instances(const int32_t* labels, const uint8_t* keep, int N, int H, int W, int M,
                          int32_t* labels_out, int32_t* counts, int32_t* new_ids, hipStream_t stream) {
  const char* fn = "unet_select_instances";
  if (!labels || !keep || !labels_out || !counts || !new_ids) {
    set_err("unet_select_instances: labels / keep / labels_out / counts / new_ids is null");
    return 1;
  }
  if (labels_out == labels) { set_err("unet_select_instances: labels_out must not alias labels"); return 1; }
  if (!measure_shape_ok(fn, N, H, W)) return 1;
  if (M < 1 || M > kMeasureMaxId) {
    errf("%s: M = %d must be in 1..%d", fn, M, kMeasureMaxId);
    return 1;
  }
  const SelectArgs a{labels, keep, N, H, W, M, labels_out, counts, new_ids};
  CK(launch_select_instances(a, stream));
  return 0;
}

// ---- linking instances across frames (track.hip) ----
static bool link_caps_ok(const char* fn, int B, int T, int max_instances, int max_pairs) {
  if (B > 0 && T > 0 && T <= kLinkMaxFrames && (int64_t)B * T <= INT32_MAX && max_instances >= 1 &&
      max_instances <= kMatchMaxId && max_pairs >= 1 && max_pairs <= kMatchMaxPairs)
    return true;
  return errf("%s: B = %d must be positive, T = %d in 1..%d with B * T < 2^31, max_instances = %d in 1..%d, "
              "max_pairs = %d in 1..%d", fn, B, T, kLinkMaxFrames, max_instances, kMatchMaxId, max_pairs,
              kMatchMaxPairs);
}

int64_t unet_link_workspace_bytes(int B, int T, int max_instances, int max_pairs) {
  if (!link_caps_ok("unet_link_workspace_bytes", B, T, max_instances, max_pairs)) return 0;
  return link_workspace_bytes(B, T, max_instances, max_pairs);
}

int unet_link_instances(const int32_t* labels, int B, int T, int H, int W, int max_instances, int max_pairs,
                        int max_tracks, int iou_num, int iou_den, int32_t* tracks_out, int64_t* table,
                        int64_t* status, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  const char* fn = "unet_link_instances";
  if (!labels || !tracks_out || !table || !status) {
    set_err("unet_link_instances: labels / tracks_out / table / status is null");
    return 1;
  }
  if (tracks_out == labels) { set_err("unet_link_instances: tracks_out must not alias labels"); return 1; }
  if (!measure_shape_ok(fn, B, H, W) || !link_caps_ok(fn, B, T, max_instances, max_pairs)) return 1;
  if (max_tracks < 1) { errf("%s: max_tracks = %d must be >= 1", fn, max_tracks); return 1; }
  if (iou_den < 1 || iou_num < 0 || iou_num >= iou_den) {
    errf("%s: the threshold iou_num / iou_den = %d / %d must satisfy 0 <= iou_num < iou_den", fn, iou_num, iou_den);
    return 1;
  }
  const int64_t per_frame = (int64_t)H * W < max_instances ? (int64_t)H * W : max_instances;
  if ((int64_t)T * per_frame > INT32_MAX) {
    errf("%s: T * min(max_instances, H * W) = %lld track ids do not fit int32", fn, (long long)(T * per_frame));
    return 1;
  }
  if (!workspace_ok(fn, "unet_link_workspace_bytes", workspace, workspace_bytes,
                    link_workspace_bytes(B, T, max_instances, max_pairs)))
    return 1;
  const LinkArgs a{labels, B, T, H, W, max_instances, max_pairs, max_tracks, iou_num, iou_den, tracks_out,
                   reinterpret_cast<long long*>(table), reinterpret_cast<long long*>(status), workspace,
                   workspace_bytes};
  CK(launch_link_instances(a, stream));
  return 0;
}

int unet_maxpool_fwd(const void* x, int ldx, void* y, uint8_t* idx, int N, int H, int W, int C,
                     hipStream_t stream) {
  MaxPoolArgs m = {};
  m.x = (const bf16_t*)x; m.ldx = ldx; m.y = (bf16_t*)y; m.ldy = C; m.idx = idx;
  m.N = N; m.H = H; m.W = W; m.C = C; m.P = (H + 1) / 2; m.Q = (W + 1) / 2;
  CK(launch_maxpool_fwd(m, stream));
  return 0;
}

int unet_maxpool_bwd(const void* dy, const uint8_t* idx, const void* addend, int ldadd, void* dx, int N, int H,
                     int W, int C, hipStream_t stream) {
  MaxPoolArgs m = {};
  m.dy = (const bf16_t*)dy; m.lddy = C; m.idx = (uint8_t*)idx; m.add = (const bf16_t*)addend; m.ldadd = ldadd;
  m.dx = (bf16_t*)dx; m.lddx = C;
  m.N = N; m.H = H; m.W = W; m.C = C; m.P = (H + 1) / 2; m.Q = (W + 1) / 2;
  CK(launch_maxpool_bwd(m, stream));
  return 0;
}

}  // extern "C"
