// Private header of the host files (plan.cpp, executor.cpp, api.cpp,
// api_ops.cpp, allreduce.cpp): error reporting, the plan data model, the
// per-launch profiler scope and the entry points the files call across.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../../include/unet_hip.h"
#include "kernels.h"

namespace unet {

extern thread_local std::string g_err;  // one per thread, defined in api.cpp (unet_last_error)
inline void set_err(const std::string& s) { g_err = s; }

#define CK(expr)                                                                      \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess) {                                                           \
      set_err(std::string(#expr) + " -> " + hipGetErrorString(e_) + " @" + __FILE__ + \
              ":" + std::to_string(__LINE__));                                        \
      return (int)e_;                                                                 \
    }                                                                                 \
  } while (0)

#define RUN(expr)              \
  do {                         \
    int r_ = (expr);           \
    if (r_) return r_;         \
  } while (0)

struct Act {  // bf16 NHWC view: ws + off, channel stride ld
  size_t off = 0;
  int ld = 0, C = 0, H = 0, W = 0;
};
inline Act slice(const Act& base, int c0, int C) {
  Act a = base;
  a.off = base.off + (size_t)c0 * 2;
  a.C = C;
  return a;
}

struct Param {
  std::string name;
  std::vector<int64_t> shape;
  int64_t numel = 0, flat = 0;
};

struct Bn {
  int gamma, beta;        // param indices
  int idx;                // BN ordinal (buffers 3*idx + 0/1)
  int C;
  size_t stats, bsums, save;  // ws offsets: fp64 [R][2C] fwd, fp64 [R][2C] bwd, fp32 mean|invstd
};

enum { L_CONV = 0, L_CONVT = 1, L_STEM = 2 };
struct Conv {
  int w, b = -1;  // param indices
  int kind, Ci, Co, R, S, stride, pad;
  size_t pk_fwd = 0, pk_dgrad = 0, wacc = 0;  // ws offsets
  size_t bias_acc = 0;                        // fp64 [kStatRep][Co] (convT bias grads)
  bool f8 = false;                            // forward in fp8 e4m3 (cfg.fp8, C >= 128)
  // forward / data gradient on conv3x3_fl_kernel: pk_fwd / pk_dgrad hold the
  // chunk-major packs (PK_CONV_FWD_CH / PK_CONV_DGRAD_CH) instead
  bool fl_fwd = false, fl_dgrad = false;
  size_t f8w = 0;                             // ws offset: e4m3 [Co][R*S*Ci]
  int f8st = -1;                              // F8State index of the weight
};

// fp8 forward: the e4m3 copy of one conv input activation (quantized once per
// forward, before its first fp8 consumer)
struct F8Act {
  size_t src = 0; int C = 0;  // the bf16 activation (ws offset, channels)
  size_t q = 0;               // ws offset: dense e4m3 [npix][C]
  int st = -1;                // F8State index
};

// BasicBlock (resnet34): conv1 3x3/s - bn1 - relu - conv2 3x3 - bn2 (+ skip) - relu.
// Bottleneck (resnet50, torchvision v1.5): conv1 1x1 - bn1 - relu - conv2 3x3/s -
// bn2 - relu - conv3 1x1 (x4 channels) - bn3 (+ skip) - relu; the block's LAST
// conv / BN are (conv3, bn3), its middle pair (conv2, bn2, y2 -> h2).
struct Block {
  int conv1, bn1, conv2, bn2, ds = -1, dsbn = -1;
  int conv3 = -1, bn3 = -1;             // bottleneck only
  Act in, y1, h, y2, yds, out;
  Act h2, y3;                           // bottleneck: relu(bn2(y2)), conv3 output
  Act d_out, dy1, dh, dy2, dyds;        // grads
  Act dh2, dy3, dds;                    // bottleneck: grads of h2 / y3, downsample dgrad (then added)
  Act d_in;                             // == previous block's d_out (or dP0)
  Act skip_add;                         // skip-concat gradient slice for the input (or empty)
  bool bottleneck() const { return conv3 >= 0; }
  int last_conv() const { return conv3 >= 0 ? conv3 : conv2; }
  int last_bn() const { return conv3 >= 0 ? bn3 : bn2; }
  const Act& last_y() const { return conv3 >= 0 ? y3 : y2; }
  const Act& last_dy() const { return conv3 >= 0 ? dy3 : dy2; }
};

struct Dec {
  int up, conv1, bn1, conv2, bn2;
  Act up_in, up_out;  // up_out = cat slice
  Act cat, y1, h, y2, out;
  Act d_out, dy2, dh, dy1, dcat, d_up_in;
  // gradient of the up-conv part of the concat: a slice of dcat, or (split,
  // when that part is narrower than a 128-B line) its own dense buffer while
  // dcat then holds only the skip channels
  Act dcat_up;
  bool split = false;
};

// use_attention=True: AttentionGate on the skip (advanced_models.py:7-40,286-331)
// and ChannelAttention on the decoder output (:43-61,294,...) of one level
struct Att {
  int wg, bng, wx, bnx, psi_w, psi_b, psibn, fc1, fc2;  // conv / BN / param indices
  int Fg, Fl, Fi, C, Cr;
  Act x;               // the skip activation (own buffer; the concat slice holds x * psi)
  Act g1, xa, s;       // W_g g, W_x x, relu(BN_g + BN_x)
  size_t p = 0, psi = 0, dbnp = 0;     // fp32 [npix]: psi logits, sigmoid(BN(p)), dL/dBN(p)
  size_t pst = 0, pbs = 0, psave = 0;  // fp64 [2] fwd sums, fp64 [2] bwd sums, fp32 mean|invstd
  Act dS, dg1, dxa, dxpsi, dskip, du;  // gradients (du = up-conv output grad incl. the W_g path)
  Act out2, d_out2;                    // decoder output * channel gate, and its gradient
  size_t psum = 0, pkey = 0;           // fp64 [N][C] pooled sums, u64 [N][C] (max, first index) keys
  size_t ca = 0, ch = 0, cam = 0;      // fp32 gate [N][C], hidden [N][2][Cr], avg|max [N][2][C]
  size_t cda = 0, cdam = 0;            // fp64 dL/dgate [N][C], fp32 dL/d(avg|max) [N][2][C]
  size_t gpsi = 0, gfc = 0;            // fp64 replica partials of the psi / fc.2|fc.0 weight gradients
};

}  // namespace unet

using namespace unet;

struct unet_plan {
  unet_config cfg;
  std::vector<Param> params;
  std::vector<Bn> bns;
  std::vector<Conv> convs;
  std::vector<Block> blocks;  // 16 encoder blocks
  std::vector<Dec> decs;      // decoder4..decoder1 (index 0 = level 4)
  std::vector<Att> atts;      // attention of decoder level (same index), when cfg.attention
  int stem_conv, stem_bn, up0_w, up0_b, fin_w, fin_b;
  Act x1, y0, p0, d_x1, d_p0;
  size_t pidx = 0;
  size_t ws_bytes = 0;
  size_t zero_fwd_off = 0, zero_fwd_bytes = 0;
  size_t zero_bwd_off = 0, zero_bwd_bytes = 0;
  // a training forward zeroes the backward's region too (it follows the
  // forward's, one fill instead of two); the next backward then skips its fill
  bool bwd_zeroed = false;          // the last training forward zeroed the backward accumulators ...
  const char* bwd_zeroed_ws = nullptr;  // ... of this workspace
  size_t head_usum = 0;
  size_t wslab = 0, wslab_bytes = 0;  // split-K partials of the halo weight-gradient kernel
  int64_t grad_numel = 0;
  std::vector<std::pair<int64_t, int64_t>> buckets;  // flat element ranges
  std::vector<std::vector<int>> bucket_convs;        // convs to unpack per bucket
  hipEvent_t events[8] = {};
  int nevents = 0;
  // without bucket events (no DDP overlap) the buckets' unpack entries are
  // collected here and launched together at the end of the backward
  UnpackTable pend{};
  // The whole backward runs on the caller's stream.  Weight gradients on a
  // second stream and split-K reduces on a third were both measured slower on
  // MI355X (8.39 vs 7.86 ms/step; 2019 vs 2201 img/s: the LDS-heavy wgrad and
  // reduce blocks contend for CUs with the critical dgrad chain) and were
  // removed.  Two split-K slabs alternate so a deferred
  // reduction never reads partials the next weight gradient overwrites.
  int slab_next = 0;
  bool want_events = false;  // DDP overlap: record one hipEvent per gradient bucket
  // in-kernel phase timing (debug build only, unet_timing_enable): one slot of
  // kTimBlocks x kTimSlots stamps per conv launch, in launch order
  unsigned long long* tim_buf = nullptr;
  int tim_n = 0;
  bool tim_on = false;
  std::vector<std::string> tim_names;
  // The switches below are read when the plan is created; the tests set them
  // to compare a fused path with its separate-pass counterpart.
  // eval forward: BN folded into the conv epilogues (UNET_NO_EVAL_FOLD=1: separate BN passes)
  bool eval_fold = std::getenv("UNET_NO_EVAL_FOLD") == nullptr;
  // BN1 + ReLU of a block / decoder level applied in the staging of the next
  // (weight-stationary) conv, which also stores the activation: no bn_apply
  // pass (UNET_NO_BN_XFORM=1: separate pass)
  bool bn_xform = std::getenv("UNET_NO_BN_XFORM") == nullptr;
  // training: decoder1's last BN + ReLU formed inside the head's two passes
  // from the raw conv output (no bn_apply pass, decoder1's activation never
  // stored; plain U-Net only).  UNET_NO_HEAD_BN_FOLD=1: separate pass
  bool head_bn_fold = std::getenv("UNET_NO_HEAD_BN_FOLD") == nullptr;
  // the stem by recompute (stem_rc.hip): the raw 7x7 conv output y0 is never
  // stored; statistics pass + act/pool pass forward, one pass for the maxpool
  // backward, the stem BN backward and the stem weight gradient.  Shapes with
  // stem rows over 256 pixels (HiRes) keep the stored-y0 path.  UNET_STEM_RC=0:
  // stored-y0 path everywhere; UNET_STEM_KEEP=1: y0 and dZ are stored
  // too (tests of the intermediates)
  bool stem_rc = !(std::getenv("UNET_STEM_RC") && std::atoi(std::getenv("UNET_STEM_RC")) == 0);
  bool stem_keep = std::getenv("UNET_STEM_KEEP") && std::atoi(std::getenv("UNET_STEM_KEEP")) != 0;
  size_t stem_part = 0, stem_tot = 0, stem_tkt = 0;
  std::vector<ConvWgradArgs> wgb;  // collected weight gradients of the current bucket
  std::vector<std::string> wgb_names;
  double wgb_flops = 0;
  double flops_fwd = 0, flops_train = 0;
  // fp8 forward (cfg.fp8): per-tensor delayed-amax states (fp8.hip) for the
  // conv weights and activations; the first forward calibrates
  std::vector<F8Act> f8acts;
  std::vector<char> f8_done;  // per F8Act: quantized in the current forward
  size_t f8st = 0;            // ws offset of the F8State array
  int f8n = 0;
  bool f8_calibrated = false;
  std::vector<std::pair<std::string, Act>> named;  // debug / test introspection
  // per-launch HIP-event profiler (unet_profile_*): one record per kernel
  struct ProfRec { std::string name; double flops; int e0, e1; std::string kernel; };
  bool prof = false;
  std::vector<hipEvent_t> evpool;
  int evused = 0;
  std::vector<ProfRec> recs;
};

inline int prof_event(unet_plan* p, hipStream_t st) {
  if (p->evused == (int)p->evpool.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return -1;
    p->evpool.push_back(e);
  }
  const int i = p->evused++;
  if (hipEventRecord(p->evpool[i], st) != hipSuccess) return -1;
  return i;
}
// RAII: brackets one launch with two events when profiling is on
struct ProfScope {
  unet_plan* p; hipStream_t st; std::string name; double flops; int e0 = -1;
  ProfScope(unet_plan* p_, hipStream_t s, std::string n, double f) : p(p_), st(s), name(std::move(n)), flops(f) {
    if (p->prof) e0 = prof_event(p, st);
  }
  void close() {
    if (p->prof && e0 >= 0) {
      const int e1 = prof_event(p, st);
      if (e1 >= 0) p->recs.push_back({name, flops, e0, e1, flops > 0 ? unet::last_kernel_tag() : ""});
    }
    e0 = -1;
  }
  ~ProfScope() { close(); }
};

// the next conv launch's phase-stamp slot (null unless timing is on)
inline unsigned long long* tim_slot(unet_plan* p, const std::string& name) {
  if (!p->tim_on || !p->tim_buf || p->tim_n >= kTimLaunches) return nullptr;
  p->tim_names.push_back(name);
  return p->tim_buf + (size_t)(p->tim_n++) * kTimBlocks * kTimSlots;
}

int build_plan(unet_plan* p);     // plan.cpp
int ensure_events(unet_plan* p);  // plan.cpp: the bucket events, created on first use
// executor.cpp
int run_forward(unet_plan* p, const float* image, const float* const* prm, float* const* buf, char* ws,
                float* logits, int training, hipStream_t st);
int run_backward(unet_plan* p, const float* image, const float* dlogits, const float* const* prm, char* ws,
                 float* grads, hipStream_t st);
