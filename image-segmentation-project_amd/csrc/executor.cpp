// Native executor for the resnet34 U-Net training step (forward + backward).
//
// The plan mirrors UNetWithBackbone(backbone='resnet34', use_attention=False)
// (/root/reference/advanced_models.py:64-100,157-160,197-205,264-357) with the
// torchvision ResNet34 encoder.  It owns: the parameter table in reference
// state_dict order, the workspace layout (bf16 NHWC activations, skip-concat
// buffers that the up-convs write into directly, BN sums, packed weights and
// fp32 weight-gradient accumulators), and the launch sequence.  Python passes
// raw device pointers; nothing here allocates device memory.
#include <algorithm>

#include "plan.h"

namespace {

struct Ctx {
  unet_plan* p;
  char* ws;
  const float* const* prm;
  float* const* buf;
  hipStream_t st;
  int training;
  bf16_t* A(const Act& a) const { return reinterpret_cast<bf16_t*>(ws + a.off); }
  template <class T> T* W(size_t off) const { return reinterpret_cast<T*>(ws + off); }
};

BnLaunch bn_launch(const Ctx& x, int bi, int64_t npix) {
  const Bn& b = x.p->bns[bi];
  BnLaunch l;
  l.stats = x.W<double>(b.stats);
  l.gamma = x.prm[b.gamma];
  l.beta = x.prm[b.beta];
  l.run_mean = x.buf ? x.buf[3 * b.idx + 0] : nullptr;  // (backward contexts carry no buffers)
  l.run_var = x.buf ? x.buf[3 * b.idx + 1] : nullptr;
  l.save_mean = x.W<float>(b.save);
  l.save_invstd = x.W<float>(b.save) + b.C;
  l.count = (double)npix;
  l.C = b.C;
  l.eps = x.p->cfg.bn_eps;
  l.momentum = x.p->cfg.bn_momentum;
  l.training = x.training;
  // buffers are (running_mean, running_var, num_batches_tracked) per BN
  l.nbt = x.buf && x.training ? reinterpret_cast<long long*>(x.buf[3 * b.idx + 2]) : nullptr;
  return l;
}

double conv_flops(const unet_plan* p, const Conv& cv, const Act& fwd_out) {
  const double N = p->cfg.N;
  if (cv.kind == L_CONVT) return 2.0 * N * (fwd_out.H / 2) * (fwd_out.W / 2) * cv.Ci * cv.Co * 4;
  return 2.0 * N * fwd_out.H * fwd_out.W * cv.Co * cv.Ci * cv.R * cv.S;
}
const std::string& pname(const Ctx& x, int param) { return x.p->params[param].name; }

// geometry and leading dimensions of conv cv reading `in`, writing `out`;
// dgrad: the data gradient's view (in = dY with Co channels, out = dX with Ci)
ConvFwdArgs conv_geom(const Ctx& x, const Conv& cv, const Act& in, const Act& out, bool dgrad = false) {
  ConvFwdArgs a = {};
  a.ldx = in.ld; a.ldy = out.ld;
  a.N = x.p->cfg.N; a.H = in.H; a.W = in.W; a.C = dgrad ? cv.Co : cv.Ci;
  a.P = out.H; a.Q = out.W; a.Cout = dgrad ? cv.Ci : cv.Co;
  a.R = cv.R; a.S = cv.S; a.stride = cv.stride; a.pad = cv.pad;
  return a;
}

// what conv_forward fuses into the launch beyond conv (+ bias, + BN sums)
struct FwdOpt {
  // fold_bn >= 0 (eval only): that BN (running statistics) is applied in the
  // conv epilogue, then `res` is added and ReLU applied (relu), so the BN pass
  // after the conv disappears (§8(f) row 4)
  int fold_bn = -1;
  bool relu = false;
  const Act* res = nullptr;
  // xbn >= 0 (training): `in` is the RAW output of the previous conv; BN xbn +
  // ReLU is applied while staging and the activation is stored to *xh by the
  // conv itself (ConvFwdArgs::xform), replacing that BN's bn_apply pass
  int xbn = -1;
  const Act* xh = nullptr;
  // ds >= 0 (training, the 3x3 / stride-2 conv1 of a downsample block): that
  // 1x1 / stride-2 downsample (output *yds, BN dsbn's sums) rides in the same
  // launch when the implicit-GEMM forward takes it; *ds_done says whether it did
  int ds = -1;
  const Act* yds = nullptr;
  int dsbn = -1;
  bool* ds_done = nullptr;
};
// the eval fold of BN `bn` (+ residual `res`) + ReLU (relu)
FwdOpt fold_opt(int bn, bool relu, const Act* res = nullptr) {
  FwdOpt o;
  o.fold_bn = bn; o.relu = relu; o.res = res;
  return o;
}

bool ds_fold_fwd_ok(const Ctx& x, int ci, int ds) {
  const Conv& cv = x.p->convs[ci];
  if (ds < 0 || !x.training || cv.f8 || cv.fl_fwd || cv.kind != L_CONV) return false;
  const Conv& dv = x.p->convs[ds];
  return cv.R == 3 && cv.S == 3 && cv.stride == 2 && cv.pad == 1 && cv.Ci % 64 == 0 && !dv.f8 &&
         dv.kind == L_CONV && dv.R == 1 && dv.S == 1 && dv.stride == 2 && dv.pad == 0 && dv.Co == cv.Co &&
         dv.Ci == cv.Ci && dv.b < 0;
}
int conv_forward(const Ctx& x, int ci, const Act& in, const Act& out, int bn_for_stats, const FwdOpt& o = {}) {
  const Conv& cv = x.p->convs[ci];
  if (o.ds_done) *o.ds_done = false;
  ConvFwdArgs a = conv_geom(x, cv, in, out);
  bool dsf = o.yds && ds_fold_fwd_ok(x, ci, o.ds) && o.fold_bn < 0 && o.xbn < 0;
  if (dsf) {  // the kernel's own geometry / tile test (it reads the geometry and ldyds, not ldx / ldy)
    ConvFwdArgs g = a;
    g.ldyds = o.yds->ld;
    dsf = conv_fwd_ds_ok(g);
  }
  ProfScope ps(x.p, x.st, "fwd " + pname(x, cv.w) + (o.xbn >= 0 ? " +bn" : "") + (dsf ? " +ds" : ""),
               conv_flops(x.p, cv, out) + (dsf ? conv_flops(x.p, x.p->convs[o.ds], *o.yds) : 0.0));
  a.x = x.A(in); a.y = x.A(out);
  a.w = x.W<bf16_t>(cv.pk_fwd);
  a.bias = cv.b >= 0 ? x.prm[cv.b] : nullptr;
  a.stats = (bn_for_stats >= 0 && x.training) ? x.W<double>(x.p->bns[bn_for_stats].stats) : nullptr;
  if (o.fold_bn >= 0) {
    a.fold = bn_launch(x, o.fold_bn, (int64_t)a.N * out.H * out.W);
    a.fold.training = 0;
    a.fold_on = 1;
    a.fold_relu = o.relu ? 1 : 0;
    if (o.res) { a.add = x.A(*o.res); a.ldadd = o.res->ld; }
  }
  if (o.xbn >= 0) {
    a.xbn = bn_launch(x, o.xbn, (int64_t)a.N * in.H * in.W);
    a.xh = x.A(*o.xh); a.ldxh = o.xh->ld;
    a.xform = 1;
  }
  if (cv.f8) {  // e4m3 operands: quantize the input once per forward, block-scaled MFMA
    unet_plan* p = x.p;
    int fi = -1;
    for (int i = 0; i < (int)p->f8acts.size(); ++i)
      if (p->f8acts[i].src == in.off && p->f8acts[i].C == in.C) fi = i;
    if (fi < 0) { set_err("fp8 conv without a registered input"); return 1; }
    const F8Act& f = p->f8acts[fi];
    F8State* sts = x.W<F8State>(p->f8st);
    if (!p->f8_done[fi]) {
      ProfScope pq(p, x.st, "f8_quant " + pname(x, cv.w), 0);
      CK(launch_f8_quant_act(x.A(in), in.ld, in.C, (int64_t)a.N * in.H * in.W, x.W<uint8_t>(f.q), sts + f.st,
                             (p->f8_calibrated ? 0 : F8_CALIBRATE) | (x.training ? 0 : F8_FROZEN), x.st));
      p->f8_done[fi] = 1;
    }
    a.x = reinterpret_cast<const bf16_t*>(x.W<uint8_t>(f.q)); a.ldx = in.C;
    a.w = reinterpret_cast<const bf16_t*>(x.W<uint8_t>(cv.f8w));
    a.f8x = sts + f.st; a.f8w = sts + cv.f8st;
    CK(launch_conv_fwd_f8(a, x.st));
    return 0;
  }
  a.tim = tim_slot(x.p, "fwd " + pname(x, cv.w));
  if (cv.fl_fwd) {  // chunk-major pack: only conv3x3_fl_kernel reads it
    a.wch = a.w;
    a.w = nullptr;
    CK(launch_conv3x3_fl(a, 0, x.st));
    return 0;
  }
  if (dsf) {
    ConvFwdArgs b = a;
    b.wds = x.W<bf16_t>(x.p->convs[o.ds].pk_fwd);
    b.yds = x.A(*o.yds); b.ldyds = o.yds->ld;
    b.stats_ds = o.dsbn >= 0 ? x.W<double>(x.p->bns[o.dsbn].stats) : nullptr;
    const hipError_t e = launch_conv_fwd(b, MODE_FWD, x.st);
    if (e != hipErrorNotSupported) {
      CK(e);
      if (o.ds_done) *o.ds_done = true;
      return 0;
    }
  }
  if (cv.kind == L_CONV && cv.R == 1 && cv.S == 1 && cv.stride == 1) {  // weight-stationary 1x1 where covered
    const hipError_t e = launch_conv1x1(a, 0, x.st);
    if (e != hipErrorNotSupported) {
      CK(e);
      return 0;
    }
  }
  if (cv.kind == L_CONVT) {  // weight-stationary up-conv (convt.hip) where it covers the shape
    const hipError_t e = launch_convt2x2(a, 0, x.st);
    if (e != hipErrorNotSupported || a.xform) {  // (an xform launch has no fallback)
      CK(e);
      return 0;
    }
  }
  CK(launch_conv_fwd(a, cv.kind == L_CONVT ? MODE_SHUF : MODE_FWD, x.st));
  return 0;
}

// can conv `ci` (input: raw y of BN bi's conv, output `out`) apply that BN +
// ReLU in its staging and store the activation `h` itself?
bool xform_ok(const Ctx& x, int ci, const Act& yraw, const Act& h, const Act& out) {
  const unet_plan* p = x.p;
  if (!x.training || !p->bn_xform) return false;
  const Conv& cv = p->convs[ci];
  if (cv.f8 || cv.kind != L_CONV || h.H != yraw.H || h.W != yraw.W || h.C != yraw.C) return false;
  ConvFwdArgs a = conv_geom(x, cv, yraw, out);
  a.ldxh = h.ld;
  return conv3x3_ws_xform_ok(a);
}

// the same for the next decoder level's up-conv (convt2x2_kernel forward):
// decoder level l's last BN + ReLU applied to the up-conv's pixel operand and
// the activation d.out stored by it (the plain U-Net: with attention the
// channel-attention forward reads d.out first)
bool up_xform_ok(const Ctx& x, int l) {
  const unet_plan* p = x.p;
  if (!x.training || !p->bn_xform || !p->atts.empty() || l + 1 >= (int)p->decs.size()) return false;
  const Dec& d = p->decs[l];
  const Dec& n = p->decs[l + 1];
  const Conv& cv = p->convs[n.up];
  if (cv.f8 || cv.kind != L_CONVT || n.up_in.off != d.out.off || d.y2.C != d.out.C || d.y2.H != d.out.H ||
      d.y2.W != d.out.W)
    return false;
  ConvFwdArgs a = conv_geom(x, cv, d.y2, n.up_out);  // (the test reads N, H, W, C, Cout and the strides)
  a.ldxh = d.out.ld;
  return cv.Ci == d.y2.C && convt2x2_xform_ok(a);
}

// what conv_dgrad fuses into the launch beyond dx = dgrad(dy) (+ addend)
struct DgradOpt {
  // dx is dA of that BN(+ReLU); the epilogue stores dZ and runs the
  // BN-backward reduction (ConvFwdArgs::bb)
  const BnBwdArgs* fuse = nullptr;
  // ds >= 0: the block's 1x1/s2 downsample dgrad (dY = dyds) is folded into this
  // 3x3/s2 conv1 dgrad as a second reduction range of parity class 0
  int ds = -1;
  const Act* dyds = nullptr;
  const Act* dx_split = nullptr;  // channels >= dx.C go to their own buffer
  // convT only: bias_acc = the up-conv's bias-gradient replicas; *bias_done tells
  // whether the launch summed them (the weight-stationary kernel does, in the
  // same pass over dY)
  double* bias_acc = nullptr;
  bool* bias_done = nullptr;
};

int conv_dgrad(const Ctx& x, int ci, const Act& dy, const Act& dx, const Act* add, const DgradOpt& o = {}) {
  const Conv& cv = x.p->convs[ci];
  const double fl = conv_flops(x.p, cv, dy) + (o.ds >= 0 ? conv_flops(x.p, x.p->convs[o.ds], *o.dyds) : 0.0);
  ProfScope ps(x.p, x.st, "dgrad " + pname(x, cv.w) + (o.ds >= 0 ? " +ds" : ""), fl);
  ConvFwdArgs a = conv_geom(x, cv, dy, dx, true);
  a.x = x.A(dy); a.y = x.A(dx);
  a.w = x.W<bf16_t>(cv.pk_dgrad);
  if (add && add->ld) { a.add = x.A(*add); a.ldadd = add->ld; }
  if (o.fuse) a.bb = *o.fuse;
  if (o.dx_split) { a.ysplit = x.A(*o.dx_split); a.ldysplit = o.dx_split->ld; a.csplit = dx.C; }
  if (o.ds >= 0) {
    const Conv& dv = x.p->convs[o.ds];
    a.x2 = x.A(*o.dyds); a.ldx2 = o.dyds->ld;
    a.w2 = x.W<bf16_t>(dv.pk_dgrad); a.C2 = dv.Co;
  }
  // convT: an ordinary k2s2 conv of dY; conv: the transposed gather
  a.tim = tim_slot(x.p, "dgrad " + pname(x, cv.w));
  if (cv.fl_dgrad) {  // chunk-major pack: only conv3x3_fl_kernel reads it
    a.wch = a.w;
    a.w = nullptr;
    CK(launch_conv3x3_fl(a, 1, x.st));
    return 0;
  }
  if (o.bias_done) *o.bias_done = false;
  if (cv.kind == L_CONV && cv.R == 1 && cv.S == 1 && cv.stride == 1 && !o.fuse) {  // weight-stationary 1x1
    const hipError_t e = launch_conv1x1(a, 1, x.st);
    if (e != hipErrorNotSupported) {
      CK(e);
      return 0;
    }
  }
  if (cv.kind == L_CONVT) {  // weight-stationary up-conv (convt.hip): its own geometry, the input grid
    ConvFwdArgs b = a;
    b.H = dx.H; b.W = dx.W; b.C = cv.Ci; b.Cout = cv.Co;
    b.P = dy.H; b.Q = dy.W;
    b.bias_acc = o.bias_acc;
    const hipError_t e = launch_convt2x2(b, 1, x.st);
    if (e != hipErrorNotSupported) {
      CK(e);
      if (o.bias_done) *o.bias_done = o.bias_acc != nullptr;
      return 0;
    }
  }
  if (cv.kind == L_CONVT && dy.ld == cv.Co && (2 * cv.Co) % 64 == 0 && dy.W % 2 == 0 && !a.x2 && !a.ysplit) {
    // ConvTranspose2d(k2, s2) data gradient = the k2s2 conv of dY.  Output
    // pixel (i, j) reads dY rows 2i, 2i+1 at columns 2j, 2j+1: in a dense dY
    // those column pairs are one contiguous 2*Co-channel "pixel", so the conv
    // runs as R = 2, S = 1, stride (2, 1) over W/2 merged pixels with K steps of
    // whole 128-B lines (the round-5 form staged 64-B half lines per tap).  The
    // PK_CONVT_DGRAD pack [Ci][a][b][Co] is already the [Ci][a][b*Co + c]
    // layout this view reads.
    a.W = dy.W / 2; a.C = 2 * cv.Co; a.ldx = 2 * dy.ld;
    a.R = 2; a.S = 1; a.stride = 2; a.stride_w = 1; a.pad = 0;
  }
  CK(launch_conv_fwd(a, cv.kind == L_CONVT ? MODE_FWD : MODE_TRANS, x.st));
  return 0;
}

// launch one weight gradient (args a, slab filled in here) and its split-K
// reduction, deferred into the next BN-backward apply launch when possible
int wgrad_and_reduce(const Ctx& x, ConvWgradArgs& a, int mode, const std::string& name, double flops) {
  unet_plan* p = x.p;
  const int si = p->slab_next;
  p->slab_next ^= 1;
  a.slab = x.W<float>(p->wslab + (size_t)si * p->wslab_bytes);
  a.slab_bytes = p->wslab_bytes;
  // a reduction deferred two wgrads ago (the one between had no split-K, and
  // no apply launch took it) still reads this slab: it runs first
  if (wgrad_deferred_reads(a.slab)) {
    ProfScope pr(p, x.st, "wgrad_reduce (deferred)", 0);
    CK(launch_wgrad_flush(x.st));
  }
  a.tim = tim_slot(p, "wgrad " + name);
  {
    ProfScope ps(p, x.st, "wgrad " + name, flops);
    if (mode == 2) CK(launch_convt_wgrad(a, x.st));
    else CK(launch_conv_wgrad(a, mode, x.st));
  }
  if (!wgrad_pending()) return 0;
  // one reduction at most waits for an apply launch; an older one runs now
  // (it reads the other slab, so the order against this wgrad is free)
  if (wgrad_deferred()) {
    ProfScope pr(p, x.st, "wgrad_reduce (deferred)", 0);
    CK(launch_wgrad_flush(x.st));
  }
  if (wgrad_defer()) return 0;
  {
    ProfScope pr(p, x.st, "wgrad_reduce " + name, 0);
    CK(launch_wgrad_finish(x.st));
  }
  return 0;
}

// ds >= 0: the block's 1x1 / stride-2 downsample weight gradient (dY = *dyds,
// same input) folded into this 3x3 / stride-2 conv's launch (ds_fold_ok).
int conv_wgrad(const Ctx& x, int ci, const Act& dy, const Act& in, int ds = -1, const Act* dyds = nullptr) {
  const Conv& cv = x.p->convs[ci];
  ConvWgradArgs a = {};
  a.N = x.p->cfg.N;
  a.dw = x.W<float>(cv.wacc);
  a.R = cv.R; a.S = cv.S; a.stride = cv.stride; a.pad = cv.pad;
  if (cv.kind == L_CONVT) {
    // one GEMM over the input pixels: "dy" := X [Ci], "x" := dY gathered as
    // 4 output pixels x Co per input pixel (XLOAD_SHUF), dW [Ci][2][2][Co]
    a.dy = x.A(in); a.lddy = in.ld;
    a.x = x.A(dy); a.ldx = dy.ld;
    a.H = dy.H; a.W = dy.W; a.C = 4 * cv.Co;
    a.P = in.H; a.Q = in.W; a.Cout = cv.Ci;
    return wgrad_and_reduce(x, a, 2, pname(x, cv.w), conv_flops(x.p, cv, dy));
  }
  a.dy = x.A(dy); a.lddy = dy.ld;
  a.x = x.A(in); a.ldx = in.ld;
  a.H = in.H; a.W = in.W; a.C = cv.Ci;
  a.P = dy.H; a.Q = dy.W; a.Cout = cv.Co;
  double fl = conv_flops(x.p, cv, dy);
  std::string name = pname(x, cv.w);
  if (ds >= 0) {
    const Conv& dv = x.p->convs[ds];
    a.dy2 = x.A(*dyds); a.lddy2 = dyds->ld;
    a.dw2 = x.W<float>(dv.wacc);
    fl += conv_flops(x.p, dv, *dyds);
    name += " +ds";
  }
  if (wgrad_batch_ok(a)) {  // runs in the bucket's batch (flush_wgrad_batch)
    x.p->wgb.push_back(a);
    x.p->wgb_names.push_back(name);
    x.p->wgb_flops += fl;
    return 0;
  }
  return wgrad_and_reduce(x, a, 0, name, fl);
}

int flush_reduce(const Ctx& x);

// the collected weight gradients (conv_wgrad) as batched launches of at most
// kWbMaxLayers layers whose partials fit the halo slab (the per-layer
// reductions that read it have run: flush_reduce first)
int flush_wgrad_batch(const Ctx& x) {
  unet_plan* p = x.p;
  if (p->wgb.empty()) return 0;
  RUN(flush_reduce(x));
  const int grid = wgrad_batch_grid();
  const size_t cap = 2 * p->wslab_bytes / kWbPartBytes;  // slab slots
  size_t first = 0;
  while (first < p->wgb.size()) {
    // as many layers of one tile geometry as the table and the slab hold
    const int tw = wgrad_batch_tw(p->wgb[first]);
    size_t n = 0;
    while (first + n < p->wgb.size() && n < (size_t)kWbMaxLayers && wgrad_batch_tw(p->wgb[first + n]) == tw) ++n;
    WgBatchArgs b;
    for (;;) {
      b = WgBatchArgs{};
      b.grid = grid;
      b.N = p->cfg.N;
      b.tw = tw;
      long long items = 0;
      int units = 0;
      for (size_t j = 0; j < n; ++j) {
        const ConvWgradArgs& a = p->wgb[first + j];
        WgBatchLayer& L = b.L[j];
        L.dy = a.dy; L.x = a.x; L.dw = a.dw;
        L.H = a.H; L.W = a.W; L.C = a.C; L.Cout = a.Cout; L.lddy = a.lddy; L.ldx = a.ldx;
        L.tq = a.Q / tw; L.tp = a.P / (128 / tw);
        L.co_blocks = a.Cout / 64; L.c_blocks = a.C / 64;
        L.tiles = a.N * L.tp * L.tq;
        L.unit0 = units; L.item0 = items;
        units += L.co_blocks * L.c_blocks;
        items += (long long)L.co_blocks * L.c_blocks * L.tiles;
      }
      b.nl = (int)n; b.units = units; b.items = items;
      b.maxseg = wgrad_batch_maxseg(b);
      if ((size_t)grid * b.maxseg <= cap || n == 1) break;
      n = (n + 1) / 2;
    }
    if ((size_t)grid * b.maxseg > cap) {
      set_err("weight-gradient batch: slab too small");
      return -1;
    }
    b.slab = x.W<float>(p->wslab);
    std::string nm = "wgrad batch";
    for (size_t j = 0; j < n; ++j) nm += (j ? "," : " ") + p->wgb_names[first + j];
    b.tim = tim_slot(p, "wgrad batch x" + std::to_string(n));
    double fl = 0;
    for (size_t j = 0; j < n; ++j) {
      const ConvWgradArgs& a = p->wgb[first + j];
      fl += 2.0 * a.N * a.P * a.Q * a.Cout * a.C * 9;
    }
    {
      ProfScope ps(p, x.st, nm, fl);
      CK(launch_wgrad_batch(b, x.st));
    }
    first += n;
  }
  p->wgb.clear();
  p->wgb_names.clear();
  p->wgb_flops = 0;
  return 0;
}

// the downsample's weight gradient can ride in conv1's stride-2 halo wgrad
bool ds_fold_ok(const Ctx& x, const Block& b) {
  if (b.ds < 0 || b.bottleneck()) return false;
  const Conv& c1 = x.p->convs[b.conv1];
  const Conv& dv = x.p->convs[b.ds];
  if (dv.R != 1 || dv.stride != 2 || dv.pad != 0 || dv.Co != c1.Co || dv.Ci != c1.Ci) return false;
  ConvWgradArgs a = {};
  a.N = x.p->cfg.N;
  a.R = c1.R; a.S = c1.S; a.stride = c1.stride; a.pad = c1.pad;
  a.lddy = b.dy1.ld; a.ldx = b.in.ld; a.lddy2 = b.dyds.ld;
  a.dy2 = x.A(b.dyds);
  a.H = b.in.H; a.W = b.in.W; a.C = c1.Ci;
  a.P = b.dy1.H; a.Q = b.dy1.W; a.Cout = c1.Co;
  return b.dyds.H == b.dy1.H && b.dyds.W == b.dy1.W && wgrad_s2_fold_ok(a);
}

int bn_apply(const Ctx& x, int bi, const Act& y, const Act& out, int res_mode, const Act* res, int bi2,
             bool relu) {
  BnApplyArgs a = {};
  const int64_t npix = (int64_t)x.p->cfg.N * y.H * y.W;
  ProfScope ps(x.p, x.st, "bn_fwd " + pname(x, x.p->bns[bi].gamma), 0);
  a.y = x.A(y); a.ldy = y.ld;
  a.out = x.A(out); a.ldo = out.ld;
  a.bn = bn_launch(x, bi, npix);
  if (res_mode) { a.res = x.A(*res); a.ldr = res->ld; }
  if (res_mode == 2) a.bn2 = bn_launch(x, bi2, npix);
  a.npix = npix; a.C = y.C; a.res_mode = res_mode; a.relu = relu ? 1 : 0;
  CK(launch_bn_apply(a, x.st));
  return 0;
}

// BN(+ReLU) backward argument block for out = relu(bn(y) [+ bn2(y2) | + res]).
BnBwdArgs bwd_args(const Ctx& x, int bi, const Act& dout, const Act& out, const Act& y, const Act& dy,
                   int bi2, const Act* y2, const Act* dy2, float* grads) {
  BnBwdArgs a = {};
  const Bn& b = x.p->bns[bi];
  a.da = x.A(dout); a.ldda = dout.ld;
  a.act = x.A(out); a.ldact = out.ld;
  a.y = x.A(y); a.ldy = y.ld;
  a.mean = x.W<float>(b.save); a.invstd = x.W<float>(b.save) + b.C; a.gamma = x.prm[b.gamma];
  a.sums = x.W<double>(b.bsums);
  a.dy = x.A(dy); a.lddy = dy.ld;
  a.dgamma = grads + x.p->params[b.gamma].flat;
  a.dbeta = grads + x.p->params[b.beta].flat;
  if (bi2 >= 0) {
    const Bn& b2 = x.p->bns[bi2];
    a.y2 = x.A(*y2); a.ldy2 = y2->ld;
    a.mean2 = x.W<float>(b2.save); a.invstd2 = x.W<float>(b2.save) + b2.C; a.gamma2 = x.prm[b2.gamma];
    a.sums2 = x.W<double>(b2.bsums);
    a.dy2 = x.A(*dy2); a.lddy2 = dy2->ld;
    a.dgamma2 = grads + x.p->params[b2.gamma].flat;
    a.dbeta2 = grads + x.p->params[b2.beta].flat;
  }
  a.npix = (int64_t)x.p->cfg.N * y.H * y.W; a.C = y.C; a.relu = 1;
  return a;
}

// The producer of dA already stored dZ (in dA's buffer, which then also serves
// as the identity-residual gradient) and reduced it; only the apply runs.
int bn_backward(const Ctx& x, int bi, BnBwdArgs a) {
  ProfScope ps(x.p, x.st, "bn_bwd " + pname(x, x.p->bns[bi].gamma), 0);
  a.relu = 0;
  ReduceTail r;
  if (wgrad_deferred() && wgrad_take_deferred(&r)) {
    const hipError_t e = launch_bn_bwd_apply_reduce(a, r, x.st);
    if (e == hipSuccess) return 0;
    if (e != hipErrorNotSupported) CK(e);
    // this apply's shape cannot carry it: the reduction on its own, then the apply
    CK(launch_bn_bwd_apply(a, x.st));
    CK(launch_slab_reduce(r, x.st));
    return 0;
  }
  CK(launch_bn_bwd_apply(a, x.st));
  return 0;
}

// a deferred reduction that no apply launch took (bucket boundaries, end of
// the backward)
int flush_reduce(const Ctx& x) {
  if (!wgrad_deferred()) return 0;
  ProfScope pr(x.p, x.st, "wgrad_reduce (deferred)", 0);
  CK(launch_wgrad_flush(x.st));
  return 0;
}

int unpack_bucket(const Ctx& x, int bk, float* grads) {
  RUN(flush_wgrad_batch(x));
  RUN(flush_reduce(x));
  ProfScope ps(x.p, x.st, "unpack", 0);
  UnpackTable local;
  local.n = 0;
  // no bucket events: nothing waits for this bucket before the backward ends,
  // so its entries join the pending table (fewer, fuller launches)
  const bool defer = x.p->nevents == 0;
  UnpackTable& t = defer ? x.p->pend : local;
  if (bk == 0) {
    // decoder (and attention W_g / W_x / psi) conv biases feed a training-mode
    // BN: their exact gradient is sum(dY) = 0 (BN removes the mean); written
    // here instead of one memset launch each
    auto zero = [&](int param) -> int {
      t.e[t.n++] = UnpackEntry{nullptr, grads + x.p->params[param].flat, UP_ZERO,
                               (int)x.p->params[param].numel, 1, 1, 1};
      if (t.n == kMaxPack) { CK(launch_unpack(t, x.st)); t.n = 0; }
      return 0;
    };
    for (const Dec& d : x.p->decs) {
      RUN(zero(x.p->convs[d.conv1].b));
      RUN(zero(x.p->convs[d.conv2].b));
    }
    for (const Att& a : x.p->atts) {
      RUN(zero(x.p->convs[a.wg].b));
      RUN(zero(x.p->convs[a.wx].b));
      RUN(zero(a.psi_b));
    }
    // up-conv (ConvTranspose) bias gradients: the channel sums' fp64 replicas
    for (const Dec& d : x.p->decs) {
      if (d.up < 0) continue;
      const Conv& up = x.p->convs[d.up];
      t.e[t.n++] = UnpackEntry{reinterpret_cast<const float*>(x.W<double>(up.bias_acc)),
                               grads + x.p->params[up.b].flat, UP_D2F, up.Co, 1, 1, 1};
      if (t.n == kMaxPack) { CK(launch_unpack(t, x.st)); t.n = 0; }
    }
  }
  for (int ci : x.p->bucket_convs[bk]) {
    const Conv& cv = x.p->convs[ci];
    UnpackEntry& e = t.e[t.n++];
    e.acc = x.W<float>(cv.wacc);
    e.dst = grads + x.p->params[cv.w].flat;
    e.R = cv.R; e.S = cv.S;
    if (cv.kind == L_CONV) { e.kind = UP_CONV; e.Co = cv.Co; e.Ci = cv.Ci; }
    else if (cv.kind == L_CONVT) { e.kind = UP_CONVT; e.Co = cv.Co; e.Ci = cv.Ci; }
    else { e.kind = UP_STEM; e.Co = cv.Co; e.Ci = 1; e.R = 7; e.S = 7; }
    if (t.n == kMaxPack) { CK(launch_unpack(t, x.st)); t.n = 0; }
  }
  if (!defer || bk == (int)x.p->buckets.size() - 1) {  // the last bucket (the stem's) ends the backward
    CK(launch_unpack(t, x.st));
    t.n = 0;
  }
  return 0;
}

}  // namespace


// attention-gate / channel-attention argument blocks of decoder level l
AttGateArgs gate_args(const Ctx& x, int l, float* grads) {
  const unet_plan* p = x.p;
  const Att& t = p->atts[l];
  const Dec& d = p->decs[l];
  const Bn& b = p->bns[t.psibn];
  AttGateArgs a = {};
  a.s = x.A(t.s); a.lds = t.s.ld;
  a.psi_w = x.prm[t.psi_w]; a.psi_b = x.prm[t.psi_b];
  a.p = x.W<float>(t.p); a.psi = x.W<float>(t.psi); a.dbnp = x.W<float>(t.dbnp);
  a.pst = x.W<double>(t.pst); a.pbs = x.W<double>(t.pbs); a.save = x.W<float>(t.psave);
  a.gamma = x.prm[b.gamma]; a.beta = x.prm[b.beta];
  a.run_mean = x.buf ? x.buf[3 * b.idx + 0] : nullptr;
  a.run_var = x.buf ? x.buf[3 * b.idx + 1] : nullptr;
  a.nbt = x.buf && x.training ? reinterpret_cast<long long*>(x.buf[3 * b.idx + 2]) : nullptr;
  a.npix = (int64_t)p->cfg.N * d.cat.H * d.cat.W;
  a.count = (double)a.npix; a.eps = p->cfg.bn_eps; a.momentum = p->cfg.bn_momentum; a.training = x.training;
  a.x = x.A(t.x); a.ldx = t.x.ld;
  const Act xs = slice(d.cat, 0, t.Fl);
  a.xatt = x.A(xs); a.ldxatt = xs.ld;
  a.dxatt = x.A(d.dcat); a.lddxatt = d.dcat.ld;  // skip channels come first (split or not)
  a.dxpsi = x.A(t.dxpsi); a.lddxpsi = t.dxpsi.ld;
  a.dS = x.A(t.dS); a.lddS = t.dS.ld;
  if (grads) {
    a.gpsi_w = grads + p->params[t.psi_w].flat;
    a.gpsi_acc = x.W<double>(t.gpsi);
    a.ggamma = grads + p->params[b.gamma].flat;
    a.gbeta = grads + p->params[b.beta].flat;
  }
  a.Fi = t.Fi; a.Fl = t.Fl;
  return a;
}

ChAttArgs ch_args(const Ctx& x, int l, float* grads) {
  const unet_plan* p = x.p;
  const Att& t = p->atts[l];
  const Dec& d = p->decs[l];
  ChAttArgs c = {};
  c.y = x.A(d.out); c.ldy = d.out.ld;
  c.out = x.A(t.out2); c.ldo = t.out2.ld;
  c.psum = x.W<double>(t.psum); c.pkey = x.W<unsigned long long>(t.pkey);
  c.gw_acc = x.W<double>(t.gfc);
  c.w1 = x.prm[t.fc1]; c.w2 = x.prm[t.fc2];
  c.am = x.W<float>(t.cam); c.h = x.W<float>(t.ch); c.gate = x.W<float>(t.ca);
  c.dout2 = x.A(t.d_out2); c.lddo2 = t.d_out2.ld;
  c.dgate = x.W<double>(t.cda); c.dam = x.W<float>(t.cdam);
  if (grads) {
    c.gw1 = grads + p->params[t.fc1].flat;
    c.gw2 = grads + p->params[t.fc2].flat;
  }
  c.dout = x.A(d.d_out); c.lddo = d.d_out.ld;
  c.HW = (int64_t)d.out.H * d.out.W;
  c.inv_hw = 1.0f / (float)c.HW;
  c.N = p->cfg.N; c.C = t.C; c.Cr = t.Cr;
  return c;
}

// AttentionGate forward (advanced_models.py:28-40): x_att = x * sigmoid(BN(psi(relu(BN(W_g g) + BN(W_x x)))))
int att_gate_forward(const Ctx& x, int l) {
  const Att& t = x.p->atts[l];
  const Dec& d = x.p->decs[l];
  RUN(conv_forward(x, t.wg, d.up_out, t.g1, t.bng));
  RUN(conv_forward(x, t.wx, t.x, t.xa, t.bnx));
  RUN(bn_apply(x, t.bng, t.g1, t.s, 2, &t.xa, t.bnx, true));
  const AttGateArgs a = gate_args(x, l, nullptr);
  ProfScope ps(x.p, x.st, "att_gate_fwd", 0);
  CK(launch_att_gate(a, 0, x.st));
  CK(launch_att_gate(a, 1, x.st));
  return 0;
}

// ChannelAttention forward (advanced_models.py:56-61)
int ch_att_forward(const Ctx& x, int l) {
  const ChAttArgs c = ch_args(x, l, nullptr);
  ProfScope ps(x.p, x.st, "ch_att_fwd", 0);
  for (int pass = 0; pass < 3; ++pass) CK(launch_ch_att(c, pass, x.st));
  return 0;
}

// the stem-by-recompute arguments shared by its forward and backward passes
StemRcArgs stem_rc_args(const Ctx& x, const float* image) {
  const unet_plan* p = x.p;
  const Conv& cv = p->convs[p->stem_conv];
  StemRcArgs s = {};
  s.img = image; s.H = p->cfg.H; s.W = p->cfg.W;
  s.w = x.W<bf16_t>(cv.pk_fwd);
  s.N = p->cfg.N; s.P = p->y0.H; s.Q = p->y0.W; s.Cout = cv.Co; s.Pp = p->p0.H; s.Qp = p->p0.W;
  s.bn = bn_launch(x, p->stem_bn, (int64_t)s.N * s.P * s.Q);
  s.stats = x.training ? x.W<double>(p->bns[p->stem_bn].stats) : nullptr;
  if (p->stem_keep) { s.y = x.A(p->y0); s.ldy = p->y0.ld; }
  s.act = x.A(p->x1); s.ldact = p->x1.ld;
  s.pool = x.A(p->p0); s.ldpool = p->p0.ld; s.idx = x.W<uint8_t>(p->pidx);
  return s;
}

int run_forward(unet_plan* p, const float* image, const float* const* prm, float* const* buf, char* ws,
                       float* logits, int training, hipStream_t st) {
  Ctx x{p, ws, prm, buf, st, training};
  const int N = p->cfg.N;
  // the zeroed region: one PK_ZERO entry of the weight-pack launch below (the
  // first kernel of the step) unless the fp8 kernels run before that launch
  const size_t zbytes = p->zero_fwd_bytes + (training ? p->zero_bwd_bytes : 0);
  const bool zero_in_pack = !p->f8n && zbytes % 16 == 0 && zbytes / 16 < (size_t)INT32_MAX;
  if (!zero_in_pack) CK(hipMemsetAsync(ws + p->zero_fwd_off, 0, zbytes, st));
  // the backward accumulators were zeroed for THIS workspace (an eval forward or
  // another workspace makes the next unet_backward zero them itself)
  p->bwd_zeroed = training != 0;
  p->bwd_zeroed_ws = training ? ws : nullptr;
  if (p->f8n) {  // fp8 scale states: calibrate on the plan's first forward, else roll
    // (training only: an eval forward quantizes with the scales in use and
    // commits no amax, so validation never moves the training scales)
    if (!p->f8_calibrated) CK(hipMemsetAsync(ws + p->f8st, 0, (size_t)p->f8n * sizeof(F8State), st));
    else if (training) CK(launch_f8_roll(x.W<F8State>(p->f8st), p->f8n, st));
    std::fill(p->f8_done.begin(), p->f8_done.end(), 0);
    for (auto& cv : p->convs)
      if (cv.f8) {
        ProfScope ps(p, st, "f8_pack " + pname(x, cv.w), 0);
        CK(launch_f8_pack_w(prm[cv.w], cv.Co, cv.Ci, cv.R, cv.S, x.W<uint8_t>(cv.f8w), x.W<F8State>(p->f8st) + cv.f8st,
                            (p->f8_calibrated ? 0 : F8_CALIBRATE) | (training ? 0 : F8_FROZEN), st));
      }
  }
  // pack weights (fp32 torch layout -> bf16 kernel layouts)
  {
    PackTable t;
    t.n = 0;
    if (zero_in_pack)
      t.e[t.n++] = PackEntry{nullptr, reinterpret_cast<bf16_t*>(ws + p->zero_fwd_off), PK_ZERO, (int)(zbytes / 16), 0, 0, 0};
    auto flush = [&]() -> int {
      ProfScope ps(p, st, "pack", 0);
      CK(launch_pack(t, st));
      t.n = 0;
      return 0;
    };
    for (auto& cv : p->convs) {
      if (cv.kind == L_STEM) {
        t.e[t.n++] = PackEntry{prm[cv.w], x.W<bf16_t>(cv.pk_fwd), PK_STEM, cv.Co, 1, 7, 7};
      } else if (cv.kind == L_CONV) {
        const int fk = cv.fl_fwd ? PK_CONV_FWD_CH : PK_CONV_FWD;
        const int dk = cv.fl_dgrad ? PK_CONV_DGRAD_CH : PK_CONV_DGRAD;
        if (training && !cv.f8) {  // both layouts from one read of the fp32 weight
          t.e[t.n++] = PackEntry{prm[cv.w], x.W<bf16_t>(cv.pk_dgrad), dk, cv.Co, cv.Ci, cv.R, cv.S,
                                 x.W<bf16_t>(cv.pk_fwd), fk};
        } else {
          if (!cv.f8) t.e[t.n++] = PackEntry{prm[cv.w], x.W<bf16_t>(cv.pk_fwd), fk, cv.Co, cv.Ci, cv.R, cv.S};
          if (t.n == kMaxPack) RUN(flush());
          if (training) t.e[t.n++] = PackEntry{prm[cv.w], x.W<bf16_t>(cv.pk_dgrad), dk, cv.Co, cv.Ci, cv.R, cv.S};
        }
      } else {
        t.e[t.n++] = PackEntry{prm[cv.w], x.W<bf16_t>(cv.pk_fwd), PK_CONVT_FWD, cv.Co, cv.Ci, cv.R, cv.S};
        if (t.n == kMaxPack) RUN(flush());
        if (training) t.e[t.n++] = PackEntry{prm[cv.w], x.W<bf16_t>(cv.pk_dgrad), PK_CONVT_DGRAD, cv.Co, cv.Ci, cv.R, cv.S};
      }
      if (t.n >= kMaxPack - 1) RUN(flush());
    }
    RUN(flush());
  }
  // stem: conv7x7/s2 -> bn1 -> relu into cat1[:, :c0]; maxpool
  if (p->stem_rc) {
    StemRcArgs s = stem_rc_args(x, image);
    const double fl = 2.0 * N * p->y0.H * p->y0.W * p->convs[p->stem_conv].Co * 49;
    if (training) {
      ProfScope ps(p, st, "fwd input_conv.weight (stats)", fl);
      s.tim = tim_slot(p, "fwd input_conv.weight (stats)");
      CK(launch_stem_rc_fwd(s, 0, st));
    }
    ProfScope ps(p, st, "fwd input_conv.weight +bn+pool", fl);
    s.tim = tim_slot(p, "fwd input_conv.weight +bn+pool");
    CK(launch_stem_rc_fwd(s, 1, st));
  } else {
    const Conv& cv = p->convs[p->stem_conv];
    ConvFwdArgs a = {};
    a.x = reinterpret_cast<const bf16_t*>(image); a.ldx = 1;
    a.w = x.W<bf16_t>(cv.pk_fwd);
    a.y = x.A(p->y0); a.ldy = p->y0.ld;
    a.stats = training ? x.W<double>(p->bns[p->stem_bn].stats) : nullptr;
    a.N = N; a.H = p->cfg.H; a.W = p->cfg.W; a.C = 1;
    a.P = p->y0.H; a.Q = p->y0.W; a.Cout = cv.Co;
    a.R = 7; a.S = 7; a.stride = 2; a.pad = 3;
    {
      ProfScope ps(p, st, "fwd input_conv.weight", 2.0 * N * p->y0.H * p->y0.W * cv.Co * 49);
      CK(launch_conv_fwd(a, MODE_STEM, st));
    }
    // bn1 + relu + maxpool in one pass: x1 (the decoder1 skip, inside the
    // concat buffer) and the pooled p0 + argmax index
    MaxPoolArgs m = {};
    m.x = x.A(p->y0); m.ldx = p->y0.ld; m.y = x.A(p->p0); m.ldy = p->p0.ld; m.idx = x.W<uint8_t>(p->pidx);
    m.act = x.A(p->x1); m.ldact = p->x1.ld;
    m.bn = bn_launch(x, p->stem_bn, (int64_t)N * p->y0.H * p->y0.W);
    m.N = N; m.H = p->x1.H; m.W = p->x1.W; m.C = p->x1.C; m.P = p->p0.H; m.Q = p->p0.W;
    {
      ProfScope ps(p, st, "bn_relu_maxpool_fwd", 0);
      CK(launch_bn_relu_maxpool_fwd(m, st));
    }
  }
  // eval: every BN of the encoder / decoder blocks folded into its conv's
  // epilogue (running statistics; residual added there), no BN passes
  const bool fold = !training && p->eval_fold;
  for (auto& b : p->blocks) {
    if (b.bottleneck()) {  // torchvision Bottleneck (resnet50)
      if (fold) {
        RUN(conv_forward(x, b.conv1, b.in, b.h, -1, fold_opt(b.bn1, true)));
        RUN(conv_forward(x, b.conv2, b.h, b.h2, -1, fold_opt(b.bn2, true)));
        if (b.ds >= 0) RUN(conv_forward(x, b.ds, b.in, b.yds, -1, fold_opt(b.dsbn, false)));
        RUN(conv_forward(x, b.conv3, b.h2, b.out, -1, fold_opt(b.bn3, true, b.ds >= 0 ? &b.yds : &b.in)));
        continue;
      }
      RUN(conv_forward(x, b.conv1, b.in, b.y1, b.bn1));
      RUN(bn_apply(x, b.bn1, b.y1, b.h, 0, nullptr, -1, true));
      RUN(conv_forward(x, b.conv2, b.h, b.y2, b.bn2));
      RUN(bn_apply(x, b.bn2, b.y2, b.h2, 0, nullptr, -1, true));
      RUN(conv_forward(x, b.conv3, b.h2, b.y3, b.bn3));
      if (b.ds >= 0) {
        RUN(conv_forward(x, b.ds, b.in, b.yds, b.dsbn));
        RUN(bn_apply(x, b.bn3, b.y3, b.out, 2, &b.yds, b.dsbn, true));
      } else {
        RUN(bn_apply(x, b.bn3, b.y3, b.out, 1, &b.in, -1, true));
      }
      continue;
    }
    if (fold) {
      RUN(conv_forward(x, b.conv1, b.in, b.h, -1, fold_opt(b.bn1, true)));
      if (b.ds >= 0) RUN(conv_forward(x, b.ds, b.in, b.yds, -1, fold_opt(b.dsbn, false)));
      RUN(conv_forward(x, b.conv2, b.h, b.out, -1, fold_opt(b.bn2, true, b.ds >= 0 ? &b.yds : &b.in)));
      continue;
    }
    // (a downsample block's 1x1 / stride-2 conv folded into conv1's launch)
    bool ds_done = false;
    FwdOpt o1;
    o1.ds = b.ds; o1.yds = b.ds >= 0 ? &b.yds : nullptr; o1.dsbn = b.dsbn; o1.ds_done = &ds_done;
    RUN(conv_forward(x, b.conv1, b.in, b.y1, b.bn1, o1));
    if (xform_ok(x, b.conv2, b.y1, b.h, b.y2)) {  // bn1 + ReLU inside conv2's staging
      FwdOpt o2; o2.xbn = b.bn1; o2.xh = &b.h;
      RUN(conv_forward(x, b.conv2, b.y1, b.y2, b.bn2, o2));
    } else {
      RUN(bn_apply(x, b.bn1, b.y1, b.h, 0, nullptr, -1, true));
      RUN(conv_forward(x, b.conv2, b.h, b.y2, b.bn2));
    }
    if (b.ds >= 0) {
      if (!ds_done) RUN(conv_forward(x, b.ds, b.in, b.yds, b.dsbn));
      RUN(bn_apply(x, b.bn2, b.y2, b.out, 2, &b.yds, b.dsbn, true));
    } else {
      RUN(bn_apply(x, b.bn2, b.y2, b.out, 1, &b.in, -1, true));
    }
  }
  const bool att = !p->atts.empty();
  const bool hfold = training && p->head_bn_fold;
  bool up_xf = false;  // the previous level's last BN + ReLU rides in this level's up-conv
  for (int l = 0; l < (int)p->decs.size(); ++l) {
    Dec& d = p->decs[l];
    if (up_xf) {
      const Dec& pd = p->decs[l - 1];
      FwdOpt ou; ou.xbn = pd.bn2; ou.xh = &pd.out;
      RUN(conv_forward(x, d.up, pd.y2, d.up_out, -1, ou));
    } else {
      RUN(conv_forward(x, d.up, d.up_in, d.up_out, -1));
    }
    up_xf = !fold && up_xform_ok(x, l);
    if (att) RUN(att_gate_forward(x, l));
    if (fold) {
      RUN(conv_forward(x, d.conv1, d.cat, d.h, -1, fold_opt(d.bn1, true)));
      RUN(conv_forward(x, d.conv2, d.h, d.out, -1, fold_opt(d.bn2, true)));
    } else {
      RUN(conv_forward(x, d.conv1, d.cat, d.y1, d.bn1));
      if (xform_ok(x, d.conv2, d.y1, d.h, d.y2)) {
        FwdOpt o2; o2.xbn = d.bn1; o2.xh = &d.h;
        RUN(conv_forward(x, d.conv2, d.y1, d.y2, d.bn2, o2));
      } else {
        RUN(bn_apply(x, d.bn1, d.y1, d.h, 0, nullptr, -1, true));
        RUN(conv_forward(x, d.conv2, d.h, d.y2, d.bn2));
      }
      if (!(hfold && l == 3) && !up_xf) RUN(bn_apply(x, d.bn2, d.y2, d.out, 0, nullptr, -1, true));
    }
    if (att) RUN(ch_att_forward(x, l));
  }
  {
    const Act& o = att ? p->atts[3].out2 : p->decs[3].out;
    HeadArgs h = {};
    h.x = x.A(o); h.ldx = o.ld;
    if (hfold) {  // the head reads decoder1's raw conv output and applies its last BN + ReLU
      const Dec& d = p->decs[3];
      h.x = x.A(d.y2); h.ldx = d.y2.ld;
      h.bn = bn_launch(x, d.bn2, (int64_t)N * d.y2.H * d.y2.W);
      h.bn_fold = 1;
    }
    h.w0 = prm[p->up0_w]; h.b0 = prm[p->up0_b]; h.wf = prm[p->fin_w]; h.bf = prm[p->fin_b];
    h.logits = logits;
    h.N = N; h.H = o.H; h.W = o.W; h.Cin = o.C; h.Co = (int)p->params[p->up0_b].numel;
    h.K = p->cfg.n_classes;
    ProfScope ps(p, st, hfold ? "head_fwd +bn" : "head_fwd", 0);
    CK(launch_head_fwd(h, st));
  }
  return 0;
}

int run_backward(unet_plan* p, const float* image, const float* dlogits, const float* const* prm, char* ws,
                        float* grads, hipStream_t st) {
  Ctx x{p, ws, prm, nullptr, st, 1};
  const int N = p->cfg.N;
  wgrad_reset();  // nothing queued by an earlier backward that failed midway
  p->pend.n = 0;
  p->wgb.clear();
  p->wgb_names.clear();
  p->wgb_flops = 0;
  if (p->want_events) RUN(ensure_events(p));
  if (!p->bwd_zeroed || p->bwd_zeroed_ws != ws) CK(hipMemsetAsync(ws + p->zero_bwd_off, 0, p->zero_bwd_bytes, st));
  p->bwd_zeroed = false;
  p->bwd_zeroed_ws = nullptr;
  const bool att = !p->atts.empty();
  // head (upconv0 + conv_final)
  {
    const Act& o = att ? p->atts[3].out2 : p->decs[3].out;
    HeadArgs h = {};
    h.x = x.A(o); h.ldx = o.ld;
    h.w0 = prm[p->up0_w]; h.b0 = prm[p->up0_b]; h.wf = prm[p->fin_w]; h.bf = prm[p->fin_b];
    h.dl = dlogits;
    const Act& hdx = att ? p->atts[3].d_out2 : p->decs[3].d_out;
    h.dx = x.A(hdx); h.lddx = hdx.ld;
    h.usum = x.W<double>(p->head_usum);
    h.gw0 = grads + p->params[p->up0_w].flat; h.gb0 = grads + p->params[p->up0_b].flat;
    h.gwf = grads + p->params[p->fin_w].flat; h.gbf = grads + p->params[p->fin_b].flat;
    h.N = N; h.H = o.H; h.W = o.W; h.Cin = o.C; h.Co = (int)p->params[p->up0_b].numel;
    h.K = p->cfg.n_classes;
    if (!att) {  // the head produces dA of decoder1's last BN: reduce it here
      const Dec& d = p->decs[3];
      h.bb = bwd_args(x, d.bn2, d.d_out, d.out, d.y2, d.dy2, -1, nullptr, nullptr, grads);
      if (p->head_bn_fold) {  // the forward never stored act: recomputed from y2 (same bits)
        h.x = x.A(d.y2); h.ldx = d.y2.ld;
        h.bb.act = nullptr;
        h.bn = bn_launch(x, d.bn2, (int64_t)N * d.y2.H * d.y2.W);
        h.bn_fold = 1;
      }
    }
    ProfScope ps(p, st, h.bn_fold ? "head_bwd +bn" : "head_bwd", 0);
    CK(launch_head_bwd(h, st));
    CK(launch_head_grads(h, st));
  }
  // BN-backward reductions are fused into the conv dgrad that produces each
  // BN's dA (all but decoder1's second BN, fed by the head, and the stem BN).
  const int nb = (int)p->blocks.size();
  auto dec_bn1 = [&](int l) {
    Dec& d = p->decs[l];
    return bwd_args(x, d.bn1, d.dh, d.h, d.y1, d.dy1, -1, nullptr, nullptr, grads);
  };
  auto dec_bn2 = [&](int l) {
    Dec& d = p->decs[l];
    return bwd_args(x, d.bn2, d.d_out, d.out, d.y2, d.dy2, -1, nullptr, nullptr, grads);
  };
  auto blk_bn1 = [&](int i) {
    Block& b = p->blocks[i];
    return bwd_args(x, b.bn1, b.dh, b.h, b.y1, b.dy1, -1, nullptr, nullptr, grads);
  };
  // the block's last BN (bn2 of a BasicBlock, bn3 of a Bottleneck), paired
  // with the downsample BN when the block has one
  auto blk_bn2 = [&](int i) {
    Block& b = p->blocks[i];
    const int bl = b.last_bn();
    const Act& yl = b.last_y();
    const Act& dyl = b.last_dy();
    if (b.ds >= 0) return bwd_args(x, bl, b.d_out, b.out, yl, dyl, b.dsbn, &b.yds, &b.dyds, grads);
    return bwd_args(x, bl, b.d_out, b.out, yl, dyl, -1, nullptr, nullptr, grads);
  };
  // decoder1 .. decoder4 (+ their up-convs)
  for (int l = 3; l >= 0; --l) {
    Dec& d = p->decs[l];
    if (att) {  // ChannelAttention backward: dOut2 -> dZ of the decoder's last BN (its reduction fused)
      ChAttArgs c = ch_args(x, l, grads);
      c.bb = dec_bn2(l);
      {
        ProfScope ps(p, st, "ch_att_bwd", 0);
        for (int pass = 3; pass < 6; ++pass) CK(launch_ch_att(c, pass, st));
      }
      RUN(bn_backward(x, d.bn2, c.bb));
    } else {
      RUN(bn_backward(x, d.bn2, dec_bn2(l)));
    }
    RUN(conv_wgrad(x, d.conv2, d.dy2, d.h));
    const BnBwdArgs f1 = dec_bn1(l);
    DgradOpt o2; o2.fuse = &f1;
    RUN(conv_dgrad(x, d.conv2, d.dy2, d.dh, nullptr, o2));
    RUN(bn_backward(x, d.bn1, f1));
    RUN(conv_wgrad(x, d.conv1, d.dy1, d.cat));
    DgradOpt o1; o1.dx_split = d.split ? &d.dcat_up : nullptr;
    RUN(conv_dgrad(x, d.conv1, d.dy1, d.dcat, nullptr, o1));
    // (decoder conv bias gradients: exactly 0, written by bucket 0's unpack)
    // up-conv: dU = dcat[:, skip:]; its dgrad is dA of the previous decoder's
    // (or enc4's) last BN
    if (att) {  // AttentionGate backward (skip gradient -> dskip, g-path gradient added into du)
      Att& t = p->atts[l];
      AttGateArgs a = gate_args(x, l, grads);
      // relu(BN_g + BN_x) backward: its reduction runs inside the gate's apply
      // pass (which produces dA and already reads the relu output)
      a.bb = bwd_args(x, t.bng, t.dS, t.s, t.g1, t.dg1, t.bnx, &t.xa, &t.dxa, grads);
      {
        ProfScope ps(p, st, "att_gate_bwd", 0);
        CK(launch_att_gate(a, 2, st));
        CK(launch_att_gate(a, 3, st));
      }
      RUN(bn_backward(x, t.bng, a.bb));
      RUN(conv_wgrad(x, t.wg, t.dg1, d.up_out));
      RUN(conv_wgrad(x, t.wx, t.dxa, t.x));
      RUN(conv_dgrad(x, t.wg, t.dg1, t.du, &d.dcat_up));
      RUN(conv_dgrad(x, t.wx, t.dxa, t.dskip, &t.dxpsi));
      // (W_g / W_x / psi conv bias gradients: exactly 0, written by bucket 0's unpack)
    }
    const Conv& up = p->convs[d.up];
    const Act du = att ? p->atts[l].du : d.dcat_up;
    RUN(conv_wgrad(x, d.up, du, d.up_in));
    const BnBwdArgs fu = l > 0 ? dec_bn2(l - 1) : blk_bn2(nb - 1);
    // with attention the up-conv input of levels 3..1 is the channel-gated
    // output: its gradient is not dA of a BN
    const bool fuse_up = l == 0 || !att;
    // the bias gradient (replicas -> fp32 in bucket 0's unpack launch, UP_D2F)
    // rides in the data-gradient pass when its kernel covers the shape
    bool bias_fused = false;
    DgradOpt ou;
    ou.fuse = fuse_up ? &fu : nullptr; ou.bias_acc = x.W<double>(up.bias_acc); ou.bias_done = &bias_fused;
    RUN(conv_dgrad(x, d.up, du, d.d_up_in, nullptr, ou));
    if (!bias_fused) {
      ProfScope ps(p, x.st, "bias_sum", 0);
      CK(launch_channel_sum(x.A(du), du.ld, (int64_t)N * du.H * du.W, up.Co, x.W<double>(up.bias_acc), x.st));
    }
  }
  // bucket 0 also holds the head's and the decoder biases' gradients
  RUN(unpack_bucket(x, 0, grads));
  if (p->nevents) CK(hipEventRecord(p->events[0], x.st));
  // encoder blocks, deepest first
  for (int i = nb - 1; i >= 0; --i) {
    Block& b = p->blocks[i];
    // the last writer of d_in produces dA of the previous block's last BN
    BnBwdArgs fp = {};
    const BnBwdArgs* fprev = nullptr;
    if (i > 0) { fp = blk_bn2(i - 1); fprev = &fp; }
    DgradOpt oprev; oprev.fuse = fprev;
    RUN(bn_backward(x, b.last_bn(), blk_bn2(i)));  // dY of the last conv (+ dY of the downsample BN)
    if (b.bottleneck()) {
      RUN(conv_wgrad(x, b.conv3, b.dy3, b.h2));
      if (b.ds >= 0) RUN(conv_wgrad(x, b.ds, b.dyds, b.in));
      const BnBwdArgs f2 = bwd_args(x, b.bn2, b.dh2, b.h2, b.y2, b.dy2, -1, nullptr, nullptr, grads);
      DgradOpt o3; o3.fuse = &f2;
      RUN(conv_dgrad(x, b.conv3, b.dy3, b.dh2, nullptr, o3));
      RUN(bn_backward(x, b.bn2, f2));
      RUN(conv_wgrad(x, b.conv2, b.dy2, b.h));
      const BnBwdArgs f1 = blk_bn1(i);
      DgradOpt o2; o2.fuse = &f1;
      RUN(conv_dgrad(x, b.conv2, b.dy2, b.dh, nullptr, o2));
      RUN(bn_backward(x, b.bn1, f1));
      RUN(conv_wgrad(x, b.conv1, b.dy1, b.in));
      if (b.ds >= 0) {
        // downsample (1x1 / stride) data gradient (+ the skip-concat gradient
        // of the input), then conv1's (1x1) added to it with the previous
        // block's BN-backward reduction in the epilogue
        RUN(conv_dgrad(x, b.ds, b.dyds, b.dds, b.skip_add.ld ? &b.skip_add : nullptr));
        RUN(conv_dgrad(x, b.conv1, b.dy1, b.d_in, &b.dds, oprev));
      } else {
        RUN(conv_dgrad(x, b.conv1, b.dy1, b.d_in, &b.d_out, oprev));  // identity path: d_out holds dZ of bn3
      }
    } else {
      RUN(conv_wgrad(x, b.conv2, b.dy2, b.h));
      const bool dsfold = ds_fold_ok(x, b);
      if (b.ds >= 0 && !dsfold) RUN(conv_wgrad(x, b.ds, b.dyds, b.in));
      const BnBwdArgs f1 = blk_bn1(i);
      DgradOpt o2; o2.fuse = &f1;
      RUN(conv_dgrad(x, b.conv2, b.dy2, b.dh, nullptr, o2));
      RUN(bn_backward(x, b.bn1, f1));
      RUN(conv_wgrad(x, b.conv1, b.dy1, b.in, dsfold ? b.ds : -1, &b.dyds));
      if (b.ds >= 0) {
        // conv1 (3x3/s2) and downsample (1x1/s2) data gradients in one launch
        oprev.ds = b.ds; oprev.dyds = &b.dyds;
        RUN(conv_dgrad(x, b.conv1, b.dy1, b.d_in, b.skip_add.ld ? &b.skip_add : nullptr, oprev));
      } else {
        RUN(conv_dgrad(x, b.conv1, b.dy1, b.d_in, &b.d_out, oprev));  // identity path: d_out holds dZ of bn2
      }
    }
    // bucket boundaries: enc4 done at i == 13, enc3 at i == 7
    if (i == 13 || i == 7) {
      const int bk = i == 13 ? 1 : 2;
      RUN(unpack_bucket(x, bk, grads));
      if (p->nevents) CK(hipEventRecord(p->events[bk], x.st));
    }
  }
  // bucket 3 (enc2 + enc1) is final: its all-reduce overlaps the stem's backward
  {
    const int bk = (int)p->buckets.size() - 2;
    RUN(unpack_bucket(x, bk, grads));
    if (p->nevents) CK(hipEventRecord(p->events[bk], x.st));
  }
  // maxpool + stem.  dY of the stem is never stored: both paths form it from
  // dZ and y inside the stem weight gradient
  const Act skip = att ? p->atts[3].dskip : slice(p->decs[3].dcat, 0, p->x1.C);
  BnBwdArgs sb = bwd_args(x, p->stem_bn, p->d_x1, p->x1, p->y0, Act(), -1, nullptr, nullptr, grads);
  sb.dy = nullptr;
  if (p->stem_rc) {
    // one pass: maxpool backward, stem BN backward, stem weight gradient
    StemRcArgs s = stem_rc_args(x, image);
    s.dpool = x.A(p->d_p0); s.lddpool = p->d_p0.ld;
    s.add = x.A(skip); s.ldadd = skip.ld;
    s.mean = sb.mean; s.invstd = sb.invstd;
    if (p->stem_keep) { s.dz = x.A(p->d_x1); s.lddz = p->d_x1.ld; }
    s.part = x.W<float>(p->stem_part);
    s.l2 = reinterpret_cast<double*>(s.part + stem_rc_l2_offset(N, p->y0.H, p->y0.W, p->x1.C) / sizeof(float));
    s.tot = x.W<double>(p->stem_tot);
    s.tkt = x.W<unsigned>(p->stem_tkt);
    s.imsum = reinterpret_cast<float*>(reinterpret_cast<char*>(s.tot) + stem_rc_imsum_offset(p->x1.C));
    s.dw = x.W<float>(p->convs[p->stem_conv].wacc);
    s.dgamma = sb.dgamma; s.dbeta = sb.dbeta;
    s.npix = (int64_t)N * p->y0.H * p->y0.W;
    {
      ProfScope ps(p, st, "wgrad input_conv.weight +maxpool+bn", 3.0 * 2.0 * N * p->y0.H * p->y0.W * p->x1.C * 49);
      s.tim = tim_slot(p, "wgrad input_conv.weight +maxpool+bn");
      CK(launch_stem_rc_bwd(s, 0, st));
    }
    {
      ProfScope ps(p, st, "wgrad_reduce input_conv.weight", 0);
      CK(launch_stem_rc_bwd(s, 1, st));
    }
  } else {
    MaxPoolArgs m = {};
    m.dy = x.A(p->d_p0); m.lddy = p->d_p0.ld; m.idx = x.W<uint8_t>(p->pidx);
    m.add = x.A(skip); m.ldadd = skip.ld;
    m.dx = x.A(p->d_x1); m.lddx = p->d_x1.ld;
    m.N = N; m.H = p->x1.H; m.W = p->x1.W; m.C = p->x1.C; m.P = p->p0.H; m.Q = p->p0.W;
    m.bb = sb;  // the maxpool backward produces dA of the stem BN: its reduction rides here
    {
      ProfScope ps(p, st, "maxpool_bwd", 0);
      CK(launch_maxpool_bwd(m, st));
    }
    const Conv& cv = p->convs[p->stem_conv];
    ConvWgradArgs a = {};
    a.bn = sb; a.bn_fuse = 1;
    a.dw = x.W<float>(cv.wacc);
    a.N = N; a.H = p->cfg.H; a.W = p->cfg.W; a.C = 1;
    a.P = p->y0.H; a.Q = p->y0.W; a.Cout = cv.Co;
    a.R = 7; a.S = 7; a.stride = 2; a.pad = 3;
    a.x = reinterpret_cast<const bf16_t*>(image);
    RUN(wgrad_and_reduce(x, a, 1, "input_conv.weight", 2.0 * N * p->y0.H * p->y0.W * cv.Co * 49));
  }
  {
    const int bk = (int)p->buckets.size() - 1;
    RUN(unpack_bucket(x, bk, grads));
    if (p->nevents) CK(hipEventRecord(p->events[bk], x.st));
  }
  return 0;
}
