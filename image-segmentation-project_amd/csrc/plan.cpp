// Plan construction: the parameter table in reference state_dict order, the
// workspace layout, the DDP gradient buckets and the named views of one U-Net
// configuration (unet_plan_create).
#include "plan.h"

namespace {

struct Alloc {
  size_t top = 0;
  size_t take(size_t bytes) {
    const size_t off = top;
    top += (bytes + 255) & ~size_t(255);
    return off;
  }
};

int add_param(unet_plan* p, const std::string& name, std::vector<int64_t> shape) {
  Param q;
  q.name = name;
  q.shape = shape;
  q.numel = 1;
  for (auto s : shape) q.numel *= s;
  q.flat = p->grad_numel;
  p->grad_numel += q.numel;
  p->params.push_back(q);
  return (int)p->params.size() - 1;
}

int add_bn(unet_plan* p, const std::string& prefix, int C) {
  Bn b;
  b.gamma = add_param(p, prefix + ".weight", {C});
  b.beta = add_param(p, prefix + ".bias", {C});
  b.idx = (int)p->bns.size();
  b.C = C;
  p->bns.push_back(b);
  return b.idx;
}

int add_conv(unet_plan* p, const std::string& prefix, int kind, int Ci, int Co, int R, int stride, int pad,
             bool bias) {
  Conv c;
  c.kind = kind;
  c.Ci = Ci; c.Co = Co; c.R = R; c.S = R; c.stride = stride; c.pad = pad;
  if (kind == L_CONVT) c.w = add_param(p, prefix + ".weight", {Ci, Co, R, R});
  else c.w = add_param(p, prefix + ".weight", {Co, Ci, R, R});
  if (bias) c.b = add_param(p, prefix + ".bias", {Co});
  p->convs.push_back(c);
  return (int)p->convs.size() - 1;
}

Act act(Alloc& A, int N, int H, int W, int C) {
  Act a;
  a.off = A.take((size_t)N * H * W * C * 2);
  a.ld = C; a.C = C; a.H = H; a.W = W;
  return a;
}

}  // namespace

int build_plan(unet_plan* p) {
  const unet_config& c = p->cfg;
  const int N = c.N, H = c.H, W = c.W, w = c.width;
  if (H % 32 || W % 32 || N <= 0 || w <= 0) {
    set_err("unet_plan_create: H and W must be multiples of 32 (advanced_models.py:317-347 crops "
            "only fix the last two levels)");
    return 1;
  }
  if (c.n_classes < 1 || c.n_classes > kHeadMaxClasses) {
    set_err("unet_plan_create: n_classes must be 1..16 (the fused head contracts upconv0 with conv_final; "
            "above upconv0's output channels the contracted form does more work than the two convs)");
    return 1;
  }
  const bool r50 = c.backbone == 50;
  if (c.backbone != 0 && c.backbone != 34 && c.backbone != 50) {
    set_err("unet_plan_create: backbone must be 34 (resnet34) or 50 (resnet50)");
    return 1;
  }
  if (r50 && w != 1) { set_err("unet_plan_create: resnet50 is built at width 1 only"); return 1; }
  if (c.fp8 && (r50 || c.attention)) {
    set_err("unet_plan_create: the fp8 forward is built for the resnet34 U-Net without attention (Wide / Base)");
    return 1;
  }
  // stage output channels (x2..x5): resnet34 64..512, resnet50 (expansion 4) 256..2048
  const int c0 = 64 * w, c1 = 128 * w, c2 = 256 * w, c3 = 512 * w;
  const int chan[4] = {r50 ? 256 : c0, r50 ? 512 : c1, r50 ? 1024 : c2, r50 ? 2048 : c3};
  const int planes[4] = {64, 128, 256, 512};
  const int nblk[4] = {3, 4, 6, 3};

  // ---- parameters, in reference registration order ----
  p->stem_conv = add_conv(p, "input_conv", L_STEM, 1, c0, 7, 2, 3, false);
  p->stem_bn = add_bn(p, "bn1", c0);
  struct BlkSpec { int conv1, bn1, conv2, bn2, conv3, bn3, ds, dsbn, cin, cout, mid, stride, stage; };
  std::vector<BlkSpec> specs;
  int cin = c0;
  for (int s = 0; s < 4; ++s) {
    for (int b = 0; b < nblk[s]; ++b) {
      const std::string pre = "enc" + std::to_string(s + 1) + "." + std::to_string(b);
      const int stride = (b == 0 && s > 0) ? 2 : 1;
      const int cout = chan[s];
      BlkSpec bs;
      bs.conv3 = bs.bn3 = -1;
      if (r50) {  // torchvision Bottleneck: 1x1 -> 3x3/stride -> 1x1 (x4)
        const int mid = planes[s];
        bs.conv1 = add_conv(p, pre + ".conv1", L_CONV, cin, mid, 1, 1, 0, false);
        bs.bn1 = add_bn(p, pre + ".bn1", mid);
        bs.conv2 = add_conv(p, pre + ".conv2", L_CONV, mid, mid, 3, stride, 1, false);
        bs.bn2 = add_bn(p, pre + ".bn2", mid);
        bs.conv3 = add_conv(p, pre + ".conv3", L_CONV, mid, cout, 1, 1, 0, false);
        bs.bn3 = add_bn(p, pre + ".bn3", cout);
        bs.mid = mid;
      } else {
        bs.conv1 = add_conv(p, pre + ".conv1", L_CONV, cin, cout, 3, stride, 1, false);
        bs.bn1 = add_bn(p, pre + ".bn1", cout);
        bs.conv2 = add_conv(p, pre + ".conv2", L_CONV, cout, cout, 3, 1, 1, false);
        bs.bn2 = add_bn(p, pre + ".bn2", cout);
        bs.mid = cout;
      }
      bs.ds = bs.dsbn = -1;
      if (stride != 1 || cin != cout) {
        bs.ds = add_conv(p, pre + ".downsample.0", L_CONV, cin, cout, 1, stride, 0, false);
        bs.dsbn = add_bn(p, pre + ".downsample.1", cout);
      }
      bs.cin = cin; bs.cout = cout; bs.stride = stride; bs.stage = s;
      specs.push_back(bs);
      cin = cout;
    }
  }
  const int enc_end_param = (int)p->params.size();
  // decoder: level 4 (deepest) .. 1
  struct DecSpec { int up, conv1, bn1, conv2, bn2, upin, upout, skipc, outc; };
  std::vector<DecSpec> dspecs;
  {
    // advanced_models.py:89-100 (resnet34) / :119-130 (resnet50)
    const int upin[4] = {chan[3], chan[2], chan[1], chan[0]};
    const int upout[4] = {chan[2], chan[1], chan[0], r50 ? c0 : c0 / 2};
    const int skipc[4] = {chan[2], chan[1], chan[0], c0};
    const int outc[4] = {chan[2], chan[1], chan[0], r50 ? c0 : c0 / 2};
    for (int l = 0; l < 4; ++l) {
      const int lvl = 4 - l;
      DecSpec d;
      d.up = add_conv(p, "upconv" + std::to_string(lvl), L_CONVT, upin[l], upout[l], 2, 2, 0, true);
      const std::string pre = "decoder" + std::to_string(lvl);
      const int catc = skipc[l] + upout[l];
      d.conv1 = add_conv(p, pre + ".0", L_CONV, catc, outc[l], 3, 1, 1, true);
      d.bn1 = add_bn(p, pre + ".1", outc[l]);
      d.conv2 = add_conv(p, pre + ".3", L_CONV, outc[l], outc[l], 3, 1, 1, true);
      d.bn2 = add_bn(p, pre + ".4", outc[l]);
      d.upin = upin[l]; d.upout = upout[l]; d.skipc = skipc[l]; d.outc = outc[l];
      dspecs.push_back(d);
    }
  }
  const int up0_in = dspecs[3].outc;  // 32 (resnet34) / 64 (resnet50), advanced_models.py:158-159
  p->up0_w = add_param(p, "upconv0.weight", {up0_in, c0 / 4, 2, 2});
  p->up0_b = add_param(p, "upconv0.bias", {c0 / 4});
  p->fin_w = add_param(p, "conv_final.weight", {c.n_classes, c0 / 4, 1, 1});
  p->fin_b = add_param(p, "conv_final.bias", {c.n_classes});
  if (c.attention) {  // advanced_models.py:163-172 / :175-183, registered after conv_final
    const int fi34[4] = {c1, c0, c0 / 2, c0 / 2}, fi50[4] = {512, 256, 128, 32};
    const int* fi = r50 ? fi50 : fi34;
    for (int l = 0; l < 4; ++l) {
      const std::string pre = "attention" + std::to_string(4 - l);
      Att t;
      t.Fg = dspecs[l].upout; t.Fl = dspecs[l].skipc; t.Fi = fi[l];
      t.wg = add_conv(p, pre + ".W_g.0", L_CONV, t.Fg, t.Fi, 1, 1, 0, true);
      t.bng = add_bn(p, pre + ".W_g.1", t.Fi);
      t.wx = add_conv(p, pre + ".W_x.0", L_CONV, t.Fl, t.Fi, 1, 1, 0, true);
      t.bnx = add_bn(p, pre + ".W_x.1", t.Fi);
      t.psi_w = add_param(p, pre + ".psi.0.weight", {1, t.Fi, 1, 1});
      t.psi_b = add_param(p, pre + ".psi.0.bias", {1});
      t.psibn = add_bn(p, pre + ".psi.1", 1);
      p->atts.push_back(t);
    }
    for (int l = 0; l < 4; ++l) {
      const std::string pre = "ch_attention" + std::to_string(4 - l);
      Att& t = p->atts[l];
      t.C = dspecs[l].outc; t.Cr = t.C / 16;
      t.fc1 = add_param(p, pre + ".fc.0.weight", {t.Cr, t.C, 1, 1});
      t.fc2 = add_param(p, pre + ".fc.2.weight", {t.C, t.Cr, 1, 1});
    }
  }

  // ---- DDP buckets in backward completion order ----
  auto stage_range = [&](int s) {
    int lo = -1, hi = -1;
    const std::string pre = "enc" + std::to_string(s + 1) + ".";
    for (int i = 0; i < (int)p->params.size(); ++i)
      if (p->params[i].name.rfind(pre, 0) == 0) { if (lo < 0) lo = i; hi = i; }
    return std::make_pair(lo, hi);
  };
  {
    const int64_t dec_begin = p->params[enc_end_param].flat;
    p->buckets.push_back({dec_begin, p->grad_numel});
    auto r4 = stage_range(3), r3 = stage_range(2), r1 = stage_range(0);
    p->buckets.push_back({p->params[r4.first].flat, p->params[r4.second].flat + p->params[r4.second].numel});
    p->buckets.push_back({p->params[r3.first].flat, p->params[r3.second].flat + p->params[r3.second].numel});
    // enc2 + enc1 final before the stem's backward, so only the stem's 3.3 k
    // parameters (bucket 4) trail the backward
    p->buckets.push_back({p->params[r1.first].flat, p->params[r3.first].flat});
    p->buckets.push_back({0, p->params[r1.first].flat});
  }
  static_assert(sizeof(((unet_plan*)nullptr)->events) / sizeof(hipEvent_t) >= 5, "one event per bucket");

  // ---- workspace ----
  Alloc A;
  // zeroed at forward start: BN fwd sums
  p->zero_fwd_off = A.take(0);
  for (auto& b : p->bns) b.stats = A.take((size_t)kStatRep * 2 * b.C * sizeof(double));
  for (int l = 0; l < (int)p->atts.size(); ++l) {
    Att& t = p->atts[l];
    t.pst = A.take(2 * sizeof(double));
    t.psum = A.take((size_t)N * t.C * sizeof(double));
    t.pkey = A.take((size_t)N * t.C * sizeof(unsigned long long));
  }
  p->zero_fwd_bytes = A.top - p->zero_fwd_off;
  // zeroed at backward start: BN bwd sums, convT bias sums, head sums, wgrad accumulators
  p->zero_bwd_off = A.take(0);
  for (auto& b : p->bns) b.bsums = A.take((size_t)kStatRep * 2 * b.C * sizeof(double));
  for (auto& cv : p->convs)
    if (cv.kind == L_CONVT) cv.bias_acc = A.take((size_t)kStatRep * cv.Co * sizeof(double));
  // [kStatRep][K * (Cin*4 + 1)]
  p->head_usum = A.take((size_t)kStatRep * c.n_classes * (up0_in * 4 + 1) * sizeof(double));
  p->stem_tkt = A.take(kStemTickets * sizeof(unsigned));
  for (auto& t : p->atts) {
    t.pbs = A.take(2 * sizeof(double));
    t.cda = A.take((size_t)N * t.C * sizeof(double));
    t.gpsi = A.take((size_t)kStatRep * t.Fi * sizeof(double));
    t.gfc = A.take((size_t)kStatRep * 2 * t.C * t.Cr * sizeof(double));
  }
  p->zero_bwd_bytes = A.top - p->zero_bwd_off;  // starts where the forward's region ends: one fill spans both
  // weight-gradient accumulators: every element is WRITTEN by its wgrad launch
  // (deterministic split-K slab reduction, kernels.h SlabLayout), so they are
  // not zeroed
  for (auto& cv : p->convs) {
    size_t n;
    if (cv.kind == L_STEM) n = (size_t)cv.Co * 64;
    else n = (size_t)cv.Co * cv.Ci * cv.R * cv.S;
    cv.wacc = A.take(n * sizeof(float));
  }
  for (auto& b : p->bns) b.save = A.take((size_t)2 * b.C * sizeof(float));
  for (auto& cv : p->convs) {
    if (cv.kind == L_STEM) {
      cv.pk_fwd = A.take((size_t)cv.Co * 64 * 2);
    } else {
      const size_t n = (size_t)cv.Co * cv.Ci * cv.R * cv.S * 2;
      cv.pk_fwd = A.take(n);
      cv.pk_dgrad = A.take(n);
    }
  }

  // forward activations
  const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4;
  Act cat1 = act(A, N, H2, W2, c0 + dspecs[3].upout);
  p->x1 = c.attention ? act(A, N, H2, W2, c0) : slice(cat1, 0, c0);
  p->y0 = act(A, N, H2, W2, c0);
  p->p0 = act(A, N, H4, W4, c0);
  p->pidx = A.take((size_t)N * H4 * W4 * c0);
  p->stem_rc = p->stem_rc && stem_rc_ok(c0, H2, W2) && H2 == 2 * H4 && W2 == 2 * W4 && H == 2 * H2 && W == 2 * W2;
  if (p->stem_rc) {
    p->stem_part = A.take(stem_rc_part_bytes(N, H2, W2, c0));
    p->stem_tot = A.take(stem_rc_tot_bytes(c0));
  }
  // split-K partials of one weight-gradient launch (register-native layout);
  // launchers cap their split count to what fits
  p->wslab_bytes = (size_t)(64 * w * w) << 20;
  p->wslab = A.take(2 * p->wslab_bytes);  // two slabs, alternating
  Act cats[4];  // cats[l] for decoder level index l (0 = level 4)
  cats[3] = cat1;
  cats[2] = act(A, N, H4, W4, 2 * chan[0]);
  cats[1] = act(A, N, H / 8, W / 8, 2 * chan[1]);
  cats[0] = act(A, N, H / 16, W / 16, 2 * chan[2]);
  Act x5 = act(A, N, H / 32, W / 32, chan[3]);

  Act prev = p->p0;
  for (size_t i = 0; i < specs.size(); ++i) {
    const BlkSpec& s = specs[i];
    Block b;
    b.conv1 = s.conv1; b.bn1 = s.bn1; b.conv2 = s.conv2; b.bn2 = s.bn2; b.ds = s.ds; b.dsbn = s.dsbn;
    b.conv3 = s.conv3; b.bn3 = s.bn3;
    const int Hs = H4 >> s.stage, Ws = W4 >> s.stage;
    b.in = prev;
    if (b.bottleneck()) {  // conv1 (1x1) at the input resolution, the stride sits on conv2
      b.y1 = act(A, N, prev.H, prev.W, s.mid);
      b.h = act(A, N, prev.H, prev.W, s.mid);
      b.y2 = act(A, N, Hs, Ws, s.mid);
      b.h2 = act(A, N, Hs, Ws, s.mid);
      b.y3 = act(A, N, Hs, Ws, s.cout);
    } else {
      b.y1 = act(A, N, Hs, Ws, s.cout);
      b.h = act(A, N, Hs, Ws, s.cout);
      b.y2 = act(A, N, Hs, Ws, s.cout);
    }
    if (s.ds >= 0) b.yds = act(A, N, Hs, Ws, s.cout);
    const bool last = (i + 1 == specs.size()) || specs[i + 1].stage != s.stage;
    if (last) {
      if (s.stage == 3) b.out = x5;
      else if (c.attention) b.out = act(A, N, Hs, Ws, s.cout);  // gated copy goes into the concat
      else b.out = slice(cats[2 - s.stage], 0, s.cout);  // x2->cat2, x3->cat3, x4->cat4
    } else {
      b.out = act(A, N, Hs, Ws, s.cout);
    }
    p->blocks.push_back(b);
    prev = b.out;
  }
  Act dec_in = x5;
  for (int l = 0; l < 4; ++l) {
    const DecSpec& s = dspecs[l];
    Dec d;
    d.up = s.up; d.conv1 = s.conv1; d.bn1 = s.bn1; d.conv2 = s.conv2; d.bn2 = s.bn2;
    d.cat = cats[l];
    d.up_in = dec_in;
    d.up_out = slice(cats[l], s.skipc, s.upout);
    const int Hl = d.cat.H, Wl = d.cat.W;
    d.y1 = act(A, N, Hl, Wl, s.outc);
    d.h = act(A, N, Hl, Wl, s.outc);
    d.y2 = act(A, N, Hl, Wl, s.outc);
    d.out = act(A, N, Hl, Wl, s.outc);
    p->decs.push_back(d);
    dec_in = d.out;
    if (c.attention) {
      Att& t = p->atts[l];
      const int64_t np = (int64_t)N * Hl * Wl;
      t.g1 = act(A, N, Hl, Wl, t.Fi);
      t.xa = act(A, N, Hl, Wl, t.Fi);
      t.s = act(A, N, Hl, Wl, t.Fi);
      t.p = A.take(np * sizeof(float));
      t.psi = A.take(np * sizeof(float));
      t.dbnp = A.take(np * sizeof(float));
      t.psave = A.take(2 * sizeof(float));
      t.ca = A.take((size_t)N * t.C * sizeof(float));
      t.ch = A.take((size_t)N * 2 * t.Cr * sizeof(float));
      t.cam = A.take((size_t)N * 2 * t.C * sizeof(float));
      t.cdam = A.take((size_t)N * 2 * t.C * sizeof(float));
      t.out2 = act(A, N, Hl, Wl, t.C);
      t.d_out2 = act(A, N, Hl, Wl, t.C);
      t.dS = act(A, N, Hl, Wl, t.Fi);
      t.dg1 = act(A, N, Hl, Wl, t.Fi);
      t.dxa = act(A, N, Hl, Wl, t.Fi);
      t.dxpsi = act(A, N, Hl, Wl, t.Fl);
      t.dskip = act(A, N, Hl, Wl, t.Fl);
      t.du = act(A, N, Hl, Wl, t.Fg);
      dec_in = t.out2;
    }
  }
  if (c.attention) {  // skips: x4 = enc3 out, x3 = enc2 out, x2 = enc1 out, x1 = stem
    int last[3] = {-1, -1, -1};
    for (size_t i = 0; i < specs.size(); ++i)
      if (specs[i].stage < 3) last[specs[i].stage] = (int)i;
    p->atts[0].x = p->blocks[last[2]].out;
    p->atts[1].x = p->blocks[last[1]].out;
    p->atts[2].x = p->blocks[last[0]].out;
    p->atts[3].x = p->x1;
  }

  // fp8 forward: e4m3 weight packs and input copies of every conv with C >= 128
  if (c.fp8) {
    auto f8_input = [&](int ci, const Act& in) {
      Conv& cv = p->convs[ci];
      if (cv.kind != L_CONV || cv.Ci < 128 || cv.Ci % 16 || in.ld % 8) return;
      cv.f8 = true;
      cv.f8w = A.take((size_t)cv.Co * cv.Ci * cv.R * cv.S);
      cv.f8st = p->f8n++;
      for (auto& f : p->f8acts)
        if (f.src == in.off && f.C == in.C) return;
      F8Act f;
      f.src = in.off; f.C = in.C;
      f.q = A.take((size_t)N * in.H * in.W * in.C);
      f.st = p->f8n++;
      p->f8acts.push_back(f);
    };
    for (auto& b : p->blocks) {
      f8_input(b.conv1, b.in);
      f8_input(b.conv2, b.h);
      if (b.ds >= 0) f8_input(b.ds, b.in);
    }
    for (auto& d : p->decs) {
      f8_input(d.conv1, d.cat);
      f8_input(d.conv2, d.h);
    }
    p->f8st = A.take((size_t)p->f8n * sizeof(F8State));
    p->f8_done.assign(p->f8acts.size(), 0);
  }

  // 3x3 / s1 convs on the full-line halo kernel (conv_fl.hip): their packs
  // are chunk-major, every launch of them goes to that kernel
  {
    auto fl_mark = [&](int ci, const Act& in) {
      Conv& cv = p->convs[ci];
      if (cv.kind != L_CONV || cv.R != 3 || cv.S != 3 || cv.stride != 1 || cv.pad != 1) return;
      cv.fl_fwd = !cv.f8 && conv3x3_fl_shape(N, cv.Ci, cv.Co, in.H, in.W);
      cv.fl_dgrad = conv3x3_fl_shape(N, cv.Co, cv.Ci, in.H, in.W);
    };
    for (auto& b : p->blocks) {
      fl_mark(b.conv1, b.in);
      fl_mark(b.conv2, b.h);
    }
    for (auto& d : p->decs) {
      fl_mark(d.conv1, d.cat);
      fl_mark(d.conv2, d.h);
    }
  }

  // backward gradient tensors
  for (int l = 3; l >= 0; --l) {
    Dec& d = p->decs[l];
    const int Hl = d.cat.H, Wl = d.cat.W, oc = d.out.C;
    d.d_out = act(A, N, Hl, Wl, oc);
    d.dy2 = act(A, N, Hl, Wl, oc);
    d.dh = act(A, N, Hl, Wl, oc);
    d.dy1 = act(A, N, Hl, Wl, oc);
    const int upc = d.up_out.C, skc = d.cat.C - upc;
    d.split = upc * 2 < 128;
    if (d.split) {
      d.dcat = act(A, N, Hl, Wl, skc);
      d.dcat_up = act(A, N, Hl, Wl, upc);
    } else {
      d.dcat = act(A, N, Hl, Wl, d.cat.C);
      d.dcat_up = slice(d.dcat, skc, upc);
    }
  }
  for (int l = 0; l < 4; ++l) {
    Dec& d = p->decs[l];
    d.d_up_in = (l == 0) ? act(A, N, H / 32, W / 32, chan[3])
                         : (c.attention ? p->atts[l - 1].d_out2 : p->decs[l - 1].d_out);
  }
  for (auto& b : p->blocks) {
    b.dy1 = act(A, N, b.y1.H, b.y1.W, b.y1.C);
    b.dh = act(A, N, b.h.H, b.h.W, b.h.C);
    b.dy2 = act(A, N, b.y2.H, b.y2.W, b.y2.C);
    if (b.bottleneck()) {
      b.dh2 = act(A, N, b.h2.H, b.h2.W, b.h2.C);
      b.dy3 = act(A, N, b.y3.H, b.y3.W, b.y3.C);
      if (b.ds >= 0) b.dds = act(A, N, b.in.H, b.in.W, b.in.C);
    }
    const Act& o = b.out;
    if (b.ds >= 0) b.dyds = act(A, N, o.H, o.W, o.C);
  }
  // block output grads: last encoder block's d_out = decoder-4's d_up_in
  const int nb = (int)p->blocks.size();
  p->blocks[nb - 1].d_out = p->decs[0].d_up_in;
  for (int i = nb - 2; i >= 0; --i) {
    Block& b = p->blocks[i];
    b.d_out = act(A, N, b.out.H, b.out.W, b.out.C);
  }
  p->d_p0 = act(A, N, H4, W4, c0);
  for (int i = 0; i < nb; ++i) {
    Block& b = p->blocks[i];
    b.d_in = i == 0 ? p->d_p0 : p->blocks[i - 1].d_out;
    b.skip_add = Act();
    if (i > 0 && specs[i].stage != specs[i - 1].stage) {
      // input x_{s+1} also fed cat_{s+1} slice 0: add that slice's gradient
      const int s = specs[i].stage;            // 1..3
      const int l = 3 - s;                     // x2 (s=1) -> cats[2], x3 -> cats[1], x4 -> cats[0]
      b.skip_add = c.attention ? p->atts[l].dskip : slice(p->decs[l].dcat, 0, specs[i].cin);
    }
  }
  p->d_x1 = act(A, N, H2, W2, c0);
  p->ws_bytes = A.top;

  {
    const int hc = p->decs[3].out.C;
    p->head_bn_fold = p->head_bn_fold && p->atts.empty() && (hc == 32 || hc == 64) && p->decs[3].y2.C == hc;
  }

  // named views for tests: forward activations and their gradients
  auto& nm = p->named;
  const bool y0_stored = !p->stem_rc || p->stem_keep;  // recompute: y0 / dZ only kept for tests
  if (y0_stored) nm.push_back({"y0", p->y0});
  nm.push_back({"x1", p->x1}); nm.push_back({"p0", p->p0});
  if (y0_stored) nm.push_back({"d.x1", p->d_x1});
  nm.push_back({"d.p0", p->d_p0});
  {
    int bi = 0;
    for (int s = 0; s < 4; ++s)
      for (int k = 0; k < nblk[s]; ++k, ++bi) {
        const Block& b = p->blocks[bi];
        const std::string pre = "enc" + std::to_string(s + 1) + "." + std::to_string(k) + ".";
        nm.push_back({pre + "y1", b.y1}); nm.push_back({pre + "h", b.h}); nm.push_back({pre + "y2", b.y2});
        if (b.bottleneck()) {
          nm.push_back({pre + "h2", b.h2}); nm.push_back({pre + "y3", b.y3});
          nm.push_back({pre + "d.h2", b.dh2}); nm.push_back({pre + "d.y3", b.dy3});
        }
        if (b.ds >= 0) { nm.push_back({pre + "yds", b.yds}); nm.push_back({pre + "d.yds", b.dyds}); }
        nm.push_back({pre + "out", b.out});
        nm.push_back({pre + "d.out", b.d_out}); nm.push_back({pre + "d.y2", b.dy2});
        nm.push_back({pre + "d.h", b.dh}); nm.push_back({pre + "d.y1", b.dy1});
      }
  }
  for (int l = 0; l < 4; ++l) {
    const Dec& d = p->decs[l];
    const std::string pre = "dec" + std::to_string(4 - l) + ".";
    nm.push_back({pre + "up", d.up_out}); nm.push_back({pre + "cat", d.cat});
    nm.push_back({pre + "y1", d.y1}); nm.push_back({pre + "h", d.h}); nm.push_back({pre + "y2", d.y2});
    // (dec1.out: written by eval forwards; a training forward with head_bn_fold leaves it untouched)
    nm.push_back({pre + "out", d.out});
    nm.push_back({pre + "d.out", d.d_out}); nm.push_back({pre + "d.y2", d.dy2}); nm.push_back({pre + "d.h", d.dh});
    nm.push_back({pre + "d.y1", d.dy1});
    if (!p->atts.empty()) {
      const Att& t = p->atts[l];
      const std::string ap = "att" + std::to_string(4 - l) + ".";
      nm.push_back({ap + "x", t.x}); nm.push_back({ap + "g1", t.g1}); nm.push_back({ap + "xa", t.xa});
      nm.push_back({ap + "s", t.s}); nm.push_back({ap + "out2", t.out2}); nm.push_back({ap + "d.out2", t.d_out2});
      nm.push_back({ap + "d.S", t.dS}); nm.push_back({ap + "d.g1", t.dg1}); nm.push_back({ap + "d.xa", t.dxa});
      nm.push_back({ap + "d.skip", t.dskip}); nm.push_back({ap + "d.u", t.du});
    }
    if (d.split) { nm.push_back({pre + "d.cat.skip", d.dcat}); nm.push_back({pre + "d.cat.up", d.dcat_up}); }
    else nm.push_back({pre + "d.cat", d.dcat});
  }

  // unpack groups per bucket
  p->bucket_convs.assign(p->buckets.size(), {});
  for (int i = 0; i < (int)p->convs.size(); ++i) {
    const int64_t f = p->params[p->convs[i].w].flat;
    for (int bk = 0; bk < (int)p->buckets.size(); ++bk)
      if (f >= p->buckets[bk].first && f < p->buckets[bk].second) p->bucket_convs[bk].push_back(i);
  }

  // algorithmic FLOPs: 2*MACs; training = 3x fwd - stem dgrad
  double fw = 0, stem = 0;
  for (auto& cv : p->convs) {
    double macs;
    if (cv.kind == L_STEM) { macs = (double)N * H2 * W2 * cv.Co * 49; stem = 2 * macs; }
    else if (cv.kind == L_CONVT) {
      // input pixels x Ci x Co x 4
      int hin = 0;
      for (auto& d : p->decs) if (d.up >= 0 && &p->convs[d.up] == &cv) hin = d.up_in.H * d.up_in.W;
      macs = (double)N * hin * cv.Ci * cv.Co * 4;
    } else {
      macs = 0;
    }
    fw += 2 * macs;
  }
  for (auto& b : p->blocks) {
    auto cf = [&](int ci, const Act& o) {
      const Conv& cv = p->convs[ci];
      return 2.0 * N * o.H * o.W * cv.Ci * cv.Co * cv.R * cv.S;
    };
    fw += cf(b.conv1, b.y1) + cf(b.conv2, b.y2);
    if (b.bottleneck()) fw += cf(b.conv3, b.y3);
    if (b.ds >= 0) fw += cf(b.ds, b.yds);
  }
  for (auto& d : p->decs) {
    const double px = (double)N * d.y1.H * d.y1.W;
    fw += 2 * px * p->convs[d.conv1].Ci * p->convs[d.conv1].Co * 9;
    fw += 2 * px * p->convs[d.conv2].Ci * p->convs[d.conv2].Co * 9;
  }
  for (int l = 0; l < (int)p->atts.size(); ++l) {  // attention 1x1 convs + psi + channel MLP
    const Att& t = p->atts[l];
    const double px = (double)N * p->decs[l].y1.H * p->decs[l].y1.W;
    fw += 2 * px * t.Fi * (t.Fg + t.Fl + 1) + 2.0 * N * 2 * 2 * t.C * t.Cr;
  }
  fw += 2.0 * N * H2 * W2 * up0_in * (c0 / 4) * 4;  // upconv0
  fw += 2.0 * N * H * W * (c0 / 4) * c.n_classes;      // conv_final
  p->flops_fwd = fw;
  p->flops_train = 3 * fw - stem;

  // bucket events are created lazily; plan creation does query the current
  // device's CU count (device_cu_count: the full-line conv routing and the
  // chunk-major packs depend on it), so it initialises the HIP runtime and the
  // plan is bound to the device current at creation
  return 0;
}

int ensure_events(unet_plan* p) {
  if (p->nevents) return 0;
  const int nb = (int)p->buckets.size();
  for (int i = 0; i < nb; ++i) CK(hipEventCreateWithFlags(&p->events[i], hipEventDisableTiming));
  p->nevents = nb;
  return 0;
}
