"""Every conv dispatch instance and every fused epilogue as a SINGLE op, through
the C-ABI entry unet_conv_ex (one launch with the whole ConvFwdArgs epilogue),
against torch fp32 on the same bf16-rounded operands (CPU reference).

The ops underneath are the reference's BasicBlock / decoder convs and their
BatchNorm2d (advanced_models.py:72-100,197-205).  unet_conv_fwd reaches only
bias / addend / BN sums; the fused BN(+ReLU) backward (one and two BNs), the
folded downsample data gradient (x2 / w2), the split concat gradient (ysplit),
the eval-mode BN fold and the forward downsample fold (wds / yds) were seen
only by the model-level tests, at relative L2 <= 2e-2 per tensor and on
whichever template instance the fixture shapes happened to select.  Here each
case
  * asserts the template instance that ran (unet_last_kernel_tag), so a change
    of the dispatch tree shows up as a failure, not as silent loss of coverage;
  * checks the output elementwise, |err| <= 1e-2 * max|ref| + 1e-2 * |ref|
    (close() of test_kernels_gpu.py);
  * checks the fused sums with the bars of test_conv_fl_gpu.py: BN-backward
    sums of the STORED bf16 dZ in fp64, rtol 1e-4 and atol 1e-5 * (largest
    per-channel sum |dZ|) [* max|xhat|]; forward BN sums rtol 1e-3 / 2e-3.
Shapes are the smallest that select the instance: K-loop kernels get C >= 128
(both LDS stages reused), persistent kernels a grid cap so a block walks >= 2
tiles, most maps are not square.  The instance selection depends on constants
in the launchers, not on the device's CU count, so no case is device specific.
A reference conv is computed once per geometry and shared by its cases.
Every case prints one line `RESULT id | tag | worst err/tol | worst sum rel`
(pytest -s); DESIGN.md holds the table measured on the MI355X."""
import ctypes
import functools
import importlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PK_CONV_FWD, PK_CONV_DGRAD, PK_CONV_FWD_CH, PK_CONV_DGRAD_CH = 0, 1, 5, 6
REP = 16  # kStatRep: BN sums are [16][2][C] replicas
SENTINEL = 768.0  # exactly representable in bf16


@pytest.fixture(scope="module")
def L(pkg):
    return importlib.import_module("image-segmentation-project_amd._lib").load()


def S():
    return torch.cuda.current_stream().cuda_stream


def bf(t):
    return t.to(torch.bfloat16)


def ratio(got, ref, rel=1e-2):
    """worst |err| / tol of close() (test_kernels_gpu.py); <= 1 passes."""
    got, ref = got.float().cpu(), ref.float().cpu()
    tol = rel * ref.abs().max().item() + rel * ref.abs()
    err = (got - ref).abs()
    bad = (err > tol).sum().item()
    assert bad == 0, (f"{bad} / {ref.numel()} elements off; max err {err.max().item():.4g} "
                      f"(ref max {ref.abs().max().item():.4g})")
    return (err / tol.clamp_min(1e-30)).max().item()


def dev(t, ld=None, fill=0.0):
    """NCHW cpu bf16 -> NHWC device tensor with channel stride ld (padding columns = fill)."""
    t = t.permute(0, 2, 3, 1)
    C = t.shape[-1]
    ld = ld or C
    out = torch.full(t.shape[:-1] + (ld,), fill, dtype=torch.bfloat16)
    out[..., :C] = t
    return out.cuda()


def pack(L, w, kind):
    """w: forward weight [Co][Ci][R][S] fp32 (cpu)."""
    Co, Ci, R, S_ = w.shape
    dst = torch.empty(w.numel(), dtype=torch.bfloat16, device="cuda")
    assert L.unet_pack_weight(w.cuda().data_ptr(), dst.data_ptr(), kind, Co, Ci, R, S_, S()) == 0, L.unet_last_error()
    return dst


class Case:
    def __init__(self, cid, mode, geom, epi, tag, R=3, stride=1, pad=1, grid_cap=0, chunk=False, ypad=0, sidepad=0,
                 csplit=0):
        self.id, self.mode, self.geom, self.tag = cid, mode, geom, tag
        self.epi = set(epi.split("+")) - {"plain"}
        self.R, self.stride, self.pad = R, stride, pad
        self.grid_cap, self.chunk, self.ypad, self.sidepad, self.csplit = grid_cap, chunk, ypad, sidepad, csplit

    def __repr__(self):
        return self.id


@functools.lru_cache(maxsize=2)
def base(mode, geom, R, stride, pad, chunk):
    """Operands and the reference conv of one geometry (op view: x [N,C,H,W] ->
    y [N,Co,P,Q]); shared by all epilogue cases of that geometry."""
    N, C, H, W, Co = geom
    g = torch.Generator().manual_seed(101 + mode)
    b = {}
    if mode == 0:
        P, Q = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
        w = torch.randn(Co, C, R, R, generator=g) / (C * R * R) ** 0.5
        x = bf(torch.randn(N, C, H, W, generator=g))
        b["conv"] = F.conv2d(x.float(), bf(w).float(), None, stride=stride, padding=pad)
        b["kind"] = PK_CONV_FWD_CH if chunk else PK_CONV_FWD
    else:  # x = dY of a forward conv w [C][Co][R][R] (forward Cout = this op's C)
        P, Q = H * stride, W * stride
        w = torch.randn(C, Co, R, R, generator=g) / (Co * R * R) ** 0.5
        x = bf(torch.randn(N, C, H, W, generator=g))
        b["conv"] = torch.nn.grad.conv2d_input((N, Co, P, Q), bf(w).float(), x.float(), stride=stride, padding=pad)
        b["kind"] = PK_CONV_DGRAD_CH if chunk else PK_CONV_DGRAD
    assert tuple(b["conv"].shape) == (N, Co, P, Q)
    b.update(x=x, w=w, P=P, Q=Q, mode=mode)
    return b


EXTRA_SEEDS = {"bias": 1, "w2": 2, "x2": 3, "add": 4, "wds": 5}


def gen(b, key):
    """A generator of its own for every lazily drawn operand: a case sees the
    same data alone (-k) as in the full run, whatever ran before it."""
    return torch.Generator().manual_seed(1000 * (1 + b["mode"]) + EXTRA_SEEDS[key])


def extra(b, key, make):
    if key not in b:
        b[key] = make()
    return b[key]


RESULTS = {}  # case id -> (tag, worst err / tol, worst relative error of the sums)
ATTEMPTED = set()  # case ids that were started (a failed case is in here and not in RESULTS)


def sums_rel(s, r):
    return ((s - r).abs().max() / r.abs().max().clamp_min(1e-30)).item()


def run_case(L, c):
    lib_mod = importlib.import_module("image-segmentation-project_amd._lib")
    ATTEMPTED.add(c.id)
    N, C, H, W, Co = c.geom
    b = base(c.mode, c.geom, c.R, c.stride, c.pad, c.chunk)
    P, Q, g = b["P"], b["Q"], torch.Generator().manual_seed(7)
    e, sp = c.epi, c.sidepad
    keep = []  # device tensors alive until the sync
    a = lib_mod.ConvExArgs(mode=c.mode, chunk_major=int(c.chunk), grid_cap=c.grid_cap, N=N, H=H, W=W, C=C, P=P, Q=Q,
                           Cout=Co, R=c.R, S=c.R, stride=c.stride, pad=c.pad)

    def put(t, ld=None):
        keep.append(t if t.is_cuda else t.cuda())
        return keep[-1]

    xp = 8 if sp else 0  # the pixel operands are staged in 16-B pieces: ld % 8 == 0
    xg = put(dev(b["x"], C + xp))
    wp = put(extra(b, "wp", lambda: pack(L, b["w"], b["kind"])))
    a.x, a.ldx, a.w = xg.data_ptr(), C + xp, wp.data_ptr()
    ref = b["conv"]
    split = "split" in e
    ny = c.csplit if split else Co
    ldy = ny + c.ypad
    y = torch.full((N, P, Q, ldy), SENTINEL, dtype=torch.bfloat16, device="cuda")
    a.y, a.ldy = y.data_ptr(), ldy
    ys = None
    if split:
        ldys = Co - c.csplit + c.ypad
        ys = torch.full((N, P, Q, ldys), SENTINEL, dtype=torch.bfloat16, device="cuda")
        a.ysplit, a.ldysplit, a.csplit = ys.data_ptr(), ldys, c.csplit
    bias = None
    if "bias" in e:
        bias = extra(b, "bias", lambda: torch.randn(Co, generator=gen(b, "bias")))
        a.bias = put(bias).data_ptr()
        ref = ref + bias.view(1, -1, 1, 1)
    if "fold" in e:
        gam, bet = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g) * 0.2
        rm, rv, eps = torch.randn(Co, generator=g) * 0.2, torch.rand(Co, generator=g) + 0.25, 1e-5
        scale = gam / torch.sqrt(rv + eps)
        shift = bet - rm * scale
        ref = ref * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        a.gamma, a.beta, a.running_mean, a.running_var = (put(t).data_ptr() for t in (gam, bet, rm, rv))
        a.eps, a.relu = eps, int("relu" in e)
    if "x2" in e:  # the block's 1x1 / stride-2 downsample data gradient, folded in (C2 == C)
        w2 = extra(b, "w2", lambda: torch.randn(C, Co, 1, 1, generator=gen(b, "w2")) / Co ** 0.5)
        x2 = extra(b, "x2", lambda: bf(torch.randn(N, C, H, W, generator=gen(b, "x2"))))
        ref = ref + extra(b, "conv2", lambda: torch.nn.grad.conv2d_input((N, Co, P, Q), bf(w2).float(), x2.float(),
                                                                         stride=2, padding=0))
        a.x2, a.ldx2, a.C2 = put(dev(x2, C + xp)).data_ptr(), C + xp, C
        a.w2 = put(extra(b, "w2p", lambda: pack(L, w2, PK_CONV_DGRAD))).data_ptr()
    if "add" in e:
        add = extra(b, "add", lambda: bf(torch.randn(N, Co, P, Q, generator=gen(b, "add"))))
        ref = ref + add.float()
        a.addend, a.ldadd = put(dev(add, Co + sp)).data_ptr(), Co + sp
    if "relu" in e:
        ref = torch.relu(ref)
    stats = stats_ds = None
    if "stats" in e:
        stats = torch.zeros(REP * 2 * Co, dtype=torch.float64, device="cuda")
        a.stats = stats.data_ptr()
    if "ds" in e:  # the block's 1x1 / stride-2 downsample forward from the same launch
        wds = extra(b, "wds", lambda: torch.randn(Co, C, 1, 1, generator=gen(b, "wds")) / C ** 0.5)
        ref_ds = extra(b, "convds", lambda: F.conv2d(b["x"].float(), bf(wds).float(), None, stride=2))
        assert tuple(ref_ds.shape) == (N, Co, P, Q)
        yds = torch.full((N, P, Q, Co + c.ypad), SENTINEL, dtype=torch.bfloat16, device="cuda")
        stats_ds = torch.zeros(REP * 2 * Co, dtype=torch.float64, device="cuda")
        a.wds = put(extra(b, "wdsp", lambda: pack(L, wds, PK_CONV_FWD))).data_ptr()
        a.yds, a.ldyds, a.stats_ds = yds.data_ptr(), Co + c.ypad, stats_ds.data_ptr()
    fused = "bb" in e or "two" in e
    if fused:
        yraw = bf(torch.randn(N, Co, P, Q, generator=g))
        act = bf(torch.relu(torch.randn(N, Co, P, Q, generator=g)))  # ~half the mask zero
        mean, invstd = torch.randn(Co, generator=g) * 0.1, torch.rand(Co, generator=g) + 0.5
        bsums = torch.zeros(REP * 2 * Co, dtype=torch.float64, device="cuda")
        a.act, a.ldact, a.yraw, a.ldyraw = put(dev(act, Co + sp)).data_ptr(), Co + sp, put(dev(yraw, Co + sp)).data_ptr(), Co + sp
        a.mean, a.invstd, a.bsums = put(mean).data_ptr(), put(invstd).data_ptr(), bsums.data_ptr()
        if "two" in e:
            yraw2 = bf(torch.randn(N, Co, P, Q, generator=g))
            mean2, invstd2 = torch.randn(Co, generator=g) * 0.1, torch.rand(Co, generator=g) + 0.5
            bsums2 = torch.zeros(REP * 2 * Co, dtype=torch.float64, device="cuda")
            a.yraw2, a.ldyraw2 = put(dev(yraw2, Co + sp)).data_ptr(), Co + sp
            a.mean2, a.invstd2, a.bsums2 = put(mean2).data_ptr(), put(invstd2).data_ptr(), bsums2.data_ptr()
        ref = ref * (act.float() > 0).float()

    rc = L.unet_conv_ex(ctypes.byref(a), S())
    assert rc == 0, L.unet_last_error().decode()
    tag = L.unet_last_kernel_tag().decode()
    torch.cuda.synchronize()
    assert tag == c.tag, f"dispatch selected {tag!r}, the case was written for {c.tag!r}"

    yc = y.cpu()
    out = yc[..., :ny].permute(0, 3, 1, 2)
    assert bool((yc[..., ny:].float() == SENTINEL).all()), "columns past the stored channels were written"
    worst, srel = 0.0, 0.0
    if split:
        ysc = ys.cpu()
        assert bool((ysc[..., Co - c.csplit:].float() == SENTINEL).all()), "ysplit padding columns were written"
        worst = max(worst, ratio(out, ref[:, :c.csplit]), ratio(ysc[..., :Co - c.csplit].permute(0, 3, 1, 2), ref[:, c.csplit:]))
    else:
        worst = ratio(out, ref)
    npix = N * P * Q

    def check_fwd_sums(st, r):  # sums of the fp32 values before the bf16 store (test_conv_fl_gpu.py:114-119)
        s = st.cpu().view(REP, 2, Co).sum(0)
        r0, r1 = r.double().sum((0, 2, 3)), r.double().pow(2).sum((0, 2, 3))
        torch.testing.assert_close(s[0], r0, rtol=1e-3, atol=1e-3 * r.abs().max().item() * npix ** 0.5)
        torch.testing.assert_close(s[1], r1, rtol=2e-3, atol=1.0)
        return max(sums_rel(s[0], r0), sums_rel(s[1], r1))

    if stats is not None:
        srel = max(srel, check_fwd_sums(stats, ref))
    if stats_ds is not None:
        ydc = yds.cpu()
        assert bool((ydc[..., Co:].float() == SENTINEL).all())
        worst = max(worst, ratio(ydc[..., :Co].permute(0, 3, 1, 2), ref_ds))
        srel = max(srel, check_fwd_sums(stats_ds, ref_ds))
    if fused:  # test_conv_fl_gpu.py:159-172: the sums are of the STORED bf16 dZ
        dz = out.double()
        assert bool((dz[act == 0] == 0).all())
        s = bsums.cpu().view(REP, 2, Co).sum(0)
        xhat = (yraw.double() - mean.double().view(1, -1, 1, 1)) * invstd.double().view(1, -1, 1, 1)
        r0, r1 = dz.sum((0, 2, 3)), (dz * xhat).sum((0, 2, 3))
        sc = dz.abs().sum((0, 2, 3)).max().item()
        torch.testing.assert_close(s[0], r0, rtol=1e-4, atol=1e-5 * sc)
        torch.testing.assert_close(s[1], r1, rtol=1e-4, atol=1e-5 * sc * xhat.abs().max().item())
        srel = max(srel, sums_rel(s[0], r0), sums_rel(s[1], r1))
        if "two" in e:
            s2 = bsums2.cpu().view(REP, 2, Co).sum(0)
            xhat2 = (yraw2.double() - mean2.double().view(1, -1, 1, 1)) * invstd2.double().view(1, -1, 1, 1)
            r2 = (dz * xhat2).sum((0, 2, 3))
            torch.testing.assert_close(s2[1], r2, rtol=1e-4, atol=1e-5 * sc * xhat2.abs().max().item())
            assert s2[0].abs().max().item() == 0.0  # only the dZ * xhat2 half is used
            srel = max(srel, sums_rel(s2[1], r2))
    RESULTS[c.id] = (tag, worst, srel)
    print(f"RESULT {c.id} | {tag} | {worst:.3f} | {srel:.2e}")


CASES = []


def add_cases(prefix, mode, geom, epis, tag, **kw):
    for epi in epis:
        k = dict(kw)
        if isinstance(epi, tuple):
            epi, more = epi
            k.update(more)
        name = f"{prefix}-{'x'.join(map(str, geom))}-{epi}" + "".join(f"-{n}{v}" for n, v in sorted(k.items())
                                                                      if n in ("grid_cap", "ypad", "sidepad"))
        CASES.append(Case(name, mode, geom, epi, tag, **k))


DG4 = ["plain", "add", "bb", "bb+add"]

# ---- stride-2 data gradient by parity class (conv3x3s2_dgrad_kernel); geometry = the dY grid ----
# <4, 2, 8>: H % 16 == 0 and N (H/16) (W/16) (Cout/64) >= 256; <4, 2, 8, true> with bb+add is enc2.0's launch
for geom, tile, sp_ in [((8, 128, 32, 128, 128), "4, 2, 8", 0), ((2, 128, 8, 32, 64), "2, 1, 8", 4),
                        ((2, 128, 12, 16, 64), "2, 1, 4", 0)]:
    for ext in (False, True):  # EXT: the folded downsample range x2 / w2
        add_cases("s2d", 1, geom, [ep + ("+x2" if ext else "") for ep in DG4],
                  f"conv3x3s2_dgrad_kernel<{tile}, {'true' if ext else 'false'}>", stride=2, sidepad=sp_)

# ---- halo-streamed (C >= 128), data gradient ----
HS_A, HS_B, HS_C = (1, 128, 16, 32, 64), (1, 128, 48, 176, 256), (1, 128, 24, 32, 64)
add_cases("hs", 1, HS_A, DG4, "conv3x3_hs_kernel<2, 16, 8, true, false, false>", sidepad=4)   # b32 <= 256
add_cases("hs", 1, HS_A, ["two", "two+add"], "conv3x3_hs_kernel<2, 16, 8, true, true, false>")
add_cases("hs", 1, HS_B, DG4, "conv3x3_hs_kernel<2, 16, 4, true, false, false>")              # b32 = 264 > 256
add_cases("hs", 1, HS_C, DG4, "conv3x3_hs_kernel<4, 8, 4, true, false, false>")               # P % 16 == 8
add_cases("hs", 1, HS_C, ["two", "two+add"], "conv3x3_hs_kernel<4, 8, 4, true, true, false>", sidepad=4)
# ---- halo-streamed, forward; MT = the persistent form (grid capped: a block walks several tiles) ----
# the eval fold y = act((conv + bias) * scale + shift [+ add]): with / without ReLU x with / without add, and
# with a bias (shift' = bias * scale + shift; the decoder convs in eval are bias+fold+relu, advanced_models.py:72-73)
FOLD4 = ["fold", "bias+fold+relu", "bias+fold+add", "fold+add+relu"]
FW3 = ["bias+stats"] + FOLD4
add_cases("hs", 0, HS_A, FW3, "conv3x3_hs_kernel<2, 16, 8, false, false, false>")
add_cases("hs", 0, HS_A, ["bias+stats"], "conv3x3_hs_kernel<2, 16, 8, false, false, true>", grid_cap=2)
add_cases("hs", 0, HS_B, FW3, "conv3x3_hs_kernel<2, 16, 4, false, false, false>")
add_cases("hs", 0, HS_B, ["bias+fold+add", "fold+add+relu"], "conv3x3_hs_kernel<2, 16, 4, false, false, true>", grid_cap=64)
add_cases("hs", 0, HS_C, FW3, "conv3x3_hs_kernel<4, 8, 4, false, false, false>", sidepad=4)
add_cases("hs", 0, HS_C, ["bias+stats", "bias+fold+relu", "fold+add+relu"], "conv3x3_hs_kernel<4, 8, 4, false, false, true>",
          grid_cap=2)
# 528 tile x channel blocks: the launcher's own cap of 512
add_cases("hs", 0, (2, 128, 48, 176, 256), ["bias+stats"], "conv3x3_hs_kernel<2, 16, 4, false, false, true>")

# ---- weight-stationary (C <= 96): (C, Co) both directions; grid caps give 2 tiles per block ----
WS = [((64, 64), "conv3x3_ws_kernel<2, 4, 16, 8, %s>", 2), ((32, 32), None, 2), ((32, 96), None, 6),
      ((32, 64), "conv3x3_ws_kernel<1, 4, 16, 8, %s>", 2), ((96, 32), "conv3x3_ws_kernel<3, 2, 8, 8, %s>", 2)]
for (C_, Co_), tg, cap in WS:
    geom = (2, C_, 16, 32, Co_)
    if (C_, Co_) == (32, 32):
        tb, tfw = "conv3x3_ws_kernel<1, 2, 8, 8, true>", "conv3x3_ws_kernel<1, 2, 16, 4, false>"
    elif (C_, Co_) == (32, 96):
        tb, tfw = "conv3x3_ws_kernel<1, 2, 16, 4, true>", "conv3x3_ws_kernel<1, 2, 8, 8, false>"
    else:
        tb, tfw = tg % "true", tg % "false"
    if C_ == 64:  # the full-line weight-stationary kernel takes the C = 64 data gradients it covers ...
        add_cases("ws2", 1, geom, ["add"], "conv3x3_ws2_kernel<true, 2>")
        add_cases("ws2", 1, geom, ["bb"], "conv3x3_ws2_kernel<true, 12>")
        add_cases("ws2", 1, geom, ["bb+add"], "conv3x3_ws2_kernel<true, 14>", grid_cap=cap)
        # ... and refuses ld % 8 == 4 operands: conv3x3_ws_kernel<2, 4, 16, 8, true> is alive
        add_cases("ws", 1, geom, ["add", "bb", ("bb+add", dict(grid_cap=cap))], tb, ypad=4, sidepad=4)
    else:
        add_cases("ws", 1, geom, ["add", "bb", ("bb+add", dict(grid_cap=cap))], tb)
    # C = 64 with the fold lands on conv3x3_ws_kernel<2, 4, 16, 8, false> (ws2 refuses the fold)
    add_cases("ws", 0, geom, ["fold", "bias+fold+relu", ("bias+fold+add", dict(grid_cap=cap)),
                              ("fold+add+relu", dict(grid_cap=cap))], tfw)

# ---- split concat gradient: ld % 8 == 0 (16-B stores) and ld % 8 == 4 (8-B stores) ----
add_cases("split", 1, (2, 64, 16, 32, 128), ["split"], "conv3x3_ws_kernel<2, 4, 16, 8, true>", csplit=64, ypad=8)
add_cases("split", 1, (2, 64, 16, 32, 128), ["split"], "conv3x3_ws_kernel<2, 4, 16, 8, true>", csplit=64, ypad=4)
add_cases("split", 1, (1, 128, 16, 32, 128), ["split"], "conv3x3_hs_kernel<2, 16, 8, true, false, false>", csplit=64, ypad=8)
add_cases("split", 1, (1, 128, 16, 32, 128), ["split"], "conv3x3_hs_kernel<2, 16, 8, true, false, false>", csplit=32, ypad=4)

# ---- implicit-GEMM fallback: maps the halo kernels refuse (W = 24, 2 x 3) ----
GL = "conv_glds_kernel<%d, 64, 64, 64, 3, 2, 2>"
add_cases("glds", 1, (2, 128, 16, 24, 64), ["bb", "bb+add", "two"], GL % 1)
add_cases("glds", 1, (2, 128, 16, 24, 128), ["split"], GL % 1, csplit=64, ypad=4)
add_cases("glds", 1, (2, 128, 8, 12, 64), ["x2", "bb+add+x2"], GL % 1, stride=2)
add_cases("glds", 0, (4, 128, 2, 3, 64), FOLD4 + ["bias+stats"], GL % 0)

# ---- forward downsample fold (conv_glds_kernel ... +ds): y and yds = conv1x1/s2(x, wds) from one launch ----
add_cases("ds", 0, (2, 64, 32, 48, 128), ["bias+stats+ds"], "conv_glds_kernel<0, 64, 64, 64, 3, 2, 2> +ds", stride=2)
add_cases("ds", 0, (1, 128, 256, 240, 256), ["stats+ds"], "conv_glds_kernel<0, 128, 128, 64, 3, 2, 4> +ds", stride=2)
# C = 256: the configuration's LDS is exactly 160 KB (3 stages + the 4-chunk downsample tile)
add_cases("ds", 0, (1, 256, 256, 240, 256), ["stats+ds"], "conv_glds_kernel<0, 128, 128, 64, 3, 2, 4> +ds", stride=2)

# ---- 1 x 1 weight-stationary GEMM: the {32, 64}^2 table ----
for C_, Co_ in [(32, 32), (64, 32), (32, 64), (64, 64)]:
    tg = f"conv1x1_kernel<{Co_ // 16}, {C_ // 32}>"
    add_cases("c1", 0, (2, C_, 16, 24, Co_), ["bias+stats"], tg, R=1, pad=0, grid_cap=2 if C_ == 64 else 0)
    add_cases("c1", 1, (2, C_, 16, 24, Co_), ["add"], tg, R=1, pad=0, grid_cap=0 if C_ == 64 else 2)

# ---- full-line kernel, forward with the eval fold (chunk-major pack; EP_RT = 32: run-time flags) ----
for geom, cap in [((2, 256, 32, 32, 256), 0), ((2, 256, 32, 32, 256), 8), ((1, 128, 32, 48, 128), 2)]:
    add_cases("fl", 0, geom, FOLD4 + ["fold+relu"], "conv3x3_fl_kernel<false, false, 32>", chunk=True,
              grid_cap=cap)

assert len({c.id for c in CASES}) == len(CASES)

# every template instance the cases above select: the instances of the conv
# dispatch tree that are reachable through unet_conv_ex (the 64-channel 16-row
# halo-streamed instance conv3x3_hs_kernel<4, 16, 8, ...> could not be selected
# by any shape and was removed from launch_halo_shape)
EXPECTED_TAGS = sorted([
    "conv3x3s2_dgrad_kernel<4, 2, 8, false>", "conv3x3s2_dgrad_kernel<4, 2, 8, true>",
    "conv3x3s2_dgrad_kernel<2, 1, 8, false>", "conv3x3s2_dgrad_kernel<2, 1, 8, true>",
    "conv3x3s2_dgrad_kernel<2, 1, 4, false>", "conv3x3s2_dgrad_kernel<2, 1, 4, true>",
    "conv3x3_hs_kernel<2, 16, 8, true, false, false>", "conv3x3_hs_kernel<2, 16, 4, true, false, false>",
    "conv3x3_hs_kernel<4, 8, 4, true, false, false>",
    "conv3x3_hs_kernel<2, 16, 8, true, true, false>", "conv3x3_hs_kernel<4, 8, 4, true, true, false>",
    "conv3x3_hs_kernel<2, 16, 8, false, false, false>", "conv3x3_hs_kernel<2, 16, 4, false, false, false>",
    "conv3x3_hs_kernel<4, 8, 4, false, false, false>",
    "conv3x3_hs_kernel<2, 16, 8, false, false, true>", "conv3x3_hs_kernel<2, 16, 4, false, false, true>",
    "conv3x3_hs_kernel<4, 8, 4, false, false, true>",
    "conv3x3_ws_kernel<2, 4, 16, 8, true>", "conv3x3_ws_kernel<2, 4, 16, 8, false>",
    "conv3x3_ws_kernel<1, 2, 8, 8, true>", "conv3x3_ws_kernel<1, 2, 8, 8, false>",
    "conv3x3_ws_kernel<1, 2, 16, 4, true>", "conv3x3_ws_kernel<1, 2, 16, 4, false>",
    "conv3x3_ws_kernel<1, 4, 16, 8, true>", "conv3x3_ws_kernel<1, 4, 16, 8, false>",
    "conv3x3_ws_kernel<3, 2, 8, 8, true>", "conv3x3_ws_kernel<3, 2, 8, 8, false>",
    "conv3x3_ws2_kernel<true, 2>", "conv3x3_ws2_kernel<true, 12>", "conv3x3_ws2_kernel<true, 14>",
    "conv_glds_kernel<1, 64, 64, 64, 3, 2, 2>", "conv_glds_kernel<0, 64, 64, 64, 3, 2, 2>",
    "conv_glds_kernel<0, 64, 64, 64, 3, 2, 2> +ds", "conv_glds_kernel<0, 128, 128, 64, 3, 2, 4> +ds",
    "conv1x1_kernel<2, 1>", "conv1x1_kernel<2, 2>", "conv1x1_kernel<4, 1>", "conv1x1_kernel<4, 2>",
    "conv3x3_fl_kernel<false, false, 32>",
])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_conv_epilogue(L, case, cuda):
    run_case(L, case)


@pytest.mark.parametrize("geom,caps", [(HS_C, (0, 2, 3)), ((2, 32, 16, 32, 64), (0, 1, 2)), ((2, 96, 16, 32, 32), (0, 3))],
                         ids=["hs", "ws-32-64", "ws-96-32"])
def test_grid_cap_is_bit_identical(L, geom, caps, cuda):
    """The grid cap of the halo kernels' forward (launch_hs / launch_ws) only
    changes which block walks which tile: every tile is computed in the same
    MFMA order, so the outputs are bit-identical whatever the cap (0 = the
    production grid, which the cap must leave untouched)."""
    lib_mod = importlib.import_module("image-segmentation-project_amd._lib")
    N, C, H, W, Co = geom
    b = base(0, geom, 3, 1, 1, False)
    x, wp = dev(b["x"]), pack(L, b["w"], PK_CONV_FWD)
    bias = torch.randn(Co, generator=torch.Generator().manual_seed(5)).cuda()
    outs = []
    for cap in caps:
        y = torch.empty(N, H, W, Co, dtype=torch.bfloat16, device="cuda")
        a = lib_mod.ConvExArgs(mode=0, grid_cap=cap, N=N, H=H, W=W, C=C, P=H, Q=W, Cout=Co, R=3, S=3, stride=1, pad=1,
                               x=x.data_ptr(), ldx=C, w=wp.data_ptr(), y=y.data_ptr(), ldy=Co, bias=bias.data_ptr())
        assert L.unet_conv_ex(ctypes.byref(a), S()) == 0, L.unet_last_error().decode()
        outs.append(y)
    torch.cuda.synchronize()
    ratio(outs[0].permute(0, 3, 1, 2), b["conv"] + bias.cpu().view(1, -1, 1, 1))
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


def test_refused_combinations_write_nothing(L, cuda):
    """Combinations no launcher implements return non-zero with a message, name
    no kernel and leave the output untouched."""
    lib_mod = importlib.import_module("image-segmentation-project_amd._lib")
    N, C, H, W, Co = 1, 128, 16, 32, 64
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")
    f = lambda n: torch.ones(n, device="cuda")
    x, w, side = z(N, H, W, C), z(Co * 9 * C), z(N, H, W, Co)
    d = torch.zeros(REP * 2 * Co, dtype=torch.float64, device="cuda")
    v = f(Co)
    common = dict(N=N, H=H, W=W, C=C, P=H, Q=W, Cout=Co, R=3, S=3, stride=1, pad=1, x=x.data_ptr(), ldx=C,
                  w=w.data_ptr(), ldy=Co)
    bb = dict(act=side.data_ptr(), ldact=Co, yraw=side.data_ptr(), ldyraw=Co, mean=v.data_ptr(), invstd=v.data_ptr(),
              bsums=d.data_ptr())
    fold = dict(gamma=v.data_ptr(), beta=v.data_ptr(), running_mean=v.data_ptr(), running_var=v.data_ptr(), eps=1e-5)
    split = dict(ysplit=side.data_ptr(), ldysplit=Co, csplit=32)
    add = dict(addend=side.data_ptr(), ldadd=Co)
    refused = {
        "bb in a forward": dict(mode=0, **bb),
        "fold in a data gradient": dict(mode=1, **fold),
        "ysplit with an addend": dict(mode=1, **split, **add),
        "ysplit with the fused BN backward": dict(mode=1, **split, **bb),
        "fold with BN sums": dict(mode=0, stats=d.data_ptr(), **fold),
        "relu without the fold": dict(mode=0, relu=1),
        "half a fused BN backward": dict(mode=1, bsums=d.data_ptr()),
        "two-BN form without its sums": dict(mode=1, yraw2=side.data_ptr(), ldyraw2=Co, **bb),
        "x2 on a stride-1 data gradient": dict(mode=1, x2=x.data_ptr(), ldx2=C, w2=w.data_ptr(), C2=C),
        "wds on a stride-1 forward": dict(mode=0, wds=w.data_ptr(), yds=side.data_ptr(), ldyds=Co),
        "chunk-major pack of an uncovered map": dict(mode=0, chunk_major=1, **{**common, "W": 24, "Q": 24}),
        "bad mode": dict(mode=2),
    }
    for what, kw in refused.items():
        y = torch.full((N, H, W, Co), SENTINEL, dtype=torch.bfloat16, device="cuda")
        a = lib_mod.ConvExArgs(**{**common, **kw})
        a.y = y.data_ptr()
        rc = L.unet_conv_ex(ctypes.byref(a), S())
        torch.cuda.synchronize()
        assert rc != 0, what
        assert L.unet_last_error().decode().startswith("unet_conv_ex: "), what
        assert L.unet_last_kernel_tag() == b"", what
        assert bool((y.float() == SENTINEL).all()) and side.abs().sum().item() == 0 and d.abs().sum().item() == 0, what
    a = lib_mod.ConvExArgs(**common)
    a.size -= 8  # a caller built against another layout
    assert L.unet_conv_ex(ctypes.byref(a), S()) != 0


def test_every_dispatch_instance_was_selected(L, cuda):
    """The union of the tags the cases selected is exactly EXPECTED_TAGS: an
    instance dropping out of the dispatch (or a new one appearing) fails here."""
    failed = sorted(ATTEMPTED - set(RESULTS))
    assert not failed, f"cases that failed earlier in this session (not launched again): {failed}"
    for c in CASES:  # a partial run (-k): launch what was not selected
        if c.id not in ATTEMPTED:
            run_case(L, c)
    assert sorted({t for t, _, _ in RESULTS.values()}) == EXPECTED_TAGS
