"""Softmax cross-entropy / multi-class Dice sums, loss, gradient and the argmax
confusion matrix (csrc/softmax_loss.hip) as single ops, through the C ABI and
through the modules, against an fp64 CPU restatement: ``F.cross_entropy`` in
float64 and the Dice formula on a float64 softmax.

Shapes are the smallest that reach every path: 2 x K x 7 x 9 (HW % 4 != 0:
scalar loads and the per-pixel tail of the gradient and confusion kernels),
3 x K x 64 x 64 (their float4 path, several blocks per image), the same from
a base pointer offset by one float (scalar fallback), and 2 x 2 x 1024 x 1024,
where every thread walks at least two grid strides: the gradient and
confusion kernels over four-pixel groups, the sums kernel over pixels.

Bars.  K = 2 is the BCE sums in another form, so test_loss_gpu.py's bars hold:
every sum within 1e-6 relative of fp64, the per-element term within 2e-6 (kept
for every K: test_nll_term_per_margin).  For K > 2 the bar of a sum is
max(1e-6, 4 x the relative error of torch's own fp32 CPU result on the same
inputs), computed here (the factor covers v_exp_f32 / v_log_f32 at ~1 ulp
against libm and up to 15 summed exponentials).  Loss value: 1e-5 relative +
1e-6 (test_loss_kernels_match_fixture).  Gradients: fp64 autograd, rtol 1e-4,
atol 1e-9.

Worst observed on the MI355X (profiles/softmax_loss.md): sums 8.8e-8 relative
(K = 2) and 8.1e-8 (K > 2), per-element term 1.7e-7, loss 9.6e-8 relative
(5.2e-7 absolute on Dice values of ~1e-6), gradient 9.5e-6 relative."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTYPES = {"u8": torch.uint8, "i32": torch.int32, "i64": torch.int64}
WORST = {}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module")
def lib_mod(pkg):
    return importlib.import_module("image-segmentation-project_amd._lib")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst observed errors:", {k: f"{v:.3e}" for k, v in sorted(WORST.items())})


# ---------------------------------------------------------------- C ABI wrappers
def _forward(lib_mod, x, y, w=None, ign=-100, kind=2, alpha=0.5, smooth=1.0):
    """x: device fp32 [N,K,H,W] (any 4-B aligned view), y: device labels [N,H,W]."""
    L = lib_mod.load()
    n, k, h, wd = x.shape
    sums, scratch = lib_mod.softmax_buffers(x.device)
    out = torch.empty((), dtype=torch.float32, device=x.device)
    rc = L.unet_softmax_loss_forward(x.data_ptr(), y.data_ptr(), lib_mod.LABEL_DTYPES[y.dtype], n, k, h * wd,
                                     lib_mod.ptr(w), ign, kind, alpha, smooth, sums.data_ptr(), scratch.data_ptr(),
                                     scratch.numel(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.unet_last_error()
    return sums, out


def _backward(lib_mod, x, y, sums, w=None, ign=-100, kind=2, alpha=0.5, smooth=1.0, gscale=None, out=None):
    L = lib_mod.load()
    n, k, h, wd = x.shape
    dl = torch.full_like(x, float("nan")) if out is None else out  # NaN: an unwritten element shows
    rc = L.unet_softmax_loss_backward(x.data_ptr(), y.data_ptr(), lib_mod.LABEL_DTYPES[y.dtype], n, k, h * wd,
                                      lib_mod.ptr(w), ign, kind, alpha, smooth, sums.data_ptr(), lib_mod.ptr(gscale),
                                      dl.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.unet_last_error()
    return dl


def _confusion(lib_mod, x, y, ign=-100):
    L = lib_mod.load()
    n, k, h, wd = x.shape
    _, scratch = lib_mod.softmax_buffers(x.device)
    cm = torch.full((k, k), -1, dtype=torch.int64, device=x.device)
    rc = L.unet_confusion_matrix(x.data_ptr(), y.data_ptr(), lib_mod.LABEL_DTYPES[y.dtype], n, k, h * wd, ign,
                                 cm.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.unet_last_error()
    return cm


# ---------------------------------------------------------------- references
def _valid(y, k, ign):
    y = y.long()
    return (y >= 0) & (y < k) & (y != ign)


def _ref(x, y, w, ign, dtype=torch.float64, smooth=1.0, alpha=0.5, grad=False):
    """The definitions in ``dtype`` on the CPU: (sums [52] in the library's
    layout, {kind: loss}, {kind: dL/dlogits} when grad)."""
    x, y = x.detach().cpu(), y.detach().cpu().long()
    k = x.shape[1]
    valid = _valid(y, k, ign)
    yy = torch.where(valid, y, torch.full_like(y, -100))
    z = x.to(dtype).requires_grad_(grad)
    wt = None if w is None else w.detach().cpu().to(dtype)
    ce_num = F.cross_entropy(z, yy, weight=wt, ignore_index=-100, reduction="sum")
    vf = valid.to(dtype)
    yc = y.clamp(0, k - 1)
    w_den = (vf if wt is None else wt[yc] * vf).sum()
    p = torch.softmax(z, 1)
    oh = F.one_hot(yc, k).permute(0, 3, 1, 2).to(dtype) * vf[:, None]
    I, P, Y = (p * oh).sum((0, 2, 3)), (p * vf[:, None]).sum((0, 2, 3)), oh.sum((0, 2, 3))
    if valid.any():
        ce = F.cross_entropy(z, yy, weight=wt, ignore_index=-100, reduction="mean")
    else:
        ce = ce_num * 0  # the one deviation from torch (NaN): no valid pixel -> 0
    dice = 1 - ((2 * I + smooth) / (P + Y + smooth)).mean()
    losses = {0: ce, 1: dice, 2: alpha * ce + (1 - alpha) * dice}
    s = torch.zeros(52, dtype=torch.float64)
    s[0], s[1], s[2] = ce_num.item(), w_den.item(), valid.sum().item()
    s[3] = ((~valid) & (y != ign)).sum().item()
    s[4:4 + k], s[20:20 + k], s[36:36 + k] = I.detach().double(), P.detach().double(), Y.detach().double()
    grads = {}
    if grad:
        for kind, lv in losses.items():
            grads[kind] = torch.autograd.grad(lv, z, retain_graph=True)[0]
    return s, {kd: v.item() for kd, v in losses.items()}, grads


def _rel(a, b):
    a, b = a.double(), b.double()
    return torch.where(b == 0, (a != 0).double(), (a - b).abs() / b.abs().clamp_min(1e-300))


def _sum_bars(x, y, w, ign, s64):
    """[52] relative bars: 1e-6 for K = 2; max(1e-6, 4 x torch's fp32 error) above."""
    bars = torch.full((52,), 1e-6, dtype=torch.float64)
    if x.shape[1] > 2:
        s32, _, _ = _ref(x, y, w, ign, dtype=torch.float32)
        bars = torch.maximum(bars, 4 * _rel(s32, s64))
    return bars


def _check_all(lib_mod, name, x, y, w, ign, kinds=(0, 1, 2)):
    """Sums, loss value and gradient of every kind, and determinism."""
    k = x.shape[1]
    xd, yd = x.cuda(), y.cuda()
    refs = {}
    for kind in kinds:
        wk = None if kind == 1 else w  # class weights belong to the CE term
        key = wk is not None
        if key not in refs:
            s64, loss64, g64 = _ref(x, y, wk, ign, grad=True)
            refs[key] = (s64, loss64, g64, _sum_bars(x, y, wk, ign, s64))
        s64, loss64, g64, bars = refs[key]
        wdev = None if wk is None else wk.cuda()
        sums, out = _forward(lib_mod, xd, yd, wdev, ign, kind)
        dl = _backward(lib_mod, xd, yd, sums, wdev, ign, kind)
        sums2, out2 = _forward(lib_mod, xd, yd, wdev, ign, kind)
        dl2 = _backward(lib_mod, xd, yd, sums2, wdev, ign, kind)
        torch.cuda.synchronize()
        assert torch.equal(sums, sums2) and torch.equal(out, out2) and torch.equal(dl, dl2), (name, kind)
        s = sums.cpu()
        rel = _rel(s, s64)
        _note("sums K=2" if k == 2 else "sums K>2", rel.max())
        bad = [(i, s[i].item(), s64[i].item(), rel[i].item(), bars[i].item()) for i in range(52)
               if not rel[i] <= bars[i]]
        assert not bad, (name, kind, bad)
        assert s[2] == s64[2] and s[3] == s64[3] and torch.equal(s[36:], s64[36:])  # counts are exact
        want, gref = loss64[kind], g64[kind]
        err = abs(out.item() - want)
        _note("loss, absolute", err)
        if abs(want) >= 1e-2:  # below, 1 - ratio of the Dice term cancels and the absolute part of the bar decides
            _note("loss, relative (|loss| >= 1e-2)", err / abs(want))
        print(f"{name} kind {kind}: loss {out.item():.9g} vs {want:.9g}, worst sum rel {rel.max():.2e}")
        assert err <= 1e-5 * abs(want) + 1e-6, (name, kind, out.item(), want)
        g = dl.cpu().double()
        assert torch.isfinite(g).all(), (name, kind)
        gerr = ((g - gref).abs() - 1e-9).clamp_min(0) / gref.abs().clamp_min(1e-300)
        _note("grad excess over atol, relative", gerr.max())
        big = gref.abs() >= 1e-7
        if big.any():
            _note("grad relative (|g| >= 1e-7)", ((g - gref).abs() / gref.abs().clamp_min(1e-300))[big].max())
        torch.testing.assert_close(g, gref, rtol=1e-4, atol=1e-9, msg=lambda m: f"{name} kind {kind}: {m}")
        inval = ~_valid(y, k, ign)
        assert torch.count_nonzero(g.permute(0, 2, 3, 1)[inval]) == 0  # exact zeros on ignored pixels


# ---------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _random_case(n, k, h, w, dtype, seed, ign=255, p_ignore=0.1, n_bad=0, weights=False):
    g = _gen(seed)
    x = (torch.rand(n, k, h, w, generator=g) * 10 - 5).float()
    y = torch.randint(0, k, (n, h, w), generator=g)
    if p_ignore:
        y[torch.rand(n, h, w, generator=g) < p_ignore] = ign
    flat = y.view(-1)
    for i in range(n_bad):  # a few labels equal to K and to 200: ignored, and counted
        flat[(7 + 13 * i) % flat.numel()] = k if i % 2 == 0 else 200
    wt = (0.5 + 1.5 * torch.rand(k, generator=g)).float() if weights else None
    return x, y.to(dtype), wt


def _confident_case(n, k, h, w, lo, hi, seed, mode="mixed"):
    """The winning channel leads the runner-up by a margin in [lo, hi]; the label
    is the winner (right), another class (wrong) or either (mixed)."""
    g = _gen(seed)
    x = (torch.rand(n, k, h, w, generator=g) * 2 - 1).float()
    win = torch.randint(0, k, (n, h, w), generator=g)
    margin = lo + (hi - lo) * torch.rand(n, h, w, generator=g)
    x.scatter_(1, win[:, None], (x.max(1).values + margin)[:, None].float())
    other = (win + torch.randint(1, k, (n, h, w), generator=g)) % k
    if mode == "right":
        y = win
    elif mode == "wrong":
        y = other
    else:
        y = torch.where(torch.rand(n, h, w, generator=g) < 0.5, win, other)
    return x, y


# ---------------------------------------------------------------- sums / loss / gradient
@pytest.mark.parametrize("k,dt,weights", [(2, "u8", False), (3, "i32", True), (5, "i64", False), (16, "u8", True)])
def test_scalar_tail_7x9(lib_mod, cuda, k, dt, weights):
    x, y, w = _random_case(2, k, 7, 9, DTYPES[dt], seed=k, n_bad=4, weights=weights)
    assert (y == 255).any() and (y.long() == k).any() and (y == 200).any()
    s = _forward(lib_mod, x.cuda(), y.cuda(), None, 255)[0].cpu()
    assert s[3] == 4  # the invalid-label slot
    _check_all(lib_mod, f"7x9 K={k} {dt}", x, y, w, 255)


@pytest.mark.parametrize("k,dt,weights", [(2, "i64", True), (3, "u8", False), (5, "i32", True), (16, "i64", False)])
def test_vector_path_64x64(lib_mod, cuda, k, dt, weights):
    x, y, w = _random_case(3, k, 64, 64, DTYPES[dt], seed=10 + k, n_bad=6, weights=weights)
    frac = (y == 255).float().mean().item()
    assert 0.07 < frac < 0.13
    _check_all(lib_mod, f"64x64 K={k} {dt}", x, y, w, 255)


@pytest.mark.parametrize("dt", ["i32", "i64"])
def test_negative_ignore_index(lib_mod, cuda, dt):
    """torch's default -100 (no uint8 label can hold it)."""
    x, y, w = _random_case(2, 3, 7, 9, DTYPES[dt], seed=3, ign=-100, weights=True)
    assert (y == -100).any()
    _check_all(lib_mod, f"ign -100 {dt}", x, y, w, -100)


@pytest.mark.parametrize("lo,hi", [(5.0, 20.0), (12.0, 16.0)])
@pytest.mark.parametrize("mode", ["right", "wrong", "mixed"])
@pytest.mark.parametrize("k", [2, 3, 16])
def test_confident_logits(lib_mod, cuda, k, lo, hi, mode):
    """exp(-margin) in [2e-9, 7e-3]: the summed terms range from ~1e-9
    (confident and right) to ~20 (confident and wrong)."""
    x, y = _confident_case(3, k, 64, 64, lo, hi, seed=100 + k, mode=mode)
    _check_all(lib_mod, f"confident K={k} [{lo},{hi}] {mode}", x, y.to(torch.uint8), None, 255)


@pytest.mark.parametrize("k", [2, 3, 5, 16])
@pytest.mark.parametrize("margin", [5.0, 10.0, 15.0, 20.0])
def test_nll_term_per_margin(lib_mod, cuda, k, margin):
    """A constant tensor per margin, label right and label wrong: the sum is
    n * nll of identical terms, so the per-element value is checked, to 2e-6
    relative for every K.  (For K > 2 torch's own fp32 result is no yardstick
    here: it loses the confident-and-right terms, 4 x its error is up to 4.  The
    term is K - 1 exponentials of <= 2 ulp each, their sum of positive terms,
    <= (K - 1) * 2^-24, and the ~3 ulp log1p correction: below 2e-6 in all.)"""
    n, h, w = 2, 7, 9
    x = torch.zeros(n, k, h, w)
    x[:, k - 1] = margin
    for lab in (k - 1, 0):
        y = torch.full((n, h, w), lab, dtype=torch.int32)
        s = _forward(lib_mod, x.cuda(), y.cuda(), None, -100, 0)[0].cpu()
        r64 = _ref(x, y, None, -100)[0]
        bar = 2e-6
        rel = _rel(s, r64)[0].item()
        _note("per-element nll", rel)
        print(f"K={k} margin {margin} label {lab}: nll {s[0].item() / (n * h * w):.9g} rel {rel:.2e} (bar {bar:.1e})")
        assert rel <= bar, (k, margin, lab, s[0].item(), r64[0].item(), rel)


@pytest.mark.parametrize("k", [2, 5])
def test_shift_by_100_changes_nothing(lib_mod, cuda, k):
    """Logits that are multiples of 1/8 shifted by +100 (exact in fp32): sums,
    loss and gradients equal the unshifted ones bit for bit, where a naive
    exp(z) overflows."""
    g = _gen(5)
    x = torch.randint(-40, 41, (3, k, 64, 64), generator=g).float() / 8
    y = torch.randint(0, k, (3, 64, 64), generator=g).to(torch.uint8)
    xs = x + 100
    assert torch.equal((xs.double() - 100), x.double()) and not torch.isfinite(torch.exp(xs)).any()
    a = _forward(lib_mod, x.cuda(), y.cuda())
    b = _forward(lib_mod, xs.cuda(), y.cuda())
    ga = _backward(lib_mod, x.cuda(), y.cuda(), a[0])
    gb = _backward(lib_mod, xs.cuda(), y.cuda(), b[0])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(ga, gb)
    assert torch.isfinite(b[0]).all() and torch.isfinite(gb).all()
    _check_all(lib_mod, f"shifted K={k}", xs, y, None, 255, kinds=(2,))


@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (3, 4, 64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_minus_infinity_masks_a_class(lib_mod, cuda, shape):
    """A channel at -inf on a third of the pixels (a masked-out class, never the
    label there): probability and gradient exactly 0, everything else finite."""
    n, k, h, w = shape
    x, y, wt = _random_case(n, k, h, w, torch.uint8, seed=60 + k, weights=True)
    off = torch.rand(n, h, w, generator=_gen(61)) < 0.33
    x[:, k - 1][off] = float("-inf")
    y[off & (y == k - 1)] = 0
    assert off.sum() > 10 and torch.isinf(x).any()
    _check_all(lib_mod, f"-inf channel K={k}", x, y, wt, 255)
    sums, _ = _forward(lib_mod, x.cuda(), y.cuda(), None, 255)
    dl = _backward(lib_mod, x.cuda(), y.cuda(), sums, None, 255).cpu()
    assert torch.count_nonzero(dl[:, k - 1][off]) == 0 and torch.isfinite(dl).all()


def test_whole_image_ignored(lib_mod, cuda):
    x, y, w = _random_case(3, 3, 64, 64, torch.uint8, seed=8, p_ignore=0.0, weights=True)
    y[1] = 255
    _check_all(lib_mod, "image 1 ignored", x, y, w, 255)


@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (3, 5, 64, 64)])
def test_every_pixel_ignored(lib_mod, pkg, cuda, shape):
    """No valid pixel: CE is exactly 0 (torch: NaN), every gradient exactly 0."""
    n, k, h, w = shape
    x = (torch.rand(shape, generator=_gen(1)) * 10 - 5).cuda()
    y = torch.full((n, h, w), 255, dtype=torch.uint8).cuda()
    y.view(-1)[3] = 200  # not the ignore value, still outside [0, K)
    for kind in (0, 1, 2):
        sums, out = _forward(lib_mod, x, y, None, 255, kind)
        dl = _backward(lib_mod, x, y, sums, None, 255, kind)
        assert out.item() == 0.0, kind  # Dice of empty sums: 1 - mean(smooth / smooth)
        assert torch.count_nonzero(dl) == 0 and torch.isfinite(dl).all()
        s = sums.cpu()
        assert s[3] == 1 and torch.count_nonzero(s[:3]) == 0 and torch.count_nonzero(s[4:]) == 0
    xr = x.clone().requires_grad_(True)
    loss = pkg.CrossEntropyLoss(ignore_index=255)(xr, y)
    loss.backward()
    assert loss.item() == 0.0 and torch.count_nonzero(xr.grad) == 0


@pytest.mark.parametrize("k,dt", [(2, "u8"), (5, "i32"), (16, "i64")])
def test_unaligned_base_gives_the_same_result(lib_mod, cuda, k, dt):
    """Logits (and dlogits) starting one float into a larger buffer: the scalar
    fallback hands every thread the same pixels in the same order, so sums,
    loss, gradient and confusion matrix equal the aligned call's bit for bit."""
    x, y, w = _random_case(3, k, 64, 64, DTYPES[dt], seed=20 + k, n_bad=2, weights=True)
    xd, yd, wd = x.cuda(), y.cuda(), w.cuda()
    big = torch.zeros(x.numel() + 5, device="cuda")
    xu = big[1:1 + x.numel()].view_as(xd)
    xu.copy_(xd)
    assert xd.data_ptr() % 16 == 0 and xu.data_ptr() % 16 == 4
    sa, la = _forward(lib_mod, xd, yd, wd, 255)
    su, lu = _forward(lib_mod, xu, yd, wd, 255)
    assert torch.equal(sa, su) and torch.equal(la, lu)
    ga = _backward(lib_mod, xd, yd, sa, wd, 255)
    gbig = torch.full((x.numel() + 5,), float("nan"), device="cuda")
    gu = _backward(lib_mod, xu, yd, su, wd, 255, out=gbig[1:1 + x.numel()].view_as(xd))
    assert torch.equal(ga, gu)
    assert torch.isnan(gbig[0]) and torch.isnan(gbig[1 + x.numel():]).all()  # nothing outside the view is written
    assert torch.equal(_confusion(lib_mod, xd, yd, 255), _confusion(lib_mod, xu, yd, 255))
    _check_all(lib_mod, f"unaligned K={k}", x, y, w, 255, kinds=(2,))


def test_two_grid_strides_1024(lib_mod, cuda):
    """2 x 2 x 1024 x 1024: 2 * MAX_BLOCKS * THREADS four-pixel groups, so every
    thread of even the largest grid the launcher may use walks two strides."""
    n, k, h, w = 2, 2, 1024, 1024
    groups = n * h * w // 4
    assert groups >= 2 * lib_mod.SOFTMAX_MAX_BLOCKS * lib_mod.SOFTMAX_THREADS
    g = _gen(9)
    x = (torch.rand(n, k, h, w, generator=g) * 10 - 5).float()
    y = torch.randint(0, k, (n, h, w), generator=g, dtype=torch.int64).to(torch.uint8)
    y[torch.rand(n, h, w, generator=g) < 0.1] = 255
    _check_all(lib_mod, "1024x1024 K=2", x, y, None, 255, kinds=(2,))
    cm = _confusion(lib_mod, x.cuda(), y.cuda(), 255).cpu().numpy()
    assert np.array_equal(cm, _np_confusion(x, y, 255))


def test_grad_scale_and_modules(lib_mod, pkg, cuda):
    """The modules (one autograd.Function) against the same references, through
    autograd with a non-unit upstream gradient; [N,1,H,W] labels are accepted."""
    x, y, w = _random_case(2, 3, 7, 9, torch.int64, seed=30, ign=-100, weights=True)
    _, loss64, g64 = _ref(x, y, w, -100, alpha=0.3, smooth=2.0, grad=True)
    _, lossd, gd = _ref(x, y, None, -100, smooth=2.0, grad=True)
    crits = {0: pkg.CrossEntropyLoss(weight=w), 1: pkg.SoftmaxDiceLoss(smooth=2.0),
             2: pkg.SoftmaxComboLoss(alpha=0.3, smooth=2.0, weight=w.tolist())}
    for kind, crit in crits.items():
        want, gref = (lossd[1], gd[1]) if kind == 1 else (loss64[kind], g64[kind])
        for lab in (y.cuda(), y[:, None].cuda()):
            xr = x.cuda().requires_grad_(True)
            loss = crit(xr, lab)
            (2.5 * loss).backward()
            assert abs(loss.item() - want) <= 1e-5 * abs(want) + 1e-6, (kind, loss.item(), want)
            torch.testing.assert_close(xr.grad.cpu().double(), 2.5 * gref, rtol=1e-4, atol=1e-9)
    assert crits[0].weight.is_cuda  # moved once, on first use
    m = pkg.calculate_multiclass_metrics(x.cuda(), y.cuda())
    want = pkg.metrics_from_confusion(_np_confusion(x, y, -100))
    assert m == want


# ---------------------------------------------------------------- confusion matrix
def _np_confusion(x, y, ign):
    x, y = x.cpu().numpy(), y.cpu().numpy().astype(np.int64)
    k = x.shape[1]
    pred = np.argmax(x, axis=1)  # first maximum
    ok = (y >= 0) & (y < k) & (y != ign)
    cm = np.zeros((k, k), dtype=np.int64)
    np.add.at(cm, (y[ok], pred[ok]), 1)
    return cm


@pytest.mark.parametrize("shape", [(2, 2, 7, 9), (2, 3, 7, 9), (2, 5, 7, 9), (2, 16, 7, 9), (3, 2, 64, 64),
                                   (3, 3, 64, 64), (3, 16, 64, 64)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", ["u8", "i32", "i64"])
def test_confusion_matrix_random(lib_mod, pkg, cuda, shape, dt):
    n, k, h, w = shape
    x, y, _ = _random_case(n, k, h, w, DTYPES[dt], seed=40 + k, n_bad=3)
    assert (y == 255).any() and (y.long() == k).any()
    want = _np_confusion(x, y, 255)
    assert want.sum() == _valid(y, k, 255).sum().item() < y.numel()
    got = _confusion(lib_mod, x.cuda(), y.cuda(), 255)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    again = pkg.confusion_matrix(x.cuda(), y.cuda(), ignore_index=255)
    assert torch.equal(got, again) and again.is_cuda


@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (3, 5, 64, 64), (3, 16, 64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_confusion_matrix_ties(lib_mod, cuda, shape):
    """Exact ties between two channels (a third of the pixels) and between all
    channels (another third): the lowest index wins, as np.argmax."""
    n, k, h, w = shape
    g = _gen(50 + k)
    x = torch.randint(-8, 9, (n, k, h, w), generator=g).float() / 4
    which = torch.randint(0, 3, (n, h, w), generator=g)
    a = torch.randint(0, k, (n, h, w), generator=g)
    b = (a + torch.randint(1, k, (n, h, w), generator=g)) % k
    top = (x.max(1).values + 1)[:, None]
    two = (which == 1)[:, None]
    x = torch.where(two & (torch.arange(k).view(1, k, 1, 1) == a[:, None]), top, x)
    x = torch.where(two & (torch.arange(k).view(1, k, 1, 1) == b[:, None]), top, x)
    x = torch.where((which == 2)[:, None], top.expand_as(x), x).contiguous()
    y = torch.randint(0, k, (n, h, w), generator=g).to(torch.uint8)
    y[torch.rand(n, h, w, generator=g) < 0.1] = 255
    # the reference inputs hold what the test claims
    nmax = (x == x.max(1, keepdim=True).values).sum(1)
    assert (nmax[which == 1] == 2).all() and (nmax[which == 2] == k).all()
    assert (which == 1).sum() > 10 and (which == 2).sum() > 10 and (y == 255).sum() > 5
    hi_first = (torch.minimum(a, b) != a)[which == 1]
    assert hi_first.any() and (~hi_first).any()  # the tie's lower index is sometimes the second one written
    got = _confusion(lib_mod, x.cuda(), y.cuda(), 255).cpu().numpy()
    assert np.array_equal(got, _np_confusion(x, y, 255))
