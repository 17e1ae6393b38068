"""The attention gate and channel attention kernels (csrc/attention.hip) one pass
at a time, through the C-ABI entries unet_att_gate_op / unet_ch_att_op, against
the oracle's AttentionGate (its psi part and x * psi) and ChannelAttention
(advanced_models.py:7-61) in fp64 on the CPU with autograd.

Both sides get the same bf16-rounded activations, fp32 parameters and upstream
gradients.  Every pass is teacher-forced: its reference starts from the GPU's
own outputs of the earlier passes (value-substituted into the autograd graph,
`forced()`), so each bound is the rounding of ONE kernel.  Where the reference
recomputes a quantity that the kernel reads from an earlier pass (the BN(1)
mean / invstd, psi, the gate, the hidden vector), the asserted bound of that
quantity is propagated into the bounds downstream of it.

Bounds (u = 2^-24, the fp32 unit roundoff), all derived, none fitted:
  * bf16 outputs (xatt, dxpsi, dS, out, dout): the kernel rounds an fp32 value
    once: |got - ref| <= 2^-8 |ref| + 2^-16 max|ref|.
  * reductions: n u S, S the fp64 sum of the absolute values of the entry's
    terms and n the length of the fp32 accumulation chain read off the kernel
    (pixels per thread + LDS rows + the roundings of one term), given next to
    each check.  For most entries n < 130 and n u S < 2^-16 S; the chains that
    are longer are the sequential dot products over C of the MLP kernels
    (n = C + ...) and the 256 LDS rows of the gate's pass 3 at F_int = 8.
    Sums that are accumulated in fp64 from fp32 terms take the sum of the
    terms' bounds.
  * fp32 elementwise outputs (psi, save, running statistics, the gate): 8 fp32
    ulp of the reference plus the propagated input error.
  * exact: pkey (maximum and FIRST argmax of every (n, c)), psum and avg | max
    (y holds small integers, every partial sum is exact), the integer variant
    of the gate's p and its BN sums, sentinels, nbt, the pixel that carries
    the dmax term.
y never holds -0.0: its producers (ReLU epilogues) store +0 only, and the
packed argmax key orders -0 below +0 where torch compares them equal.
Every case prints `RATIO <quantity> <worst err / bound>` (pytest -s); the
values measured on the MI355X are in DESIGN.md."""
import ctypes
import importlib
import math

import numpy as np
import pytest
import torch

from oracle import unet_ref

pytestmark = pytest.mark.gpu

REP = 16          # kStatRep
SENT = 768.0      # exactly representable in bf16; no checked value reaches it
FSENT = -777.25   # sentinel of fp32 outputs
U = 2.0 ** -24
BF = torch.bfloat16
WORST = {}


@pytest.fixture(scope="module")
def lib(pkg, cuda):
    m = importlib.import_module("image-segmentation-project_amd._lib")
    return m, m.load()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for k in sorted(WORST):
        print(f"WORST {k:28s} {WORST[k]:.3e}")


def S():
    return torch.cuda.current_stream().cuda_stream


def np64(t):
    return t.detach().double().cpu().numpy()


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


class Rec:
    """Collects err / bound of every checked quantity of one case; finish() asserts them all."""

    def __init__(self, prefix):
        self.prefix, self.bad = prefix, []

    def add(self, name, got, ref, bound):
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        assert np.isfinite(got).all(), name
        err = np.abs(got - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / bound)
        worst = float(r.max()) if r.size else 0.0
        print(f"RATIO {self.prefix}{name:10s} {worst:.3e}")
        key = self.prefix.split(" ")[0] + name
        WORST[key] = max(WORST.get(key, 0.0), worst)
        if not worst <= 1.0:
            i = int(np.argmax(r))
            self.bad.append(f"{name}: err/bound {worst:.3g} at flat index {i} (got {got.flat[i]!r}, ref {ref.flat[i]!r})")

    def bf16(self, name, got, ref):
        """the bf16-output rule"""
        ref = np.asarray(ref, dtype=np.float64)
        self.add(name, got, ref, 2.0 ** -8 * np.abs(ref) + 2.0 ** -16 * np.abs(ref).max())

    def exact(self, name, got, ref):
        ok = np.array_equal(np.asarray(got), np.asarray(ref))
        print(f"EXACT {self.prefix}{name:10s} {'ok' if ok else 'MISMATCH'}")
        if not ok:
            d = np.flatnonzero(np.asarray(got).ravel() != np.asarray(ref).ravel())
            self.bad.append(f"{name}: {d.size} entries differ, first at {d[:5]}: got {np.asarray(got).ravel()[d[:5]]} "
                            f"ref {np.asarray(ref).ravel()[d[:5]]}")

    def finish(self):
        assert not self.bad, "\n".join(self.bad)


class Padded:
    """bf16 device tensor [rows][w] inside a [rows][ld] buffer at column off; the rest is sentinel."""

    def __init__(self, rows, w, ld, off=0, data=None):
        self.w, self.off, self.ld = w, off, ld
        self.buf = torch.full((rows, ld), SENT, dtype=BF, device="cuda")
        self.v = self.buf[:, off:off + w]
        if data is not None:
            self.v.copy_(data.reshape(rows, w))
        self.ptr = self.v.data_ptr()

    def get(self, rec, name):
        """the slice as fp64; asserts nothing outside it changed and nothing inside kept the sentinel"""
        c = self.buf.cpu()
        inside = c[:, self.off:self.off + self.w]
        rec.exact(name + ".pad", bool((c[:, :self.off] == SENT).all() and (c[:, self.off + self.w:] == SENT).all()), True)
        rec.exact(name + ".all", bool((inside == SENT).any()), False)
        return inside.double().numpy()


def f32out(n):
    """fp32 output [n] followed by 8 guard elements"""
    return torch.full((n + 8,), FSENT, dtype=torch.float32, device="cuda")


def f32get(rec, name, t, n):
    c = t.cpu()
    rec.exact(name + ".pad", bool((c[n:] == FSENT).all()), True)
    rec.exact(name + ".all", bool((c[:n] == FSENT).any()), False)
    return c[:n].double().numpy()


def forced(ref, gpu):
    """ref's autograd graph carrying the GPU's value (teacher forcing)"""
    return ref + (gpu - ref).detach()


def dev(t, dtype=torch.float32):
    return t.to(dtype).cuda().contiguous()


# ---------------------------------------------------------------------------------------------------
# attention gate
# ---------------------------------------------------------------------------------------------------
def ppb(F):
    return 256 // (F // 8)


GATE_PAIRS = [(8, 8), (64, 32), (128, 64), (256, 128), (512, 256)]


def gate_npix(Fl, Fi):
    m = max(ppb(Fl), ppb(Fi))
    return [1, m - 1, 2 * 2048 * m + 3]


GATE_CASES = [(Fl, Fi, n, 0.4) for Fl, Fi in GATE_PAIRS for n in gate_npix(Fl, Fi)] + [(64, 32, 2 * 2048 * 8 + 3, 100.0)]


def bn_train(bn, v):
    """bn(v) in training mode; torch refuses one value per channel, where the
    batch statistics are still defined (variance 0): the same op without the check"""
    if v.numel() > 1:
        return bn(v)
    return torch.batch_norm(v, bn.weight, bn.bias, None, None, True, bn.momentum, bn.eps, False)


def run_gate(L, a, ps):
    a.pass_ = ps
    rc = L.unet_att_gate_op(ctypes.byref(a), S())
    assert rc == 0, L.unet_last_error().decode()


@pytest.mark.parametrize("Fl,Fi,npix,bias", GATE_CASES, ids=[f"Fl{c[0]}-Fi{c[1]}-npix{c[2]}-b{c[3]:g}" for c in GATE_CASES])
def test_gate_passes(lib, Fl, Fi, npix, bias):
    m, L = lib
    rec = Rec(f"gate. [{Fl},{Fi},{npix},{bias:g}] ")
    g = torch.Generator().manual_seed(7 * Fl + Fi + npix % 1000)
    Fg = max(8, Fl // 4)
    CCi, CCl = Fi // 8, Fl // 8
    M = float(npix)
    s = torch.relu(torch.randn(npix, Fi, generator=g)).to(BF)
    x = torch.randn(npix, Fl, generator=g).to(BF)
    dxatt = (torch.randn(npix, Fl, generator=g) * 0.5).to(BF)
    yraw = torch.randn(npix, Fi, generator=g).to(BF)
    yraw2 = (torch.randn(npix, Fi, generator=g) * 2 + 1).to(BF)
    psi_w = (torch.randn(Fi, generator=g) * (2.0 / Fi ** 0.5)).float()
    psi_b = torch.tensor([bias], dtype=torch.float32)
    gamma, beta = torch.tensor([1.3]), torch.tensor([-0.2])
    rm0, rv0, nbt0 = torch.tensor([0.3]), torch.tensor([1.7]), 5
    mean = torch.randn(Fi, generator=g).float() * 0.3
    invstd = (torch.rand(Fi, generator=g) * 1.5 + 0.5).float()
    mean2 = torch.randn(Fi, generator=g).float() * 0.3 + 1
    invstd2 = (torch.rand(Fi, generator=g) * 0.5 + 0.25).float()

    # ---- device side: every activation has a leading dimension larger than its width
    d_s = Padded(npix, Fi, Fi + 8, 0, s)
    d_x = Padded(npix, Fl, Fl + 16, 8, x)
    d_dxatt = Padded(npix, Fl, Fl + Fg, 0, dxatt)            # the concat gradient, skip channels first
    d_yraw, d_yraw2 = Padded(npix, Fi, Fi + 8, 8, yraw), Padded(npix, Fi, Fi + 24, 16, yraw2)
    d_w, d_b, d_gamma, d_beta = dev(psi_w), dev(psi_b), dev(gamma), dev(beta)
    d_mean, d_inv, d_mean2, d_inv2 = dev(mean), dev(invstd), dev(mean2), dev(invstd2)
    d_rm, d_rv = dev(rm0), dev(rv0)
    d_nbt = torch.tensor([nbt0], dtype=torch.int64, device="cuda")
    d_p, d_psi, d_dbnp = f32out(npix), f32out(npix), f32out(npix)
    d_pst = torch.zeros(2, dtype=torch.float64, device="cuda")
    d_pbs = torch.zeros(2, dtype=torch.float64, device="cuda")
    d_save = torch.full((2 + 8,), FSENT, dtype=torch.float32, device="cuda")
    d_xatt = Padded(npix, Fl, Fl + Fg, 0)                     # the plan's concat: skip slice first
    d_dxpsi, d_dS = Padded(npix, Fl, Fl + 8, 8), Padded(npix, Fi, Fi + 16, 8)
    d_gw, d_gg, d_gb = f32out(Fi), f32out(1), f32out(1)
    d_gacc = torch.zeros(REP * Fi, dtype=torch.float64, device="cuda")
    a = m.AttGateOpArgs(
        training=0, Fi=Fi, Fl=Fl, lds=d_s.ld, ldx=d_x.ld, ldxatt=d_xatt.ld, lddxatt=d_dxatt.ld, lddxpsi=d_dxpsi.ld,
        lddS=d_dS.ld, eps=1e-5, momentum=0.1, npix=npix, s=d_s.ptr, psi_w=d_w.data_ptr(), psi_b=d_b.data_ptr(),
        p=d_p.data_ptr(), psi=d_psi.data_ptr(), dbnp=d_dbnp.data_ptr(), pst=d_pst.data_ptr(), pbs=d_pbs.data_ptr(),
        save=d_save.data_ptr(), gamma=d_gamma.data_ptr(), beta=d_beta.data_ptr(), run_mean=d_rm.data_ptr(),
        run_var=d_rv.data_ptr(), nbt=d_nbt.data_ptr(), x=d_x.ptr, xatt=d_xatt.ptr, dxatt=d_dxatt.ptr,
        dxpsi=d_dxpsi.ptr, dS=d_dS.ptr, gpsi_w=d_gw.data_ptr(), ggamma=d_gg.data_ptr(), gbeta=d_gb.data_ptr(),
        gpsi_acc=d_gacc.data_ptr())

    # ---- the oracle's gate in fp64 (W_g / W_x are convolutions, tested elsewhere)
    gate = unet_ref.AttentionGate(Fg, Fl, Fi).double()
    conv, bn, sig = gate.psi[0], gate.psi[1], gate.psi[2]
    with torch.no_grad():
        conv.weight.copy_(psi_w.double().view(1, Fi, 1, 1))
        conv.bias.copy_(psi_b.double())
        bn.weight.copy_(gamma.double())
        bn.bias.copy_(beta.double())
        bn.running_mean.copy_(rm0.double())
        bn.running_var.copy_(rv0.double())
        bn.num_batches_tracked.fill_(nbt0)
    s_t = s.double().t().contiguous().view(1, Fi, npix, 1).requires_grad_(True)
    x_t = x.double().t().contiguous().view(1, Fl, npix, 1).requires_grad_(True)
    sn, xn, dn, wn = np64(s), np64(x), np64(dxatt), np64(psi_w)

    # ================= eval forward (running statistics; nothing else may change) =================
    run_gate(L, a, 0)
    run_gate(L, a, 1)
    p_e = f32get(rec, "p(eval)", d_p, npix)
    psi_e = f32get(rec, "psi(eval)", d_psi, npix)
    xatt_e = d_xatt.get(rec, "xatt(eval)")
    rec.exact("eval:pst", np64(d_pst), np.zeros(2))
    rec.exact("eval:save", np64(d_save), np.full(10, FSENT))
    rec.exact("eval:run", [d_rm.item(), d_rv.item(), d_nbt.item()], [rm0.item(), rv0.item(), nbt0])
    p_ref = conv(s_t).flatten()
    S_p = abs(bias) + np.abs(sn) @ np.abs(wn)
    # p: 8 products + adds per lane, log2(Fi/8) shuffle adds, the bias, one product rounding
    n_p = 10 + int(math.log2(CCi))
    rec.add("p(eval)", p_e, np64(p_ref), n_p * U * S_p)
    gate.eval()
    pe_t = torch.from_numpy(p_e)
    with torch.no_grad():
        psi_ref_e = np64(sig(bn(pe_t.view(1, 1, npix, 1))).flatten())
    inv_e = 1.0 / math.sqrt(rv0.item() + 1e-5)
    sc_e = gamma.item() * inv_e
    dz_e = 8 * U * (np.abs(p_e * sc_e) + abs(rm0.item() * sc_e) + abs(beta.item()))
    rec.add("psi(eval)", psi_e, psi_ref_e, 8 * ulp32(psi_ref_e) + psi_ref_e * (1 - psi_ref_e) * dz_e)
    rec.bf16("xatt(eval)", xatt_e, xn * psi_e[:, None])

    # ================= training forward =================
    gate.train()
    d_p.fill_(FSENT)
    d_psi.fill_(FSENT)
    d_xatt.buf.fill_(SENT)
    a.training = 1
    run_gate(L, a, 0)
    run_gate(L, a, 1)
    p_g = f32get(rec, "p", d_p, npix)
    psi_g = f32get(rec, "psi", d_psi, npix)
    xatt_g = d_xatt.get(rec, "xatt")
    save_g = d_save.cpu()
    rec.exact("save.pad", bool((save_g[2:] == FSENT).all()), True)
    save_g = save_g[:2].double().numpy()
    rec.exact("p==p(eval)", p_g, p_e)   # the same arithmetic in both modes
    rec.add("p", p_g, np64(p_ref), n_p * U * S_p)
    # pst: fp64 sums of the fp32 p: <= 8 per thread, 8 tree levels, <= 2048 atomics: n < 2^12 at 2^-53
    pst_ref = np.array([p_g.sum(), (p_g * p_g).sum()])
    rec.add("pst", np64(d_pst), pst_ref, 2.0 ** -41 * np.array([np.abs(p_g).sum(), (p_g * p_g).sum()]))
    p_used = forced(p_ref, torch.from_numpy(p_g))
    p_used.retain_grad()
    z = bn_train(bn, p_used.view(1, 1, npix, 1))
    z.retain_grad()
    psi_ref_t = sig(z).flatten()
    psi_ref = np64(psi_ref_t)
    mean_r = p_g.mean()
    var_r = float(np.var(p_g))
    inv_r = 1.0 / math.sqrt(var_r + 1e-5)
    # propagated: the kernel forms var = E[p^2] - mean^2 in fp64 (cancellation at a large mean)
    var_err = 4 * 2.0 ** -53 * ((p_g * p_g).mean() + mean_r * mean_r)
    b_mean = 8 * ulp32(mean_r) + 2.0 ** -41 * np.abs(p_g).mean()
    b_inv = 8 * ulp32(inv_r) + 0.5 * inv_r * var_err / (var_r + 1e-5)
    rec.add("save", save_g, [mean_r, inv_r], [b_mean, b_inv])
    unb = var_r * (M / (M - 1.0) if M > 1 else 1.0)
    if npix > 1:
        run_ref = np.array([bn.running_mean.item(), bn.running_var.item()])
        rec.exact("nbt(ref)", bn.num_batches_tracked.item(), nbt0 + 1)
    else:  # torch has no unbiased variance of one value; the kernel's rule there: the factor n / (n - 1) is 1
        run_ref = np.array([0.9 * rm0.double().item() + 0.1 * mean_r, 0.9 * rv0.double().item()])
    # (1 - m) r + m v in fp32; the two terms of the mean may cancel; the inputs' own bounds at weight m
    b_run = 8 * ulp32(run_ref) + 8 * U * np.array([abs(0.9 * 0.3) + abs(0.1 * mean_r), 0.0]) \
        + 0.1 * np.array([b_mean, (M / (M - 1.0) if M > 1 else 1.0) * var_err + 2 * U * unb])
    rec.add("running", [d_rm.item(), d_rv.item()], run_ref, b_run)
    rec.exact("nbt", d_nbt.item(), nbt0 + 1)
    sc_r = gamma.item() * inv_r
    dz_t = 8 * U * (np.abs(p_g * sc_r) + abs(mean_r * sc_r) + abs(beta.item()))
    b_psi = 8 * ulp32(psi_ref) + psi_ref * (1 - psi_ref) * dz_t
    rec.add("psi", psi_g, psi_ref, b_psi)
    rec.bf16("xatt", xatt_g, xn * psi_g[:, None])

    # ================= backward, pass 2 =================
    run_gate(L, a, 2)
    xatt_ref = x_t * forced(psi_ref_t, torch.from_numpy(psi_g)).view(1, 1, npix, 1)
    xatt_ref.backward(dxatt.double().t().contiguous().view(1, Fl, npix, 1))
    dxpsi_g = d_dxpsi.get(rec, "dxpsi")
    rec.bf16("dxpsi", dxpsi_g, np64(x_t.grad.view(Fl, npix).t()))
    dbnp_g = f32get(rec, "dbnp", d_dbnp, npix)
    dz_ref = np64(z.grad.flatten())
    q = psi_g * (1 - psi_g)
    S_px = (np.abs(dn) * np.abs(xn)).sum(1)
    dpsi_ref = (dn * xn).sum(1)
    # dz = dpsi ps (1 - ps): dot product as p (no bias) and three more roundings; psi's own bound propagated
    n_dz = 12 + int(math.log2(CCl))
    b_dz = n_dz * U * S_px * q + np.abs(dpsi_ref) * np.abs(1 - 2 * psi_g) * b_psi
    rec.add("dbnp", dbnp_g, dz_ref, b_dz)
    phat = (p_g - mean_r) * inv_r
    b_phat = b_mean * inv_r + np.abs(phat) * (b_inv / inv_r) + 2 * U * np.abs(phat)
    pbs_ref = np.array([bn.bias.grad.item(), bn.weight.grad.item()])
    # fp64 sums of fp32 terms: the sum of the terms' bounds (one more rounding for the product dz * phat)
    b_pbs = np.array([b_dz.sum(), (b_dz * np.abs(phat) + np.abs(dz_ref) * (b_phat + U * np.abs(phat))).sum()]) \
        + 2.0 ** -41 * np.array([np.abs(dz_ref).sum(), np.abs(dz_ref * phat).sum()])
    rec.add("pbs", np64(d_pbs), pbs_ref, b_pbs)

    # ================= backward, pass 3 (plain, then with the two-BN reduction fused) =================
    k1 = gamma.item() * inv_r
    m1, m2 = pbs_ref / M
    dp_abs = k1 * (S_px * q + abs(m1) + np.abs(phat * m2))
    b_dp = k1 * (b_dz + b_pbs[0] / M + abs(m2) * b_phat + np.abs(phat) * b_pbs[1] / M) + 8 * U * dp_abs
    dS_ref = np64(s_t.grad.view(Fi, npix).t())
    rows = 256 // CCi
    grid3 = min(1024, (npix + rows * 8 - 1) // (rows * 8))
    # weight-gradient / BN sums of pass 3: pixels per thread + the LDS rows (256 at Fi = 8) + one product
    n_red = -(-npix // (grid3 * rows)) + rows + 2
    b_gw = (b_dp[:, None] * np.abs(sn)).sum(0) + n_red * U * (dp_abs[:, None] * np.abs(sn)).sum(0)
    mask = sn > 0
    xh1 = (np64(yraw) - np64(mean)) * np64(invstd)
    xh2 = (np64(yraw2) - np64(mean2)) * np64(invstd2)
    dZ = dS_ref * mask
    e_dS = (b_dp[:, None] * np.abs(wn) + U * dp_abs[:, None] * np.abs(wn)) * mask
    m_dS = dp_abs[:, None] * np.abs(wn) * mask
    d_bs = torch.zeros(REP * 2 * Fi, dtype=torch.float64, device="cuda")
    d_bs2 = torch.zeros(REP * 2 * Fi, dtype=torch.float64, device="cuda")
    for fused in (False, True):
        tag = "+bb" if fused else ""
        d_gacc.zero_()
        d_dS.buf.fill_(SENT)
        for t in (d_gw, d_gg, d_gb):
            t.fill_(FSENT)
        if fused:
            a.yraw, a.yraw2, a.ldyraw, a.ldyraw2 = d_yraw.ptr, d_yraw2.ptr, d_yraw.ld, d_yraw2.ld
            a.mean, a.invstd, a.mean2, a.invstd2 = d_mean.data_ptr(), d_inv.data_ptr(), d_mean2.data_ptr(), d_inv2.data_ptr()
            a.bsums, a.bsums2 = d_bs.data_ptr(), d_bs2.data_ptr()
        run_gate(L, a, 3)
        rec.bf16("dS" + tag, d_dS.get(rec, "dS" + tag), dZ if fused else dS_ref)
        rec.add("gpsi_w" + tag, f32get(rec, "gpsi_w" + tag, d_gw, Fi), np64(conv.weight.grad.flatten()),
                b_gw + U * np.abs(np64(conv.weight.grad.flatten())))
        rec.add("ggamma" + tag, f32get(rec, "ggamma" + tag, d_gg, 1), pbs_ref[1:], b_pbs[1:] + ulp32(pbs_ref[1:]))
        rec.add("gbeta" + tag, f32get(rec, "gbeta" + tag, d_gb, 1), pbs_ref[:1], b_pbs[:1] + ulp32(pbs_ref[:1]))
    bs = np64(d_bs).reshape(REP, 2, Fi).sum(0)
    bs2 = np64(d_bs2).reshape(REP, 2, Fi)
    rec.exact("bsums2[0]", bs2[:, 0], np.zeros((REP, Fi)))
    bs2 = bs2.sum(0)
    rec.add("bsums[0]", bs[0], dZ.sum(0), e_dS.sum(0) + n_red * U * m_dS.sum(0))
    # xhat in fp32: a subtraction and a product, then the product with dZ
    rec.add("bsums[1]", bs[1], (dZ * xh1).sum(0), (e_dS * np.abs(xh1)).sum(0) + (n_red + 3) * U * (m_dS * np.abs(xh1)).sum(0))
    rec.add("bsums2[1]", bs2[1], (dZ * xh2).sum(0), (e_dS * np.abs(xh2)).sum(0) + (n_red + 3) * U * (m_dS * np.abs(xh2)).sum(0))
    rec.finish()


@pytest.mark.parametrize("Fl,Fi", GATE_PAIRS, ids=[f"Fl{a}-Fi{b}" for a, b in GATE_PAIRS])
def test_gate_psi_forward_exact_on_integers(lib, Fl, Fi):
    """s, psi_w in {-2..2}, integer bias: every fp32 partial sum is an integer
    below 2^24, so p and its BN sums (sum, sum of squares, fp64) are bit-exact: a
    dropped, doubled or misattributed pixel cannot hide behind a tolerance.
    One more size than test_gate_passes: 4 * 2048 * ppb(Fi) + 5 pixels give THIS
    kernel (the F_int layout, the larger ppb of every pair) its second loop
    iteration, ragged in slot 0."""
    m, L = lib
    rec = Rec(f"gateint. [{Fl},{Fi}] ")
    for npix in gate_npix(Fl, Fi) + [4 * 2048 * ppb(Fi) + 5]:
        g = torch.Generator().manual_seed(npix + Fi)
        s = torch.randint(-2, 3, (npix, Fi), generator=g)
        w = torch.randint(-2, 3, (Fi,), generator=g)
        w[0] = 1  # never all zero
        d_s = Padded(npix, Fi, Fi + 8, 8, s.to(BF))
        d_w, d_b = dev(w), dev(torch.tensor([3.0]))
        d_p = f32out(npix)
        d_pst = torch.zeros(2, dtype=torch.float64, device="cuda")
        a = m.AttGateOpArgs(training=1, Fi=Fi, Fl=Fl, lds=d_s.ld, npix=npix, s=d_s.ptr, psi_w=d_w.data_ptr(),
                            psi_b=d_b.data_ptr(), p=d_p.data_ptr(), pst=d_pst.data_ptr())
        run_gate(L, a, 0)
        p_ref = (s @ w + 3).numpy()
        rec.exact(f"p@{npix}", f32get(rec, f"p@{npix}", d_p, npix), p_ref.astype(np.float64))
        rec.exact(f"pst@{npix}", np64(d_pst), np.array([p_ref.sum(), (p_ref * p_ref).sum()], dtype=np.float64))
    rec.finish()


# ---------------------------------------------------------------------------------------------------
# channel attention
# ---------------------------------------------------------------------------------------------------
CH_PAIRS = [(32, 2), (64, 4), (128, 8), (256, 16), (512, 32), (1024, 64)]


def ch_hw(C):
    rows = 256 // (C // 8)
    return sorted({1, rows - 1, 16 * rows, 16 * rows + 1, 2 * 64 * 16 * rows + 5})   # C = 1024: rows - 1 = 1


CH_CASES = [(C, Cr, hw, N) for C, Cr in CH_PAIRS for hw in ch_hw(C) for N in (1, 3)] + [(128, 8, 16 * 16 + 1, 17)]


def make_y(N, HW, C, rows, g):
    """small non-negative integers (ties everywhere) with the tie / edge patterns
    on channels (5 n + k) % C of image n; never -0.0"""
    y = torch.randint(0, 4, (N, HW, C), generator=g).float()
    last_block = ((HW - 1) // (16 * rows)) * 16 * rows
    for n in range(N):
        ch = [(5 * n + k) % C for k in range(5)]
        y[n, :, ch[0]] = 0.0                                  # a dead channel
        y[n, :, ch[1]] = -1.5                                 # all negative, one -0.5
        y[n, HW // 2, ch[1]] = -0.5
        for c in ch[2:]:
            y[n, :, c] = torch.clamp(y[n, :, c], max=2.0)
        y[n, 0, ch[2]] = 3.0                                  # the maximum at pixel 0 and again in the last block
        y[n, HW - 1, ch[2]] = 3.0
        y[n, HW - 1, ch[3]] = 3.0                             # only at the last pixel
        y[n, last_block, ch[4]] = 3.0                         # only at the first pixel of the last (partial) block
    return y


def decode_pkey(k):
    k = k.astype(np.uint64)
    o = (k >> np.uint64(32)).astype(np.uint32)
    idx = np.uint32(0xFFFFFFFF) - (k & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    bits = np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32)
    return bits.view(np.float32), idx.astype(np.int64)


def run_ch(L, a, ps):
    a.pass_ = ps
    rc = L.unet_ch_att_op(ctypes.byref(a), S())
    assert rc == 0, L.unet_last_error().decode()


@pytest.mark.parametrize("C,Cr,HW,N", CH_CASES, ids=[f"C{c[0]}-HW{c[2]}-N{c[3]}" for c in CH_CASES])
def test_channel_attention_passes(lib, C, Cr, HW, N):
    m, L = lib
    rec = Rec(f"ch. [{C},{HW},{N}] ")
    g = torch.Generator().manual_seed(C + HW + N)
    rows = 256 // (C // 8)
    npx = N * HW
    pad = 8 if N == 3 else 0                                  # out / dout strided at N = 3, dense otherwise
    y = make_y(N, HW, C, rows, g)
    dout2 = (torch.randn(N, HW, C, generator=g) * 0.5).to(BF)
    act = torch.randn(N, HW, C, generator=g).to(BF)
    yraw = torch.randn(N, HW, C, generator=g).to(BF)
    mean = torch.randn(C, generator=g).float() * 0.3
    invstd = (torch.rand(C, generator=g) * 1.5 + 0.5).float()
    w1 = (torch.randn(Cr, C, generator=g) * (2.0 / C ** 0.5)).float()
    w2 = (torch.randn(C, Cr, generator=g) / Cr ** 0.5).float()
    yn, dn = np64(y), np64(dout2)

    d_y = Padded(npx, C, C + 8, 8, y.to(BF))
    d_out, d_dout = Padded(npx, C, C + pad, 0), Padded(npx, C, C + 2 * pad, pad)
    d_dout2 = Padded(npx, C, C + pad, 0, dout2)
    d_act, d_yraw = Padded(npx, C, C + 8, 0, act), Padded(npx, C, C + 16, 8, yraw)
    d_w1, d_w2, d_mean, d_inv = dev(w1), dev(w2), dev(mean), dev(invstd)
    d_psum = torch.zeros(N * C, dtype=torch.float64, device="cuda")
    d_pkey = torch.zeros(N * C, dtype=torch.int64, device="cuda")
    d_dgate = torch.zeros(N * C, dtype=torch.float64, device="cuda")
    d_gacc = torch.zeros(REP * 2 * C * Cr, dtype=torch.float64, device="cuda")
    d_bs = torch.zeros(REP * 2 * C, dtype=torch.float64, device="cuda")
    d_am, d_h, d_gate, d_dam = f32out(N * 2 * C), f32out(N * 2 * Cr), f32out(N * C), f32out(N * 2 * C)
    d_gw1, d_gw2 = f32out(C * Cr), f32out(C * Cr)
    a = m.ChAttOpArgs(N=N, C=C, Cr=Cr, ldy=d_y.ld, ldo=d_out.ld, lddo2=d_dout2.ld, lddo=d_dout.ld, HW=HW, y=d_y.ptr,
                      out=d_out.ptr, psum=d_psum.data_ptr(), pkey=d_pkey.data_ptr(), w1=d_w1.data_ptr(),
                      w2=d_w2.data_ptr(), am=d_am.data_ptr(), h=d_h.data_ptr(), gate=d_gate.data_ptr(),
                      dout2=d_dout2.ptr, dgate=d_dgate.data_ptr(), dam=d_dam.data_ptr(), gw1=d_gw1.data_ptr(),
                      gw2=d_gw2.data_ptr(), gw_acc=d_gacc.data_ptr(), dout=d_dout.ptr)

    cha = unet_ref.ChannelAttention(C, C // Cr).double()
    fc0, fc2 = cha.fc[0], cha.fc[2]
    with torch.no_grad():
        fc0.weight.copy_(w1.double().view(Cr, C, 1, 1))
        fc2.weight.copy_(w2.double().view(C, Cr, 1, 1))
    w1n, w2n = np64(w1), np64(w2)

    # ================= pass 0: pooling (exact) =================
    run_ch(L, a, 0)
    kv, ki = decode_pkey(d_pkey.cpu().numpy().view(np.uint64).reshape(N, C))
    ynf = y.numpy()
    arg_ref = ynf.argmax(1)                                   # numpy: the first occurrence
    rec.exact("pkey.max", kv, ynf.max(1))
    rec.exact("pkey.arg", ki, arg_ref)
    psum_g = np64(d_psum).reshape(N, C)
    rec.exact("psum", psum_g, yn.sum(1))

    # ================= pass 1: MLP =================
    run_ch(L, a, 1)
    am_g = f32get(rec, "am", d_am, N * 2 * C).reshape(N, 2, C)
    inv_hw = np.float32(1.0) / np.float32(HW)
    rec.exact("am.avg", am_g[:, 0].astype(np.float32), psum_g.astype(np.float32) * inv_hw)
    rec.exact("am.max", am_g[:, 1].astype(np.float32), ynf.max(1))
    y_t = y.double().permute(0, 2, 1).contiguous().view(N, C, HW, 1).requires_grad_(True)
    am_o = torch.stack([cha.avg_pool(y_t).flatten(1), cha.max_pool(y_t).flatten(1)], 1)   # [N][2][C]
    rec.add("am(oracle)", am_g, np64(am_o), 3 * U * np.abs(np64(am_o)))   # float(psum) * float(1 / HW): 3 roundings
    am_t = torch.from_numpy(am_g).requires_grad_(True)
    h_ref_t = torch.relu(fc0(am_t.view(N * 2, C, 1, 1))).view(N, 2, Cr)
    h_g = f32get(rec, "h", d_h, N * 2 * Cr).reshape(N, 2, Cr)
    # h: a sequential dot product over C in one thread: C adds + one product rounding
    S_h = np.abs(am_g) @ np.abs(w1n).T
    b_h = (C + 1) * U * S_h
    rec.add("h", h_g, np64(h_ref_t), b_h)
    h_used = forced(h_ref_t, torch.from_numpy(h_g))
    o_t = fc2(h_used.view(N * 2, Cr, 1, 1)).view(N, 2, C).sum(1)
    gate_ref_t = torch.sigmoid(o_t)
    gate_ref = np64(gate_ref_t)
    gate_g = f32get(rec, "gate", d_gate, N * C).reshape(N, C)
    # o = o1 + o2: two sequential dot products over Cr and their sum
    b_o = (Cr + 2) * U * (np.abs(h_g).sum(1) @ np.abs(w2n).T)
    b_gate = 8 * ulp32(gate_ref) + gate_ref * (1 - gate_ref) * b_o
    rec.add("gate", gate_g, gate_ref, b_gate)

    # ================= pass 2: scale =================
    run_ch(L, a, 2)
    out_g = d_out.get(rec, "out").reshape(N, HW, C)
    rec.bf16("out", out_g, yn * gate_g[:, None, :])

    # ================= pass 3: dgate =================
    run_ch(L, a, 3)
    per_img = min(64, -(-HW // (rows * 16)))
    # pixels per thread + LDS rows + one product
    n3 = -(-HW // (per_img * rows)) + rows + 1
    dgate_g = np64(d_dgate).reshape(N, C)
    rec.add("dgate", dgate_g, (dn * yn).sum(1), n3 * U * (np.abs(dn) * np.abs(yn)).sum(1))

    # ================= pass 4: MLP backward =================
    run_ch(L, a, 4)
    (forced(gate_ref_t, torch.from_numpy(gate_g)) * torch.from_numpy(dgate_g)).sum().backward()
    qg = gate_g * (1 - gate_g)
    dov_abs = np.abs(dgate_g) * qg                                            # [N][C]
    b_dov = 4 * U * dov_abs + np.abs(dgate_g) * np.abs(1 - 2 * gate_g) * b_gate
    dh_abs = dov_abs @ np.abs(w2n)                                            # [N][Cr]
    b_dh = (C + 1) * U * dh_abs + b_dov @ np.abs(w2n)                         # sequential over C
    live = (h_g > 0).astype(np.float64)                                       # [N][2][Cr]
    rec.exact("relu mask", np64(h_ref_t) > 0, h_g > 0)
    hs = h_g.sum(1)                                                           # h_avg + h_max
    gw2_ref, gw1_ref = np64(fc2.weight.grad.view(C, Cr)), np64(fc0.weight.grad.view(Cr, C))
    # per image a few fp32 roundings, fp64 over the images, one rounding to fp32
    b_gw2 = np.einsum("nc,nj->cj", b_dov + 3 * U * dov_abs, hs) + U * np.abs(gw2_ref)
    dh_abs2, b_dh2 = dh_abs[:, None, :] * live, b_dh[:, None, :] * live       # [N][2][Cr]
    b_gw1 = np.einsum("nkj,nkc->jc", b_dh2 + 4 * U * dh_abs2, np.abs(am_g)) + U * np.abs(gw1_ref)
    rec.add("gw2", f32get(rec, "gw2", d_gw2, C * Cr).reshape(C, Cr), gw2_ref, b_gw2)
    rec.add("gw1", f32get(rec, "gw1", d_gw1, C * Cr).reshape(Cr, C), gw1_ref, b_gw1)
    dam_g = f32get(rec, "dam", d_dam, N * 2 * C).reshape(N, 2, C)
    # dam: a sequential dot product over Cr
    b_dam = b_dh2 @ np.abs(w1n) + (Cr + 1) * U * (dh_abs2 @ np.abs(w1n))
    rec.add("dam", dam_g, np64(am_t.grad), b_dam)

    # ================= pass 5: dout (plain, then with the BN reduction fused) =================
    L5 = (am_o * torch.from_numpy(dam_g)).sum() + (y_t * torch.from_numpy(gate_g).view(N, C, 1, 1)
                                                   * dout2.double().permute(0, 2, 1).reshape(N, C, HW, 1)).sum()
    L5.backward()
    dout_ref = np64(y_t.grad.view(N, C, HW).permute(0, 2, 1))                 # torch routes dmax to the first maximum
    base = dn * gate_g[:, None, :] + (dam_g[:, 0] / HW)[:, None, :]
    spike = np.zeros_like(base)
    np.put_along_axis(spike, arg_ref[:, None, :], dam_g[:, 1][:, None, :], 1)
    # the closed form with numpy's first argmax is the oracle's gradient (fp64 roundoff of three terms)
    rec.add("dout(ref)", base + spike, dout_ref, 2.0 ** -50 * np.abs(dout_ref).max())
    xh = (np64(yraw) - np64(mean)) * np64(invstd)
    keep = np64(act) > 0
    ew_img = max(1, min(2048 // N, -(-HW // (rows * 4))))
    n5 = -(-HW // (ew_img * rows)) + rows + 1
    for fused in (False, True):
        tag = "+bb" if fused else ""
        d_dout.buf.fill_(SENT)
        if fused:
            a.act, a.yraw, a.ldact, a.ldyraw = d_act.ptr, d_yraw.ptr, d_act.ld, d_yraw.ld
            a.mean, a.invstd, a.bsums = d_mean.data_ptr(), d_inv.data_ptr(), d_bs.data_ptr()
        run_ch(L, a, 5)
        dout_g = d_dout.get(rec, "dout" + tag).reshape(N, HW, C)
        ref = dout_ref * keep if fused else dout_ref
        rec.bf16("dout" + tag, dout_g, ref)
    bs = np64(d_bs).reshape(REP, 2, C).sum(0)
    dZ = dout_ref * keep
    magn = (np.abs(dn) * gate_g[:, None, :] + np.abs(dam_g[:, 0] / HW)[:, None, :] + np.abs(spike)) * keep
    # d g + da + dm: three roundings (and da = dam * float(1 / HW): two more)
    rec.add("bsums[0]", bs[0], dZ.sum((0, 1)), (n5 + 5) * U * magn.sum((0, 1)))
    rec.add("bsums[1]", bs[1], (dZ * xh).sum((0, 1)), (n5 + 8) * U * (magn * np.abs(xh)).sum((0, 1)))
    # the one pixel that carries dmax, for EVERY (n, c): the same pass with a dmax that stands clear of the dense
    # terms (dam is an input of this pass); what is left after subtracting them sits on the reference's pixel
    big = float(np.float32(4.0 * (np.abs(base).max() + 1.0)))
    dam_s = dam_g.copy()
    dam_s[:, 1] = big * np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
    d_dam[:N * 2 * C].copy_(torch.from_numpy(dam_s.reshape(-1)).float())
    a.act = a.yraw = a.mean = a.invstd = a.bsums = None
    a.ldact = a.ldyraw = 0
    d_dout.buf.fill_(SENT)
    run_ch(L, a, 5)
    dout_s = d_dout.get(rec, "dout@big").reshape(N, HW, C)
    spike_s = np.zeros_like(base)
    np.put_along_axis(spike_s, arg_ref[:, None, :], dam_s[:, 1][:, None, :], 1)
    rec.bf16("dout@big", dout_s, base + spike_s)
    rec.exact("dmax pixel", np.abs(dout_s - base).argmax(1), arg_ref)
    rec.finish()
