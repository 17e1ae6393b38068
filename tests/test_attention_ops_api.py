"""CPU checks of the attention single-op entries unet_att_gate_op / unet_ch_att_op
(include/unet_hip.h): every bad argument is refused with a message that names
the field BEFORE anything is launched, so none of these calls touches a GPU.
The well-formed calls (and what the kernels compute) are test_attention_ops_gpu.py's."""
import ctypes
import importlib

import pytest

P = 4096  # a non-null, 16-byte aligned stand-in: every call below is refused before any pointer is used

GATE_PTRS = ("s", "psi_w", "psi_b", "p", "psi", "dbnp", "pst", "pbs", "save", "gamma", "beta", "run_mean", "run_var",
             "nbt", "x", "xatt", "dxatt", "dxpsi", "dS", "gpsi_w", "ggamma", "gbeta", "gpsi_acc")
GATE_BB = ("yraw", "yraw2", "mean", "invstd", "mean2", "invstd2", "bsums", "bsums2")
CH_PTRS = ("y", "out", "psum", "pkey", "w1", "w2", "am", "h", "gate", "dout2", "dgate", "dam", "gw1", "gw2", "gw_acc",
           "dout")
CH_BB = ("act", "yraw", "mean", "invstd", "bsums")


def _lib():
    return importlib.import_module("image-segmentation-project_amd._lib")


def _gate(lib, **kw):
    a = dict(pass_=0, training=1, Fi=32, Fl=64, lds=32, ldx=64, ldxatt=128, lddxatt=128, lddxpsi=64, lddS=32,
             eps=1e-5, momentum=0.1, npix=100, **{n: P for n in GATE_PTRS})
    a.update(kw)
    return lib.AttGateOpArgs(**a)


def _ch(lib, **kw):
    a = dict(pass_=0, N=2, C=64, Cr=4, ldy=64, ldo=64, lddo2=64, lddo=64, HW=100, **{n: P for n in CH_PTRS})
    a.update(kw)
    return lib.ChAttOpArgs(**a)


GATE_FUSED = dict(pass_=3, ldyraw=32, ldyraw2=32, **{n: P for n in GATE_BB})
CH_FUSED = dict(pass_=5, ldact=64, ldyraw=64, **{n: P for n in CH_BB})

# (entry, overrides, words the message must hold)
BAD = [
    ("gate", dict(size=8), ["size"]),
    ("ch", dict(size=8), ["size"]),
    ("gate", dict(pass_=4), ["pass", "0..3"]),
    ("gate", dict(pass_=-1), ["pass", "0..3"]),
    ("ch", dict(pass_=6), ["pass", "0..5"]),
    ("gate", dict(Fi=24, lds=24), ["Fi", "divide 64"]),
    ("gate", dict(Fl=24), ["Fl", "divide 64"]),
    ("gate", dict(Fi=1024, lds=1024), ["Fi", "divide 64"]),
    ("gate", dict(Fl=1024, ldx=1024, ldxatt=1024), ["Fl", "divide 64"]),
    ("gate", dict(Fi=0), ["Fi"]),
    ("gate", dict(Fi=36, lds=40), ["Fi"]),
    ("gate", dict(npix=0), ["npix"]),
    ("ch", dict(C=48, ldy=48), ["C / 8", "divide 256"]),
    ("ch", dict(C=0), ["C / 8"]),
    ("ch", dict(C=4096, ldy=4096), ["C / 8"]),
    ("ch", dict(Cr=0), ["Cr"]),
    ("ch", dict(Cr=-2), ["Cr"]),
    ("ch", dict(N=0), ["N"]),
    ("ch", dict(HW=0), ["HW"]),
    ("ch", dict(HW=2 ** 32 - 1), ["HW", "2^32-2"]),
    # a leading dimension smaller than the width / not a multiple of 8, in the pass that uses it
    ("gate", dict(pass_=0, lds=24), ["lds", "smaller"]),
    ("gate", dict(pass_=0, lds=36), ["lds", "multiple of 8"]),
    ("gate", dict(pass_=1, ldx=56), ["ldx", "smaller"]),
    ("gate", dict(pass_=1, ldxatt=132), ["ldxatt", "multiple of 8"]),
    ("gate", dict(pass_=2, lddxatt=60), ["lddxatt", "smaller"]),
    ("gate", dict(pass_=2, lddxpsi=68), ["lddxpsi", "multiple of 8"]),
    ("gate", dict(pass_=3, lddS=16), ["lddS", "smaller"]),
    ("gate", dict(GATE_FUSED, ldyraw=24), ["ldyraw", "smaller"]),
    ("gate", dict(GATE_FUSED, ldyraw2=36), ["ldyraw2", "multiple of 8"]),
    ("ch", dict(pass_=0, ldy=56), ["ldy", "smaller"]),
    ("ch", dict(pass_=0, ldy=68), ["ldy", "multiple of 8"]),
    ("ch", dict(pass_=2, ldo=60), ["ldo", "smaller"]),
    ("ch", dict(pass_=3, lddo2=100), ["lddo2", "multiple of 8"]),
    ("ch", dict(pass_=5, lddo=8), ["lddo", "smaller"]),
    ("ch", dict(CH_FUSED, ldact=32), ["ldact", "smaller"]),
    ("ch", dict(CH_FUSED, ldyraw=76), ["ldyraw", "multiple of 8"]),
    # a misaligned bf16 buffer (16-byte chunks)
    ("gate", dict(pass_=0, s=P + 2), ["s must", "aligned"]),
    ("ch", dict(pass_=2, out=P + 8), ["out", "aligned"]),
    # a null buffer that the chosen pass reads or writes
    ("gate", dict(pass_=0, s=None), ["s is null"]),
    ("gate", dict(pass_=0, p=None), ["p is null"]),
    ("gate", dict(pass_=0, pst=None), ["pst is null"]),
    ("gate", dict(pass_=1, xatt=None), ["xatt is null"]),
    ("gate", dict(pass_=1, save=None), ["save is null"]),
    ("gate", dict(pass_=1, training=0, run_var=None), ["run_var is null"]),
    ("gate", dict(pass_=2, dxatt=None), ["dxatt is null"]),
    ("gate", dict(pass_=2, pbs=None), ["pbs is null"]),
    ("gate", dict(pass_=3, dS=None), ["dS is null"]),
    ("gate", dict(pass_=3, gpsi_acc=None), ["gpsi_acc is null"]),
    ("gate", dict(pass_=3, ggamma=None), ["ggamma is null"]),
    ("ch", dict(pass_=0, pkey=None), ["pkey is null"]),
    ("ch", dict(pass_=1, w1=None), ["w1 is null"]),
    ("ch", dict(pass_=2, gate=None), ["gate is null"]),
    ("ch", dict(pass_=3, dgate=None), ["dgate is null"]),
    ("ch", dict(pass_=4, gw_acc=None), ["gw_acc is null"]),
    ("ch", dict(pass_=4, dam=None), ["dam is null"]),
    ("ch", dict(pass_=5, dout=None), ["dout is null"]),
    # a fused BN backward that is only partly given
    ("gate", dict(GATE_FUSED, bsums2=None), ["fused", "bsums2"]),
    ("gate", dict(GATE_FUSED, mean2=None), ["fused", "mean2"]),
    ("gate", dict(GATE_FUSED, bsums=None), ["fused", "bsums"]),
    ("gate", dict(pass_=3, ldyraw=32), ["fused", "yraw"]),
    ("ch", dict(CH_FUSED, act=None), ["fused", "act"]),
    ("ch", dict(CH_FUSED, bsums=None), ["fused", "bsums"]),
    ("ch", dict(pass_=5, mean=P), ["fused", "invstd"]),
]


@pytest.mark.parametrize("entry,over,words", BAD, ids=[f"{i:02d}-{b[0]}-{b[2][0].strip()}" for i, b in enumerate(BAD)])
def test_abi_rejects_bad_arguments_before_any_launch(pkg, entry, over, words):
    lib = _lib()
    L = lib.load()
    over = dict(over)
    size = over.pop("size", None)
    a = _gate(lib, **over) if entry == "gate" else _ch(lib, **over)
    if size is not None:
        a.size = size
    fn, name = (L.unet_att_gate_op, "unet_att_gate_op") if entry == "gate" else (L.unet_ch_att_op, "unet_ch_att_op")
    rc = fn(ctypes.byref(a), None)
    err = L.unet_last_error().decode()
    assert rc != 0 and err.startswith(name + ":"), (rc, err)
    for w in words:
        assert w in err, (w, err)


def test_null_argument_struct_is_refused(pkg):
    L = _lib().load()
    assert L.unet_att_gate_op(None, None) != 0 and "unet_att_gate_op" in L.unet_last_error().decode()
    assert L.unet_ch_att_op(None, None) != 0 and "unet_ch_att_op" in L.unet_last_error().decode()


def test_struct_sizes_match_the_header(pkg):
    """The ctypes mirrors are laid out as the C structs: 13 / 11 ints, (2 floats,)
    one int64 and 31 / 21 pointers, naturally aligned."""
    lib = _lib()
    assert ctypes.sizeof(lib.AttGateOpArgs) == 13 * 4 + 2 * 4 + 4 + 8 + 31 * 8
    assert ctypes.sizeof(lib.ChAttOpArgs) == 11 * 4 + 4 + 8 + 21 * 8
