"""Softmax segmentation end to end at 4 x 64 x 64 (base64.npz inputs): the
K-channel U-Net's fp32 logits feed the fused softmax losses and the argmax
confusion metrics through the module API, train_epoch / evaluate, and a
captured GraphedTrainStep.

Labels are made here from the golden cell mask: 0 background, 1 the mask's
boundary (mask minus its 3x3 erosion), 2 its eroded interior.  References are
fp64 restatements on the NATIVE logits copied to the host, so both sides see
the same logits and no pixel has to be excluded; bars are those of
test_softmax_loss_gpu.py (loss 1e-5 relative + 1e-6; metrics from an integer
confusion matrix: equal)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle

pytestmark = pytest.mark.gpu
KEYS = ["accuracy", "f1", "iou", "loss", "precision", "recall"]


def _labels(mask, dtype=torch.uint8):
    m = torch.as_tensor(mask).float()
    interior = 1 - F.max_pool2d(1 - m, 3, 1, 1)  # 3x3 erosion
    return (m + interior)[:, 0].to(dtype).contiguous()


@pytest.fixture(scope="module")
def data(golden):
    base = golden("base64.npz")
    x = torch.from_numpy(base["x"])
    y = _labels(base["masks"])
    assert tuple(y.shape) == (4, 64, 64) and sorted(y.unique().tolist()) == [0, 1, 2]
    return x, y


def _model(pkg, k=3, **kw):
    ref = oracle.ReferenceUNet(n_classes=k)
    sd = oracle.closed_form_state_dict(ref, seed=0)
    m = pkg.UNetWithBackbone(n_classes=k, pretrained=False, use_attention=False, **kw)
    m.load_state_dict(sd)
    return m.cuda(), sd


def _ref_losses(lg, y, ign=-100, alpha=0.5, smooth=1.0, weight=None):
    """fp64: F.cross_entropy and the global per-class Dice on softmax."""
    z, yl = lg.double(), y.long()
    k = z.shape[1]
    valid = (yl >= 0) & (yl < k) & (yl != ign)
    yy = torch.where(valid, yl, torch.full_like(yl, -100))
    w = None if weight is None else torch.as_tensor(weight, dtype=torch.float64)
    ce = F.cross_entropy(z, yy, weight=w, ignore_index=-100).item()
    v = valid.double()[:, None]
    p = torch.softmax(z, 1) * v
    oh = F.one_hot(yl.clamp(0, k - 1), k).permute(0, 3, 1, 2).double() * v
    dice = (1 - ((2 * (p * oh).sum((0, 2, 3)) + smooth) / (p.sum((0, 2, 3)) + oh.sum((0, 2, 3)) + smooth)).mean()).item()
    return {"ce": ce, "softmax_dice": dice, "softmax_combo": alpha * ce + (1 - alpha) * dice}


def _np_confusion(lg, y, ign=-100):
    lg, y = lg.numpy(), y.numpy().astype(np.int64)
    k = lg.shape[1]
    ok = (y >= 0) & (y < k) & (y != ign)
    cm = np.zeros((k, k), dtype=np.int64)
    np.add.at(cm, (y[ok], np.argmax(lg, axis=1)[ok]), 1)
    return cm


def _close(got, want):
    return abs(got - want) <= 1e-5 * abs(want) + 1e-6


def test_model_plus_loss_and_metrics(pkg, cuda, data):
    x, y = data
    m, _ = _model(pkg)
    m.train()
    logits = m(x.cuda())
    assert tuple(logits.shape) == (4, 3, 64, 64) and logits.dtype == torch.float32
    loss = pkg.CrossEntropyLoss()(logits, y.cuda())
    loss.backward()
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert m.conv_final.weight.grad.abs().sum() > 0
    lg = logits.detach().cpu()
    want = _ref_losses(lg, y, alpha=0.3, smooth=2.0, weight=[1.0, 4.0, 2.0])
    plain = _ref_losses(lg, y)
    print("ce", loss.item(), plain["ce"])
    assert _close(loss.item(), plain["ce"])
    cfg = {"loss_alpha": 0.3, "smooth": 2.0, "class_weights": [1.0, 4.0, 2.0]}
    for name in ("ce", "softmax_dice", "softmax_combo"):
        got = pkg.get_loss_function(dict(cfg, loss_fn=name))(logits.detach(), y.cuda()).item()
        print(name, got, want[name])
        assert _close(got, want[name]), name
    got = pkg.calculate_multiclass_metrics(logits.detach(), y.cuda())
    ref = pkg.metrics_from_confusion(_np_confusion(lg, y))
    assert got == ref and np.isfinite([got[k] for k in KEYS if k != "loss"]).all()
    # ~10 % of the pixels ignored: the same agreement
    yi = y.clone()
    yi[torch.rand(yi.shape, generator=torch.Generator().manual_seed(0)) < 0.1] = 255
    got = pkg.CrossEntropyLoss(ignore_index=255)(logits.detach(), yi.cuda()).item()
    assert _close(got, _ref_losses(lg, yi, ign=255)["ce"])
    assert pkg.calculate_multiclass_metrics(logits.detach(), yi.cuda(), 255) == \
        pkg.metrics_from_confusion(_np_confusion(lg, yi, 255))


@pytest.mark.parametrize("name", ["ce", "softmax_combo"])
def test_train_epoch_and_evaluate(pkg, cuda, data, name):
    x, y = data
    m, _ = _model(pkg)
    loader = [(x[:3], y[:3]), (x[3:], y[3:])]  # unequal batches: the weighting shows
    crit = pkg.get_loss_function({"loss_fn": name})
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5)
    dev = torch.device("cuda")
    e = pkg.train_epoch(m, loader, opt, crit, dev)
    v = pkg.evaluate(m, loader, dev, crit)
    for d in (e, v):
        assert sorted(d) == KEYS
        assert all(np.isfinite(d[k]) for k in KEYS), d
    m.eval()
    want = {k: 0.0 for k in KEYS}
    with torch.no_grad():
        for xb, yb in loader:
            lg = m(xb.cuda()).cpu()
            mm = pkg.metrics_from_confusion(_np_confusion(lg, yb))
            for k in ("iou", "accuracy", "precision", "recall", "f1"):
                want[k] += mm[k] * len(xb) / len(x)
            want["loss"] += _ref_losses(lg, yb)[name] * len(xb) / len(x)
    print(name, v, want)
    for k in ("iou", "accuracy", "precision", "recall", "f1"):
        assert v[k] == pytest.approx(want[k], rel=1e-12, abs=1e-15), k
    assert _close(v["loss"], want["loss"])


def test_label_layouts_and_ignore_index_in_the_loop(pkg, cuda, data):
    """[N,1,H,W] int64 labels, and the record's ignore_index taken from the criterion."""
    x, y = data
    m, _ = _model(pkg)
    yi = y.clone()
    yi[:, :8] = 255
    crit = pkg.CrossEntropyLoss(ignore_index=255)
    dev = torch.device("cuda")
    a = pkg.evaluate(m, [(x, yi)], dev, crit)
    b = pkg.evaluate(m, [(x, yi[:, None].long())], dev, crit)
    assert dict(a) == dict(b)
    m.eval()
    with torch.no_grad():
        lg = m(x.cuda()).cpu()
    mm = pkg.metrics_from_confusion(_np_confusion(lg, yi, 255))
    assert a["iou"] == pytest.approx(mm["iou"], rel=1e-12) and a["accuracy"] == pytest.approx(mm["accuracy"], rel=1e-12)
    full = pkg.metrics_from_confusion(_np_confusion(lg, y))
    assert a["accuracy"] != full["accuracy"]  # the ignored rows do count when nothing is ignored


def test_graphed_train_step_uint8_labels(pkg, cuda, data):
    x, y = data
    x1, y1 = x[:2].cuda(), y[:2].cuda()
    x2, y2 = x[2:].cuda(), y[2:].cuda()
    assert y1.dtype == torch.uint8
    crit = pkg.get_loss_function({"loss_fn": "ce"})
    # eager losses of both batches at the initial state (train-mode BN: batch statistics)
    ma, sd = _model(pkg)
    ma.train()
    with torch.no_grad():
        eager1 = crit(ma(x1), y1).item()
        eager2 = crit(ma(x2), y2).item()
    del ma
    m, _ = _model(pkg)
    m.train()
    opt = pkg.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5)
    step = pkg.GraphedTrainStep(m, crit, opt, x1, y1)
    assert step.y.dtype == torch.uint8 and step.y.data_ptr() != y1.data_ptr()

    def reset():  # back to the initial state, in place (the graph keeps its pointers)
        m.load_state_dict(sd)
        for st in opt.state.values():
            for t in st.values():
                if isinstance(t, torch.Tensor):
                    t.zero_()

    reset()
    losses = []
    for _ in range(3):
        out, loss = step()
        losses.append(float(loss))
    print("graphed K=3 ce losses", losses, "eager", eager1, eager2)
    assert all(np.isfinite(losses)) and torch.isfinite(out).all() and tuple(out.shape) == (2, 3, 64, 64)
    assert _close(losses[0], eager1), (losses[0], eager1)
    assert losses[1] != losses[0]  # the captured optimizer step moved the parameters
    reset()
    out, loss = step(x[2:], y[2:])  # a second batch, copied in from the host
    assert torch.equal(step.x, x2) and torch.equal(step.y, y2)
    assert _close(float(loss), eager2), (float(loss), eager2)
    assert abs(eager1 - eager2) > 1e-4 * abs(eager1)  # the two batches do differ


def test_ten_steps_lower_the_loss(pkg, cuda, data):
    x, y = data
    m, _ = _model(pkg)
    m.train()
    crit = pkg.get_loss_function({"loss_fn": "ce"})
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5)
    xd, yd = x.cuda(), y.cuda()
    losses = []
    for _ in range(10):
        loss = crit(m(xd), yd)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("ce over ten steps", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_resnet50_head_feeds_the_same_loss_k2(pkg, golden, cuda):
    base = golden("base64.npz")
    x = torch.from_numpy(base["x"])[:2].cuda()
    y = torch.from_numpy(base["masks"])[:2, 0].to(torch.int64)
    assert sorted(y.unique().tolist()) == [0, 1]
    torch.manual_seed(0)
    m = pkg.UNetWithBackbone(n_classes=2, pretrained=False, use_attention=False, backbone="resnet50").cuda().train()
    logits = m(x)
    assert tuple(logits.shape) == (2, 2, 64, 64)
    loss = pkg.SoftmaxComboLoss()(logits, y.cuda())
    loss.backward()
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert m.conv_final.weight.grad.abs().sum() > 0
    assert _close(loss.item(), _ref_losses(logits.detach().cpu(), y)["softmax_combo"])
