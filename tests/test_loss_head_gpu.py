"""The HIP loss / accuracy head (csrc/kernels/softmax.hip: softmax_xent_fwd / xent_reduce /
softmax_xent_bwd, softmax_fwd / softmax_bwd, accuracy_rows) at its edges.

Every numeric comparison is against fp64 torch on the CPU fed the same bf16 inputs; top-k
accuracy is compared exactly against the sort-of-(score, index)-pairs oracle.  Shapes, oracles
and the derived error bounds live in tests/loss_head_cases.py; tests/test_loss_head.py anchors
the fp32 CPU reference to the same oracles.  In each test the fp32 CPU reference's own error
against fp64 is asserted to lie within the bound in use, so no bound is tighter than fp32 allows.

The issue that asked for these tests states that a label score 60 below the row maximum gives
a row loss of -log(FLT_MIN).  It does not: p = e^-60 / sum >= 8.7e-27 / C is a normal fp32 and
the row loss is 60 + log(sum).  Both regimes are tested: ``saturated`` (60 below, inside the
|x - max| <= 64 range of the probability bound, against fp64) and ``clamped`` (100 below,
p < FLT_MIN, where every row loss must be -log(FLT_MIN) = 87.3365).
"""
import pytest
import torch
import torch.nn.functional as F

from sparknet_amd.ops import ref

import loss_head_cases as lh
from test_layers_gpu import _net
from test_loss_head import collapsed_net_accuracy

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _hip():
    from sparknet_amd.ops import hip
    return hip


def _within(out, ref64, bound, what):
    err = (out.detach().double().cpu() - ref64).abs()
    over = err - bound
    assert bool((over <= 0).all()), (what, "max error", float(err.max()), "worst excess over bound", float(over.max()))


def _forward_checked(x, labels, ignore, normalize, outer, r):
    """Forward on the device twice (bitwise equal), checked against the fp64 reference ``r``;
    the fp32 CPU reference must itself lie within the same bounds."""
    hip = _hip()
    xd, ld = x.to(DEV), labels.to(DEV)
    loss, prob, norm = hip.softmax_loss_forward(xd, ld, ignore, normalize, outer)
    loss2, prob2, norm2 = hip.softmax_loss_forward(xd, ld, ignore, normalize, outer)
    assert torch.equal(loss, loss2) and torch.equal(prob, prob2) and torch.equal(norm, norm2)
    l32, p32, n32 = ref.softmax_loss_forward(x, labels, ignore, normalize, outer)
    assert abs(float(l32) - r["loss"]) <= lh.loss_bound(r), "bound tighter than the fp32 reference's error"
    _within(p32, r["prob"], lh.prob_bound(r), "fp32 reference prob")
    assert float(n32) == r["norm"]
    assert norm.shape == (1,) and float(norm) == r["norm"]
    err = abs(float(loss) - r["loss"])
    assert err <= lh.loss_bound(r), ("loss", float(loss), r["loss"], err, lh.loss_bound(r))
    _within(prob, r["prob"], lh.prob_bound(r), "prob")
    return loss, prob, norm, p32, n32


@pytest.mark.parametrize("ignore", lh.IGNORES, ids=lambda v: f"ignore_{v}")
@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "nonorm"])
@pytest.mark.parametrize("mc", lh.GRID, ids=lh.grid_id)
def test_softmax_loss_grid(gpu, mc, normalize, ignore):
    hip = _hip()
    M, C = mc
    ignore = lh.resolve_ignore(ignore, C)
    outer = None if normalize else (M // 3 or 1)
    labels = lh.make_labels(M, C, ignore)
    x = lh.make_logits(M, C)
    r = lh.xent_ref64(x, labels, ignore, normalize, outer)
    loss, prob, norm, p32, n32 = _forward_checked(x, labels, ignore, normalize, outer, r)
    for lw in (1.0, 0.3):
        r = lh.xent_ref64(x, labels, ignore, normalize, outer, lw)
        dx = hip.softmax_loss_backward(prob, labels.to(DEV), torch.tensor([lw], device=DEV), norm, ignore)
        assert dx.dtype == torch.bfloat16
        d32 = ref.softmax_loss_backward(p32, labels, torch.tensor(lw), n32, ignore, torch.bfloat16)
        _within(d32, r["dx"], lh.xent_dx_bound(r), "fp32 reference dx")
        _within(dx, r["dx"], lh.xent_dx_bound(r), f"dx lw={lw}")
        assert float(dx[~r["valid"].to(DEV)].float().abs().sum()) == 0.0   # ignored rows: exactly zero


@pytest.mark.parametrize("ignore", [0, "C+5", -1], ids=lambda v: f"ignore_{v}")
@pytest.mark.parametrize("mc", [(3, 10), (7, 65), (1029, 10)], ids=lh.grid_id)
def test_softmax_loss_all_rows_ignored(gpu, mc, ignore):
    hip = _hip()
    M, C = mc
    ignore = lh.resolve_ignore(ignore, C)
    labels = lh.make_labels(M, C, ignore, all_ignored=True).to(DEV)
    x = lh.make_logits(M, C).to(DEV)
    loss, prob, norm = hip.softmax_loss_forward(x, labels, ignore, True, M)
    assert float(loss) == 0.0 and float(norm) == 1.0      # normaliser: max(count, 1)
    dx = hip.softmax_loss_backward(prob, labels, torch.tensor([0.3], device=DEV), norm, ignore)
    assert float(dx.float().abs().max()) == 0.0
    loss, _, norm = hip.softmax_loss_forward(x, labels, ignore, False, M // 3 or 1)
    assert float(loss) == 0.0 and float(norm) == float(M // 3 or 1)


@pytest.mark.parametrize("regime", ["saturated", "clamped", "confident"])
@pytest.mark.parametrize("mc", lh.GRID, ids=lh.grid_id)
def test_softmax_loss_regimes(gpu, mc, regime):
    hip = _hip()
    M, C = mc
    labels = lh.make_labels(M, C)
    x = lh.make_logits(M, C, regime, labels)
    r = lh.xent_ref64(x, labels)
    loss, prob, norm, _, _ = _forward_checked(x, labels, None, True, None, r)
    assert float(loss) >= 0.0
    if regime == "clamped":
        assert bool((r["nll"] == lh.NLL_MAX).all())
        assert abs(float(loss) - lh.NLL_MAX) <= lh.P_REL * lh.NLL_MAX + lh.ROW_ABS
    if regime == "confident":
        assert r["loss"] < 1e-7 * C
    dx = hip.softmax_loss_backward(prob, labels.to(DEV), torch.tensor([1.0], device=DEV), norm)
    _within(dx, r["dx"], lh.xent_dx_bound(r), "dx")


@pytest.mark.parametrize("C", [2, 10, 65, 1000])
def test_softmax_loss_single_row_clamp(gpu, C):
    """M = 1: the loss is the row loss.  60 below the maximum it is 60 + log(sum); 100 below, the
    label probability is under FLT_MIN and the row loss is -log(FLT_MIN)."""
    labels = lh.make_labels(1, C, seed=3)
    for regime in ("saturated", "clamped"):
        x = lh.make_logits(1, C, regime, labels, seed=3)
        r = lh.xent_ref64(x, labels)
        loss, _, _, _, _ = _forward_checked(x, labels, None, True, None, r)
        want = lh.NLL_MAX if regime == "clamped" else 60.0 + float(torch.log(torch.exp(x.double() - 8.0).sum()))
        assert abs(r["loss"] - want) <= 1e-12 * want
        assert abs(float(loss) - want) <= lh.P_REL * want + lh.ROW_ABS, (regime, float(loss), want)


@pytest.mark.parametrize("mc", lh.GRID + [(1, 129)], ids=lh.grid_id)
def test_softmax_forward_backward(gpu, mc):
    """bf16 in / out; (1, 129) is one saturated row: the label 100 below the maximum."""
    hip = _hip()
    M, C = mc
    if mc == (1, 129):
        x = lh.make_logits(M, C, "clamped", lh.make_labels(M, C))
    else:
        x = lh.make_logits(M, C)
    y64 = torch.softmax(x.double(), -1)
    _within(ref.softmax_forward(x), y64, lh.softmax_y_bound(y64), "fp32 reference y")
    y = hip.softmax_forward(x.to(DEV))
    assert y.dtype == torch.bfloat16
    _within(y, y64, lh.softmax_y_bound(y64), "y")
    assert torch.equal(y, hip.softmax_forward(x.to(DEV)))
    yb = y64.bfloat16()
    dy = lh.make_logits(M, C, seed=7)
    dx64 = lh.softmax_bwd_ref64(dy, yb)
    bound = lh.softmax_bwd_bound(dy, yb, dx64)
    _within(ref.softmax_backward(dy, yb), dx64, bound, "fp32 reference dx")
    _within(hip.softmax_backward(dy.to(DEV), yb.to(DEV)), dx64, bound, "dx")


@pytest.mark.parametrize("name", sorted(lh.ACCURACY_CASES))
def test_accuracy_cases(gpu, name):
    hip = _hip()
    x, labels, ks, ignore = lh.ACCURACY_CASES[name]
    xd, ld = x.to(DEV), labels.to(DEV)
    for k in ks:
        acc = hip.accuracy(xd, ld, k, ignore)
        hits, n = lh.check_accuracy(acc, x, labels, k, ignore)
        if k == x.shape[1] and n:
            assert float(acc) == 1.0
        if name.startswith("all_ignored"):
            assert n == 0 and float(acc) == 0.0
    if name == "tie_0_vs_64_6x65":
        assert float(hip.accuracy(xd, ld, 1)) == 0.0 and float(hip.accuracy(xd, ld, 2)) == 1.0
    if name == "label_last_6x64":
        assert float(hip.accuracy(xd, ld, 1)) == 1.0


@pytest.mark.parametrize("mc", lh.GRID, ids=lh.grid_id)
def test_accuracy_grid(gpu, mc):
    hip = _hip()
    M, C = mc
    x = lh.half_logits(M, C, seed=4)
    for ignore in (None, 0, C + 5, -1):
        labels = lh.make_labels(M, C, ignore, seed=4)
        for k in sorted({1, min(2, C), min(5, C)}):
            lh.check_accuracy(hip.accuracy(x.to(DEV), labels.to(DEV), k, ignore), x, labels, k, ignore)


def test_fp32_logits_are_cast_not_reinterpreted(gpu):
    """Non-image Input tops are fp32 blobs even in a bf16 net: the wrappers hand the bf16-only
    kernels a bf16 copy (as ``softmax_forward`` does) instead of fp32 bytes read as bf16."""
    hip = _hip()
    x, labels = lh.half_logits(7, 65, seed=6), lh.make_labels(7, 65, seed=6)
    xb, xf, ld = x.to(DEV), x.float().to(DEV), labels.to(DEV)
    assert torch.equal(hip.accuracy(xf, ld, 2), hip.accuracy(xb, ld, 2))
    for a, b in zip(hip.softmax_loss_forward(xf, ld), hip.softmax_loss_forward(xb, ld)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [None, torch.float32], ids=["bf16", "fp32dev"])
def test_collapsed_net_on_device(gpu, dtype):
    """All-zero scores through the bf16 engine (accuracy_rows) and the fp32 device mode."""
    acc, want = collapsed_net_accuracy(DEV, dtype)
    assert abs(acc - want) < 1e-6, (acc, want)


# --------------------------------------------------------------------------------------
# layers on the GPU
# --------------------------------------------------------------------------------------

def _head_inputs(xshape, lshape, C, half=False):
    g = torch.Generator().manual_seed(21)
    x = torch.randn(xshape, generator=g) * 2
    if half:
        x = torch.round(x * 2) / 2
    x = x.bfloat16().float()   # non-image Input tops are fp32 blobs: feed values a bf16 cast keeps
    labels = torch.randint(0, C, lshape, generator=g).float()
    labels.view(-1)[1::4] = 255.0
    return x, labels


def _loss_layer_case(xshape, lshape, normalize):
    C = xshape[1]
    txt = ('layer { name: "L" type: "SoftmaxWithLoss" bottom: "x" bottom: "label" top: "loss" top: "prob" '
           'loss_weight: 0.3 loss_weight: 0 softmax_param { axis: 1 } '
           f'loss_param {{ ignore_label: 255 normalize: {"true" if normalize else "false"} }} }}')
    net = _net(txt, {"x": xshape, "label": lshape}, DEV)
    x, labels = _head_inputs(xshape, lshape, C)
    bx, bl = net.blob_by_name("x"), net.blob_by_name("label")
    bx.set_nchw(x)
    bl.set_nchw(labels)
    total = net.forward()
    li = len(net.layers) - 1
    net.prefill_loss_diffs()
    net.layers[li].backward(net.top_vecs[li], [True, False], net.bottom_vecs[li])

    x64 = bx.nchw().double().cpu().clone().requires_grad_(True)       # the bf16 logits, logical layout
    lab = labels.reshape((xshape[0],) + tuple(xshape[2:])).long()
    count = int((lab != 255).sum())
    norm = float(max(count, 1)) if normalize else float(xshape[0])
    loss64 = F.cross_entropy(x64, lab, ignore_index=255, reduction="sum") / norm
    lw = float(torch.tensor(0.3, dtype=torch.float32))
    (lw * loss64).backward()
    loss64 = float(loss64.detach())
    p64 = torch.softmax(x64.detach(), 1)

    loss = float(net.blob_by_name("loss").data)
    bound = lh.P_REL * abs(loss64) + lh.ROW_ABS * count / norm
    assert abs(loss - loss64) <= bound, (loss, loss64, bound)
    assert abs(float(total) - lw * loss64) <= lw * bound + 2.0 ** -23 * lw * loss64
    _within(net.blob_by_name("prob").nchw(), p64, lh.softmax_y_bound(p64), "prob top")
    dbound = lh.BF16_REL * x64.grad.abs() + lh.P_REL * p64 * lw / norm + lh.P_ABS
    dx = bx.nchw(diff=True)
    _within(dx, x64.grad, dbound, "bottom diff")
    ignored = (lab == 255).unsqueeze(1).expand_as(p64)
    assert float(dx.float().cpu()[ignored].abs().sum()) == 0.0


@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "nonorm"])
def test_softmax_with_loss_layer_spatial(gpu, normalize):
    """axis 1 of an image blob with per-pixel labels (NHWC storage: every pixel is a row)."""
    _loss_layer_case((2, 5, 3, 4), (2, 1, 3, 4), normalize)


@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "nonorm"])
def test_softmax_with_loss_layer_3d(gpu, normalize):
    """A non-image (2, 4, 6) bottom: the generic transpose path of rows_view."""
    _loss_layer_case((2, 4, 6), (2, 6), normalize)


@pytest.mark.parametrize("xshape,lshape", [((2, 5, 3, 4), (2, 1, 3, 4)), ((2, 4, 6), (2, 6))], ids=["spatial", "3d"])
def test_accuracy_layer_axis1(gpu, xshape, lshape):
    C = xshape[1]
    txt = ('layer { name: "L" type: "Accuracy" bottom: "x" bottom: "label" top: "acc" '
           'accuracy_param { top_k: 2 axis: 1 ignore_label: 255 } }')
    net = _net(txt, {"x": xshape, "label": lshape}, DEV)
    x, labels = _head_inputs(xshape, lshape, C, half=True)
    net.blob_by_name("x").set_nchw(x)
    net.blob_by_name("label").set_nchw(labels)
    net.forward()
    rows = x.bfloat16().movedim(1, -1).reshape(-1, C)                 # Caffe's outer-major, inner-minor rows
    hits, n = lh.check_accuracy(net.blob_by_name("acc").data, rows, labels.reshape(-1), 2, 255)
    assert 0 < hits < n
