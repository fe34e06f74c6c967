"""ROIPooling, ROIAlign, SmoothL1Loss and the Fast R-CNN zoo model, CPU side: ``ops.ref`` against the oracle of
tests/roi_cases.py, the layers built from prototxt, the model's shapes (tests/test_roi_gpu.py holds the HIP
kernels to the same oracle)."""
import pytest
import torch

import roi_cases as rc
from sparknet_amd import models, proto
from sparknet_amd.core.net import Net
from sparknet_amd.ops import ref


def test_no_sample_near_a_cutoff():
    """A condition on the cases, not a tolerance: a sample within 1e-4 of -1 or H could fall on either side."""
    seen = {"clamped_low": 0, "clamped_high": 0, "zero": 0}
    for case in rc.CASES:
        for sampling in (0, 2):
            for _, _, ys, xs, _, _ in rc.align_axes(case, sampling):
                for samples, L in ((ys, case.H), (xs, case.W)):
                    for _, v, corners in samples:
                        assert min(abs(float(v) + 1), abs(float(v) - L)) > 1e-4, (case.name, v)
                        seen["clamped_low"] += -1 < v < 0
                        seen["clamped_high"] += L - 1 < v < L
                        seen["zero"] += not corners
    assert all(seen.values()), seen


@pytest.mark.parametrize("case", rc.CASES, ids=rc.IDS)
def test_ref_roi_pool(case):
    i = rc.inputs(case)
    y, am = ref.roi_pool_forward(i["x"].float(), i["rois"], case.PH, case.PW, case.scale)
    want_y, want_am, dx = rc.pool_oracle(case)
    assert torch.equal(y.double(), torch.from_numpy(want_y)) and torch.equal(am.long(), torch.from_numpy(want_am))
    got = ref.roi_pool_backward(i["dy"].float(), i["rois"], am, i["x"].shape, case.PH, case.PW, case.scale)
    assert rc.worst(got, *rc.bound(*dx)) <= 1.0


@pytest.mark.parametrize("sampling", (0, 2))
@pytest.mark.parametrize("case", rc.CASES, ids=rc.IDS)
def test_ref_roi_align(case, sampling):
    i = rc.inputs(case)
    fwd, bwd = rc.align_oracle(case, sampling)
    y = ref.roi_align_forward(i["x"].float(), i["rois"], case.PH, case.PW, case.scale, sampling)
    dx = ref.roi_align_backward(i["dy"].float(), i["rois"], i["x"].shape, case.PH, case.PW, case.scale, sampling)
    assert max(rc.worst(y, *rc.bound(*fwd)), rc.worst(dx, *rc.bound(*bwd))) <= 1.0


@pytest.mark.parametrize("sigma, nb", rc.L1_CASES)
def test_ref_smooth_l1(sigma, nb):
    (pred, target, in_w, out_w), loss, grad = rc.smooth_l1(sigma, nb)
    assert rc.worst(ref.smooth_l1_forward(pred.float(), target, in_w, out_w, sigma), *loss) <= 1.0
    dp, dt = ref.smooth_l1_backward(pred.float(), target, in_w, out_w, sigma, torch.tensor(0.75), True)
    assert rc.worst(dp, *grad) <= 1.0 and torch.equal(dt, -dp)


def _net(layer, rois=3, extra=""):
    return proto.parse_prototxt(
        f'name: "roi" force_backward: true\n'
        f'layer {{ name: "x" type: "Input" top: "x" java_data_param {{ shape {{ dim: 2 dim: 5 dim: 6 dim: 7 }} }} }}\n'
        f'layer {{ name: "r" type: "Input" top: "r" java_data_param {{ shape {{ dim: {rois} dim: 5 }} }} }}\n'
        f'layer {{ name: "p" type: "{layer}" bottom: "x" bottom: "r" top: "y" {extra} }}')


@pytest.mark.parametrize("layer, extra, fn", [
    ("ROIPooling", "roi_pooling_param { pooled_h: 3 pooled_w: 2 spatial_scale: 0.5 }",
     lambda x, r: ref.roi_pool_forward(x, r, 3, 2, 0.5)[0]),
    ("ROIAlign", "roi_align_param { pooled_h: 3 pooled_w: 2 spatial_scale: 0.5 sampling_ratio: 2 }",
     lambda x, r: ref.roi_align_forward(x, r, 3, 2, 0.5, 2))])
def test_roi_layers(layer, extra, fn):
    """Top [R, C, PH, PW]; the forward is the op; the gradient reaches bottom 0 only."""
    param = _net(layer, extra=extra)
    assert proto.parse_prototxt(proto.to_prototxt(param)) == param
    net = Net(param, phase=proto.TRAIN, device="cpu")
    top, (x, r) = net.top_vecs[-1][0], net.bottom_vecs[-1]
    assert tuple(top.shape) == (3, 5, 3, 2) and net.bottom_need_backward[-1] == [True, False]
    x.set_nchw(torch.randn(2, 5, 6, 7))
    r.data.copy_(torch.tensor([[0, 0, 0, 12, 10], [1, 2, 2, 9, 7], [2, 0, 0, 4, 4.0]]))
    net.forward()
    assert torch.equal(top.data, fn(x.data, r.data)) and float(top.data[2].abs().sum()) == 0
    top.set_nchw(torch.ones(top.shape), diff=True)
    net.layers[-1].backward([top], [True, False], [x, r])
    assert float(x.diff.sum()) == pytest.approx(2 * 5 * 3 * 2) and not r.has_diff()
    with pytest.raises(ValueError, match="cannot backpropagate"):
        net.layers[-1].backward([top], [True, True], [x, r])


@pytest.mark.parametrize("layer, extra", [("ROIPooling", "roi_pooling_param { pooled_h: 0 pooled_w: 2 }"),
                                          ("ROIPooling", ""), ("ROIAlign", "roi_align_param { pooled_h: 2 }")])
def test_roi_construction_errors(layer, extra):
    with pytest.raises(ValueError, match="must be positive"):
        Net(_net(layer, extra=extra), phase=proto.TRAIN, device="cpu")


@pytest.mark.parametrize("sigma, nb", rc.L1_CASES)
def test_smooth_l1_layer(sigma, nb):
    (pred, target, in_w, out_w), loss, grad = rc.smooth_l1(sigma, nb)
    names = ["pred", "target", "in_w", "out_w"][:nb]
    inputs = "".join(f'layer {{ name: "{n}" type: "Input" top: "{n}" java_data_param {{ shape {{ dim: 6 dim: 12 }} }} }}\n'
                     for n in names)
    net = Net(proto.parse_prototxt(
        f'name: "l1" force_backward: true\n{inputs}layer {{ name: "loss" type: "SmoothL1Loss" loss_weight: 0.75 '
        f'{" ".join(f"bottom: {chr(34)}{n}{chr(34)}" for n in names)} top: "loss" smooth_l1_loss_param {{ sigma: {sigma} }} }}'),
        phase=proto.TRAIN, device="cpu")
    assert net.bottom_need_backward[-1] == [True] + [False] * (nb - 1)
    for n, t in zip(names, (pred.float(), target, in_w, out_w)):
        net.blob_by_name(n).data.copy_(t)
    assert rc.worst(net.forward() / 0.75, *loss) <= 1.0
    net.backward()
    assert rc.worst(net.blob_by_name("pred").diff, *grad) <= 1.0


def test_fast_rcnn_builds():
    """Blob shapes and the learnable-element count of the thinned CaffeNet model; VGG-16 with ROIAlign."""
    net = Net(models.fast_rcnn(width=0.125, rois=8, size=64), phase=proto.TRAIN, device="cpu")
    size = lambda name: tuple(net.blob_by_name(name).shape)
    assert size("conv5") == (2, 32, 3, 3) and size("roi_pool5") == (8, 32, 6, 6) and size("fc7") == (8, 512)
    assert size("cls_score") == (8, 21) and size("bbox_pred") == (8, 84) and size("rois") == (8, 5)
    assert sum(p.count for l in net.layers for p in l.params) == 950345
    assert [l.type_name for l in net.layers[-2:]] == ["SoftmaxWithLoss", "SmoothL1Loss"]
    assert not net.layer_by_name("conv1").param_grads_needed(0) and net.layer_by_name("conv2").param_grads_needed(0)
    vgg = Net(models.fast_rcnn("vgg16", width=0.125, rois=8, size=64, align=True), phase=proto.TRAIN, device="cpu")
    assert vgg.layer_by_name("roi_pool5").type_name == "ROIAlign" and tuple(vgg.blob_by_name("roi_pool5").shape) == (8, 64, 7, 7)
    assert "fast_rcnn" in models.MODELS and models.solver_for("fast_rcnn", width=0.125, size=64).net_param.name
