"""The Proposal layer and the Faster R-CNN zoo model, CPU side: ``ops.ref.proposal`` against the oracle of
tests/proposal_cases.py, ``hip.proposal_ok``'s refusals, the layer built from prototxt (its own type and the
public Python layer), the model's shapes (tests/test_proposal_gpu.py holds the HIP kernels to the same oracle)."""
import numpy as np
import pytest
import torch

import proposal_cases as pc
from sparknet_amd import models, proto
from sparknet_amd.core.net import Net
from sparknet_amd.ops import hip, ref


@pytest.mark.parametrize("case", pc.CASES, ids=pc.IDS)
def test_ref_proposal(case):
    i, want = pc.inputs(case), pc.expected(case)
    got = ref.proposal(i["scores"].float(), i["deltas"].float(), i["im_info"], i["anchors"], 16, case.min_size,
                       case.pre, case.post, case.thresh)
    assert pc.check(got, want, case.exact) <= 1.0
    boxes = case.H * case.W * len(case.ratios) * len(case.scales)
    if case.name == "decode":  # both the filter and the clipping are active
        assert all(0 < c < boxes for c in want.count) and (want.rois[:, 1:] == 0).any()
    if case.name in ("few", "empty"):  # padding rows
        assert (want.count < case.post).all() and (want.rois[:, 0] == -1).any()


def test_proposal_ok_refusals(monkeypatch):
    monkeypatch.delenv("SN_FEATURES", raising=False)
    t = lambda *shape, dtype=torch.bfloat16: torch.zeros(shape, dtype=dtype)
    s, d, info = t(1, 5, 7, 18), t(1, 5, 7, 36), t(1, 3, dtype=torch.float32)
    assert hip.proposal_ok(s, d, info) and hip.proposal_ok(s, d, info, 0, 315, 1.0)
    assert not hip.proposal_ok(s.float(), d, info) and not hip.proposal_ok(s, d, info.bfloat16())
    assert not hip.proposal_ok(t(1, 128, 256, 4), t(1, 128, 256, 8), info)         # A H W = 65536
    assert hip.proposal_ok(t(1, 255, 257, 2), t(1, 255, 257, 4), info)             # 65535
    assert not hip.proposal_ok(t(1, 255, 257, 2), t(1, 255, 257, 4), info, 0, 300)  # all of them: above 16384
    assert not hip.proposal_ok(s, d, info, 16385, 300) and hip.proposal_ok(s, d, info, 16384, 16384)
    assert not hip.proposal_ok(s, d, info, 100, 101) and not hip.proposal_ok(s, d, info, 100, 0)
    assert not hip.proposal_ok(s, d, info, 100, 10, 1.5)
    monkeypatch.setenv("SN_FEATURES", "proposal_kernels=0")
    assert not hip.proposal_ok(s, d, info)


def _net(layer, force=False, tops='top: "rois" top: "scores"'):
    inputs = "".join(f'layer {{ name: "{n}" type: "Input" top: "{n}" java_data_param {{ shape {{ {dims} }} }} }}\n'
                     for n, dims in (("s", "dim: 2 dim: 18 dim: 5 dim: 7"), ("d", "dim: 2 dim: 36 dim: 5 dim: 7"),
                                     ("i", "dim: 2 dim: 3")))
    return proto.parse_prototxt(f'name: "p" force_backward: {str(force).lower()}\n{inputs}'
                                f'layer {{ name: "p" {layer} bottom: "s" bottom: "d" bottom: "i" {tops} }}')


PUBLIC = ('type: "Python" python_param { module: "rpn.proposal_layer" layer: "ProposalLayer" '
          'param_str: "\'feat_stride\': 16" }')


def test_proposal_layer():
    """Both tops, the forward is the op, no gradient to any bottom even under force_backward."""
    param = _net('type: "Proposal" proposal_param { pre_nms_topn: 50 post_nms_topn: 8 min_size: 4 nms_thresh: 0.5 }', True)
    assert proto.parse_prototxt(proto.to_prototxt(param)) == param
    net = Net(param, phase=proto.TEST, device="cpu")
    layer, (rois, scores), bottoms = net.layers[-1], net.top_vecs[-1], net.bottom_vecs[-1]
    assert tuple(rois.shape) == (16, 5) and tuple(scores.shape) == (16, 1) and net.bottom_need_backward[-1] == [False] * 3
    g = torch.Generator().manual_seed(1)
    bottoms[0].set_nchw(torch.rand(2, 18, 5, 7, generator=g))
    bottoms[1].set_nchw(0.3 * torch.randn(2, 36, 5, 7, generator=g))
    bottoms[2].data.copy_(torch.tensor([[80.0, 112, 1], [60, 100, 2]]))
    net.forward()
    want = ref.proposal(bottoms[0].data, bottoms[1].data, bottoms[2].data, layer.anchors, 16, 4.0, 50, 8, 0.5)
    assert all(torch.equal(a, b) for a, b in zip((rois.data, scores.data, layer.count), want)) and int(want[2].sum()) > 0
    with pytest.raises(ValueError, match="cannot backpropagate"):
        layer.backward([rois, scores], [False, True, False], bottoms)


@pytest.mark.parametrize("phase, pre, post", [(proto.TEST, 6000, 300), (proto.TRAIN, 12000, 2000)])
def test_public_python_layer_is_a_proposal_layer(phase, pre, post):
    layer = Net(_net(PUBLIC, tops='top: "rois"'), phase=phase, device="cpu").layers[-1]
    assert layer.type_name == "Proposal" and (layer.pre, layer.post, layer.nms_thresh, layer.min_size) == (pre, post, 0.7, 16)
    assert layer.feat_stride == 16 and np.array_equal(layer.anchors.numpy(), pc.anchors(pc.R3, pc.S3))


@pytest.mark.parametrize("layer, match", [
    ('type: "Proposal" proposal_param { post_nms_topn: 0 }', "post_nms_topn"),
    ('type: "Proposal" proposal_param { pre_nms_topn: 10 post_nms_topn: 11 }', "post_nms_topn"),
    ('type: "Proposal" proposal_param { nms_thresh: 1.5 }', "nms_thresh"),
    ('type: "Proposal" proposal_param { scale: 8 }', "bottoms of shape"),     # one anchor scale: 3 anchors, not 9
    (PUBLIC.replace("feat_stride", "stride"), "param_str")])
def test_proposal_construction_errors(layer, match):
    with pytest.raises(ValueError, match=match):
        Net(_net(layer), phase=proto.TEST, device="cpu")


def test_faster_rcnn_builds():
    """Phase filtering, blob shapes and the learnable-element counts of the thinned CaffeNet model; VGG-16."""
    kw = dict(trunk="caffenet", width=0.125, size=96, pre_nms_topn=200, post_nms_topn=16)
    train, test = (Net(models.faster_rcnn(**kw), phase=p, device="cpu") for p in (proto.TRAIN, proto.TEST))
    size = lambda net, name: tuple(net.blob_by_name(name).shape)
    assert size(train, "conv5") == (1, 32, 5, 5) and size(train, "rpn_cls_score_reshape") == (1, 2, 45, 5)
    assert size(train, "rpn_labels") == (1, 1, 45, 5) and size(train, "rpn_bbox_targets") == (1, 36, 5, 5)
    assert [l.name for l in train.layers[-2:]] == ["rpn_loss_cls", "rpn_loss_bbox"] and "proposal" not in train.layer_names
    assert size(test, "rpn_cls_prob_reshape") == (1, 18, 5, 5) and size(test, "rois") == (16, 5)
    assert size(test, "roi_pool5") == (16, 32, 6, 6) and size(test, "cls_prob") == (16, 21) and size(test, "bbox_pred") == (16, 84)
    assert "rpn_loss_cls" not in test.layer_names and test.layer_by_name("proposal").type_name == "Proposal"
    count = lambda net: sum(p.count for l in net.layers for p in l.params)
    assert (count(train), count(test)) == (65494, 972351)
    vgg = Net(models.faster_rcnn(width=0.125, size=64), phase=proto.TRAIN, device="cpu")
    assert size(vgg, "conv5_3") == (1, 64, 4, 4) and size(vgg, "rpn_labels") == (1, 1, 36, 4)
    assert "faster_rcnn" in models.MODELS and models.solver_for("faster_rcnn", width=0.125, size=64).stepsize == 60000
