"""The proposal kernels (csrc/kernels/proposal.hip) through ``hip.proposal``, held to the float64 oracle of
tests/proposal_cases.py on every case with a spy on the launch names, and one TEST-phase forward of
faster_rcnn("caffenet", width=0.125, size=96, pre_nms_topn=200, post_nms_topn=16) whose ROIs are held to the same
oracle, and to ``ops.ref.proposal``, on the net's own blobs."""
import pytest
import torch

import proposal_cases as pc
from sparknet_amd import models, proto

pytestmark = pytest.mark.gpu
FOUR = ["proposal_decode", "proposal_select", "proposal_mask", "proposal_scan"]


@pytest.mark.parametrize("case", pc.CASES, ids=pc.IDS)
def test_proposal_kernels(case, gpu, monkeypatch):
    """Membership, order, padding, scores and count exactly; coordinates within the derived bound (exactly with
    zero deltas); two runs bitwise equal; exactly the four launches per run."""
    from sparknet_amd.ops import _lib, hip
    names = []
    monkeypatch.delenv("SN_FEATURES", raising=False)
    monkeypatch.setattr(hip, "call", lambda name, *args: (names.append(name), _lib.call(name, *args))[1])
    i = {k: v.to(gpu) for k, v in pc.inputs(case).items()}
    args = (i["scores"], i["deltas"], i["im_info"], i["anchors"], 16, float(case.min_size), case.pre, case.post,
            case.thresh)
    got, again = hip.proposal(*args), hip.proposal(*args)
    r = pc.check(got, pc.expected(case), case.exact)
    print("proposal", case.name, "count", got[2].tolist(), "worst / bound", r)
    assert r <= 1.0 and all(torch.equal(a, b) for a, b in zip(got, again))
    assert names == FOUR * 2 == [hip.PROPOSAL_DECODE, hip.PROPOSAL_SELECT, hip.PROPOSAL_MASK, hip.PROPOSAL_SCAN] * 2


@pytest.fixture(scope="module")
def runs(gpu):
    """The net's forward with the kernels and with proposal_kernels=0: ROIs, count, launch names, the blobs."""
    from sparknet_amd.core.net import Net
    from sparknet_amd.ops import _lib, hip
    out, names, mp = {}, [], pytest.MonkeyPatch()
    try:
        mp.setattr(hip, "call", lambda name, *args: (names.append(name), _lib.call(name, *args))[1])
        for key, feat in (("on", ""), ("off", "proposal_kernels=0")):
            mp.setenv("SN_FEATURES", feat)
            net = Net(models.faster_rcnn("caffenet", width=0.125, size=96, pre_nms_topn=200, post_nms_topn=16),
                      phase=proto.TEST, device=torch.device(gpu), seed=5)
            net.blob_by_name("data").set_nchw(50 * torch.randn(1, 3, 96, 96, generator=torch.Generator().manual_seed(2)))
            net.blob_by_name("im_info").data.copy_(torch.tensor([[96.0, 96.0, 1.0]]))
            del names[:]
            net.forward()
            layer = net.layer_by_name("proposal")
            out[key] = (net.blob_by_name("rois").data.clone(), layer.count.clone(), [n for n in names if "proposal" in n])
        out["blobs"] = [net.blob_by_name(n).data.clone() for n in ("rpn_cls_prob_reshape", "rpn_bbox_pred", "im_info")]
        out["anchors"], out["cls_prob"] = layer.anchors, tuple(net.blob_by_name("cls_prob").shape)
    finally:
        mp.undo()
    torch.cuda.synchronize()
    return out


def test_faster_rcnn_rois(runs):
    from sparknet_amd.ops import ref
    scores, deltas, info = runs["blobs"]
    assert scores.dtype == deltas.dtype == torch.bfloat16 and runs["cls_prob"] == (16, 21)
    want = pc.oracle(scores.cpu(), deltas.cpu(), info.cpu(), runs["anchors"].cpu(), 16, 16.0, 200, 16, 0.7)
    print("faster_rcnn count", want.count.tolist(), "margins", want.m_extent, want.m_iou)
    by_ref = ref.proposal(scores, deltas, info, runs["anchors"], 16, 16.0, 200, 16, 0.7)
    for key in ("on", "off"):
        rois, count, _ = runs[key]
        assert pc.check((rois, by_ref[1], count), want) <= 1.0
        assert torch.equal(rois[:, 0], by_ref[0][:, 0]) and torch.equal(count, by_ref[2])
    assert pc.check(by_ref, want) <= 1.0


def test_faster_rcnn_launches(runs):
    assert runs["on"][2] == FOUR and runs["off"][2] == []
