"""The region-of-interest kernels (csrc/kernels/roi.hip) through the ``hip`` wrappers, held to the oracle and the
derived bounds of tests/roi_cases.py on every case with a spy on the launch names, and one forward / backward of
fast_rcnn(trunk="caffenet", width=0.125, images=2, rois=8, size=64) against the fp32 CPU engine."""
import pytest
import torch

import roi_cases as rc
from sparknet_amd import models, proto

pytestmark = pytest.mark.gpu


@pytest.fixture
def spy(gpu, monkeypatch):
    """Names of the native launches ops/hip.py makes, in order; the switches at their defaults."""
    from sparknet_amd.ops import _lib, hip
    names = []
    monkeypatch.delenv("SN_FEATURES", raising=False)
    monkeypatch.setattr(hip, "call", lambda name, *args: (names.append(name), _lib.call(name, *args))[1])
    return names


@pytest.mark.parametrize("case", rc.CASES, ids=rc.IDS)
def test_roi_pool(case, gpu, spy):
    """The forward exactly, argmax included; the backward within its bound and bitwise equal when run twice."""
    from sparknet_amd.ops import hip
    assert hip.ROI_CHUNK == rc.CHUNK == hip._lib.kernels().sn_roi_chunk()
    i, geo = {k: v.to(gpu) for k, v in rc.inputs(case).items()}, (case.PH, case.PW, case.scale)
    want_y, want_am, dxo = rc.pool_oracle(case)
    y, am = hip.roi_pool_forward(i["x"], i["rois"], *geo)
    assert y.dtype == torch.bfloat16 and torch.equal(y.double().cpu(), torch.from_numpy(want_y))
    assert am.dtype == torch.int32 and torch.equal(am.long().cpu(), torch.from_numpy(want_am))
    dx, again = (hip.roi_pool_backward(i["dy"], i["rois"], am, i["x"].shape, *geo) for _ in range(2))
    r = rc.worst(dx, *rc.bound(*dxo))
    print("roi_pool", case.name, "backward worst / bound", r)
    assert r <= 1.0 and torch.equal(dx, again)
    assert spy == [hip.ROI_POOL_FWD] + [hip.ROI_POOL_BWD] * 2 == ["roi_pool_fwd"] + ["roi_pool_bwd"] * 2, spy


@pytest.mark.parametrize("sampling", (0, 2))
@pytest.mark.parametrize("case", rc.CASES, ids=rc.IDS)
def test_roi_align(case, sampling, gpu, spy):
    from sparknet_amd.ops import hip
    i, geo = {k: v.to(gpu) for k, v in rc.inputs(case).items()}, (case.PH, case.PW, case.scale, sampling)
    fwd, bwd = rc.align_oracle(case, sampling)
    y = hip.roi_align_forward(i["x"], i["rois"], *geo)
    dx, again = (hip.roi_align_backward(i["dy"], i["rois"], i["x"].shape, *geo) for _ in range(2))
    r = (rc.worst(y, *rc.bound(*fwd)), rc.worst(dx, *rc.bound(*bwd)))
    print("roi_align", case.name, sampling, "worst / bound (y, dx)", r)
    assert max(r) <= 1.0 and torch.equal(dx, again)
    assert spy == [hip.ROI_ALIGN_FWD] + [hip.ROI_ALIGN_BWD] * 2 == ["roi_align_fwd"] + ["roi_align_bwd"] * 2, spy


@pytest.mark.parametrize("sigma, nb", rc.L1_CASES)
def test_smooth_l1(sigma, nb, gpu, spy):
    from sparknet_amd.ops import hip
    ops_, loss, grad = rc.smooth_l1(sigma, nb)
    pred, target, in_w, out_w = (None if t is None else t.to(gpu) for t in ops_)
    got = hip.smooth_l1_forward(pred, target, in_w, out_w, sigma)
    dp, dt = hip.smooth_l1_backward(pred, target, in_w, out_w, sigma, torch.tensor(0.75, device=gpu), True)
    r = (rc.worst(got, *loss), rc.worst(dp, *grad), rc.worst(-dt, *grad))
    print("smooth_l1", sigma, nb, "worst / bound (loss, dpred, dtarget)", r)
    assert dp.dtype == torch.bfloat16 and dt.dtype == torch.float32 and max(r) <= 1.0
    assert spy == [hip.SMOOTH_L1_FWD, hip.SMOOTH_L1_BWD] == ["smooth_l1_fwd", "smooth_l1_bwd"], spy


def _run(dev, w0, feed):
    from sparknet_amd.core.net import Net
    net = Net(models.fast_rcnn("caffenet", width=0.125, images=2, rois=8, size=64), phase=proto.TRAIN,
              device=torch.device(dev), seed=5)
    if w0 is not None:
        net.flat_data.copy_(w0.to(net.flat_data.device))
        net.sync_compute()
    start = net.flat_data.detach().cpu().clone()
    for name, t in feed.items():
        net.blob_by_name(name).set_nchw(t)
    loss = float(net.forward())
    net.backward()
    return start, loss


@pytest.fixture(scope="module")
def runs(gpu):
    from sparknet_amd.ops import _lib, hip
    g = torch.Generator().manual_seed(8)
    boxes = torch.randint(0, 32, (8, 2, 2), generator=g).sort(dim=1).values.float() + torch.tensor([[[0.0], [31.0]]])
    inside = (torch.rand(8, 84, generator=g) > 0.8).float()
    feed = {"data": torch.randn(2, 3, 64, 64, generator=g), "labels": torch.randint(0, 21, (8,), generator=g).float(),
            "rois": torch.cat([torch.arange(8.0).reshape(8, 1) % 2, boxes[:, 0], boxes[:, 1]], 1),
            "bbox_targets": torch.randn(8, 84, generator=g), "bbox_inside_weights": inside,
            "bbox_outside_weights": inside}
    w0, cpu = _run("cpu", None, feed)
    out, names = {"cpu": cpu}, []
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(hip, "call", lambda name, *args: (names.append(name), _lib.call(name, *args))[1])
        for key, feat in (("roi", ""), ("off", "roi_kernels=0")):
            mp.setenv("SN_FEATURES", feat)
            del names[:]
            out[key] = _run(gpu, w0, feed)[1]
            out["launches_" + key] = {n: names.count(n) for n in set(names) if n.startswith(("roi_", "smooth_l1"))}
    finally:
        mp.undo()
    torch.cuda.synchronize()
    return out


def test_fast_rcnn_launches(runs):
    assert runs["launches_roi"] == {"roi_pool_fwd": 1, "roi_pool_bwd": 1, "smooth_l1_fwd": 1, "smooth_l1_bwd": 1}
    assert runs["launches_off"] == {"smooth_l1_fwd": 1, "smooth_l1_bwd": 1}


def test_fast_rcnn_loss_matches_fp32_cpu(runs):
    """The yardstick is the roi_kernels=0 run's deviation from the fp32 CPU loss — the same net with ROIPooling on
    the tensor route, everything else identical; the kernels get twice that.  Measured on an MI355X: CPU loss
    11.680638, both GPU runs 11.680683, so both deviations are 4.48e-05 (the forward is a selection: bitwise equal)."""
    lc, lg, lo = runs["cpu"], runs["roi"], runs["off"]
    print("loss cpu", lc, "roi kernels", lg, "roi_kernels=0", lo, "deviations", abs(lg - lc), abs(lo - lc))
    assert abs(lg - lc) <= 2 * abs(lo - lc)
