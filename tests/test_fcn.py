"""Depthwise Deconvolution dispatch, the Crop layer and the FCN-8s zoo model, CPU side
(tests/test_conv_updw_gpu.py holds the HIP kernels to the oracle of tests/conv_updw_cases.py)."""
import pytest
import torch

import conv_updw_cases as uc
from sparknet_amd import models, proto
from sparknet_amd.core.net import Net
from sparknet_amd.ops.spec import ConvSpec


def test_updw_ok_truth_table(monkeypatch):
    from sparknet_amd.ops.hip import updw_ok
    monkeypatch.delenv("SN_FEATURES", raising=False)

    def mk(P=16, C=21, K=None, r=4, st=2, groups=None):  # the convolution top -> bottom of a deconvolution
        H = (P - 1) * st + r
        return ConvSpec(1, H, H, C if K is None else K, C, r, r, st, st, 0, 0, 1, 1, C if groups is None else groups)
    fcn = (mk(16), mk(34), mk(70, r=16, st=8))  # upscore2, upscore_pool4, upscore8
    assert all(updw_ok(s) for s in fcn) and all(updw_ok(uc.spec(c)) for c in uc.CASES)
    for s in (mk(groups=1), mk(K=42), mk(r=18, st=9), mk(r=17, st=8), mk(r=64, st=32)):  # ungrouped, Kg = 2, ...
        assert not updw_ok(s), s
    monkeypatch.setenv("SN_FEATURES", "deconv_dw=0")  # read at use, not at import
    assert not any(updw_ok(s) for s in fcn)


def _crop_net(shape, ref_shape, axis, offsets):
    dims = lambda sh: " ".join(f"dim: {d}" for d in sh)
    offs = " ".join(f"offset: {o}" for o in offsets)
    return proto.parse_prototxt(
        f'name: "crop" force_backward: true\n'
        f'layer {{ name: "a" type: "Input" top: "a" java_data_param {{ shape {{ {dims(shape)} }} }} }}\n'
        f'layer {{ name: "b" type: "Input" top: "b" java_data_param {{ shape {{ {dims(ref_shape)} }} }} }}\n'
        f'layer {{ name: "c" type: "Crop" bottom: "a" bottom: "b" top: "y" crop_param {{ axis: {axis} {offs} }} }}')


@pytest.mark.parametrize("shape, ref_shape, axis, offsets, window", [
    ((2, 3, 7, 9), (5, 1, 4, 5), 2, (2,), (slice(None), slice(None), slice(2, 6), slice(2, 7))),
    ((2, 5, 7, 9), (9, 3, 4, 5), 1, (1, 3, 0), (slice(None), slice(1, 4), slice(3, 7), slice(0, 5))),
    ((4, 9), (4, 6), 1, (2,), (slice(None), slice(2, 8))),
])
def test_crop_layer(shape, ref_shape, axis, offsets, window):
    """Forward equals the slice; the gradient goes to bottom 0 only and is zero outside the window."""
    param = _crop_net(shape, ref_shape, axis, offsets)
    assert proto.parse_prototxt(proto.to_prototxt(param)) == param
    net = Net(param, phase=proto.TRAIN, device="cpu")
    layer, (top,), (a, b) = net.layers[-1], net.top_vecs[-1], net.bottom_vecs[-1]
    x = torch.randn(shape)
    a.set_nchw(x)
    net.forward()
    assert torch.equal(top.nchw().float(), x[window])
    dy = torch.randn(top.shape)
    top.set_nchw(dy, diff=True)
    layer.backward([top], [True, False], [a, b])
    want = torch.zeros(shape)
    want[window] = dy
    assert torch.equal(a.nchw(diff=True).float(), want)


def test_crop_out_of_range_is_an_error():
    with pytest.raises(ValueError, match="Crop"):
        Net(_crop_net((2, 3, 7, 9), (2, 3, 4, 5), 2, (4,)), phase=proto.TRAIN, device="cpu")


def test_fcn8s_builds_with_the_published_sizes():
    net = Net(models.fcn8s(width=0.125, crop=500), phase=proto.TRAIN, device="cpu")
    size = lambda name: tuple(net.blob_by_name(name).shape)
    assert size("fc6")[2:] == (16, 16) and size("upscore2")[2:] == (34, 34)
    assert size("upscore_pool4")[2:] == (70, 70) and size("upscore8")[2:] == (568, 568)
    assert size("score") == (1, 21, 500, 500)
    ups = {l.name: l for l in net.layers if l.type_name == "Deconvolution"}
    assert list(ups) == ["upscore2", "upscore_pool4", "upscore8"]
    assert [l.param_grads_needed(0) for l in ups.values()] == [True, True, False]
    w = ups["upscore8"].params[0].data  # the bilinear filler: every channel the same separable tent
    assert w.shape[0] == 21 and float(w.max()) < 1.0 and torch.equal(w[0], w[20])
    assert "fcn8s" in models.MODELS and models.solver_for("fcn8s", width=0.125, crop=64).net_param.name


def test_fcn8s_cpu_step():
    net = Net(models.fcn8s(width=0.125, crop=64), phase=proto.TRAIN, device="cpu")
    g = torch.Generator().manual_seed(3)
    net.blob_by_name("data").set_nchw(torch.randn(1, 3, 64, 64, generator=g))
    label = torch.randint(0, 21, (1, 1, 64, 64), generator=g).float()
    label[0, 0, :4] = 255
    net.blob_by_name("label").set_nchw(label)
    loss = float(net.forward())
    net.backward()
    assert loss == loss and abs(loss) != float("inf") and loss > 0
    assert float(net.layer_by_name("upscore2").params[0].diff.abs().sum()) > 0
