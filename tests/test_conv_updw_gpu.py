"""The depthwise transposed-convolution kernels (csrc/kernels/conv_updw.hip) through ``hip.deconv_dw_forward``
and ``hip.deconv_dw_backward``, held elementwise to the fp64 oracle and the derived bounds of
tests/conv_updw_cases.py on every case, with a spy on the kernel call; one case through a ``Deconvolution``
layer of a net built from prototxt."""
import pytest
import torch

import conv_updw_cases as uc

pytestmark = pytest.mark.gpu


@pytest.fixture
def spy(gpu, monkeypatch):
    """Names of the native launches ops/hip.py makes, in order; the switches at their defaults."""
    from sparknet_amd.ops import _lib, hip
    names = []

    def call(name, *args):
        names.append(name)
        return _lib.call(name, *args)
    monkeypatch.delenv("SN_FEATURES", raising=False)
    monkeypatch.setattr(hip, "call", call)
    return names


@pytest.mark.parametrize("case", uc.CASES, ids=uc.IDS)
def test_forward(case, gpu, spy):
    from sparknet_amd.ops import hip
    i, s = {k: v.to(gpu) for k, v in uc.inputs(case).items()}, uc.spec(case)
    for bias in (True, False):
        y = hip.deconv_dw_forward(i["x"], i["w"], i["bias"] if bias else None, s)
        assert tuple(y.shape) == (s.N, s.H, s.W, s.C) and y.dtype == torch.bfloat16
        r = uc.worst(y, *uc.forward_bound(case, bias))
        print("forward", case, "bias", bias, "worst / bound", r)
        assert r <= 1.0, (bias, r)
    assert spy == [hip.UPDW_FWD] * 2 == ["conv_updw_fwd"] * 2, spy


@pytest.mark.parametrize("case", uc.CASES, ids=uc.IDS)
def test_backward(case, gpu, spy):
    """Store onto 7.0, then accumulate onto 7.0."""
    from sparknet_amd.ops import hip
    i, s = {k: v.to(gpu) for k, v in uc.inputs(case).items()}, uc.spec(case)
    for acc in (False, True):
        dw = torch.full((s.C, s.R, s.S, 1), uc.PREFILL, dtype=torch.float32, device=gpu)
        db = torch.full((s.C,), uc.PREFILL, dtype=torch.float32, device=gpu)
        dx = hip.deconv_dw_backward(i["dy"], i["x"], i["w"], s, True, dw, db, dw_acc=acc, db_acc=acc)
        assert tuple(dx.shape) == (s.N, s.P, s.Q, s.C) and dx.dtype == torch.bfloat16
        bw, bb = uc.wgrad_bound(case, uc.PREFILL if acc else None)
        r = (uc.worst(dx, *uc.dgrad_bound(case)), uc.worst(dw, *bw), uc.worst(db, *bb))
        print("backward", case, "acc", acc, "worst / bound (dx, dw, db)", r)
        assert max(r) <= 1.0, (acc, r)
    assert spy == [hip.UPDW_WGRAD, hip.UPDW_DGRAD] * 2 == ["conv_updw_wgrad", "conv_updw_dgrad"] * 2, spy


def test_deconvolution_layer(gpu, spy):
    """upscore2's shape with a bias through a ``Deconvolution`` layer: top, bottom diff, weight diff, bias diff."""
    from sparknet_amd import proto
    from sparknet_amd.core.net import Net
    from sparknet_amd.ops import hip
    case = uc.UPSCORE2
    i, s = uc.inputs(case), uc.spec(case)
    nchw = lambda t: t.float().permute(0, 3, 1, 2).contiguous()
    net = Net(proto.parse_prototxt(
        f'name: "updw" force_backward: true\n'
        f'layer {{ name: "in" type: "Input" top: "x" java_data_param {{ shape {{ dim: {s.N} dim: {s.C} dim: {s.P} '
        f'dim: {s.Q} }} }} }}\n'
        f'layer {{ name: "up" type: "Deconvolution" bottom: "x" top: "y" convolution_param {{ num_output: {s.C} '
        f'group: {s.C} kernel_size: {s.R} stride: {s.sh} pad: {s.ph} }} }}'),
        phase=proto.TRAIN, device=torch.device(gpu))
    layer, (top,), (bottom,) = net.layers[-1], net.top_vecs[-1], net.bottom_vecs[-1]
    layer.params[0].data.copy_(nchw(i["w"]).reshape(layer.params[0].data.shape))
    layer.params[1].data.copy_(i["bias"])
    net.sync_compute()
    bottom.set_nchw(nchw(i["x"]))
    net.forward()
    top.set_nchw(nchw(i["dy"]), diff=True)
    layer.params[0].diff.zero_()
    layer.params[1].diff.zero_()
    layer.backward([top], [True], [bottom])
    assert [n for n in spy if n.startswith("conv")] == [hip.UPDW_FWD, hip.UPDW_WGRAD, hip.UPDW_DGRAD], spy
    bw, bb = uc.wgrad_bound(case, 0.0)
    r = (uc.worst(top.nchw().permute(0, 2, 3, 1), *uc.forward_bound(case, True)),
         uc.worst(bottom.nchw(diff=True).permute(0, 2, 3, 1), *uc.dgrad_bound(case)),
         uc.worst(layer.params[0].diff.reshape(s.C, s.R, s.S, 1), *bw), uc.worst(layer.params[1].diff, *bb))
    print("layer: worst / bound (y, dx, dw, db)", r)
    assert max(r) <= 1.0, r
