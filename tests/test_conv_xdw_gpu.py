"""The wide-window depthwise kernels (csrc/kernels/conv_xdw.hip) through ``hip.conv_forward`` and
``hip.conv_backward``, held elementwise to the fp64 oracle and the derived bounds of
tests/conv_xdw_cases.py on every case, with a spy on the kernel call; one case through a
``Convolution`` layer object."""
import pytest
import torch

import conv_xdw_cases as xc

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


def _grads(s, gpu):
    return (torch.full((s.C, s.R, s.S, 1), xc.PREFILL, dtype=torch.float32, device=gpu),
            torch.full((s.C,), xc.PREFILL, dtype=torch.float32, device=gpu))


@pytest.mark.parametrize("case", xc.CASES, ids=xc.IDS)
def test_forward(case, gpu, spy):
    from sparknet_amd.ops import hip
    i, s = {k: v.to(gpu) for k, v in xc.inputs(case).items()}, xc.spec(case)
    for bias in (True, False):
        for relu in (True, False):
            y = hip.conv_forward(i["x"], i["w"], i["bias"] if bias else None, s, relu=relu)
            assert tuple(y.shape) == (s.N, s.P, s.Q, s.C) and y.dtype == torch.bfloat16
            r = xc.worst(y, *xc.forward_bound(case, bias, relu))
            print("forward", case, "bias", bias, "relu", relu, "worst / bound", r)
            assert r <= 1.0, (bias, relu, r)
    assert spy == [hip.XDW_FWD] * 4, spy


@pytest.mark.parametrize("case", xc.CASES, ids=xc.IDS)
def test_backward(case, gpu, spy):
    """gate on + store onto 7.0; gate off + accumulate onto 7.0."""
    from sparknet_amd.ops import hip
    i, s = {k: v.to(gpu) for k, v in xc.inputs(case).items()}, xc.spec(case)
    for gate, acc in ((True, False), (False, True)):
        dw, db = _grads(s, gpu)
        dx = hip.conv_backward(i["dy"], i["x"], i["w"], s, True, dw, db, i["gate"] if gate else None,
                               dw_acc=acc, db_acc=acc)
        assert tuple(dx.shape) == (s.N, s.H, s.W, s.C) and dx.dtype == torch.bfloat16
        bw, bb = xc.wgrad_bound(case, xc.PREFILL if acc else None)
        r = (xc.worst(dx, *xc.dgrad_bound(case, gate)), xc.worst(dw, *bw), xc.worst(db, *bb))
        print("backward", case, "gate", gate, "acc", acc, "worst / bound (dx, dw, db)", r)
        assert max(r) <= 1.0, (gate, acc, r)
    assert spy == [hip.XDW_WGRAD, hip.XDW_DGRAD] * 2, spy


def test_convolution_layer(gpu, spy):
    """A 5x5 / 2 depthwise ``Convolution`` layer of a net: its top, bottom gradient and weight gradient."""
    from sparknet_amd import proto
    from sparknet_amd.core.net import Net
    from sparknet_amd.ops import hip
    case = xc.MNASNET_LIKE
    i, s = xc.inputs(case), xc.spec(case)
    nchw = lambda t: t.float().permute(0, 3, 1, 2).contiguous()
    net = Net(proto.parse_prototxt(
        f'name: "xdw" force_backward: true\n'
        f'layer {{ name: "in" type: "Input" top: "x" java_data_param {{ shape {{ dim: {s.N} dim: {s.C} dim: {s.H} '
        f'dim: {s.W} }} }} }}\n'
        f'layer {{ name: "dw" type: "Convolution" bottom: "x" top: "y" convolution_param {{ num_output: {s.C} '
        f'group: {s.C} kernel_size: {s.R} stride: {s.sh} pad: {s.ph} bias_term: false }} }}'),
        phase=proto.TRAIN, device=torch.device(gpu))
    layer, (top,), (bottom,) = net.layers[-1], net.top_vecs[-1], net.bottom_vecs[-1]
    layer.params[0].data.copy_(nchw(i["w"]).reshape(layer.params[0].data.shape))
    net.sync_compute()
    bottom.set_nchw(nchw(i["x"]))
    net.forward()
    top.set_nchw(nchw(i["dy"]), diff=True)
    layer.params[0].diff.zero_()
    layer.backward([top], [True], [bottom])
    assert [n for n in spy if n.startswith("conv")] == [hip.XDW_FWD, hip.XDW_WGRAD, hip.XDW_DGRAD], spy
    r = (xc.worst(top.nchw().permute(0, 2, 3, 1), *xc.forward_bound(case, False, False)),
         xc.worst(bottom.nchw(diff=True).permute(0, 2, 3, 1), *xc.dgrad_bound(case, False)),
         xc.worst(layer.params[0].diff.reshape(s.C, s.R, s.S, 1), *xc.wgrad_bound(case, 0.0)[0]))
    print("layer: worst / bound (y, dx, dw)", r)
    assert max(r) <= 1.0, r
