"""Grouped pointwise convolution, channel shuffle and ShuffleNet, CPU side (tests/test_conv_gpw_gpu.py
holds the HIP kernels to the oracle of tests/conv_gpw_cases.py): the dispatch predicate, the launches of
one forward + backward, the ShuffleChannel layer and the zoo model."""
import pytest
import torch

import conv_gpw_cases as gc
import conv_trace_cases as tc
from sparknet_amd import dsl, models, proto
from sparknet_amd.core.net import Net
from sparknet_amd.ops.spec import ConvSpec


def test_gpw_ok_truth_table(monkeypatch):
    from sparknet_amd.ops.hip import gpw_ok
    monkeypatch.delenv("SN_FEATURES", raising=False)
    for case in gc.CASES:
        assert gpw_ok(gc.spec(case)), case
    mk = lambda C=48, K=96, r=1, **kw: ConvSpec(2, 8, 8, C, K, r, r, **{"groups": 3, **kw})
    assert gpw_ok(mk())
    for s in (mk(r=3, ph=1, pw=1), mk(sh=2, sw=2), mk(groups=1), mk(C=30), mk(K=30), mk(ph=1, pw=1),
              mk(C=3 * 1028), mk(C=3 * 1024, K=3 * 1024)):  # 3x3, stride 2, ungrouped, Cg = 10, Kg = 10, pad, width, LDS
        assert not gpw_ok(s), s
    monkeypatch.setenv("SN_FEATURES", "conv_gpw=0")  # read at use, not at import
    assert not any(gpw_ok(gc.spec(case)) for case in gc.CASES)


@pytest.mark.parametrize("switch, want", [("", True), ("conv_gpw=0", False)])
def test_forward_and_backward_launch_the_gpw_kernels(switch, want):
    from sparknet_amd.ops import hip
    case = tc.Case(gc.spec(gc.ISOLATION), features=switch, patch={"_gpw_part": lambda s, device: (torch.zeros(8), 8),
                                                                 "relu_backward": lambda dx, gate: dx})
    names = [launch[0] for launch in tc.run(case) if launch[0] != "result"]
    if want:
        assert names == [hip.GPW_FWD, "colsum", hip.GPW_WGRAD, hip.GPW_WGRAD_FINALIZE, hip.GPW_DGRAD]
        assert names == ["conv_gpw_fwd", "colsum", "conv_gpw_wgrad", "conv_gpw_wgrad_finalize", "conv_gpw_dgrad"]
    else:
        assert names and not [n for n in names if n.startswith("conv_gpw")] and "im2col" in names


@pytest.mark.parametrize("shape, G", [((2, 6, 3, 5), 3), ((3, 8), 4)])
def test_shuffle_channel_layer(shape, G):
    dims = " ".join(f"dim: {d}" for d in shape)
    text = (f'name: "shuffle" force_backward: true\n'
            f'layer {{ name: "in" type: "Input" top: "x" java_data_param {{ shape {{ {dims} }} }} }}\n'
            f'layer {{ name: "sh" type: "ShuffleChannel" bottom: "x" top: "y" shuffle_channel_param {{ group: {G} }} }}')
    param = proto.parse_prototxt(text)
    assert proto.parse_prototxt(proto.to_prototxt(param)) == param and param.layer[1].shuffle_channel_param.group == G
    assert dsl.ShuffleChannelLayer("sh", ["x"], G, top=["y"]) == param.layer[1]
    net = Net(param, phase=proto.TRAIN, device="cpu")
    layer, (top,), (bottom,) = net.layers[-1], net.top_vecs[-1], net.bottom_vecs[-1]
    x, dy = torch.randn(shape), torch.randn(shape)
    N, C = shape[:2]
    shuffled = lambda t, g: t.reshape(N, g, C // g, -1).transpose(1, 2).reshape(shape)  # logical (NCHW) order
    bottom.set_nchw(x)
    net.forward()
    assert torch.equal(top.nchw().float(), shuffled(x, G))
    top.set_nchw(dy, diff=True)
    layer.backward([top], [True], [bottom])
    assert torch.equal(bottom.nchw(diff=True).float(), shuffled(dy, C // G))
    assert torch.equal(shuffled(shuffled(x, G), C // G), x)
    with pytest.raises(ValueError, match="ShuffleChannel"):
        Net(proto.parse_prototxt(text.replace(f"group: {G}", "group: 5")), phase=proto.TRAIN, device="cpu")


def test_shufflenet_builds():
    """Learnable elements at groups = 3, worked out by hand from the widths 240 / 480 / 960 (quarter-width
    bottlenecks, Scale with bias after every conv, no conv bias): conv1 648 + 48; stage 2 6 972 + 3 x 10 860;
    stage 3 21 240 + 7 x 40 920; stage 4 80 880 + 3 x 158 640; fc 961 000."""
    net = Net(models.shufflenet(train_batch=2, test_batch=2), phase=proto.TRAIN, device="cpu")
    assert sum(p.data.numel() for l in net.layers if l.type_name != "BatchNorm" for p in l.params) == 1865728
    assert tuple(net.blob_by_name("resx16_elewise").shape) == (2, 960, 7, 7)
    assert tuple(net.blob_by_name("fc1000").shape) == (2, 1000)
    assert sum(l.type_name == "ShuffleChannel" for l in net.layers) == 16
    pointwise = [l for l in net.layers if l.type_name == "Convolution" and l.params[0].data.shape[1] == 1]
    assert [l.lp.convolution_param.group for l in pointwise] == [1] + [3] * 31
    assert "shufflenet" in models.MODELS and models.solver_for("shufflenet", train_batch=1, test_batch=1).net_param.name
