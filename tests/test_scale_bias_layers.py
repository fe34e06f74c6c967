"""Scale and Bias layers on the fp32 CPU engine against a plain torch broadcasting + autograd
oracle (upstream Caffe's test_scale_layer.cpp / test_bias_layer.cpp cover the same forms:
eltwise, broadcast begin / middle / end, scalar, bias term, in place, two bottoms), the schema
of ``scale_param`` / ``bias_param`` and the DSL constructors.

``CONFIGS`` and ``run_config`` are shared with tests/test_scale_bias_gpu.py, which runs every
configuration on the GPU against this CPU engine."""
import pytest
import torch

from sparknet_amd import dsl, proto
from sparknet_amd.core.layer import layer_types
from sparknet_amd.core.net import Net
from test_gradcheck import check_layer

X4 = (2, 3, 4, 5)

# name: (type, bottom[0] shape, param text, in_place, bottom[1] shape or None)
CONFIGS = {
    # one [outer][A][inner] decomposition of the NHWC storage
    "eltwise": ("Scale", X4, "axis: 0 num_axes: -1", False, None),
    "end_hw": ("Scale", X4, "axis: 2 num_axes: 2", False, None),
    "channel_bias": ("Scale", X4, "bias_term: true", False, None),
    "channel8_inplace": ("Scale", (3, 8, 3, 3), "bias_term: true", True, None),
    "chw_num_axes_neg1": ("Scale", X4, "axis: 1 num_axes: -1 bias_term: true", False, None),
    "scalar": ("Scale", X4, "num_axes: 0 bias_term: true", False, None),
    "scalar_axis2": ("Scale", X4, "axis: 2 num_axes: 0", False, None),
    "axis_neg1": ("Scale", X4, "axis: -1", False, None),
    "h_axis": ("Scale", X4, "axis: 2 bias_term: true", False, None),
    "n_axis": ("Scale", X4, "axis: 0", False, None),
    "two_d": ("Scale", (5, 7), "bias_term: true", False, None),
    "three_d_middle": ("Scale", (3, 4, 5), "axis: 1", True, None),
    # covered axes not adjacent in the storage: the NCHW-copy route
    "begin_nc": ("Scale", X4, "axis: 0 num_axes: 2", False, None),
    "middle_ch": ("Scale", X4, "axis: 1 num_axes: 2 bias_term: true", False, None),
    "begin_nch_inplace": ("Scale", X4, "axis: 0 num_axes: 3", True, None),
    # two bottoms: the coefficient is bottom[1] and takes a gradient
    "two_channel": ("Scale", X4, "axis: 1", False, (3,)),
    "two_channel_bias_inplace": ("Scale", X4, "axis: 1 bias_term: true", True, (3,)),
    "two_middle_ch": ("Scale", X4, "axis: 1", False, (3, 4)),
    "two_chw": ("Scale", X4, "axis: 1", False, (3, 4, 5)),
    "two_eltwise": ("Scale", X4, "axis: 0", False, X4),
    "two_scalar": ("Scale", X4, "axis: 1", False, ()),
    # Bias
    "bias_channel": ("Bias", X4, "", False, None),
    "bias_channel8_inplace": ("Bias", (3, 8, 3, 3), "", True, None),
    "bias_eltwise": ("Bias", X4, "axis: 0 num_axes: -1", False, None),
    "bias_end_hw": ("Bias", X4, "axis: 2 num_axes: 2", False, None),
    "bias_middle_ch": ("Bias", X4, "axis: 1 num_axes: 2", False, None),
    "bias_scalar": ("Bias", X4, "num_axes: 0", False, None),
    "bias_two_channel": ("Bias", X4, "axis: 1", False, (3,)),
    "bias_two_d": ("Bias", (5, 7), "", False, None),
}


def layer_text(cfg):
    typ, _, ptxt, in_place, s1 = CONFIGS[cfg]
    pname = "scale_param" if typ == "Scale" else "bias_param"
    bottoms = 'bottom: "x"' + (' bottom: "s"' if s1 is not None else "")
    return (f'layer {{ name: "L" type: "{typ}" {bottoms} top: "{"x" if in_place else "y"}" '
            f'{pname} {{ {ptxt} }} }}')


def build_net(cfg, device="cpu", dtype=None):
    _, s0, _, _, s1 = CONFIGS[cfg]
    bottoms = {"x": s0} if s1 is None else {"x": s0, "s": s1}
    inputs = "".join(
        f'layer {{ name: "in_{n}" type: "Input" top: "{n}" '
        f'java_data_param {{ shape {{ {" ".join(f"dim: {d}" for d in shp)} }} }} }}\n'
        for n, shp in bottoms.items())
    return Net(proto.parse_prototxt(f'name: "g" force_backward: true\n{inputs}{layer_text(cfg)}'),
               phase=proto.TRAIN, seed=3, device=device, dtype=dtype)


def inputs_for(cfg, seed=0):
    """Logical bottoms, Caffe-order params and the top diff, all bf16-representable."""
    net = build_net(cfg)
    layer = net.layers[-1]
    g = torch.Generator().manual_seed(seed)
    rnd = lambda shp: torch.randn(tuple(shp), generator=g).bfloat16().float()
    bottoms = [rnd(b.shape) for b in net.bottom_vecs[-1]]
    params = [rnd(p.caffe_shape) for p in layer.params]
    return bottoms, params, rnd(net.top_vecs[-1][0].shape)


def run_config(cfg, device="cpu", dtype=None, accumulate=False):
    """Forward + backward of the one-layer net; logical tops / bottom diffs and Caffe-order
    param diffs as fp32 CPU tensors.  ``accumulate`` starts from param diffs of 1."""
    bottoms, params, dy = inputs_for(cfg)
    net = build_net(cfg, device, dtype)
    layer, bvec, tvec = net.layers[-1], net.bottom_vecs[-1], net.top_vecs[-1]
    for b, v in zip(bvec, bottoms):
        b.set_nchw(v)
    for p, v in zip(layer.params, params):
        p.set_caffe(v)
        p.diff.fill_(1.0 if accumulate else 0.0)
    layer.forward(bvec, tvec)
    top = tvec[0].nchw().float().cpu().clone()
    tvec[0].set_nchw(dy, diff=True)
    layer.backward(tvec, [True] * len(bvec), bvec)
    return dict(top=top, bdiff=[b.nchw(diff=True).float().cpu().clone() for b in bvec],
                pdiff=[p.to_caffe(p.diff).cpu().clone() for p in layer.params])


def oracle(cfg):
    typ, s0, ptxt, _, s1 = CONFIGS[cfg]
    bottoms, params, dy = inputs_for(cfg)
    sp = proto.parse_prototxt(layer_text(cfg)).layer[0]
    p = sp.scale_param if typ == "Scale" else sp.bias_param
    nd = len(s0)
    if s1 is not None:
        k, a = len(s1), (0 if len(s1) == 0 else (p.axis + nd if p.axis < 0 else p.axis))
    else:
        a = p.axis + nd if p.axis < 0 else p.axis
        k = nd - a if p.num_axes == -1 else p.num_axes
    bshape = [1] * a + list(s0[a:a + k]) + [1] * (nd - a - k)
    leaves = [t.clone().requires_grad_(True) for t in bottoms + params]
    x = leaves[0]
    coefs = [t.reshape(bshape) for t in leaves[1:]]
    if typ == "Scale":
        y = x * coefs[0]
        if len(coefs) > 1:
            y = y + coefs[1]
    else:
        y = x + coefs[0]
    (y * dy).sum().backward()
    nb = len(bottoms)
    return dict(top=y.detach(), bdiff=[t.grad for t in leaves[:nb]], pdiff=[t.grad for t in leaves[nb:]])


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-6)


def compare(got, ref, tol):
    assert got["top"].shape == ref["top"].shape and rel(got["top"], ref["top"]) < tol, ("top", rel(got["top"], ref["top"]))
    assert len(got["bdiff"]) == len(ref["bdiff"]) and len(got["pdiff"]) == len(ref["pdiff"])
    for kind in ("bdiff", "pdiff"):
        for i, (a, b) in enumerate(zip(got[kind], ref[kind])):
            assert a.shape == b.shape, (kind, i, a.shape, b.shape)
            assert rel(a, b) < tol, (kind, i, rel(a, b))


_CPU = {}


def cpu_result(cfg):
    """The CPU engine's result, computed once per configuration and shared."""
    if cfg not in _CPU:
        _CPU[cfg] = run_config(cfg)
    return _CPU[cfg]


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_matches_torch_oracle(cfg):
    compare(cpu_result(cfg), oracle(cfg), 1e-5)


@pytest.mark.parametrize("cfg", ["channel_bias", "middle_ch"])
def test_param_diffs_accumulate(cfg):
    ref = cpu_result(cfg)
    got = run_config(cfg, accumulate=True)
    for a, b in zip(got["pdiff"], ref["pdiff"]):
        assert rel(a, b + 1.0) < 1e-5


def test_lazy_clear_overwrites():
    """After Net.clear_param_diffs(lazy=True) the first backward stores into the stale buffer."""
    bottoms, params, dy = inputs_for("channel_bias")
    net = build_net("channel_bias")
    layer, bvec, tvec = net.layers[-1], net.bottom_vecs[-1], net.top_vecs[-1]
    bvec[0].set_nchw(bottoms[0])
    for p, v in zip(layer.params, params):
        p.set_caffe(v)
    net.flat_diff.fill_(7.0)
    net.clear_param_diffs(lazy=True)
    assert float(net.flat_diff.abs().max()) == 7.0  # nothing was zeroed eagerly
    layer.forward(bvec, tvec)
    tvec[0].set_nchw(dy, diff=True)
    layer.backward(tvec, [True], bvec)
    net.finish_param_diffs()
    ref = cpu_result("channel_bias")
    for p, b in zip(layer.params, ref["pdiff"]):
        assert rel(p.to_caffe(p.diff), b) < 1e-5


@pytest.mark.parametrize("cfg", ["middle_ch", "two_channel"])
def test_finite_difference_gradient(cfg):
    _, s0, _, _, s1 = CONFIGS[cfg]
    check_layer(layer_text(cfg), {"x": s0} if s1 is None else {"x": s0, "s": s1})


def test_default_fillers():
    net = build_net("channel_bias")
    scale, bias = net.layers[-1].params
    assert scale.caffe_shape == (3,) and bias.caffe_shape == (3,)
    assert torch.equal(scale.data, torch.ones(3)) and torch.equal(bias.data, torch.zeros(3))
    net = build_net("bias_channel")
    (bias,) = net.layers[-1].params
    assert torch.equal(bias.data, torch.zeros(3))
    assert [p.caffe_shape for p in build_net("two_channel_bias_inplace").layers[-1].params] == [(3,)]
    assert build_net("two_channel").layers[-1].params == []
    assert build_net("chw_num_axes_neg1").layers[-1].params[0].caffe_shape == (3, 4, 5)
    assert build_net("scalar").layers[-1].params[0].caffe_shape == ()


def test_filler_is_honoured_in_caffe_order():
    txt = ('layer { name: "L" type: "Scale" bottom: "x" top: "y" scale_param { axis: 1 num_axes: 3 '
           'filler { type: "gaussian" std: 1 } bias_term: true bias_filler { type: "constant" value: 0.5 } } }')
    inputs = 'layer { name: "in" type: "Input" top: "x" java_data_param { shape { dim: 2 dim: 3 dim: 4 dim: 5 } } }\n'
    net = Net(proto.parse_prototxt(f'name: "g"\n{inputs}{txt}'), phase=proto.TRAIN, seed=3)
    scale, bias = net.layers[-1].params
    assert scale.caffe_shape == (3, 4, 5) and scale.shape == (4, 5, 3)  # stored in NHWC order
    c = scale.to_caffe()
    assert torch.equal(scale.from_caffe(c), scale.data) and float(c.std()) > 0.5
    assert torch.equal(bias.data, torch.full((4, 5, 3), 0.5))
    x = torch.randn(2, 3, 4, 5)
    net.blob_by_name("x").set_nchw(x)
    net.forward()
    assert rel(net.blob_by_name("y").nchw(), x * c + 0.5) < 1e-6


def test_bad_axes_are_rejected():
    inputs = 'layer { name: "in" type: "Input" top: "x" java_data_param { shape { dim: 2 dim: 3 } } }\n'
    txt = 'layer { name: "L" type: "Scale" bottom: "x" top: "y" scale_param { axis: 1 num_axes: 2 } }'
    with pytest.raises(ValueError):
        Net(proto.parse_prototxt(f'name: "g"\n{inputs}{txt}'), phase=proto.TRAIN)


def test_schema_text_and_binary_round_trip():
    txt = ('name: "s" type: "Scale" bottom: "a" top: "a" scale_param { axis: -1 num_axes: 2 '
           'filler { type: "constant" value: 2 } bias_term: true bias_filler { type: "gaussian" std: 0.1 } }')
    lp = proto.parse_prototxt(txt, proto.LayerParameter)
    sp = lp.scale_param
    assert (sp.axis, sp.num_axes, sp.bias_term, sp.filler.value) == (-1, 2, True, 2.0)
    assert abs(sp.bias_filler.std - 0.1) < 1e-7
    back = proto.LayerParameter.FromString(lp.SerializeToString())
    assert back == lp and proto.parse_prototxt(proto.to_prototxt(lp), proto.LayerParameter) == lp
    bp = proto.parse_prototxt('name: "b" type: "Bias" bias_param { axis: 2 num_axes: 0 filler { value: 3 } }',
                              proto.LayerParameter)
    assert (bp.bias_param.axis, bp.bias_param.num_axes, bp.bias_param.filler.value) == (2, 0, 3.0)
    assert proto.LayerParameter.FromString(bp.SerializeToString()) == bp
    d = proto.LayerParameter()
    assert (d.scale_param.axis, d.scale_param.num_axes, d.scale_param.bias_term) == (1, 1, False)
    assert (d.bias_param.axis, d.bias_param.num_axes) == (1, 1)
    fields = {f.name: f.number for f in proto.LayerParameter.DESCRIPTOR.fields}
    assert fields["bias_param"] == 141 and fields["scale_param"] == 142
    assert {f.name: f.number for f in sp.DESCRIPTOR.fields} == {
        "axis": 1, "num_axes": 2, "filler": 3, "bias_term": 4, "bias_filler": 5}
    assert {f.name: f.number for f in bp.bias_param.DESCRIPTOR.fields} == {"axis": 1, "num_axes": 2, "filler": 3}


def test_hand_written_wire_blob_decodes():
    # name (1) = "L", type (2) = "Scale", field 142 (tag varint f2 08, length-delimited):
    # ScaleParameter { axis (1) = 0, num_axes (2) = 2, bias_term (4) = true }
    blob = bytes([0x0A, 0x01]) + b"L" + bytes([0x12, 0x05]) + b"Scale" + bytes(
        [0xF2, 0x08, 0x06, 0x08, 0x00, 0x10, 0x02, 0x20, 0x01])
    lp = proto.LayerParameter.FromString(blob)
    assert (lp.name, lp.type) == ("L", "Scale") and lp.HasField("scale_param")
    assert (lp.scale_param.axis, lp.scale_param.num_axes, lp.scale_param.bias_term) == (0, 2, True)
    # field 141: BiasParameter { axis = 3 }
    lp = proto.LayerParameter.FromString(bytes([0xEA, 0x08, 0x02, 0x08, 0x03]))
    assert lp.bias_param.axis == 3


def test_registry_and_dsl():
    assert "Scale" in layer_types() and "Bias" in layer_types()
    bn = dsl.BatchNormLayer("bn", ["c"], in_place=True)
    assert list(bn.top) == ["c"] and [p.lr_mult for p in bn.param] == [0.0, 0.0, 0.0]
    sc = dsl.ScaleLayer("sc", ["c"], in_place=True, bias_term=True, filler={"type": "constant", "value": 2.0},
                        param=[(1.0, 0.0), (2.0, 0.0)])
    assert list(sc.top) == ["c"] and sc.scale_param.bias_term and sc.scale_param.filler.value == 2.0
    assert [(p.lr_mult, p.decay_mult) for p in sc.param] == [(1.0, 0.0), (2.0, 0.0)]
    bi = dsl.BiasLayer("bi", ["c"], top=["d"], axis=2, num_axes=2)
    assert (bi.type, bi.bias_param.axis, bi.bias_param.num_axes, list(bi.top)) == ("Bias", 2, 2, ["d"])
    el = dsl.EltwiseLayer("sum", ["a", "b"], "SUM", coeff=[1.0, -1.0])
    assert el.eltwise_param.operation == 1 and list(el.eltwise_param.coeff) == [1.0, -1.0]
    net = dsl.NetParam("n", dsl.RDDLayer("c", [2, 4, 3, 3]), bn, sc, bi)
    n = Net(net, phase=proto.TRAIN)
    n.forward()
    assert n.blob_by_name("d").shape == (2, 4, 3, 3)
