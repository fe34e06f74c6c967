"""Squeeze-and-excitation, CPU side (tests/test_se_gpu.py holds the HIP kernels to the same oracle
and bounds; tests/se_cases.py has them): every mutant of the oracle violates its bound by at least
100x, the Axpy layer on the fp32 CPU engine, the (N, C) route of Scale / Bias, and the SE-ResNet
zoo model."""
import pytest
import torch

import se_cases as sc
from sparknet_amd import dsl, models, proto
from sparknet_amd.core.layer import layer_types
from sparknet_amd.core.net import Net
from test_gradcheck import check_layer


# --- mutants ----------------------------------------------------------------------------------

def _fwd(case, **kw):
    i = sc.inputs(case)
    return sc.worst(sc.forward64(i["x"], i["s"], i["b"], i["r"], **kw), *sc.forward_bound(case))


def _bwd(case, which, **kw):
    i = sc.inputs(case)
    return sc.worst(sc.backward64(i["dy"], i["x"], i["s"], **kw)[which], *sc.backward_bound(case)[which])


def _pool(case, **kw):
    return sc.worst(sc.pool64(sc.inputs(case)["x"], **kw), *sc.pool_bound(case))


MUTANTS = {  # name: (worst ratio of a case, can the mutant show on that case?)
    "ds: the last pixel left out": (lambda c: _bwd(c, 1, skip_last=True), lambda c: c[1] * c[2] >= 2),
    "db: the last pixel left out": (lambda c: _bwd(c, 2, skip_last=True), lambda c: c[1] * c[2] >= 2),
    "pool: the last pixel left out": (lambda c: _pool(c, skip_last=True), lambda c: c[1] * c[2] >= 2),
    "forward: the gate of image 0 for every image": (lambda c: _fwd(c, gate0=True), lambda c: c[0] >= 2),
    "dx: the gate of image 0 for every image": (lambda c: _bwd(c, 0, gate0=True), lambda c: c[0] >= 2),
    "forward: r dropped": (lambda c: _fwd(c, drop_r=True), lambda c: True),
    "ds: computed without x": (lambda c: _bwd(c, 1, no_x=True), lambda c: True),
    "pool: the mean divided by M + 1": (lambda c: _pool(c, div_plus_one=True), lambda c: True),
    "ds: accumulate treated as store": (
        lambda c: sc.worst(sc.backward_bound(c)[1][0], *sc.backward_bound(c, prefill=sc.PREFILL)[1]), lambda c: True),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_every_mutant_violates_its_bound(name):
    ratio, shows = MUTANTS[name]
    ratios = {c: ratio(c) for c in sc.CASES if shows(c)}
    assert max(ratios.values()) >= 100.0, ratios


def test_the_oracle_meets_its_own_bounds():
    for c in sc.CASES:
        assert _fwd(c) == 0.0 and _bwd(c, 0) == 0.0 and _bwd(c, 1) == 0.0 and _bwd(c, 2) == 0.0 and _pool(c) == 0.0


# --- Axpy on the CPU ----------------------------------------------------------------------------

def _axpy_text(a_shape, x_shape, y_shape=None):
    dims = lambda s: " ".join(f"dim: {d}" for d in s)
    inp = "".join(f'layer {{ name: "in_{n}" type: "Input" top: "{n}" java_data_param {{ shape {{ {dims(s)} }} }} }}\n'
                  for n, s in (("a", a_shape), ("x", x_shape), ("y", y_shape or x_shape)))
    return inp, 'layer { name: "L" type: "Axpy" bottom: "a" bottom: "x" bottom: "y" top: "t" }'


def axpy_net(case, device="cpu", image_gate=False, dtype=None):
    N, H, W, C = case
    inp, txt = _axpy_text((N, C, 1, 1) if image_gate else (N, C), (N, C, H, W))
    return Net(proto.parse_prototxt(f'name: "g" force_backward: true\n{inp}{txt}'), phase=proto.TRAIN, seed=3,
               device=device, dtype=dtype)


def run_axpy(case, device="cpu", image_gate=False, propagate=(True, True, True), dtype=None):
    """Forward + backward of the one-layer net on the inputs of se_cases; NHWC top and the bottom
    gradients that were asked for (None otherwise; the gate's as [N, C])."""
    i = sc.inputs(case)
    net = axpy_net(case, device, image_gate, dtype)
    layer, bvec, tvec = net.layers[-1], net.bottom_vecs[-1], net.top_vecs[-1]
    N, H, W, C = case
    bvec[0].set_nchw(i["s"].reshape(bvec[0].shape))
    bvec[1].set_nchw(i["x"].float().permute(0, 3, 1, 2))
    bvec[2].set_nchw(i["r"].float().permute(0, 3, 1, 2))
    for b in bvec:
        b.diff = torch.full_like(b.data, 5.0)  # a gradient that is not asked for must stay as it is
    layer.forward(bvec, tvec)
    top = tvec[0].data.detach().clone()
    tvec[0].set_nchw(i["dy"].float().permute(0, 3, 1, 2), diff=True)
    layer.backward(tvec, list(propagate), bvec)
    grads = [b.diff.detach().clone() for b in bvec]
    for g, p in zip(grads, propagate):
        assert p or bool((g == 5.0).all())
    return top, [g.reshape(N, C) if k == 0 else g for k, g in enumerate(grads)]


@pytest.mark.parametrize("case", sc.CASES, ids=sc.IDS)
def test_axpy_cpu_meets_the_oracle(case):
    """fp32 in logical order: the forward within 8 u32 A, dx within 4 u32 |ref|, da within
    1.01 (M + 1) u32 S (the bounds of se_cases without their bf16 terms), dy exactly dtop."""
    for image_gate in (False, True):
        top, (da, dx, dy) = run_axpy(case, image_gate=image_gate)
        assert sc.worst(top, *sc.forward_bound(case, use=("s", "r"), fp32=True)) <= 1.0
        bx, ba, _ = sc.backward_bound(case, fp32=True)
        assert sc.worst(dx, *bx) <= 1.0 and sc.worst(da, *ba) <= 1.0
        assert torch.equal(dy, sc.inputs(case)["dy"].float())


def test_axpy_finite_difference_gradient():
    inp, txt = _axpy_text((2, 3), (2, 3, 4, 5))
    check_layer(txt, {"a": (2, 3), "x": (2, 3, 4, 5), "y": (2, 3, 4, 5)})
    check_layer(txt, {"a": (2, 3, 1, 1), "x": (2, 3, 4, 5), "y": (2, 3, 4, 5)})


@pytest.mark.parametrize("propagate", [(True, False, False), (False, True, False), (False, False, True),
                                       (False, False, False)])
def test_axpy_honours_propagate_down(propagate):
    case = sc.CASES[3]
    _, ref = run_axpy(case)
    _, got = run_axpy(case, propagate=propagate)  # asserts that the others are untouched
    for g, r, p in zip(got, ref, propagate):
        assert not p or torch.equal(g, r)


@pytest.mark.parametrize("a, x, y", [((2, 4), (2, 3, 4, 5), None), ((3, 3), (2, 3, 4, 5), None),
                                     ((2, 3, 1), (2, 3, 4, 5), None), ((2, 3, 4, 5), (2, 3, 4, 5), None),
                                     ((2, 3), (2, 3, 4, 5), (2, 3, 5, 4)), ((2, 3), (2, 3, 4), (2, 3, 4))])
def test_axpy_rejects_mismatched_shapes(a, x, y):
    inp, txt = _axpy_text(a, x, y)
    with pytest.raises(ValueError, match="Axpy 'L'"):
        Net(proto.parse_prototxt(f'name: "g"\n{inp}{txt}'), phase=proto.TRAIN)


def test_axpy_takes_exactly_three_bottoms():
    inp, _ = _axpy_text((2, 3), (2, 3, 4, 5))
    with pytest.raises(ValueError, match="Axpy"):
        Net(proto.parse_prototxt(f'name: "g"\n{inp}layer {{ name: "L" type: "Axpy" bottom: "a" bottom: "x" top: "t" }}'),
            phase=proto.TRAIN)


def test_registry_and_dsl():
    assert "Axpy" in layer_types()
    ax = dsl.AxpyLayer("res2a", ["gate", "x", "short"])
    assert (ax.type, list(ax.bottom), list(ax.top)) == ("Axpy", ["gate", "x", "short"], ["res2a"])
    sg = dsl.SigmoidLayer("gate", ["up"])
    assert (sg.type, list(sg.bottom), list(sg.top)) == ("Sigmoid", ["up"], ["gate"])
    assert list(dsl.SigmoidLayer("s", ["up"], in_place=True).top) == ["up"]
    net = Net(dsl.NetParam("n", dsl.RDDLayer("up", [2, 4, 1, 1]), dsl.RDDLayer("x", [2, 4, 3, 3]),
                           dsl.RDDLayer("short", [2, 4, 3, 3]), sg, ax), phase=proto.TRAIN)
    net.blob_by_name("x").set_nchw(torch.ones(2, 4, 3, 3))
    net.forward()
    assert torch.equal(net.blob_by_name("res2a").nchw(), torch.full((2, 4, 3, 3), 0.5))  # sigmoid(0) * 1 + 0


# --- the (N, C) route of Scale / Bias --------------------------------------------------------------

def _plan_of(typ, shape, ptxt, s1=None):
    dims = lambda s: " ".join(f"dim: {d}" for d in s)
    inp = "".join(f'layer {{ name: "in_{n}" type: "Input" top: "{n}" java_data_param {{ shape {{ {dims(s)} }} }} }}\n'
                  for n, s in (("x", shape), ("s", s1)) if s is not None)
    pname = "scale_param" if typ == "Scale" else "bias_param"
    bottoms = 'bottom: "x"' + (' bottom: "s"' if s1 is not None else "")
    net = Net(proto.parse_prototxt(f'name: "g"\n{inp}layer {{ name: "L" type: "{typ}" {bottoms} top: "y" '
                                   f'{pname} {{ {ptxt} }} }}'), phase=proto.TRAIN)
    return net.layers[-1]


ROUTES = [  # type, bottom[0], param text, bottom[1], on the (N, C) route?
    ("Scale", (2, 3, 4, 5), "axis: 0 num_axes: 2", None, True),
    ("Scale", (2, 3, 4, 5), "axis: 0 num_axes: 2 bias_term: true", None, True),
    ("Scale", (2, 3, 4, 5), "axis: 0", (2, 3), True),
    ("Bias", (2, 3, 4, 5), "axis: 0 num_axes: 2", None, True),
    ("Bias", (2, 3, 4, 5), "axis: 0", (2, 3), True),
    ("Scale", (2, 3, 4, 5), "axis: -4 num_axes: 2", None, True),
    ("Scale", (2, 3, 4, 5), "axis: 0 num_axes: 3", None, False),   # (N, C, H): NCHW copy
    ("Scale", (2, 3, 4, 5), "axis: 1 num_axes: 2", None, False),   # (C, H): NCHW copy
    ("Scale", (2, 3, 4, 5), "axis: 0 num_axes: 1", None, False),   # (N): one decomposition of the storage
    ("Scale", (2, 3, 4, 5), "axis: 1", None, False),               # per channel
    ("Scale", (2, 3, 4, 5), "axis: 0 num_axes: -1", None, False),
    ("Scale", (2, 3, 4), "axis: 0 num_axes: 2", None, False),      # not an image blob
    ("Scale", (2, 3), "axis: 0 num_axes: 2", None, False),
    ("Bias", (2, 3, 4, 5), "axis: 1 num_axes: 2", None, False),
]


@pytest.mark.parametrize("typ, shape, ptxt, s1, nc", ROUTES)
def test_plan_routes(monkeypatch, typ, shape, ptxt, s1, nc):
    monkeypatch.delenv("SN_FEATURES", raising=False)
    layer = _plan_of(typ, shape, ptxt, s1)
    assert layer.nc is nc
    if nc:  # Caffe order and storage order of (N, C) coincide: no permute; the fall-back stays the NCHW copy
        assert layer.phys is None and layer.perm == [0, 1] and layer.cshape == shape[:2]
        assert all(p.shape == p.caffe_shape == shape[:2] for p in layer.params)
    monkeypatch.setenv("SN_FEATURES", "se_kernels=0")
    assert _plan_of(typ, shape, ptxt, s1).nc is False


def test_gap_route_predicate(monkeypatch):
    """The Pooling route: AVE over the whole unpadded image, bf16, more than 64 positions."""
    from sparknet_amd.ops.hip import gap_ok
    from sparknet_amd.ops.spec import POOL_AVE, POOL_MAX, PoolSpec
    monkeypatch.delenv("SN_FEATURES", raising=False)
    x = torch.empty(0, dtype=torch.bfloat16)
    glob = lambda H, W, method=POOL_AVE, **kw: PoolSpec(2, H, W, 8, kw.pop("kh", H), kw.pop("kw", W), 1, 1,
                                                        kw.pop("ph", 0), kw.pop("pw", 0), method)
    assert gap_ok(glob(65, 1), x) and gap_ok(glob(9, 8), x) and gap_ok(glob(56, 56), x)
    assert not gap_ok(glob(8, 8), x) and not gap_ok(glob(7, 7), x) and not gap_ok(glob(1, 1), x)
    assert not gap_ok(glob(9, 8, POOL_MAX), x)
    assert not gap_ok(glob(9, 8, kh=3, kw=3), x) and not gap_ok(glob(9, 8, kh=9, kw=4), x)
    assert not gap_ok(glob(9, 8, ph=1), x)
    assert not gap_ok(glob(9, 8), x.float()) and not gap_ok(glob(9, 8), x, side=object())
    for c in sc.CASES:  # the cases sit where they claim: one at 64 positions, the next at 65
        assert gap_ok(glob(c[1], c[2]), x) == (c[1] * c[2] > 64)
    assert sc.HW64[1] * sc.HW64[2] == 64 and sc.HW65[1] * sc.HW65[2] == 65
    monkeypatch.setenv("SN_FEATURES", "se_kernels=0")
    assert not gap_ok(glob(65, 1), x)


# --- zoo ------------------------------------------------------------------------------------------

SMALL = dict(reps=(1, 1, 1, 1), crop=32, classes=10)


def _learnable_from_shapes(reps=(3, 4, 6, 3), reduction=16):
    se = sum(r * (2 * c * c // reduction + c // reduction + c) for r, c in zip(reps, (256, 512, 1024, 2048)))
    return 25557032 + se


def test_se_resnet50_builds():
    assert _learnable_from_shapes() == 28088024
    B = 1
    for phase in (proto.TRAIN, proto.TEST):
        net = Net(models.se_resnet50(train_batch=B, test_batch=B), phase=phase, device="cpu")
        learnable = sum(p.data.numel() for l in net.layers if l.type_name != "BatchNorm" for p in l.params)
        assert learnable == 28088024
        plain = Net(models.resnet50(train_batch=B, test_batch=B), phase=phase, device="cpu")
        tops = {b.name: b.shape for vec in plain.top_vecs for b in vec if "_split" not in b.name}
        assert len(tops) > 60
        for name, shape in tops.items():  # every top of ResNet-50 is there, with its shape
            assert net.blob_by_name(name).shape == shape, name
        kinds = [l.type_name for l in net.layers]
        assert kinds.count("Axpy") == 16 and kinds.count("Sigmoid") == 16 and kinds.count("Eltwise") == 0
        assert kinds.count("Pooling") == 2 + 16 and kinds.count("Convolution") == 53 + 32
        assert net.blob_by_name("res2a_se_pool").shape == (B, 256, 1, 1)
        assert net.blob_by_name("res2a_se_down").shape == (B, 16, 1, 1)
        assert net.blob_by_name("res5c_se_gate").shape == (B, 2048, 1, 1)
        ax = next(l for l in net.layers if l.name == "res3b")
        assert list(ax.lp.bottom)[:1] == ["res3b_se_gate"] and ax.type_name == "Axpy"
    assert "se_resnet50" in models.MODELS and models.MODELS["se_resnet50"][1]().weight_decay == pytest.approx(1e-4)
    assert models.se_resnet is models.zoo.se_resnet


def _small_batch(B, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, 32, 32, generator=g), torch.randint(0, 10, (B, 1), generator=g).float()


def test_small_se_resnet_survives_the_proto_round_trip():
    """The definition through text into a second Net; the first net's to_proto() (its layers with
    their blobs; Net.to_proto leaves out the Split layers it inserted, so it is read as a weights
    file, as for every zoo model) into that Net's layers, and its layer definitions through text
    (without the 8 M weights, which would take minutes as text)."""
    B = 2
    param = models.se_resnet(train_batch=B, test_batch=B, **SMALL)
    net = Net(param, phase=proto.TEST, device="cpu", seed=4)
    back = Net(proto.parse_prototxt(proto.to_prototxt(param)), phase=proto.TEST, device="cpu", seed=9)
    assert [(l.type_name, l.name) for l in back.layers] == [(l.type_name, l.name) for l in net.layers]
    assert not torch.equal(back.flat_data, net.flat_data)
    saved = net.to_proto()
    assert sum(l.type == "Axpy" and not l.blobs for l in saved.layer) == 4
    back.copy_trained_layers_from(saved)
    assert torch.equal(back.flat_data, net.flat_data)
    for lp in saved.layer:
        del lp.blobs[:]
    assert proto.parse_prototxt(proto.to_prototxt(saved)) == saved
    data, label = _small_batch(B)
    out = []
    for n in (net, back):
        n.blob_by_name("data").set_nchw(data)
        n.blob_by_name("label").set_nchw(label)
        n.forward()
        out.append(n.blob_by_name("fc10").data.clone())
    assert torch.equal(out[0], out[1])


def test_small_se_resnet_cpu_solver_step():
    from sparknet_amd.core.solver import Solver
    from sparknet_amd.models import zoo
    B = 4
    sp = zoo.se_resnet50_solver(models.se_resnet(train_batch=B, test_batch=B, **SMALL))
    solver = Solver(sp, device=torch.device("cpu"), seed=3, build_test_nets=False)
    data, label = _small_batch(B)
    solver.net.blob_by_name("data").set_nchw(data)
    solver.net.blob_by_name("label").set_nchw(label)
    w0 = solver.net.flat_data.detach().clone()
    solver.stage_hyper()
    loss = float(solver.iteration())
    assert loss == loss and abs(loss) < 1e3, loss
    assert not torch.equal(w0, solver.net.flat_data)
    gate = next(l for l in solver.net.layers if l.name == "res2a_se_up")
    assert float(gate.params[0].diff.abs().max()) > 0  # the gradient reaches the SE products through the Axpy
