"""The fused BatchNorm -> Scale -> ReLU kernels (csrc/kernels/bn_scale.hip) against the fp32 CPU
chain of three layers: through the layer triple with engine.fuse_bn_scale_relu applied, and
directly through the ops.layers_hip wrappers.

Shapes (N, C, H, W), the smallest that reach each code path: (2,3,7,7) scalar tail, one slab;
(2,20,5,3) tail with C % 8 != 0; (4,136,6,6) vector path with C % 64 != 0; (8,64,28,28) several
row slabs, so the slab merge runs; (16,10) 2-D.  Inputs are bf16-representable.  Bounds: 3e-2
(max-abs error over max-abs reference, the metric of tests/test_layers_gpu.py) for tops, dx,
dgamma, dbeta and the running statistics.  dx is compared where the CPU pre-activation has
|z| > 1e-3 (a bf16 top may round a ReLU gate the other way next to 0); the excluded share is
asserted <= 1 % (it is <= 0.08 % for these inputs, so the cap constrains the inputs only)."""
import itertools

import pytest
import torch

from sparknet_amd import engine
from test_bn_scale_chain import EPS, FACTOR, chain_inputs, chain_text, rel, run_chain

pytestmark = pytest.mark.gpu

TOL = 3e-2
SHAPES = [(2, 3, 7, 7), (2, 20, 5, 3), (4, 136, 6, 6), (8, 64, 28, 28), (16, 10)]
_CPU = {}


def cpu_chain(shape, **kw):
    """CPU engine result of one variant, computed once and shared between tests."""
    key = (shape, tuple(sorted(kw.items())))
    if key not in _CPU:
        out = run_chain("cpu", shape, **kw)
        out.pop("net")
        _CPU[key] = out
    return _CPU[key]


def gate_mask(shape, relu, bias_term, global_stats):
    if not relu:
        return None
    z = cpu_chain(shape, relu=False, bias_term=bias_term, global_stats=global_stats)["top"]
    mask = z.abs() > 1e-3
    assert 1.0 - mask.float().mean().item() <= 0.01
    return mask


def check(got, ref, mask=None, running=True):
    assert rel(got["top"], ref["top"]) < TOL, ("top", rel(got["top"], ref["top"]))
    if ref["dx"] is not None:
        a, b = got["dx"], ref["dx"]
        if mask is not None:
            a, b = a[mask], b[mask]
        assert rel(a, b) < TOL, ("dx", rel(a, b))
    for key in ("dgamma", "dbeta"):
        if ref[key] is not None:
            assert rel(got[key], ref[key]) < TOL, (key, rel(got[key], ref[key]))
    if running:
        for a, b in zip(got["running"], ref["running"]):
            assert rel(a, b) < TOL, ("running", rel(a, b))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("relu,bias_term,global_stats,bn_inplace", list(itertools.product([True, False], repeat=4)))
def test_fused_chain_matches_cpu(gpu, shape, relu, bias_term, global_stats, bn_inplace):
    kw = dict(relu=relu, bias_term=bias_term, global_stats=global_stats)
    got = run_chain("cuda", shape, bn_inplace=bn_inplace, fuse=True, **kw)
    assert got["fused"] == 1
    net = got["net"]
    bn, sc = net.layers[net.layer_names.index("bn")], net.layers[net.layer_names.index("sc")]
    assert bn.fused_scale is sc and sc.fused_into is bn and bn.fused_relu == relu
    check(got, cpu_chain(shape, **kw), gate_mask(shape, **kw))


@pytest.mark.parametrize("shape", [(2, 20, 5, 3), (8, 64, 28, 28)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("global_stats", [False, True])
def test_param_diffs_only(gpu, shape, global_stats):
    """propagate_down false: no bottom diff is produced, the param diffs are the same."""
    got = run_chain("cuda", shape, global_stats=global_stats, propagate=False, fuse=True)
    assert got["fused"] == 1 and got["dx"] is None
    check(got, cpu_chain(shape, global_stats=global_stats, propagate=False))


@pytest.mark.parametrize("shape", [(2, 3, 7, 7), (8, 64, 28, 28)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("grads", ["acc", "lazy"])
def test_param_gradient_accumulate_and_overwrite(gpu, shape, grads):
    """"acc": diffs start at 1 and are accumulated into; "lazy": the buffer holds garbage after
    Net.clear_param_diffs(lazy=True) and the first write stores."""
    got = run_chain("cuda", shape, grads=grads, fuse=True)
    ref = cpu_chain(shape, grads=grads)
    base = cpu_chain(shape)
    off = 1.0 if grads == "acc" else 0.0
    for key in ("dgamma", "dbeta"):  # the CPU engine itself honours both forms
        assert rel(ref[key], base[key] + off) < 1e-5
    check(got, ref, gate_mask(shape, True, True, False))


@pytest.mark.parametrize("shape", [(4, 136, 6, 6), (8, 64, 28, 28)], ids=lambda s: "x".join(map(str, s)))
def test_deterministic(gpu, shape):
    a, b = run_chain("cuda", shape, fuse=True), run_chain("cuda", shape, fuse=True)
    for key in ("top", "dx", "dgamma", "dbeta"):
        assert torch.equal(a[key], b[key]), key
    assert all(torch.equal(x, y) for x, y in zip(a["running"], b["running"]))


@pytest.mark.parametrize("shape", [(4, 136, 6, 6), (16, 10)], ids=lambda s: "x".join(map(str, s)))
def test_pass_on_and_off(gpu, shape, monkeypatch):
    """SN_FEATURES=fuse_bn_scale=0 runs the same net through the three layers."""
    on = run_chain("cuda", shape, fuse=True)
    monkeypatch.setenv("SN_FEATURES", "fuse_bn_scale=0")
    off = run_chain("cuda", shape, fuse=True)
    assert on["fused"] == 1 and off["fused"] == 0
    net = off["net"]
    assert net.layers[net.layer_names.index("bn")].fused_scale is None
    ref = cpu_chain(shape)
    mask = gate_mask(shape, True, True, False)
    check(off, ref, mask)
    check(on, off, mask)


def test_fuse_relu_calls_the_pass_and_marks_the_relu(gpu):
    """engine.fuse_relu runs the pass before fuse_relu_backward; the folded ReLU is marked like
    the fused ReLUs there, so the consumer does not gate a second time."""
    from sparknet_amd import models, proto
    from sparknet_amd.core.net import Net
    net = Net(models.resnet_cifar(n=1, train_batch=2, test_batch=2), phase=proto.TRAIN, device="cuda")
    engine.fuse_relu(net)
    bns = [l for l in net.layers if l.type_name == "BatchNorm"]
    assert net.bn_scale_fused == len(bns) == 9 and all(l.fused_scale is not None for l in bns)
    for li, layer in enumerate(net.layers):
        if layer.type_name == "ReLU" and getattr(layer, "bn_fused", False):
            assert layer.fused and layer.bwd_fused
            blob = net.top_ids[li][0]
            readers = [net.layers[lj] for lj in range(li + 1, len(net.layers)) if blob in net.bottom_ids[lj]]
            assert not any(getattr(r, "relu_gate", False) for r in readers)
    cpu = Net(models.resnet_cifar(n=1, train_batch=2, test_batch=2), phase=proto.TRAIN, device="cpu")
    engine.fuse_relu(cpu)
    assert cpu.bn_scale_fused == 0 and all(l.fused_scale is None for l in cpu.layers if l.type_name == "BatchNorm")


REJECTS = {
    "scale_not_in_place": 'layer { name: "sc" type: "Scale" bottom: "y" top: "w" scale_param { bias_term: true } }',
    "scale_two_bottoms": 'layer { name: "sc" type: "Scale" bottom: "y" bottom: "g" top: "y" scale_param { axis: 1 } }',
    "scale_other_axis": 'layer { name: "sc" type: "Scale" bottom: "y" top: "y" scale_param { axis: 2 } }',
    # A second reader of the BatchNorm top makes an in-place Scale on it an invalid net (the blob
    # would have two producers after the split), so a reader between the layers of the pattern
    # always comes with a Scale that is not in place ...
    "reader_in_between": ('layer { name: "tap" type: "Power" bottom: "y" top: "t" }\n'
                          'layer { name: "sc" type: "Scale" bottom: "y" top: "w" scale_param { bias_term: true } }'),
    # ... and a layer between the two that reads another blob breaks the adjacency
    "layer_in_between": ('layer { name: "tap" type: "Power" bottom: "x" top: "t" }\n'
                         'layer { name: "sc" type: "Scale" bottom: "y" top: "y" scale_param { bias_term: true } }'),
}


@pytest.mark.parametrize("case", sorted(REJECTS))
def test_pass_rejects(gpu, case):
    from sparknet_amd import proto
    from sparknet_amd.core.net import Net
    shape = (2, 8, 3, 3)
    text = chain_text(shape, scale_txt=REJECTS[case], relu=case in ("scale_two_bottoms", "scale_other_axis"))
    if case == "scale_two_bottoms":
        text = text.replace('layer { name: "bn"', 'layer { name: "in_g" type: "Input" top: "g" java_data_param '
                            '{ shape { dim: 8 } } }\nlayer { name: "bn"', 1)
    net = Net(proto.parse_prototxt(text), phase=proto.TRAIN, device="cuda")
    assert engine.fuse_bn_scale_relu(net) == 0
    assert all(getattr(l, "fused_scale", None) is None and getattr(l, "fused_into", None) is None
               for l in net.layers)
    net.forward()  # the unfused layers still run


def test_pass_skips_debug_info(gpu):
    from sparknet_amd import proto
    from sparknet_amd.core.net import Net
    net = Net(proto.parse_prototxt(chain_text((2, 8, 3, 3)) + "debug_info: true\n"), phase=proto.TRAIN, device="cuda")
    assert engine.fuse_bn_scale_relu(net) == 0


# -- the wrappers, called directly -----------------------------------------------------------
def _direct(shape, dtype, relu, global_stats, large_mean=False):
    from sparknet_amd.ops import layers_hip as lh
    inp = chain_inputs(shape, large_mean=large_mean)
    C_ = shape[1]
    phys = (lambda t: t.permute(0, 2, 3, 1).contiguous()) if len(shape) == 4 else (lambda t: t)
    x, dy = phys(inp["x"]).to("cuda", dtype), phys(inp["dy"]).to("cuda", dtype)
    R = x.numel() // C_
    gamma, beta = inp["gamma"].cuda(), inp["beta"].cuda()
    if large_mean:
        gamma, beta = torch.ones_like(gamma), torch.zeros_like(beta)
    rm, rv, rf = inp["rmean"].cuda(), inp["rvar"].cuda(), torch.full((1,), FACTOR, device="cuda")
    if global_stats:
        stats = (lh.BN_GLOBAL, rm, rv, rf, EPS)
    else:
        rm, rv, rf = torch.zeros_like(rm), torch.zeros_like(rv), torch.zeros_like(rf)
        mean, var, inv = lh.bn_stats(x, R, C_, EPS, (rm, rv, rf), 0.999, R / max(R - 1, 1))
        stats = (lh.BN_BATCH, mean, inv, None, EPS)
    y = lh.bn_fwd(x, R, C_, stats, gamma, beta, relu)
    dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
    coef = lh.bn_bwd_reduce(dy, x, y, R, C_, stats, relu, dgamma, lh.GRAD_STORE, dbeta, lh.GRAD_STORE)
    dx = lh.bn_bwd_dx(dy, x, y, R, C_, stats, relu, gamma, coef)
    torch.cuda.synchronize()
    logical = (lambda t: t.float().cpu().permute(0, 3, 1, 2)) if len(shape) == 4 else (lambda t: t.float().cpu())
    return dict(top=logical(y), dx=logical(dx), dgamma=dgamma.cpu(), dbeta=dbeta.cpu(),
                running=[rm.cpu(), rv.cpu(), rf.cpu()])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("relu,global_stats", [(True, False), (False, True)])
def test_wrappers_match_cpu(gpu, shape, dtype, relu, global_stats):
    kw = dict(relu=relu, bias_term=True, global_stats=global_stats)
    got = _direct(shape, dtype, relu, global_stats)
    # fp32 tensors: the fp32 device-mode bound where no ReLU gate is involved
    ref = cpu_chain(shape, **kw)
    check(got, ref, gate_mask(shape, **kw))
    if dtype == torch.float32 and not relu:
        for key in ("top", "dx", "dgamma", "dbeta"):
            assert rel(got[key], ref[key]) < 1e-3, (key, rel(got[key], ref[key]))


def test_wrappers_deterministic(gpu):
    a, b = (_direct((8, 64, 28, 28), torch.bfloat16, True, False) for _ in range(2))
    for key in ("top", "dx", "dgamma", "dbeta"):
        assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize("shape,dtype", [((64, 5), torch.float32), ((8, 64, 4, 4), torch.bfloat16)],
                         ids=["64x5-fp32", "8x64x4x4-bf16"])
def test_large_mean(gpu, shape, dtype):
    """x = 1000 + randn: the Welford partials and their merge keep the variance (E[x^2] - EX^2
    would cancel in fp32); the output with gamma 1, beta 0 and no ReLU has unit variance."""
    y = _direct(shape, dtype, False, False, large_mean=True)["top"]
    dims = [d for d in range(len(shape)) if d != 1]
    var = y.var(dim=dims, unbiased=False)
    assert (var - 1.0).abs().max().item() < 0.05, var
