"""The depthwise 3x3 kernels (csrc/kernels/conv_dw.hip) through ``hip.conv_forward`` and
``hip.conv_backward``, held elementwise to the fp64 oracle and the derived bounds of
tests/conv_dw_cases.py on every case; which launches are used (a spy on the kernel call), the
``conv_depthwise=0`` path as the reference point, determinism, the misaligned fall-back, and a
tiny net through ``fuse_relu`` against the fp32 CPU engine."""
import contextlib
import os

import pytest
import torch

import conv_dw_cases as dc

pytestmark = pytest.mark.gpu

DW_KERNELS = {"conv_dw_fwd", "conv_dw_wgrad", "conv_dw_dgrad"}


@contextlib.contextmanager
def features(value):
    old = os.environ.get("SN_FEATURES")
    if value is None:
        os.environ.pop("SN_FEATURES", None)
    else:
        os.environ["SN_FEATURES"] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SN_FEATURES", None)
        else:
            os.environ["SN_FEATURES"] = old


@pytest.fixture
def spy(gpu, monkeypatch):
    """Names of the native launches ops/hip.py makes, in order."""
    from sparknet_amd.ops import _lib, hip
    names = []

    def call(name, *args):
        names.append(name)
        return _lib.call(name, *args)
    monkeypatch.setattr(hip, "call", call)
    return names


def _dev(case, gpu):
    return {k: v.to(gpu) for k, v in dc.inputs(case).items()}


def _grads(s, gpu, fill=dc.PREFILL):
    return (torch.full((s.C, 3, 3, 1), fill, dtype=torch.float32, device=gpu),
            torch.full((s.C,), fill, dtype=torch.float32, device=gpu))


def _check_forward(case, gpu, hip):
    i, s = _dev(case, gpu), dc.spec(case)
    for bias in (True, False):
        for relu in (True, False):
            y = hip.conv_forward(i["x"], i["w"], i["bias"] if bias else None, s, relu=relu)
            assert tuple(y.shape) == (s.N, s.P, s.Q, s.C) and y.dtype == torch.bfloat16
            r = dc.worst(y, *dc.forward_bound(case, bias, relu))
            print("forward", case, "bias", bias, "relu", relu, "worst / bound", r)
            assert r <= 1.0, (bias, relu, r)


def _check_backward(case, gpu, hip):
    """gate on + store onto 7.0; gate off + accumulate onto 7.0; need_dx False with db None;
    dw None with the bias gradient alone."""
    i, s = _dev(case, gpu), dc.spec(case)
    for gate, acc in ((True, False), (False, True)):
        dw, db = _grads(s, gpu)
        dx = hip.conv_backward(i["dy"], i["x"], i["w"], s, True, dw, db, i["gate"] if gate else None,
                               dw_acc=acc, db_acc=acc)
        assert tuple(dx.shape) == (s.N, s.H, s.W, s.C) and dx.dtype == torch.bfloat16
        bw, bb = dc.wgrad_bound(case, dc.PREFILL if acc else None)
        r = (dc.worst(dx, *dc.dgrad_bound(case, gate)), dc.worst(dw, *bw), dc.worst(db, *bb))
        print("backward", case, "gate", gate, "acc", acc, "worst / bound (dx, dw, db)", r)
        assert max(r) <= 1.0, (gate, acc, r)
    dw, _ = _grads(s, gpu)
    assert hip.conv_backward(i["dy"], i["x"], i["w"], s, False, dw, None, None, dw_acc=False) is None
    r = dc.worst(dw, *dc.wgrad_bound(case)[0])
    assert r <= 1.0, ("need_dx False, db None", r)
    _, db = _grads(s, gpu)
    hip.conv_backward(i["dy"], i["x"], i["w"], s, False, None, db, None, db_acc=False)
    r = dc.worst(db, *dc.wgrad_bound(case)[1])
    assert r <= 1.0, ("dw None", r)


@pytest.mark.parametrize("case", dc.CASES, ids=dc.IDS)
def test_forward(case, gpu, spy):
    from sparknet_amd.ops import hip
    with features(None):
        _check_forward(case, gpu, hip)
    assert spy == ["conv_dw_fwd"] * 4, spy


@pytest.mark.parametrize("case", dc.CASES, ids=dc.IDS)
def test_backward(case, gpu, spy):
    from sparknet_amd.ops import hip
    with features(None):
        _check_backward(case, gpu, hip)
    assert spy == ["conv_dw_wgrad", "conv_dw_dgrad"] * 2 + ["conv_dw_wgrad"] * 2, spy


@pytest.mark.parametrize("case", dc.CASES, ids=dc.IDS)
def test_switch_off_is_the_per_group_path_and_meets_the_bounds(case, gpu, spy):
    """SN_FEATURES=conv_depthwise=0: one im2col + GEMM per group, the reference point of the new
    kernels.  Its data gradient meets the bound because dcol = dy_g W_g stays fp32 until col2im
    has summed the taps; with a bf16 dcol every tap product was rounded before the sum, and where
    the taps cancel the result was 19 to 1300 times the bound on eight of these cases."""
    from sparknet_amd.ops import hip
    with features("conv_depthwise=0"):
        _check_forward(case, gpu, hip)
        _check_backward(case, gpu, hip)
    assert spy and not DW_KERNELS & set(spy), sorted(set(spy))
    assert "im2col" in spy and "col2im" in spy


def test_weight_gradient_is_bitwise_reproducible(gpu, spy):
    from sparknet_amd.ops import hip
    case = dc.LARGEST
    i, s = _dev(case, gpu), dc.spec(case)
    runs = []
    with features(None):
        for _ in range(2):
            dw, db = _grads(s, gpu)
            hip.conv_backward(i["dy"], i["x"], i["w"], s, False, dw, db, None, dw_acc=False, db_acc=False)
            runs.append((dw.clone(), db.clone()))
    assert spy == ["conv_dw_wgrad"] * 2
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # several slabs of partials went into that sum
    from sparknet_amd.ops import _lib
    k = _lib.kernels()
    k.sn_conv_dw_part_floats.restype = _lib.C.c_longlong
    n = int(k.sn_conv_dw_part_floats(*(_lib.C.c_longlong(v) for v in (s.N, s.P, s.Q, s.C))))
    assert n % (10 * s.C) == 0 and n // (10 * s.C) > 1, n


def test_misaligned_view_falls_back_and_is_correct(gpu, spy):
    """A contiguous view at a storage offset of 2 elements starts 4 bytes into a 16-byte lane."""
    from sparknet_amd.ops import hip
    case = dc.CASES[2]
    i, s = _dev(case, gpu), dc.spec(case)
    buf = torch.zeros(i["x"].numel() + 8, dtype=torch.bfloat16, device=gpu)
    assert buf.data_ptr() % 16 == 0
    x = buf[2:2 + i["x"].numel()].view(i["x"].shape)
    x.copy_(i["x"])
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    with features(None):
        y = hip.conv_forward(x, i["w"], i["bias"], s, relu=False)
        dw, db = _grads(s, gpu)
        dx = hip.conv_backward(i["dy"], x, i["w"], s, True, dw, db, i["gate"], dw_acc=False, db_acc=False)
    assert "conv_dw_fwd" not in spy and "conv_dw_wgrad" not in spy, spy
    assert spy.count("conv_dw_dgrad") == 1  # dy, w, gate and dx are aligned
    bw, bb = dc.wgrad_bound(case)
    r = (dc.worst(y, *dc.forward_bound(case, True, False)), dc.worst(dx, *dc.dgrad_bound(case, True)),
         dc.worst(dw, *bw), dc.worst(db, *bb))
    print("misaligned: worst / bound (y, dx, dw, db)", r)
    assert max(r) <= 1.0, r


# --- a tiny net through fuse_relu: the ReLU epilogue of the forward and relu_gate of the dgrad -------

B = 4


def _tiny_solver(dev, w0=None):
    from sparknet_amd.core.solver import Solver
    from sparknet_amd.dsl import ConvolutionLayer, InnerProductLayer, NetParam, ReLULayer, SoftmaxWithLoss
    from sparknet_amd.engine import fuse_relu
    from sparknet_amd.models import zoo
    g = {"type": "gaussian", "std": 0.3}
    c = {"type": "constant", "value": 0.1}
    conv = lambda name, bottom, k, n, **kw: ConvolutionLayer(name, [bottom], (k, k), n, weight_filler=g,
                                                             bias_filler=c, **kw)
    net = NetParam("tiny_dw", *zoo.data_layers(B, B, 8, 8, 8),
                   conv("pw", "data", 1, 16), ReLULayer("relu_pw", ["pw"], in_place=True),
                   conv("dw1", "pw", 3, 16, pad=1, group=16), ReLULayer("relu_dw1", ["dw1"], in_place=True),
                   conv("dw2", "dw1", 3, 16, stride=2, pad=1, group=16), ReLULayer("relu_dw2", ["dw2"], in_place=True),
                   InnerProductLayer("ip", ["dw2"], 10, weight_filler=g, bias_filler=c),
                   SoftmaxWithLoss("loss", ["ip", "label"]))
    sp = zoo._solver(net, base_lr=0.05, lr_policy="fixed", momentum=0.9, weight_decay=1e-4, max_iter=10, display=0)
    solver = Solver(sp, device=torch.device(dev), seed=11, build_test_nets=False)
    if w0 is not None:
        solver.net.flat_data.copy_(w0.to(solver.net.flat_data.device))
        solver.net.sync_compute()
    if solver.net.device.type == "cuda":
        fuse_relu(solver.net)
    return solver


def _one_step(solver):
    """{param name: its one-step update}"""
    g = torch.Generator().manual_seed(21)
    net = solver.net
    net.blob_by_name("data").set_nchw(torch.randn(B, 8, 8, 8, generator=g))
    net.blob_by_name("label").set_nchw(torch.randint(0, 10, (B, 1), generator=g).float())
    before = net.flat_data.detach().float().cpu().clone()
    solver.stage_hyper()
    loss = float(solver.iteration())
    assert loss == loss
    after = net.flat_data.detach().float().cpu()
    out = {}
    for layer in net.layers:
        for j, p in enumerate(layer.params):
            out[f"{layer.name}[{j}]"] = (after - before)[p.offset:p.offset + p.count].double()
    return out


def test_tiny_net_update_no_worse_than_the_path_it_replaces(gpu, spy):
    """One solver step from the same weights: per parameter, the relative L2 error of the update
    against the fp32 CPU engine is at most max(1.5 x the conv_depthwise=0 path's, 1e-3)."""
    cpu = _tiny_solver("cpu")
    w0 = cpu.net.flat_data.detach().clone()
    ref = _one_step(cpu)
    with features(None):
        solver = _tiny_solver(gpu, w0)
        convs = {l.name: l for l in solver.net.layers if l.type_name == "Convolution"}
        assert all(l.fuse_relu for l in convs.values()) and convs["dw1"].relu_gate and convs["dw2"].relu_gate
        new = _one_step(solver)
    assert spy.count("conv_dw_fwd") == 2 and spy.count("conv_dw_wgrad") == 2 and spy.count("conv_dw_dgrad") == 2, spy
    del spy[:]
    with features("conv_depthwise=0"):
        old = _one_step(_tiny_solver(gpu, w0))
    assert not DW_KERNELS & set(spy)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    assert len(ref) == 8
    for name, r in ref.items():
        assert float(r.norm()) > 0, name
        e_new, e_old = rel(new[name], r), rel(old[name], r)
        print(name, "relative L2 error of the update: new", e_new, "conv_depthwise=0", e_old)
        assert e_new <= max(1.5 * e_old, 1e-3), (name, e_new, e_old)
