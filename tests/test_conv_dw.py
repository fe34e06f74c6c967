"""Depthwise 3x3 convolution, CPU side (tests/test_conv_dw_gpu.py holds the HIP kernels to the
same oracle and bounds; tests/conv_dw_cases.py has them): the bounds admit a correct fp32
implementation (ops.ref), every mutant of the oracle violates them by at least 10x, the
dispatch predicate, and the MobileNet zoo model."""
import pytest
import torch

import conv_dw_cases as dc
from sparknet_amd import models, proto
from sparknet_amd.ops import ref
from sparknet_amd.ops.spec import ConvSpec


@pytest.mark.parametrize("case", dc.CASES, ids=dc.IDS)
def test_bounds_admit_the_fp32_reference(case):
    i, s = dc.inputs(case), dc.spec(case)
    for bias in (True, False):
        for relu in (True, False):
            y = ref.conv_forward(i["x"], i["w"], i["bias"] if bias else None, s, relu=relu)
            assert y.dtype == torch.bfloat16
            assert dc.worst(y, *dc.forward_bound(case, bias, relu)) <= 1.0, (bias, relu)
    for gate, prefill in ((True, None), (False, dc.PREFILL)):
        dw = torch.full((s.C, 3, 3, 1), dc.PREFILL)
        db = torch.full((s.C,), dc.PREFILL)
        dx = ref.conv_backward(i["dy"], i["x"], i["w"], s, True, dw, db, i["gate"] if gate else None,
                               dw_acc=prefill is not None, db_acc=prefill is not None)
        assert dc.worst(dx, *dc.dgrad_bound(case, gate)) <= 1.0
        bw, bb = dc.wgrad_bound(case, prefill)
        assert dc.worst(dw, *bw) <= 1.0 and dc.worst(db, *bb) <= 1.0, prefill


def _overlap(a, b):
    p, q = min(a.shape[1], b.shape[1]), min(a.shape[2], b.shape[2])
    return a[:, :p, :q], b[:, :p, :q]


def _forward_mutant(case, **kw):
    i, s = dc.inputs(case), dc.spec(case)
    ref64, bound = dc.forward_bound(case, True, False)
    got = dc.forward64(i["x"], i["w"], i["bias"], s, False, **kw)
    if got.shape != ref64.shape:  # swapped strides: compared where both outputs exist
        bound = _overlap(bound, got)[0]
        got, ref64 = _overlap(got, ref64)
    return dc.worst(got, ref64, bound)


def _dgrad_mutant(case, **kw):
    i, s = dc.inputs(case), dc.spec(case)
    return dc.worst(dc.dgrad64(i["dy"], i["w"], i["gate"], s, **kw), *dc.dgrad_bound(case, True))


MUTANTS = {
    "forward: a dropped tap": lambda c: _forward_mutant(c, drop_tap=True),
    "forward: ph off by one": lambda c: _forward_mutant(c, ph_off=1),
    "forward: the last output row skipped": lambda c: _forward_mutant(c, skip_last_row=True),
    "dgrad: a dropped tap": lambda c: _dgrad_mutant(c, drop_tap=True),
    "dgrad: the gate ignored": lambda c: _dgrad_mutant(c, ignore_gate=True),
    "wgrad: accumulate treated as store": lambda c: dc.worst(
        dc.wgrad64(dc.inputs(c)["dy"], dc.inputs(c)["x"], dc.spec(c))[0], *dc.wgrad_bound(c, dc.PREFILL)[0]),
    "wgrad: one slab dropped from the dw sum": lambda c: dc.worst(
        dc.wgrad64(dc.inputs(c)["dy"], dc.inputs(c)["x"], dc.spec(c), drop_slab=True)[0], *dc.wgrad_bound(c)[0]),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_every_mutant_violates_its_bound(name):
    ratios = {c: MUTANTS[name](c) for c in dc.CASES}
    assert max(ratios.values()) >= 10.0, ratios


def test_swapped_strides_violate_the_bound_where_they_differ():
    assert _forward_mutant(dc.STRIDES_DIFFER, swap_strides=True) >= 10.0


def test_depthwise_ok_truth_table(monkeypatch):
    from sparknet_amd.ops.hip import depthwise_ok
    monkeypatch.delenv("SN_FEATURES", raising=False)
    mk = lambda C, K, R=3, groups=None, **kw: ConvSpec(2, 8, 8, C, K, R, R, groups=C if groups is None else groups, **kw)
    assert depthwise_ok(mk(16, 16)) and depthwise_ok(mk(520, 520, sh=2, sw=1, ph=0, pw=2))
    assert not depthwise_ok(mk(12, 12))            # C % 8 != 0
    assert not depthwise_ok(mk(16, 32))            # channel multiplier 2
    assert not depthwise_ok(mk(16, 16, R=5))       # 5x5
    assert not depthwise_ok(mk(16, 16, groups=2))  # grouped, not depthwise
    assert not depthwise_ok(mk(16, 16, dh=2, dw=2))
    monkeypatch.setenv("SN_FEATURES", "conv_depthwise=0")  # read at use, not at import
    assert not depthwise_ok(mk(16, 16))
    monkeypatch.setenv("SN_FEATURES", "conv_depthwise=1")
    assert depthwise_ok(mk(16, 16))


def test_mobilenet_builds():
    from sparknet_amd.core.net import Net
    B = 2
    net = Net(models.mobilenet(train_batch=B, test_batch=B), phase=proto.TRAIN, device="cpu")
    assert sum(l.type_name == "BatchNorm" for l in net.layers) == 27
    learnable = sum(p.data.numel() for l in net.layers if l.type_name != "BatchNorm" for p in l.params)
    assert learnable == 4231976
    convs = [l for l in net.layers if l.type_name == "Convolution"]
    assert [l.name for l in convs][:3] == ["conv1", "conv2_1/dw", "conv2_1/sep"] and convs[-1].name == "fc7"
    assert sum(l.name.endswith("/dw") for l in convs) == 13
    # fc7 is a 1x1 convolution over the globally pooled map: [B, 1000] with singleton spatial axes
    top = tuple(net.blob_by_name("fc7").shape)
    assert top[:2] == (B, 1000) and all(d == 1 for d in top[2:])
    assert "mobilenet" in models.MODELS


def test_mobilenet_widths_stay_multiples_of_8():
    from sparknet_amd.core.net import Net
    net = Net(models.mobilenet(train_batch=1, test_batch=1, crop=32, classes=10, alpha=0.3), phase=proto.TRAIN,
              device="cpu")
    for l in net.layers:
        if l.type_name == "Convolution" and l.name != "fc7":
            assert l.params[0].data.shape[0] % 8 == 0, l.name


def test_mobilenet_cpu_solver_step():
    from sparknet_amd.core.solver import Solver
    B = 4
    sp = models.solver_for("mobilenet", alpha=0.25, crop=32, classes=10, train_batch=B, test_batch=B)
    solver = Solver(sp, device=torch.device("cpu"), seed=3, build_test_nets=False)
    g = torch.Generator().manual_seed(5)
    solver.net.blob_by_name("data").set_nchw(torch.randn(B, 3, 32, 32, generator=g))
    solver.net.blob_by_name("label").set_nchw(torch.randint(0, 10, (B, 1), generator=g).float())
    w0 = solver.net.flat_data.detach().clone()
    solver.stage_hyper()
    loss = float(solver.iteration())
    assert loss == loss and abs(loss) < 1e3, loss
    assert not torch.equal(w0, solver.net.flat_data)
