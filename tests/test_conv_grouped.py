"""Narrow-group 3x3 convolution, CPU side (tests/test_conv_grouped_gpu.py holds the HIP kernels
to the same oracle and bounds; tests/conv_grouped_cases.py has them): the bounds admit a correct
fp32 implementation (ops.ref), every mutant of the oracle violates them by at least 10x, the
dispatch predicate and the launches it leads to, and the ResNeXt zoo model."""
import pytest
import torch

import conv_grouped_cases as gc
import conv_trace_cases as tc
from sparknet_amd import models, proto
from sparknet_amd.ops import ref
from sparknet_amd.ops.spec import ConvSpec


@pytest.mark.parametrize("case", gc.CASES, ids=gc.IDS)
def test_bounds_admit_the_fp32_reference(case):
    i, s = gc.inputs(case), gc.spec(case)
    for bias in (True, False):
        for relu in (True, False):
            y = ref.conv_forward(i["x"], i["w"], i["bias"] if bias else None, s, relu=relu)
            assert y.dtype == torch.bfloat16
            assert gc.worst(y, *gc.forward_bound(case, bias, relu)) <= 1.0, (bias, relu)
    for gate, prefill in ((True, None), (False, gc.PREFILL)):
        dw = torch.full((s.C, 3, 3, s.Cg), gc.PREFILL)
        db = torch.full((s.C,), gc.PREFILL)
        dx = ref.conv_backward(i["dy"], i["x"], i["w"], s, True, dw, db, i["gate"] if gate else None,
                               dw_acc=prefill is not None, db_acc=prefill is not None)
        assert gc.worst(dx, *gc.dgrad_bound(case, gate)) <= 1.0
        bw, bb = gc.wgrad_bound(case, prefill)
        assert gc.worst(dw, *bw) <= 1.0 and gc.worst(db, *bb) <= 1.0, prefill


def _overlap(a, b):
    p, q = min(a.shape[1], b.shape[1]), min(a.shape[2], b.shape[2])
    return a[:, :p, :q], b[:, :p, :q]


def _forward_mutant(case, **kw):
    i, s = gc.inputs(case), gc.spec(case)
    ref64, bound = gc.forward_bound(case, True, False)
    got = gc.forward64(i["x"], i["w"], i["bias"], s, False, **kw)
    if got.shape != ref64.shape:  # swapped strides: compared where both outputs exist
        bound = _overlap(bound, got)[0]
        got, ref64 = _overlap(got, ref64)
    return gc.worst(got, ref64, bound)


def _dgrad_mutant(case, **kw):
    i, s = gc.inputs(case), gc.spec(case)
    return gc.worst(gc.dgrad64(i["dy"], i["w"], i["gate"], s, **kw), *gc.dgrad_bound(case, True))


MUTANTS = {
    "forward: a dropped tap": lambda c: _forward_mutant(c, drop_tap=True),
    "forward: groups merged": lambda c: _forward_mutant(c, merge=True),
    "forward: ph off by one": lambda c: _forward_mutant(c, ph_off=1),
    "forward: the last output row skipped": lambda c: _forward_mutant(c, skip_last_row=True),
    "dgrad: a dropped tap": lambda c: _dgrad_mutant(c, drop_tap=True),
    "dgrad: groups merged": lambda c: _dgrad_mutant(c, merge=True),
    "dgrad: the gate ignored": lambda c: _dgrad_mutant(c, ignore_gate=True),
    "wgrad: accumulate treated as store": lambda c: gc.worst(
        gc.wgrad64(gc.inputs(c)["dy"], gc.inputs(c)["x"], gc.spec(c))[0], *gc.wgrad_bound(c, gc.PREFILL)[0]),
    "wgrad: one slab dropped from the dw sum": lambda c: gc.worst(
        gc.wgrad64(gc.inputs(c)["dy"], gc.inputs(c)["x"], gc.spec(c), drop_slab=True)[0], *gc.wgrad_bound(c)[0]),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_every_mutant_violates_its_bound(name):
    ratios = {c: MUTANTS[name](c) for c in gc.CASES}
    assert max(ratios.values()) >= 10.0, ratios


def test_swapped_strides_violate_the_bound_where_they_differ():
    assert _forward_mutant(gc.STRIDES_DIFFER, swap_strides=True) >= 10.0


def test_cases_cover_what_they_claim():
    from sparknet_amd.ops import hip
    specs = [gc.spec(c) for c in gc.CASES]
    for cg in hip.GROUPED_WIDTHS:
        assert {(s.sh, s.sw) for s in specs if s.Cg == cg} >= {(1, 1), (2, 2)}, cg
    assert {s.Cg for s in specs} == set(hip.GROUPED_WIDTHS)
    assert any(s.P * s.Q * s.N == 15 for s in specs) and any(s.P > s.H for s in specs)
    assert any(s.C // 16 > 4 for s in specs) and gc.STRIDES_DIFFER[5:7] == (2, 1)


def test_grouped_ok_truth_table(monkeypatch):
    from sparknet_amd.ops.hip import depthwise_ok, grouped_ok
    monkeypatch.delenv("SN_FEATURES", raising=False)
    mk = lambda C, K, cg, R=3, **kw: ConvSpec(2, 8, 8, C, K, R, R, groups=C // cg, **kw)
    for cg in (4, 8, 16):
        assert grouped_ok(mk(32, 32, cg)) and grouped_ok(mk(128, 128, cg, sh=2, sw=1, ph=0, pw=2))
    assert not grouped_ok(mk(32, 32, 1)) and depthwise_ok(mk(32, 32, 1))  # depthwise keeps its own kernels
    assert not grouped_ok(mk(32, 64, 4))            # Cg = 4, Kg = 8
    assert not grouped_ok(mk(24, 24, 4))            # C % 16 != 0
    assert not grouped_ok(mk(32, 32, 2))            # a width that is not routed
    assert not grouped_ok(mk(64, 64, 32))           # Cg = 32 stays on the implicit GEMM
    assert not grouped_ok(mk(32, 32, 4, R=5))       # 5x5
    assert not grouped_ok(mk(32, 32, 4, dh=2, dw=2))
    assert not grouped_ok(mk(32, 32, 4, sh=3, sw=3))
    # the kernels' 32-bit pixel arithmetic: 2^30 pixels per tensor are refused here, not by a raising launch
    assert grouped_ok(ConvSpec(2 ** 19, 32, 32, 16, 16, 3, 3, 1, 1, 1, 1, 1, 1, 4))
    assert not grouped_ok(ConvSpec(2 ** 20, 32, 32, 16, 16, 3, 3, 1, 1, 1, 1, 1, 1, 4))
    monkeypatch.setenv("SN_FEATURES", "conv_grouped=0")  # read at use, not at import
    assert not grouped_ok(mk(32, 32, 4))
    monkeypatch.setenv("SN_FEATURES", "conv_grouped=1")
    assert grouped_ok(mk(32, 32, 4))


# --- which launches the dispatch makes (the recorder of tests/conv_trace_cases.py, on CPU tensors) -----------

G4 = ConvSpec(2, 8, 8, 32, 32, 3, 3, 2, 1, 1, 1, 1, 1, 8)    # Cg = 4, strides (2, 1)
G16 = ConvSpec(2, 8, 8, 32, 32, 3, 3, 1, 1, 1, 1, 1, 1, 2)   # Cg = 16: stride 1, fp8-eligible both ways


def _part(s, device):
    return torch.zeros(8), 8


def _trace(spec, **kw):
    return tc.run(tc.Case(spec, patch={"_grouped_part": _part}, **kw))


def _kernels(trace):
    return [l[0] for l in trace if l[0] not in ("result", "raise")]


def test_a_routed_layer_launches_the_three_kernels():
    t = _trace(G4, dw_acc=False)
    assert _kernels(t) == ["conv_grouped_fwd", "colsum", "conv_grouped_wgrad", "conv_grouped_dgrad"], t
    geom = [2, 8, 8, 32, 4, 2, 1, 1, 1]  # N, H, W, C, Cg, sh, sw, ph, pw
    fwd, _, wg, dg = [l for l in t if l[0] not in ("result",)]
    assert fwd[1:5] == ["x:bfloat16[2,8,8,32]/[2048,256,32,1]+0", "w:bfloat16[32,3,3,4]/[36,12,4,1]+0",
                        "b:float32[32]/[1]+0", "t0:bfloat16[2,4,8,32]/[1024,256,32,1]+0"]
    assert fwd[5:] == geom + [1]  # ReLU in the epilogue
    assert wg[1:3] == ["dy:bfloat16[64,32]/[32,1]+0", "x:bfloat16[2,8,8,32]/[2048,256,32,1]+0"]
    assert wg[4:7] == [8, "dw:float32[32,3,3,4]/[36,12,4,1]+0", 0] and wg[7:] == geom
    assert dg[1:4] == ["dy:bfloat16[2,4,8,32]/[1024,256,32,1]+0", "w:bfloat16[32,3,3,4]/[36,12,4,1]+0",
                       "x:bfloat16[2,8,8,32]/[2048,256,32,1]+0"] and dg[5:] == geom
    # bias-free, accumulating, no data gradient: the weight gradient alone
    t = _trace(G4, db=False, need_dx=False)
    assert _kernels(t) == ["conv_grouped_fwd", "conv_grouped_wgrad"]
    assert [l for l in t if l[0] == "conv_grouped_wgrad"][0][6] == 1
    # the flip-path geometry (stride 1, Cg = 16) takes the new data gradient too, pre-flipped weights unread
    t = _trace(G16, wt=True)
    assert _kernels(t) == ["conv_grouped_fwd", "colsum", "conv_grouped_wgrad", "conv_grouped_dgrad"], t
    assert not any("w_flipped" in str(l) for l in t)


def test_what_the_predicate_refuses_keeps_its_launches():
    off = _trace(G16, features="conv_grouped=0")
    assert _kernels(off) and not any(k.startswith("conv_grouped") for k in _kernels(off))
    # an fp8 request: the e4m3 data and weight gradients run as before
    fp8 = _trace(G16, fp8=("e4m3", True, None))
    assert _kernels(fp8)[1:] == _kernels(_trace(G16, fp8=("e4m3", True, None), features="conv_grouped=0"))[1:]
    assert not any(k.startswith("conv_grouped") for k in _kernels(fp8)[1:])
    # channel slices: x is made dense for a grouped layer, a sliced dx keeps the implicit GEMM's in-place write
    sl = _trace(G16, dx_in=(64, 0))
    assert "conv_grouped_dgrad" not in _kernels(sl) and "conv_grouped_wgrad" in _kernels(sl)
    # C = 24, Cg = 4 and Cg != Kg
    for s in (ConvSpec(2, 8, 8, 24, 24, 3, 3, 1, 1, 1, 1, 1, 1, 6), ConvSpec(2, 8, 8, 32, 64, 3, 3, 1, 1, 1, 1, 1, 1, 8)):
        assert not any(k.startswith("conv_grouped") for k in _kernels(_trace(s)))


# --- the zoo model ---------------------------------------------------------------------------

def _learnable_from_shapes(reps=(3, 4, 6, 3), cardinality=32, width=4, classes=1000):
    """Convolution weights + Scale (gamma, beta) of every BatchNorm chain + the classifier."""
    conv_bn = lambda cin, cout, k, g=1: cout * (cin // g) * k * k + 2 * cout
    n, cin = conv_bn(3, 64, 7), 64
    for stage, r in enumerate(reps, 2):
        d = cardinality * width * 2 ** (stage - 2)
        for i in range(r):
            if i == 0:
                n += conv_bn(cin, 2 * d, 1)
            n += conv_bn(cin, d, 1) + conv_bn(d, d, 3, cardinality) + conv_bn(d, 2 * d, 1)
            cin = 2 * d
    return n + cin * classes + classes


def test_resnext50_builds():
    from sparknet_amd.core.net import Net
    assert _learnable_from_shapes() == 25028904
    B = 1
    for phase in (proto.TRAIN, proto.TEST):
        net = Net(models.resnext50(train_batch=B, test_batch=B), phase=phase, device="cpu")
        learnable = sum(p.data.numel() for l in net.layers if l.type_name != "BatchNorm" for p in l.params)
        assert learnable == 25028904
        convs = {l.name: l for l in net.layers if l.type_name == "Convolution"}
        grouped = [l for n, l in convs.items() if n.endswith("_branch2b")]
        assert len(grouped) == 16 and len(convs) == 53
        for l in grouped:
            K, R, S, Cg = l.params[0].data.shape
            assert l.groups == 32 and (R, S) == (3, 3) and K == 32 * Cg and Cg in (4, 8, 16, 32)
        # the stride sits on the 3x3 of a stage's first block, not on its 1x1
        tops = lambda name: tuple(net.blob_by_name(name).shape)[2:]
        assert tops("res3a_branch2a") == (56, 56) and tops("res3a_branch2b") == (28, 28)
        assert tops("res4a_branch2b") == (14, 14) and tops("res5a_branch2b") == (7, 7) and tops("res2a_branch2b") == (56, 56)
        assert tuple(net.blob_by_name("fc1000").shape)[:2] == (B, 1000)
    assert "resnext50" in models.MODELS and models.MODELS["resnext50"][1]().weight_decay == pytest.approx(1e-4)


def test_small_resnext_cpu_solver_step():
    from sparknet_amd.core.solver import Solver
    from sparknet_amd.models import zoo
    B = 4
    sp = zoo.resnext50_solver(models.resnext(reps=(1, 1, 1, 1), crop=32, classes=10, train_batch=B, test_batch=B))
    solver = Solver(sp, device=torch.device("cpu"), seed=3, build_test_nets=False)
    g = torch.Generator().manual_seed(5)
    solver.net.blob_by_name("data").set_nchw(torch.randn(B, 3, 32, 32, generator=g))
    solver.net.blob_by_name("label").set_nchw(torch.randint(0, 10, (B, 1), generator=g).float())
    w0 = solver.net.flat_data.detach().clone()
    solver.stage_hyper()
    loss = float(solver.iteration())
    assert loss == loss and abs(loss) < 1e3, loss
    assert not torch.equal(w0, solver.net.flat_data)
