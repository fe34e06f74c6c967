"""Wide-window depthwise convolution, CPU side (tests/test_conv_xdw_gpu.py holds the HIP kernels to
the oracle and bounds of tests/conv_xdw_cases.py): the bounds admit a correct fp32 implementation
(ops.ref), the dispatch predicate, the launches of one forward + backward, and the MnasNet zoo model."""
import pytest
import torch

import conv_xdw_cases as xc
from sparknet_amd import models, proto
from sparknet_amd.ops import ref
from sparknet_amd.ops.spec import ConvSpec


@pytest.mark.parametrize("case", xc.CASES, ids=xc.IDS)
def test_bounds_admit_the_fp32_reference(case):
    i, s = xc.inputs(case), xc.spec(case)
    for bias in (True, False):
        for relu in (True, False):
            y = ref.conv_forward(i["x"], i["w"], i["bias"] if bias else None, s, relu=relu)
            assert y.dtype == torch.bfloat16
            assert xc.worst(y, *xc.forward_bound(case, bias, relu)) <= 1.0, (bias, relu)
    for gate, prefill in ((True, None), (False, xc.PREFILL)):
        dw = torch.full((s.C, s.R, s.S, 1), xc.PREFILL)
        db = torch.full((s.C,), xc.PREFILL)
        dx = ref.conv_backward(i["dy"], i["x"], i["w"], s, True, dw, db, i["gate"] if gate else None,
                               dw_acc=prefill is not None, db_acc=prefill is not None)
        assert xc.worst(dx, *xc.dgrad_bound(case, gate)) <= 1.0
        bw, bb = xc.wgrad_bound(case, prefill)
        assert xc.worst(dw, *bw) <= 1.0 and xc.worst(db, *bb) <= 1.0, prefill


def test_xdepthwise_ok_truth_table(monkeypatch):
    from sparknet_amd.ops.hip import depthwise_ok, xdepthwise_ok
    monkeypatch.delenv("SN_FEATURES", raising=False)
    mk = lambda C=16, K=16, R=5, S=None, **kw: ConvSpec(2, 12, 12, C, K, R, R if S is None else S, groups=C, **kw)
    for s in (mk(), mk(R=7, sh=2, sw=1, ph=3), mk(R=3, dh=2, dw=2), mk(R=1, S=7), mk(R=3, S=2, dh=3), mk(C=72, K=72)):
        assert xdepthwise_ok(s) and not depthwise_ok(s), s
    assert depthwise_ok(mk(R=3)) and not xdepthwise_ok(mk(R=3))  # undilated 3x3 belongs to conv_dw.hip
    for s in (mk(R=9), mk(R=3, dh=4, dw=4), mk(sh=3, sw=3), mk(R=3, dh=2, dw=2, sh=2, sw=2), mk(C=12, K=12),
              mk(K=32)):  # extent 9 (twice), stride 3, dilation with a stride, C % 8, channel multiplier
        assert not xdepthwise_ok(s), s
    monkeypatch.setenv("SN_FEATURES", "conv_depthwise=0")  # the 3x3 window stays out with its own switch off
    assert not xdepthwise_ok(mk(R=3)) and xdepthwise_ok(mk())
    monkeypatch.setenv("SN_FEATURES", "conv_depthwise_wide=0")  # read at use, not at import
    assert not xdepthwise_ok(mk())


@pytest.mark.parametrize("switch, want", [("", True), ("conv_depthwise_wide=0", False)])
def test_forward_and_backward_launch_the_three_kernels(monkeypatch, switch, want):
    from sparknet_amd.ops import gemm as G, hip
    names = []
    monkeypatch.setenv("SN_FEATURES", switch)
    monkeypatch.setattr(hip, "call", lambda name, *a: names.append(name))
    monkeypatch.setattr(hip, "gemm", lambda *a, **kw: names.append("gemm"))
    monkeypatch.setattr(hip, "colsum", lambda *a, **kw: names.append("colsum"))
    monkeypatch.setattr(hip, "relu_backward", lambda dx, gate: dx)
    monkeypatch.setattr(hip, "_xdw_part", lambda s, device: (torch.zeros(8), 8))
    i, s = xc.inputs(xc.MNASNET_LIKE), xc.spec(xc.MNASNET_LIKE)
    hip.conv_forward(i["x"], i["w"], None, s, relu=True)
    hip.conv_backward(i["dy"], i["x"], i["w"], s, True, torch.zeros(s.C, s.R, s.S, 1), torch.zeros(s.C), i["gate"])
    if want:
        assert names == [hip.XDW_FWD, hip.XDW_WGRAD, hip.XDW_DGRAD]
        assert names == ["conv_xdw_fwd", "conv_xdw_wgrad", "conv_xdw_dgrad"]
    else:
        assert names and not {hip.XDW_FWD, hip.XDW_WGRAD, hip.XDW_DGRAD} & set(names) and "im2col" in names


def test_mnasnet_builds_and_takes_a_cpu_solver_step():
    from sparknet_amd.core.net import Net
    from sparknet_amd.core.solver import Solver
    net = Net(models.mnasnet(train_batch=2, test_batch=2), phase=proto.TRAIN, device="cpu")
    assert sum(p.data.numel() for l in net.layers if l.type_name != "BatchNorm" for p in l.params) == 4383312
    dws = [l for l in net.layers if l.type_name == "Convolution" and l.name.endswith("/dw")]
    assert [l.params[0].data.shape[1] for l in dws].count(5) == 10 and len(dws) == 17
    assert sum(l.type_name == "Eltwise" for l in net.layers) == 10 and tuple(net.blob_by_name("fc").shape) == (2, 1000)
    B = 4
    sp = models.solver_for("mnasnet", alpha=0.25, crop=32, classes=10, train_batch=B, test_batch=B)
    for l in sp.net_param.layer:
        if l.type == "Convolution" and l.name != "head/conv":
            assert l.convolution_param.num_output % 8 == 0, l.name
    solver = Solver(sp, device=torch.device("cpu"), seed=3, build_test_nets=False)
    g = torch.Generator().manual_seed(5)
    solver.net.blob_by_name("data").set_nchw(torch.randn(B, 3, 32, 32, generator=g))
    solver.net.blob_by_name("label").set_nchw(torch.randint(0, 10, (B, 1), generator=g).float())
    w0 = solver.net.flat_data.detach().clone()
    solver.stage_hyper()
    loss = float(solver.iteration())
    assert loss == loss and abs(loss) < 1e3, loss
    assert not torch.equal(w0, solver.net.flat_data)
