"""32-wide grouped 3x3 convolution, CPU side: the dispatch predicate and the launches it leads to
(the recorder of tests/conv_trace_cases.py).  tests/test_conv_wgroup_gpu.py holds the kernels of
csrc/kernels/conv_wgroup.hip to the fp64 oracle."""
import torch

import conv_trace_cases as tc
from sparknet_amd.ops.spec import ConvSpec


def test_wgroup_ok_truth_table(monkeypatch):
    from sparknet_amd.ops.hip import grouped_ok, wgroup_ok
    monkeypatch.delenv("SN_FEATURES", raising=False)
    mk = lambda C, K, cg, R=3, **kw: ConvSpec(2, 8, 8, C, K, R, R, groups=C // cg, **kw)
    assert wgroup_ok(mk(64, 64, 32)) and wgroup_ok(mk(1024, 1024, 32, sh=2, sw=1, ph=0, pw=2))
    # one group: taken, except the 8 x 8 images tests/conv_launch_trace.json pins to the implicit GEMM
    assert wgroup_ok(ConvSpec(2, 7, 7, 32, 32, 3, 3, groups=1)) and not wgroup_ok(mk(32, 32, 32))
    assert not grouped_ok(mk(64, 64, 32))            # the narrow-group predicate is unchanged
    assert not wgroup_ok(mk(64, 64, 16)) and not wgroup_ok(mk(128, 128, 64))
    assert not wgroup_ok(mk(64, 128, 32))            # Cg = 32, Kg = 64
    assert not wgroup_ok(ConvSpec(2, 8, 8, 32, 48, 3, 3, groups=1))   # Cg = 32, Kg = 48
    assert not wgroup_ok(ConvSpec(2, 8, 8, 48, 48, 3, 3, groups=1))   # C % 32 != 0 (then Cg is not 32 either)
    assert not wgroup_ok(mk(64, 64, 32, R=5))
    assert not wgroup_ok(mk(64, 64, 32, dh=2, dw=2))
    assert not wgroup_ok(mk(64, 64, 32, sh=3, sw=3))
    assert wgroup_ok(ConvSpec(2 ** 19, 32, 32, 32, 32, 3, 3, 1, 1, 1, 1, 1, 1, 1))
    assert not wgroup_ok(ConvSpec(2 ** 20, 32, 32, 32, 32, 3, 3, 1, 1, 1, 1, 1, 1, 1))   # 2^30 pixels
    monkeypatch.setenv("SN_FEATURES", "conv_wgroup=0")  # read at use, not at import
    assert not wgroup_ok(mk(64, 64, 32))
    monkeypatch.setenv("SN_FEATURES", "conv_wgroup=1")
    assert wgroup_ok(mk(64, 64, 32))


W21 = ConvSpec(2, 8, 8, 64, 64, 3, 3, 2, 1, 1, 1, 1, 1, 2)   # Cg = 32, strides (2, 1)


def _trace(spec, **kw):
    return tc.run(tc.Case(spec, patch={"_wgroup_part": lambda s, device: (torch.zeros(8), 8)}, **kw))


def _kernels(trace):
    return [l[0] for l in trace if l[0] not in ("result", "raise")]


def test_a_routed_layer_launches_the_three_kernels():
    t = _trace(W21, dw_acc=False)
    assert _kernels(t) == ["conv_wgroup_fwd", "colsum", "conv_wgroup_wgrad", "conv_wgroup_dgrad"], t
    geom = [2, 8, 8, 64, 2, 1, 1, 1]  # N, H, W, C, sh, sw, ph, pw
    fwd, _, wg, dg = [l for l in t if l[0] != "result"]
    assert fwd[1:5] == ["x:bfloat16[2,8,8,64]/[4096,512,64,1]+0", "w:bfloat16[64,3,3,32]/[288,96,32,1]+0",
                        "b:float32[64]/[1]+0", "t0:bfloat16[2,4,8,64]/[2048,512,64,1]+0"]
    assert fwd[5:] == geom + [1]  # ReLU in the epilogue
    assert wg[1:3] == ["dy:bfloat16[64,64]/[64,1]+0", "x:bfloat16[2,8,8,64]/[4096,512,64,1]+0"]
    assert wg[4:7] == [8, "dw:float32[64,3,3,32]/[288,96,32,1]+0", 0] and wg[7:] == geom
    assert dg[1:4] == ["dy:bfloat16[2,4,8,64]/[2048,512,64,1]+0", "w:bfloat16[64,3,3,32]/[288,96,32,1]+0",
                       "x:bfloat16[2,8,8,64]/[4096,512,64,1]+0"] and dg[5:] == geom


def test_what_the_predicate_refuses_keeps_its_launches():
    s1 = ConvSpec(2, 8, 8, 64, 64, 3, 3, 1, 1, 1, 1, 1, 1, 2)  # stride 1: fp8-eligible both ways
    off = _kernels(_trace(s1, features="conv_wgroup=0"))
    assert off and not any(k.startswith("conv_wgroup") for k in off)
    fp8 = _kernels(_trace(s1, fp8=("e4m3", True, None)))
    assert fp8[1:] == _kernels(_trace(s1, fp8=("e4m3", True, None), features="conv_wgroup=0"))[1:]
    sl = _kernels(_trace(s1, dx_in=(128, 0)))  # a sliced dx keeps the implicit GEMM's in-place write
    assert "conv_wgroup_dgrad" not in sl and "conv_wgroup_wgrad" in sl
