"""Dispatch of the stride-2 data gradient (ops.hip.tstride_ok, TSTRIDE_DGRAD) on the CPU recorder of
tests/conv_trace_cases.py; tests/test_conv_tstride_gpu.py holds the kernel to its fp64 oracle."""
import pytest

import conv_trace_cases as tc
from sparknet_amd.ops import hip
from sparknet_amd.ops.spec import ConvSpec

ELIGIBLE = tc.conv(2, 16, 16, 64, 128, 1, stride=2)  # 2 x 8 x 8 = 128 output-gradient pixels


def _kernels(trace):
    return [l[0] for l in trace if l[0] not in ("result", "raise")]


def test_an_eligible_shape_takes_one_launch():
    trace = tc.run(tc.Case(ELIGIBLE))
    assert _kernels(trace).count(hip.TSTRIDE_DGRAD) == 1 and "col2im" not in _kernels(trace), trace
    launch = [l for l in trace if l[0] == hip.TSTRIDE_DGRAD][0]
    # dy, w, gate, dx, then N, H, W, C, K, R, S, ph, pw
    assert launch[1:4] == ["dy:bfloat16[2,8,8,128]/[8192,1024,128,1]+0", "w:bfloat16[128,1,1,64]/[64,64,64,1]+0",
                           "x:bfloat16[2,16,16,64]/[16384,1024,64,1]+0"]
    assert launch[4].endswith(":bfloat16[2,16,16,64]/[16384,1024,64,1]+0")
    assert launch[5:] == [2, 16, 16, 64, 128, 1, 1, 0, 0]


def test_the_switch_restores_the_generic_route():
    on, off = (_kernels(tc.run(tc.Case(ELIGIBLE, features=f))) for f in ("", "conv_tstride=0"))
    assert hip.TSTRIDE_DGRAD not in off and "col2im" in off and "relu_bwd" in " ".join(off)
    assert [k for k in on if k != hip.TSTRIDE_DGRAD] == off[:len(on) - 1]  # forward and weight gradient unchanged


@pytest.mark.parametrize("spec", [
    tc.STRIDED,                                                   # 32 output-gradient pixels: below the bound
    tc.conv(2, 16, 16, 64, 128, 3, stride=2, pad=1, groups=2),
    ConvSpec(2, 16, 16, 64, 128, 3, 3, 2, 2, 1, 1, 2, 2, 1),      # dilated
    tc.conv(2, 16, 16, 64, 128, 5, stride=2, pad=2),
], ids=("small", "grouped", "dilated", "5x5"))
def test_other_shapes_keep_their_route(spec, monkeypatch):
    monkeypatch.delenv("SN_FEATURES", raising=False)
    assert not hip.tstride_ok(spec)
    assert hip.TSTRIDE_DGRAD not in _kernels(tc.run(tc.Case(spec)))

