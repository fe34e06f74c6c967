"""The convolution dispatch of ops.hip, pinned launch by launch (CPU; tests/conv_trace_cases.py has
the cases and the recorder).  Every case's trace — kernels, scalar arguments, tensor layouts, GEMM
operands, in order — must equal tests/conv_launch_trace.json, and the cases together must reach
every convolution launcher the dispatch can call, so a case list that stops reaching a route fails
too.  A change that moves a shape to another kernel on purpose regenerates the fixture
(``python tests/conv_trace_cases.py``) and shows the moved launches in its diff."""
import json
import re

import pytest

import conv_trace_cases as tc
from sparknet_amd.ops import hip

FIXTURE = json.loads(tc.FIXTURE.read_text())


def test_fixture_lists_the_cases():
    assert list(FIXTURE) == list(tc.CASES)


@pytest.mark.parametrize("name", tc.CASES)
def test_trace_equals_fixture(name):
    trace = json.loads(json.dumps(tc.run(tc.CASES[name])))
    want = FIXTURE[name]
    for i, (got, exp) in enumerate(zip(trace, want)):
        assert got == exp, f"launch {i}"
    assert len(trace) == len(want)


def test_every_conv_launcher_is_reached():
    src = open(hip.__file__).read()
    conv = src[src.index("# Convolution\n"):src.index("# InnerProduct\n")]
    launchers = set(re.findall(r'\bcall\("((?:conv|s2d_)\w*|flip_weights|im2col|col2im)"', conv))
    assert len(launchers) >= 15, launchers
    seen = {launch[0] for trace in FIXTURE.values() for launch in trace}
    assert launchers <= seen, sorted(launchers - seen)


@pytest.mark.parametrize("name", ["fp8 both e4m3", "fp8 dgrad e4m3, c64", "fp8 both, chunked"])
def test_a_second_backward_quantises_dy_again(name):
    """dy's fp8 bytes belong to one conv_backward call: a second call on the same workspace, with no
    forward in between, makes them anew instead of reading the first call's."""
    trace = tc.run(tc.CASES[name], backwards=2)
    ends = [i for i, launch in enumerate(trace) if launch[:2] == ["result", "dx"]]
    first, second = trace[ends[0] - (ends[1] - ends[0] - 1):ends[0]], trace[ends[0] + 1:ends[1]]
    assert [launch[0] for launch in second] == [launch[0] for launch in first]
    assert sum(launch[0] == "quant_fp8" and launch[1].startswith("dy:") for launch in second) == 1


def test_dispatch_leaves_the_switches_alone():
    before = {k: getattr(hip, k) for k in ("call", "gemm", "colsum", "_dw_part", "_MAX_PIX", "_PACKED")}
    tc.run(tc.CASES["direct k96, packed off"])
    assert before == {k: getattr(hip, k) for k in before}
