"""The GEMM front-end of ops.gemm, pinned launch by launch (CPU; tests/gemm_trace_cases.py has the
cases and the recorder).  Every case's trace — each field of every SnGemmArgs handed to the kernel
library, the reduce / fold launches around it, the tune keys it missed — must equal
tests/gemm_launch_trace.json, and the cases together must move every field of SnGemmArgs and reach
every kernel ops.gemm can call.  A change that alters a launch on purpose regenerates the fixture
(``python tests/gemm_trace_cases.py``) and shows the moved fields in its diff."""
import json
import re

import pytest

import gemm_trace_cases as tc
from sparknet_amd.ops import _lib, gemm as G

FIXTURE = json.loads(tc.FIXTURE.read_text())
SWITCHES = ("torch", "_FORCE_TILE", "_AUTOTUNE", "_THIN", "_LDS_EPI", "_SIDE_FRAG", "_TUNED", "_MISSES", "_SIDE",
            "_DEFER_SINK", "SIDE_STATS")


def test_fixture_lists_the_cases():
    assert list(FIXTURE) == list(tc.CASES)


def test_fixture_is_one_launch_per_line():
    assert tc.FIXTURE.read_text() == tc.dumps(FIXTURE)


@pytest.mark.parametrize("name", tc.CASES)
def test_trace_equals_fixture(name):
    trace = json.loads(json.dumps(tc.run(name)))
    want = FIXTURE[name]
    for i, (got, exp) in enumerate(zip(trace, want)):
        assert got == exp, f"launch {i}"
    assert len(trace) == len(want)


def test_every_field_and_kernel_is_reached():
    launches = [launch for trace in FIXTURE.values() for launch in trace]
    gemms = [launch[1] for launch in launches if launch[0] == "sn_gemm"]
    for field, _ in _lib.SnGemmArgs._fields_:
        values = {json.dumps(g.get(field, 0)) for g in gemms}
        assert len(values) >= 2, f"SnGemmArgs.{field} only ever {values}"
    for operand in "AB":
        for field in ("ptr", "ld", "gstride", "g"):
            assert len({json.dumps(g[operand].get(field, 0)) for g in gemms}) >= 2, (operand, field)
    kernels = set(re.findall(r'_lib\.call\("(\w+)"', open(G.__file__).read()))
    assert len(kernels) >= 3, kernels
    assert kernels <= {launch[0] for launch in launches}, kernels


def test_tune_keys_survive_their_string_form():
    db = json.loads(tc.DB.read_text())
    assert len(db) > 100 and all(ks in db for ks in tc.DB_KEYS)
    for ks in db:
        key = G._key_from_str(ks)
        assert G._key_to_str(key) == ks and G._key_from_str(G._key_to_str(key)) == key


def test_cases_leave_the_module_alone():
    before = ({k: getattr(G, k) for k in SWITCHES}, {k: getattr(_lib, k) for k in ("kernels", "stream_ptr", "call")},
              dict(G._TUNED), set(G._MISSES), dict(G.SIDE_STATS))
    tc.run("Fp8Side: _SIDE_FRAG off stores only through the LDS epilogue")
    tc.run("database hits: no miss; the same products on the cost model")
    assert before == ({k: getattr(G, k) for k in SWITCHES}, {k: getattr(_lib, k) for k in ("kernels", "stream_ptr", "call")},
                      dict(G._TUNED), set(G._MISSES), dict(G.SIDE_STATS))
