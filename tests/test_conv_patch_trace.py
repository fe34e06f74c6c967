"""The route to the patch-resident 5x5 data gradient in ops.hip.conv_backward, launch by launch on
the CPU with the recorder of tests/conv_trace_cases.py (imported, not changed): the CaffeNet conv2
shape reaches the new launcher with the arguments expected, ``conv_patch=0`` gives back the GEMM
launches, and operands the kernel does not take (a sliced or misaligned dx, a non-bf16 gate, the
in-place weight operand, an fp8 side output, images below the minimum band) stay on the GEMM."""
import dataclasses

import pytest
import torch

import conv_trace_cases as tc
from sparknet_amd.ops import hip

CONV2 = tc.conv(2, 27, 27, 96, 256, 5, pad=2, groups=2)
DY = "dy:bfloat16[2,27,27,256]/[186624,6912,256,1]+0"
X = "x:bfloat16[2,27,27,96]/[69984,2592,96,1]+0"
WT = "bfloat16[2,48,5,5,128]/[153600,3200,640,128,1]+0"


def _dgrad(trace):
    """The launches between the weight gradient's and the returned dx: the data gradient's."""
    end = next(i for i, launch in enumerate(trace) if launch[:2] == ["result", "dx"])
    start = max(i for i, launch in enumerate(trace[:end]) if launch[0] == "gemm" and launch[8].get("bias_grad")) + 1
    return trace[start:end]


def test_launcher_name_is_a_module_constant():
    assert hip.PATCH_DGRAD == "conv_patch_dgrad"
    assert 'call("conv_patch' not in open(hip.__file__).read()


@pytest.mark.parametrize("wt", [False, True], ids=["flip pass", "pre-flipped"])
def test_caffenet_conv2_reaches_the_patch_kernel(wt):
    trace = tc.run(tc.Case(CONV2, wt=wt))
    got = _dgrad(trace)
    flipped = "w_flipped:" + WT if wt else "t1:" + WT
    want = [] if wt else [["flip_weights", "w:bfloat16[256,5,5,48]/[1200,240,48,1]+0", flipped, 2, 128, 5, 5, 48]]
    dx = "t1" if wt else "t2"
    want.append(["conv_patch_dgrad", DY, flipped, X, f"{dx}:bfloat16[2,27,27,96]/[69984,2592,96,1]+0",
                 2, 27, 27, 2, 256, 96, 1.0, 0])
    assert got == want
    assert not any(launch[0] == "gemm" and launch[4][0] == "Im2col" and launch[4][1].startswith("dy:")
                   for launch in trace)


def test_no_gate_passes_none():
    launch = _dgrad(tc.run(tc.Case(CONV2, wt=True, gate=False)))[-1]
    assert launch[0] == "conv_patch_dgrad" and launch[3] is None


@pytest.mark.parametrize("wt", [False, True], ids=["flip pass", "pre-flipped"])
def test_switch_off_gives_back_the_gemm_launches(wt):
    """With conv_patch=0 the 27 x 27 trace is the pinned 6 x 6 grouped trace with the sizes changed:
    the same launches with the same operand kinds and keywords, and everything outside the data
    gradient is what the default route launches too."""
    on = tc.run(tc.Case(CONV2, wt=wt))
    off = tc.run(tc.Case(CONV2, wt=wt, features="conv_patch=0"))
    small = tc.run(tc.CASES["grouped, pre-flipped" if wt else "grouped implicit"])

    def shape_of(trace):
        return [[launch[0]] + ([launch[4][0], launch[5][0], sorted(launch[8])] if launch[0] == "gemm" else [])
                for launch in trace]
    assert shape_of(off) == shape_of(small)
    assert "conv_patch_dgrad" not in [launch[0] for launch in off]
    gemm = _dgrad(off)[-1]
    assert gemm[:4] == ["gemm", 2 * 27 * 27, 48, 3200]
    assert gemm[4] == ["Im2col", DY, [2, 27, 27, 256, 27, 27, 5, 5, 1, 1, 2, 2, 1, 1, 128], True, 128]
    assert gemm[5][0] == "Dense" and gemm[5][2:] == [3200, True, 48 * 3200]
    assert gemm[7] == 96 and gemm[8] == {"c_gstride": 48, "epi": hip.EPI_BF16, "gate": X, "groups": 2}
    n = len(_dgrad(on))
    assert off[:len(off) - len(_dgrad(off)) - 1] == on[:len(on) - n - 1]  # forward and weight gradient


def _stays_on_the_gemm(case):
    names = [launch[0] for launch in _dgrad(tc.run(case))]
    assert "conv_patch_dgrad" not in names and "gemm" in names, names


def test_sliced_dx_stays_on_the_gemm():
    _stays_on_the_gemm(tc.Case(CONV2, dx_in=(192, 0)))
    _stays_on_the_gemm(tc.Case(CONV2, x_in=(192, 96), dx_in=(192, 0)))


def test_inplace_weights_and_fp8_side_stay_on_the_gemm():
    _stays_on_the_gemm(tc.Case(CONV2, patch={"DGRAD_INPLACE_WEIGHTS": True}))
    _stays_on_the_gemm(tc.Case(CONV2, dx_side=True))


@pytest.mark.parametrize("H, W", [(6, 6), (7, 27), (27, 7), (27, 33)])
def test_images_outside_the_band_limits_stay_on_the_gemm(H, W):
    s = dataclasses.replace(CONV2, H=H, W=W)
    assert not hip.patch_dgrad_ok(s)
    _stays_on_the_gemm(tc.Case(s))


@pytest.mark.parametrize("H, W", [(8, 8), (12, 12), (13, 27), (27, 13), (27, 32)])
def test_images_inside_the_band_limits_are_routed(H, W):
    s = dataclasses.replace(CONV2, H=H, W=W)
    assert hip.patch_dgrad_ok(s)
    assert _dgrad(tc.run(tc.Case(s, wt=True)))[-1][0] == "conv_patch_dgrad"


@pytest.mark.parametrize("change", [dict(C=64, K=256), dict(C=96, K=128), dict(R=3, S=3, ph=1, pw=1),
                                    dict(ph=1, pw=1), dict(sh=2, sw=2), dict(dh=2, dw=2, ph=4, pw=4)])
def test_other_geometries_are_not_routed(change):
    assert not hip.patch_dgrad_ok(dataclasses.replace(CONV2, **change))


def _backward_with(dy, x, gate, dx_out=None):
    """conv_backward of CONV2 under the recorder with operands of the caller's making."""
    s = CONV2
    named = {"x": x, "dy": dy, "w": torch.zeros((s.K, 5, 5, s.Cg), dtype=tc.BF16),
             "w_flipped": torch.zeros((s.groups, s.Cg, 5, 5, s.Kg), dtype=tc.BF16)}
    if gate is not None and gate is not x:
        named["gate"] = gate
    if dx_out is not None:
        named["dx"] = dx_out
    rec = tc.Recorder(named)
    with tc._patched(rec, tc.Case(s), 0):
        hip.conv_backward(dy, x, named["w"], s, True, None, None, gate, hip.ConvScratch(wt=named["w_flipped"]),
                          dx_out=dx_out)
    return [launch[0] for launch in rec.trace]


def test_non_bf16_and_misaligned_operands_stay_on_the_gemm():
    s = CONV2
    dy = torch.zeros((s.N, s.P, s.Q, s.K), dtype=tc.BF16)
    x = torch.zeros((s.N, s.H, s.W, s.C), dtype=tc.BF16)
    assert _backward_with(dy, x, x) == ["conv_patch_dgrad"]
    assert _backward_with(dy, x, x.float()) == ["gemm"]  # a gate that is not bf16
    buf = torch.zeros(x.numel() + 8, dtype=tc.BF16)
    off = next(o for o in range(1, 8) if buf[o:].data_ptr() % 16)
    dx = buf[off:off + x.numel()].view(x.shape)  # dense, but not on a 16-byte boundary
    assert _backward_with(dy, x, None, dx_out=dx) == ["gemm"]
    wide = torch.zeros((s.N, s.H, s.W, 2 * s.C), dtype=tc.BF16)
    assert _backward_with(dy, x, None, dx_out=wide[..., s.C:]) == ["gemm"]  # a channel slice
