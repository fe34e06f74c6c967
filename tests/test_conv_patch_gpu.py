"""The patch-resident 5x5 data gradient (csrc/kernels/conv_patch.hip) through ``hip.conv_backward``,
at the smallest shapes where it can go wrong: 12 x 12 (a width below 16, one band), 13 x 27 (a
width that is no multiple of 16; bands of 7 and 6 rows) and 27 x 13 (bands of 14 and 13 rows), one
image and three, one group and two (the group offsets in both pixel strides), gate on and off.

Every case is held to two references:

* bitwise to the ``conv_patch=0`` path, the implicit grouped GEMM, run unsplit (``splits=1`` handed
  to ``hip.gemm``: the kernel keeps one accumulator per output, as the unsplit GEMM does);
* elementwise to an fp64 oracle computed on the CPU from the same bf16 inputs, within the bound of
  tests/conv_grouped_cases.py: ``2^-8 |ref| + 1.01 T 2^-24 A`` with T = 25 * 128 + 1 terms and A
  the same computation on absolute values.  With a gate scale both ref and A carry the scale; the
  scale's own fp32 rounding is the one term T has beyond the 3200 products.

A gate scale other than 1 is not something conv_backward passes, so those runs call the launcher
and the GEMM directly, with the operands conv_backward would build.  Two more tests use inputs in
which every border tap matters: all ones (dx = 128 x the number of taps inside the image, exactly)
and weights that hold their tap's number (exact integer sums, so dx is the rounded oracle).
"""
import contextlib
import functools
import os

import pytest
import torch

from sparknet_amd.ops.spec import ConvSpec

pytestmark = pytest.mark.gpu

BF16, F64 = torch.bfloat16, torch.float64
U16, U32, C_SUM = 2.0 ** -8, 2.0 ** -24, 1.01
TERMS = 25 * 128 + 1
SCALE = 1.7
SHAPES = [(N, H, W, G) for N in (1, 3) for (H, W) in ((12, 12), (13, 27), (27, 13)) for G in (1, 2)]
IDS = ["x".join(map(str, c)) for c in SHAPES]


def spec(shape) -> ConvSpec:
    N, H, W, G = shape
    return ConvSpec(N, H, W, 48 * G, 128 * G, 5, 5, 1, 1, 2, 2, 1, 1, G)


@contextlib.contextmanager
def features(value):
    old = os.environ.get("SN_FEATURES")
    os.environ["SN_FEATURES"] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SN_FEATURES", None)
        else:
            os.environ["SN_FEATURES"] = old


@functools.lru_cache(maxsize=None)
def inputs(shape) -> dict:
    s = spec(shape)
    g = torch.Generator().manual_seed(1000 * shape[0] + 100 * shape[1] + 10 * shape[2] + shape[3])
    gate = torch.randn(s.N, s.H, s.W, s.C, generator=g)
    gate[torch.rand(gate.shape, generator=g) < 0.05] = 0.0
    return {"dy": torch.randn(s.N, s.P, s.Q, s.K, generator=g).to(BF16),
            "w": (0.05 * torch.randn(s.K, 5, 5, s.Cg, generator=g)).to(BF16), "gate": gate.to(BF16)}


def dgrad64(dy, w, s, absolute=False):
    """fp64 data gradient, NHWC, of bf16 dy [N,P,Q,K] and w [K,5,5,Cg]."""
    dyn, wo = dy.to(F64).permute(0, 3, 1, 2), w.to(F64).permute(0, 3, 1, 2)
    if absolute:
        dyn, wo = dyn.abs(), wo.abs()
    dx = torch.nn.grad.conv2d_input((s.N, s.C, s.H, s.W), wo, dyn, stride=1, padding=2, groups=s.groups)
    return dx.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def oracle(shape):
    """(ref, A) without the gate, computed once per shape and never written to."""
    i, s = inputs(shape), spec(shape)
    return dgrad64(i["dy"], i["w"], s), dgrad64(i["dy"], i["w"], s, absolute=True)


def worst(got, shape, gate, scale) -> float:
    ref, A = oracle(shape)
    if gate is not None:
        ref = ref * (gate.to(F64) > 0) * float(torch.tensor(scale, dtype=torch.float32))
        A = A * scale
    d = (got.to(F64).cpu() - ref).abs()
    bound = U16 * ref.abs() + C_SUM * TERMS * U32 * A
    return float(torch.where(d == 0, torch.zeros_like(d), d / bound).max())


@pytest.fixture
def spy(gpu, monkeypatch):
    """Names of the native launches made, in order; a GEMM is recorded as "gemm" and runs unsplit."""
    from sparknet_amd.ops import _lib, hip
    names = []
    native, gemm = _lib.call, hip.gemm

    def call(name, *args):
        names.append(name)
        return native(name, *args)

    def unsplit_gemm(*args, **kw):
        names.append("gemm")
        return gemm(*args, **{**kw, "splits": 1})
    monkeypatch.setattr(hip, "call", call)
    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(hip, "gemm", unsplit_gemm)
    return names


def _backward(hip, s, dy, w, gate):
    x = gate if gate is not None else torch.zeros((s.N, s.H, s.W, s.C), dtype=BF16, device=dy.device)
    return hip.conv_backward(dy, x, w, s, True, None, None, gate)


def _direct(hip, s, dy, w, gate, scale, patch, max_blocks=0):
    """What conv_backward launches for the data gradient, with a gate scale (and a grid limit)."""
    dx = torch.full((s.N, s.H, s.W, s.C), 3.0, dtype=BF16, device=dy.device)
    wt = hip._flipped(w, s, None)
    if patch:
        hip.call(hip.PATCH_DGRAD, dy, wt, gate, dx, s.N, s.H, s.W, s.groups, s.K, s.C, scale, max_blocks)
    else:
        kr2 = 25 * s.Kg
        g2 = hip.ConvGeom(s.N, s.P, s.Q, s.K, s.H, s.W, 5, 5, 1, 1, 2, 2, 1, 1, s.Kg)
        hip.gemm(s.N * s.H * s.W, s.Cg, kr2, hip.Im2col(dy, g2, kcontig=True, gstride=s.Kg),
                 hip.Dense(wt.view(s.C, kr2), kr2, True, gstride=s.Cg * kr2), dx, s.C, epi=hip.EPI_BF16,
                 groups=s.groups, c_gstride=s.Cg, gate=gate, gate_scale=scale)
    return dx


@pytest.mark.parametrize("gated", [True, False], ids=["gate", "nogate"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bitwise_the_gemm_path_and_within_the_fp64_bound(shape, gated, gpu, spy):
    from sparknet_amd.ops import hip
    s = spec(shape)
    i = {k: v.to(gpu) for k, v in inputs(shape).items()}
    gate = i["gate"] if gated else None
    with features(""):
        new = _backward(hip, s, i["dy"], i["w"], gate)
    assert spy == ["flip_weights", "conv_patch_dgrad"], spy
    del spy[:]
    with features("conv_patch=0"):
        old = _backward(hip, s, i["dy"], i["w"], gate)
    assert spy == ["flip_weights", "gemm"], spy
    assert new.dtype == BF16 and tuple(new.shape) == (s.N, s.H, s.W, s.C)
    r = worst(new, shape, inputs(shape)["gate"] if gated else None, 1.0)
    same = torch.equal(new.view(torch.int16), old.view(torch.int16))
    print("patch dgrad", shape, "gate", gated, "worst / bound", r, "bitwise the GEMM's", same)
    assert same
    assert r <= 1.0
    if gated:  # a gate scale other than 1, launcher against GEMM
        new = _direct(hip, s, i["dy"], i["w"], gate, SCALE, True)
        old = _direct(hip, s, i["dy"], i["w"], gate, SCALE, False)
        r = worst(new, shape, inputs(shape)["gate"], SCALE)
        same = torch.equal(new.view(torch.int16), old.view(torch.int16))
        print("patch dgrad", shape, "gate scale", SCALE, "worst / bound", r, "bitwise the GEMM's", same)
        assert same
        assert r <= 1.0


@pytest.mark.parametrize("max_blocks", [1, 5])
def test_blocks_that_walk_several_bands_give_the_same_bits(max_blocks, gpu):
    """A block takes the bands (image, group, band) in steps of the grid and fetches the next one's
    patch while it finishes the current one; the training shape has six per block.  Here 3 images x
    2 groups x 2 bands = 12 bands run on one block, and on five (3, 3, 2, 2, 2 bands, the groups and
    the short last band alternating inside a block), against one band per block."""
    from sparknet_amd.ops import hip
    shape = (3, 13, 27, 2)
    s = spec(shape)
    i = {k: v.to(gpu) for k, v in inputs(shape).items()}
    each = _direct(hip, s, i["dy"], i["w"], i["gate"], SCALE, True)
    few = _direct(hip, s, i["dy"], i["w"], i["gate"], SCALE, True, max_blocks)
    assert torch.equal(few.view(torch.int16), each.view(torch.int16))
    assert worst(few, shape, inputs(shape)["gate"], SCALE) <= 1.0


def _taps_inside(n: int) -> torch.Tensor:
    """How many of the 5 taps along an axis of n pixels lie inside it, per pixel."""
    i = torch.arange(n)
    return torch.minimum(i, torch.tensor(2)) + torch.minimum(n - 1 - i, torch.tensor(2)) + 1


@pytest.mark.parametrize("shape", [c for c in SHAPES if c[0] == 3], ids=[i for i, c in zip(IDS, SHAPES) if c[0] == 3])
def test_all_ones_give_the_tap_count_pattern(shape, gpu, spy):
    from sparknet_amd.ops import hip
    s = spec(shape)
    dy = torch.ones((s.N, s.P, s.Q, s.K), dtype=BF16, device=gpu)
    w = torch.ones((s.K, 5, 5, s.Cg), dtype=BF16, device=gpu)
    with features(""):
        dx = _backward(hip, s, dy, w, None)
    assert "conv_patch_dgrad" in spy and "gemm" not in spy, spy
    want = 128.0 * (_taps_inside(s.H)[:, None] * _taps_inside(s.W)[None, :]).to(torch.float32)  # exact in bf16
    assert float(want[0, 0]) == 128 * 9 and float(want[2, 2]) == 128 * 25
    assert torch.equal(dx.float().cpu(), want[None, :, :, None].expand(s.N, s.H, s.W, s.C))


@pytest.mark.parametrize("shape", [c for c in SHAPES if c[0] == 1], ids=[i for i, c in zip(IDS, SHAPES) if c[0] == 1])
def test_numbered_taps_are_summed_exactly(shape, gpu, spy):
    """w holds its tap's number (plus its group's), dy is 0 or 1: every sum is a small integer, exact in
    fp32, so dx is the oracle rounded once to bf16 — a tap taken from the wrong place cannot hide."""
    from sparknet_amd.ops import hip
    s = spec(shape)
    g = torch.Generator().manual_seed(5)
    dy = (torch.rand((s.N, s.P, s.Q, s.K), generator=g) < 0.5).to(BF16)
    tap = torch.arange(1, 26, dtype=torch.float32).view(1, 5, 5, 1)
    w = (tap + (torch.arange(s.K) // s.Kg).view(-1, 1, 1, 1)).expand(s.K, 5, 5, s.Cg).contiguous().to(BF16)
    with features(""):
        dx = _backward(hip, s, dy.to(gpu), w.to(gpu), None)
    assert "conv_patch_dgrad" in spy and "gemm" not in spy, spy
    ref = dgrad64(dy, w, s)
    assert float(ref.max()) < 2 ** 24
    assert torch.equal(dx.cpu(), ref.to(torch.float32).to(BF16))
