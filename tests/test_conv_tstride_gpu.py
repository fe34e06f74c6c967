"""The phase-decomposed stride-2 data gradient (csrc/kernels/conv_tstride.hip) against an fp64
oracle: ``torch.nn.grad.conv2d_input`` on float64 copies of the very bf16 values the kernel reads.

Bound, of the form tests/conv_grouped_cases.py derives: the result is one bf16 rounding of an fp32
sum, in any order, of at most T = ceil(R/2) ceil(S/2) K products (the taps of one phase) that are
exact in fp32, so ``|got - ref| <= 2^-8 |ref| + 1.01 (T + 1) 2^-24 A`` with A the same gradient of
|dy| and |w|; where no dy pixel reaches, ref and bound are 0 and only an exact zero passes.  dx is
pre-filled with NaN: an element the launch misses fails.  The launcher is called directly, so shapes
below the dispatch's pixel bound are reachable.  Cases ``(N, H, W, C, K, R, S, ph, pw)``, stride 2."""
import functools
import zlib

import pytest
import torch

from sparknet_amd import proto
from sparknet_amd.core.net import Net
from sparknet_amd.ops.spec import ConvSpec

pytestmark = pytest.mark.gpu

CASES = (
    (1, 1, 1, 8, 8, 1, 1, 0, 0),        # a single pixel
    (2, 7, 7, 8, 8, 1, 1, 0, 0),        # odd image, three empty phases, one partial K chunk
    (2, 8, 8, 72, 40, 1, 1, 0, 0),      # C-tile and K-chunk tails
    (2, 6, 6, 16, 32, 2, 2, 0, 0),      # one tap per phase
    (2, 8, 8, 16, 32, 3, 3, 1, 1),
    (1, 9, 9, 16, 32, 3, 3, 1, 1),      # odd image
    (1, 8, 8, 16, 32, 3, 3, 0, 0),      # last row and column reached by no dy: zeros
    (2, 10, 12, 16, 32, 4, 4, 1, 1),    # non-square image
    (1, 8, 9, 16, 32, 3, 3, 1, 0),      # the pads differ per axis
    (2, 9, 10, 16, 32, 2, 3, 0, 1),     # R != S: the tap index and the two patch halos differ
    (3, 37, 21, 72, 64, 3, 3, 1, 1),    # several cell tiles both ways, ragged edges, halos across tiles, several images
)
F64, BF16 = torch.float64, torch.bfloat16


def spec(case) -> ConvSpec:
    N, H, W, C, K, R, S, ph, pw = case
    return ConvSpec(N, H, W, C, K, R, S, 2, 2, ph, pw, 1, 1, 1)


def bound(dy, w, s, gate=None):
    """(fp64 reference, elementwise bound) for NHWC bf16 dy, w [K][R][S][C] and an optional gate."""
    d, k = dy.cpu().to(F64).permute(0, 3, 1, 2), w.cpu().to(F64).permute(0, 3, 1, 2)
    grad = lambda a, b: torch.nn.grad.conv2d_input((s.N, s.C, s.H, s.W), b, a, stride=2,
                                                   padding=(s.ph, s.pw)).permute(0, 2, 3, 1)
    ref, A = grad(d, k), grad(d.abs(), k.abs())
    if gate is not None:
        ref = ref * (gate.cpu().to(F64) > 0)
    terms = -(-s.R // 2) * -(-s.S // 2) * s.K
    return ref, 2.0 ** -8 * ref.abs() + 1.01 * (terms + 1) * 2.0 ** -24 * A


@functools.lru_cache(maxsize=None)
def inputs(case):
    s, g = spec(case), torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    gate = torch.randn(s.N, s.H, s.W, s.C, generator=g)
    gate[torch.rand(gate.shape, generator=g) < 0.05] = 0.0
    dy = torch.randn(s.N, s.P, s.Q, s.K, generator=g).to(BF16)
    w = (0.2 * torch.randn(s.K, s.R, s.S, s.C, generator=g)).to(BF16)
    return dy, w, gate.to(BF16)


def assert_within(got, ref, bnd, what):
    assert not torch.isnan(got).any(), f"{what}: elements the launch did not write"
    ratio = ((got.cpu().to(F64) - ref).abs() / bnd.clamp_min(1e-300)).max().item()
    print(what, "worst |got - ref| / bound", ratio)
    assert ratio <= 1.0, what


@pytest.mark.parametrize("gated", (False, True), ids=("plain", "gate"))
@pytest.mark.parametrize("case", CASES, ids=["x".join(map(str, c)) for c in CASES])
def test_launcher_against_fp64(case, gated, gpu):
    from sparknet_amd.ops import hip
    s = spec(case)
    dy, w, gate = (t.to(gpu) if gated or i < 2 else None for i, t in enumerate(inputs(case)))
    dx = torch.full((s.N, s.H, s.W, s.C), float("nan"), dtype=BF16, device=gpu)
    hip.call(hip.TSTRIDE_DGRAD, dy, w, gate, dx, s.N, s.H, s.W, s.C, s.K, s.R, s.S, s.ph, s.pw)
    ref, bnd = bound(dy, w, s, gate)
    assert_within(dx, ref, bnd, f"{case} gate={gated}")


def _net(layer, shape, gpu):
    dims = " ".join(f"dim: {d}" for d in shape)
    txt = (f'name: "t" force_backward: true layer {{ name: "in" type: "Input" top: "x" java_data_param {{ shape {{ {dims} }} }} }}'
           f' layer {{ name: "l" bottom: "x" top: "y" {layer} }}')
    return Net(proto.parse_prototxt(txt), phase=proto.TRAIN, seed=7, device=gpu)


@pytest.fixture
def launches(monkeypatch):
    from sparknet_amd.ops import hip
    names, native = [], hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (names.append(name), native(name, *a))[1])
    return names


def test_deconvolution_forward(gpu, launches, monkeypatch):
    """4x4 / 2 pad 1 up-sampling, 32 -> 16 channels, with bias: the layer's forward is this data gradient
    plus a separate fp32 bias add rounded to bf16 once more, |dx + bias| <= |ref + bias| + bound."""
    from sparknet_amd.ops import hip
    monkeypatch.delenv("SN_FEATURES", raising=False)
    net = _net('type: "Deconvolution" convolution_param { num_output: 16 kernel_size: 4 stride: 2 pad: 1 '
               'weight_filler { type: "gaussian" std: 0.2 } bias_filler { type: "gaussian" } }', (2, 32, 9, 9), gpu)
    layer, x = net.layers[-1], net.blob_by_name("x")
    x.set_nchw(torch.randn(2, 32, 9, 9, generator=torch.Generator().manual_seed(1)).to(BF16).float())
    net.forward()
    assert launches.count(hip.TSTRIDE_DGRAD) == 1 and "col2im" not in launches, launches
    ref, bnd = bound(x.data.to(BF16), layer.weight.compute, ConvSpec(2, 18, 18, 16, 32, 4, 4, 2, 2, 1, 1, 1, 1, 1))
    ref = ref + layer.bias.data.cpu().to(F64)
    assert_within(net.blob_by_name("y").data, ref, bnd + 2.0 ** -8 * (ref.abs() + bnd), "deconvolution")


@pytest.mark.parametrize("switch", ("", "conv_tstride=0"), ids=("on", "off"))
def test_convolution_backward(switch, gpu, launches, monkeypatch):
    """3x3 / 2 pad 1, 16 -> 32 channels: the new route and the generic one, to the same oracle and bound."""
    from sparknet_amd.ops import hip
    monkeypatch.setenv("SN_FEATURES", switch)
    net = _net('type: "Convolution" convolution_param { num_output: 32 kernel_size: 3 stride: 2 pad: 1 '
               'weight_filler { type: "gaussian" std: 0.2 } }', (2, 16, 16, 16), gpu)
    g = torch.Generator().manual_seed(2)
    net.blob_by_name("x").set_nchw(torch.randn(2, 16, 16, 16, generator=g))
    net.forward()
    y = net.blob_by_name("y")
    y.set_nchw(torch.randn(2, 32, 8, 8, generator=g), diff=True)
    del launches[:]
    net.layers[-1].backward(net.top_vecs[-1], [True], net.bottom_vecs[-1])
    assert (hip.TSTRIDE_DGRAD in launches) == (switch == "") and ("col2im" in launches) == (switch != ""), launches
    ref, bnd = bound(y.diff.to(BF16), net.layers[-1].weight.compute, ConvSpec(2, 16, 16, 16, 32, 3, 3, 2, 2, 1, 1, 1, 1, 1))
    assert_within(net.blob_by_name("x").diff, ref, bnd, f"convolution backward, SN_FEATURES={switch!r}")
