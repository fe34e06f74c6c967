"""Shared cases, inputs, fp64 oracle and error bounds of tests/test_conv_updw_gpu.py and tests/test_fcn.py
(csrc/kernels/conv_updw.hip: depthwise transposed convolution).  Nothing here calls the code under test.

The oracle is ``torch.nn.functional.conv_transpose2d`` and its autograd in float64 with ``groups=C`` on the
very bf16 values the kernels read.  Cases ``(N, P, Q, C, R, S, sh, sw, ph, pw)``, P x Q the deconvolution's
INPUT.  The kernels' tiles: 32 channels; forward about 16 x 32 output pixels (16 / sh x 32 / sw cells); data
and weight gradient 8 x 16 input cells, the weight gradient in at most 1024 slabs of tiles.  So the last case,
2 x 19 x 33 x 44 at 3x3 / 2, is a whole and a ragged channel tile (12 of 32) on the unaligned lanes, whose
runs are not contiguous there, 3 x 3 ragged cell tiles per image in every kernel and 18 weight-gradient slabs
per channel tile.  Inputs as in tests/conv_dw_cases.py.

Bounds from the number formats (u32 = 2^-24, u16 = 2^-8; A, S: the same computation on absolute values),
with T = ceil(R / sh) ceil(S / sw) the most taps an output pixel has: forward, stored as bf16, ``u16 |ref| +
2 (T + 1) u32 A`` (one rounding to bf16 plus an fp32 sum of at most T exact products and the bias in any
order, doubled for the higher-order terms); bottom gradient ``u16 |ref| + 2 (R S + 1) u32 A``; dw, stored as
fp32, ``1.01 M u32 S`` with M = N P Q input cells, db the same with M = N H W; ``M + 1`` and ``S +
|prefill|`` when accumulated onto a prefill.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

from conv_dw_cases import BF16, F64, PREFILL, U16, U32, worst  # noqa: F401
from sparknet_amd.ops.spec import ConvSpec

CASES = (
    (1, 1, 1, 8, 4, 4, 2, 2, 1, 1),        # one cell, one tap per output
    (2, 5, 6, 21, 4, 4, 2, 2, 0, 0),       # upscore2, C = 21 on the unaligned lanes
    (2, 4, 5, 21, 16, 16, 8, 8, 0, 0),     # upscore8, the largest window and stride
    (2, 5, 4, 8, 5, 5, 3, 3, 1, 1),        # 2f - f % 2 at f = 3: phases with unequal tap counts
    (2, 4, 6, 16, 4, 6, 2, 3, 1, 0),       # strides, windows and pads differ per axis
    (1, 4, 4, 8, 2, 2, 4, 4, 0, 0),        # window smaller than the stride: phases with no tap
    (2, 5, 5, 8, 3, 3, 1, 1, 1, 1),        # stride 1
    (2, 6, 6, 8, 4, 4, 2, 2, 3, 3),        # a pad that removes every output of the first input row
    (2, 19, 33, 44, 3, 3, 2, 2, 1, 1),     # ragged in every tile dimension, two channel tiles, several slabs
)
IDS = ["x".join(map(str, c)) for c in CASES]
UPSCORE2, UPSCORE8 = CASES[1], CASES[2]


def spec(case) -> ConvSpec:
    """The convolution top -> bottom, as DeconvolutionLayer.fwd_spec builds it."""
    N, P, Q, C, R, S, sh, sw, ph, pw = case
    return ConvSpec(N, (P - 1) * sh + R - 2 * ph, (Q - 1) * sw + S - 2 * pw, C, C, R, S, sh, sw, ph, pw, 1, 1, C)


@functools.lru_cache(maxsize=None)
def inputs(case) -> dict:
    """x [N,P,Q,C] (the bottom), dy [N,H,W,C] (the top gradient), w [C,R,S,1] in bf16; bias [C] in fp32."""
    s = spec(case)
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    rn = lambda *shape: torch.randn(*shape, generator=g)
    return {"x": rn(s.N, s.P, s.Q, s.C).to(BF16), "dy": rn(s.N, s.H, s.W, s.C).to(BF16),
            "w": (0.2 * rn(s.C, s.R, s.S, 1)).to(BF16), "bias": rn(s.C)}


@functools.lru_cache(maxsize=None)
def _oracle(case, bias, absolute):
    """fp64 (y, dx, dw [C,R,S,1], db), all NHWC, from conv_transpose2d and its autograd."""
    i, s = inputs(case), spec(case)
    f = (lambda t: t.to(F64).abs()) if absolute else (lambda t: t.to(F64))
    x = f(i["x"]).permute(0, 3, 1, 2).requires_grad_()
    w = f(i["w"]).reshape(s.C, 1, s.R, s.S).requires_grad_()
    b = f(i["bias"]).requires_grad_()
    y = F.conv_transpose2d(x, w, b if bias else None, stride=(s.sh, s.sw), padding=(s.ph, s.pw), groups=s.C)
    dy = f(i["dy"]).permute(0, 3, 1, 2)
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    return nhwc(y), nhwc(dx), dw.detach().reshape(s.C, s.R, s.S, 1), dy.sum(dim=(0, 2, 3))


def forward_bound(case, bias):
    s = spec(case)
    T = -(-s.R // s.sh) * -(-s.S // s.sw)
    ref, A = _oracle(case, bias, False)[0], _oracle(case, bias, True)[0]
    return ref, U16 * ref.abs() + 2 * (T + 1) * U32 * A


def dgrad_bound(case):
    s = spec(case)
    ref, A = _oracle(case, False, False)[1], _oracle(case, False, True)[1]
    return ref, U16 * ref.abs() + 2 * (s.R * s.S + 1) * U32 * A


def wgrad_bound(case, prefill=None):
    """((dw ref, dw bound), (db ref, db bound)); prefill: what the buffers held when accumulated onto."""
    s = spec(case)
    (_, _, dw, db), (_, _, Sw, Sb) = _oracle(case, False, False), _oracle(case, False, True)
    Mw, Mb = s.N * s.P * s.Q, s.N * s.H * s.W
    if prefill is not None:
        dw, db, Sw, Sb, Mw, Mb = dw + prefill, db + prefill, Sw + abs(prefill), Sb + abs(prefill), Mw + 1, Mb + 1
    return (dw, 1.01 * Mw * U32 * Sw), (db, 1.01 * Mb * U32 * Sb)
