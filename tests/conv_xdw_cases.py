"""Shared cases, inputs, fp64 oracle and error bounds of tests/test_conv_xdw.py (CPU) and
tests/test_conv_xdw_gpu.py (csrc/kernels/conv_xdw.hip).  Nothing here calls the code under test.

The oracle is ``torch.nn.functional`` in float64 on the very bf16 values the code under test reads.
Cases ``(N, H, W, C, R, S, sh, sw, ph, pw, dh, dw)``: the kernels' tiles are 32 channels x (images x
rows x at most 32 columns) of at most 512 pixels (256 for the weight gradient), so 72 channels are
two whole channel tiles and a ragged third, 3 x 19 x 35 is 2 x 2 ragged pixel tiles (18 weight-
gradient slabs), and the 9 x 9 stride-2 case puts both images into one tile.  Inputs as in
tests/conv_dw_cases.py.  Bounds from the number formats (u32 = 2^-24, u16 = 2^-8; A, S: the same
computation on absolute values): forward and data gradient, stored as bf16, ``u16 |ref| + 2 (R S + 1)
u32 A`` (one rounding to bf16 plus an fp32 sum of at most R S + 1 exact products in any order, doubled
for the higher-order terms); dw and db, stored as fp32, ``1.01 M u32 S`` with M = N P Q terms, and
``1.01 (M + 1) u32 (S + |prefill|)`` when accumulated onto a prefill.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

from conv_dw_cases import BF16, F64, PREFILL, U16, U32, _nchw, _nhwc, worst  # noqa: F401
from sparknet_amd.ops.spec import ConvSpec

CASES = (
    (1, 1, 1, 8, 5, 5, 1, 1, 2, 2, 1, 1),      # only the centre tap is in range
    (2, 9, 10, 16, 7, 7, 1, 1, 3, 3, 1, 1),
    (2, 9, 9, 8, 5, 5, 2, 2, 2, 2, 1, 1),      # odd size, both parities
    (2, 10, 9, 8, 5, 5, 2, 1, 1, 2, 1, 1),     # the two strides differ
    (2, 8, 8, 8, 7, 7, 2, 2, 0, 0, 1, 1),      # the largest patch
    (2, 6, 9, 8, 1, 7, 1, 1, 0, 3, 1, 1),
    (2, 9, 6, 8, 7, 1, 1, 1, 3, 0, 1, 1),
    (2, 9, 9, 8, 3, 3, 1, 1, 2, 2, 2, 2),      # dilated
    (1, 8, 9, 8, 3, 2, 1, 1, 3, 0, 3, 1),      # extent 7 by dilation, dilations differ
    (2, 4, 4, 8, 5, 5, 1, 1, 4, 4, 1, 1),      # output larger than input
    (3, 5, 6, 72, 5, 5, 1, 1, 2, 2, 1, 1),     # ragged, more than one channel tile
    (3, 19, 35, 16, 5, 5, 1, 1, 2, 2, 1, 1),   # several ragged pixel tiles and weight-gradient slabs
)
IDS = ["x".join(map(str, c)) for c in CASES]
MNASNET_LIKE = CASES[2]


def spec(case) -> ConvSpec:
    N, H, W, C, R, S, sh, sw, ph, pw, dh, dw = case
    return ConvSpec(N, H, W, C, C, R, S, sh, sw, ph, pw, dh, dw, C)


@functools.lru_cache(maxsize=None)
def inputs(case) -> dict:
    """x [N,H,W,C], dy [N,P,Q,C], gate [N,H,W,C], w [C,R,S,1] in bf16; bias [C] in fp32."""
    s = spec(case)
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    rn = lambda *shape: torch.randn(*shape, generator=g)
    gate = rn(s.N, s.H, s.W, s.C)
    gate[torch.rand(gate.shape, generator=g) < 0.05] = 0.0
    return {"x": rn(s.N, s.H, s.W, s.C).to(BF16), "dy": rn(s.N, s.P, s.Q, s.C).to(BF16),
            "w": (0.2 * rn(s.C, s.R, s.S, 1)).to(BF16), "bias": rn(s.C), "gate": gate.to(BF16)}


def _kw(s):
    return dict(stride=(s.sh, s.sw), padding=(s.ph, s.pw), dilation=(s.dh, s.dw), groups=s.C)


def forward64(x, w, bias, s, relu, absolute=False):
    xn, wo = _nchw(x), w.to(F64).reshape(s.C, 1, s.R, s.S)
    b = bias.to(F64) if bias is not None else None
    if absolute:
        xn, wo, b = xn.abs(), wo.abs(), b.abs() if b is not None else None
    y = F.conv2d(xn, wo, b, **_kw(s))
    return _nhwc(F.relu(y) if relu and not absolute else y)


def dgrad64(dy, w, gate, s, absolute=False):
    dyn, wo = _nchw(dy), w.to(F64).reshape(s.C, 1, s.R, s.S)
    if absolute:
        dyn, wo = dyn.abs(), wo.abs()
    dx = _nhwc(torch.nn.grad.conv2d_input((s.N, s.C, s.H, s.W), wo, dyn, **_kw(s)))
    return dx * (gate.to(F64) > 0) if gate is not None else dx


def wgrad64(dy, x, s, absolute=False):
    """fp64 (dw [C,R,S,1], db [C])."""
    dyn, xn = _nchw(dy), _nchw(x)
    if absolute:
        dyn, xn = dyn.abs(), xn.abs()
    dw = torch.nn.grad.conv2d_weight(xn, (s.C, 1, s.R, s.S), dyn, **_kw(s))
    return dw.permute(0, 2, 3, 1).contiguous(), dyn.sum(dim=(0, 2, 3))


def _io_bound(s, ref, A):
    return ref, U16 * ref.abs() + 2 * (s.R * s.S + 1) * U32 * A


@functools.lru_cache(maxsize=None)
def forward_bound(case, bias, relu):
    i, s = inputs(case), spec(case)
    b = i["bias"] if bias else None
    return _io_bound(s, forward64(i["x"], i["w"], b, s, relu), forward64(i["x"], i["w"], b, s, False, absolute=True))


@functools.lru_cache(maxsize=None)
def dgrad_bound(case, gate):
    i, s = inputs(case), spec(case)
    return _io_bound(s, dgrad64(i["dy"], i["w"], i["gate"] if gate else None, s),
                     dgrad64(i["dy"], i["w"], None, s, absolute=True))


@functools.lru_cache(maxsize=None)
def wgrad_bound(case, prefill=None):
    """((dw ref, dw bound), (db ref, db bound)); prefill: what the buffers held when accumulated onto."""
    i, s = inputs(case), spec(case)
    dw, db = wgrad64(i["dy"], i["x"], s)
    Sw, Sb = wgrad64(i["dy"], i["x"], s, absolute=True)
    M = s.N * s.P * s.Q
    if prefill is not None:
        dw, db, Sw, Sb, M = dw + prefill, db + prefill, Sw + abs(prefill), Sb + abs(prefill), M + 1
    return (dw, 1.01 * M * U32 * Sw), (db, 1.01 * M * U32 * Sb)
