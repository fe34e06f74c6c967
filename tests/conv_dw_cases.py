"""Shared cases, inputs, fp64 oracle, mutants and error bounds of tests/test_conv_dw.py (CPU) and
tests/test_conv_dw_gpu.py (csrc/kernels/conv_dw.hip: the depthwise 3x3 forward, data gradient
and weight / bias gradient).

Nothing here calls the code under test.  The oracle is ``torch.nn.functional`` in float64 on
float64 copies of the very bf16 values the code under test reads, on an explicitly padded input,
so that each mutant below is one changed argument of the same computation.

Cases ``(N, H, W, C, sh, sw, ph, pw)``: the smallest shapes at which the kernels can go wrong —
a single pixel whose only in-range tap is the centre, strides 1 and 2 and two that differ, pads 0
to 2 (output larger than input), a ragged channel tile (40 channels = 5 lanes of a tile of 8),
more than one channel-group block (520 channels = 65 lanes, a block holds 64), and one shape
with several weight-gradient slabs and a strip tail along Q (Q = 17 = 4 strips of 4 + 1).

Inputs are seeded by the case: x and dy ~ N(0, 1), w ~ 0.2 N(0, 1), all rounded to bf16; the
bias ~ N(0, 1) in fp32 (the layer's bias blob is fp32 on the device); the gate is a random-sign
tensor with a few exact zeros (dx is zeroed where gate <= 0).

Error bounds (from the number formats and the summation shapes, never from a kernel output);
u32 = 2^-24 and u16 = 2^-8 are the unit roundoffs of fp32 and bf16, and the abs-oracle is the
same computation on absolute values:

* forward, stored as bf16: ``|got - ref| <= u16 |ref| + 16 u32 A`` with
  ``A = conv(|x|, |w|) + |bias|``.  The first term is the one rounding of the result to bf16, the
  second the fp32 accumulation of at most 10 terms (9 exact bf16 x bf16 products and the bias;
  16 > 10 (1 + u16) leaves room for the rounding being relative to the computed value, and
  for ReLU, which is 1-Lipschitz).
* data gradient, stored as bf16: the same form with dy and w in place of x and w.
* dw and db, stored as fp32: ``|got - ref| <= 1.01 M u32 S`` with ``M = N P Q`` the number of
  summed terms and ``S`` the abs-oracle sum.  Products of two bf16 numbers are exact in fp32, so
  the result is a sum of M exact terms, and a sum of M fp32 terms in ANY order errs by at most
  (M - 1) u32 S to first order; 1.01 covers the higher orders.  Accumulating onto a pre-filled
  buffer is one more term of that sum: ``1.01 (M + 1) u32 (S + |prefill|)``.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

from sparknet_amd.ops.spec import ConvSpec

CASES = (
    (1, 1, 1, 8, 1, 1, 1, 1),      # only the centre tap is in range
    (2, 2, 2, 8, 2, 2, 1, 1),
    (2, 7, 7, 16, 1, 1, 1, 1),
    (2, 8, 8, 24, 2, 2, 1, 1),
    (1, 9, 5, 8, 2, 2, 0, 0),
    (3, 5, 6, 40, 1, 1, 0, 0),     # ragged channel tile
    (2, 6, 6, 8, 1, 1, 2, 2),      # output larger than input
    (2, 9, 8, 8, 2, 1, 0, 1),      # the two strides differ
    (2, 4, 4, 520, 1, 1, 1, 1),    # more than one channel-group block
    (5, 33, 17, 16, 1, 1, 1, 1),   # several weight-gradient slabs, a strip tail in Q
)
LARGEST = CASES[-1]
STRIDES_DIFFER = CASES[7]
IDS = ["x".join(map(str, c)) for c in CASES]

U32 = 2.0 ** -24
U16 = 2.0 ** -8
PREFILL = 7.0
F64 = torch.float64
BF16 = torch.bfloat16


def spec(case) -> ConvSpec:
    N, H, W, C, sh, sw, ph, pw = case
    return ConvSpec(N, H, W, C, C, 3, 3, sh, sw, ph, pw, 1, 1, C)


@functools.lru_cache(maxsize=None)
def inputs(case) -> dict:
    """x [N,H,W,C], dy [N,P,Q,C], gate [N,H,W,C], w [C,3,3,1] in bf16; bias [C] in fp32."""
    s = spec(case)
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    rn = lambda *shape: torch.randn(*shape, generator=g)
    gate = rn(s.N, s.H, s.W, s.C)
    gate[torch.rand(gate.shape, generator=g) < 0.05] = 0.0
    return {"x": rn(s.N, s.H, s.W, s.C).to(BF16), "dy": rn(s.N, s.P, s.Q, s.C).to(BF16),
            "w": (0.2 * rn(s.C, 3, 3, 1)).to(BF16), "bias": rn(s.C), "gate": gate.to(BF16)}


def _nchw(t):
    return t.to(F64).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _w(w, drop_tap=False):
    wo = w.to(F64).reshape(-1, 1, 3, 3).clone()
    if drop_tap:
        wo[:, :, 1, 2] = 0.0
    return wo


def forward64(x, w, bias, s, relu, *, absolute=False, drop_tap=False, ph_off=0, swap_strides=False,
              skip_last_row=False):
    """fp64 forward, NHWC.  The keyword mutants: tap (1, 2) dropped; the input read one row too
    high (pad ph + 1 above, ph - 1 below); sh and sw swapped (another output shape); the last
    output row left at zero."""
    xn, wo = _nchw(x), _w(w, drop_tap)
    b = bias.to(F64) if bias is not None else None
    if absolute:
        xn, wo, b = xn.abs(), wo.abs(), b.abs() if b is not None else None
    xp = F.pad(xn, (s.pw, s.pw, s.ph + ph_off, s.ph - ph_off))
    stride = (s.sw, s.sh) if swap_strides else (s.sh, s.sw)
    y = F.conv2d(xp, wo, b, stride=stride, groups=s.C)
    if relu and not absolute:
        y = F.relu(y)
    if skip_last_row:
        y[:, :, -1] = 0.0
    return _nhwc(y)


def dgrad64(dy, w, gate, s, *, absolute=False, drop_tap=False, ignore_gate=False):
    """fp64 data gradient, NHWC, zeroed where gate <= 0."""
    dyn, wo = _nchw(dy), _w(w, drop_tap)
    if absolute:
        dyn, wo = dyn.abs(), wo.abs()
    dx = torch.nn.grad.conv2d_input((s.N, s.C, s.H, s.W), wo, dyn, stride=(s.sh, s.sw), padding=(s.ph, s.pw),
                                    groups=s.C)
    dx = _nhwc(dx)
    if gate is not None and not ignore_gate:
        dx = dx * (gate.to(F64) > 0)
    return dx


def wgrad64(dy, x, s, *, absolute=False, drop_slab=False):
    """fp64 (dw [C,3,3,1], db [C]).  drop_slab: the last image's contribution (the last output
    row's when N == 1) is missing from dw, as if one slab of partials were not summed."""
    dyn, xn = _nchw(dy), _nchw(x)
    if absolute:
        dyn, xn = dyn.abs(), xn.abs()
    db = dyn.sum(dim=(0, 2, 3))
    if drop_slab:
        dyn = dyn.clone()
        if s.N > 1:
            dyn[-1] = 0.0
        else:
            dyn[:, :, -1] = 0.0
    dw = torch.nn.grad.conv2d_weight(xn, (s.C, 1, 3, 3), dyn, stride=(s.sh, s.sw), padding=(s.ph, s.pw), groups=s.C)
    return dw.permute(0, 2, 3, 1).contiguous(), db


# --- bounds ---------------------------------------------------------------------------------

def forward_bound(case, bias, relu):
    i, s = inputs(case), spec(case)
    b = i["bias"] if bias else None
    ref = forward64(i["x"], i["w"], b, s, relu)
    A = forward64(i["x"], i["w"], b, s, False, absolute=True)
    return ref, U16 * ref.abs() + 16 * U32 * A


def dgrad_bound(case, gate):
    i, s = inputs(case), spec(case)
    g = i["gate"] if gate else None
    ref = dgrad64(i["dy"], i["w"], g, s)
    A = dgrad64(i["dy"], i["w"], None, s, absolute=True)
    return ref, U16 * ref.abs() + 16 * U32 * A


def wgrad_bound(case, prefill=None):
    """((dw ref, dw bound), (db ref, db bound)); prefill: the value the buffers held when the
    gradient was accumulated onto them (None: stored)."""
    i, s = inputs(case), spec(case)
    dw, db = wgrad64(i["dy"], i["x"], s)
    Sw, Sb = wgrad64(i["dy"], i["x"], s, absolute=True)
    M = s.N * s.P * s.Q
    if prefill is not None:
        dw, db, Sw, Sb, M = dw + prefill, db + prefill, Sw + abs(prefill), Sb + abs(prefill), M + 1
    return (dw, 1.01 * M * U32 * Sw), (db, 1.01 * M * U32 * Sb)


def worst(got, ref, bound) -> float:
    """Largest |got - ref| / bound over the elements (0 where both vanish): <= 1 passes."""
    d = (got.detach().to(F64).cpu().reshape(ref.shape) - ref).abs()
    ratio = torch.where(d == 0, torch.zeros_like(d), d / bound)
    return float(ratio.max()) if ratio.numel() else 0.0
