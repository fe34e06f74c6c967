"""Shared cases, inputs, fp64 oracle, mutants and error bounds of tests/test_conv_grouped.py (CPU)
and tests/test_conv_grouped_gpu.py (csrc/kernels/conv_grouped.hip: the narrow-group 3x3 forward,
data gradient and weight gradient, Cg == Kg channels per group).

Nothing here calls the code under test.  The oracle is ``torch.nn.functional`` in float64 with
``groups = C // Cg`` on float64 copies of the very bf16 values the code under test reads, on an
explicitly padded input, so that each mutant below is one changed argument of the same computation.

Cases ``(N, H, W, C, Cg, sh, sw, ph, pw)``: the smallest shapes at which the kernels can go wrong —
a single pixel whose only in-range tap is the centre, a 2x2 image at stride 2, every routed width
(4, 8, 16) at stride 1 and at stride 2, strides that differ, pad 0 and pad 2 (output larger than
input), 15 output pixels (one short of a 16-pixel tile), two bundles of 16 channels, eight bundles
(two blocks of four), and one shape with several weight-gradient slabs (2805 pixels = 88 chunks
of 32, the last one ragged) and a ragged last pixel tile.

Inputs are seeded by the case: x and dy ~ N(0, 1), w ~ 0.2 N(0, 1), all rounded to bf16; the
bias ~ N(0, 1) in fp32; the gate is a random-sign tensor with a few exact zeros (dx is zeroed where
gate <= 0).  Weights are [K][3][3][Cg] as the layer holds them.

Error bounds (from the number formats and the summation shapes, never from the new kernels'
output); u32 = 2^-24 and u16 = 2^-8 are the unit roundoffs of fp32 and bf16, and the abs-oracle
is the same computation on absolute values:

* forward, stored as bf16: ``|got - ref| <= u16 |ref| + c T u32 A`` with ``T = 9 Cg + 1`` terms
  (9 Cg exact bf16 x bf16 products and the bias) and ``A = conv(|x|, |w|) + |bias|``.  The first
  term is the one rounding of the result to bf16, the second the fp32 accumulation of T terms in
  any order ((T - 1) u32 A to first order).
* data gradient, stored as bf16: the same form with dy and w in place of x and w.
* dw and db, stored as fp32: ``|got - ref| <= c' (M + 1) u32 S`` with ``M = N P Q`` the number of
  summed terms and ``S`` the abs-oracle sum; accumulating onto a pre-filled buffer is one more
  term: ``c' (M + 2) u32 (S + |prefill|)``.

``c = c' = 1.01`` is the any-order fp32 summation bound with room for the higher orders.  Whether
the 32-term sum inside v_mfma_f32_16x16x32_bf16 rounds like a tree of IEEE additions is not
documented, so the constants were checked against the path these kernels replace, not against the
kernels: the implicit grouped GEMM (SN_FEATURES=conv_grouped=0), which uses the same instruction,
on the Cg = 8 and Cg = 16 cases with c = c' = 1.  MEASURED_PARENT_RATIOS below holds the worst
|got - ref| / bound it reached per product; all are below 1, so the constants stay at 1.01.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

from sparknet_amd.ops.spec import ConvSpec

CASES = (
    (1, 1, 1, 16, 4, 1, 1, 1, 1),     # only the centre tap is in range
    (2, 2, 2, 16, 8, 2, 2, 1, 1),     # a 2x2 image at stride 2
    (2, 7, 7, 32, 4, 1, 1, 1, 1),     # two bundles
    (2, 8, 8, 16, 4, 2, 2, 1, 1),
    (2, 7, 7, 16, 8, 1, 1, 1, 1),
    (2, 8, 8, 32, 8, 2, 2, 1, 1),
    (2, 7, 7, 16, 16, 1, 1, 1, 1),
    (2, 8, 8, 32, 16, 2, 2, 1, 1),
    (2, 9, 8, 16, 4, 2, 1, 0, 1),     # the two strides differ
    (1, 5, 7, 16, 8, 1, 1, 0, 0),     # pad 0, P Q = 15: one short of a pixel tile
    (2, 6, 6, 16, 4, 1, 1, 2, 2),     # output larger than input
    (1, 4, 4, 128, 4, 1, 1, 1, 1),    # eight bundles: two blocks of four
    (5, 33, 17, 32, 4, 1, 1, 1, 1),   # several weight-gradient slabs, ragged last chunk and tile
)
LARGEST = CASES[-1]
STRIDES_DIFFER = CASES[8]
IDS = ["x".join(map(str, c)) for c in CASES]

U32 = 2.0 ** -24
U16 = 2.0 ** -8
PREFILL = 7.0
F64 = torch.float64
BF16 = torch.bfloat16

# worst |got - ref| / bound of the conv_grouped=0 path with c = c' = 1, over the Cg = 8 and 16 cases
MEASURED_PARENT_RATIOS = {"forward": 0.989, "dgrad": 0.978, "wgrad": 0.208}
C_SUM = 1.01   # c and c' of the bounds above


def spec(case) -> ConvSpec:
    N, H, W, C, Cg, sh, sw, ph, pw = case
    return ConvSpec(N, H, W, C, C, 3, 3, sh, sw, ph, pw, 1, 1, C // Cg)


@functools.lru_cache(maxsize=None)
def inputs(case) -> dict:
    """x [N,H,W,C], dy [N,P,Q,C], gate [N,H,W,C], w [C,3,3,Cg] in bf16; bias [C] in fp32."""
    s = spec(case)
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    rn = lambda *shape: torch.randn(*shape, generator=g)
    gate = rn(s.N, s.H, s.W, s.C)
    gate[torch.rand(gate.shape, generator=g) < 0.05] = 0.0
    return {"x": rn(s.N, s.H, s.W, s.C).to(BF16), "dy": rn(s.N, s.P, s.Q, s.C).to(BF16),
            "w": (0.2 * rn(s.C, 3, 3, s.Cg)).to(BF16), "bias": rn(s.C), "gate": gate.to(BF16)}


def _nchw(t):
    return t.to(F64).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _w(w, drop_tap=False, merge=False):
    """[K][3][3][Cg] -> fp64 [K][Cg][3][3].  merge: groups of 16 instead, every output channel
    reading its weights from all 16 / Cg groups of its bundle (the block-diagonal mask missing)."""
    wo = w.to(F64).permute(0, 3, 1, 2).clone()
    if drop_tap:
        wo[:, :, 1, 2] = 0.0
    if merge:
        wo = wo.repeat(1, 16 // wo.shape[1], 1, 1)
    return wo


def forward64(x, w, bias, s, relu, *, absolute=False, drop_tap=False, merge=False, ph_off=0, swap_strides=False,
              skip_last_row=False):
    """fp64 forward, NHWC.  The keyword mutants: tap (1, 2) dropped; groups merged into bundles
    of 16; the input read one row too high (pad ph + 1 above, ph - 1 below); sh and sw swapped
    (another output shape); the last output row left at zero."""
    xn, wo = _nchw(x), _w(w, drop_tap, merge)
    b = bias.to(F64) if bias is not None else None
    if absolute:
        xn, wo, b = xn.abs(), wo.abs(), b.abs() if b is not None else None
    top, bottom = s.ph + ph_off, s.ph - ph_off
    xp = F.pad(xn, (s.pw, s.pw, max(top, 0), max(bottom, 0)))
    if bottom < 0:
        xp = xp[:, :, :bottom]
    stride = (s.sw, s.sh) if swap_strides else (s.sh, s.sw)
    y = F.conv2d(xp, wo, b, stride=stride, groups=s.C // 16 if merge else s.groups)
    if relu and not absolute:
        y = F.relu(y)
    if skip_last_row:
        y[:, :, -1] = 0.0
    return _nhwc(y)


def dgrad64(dy, w, gate, s, *, absolute=False, drop_tap=False, merge=False, ignore_gate=False):
    """fp64 data gradient, NHWC, zeroed where gate <= 0."""
    dyn, wo = _nchw(dy), _w(w, drop_tap, merge)
    if absolute:
        dyn, wo = dyn.abs(), wo.abs()
    dx = torch.nn.grad.conv2d_input((s.N, s.C, s.H, s.W), wo, dyn, stride=(s.sh, s.sw), padding=(s.ph, s.pw),
                                    groups=s.C // 16 if merge else s.groups)
    dx = _nhwc(dx)
    if gate is not None and not ignore_gate:
        dx = dx * (gate.to(F64) > 0)
    return dx


def wgrad64(dy, x, s, *, absolute=False, drop_slab=False):
    """fp64 (dw [C,3,3,Cg], db [C]).  drop_slab: the last image's contribution (the last output
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
    dw = torch.nn.grad.conv2d_weight(xn, (s.C, s.Cg, 3, 3), dyn, stride=(s.sh, s.sw), padding=(s.ph, s.pw),
                                     groups=s.groups)
    return dw.permute(0, 2, 3, 1).contiguous(), db


# --- bounds ---------------------------------------------------------------------------------

def _terms(case):
    return 9 * case[4] + 1


@functools.lru_cache(maxsize=None)
def forward_bound(case, bias, relu, c=C_SUM):
    i, s = inputs(case), spec(case)
    b = i["bias"] if bias else None
    ref = forward64(i["x"], i["w"], b, s, relu)
    A = forward64(i["x"], i["w"], b, s, False, absolute=True)
    return ref, U16 * ref.abs() + c * _terms(case) * U32 * A


@functools.lru_cache(maxsize=None)
def dgrad_bound(case, gate, c=C_SUM):
    i, s = inputs(case), spec(case)
    g = i["gate"] if gate else None
    ref = dgrad64(i["dy"], i["w"], g, s)
    A = dgrad64(i["dy"], i["w"], None, s, absolute=True)
    return ref, U16 * ref.abs() + c * _terms(case) * U32 * A


@functools.lru_cache(maxsize=None)
def wgrad_bound(case, prefill=None, c=C_SUM):
    """((dw ref, dw bound), (db ref, db bound)); prefill: the value the buffers held when the
    gradient was accumulated onto them (None: stored)."""
    i, s = inputs(case), spec(case)
    dw, db = wgrad64(i["dy"], i["x"], s)
    Sw, Sb = wgrad64(i["dy"], i["x"], s, absolute=True)
    M = s.N * s.P * s.Q
    if prefill is not None:
        dw, db, Sw, Sb, M = dw + prefill, db + prefill, Sw + abs(prefill), Sb + abs(prefill), M + 1
    return (dw, c * (M + 1) * U32 * Sw), (db, c * (M + 1) * U32 * Sb)


def worst(got, ref, bound) -> float:
    """Largest |got - ref| / bound over the elements (0 where both vanish): <= 1 passes."""
    d = (got.detach().to(F64).cpu().reshape(ref.shape) - ref).abs()
    ratio = torch.where(d == 0, torch.zeros_like(d), d / bound)
    return float(ratio.max()) if ratio.numel() else 0.0
