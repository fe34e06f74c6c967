"""Shared cases, inputs, fp64 oracle and error bounds of tests/test_conv_gpw_gpu.py and
tests/test_shufflenet.py (csrc/kernels/conv_gpw.hip: the grouped 1x1 forward, data gradient and weight
gradient).  Nothing here calls the code under test.

The oracle is ``torch.nn.functional.conv2d`` / ``torch.nn.grad.conv2d_input`` / ``conv2d_weight`` in
float64 with ``groups``, on float64 copies of the very bf16 values the code under test reads.  Cases
``(N, H, W, C, K, groups)``; inputs as in tests/conv_grouped_cases.py (x, dy ~ N(0, 1), w ~ 0.2 N(0, 1)
in bf16, bias ~ N(0, 1) in fp32, a random-sign gate with a few exact zeros), seeded by the case.

Bounds, the forms of tests/conv_grouped_cases.py with this kernel's term counts (u32 = 2^-24, u16 =
2^-8; A, S: the same computation on absolute values): forward ``u16 |ref| + c T u32 A`` with T = Cg + 1
(Cg exact products and the bias); data gradient the same with T = Kg; dw and db ``c' (M + 1) u32 S`` with
M = N H W summed terms, one more term when accumulated onto a prefill.  c = c' = 1.01.  The constants
were checked on the route these kernels replace (SN_FEATURES=conv_gpw=0: the implicit grouped GEMM where
Cg and Kg are multiples of 8, the per-group im2col + GEMM loop otherwise), not on the kernels: the same
cases with c = c' = 1 reached at worst MEASURED_PARENT_RATIOS of the bound per product.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

from conv_grouped_cases import BF16, F64, PREFILL, U16, U32, _nchw, _nhwc, worst  # noqa: F401
from sparknet_amd.ops.spec import ConvSpec

CASES = (
    (1, 1, 1, 8, 8, 2),        # one pixel, Cg = Kg = 4: almost all padding
    (1, 5, 3, 72, 36, 3),      # 15 rows: one short of a 16-row fragment; Cg = 24, Kg = 12
    (2, 7, 7, 60, 216, 3),     # Cg = 20 (ragged reduction), Kg = 72 = 4 x 16 + 8, 98 rows (ragged tile)
    (2, 7, 7, 240, 60, 3),     # Cg = 80: two and a half reduction steps; Kg = 20
    (1, 4, 4, 96, 96, 8),      # eight groups of 12
    (2, 4, 4, 64, 128, 2),     # multiples of 8: the shapes taken from the implicit grouped GEMM
    (1, 2, 2, 960, 240, 3),    # Cg = 320, Kg = 80: the largest group's weights in LDS
    (5, 33, 17, 48, 48, 3),    # 2805 rows: several weight-gradient slabs, ragged last slab and tile
)
IDS = ["x".join(map(str, c)) for c in CASES]
ISOLATION = CASES[2]
C_SUM = 1.01
# worst |got - ref| / bound of the conv_gpw=0 routes with c = c' = 1 over CASES (one MI355X run)
MEASURED_PARENT_RATIOS = {"forward": 0.995, "dgrad": 0.996, "wgrad": 0.246}


def spec(case) -> ConvSpec:
    N, H, W, C, K, G = case
    return ConvSpec(N, H, W, C, K, 1, 1, groups=G)


@functools.lru_cache(maxsize=None)
def inputs(case) -> dict:
    """x, gate [N,H,W,C], dy [N,H,W,K], w [K,1,1,Cg] in bf16; bias [K] in fp32."""
    s = spec(case)
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    rn = lambda *shape: torch.randn(*shape, generator=g)
    gate = rn(s.N, s.H, s.W, s.C)
    gate[torch.rand(gate.shape, generator=g) < 0.05] = 0.0
    return {"x": rn(s.N, s.H, s.W, s.C).to(BF16), "dy": rn(s.N, s.H, s.W, s.K).to(BF16),
            "w": (0.2 * rn(s.K, 1, 1, s.Cg)).to(BF16), "bias": rn(s.K), "gate": gate.to(BF16)}


def forward64(x, w, bias, s, relu, absolute=False):
    xn, wo = _nchw(x), w.to(F64).permute(0, 3, 1, 2)
    b = bias.to(F64) if bias is not None else None
    if absolute:
        xn, wo, b = xn.abs(), wo.abs(), b.abs() if b is not None else None
    y = F.conv2d(xn, wo, b, groups=s.groups)
    return _nhwc(F.relu(y) if relu and not absolute else y)


def dgrad64(dy, w, gate, s, absolute=False):
    dyn, wo = _nchw(dy), w.to(F64).permute(0, 3, 1, 2)
    if absolute:
        dyn, wo = dyn.abs(), wo.abs()
    dx = _nhwc(torch.nn.grad.conv2d_input((s.N, s.C, s.H, s.W), wo, dyn, groups=s.groups))
    return dx * (gate.to(F64) > 0) if gate is not None else dx


def wgrad64(dy, x, s, absolute=False):
    """fp64 (dw [K,1,1,Cg], db [K])."""
    dyn, xn = _nchw(dy), _nchw(x)
    if absolute:
        dyn, xn = dyn.abs(), xn.abs()
    dw = torch.nn.grad.conv2d_weight(xn, (s.K, s.Cg, 1, 1), dyn, groups=s.groups)
    return dw.permute(0, 2, 3, 1).contiguous(), dyn.sum(dim=(0, 2, 3))


@functools.lru_cache(maxsize=None)
def forward_bound(case, bias, relu, c=C_SUM):
    i, s = inputs(case), spec(case)
    b = i["bias"] if bias else None
    ref = forward64(i["x"], i["w"], b, s, relu)
    return ref, U16 * ref.abs() + c * (s.Cg + 1) * U32 * forward64(i["x"], i["w"], b, s, False, absolute=True)


@functools.lru_cache(maxsize=None)
def dgrad_bound(case, gate, c=C_SUM):
    i, s = inputs(case), spec(case)
    ref = dgrad64(i["dy"], i["w"], i["gate"] if gate else None, s)
    return ref, U16 * ref.abs() + c * s.Kg * U32 * dgrad64(i["dy"], i["w"], None, s, absolute=True)


@functools.lru_cache(maxsize=None)
def wgrad_bound(case, prefill=None, c=C_SUM):
    """((dw ref, dw bound), (db ref, db bound)); prefill: what the buffers held when accumulated onto."""
    i, s = inputs(case), spec(case)
    dw, db = wgrad64(i["dy"], i["x"], s)
    Sw, Sb = wgrad64(i["dy"], i["x"], s, absolute=True)
    M = s.N * s.H * s.W
    if prefill is not None:
        dw, db, Sw, Sb, M = dw + prefill, db + prefill, Sw + abs(prefill), Sb + abs(prefill), M + 1
    return (dw, c * (M + 1) * U32 * Sw), (db, c * (M + 1) * U32 * Sb)
