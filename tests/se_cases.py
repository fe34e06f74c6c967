"""Shared cases, inputs, fp64 oracle, mutants and error bounds of tests/test_se.py (CPU) and
tests/test_se_gpu.py (csrc/kernels/se.hip: the global average pool, the per-image, per-channel
affine forward ``y = x s[n, c] + b[n, c] + r`` and its backward ``dx = dy s``,
``ds[n, c] = sum_p dy x``, ``db[n, c] = sum_p dy``).

Nothing here calls the code under test.  The oracle is the same arithmetic in float64 on float64
copies of exactly the values the code under test reads; each mutant is one keyword argument.

Cases ``(N, H, W, C)``: the smallest shapes at which the kernels can go wrong — a single pixel,
HW = 1 with two images, HW = 64 (the Pooling layer must stay on avepool_fwd) and HW = 65 (the
first shape on gap_fwd), a channel count that is no multiple of 8 (scalar lanes), a ragged channel
tile (40 channels = 5 lanes of a tile of 8), more than one channel-group block (520 channels = 65
lanes, a block holds 64), and shapes whose HW the plan splits into several slabs with a ragged
last one.  The plan of se.hip keeps >= 8 rows per row lane in a slab, and 16 channels leave 128
row lanes of bf16 (64 of fp32), so (3, 33, 17, 16) with its 561 rows is NOT split; the case that
stands in its place is the smallest HW that is, 1025 = 41 x 25 (bf16: slabs of 513 and 512 rows;
fp32: 342, 342, 341).  One case is added to the list: (2, 13, 5, 520), which splits its 65 rows
(33 + 32) at two channel-group blocks, the second of them ragged.

Inputs are seeded by the case: x, dy, r ~ N(0, 1) rounded to bf16; s = sigmoid(N(0, 1)) and
b ~ N(0, 1), rounded to bf16 for the two-bottom form (the coefficient arrives in a bf16 blob) and
plain fp32 for the learned form.

Error bounds (from the number formats and the summation shapes, never from a kernel output);
u32 = 2^-24 and u16 = 2^-8 are the unit roundoffs of fp32 and bf16, ``A`` and ``S`` the oracle on
absolute values, M = H W:

* forward, stored as bf16: ``u16 |ref| + 8 u32 A`` with ``A = |x| |s| + |b| + |r|`` — at most three
  fp32 operations, then one rounding to bf16; fp32 tensors: ``8 u32 A``.
* dx: ``u16 |ref| + 4 u32 |ref|`` — one fp32 product, one rounding (fp32 tensors: ``4 u32 |ref|``).
* ds, db as fp32: ``1.01 (M + 1) u32 S`` — a sum of M terms in any order; products of two bf16
  values are exact in fp32.  Accumulated onto a prefill of 7.0 (one more term):
  ``1.01 (M + 2) u32 (S + |prefill|)``.  Stored into a bf16 bottom[1]: ``u16 |ref|`` more.
* pool, bf16: ``u16 |ref| + 1.01 (M + 3) u32 mean|x|`` — the M-term sum, then the 1 / M scaling and
  its rounding.
"""
import functools
import zlib

import torch

CASES = (
    (1, 1, 1, 8),      # single pixel
    (2, 1, 1, 16),     # HW = 1, two images
    (3, 3, 3, 8),
    (2, 7, 7, 16),
    (5, 8, 8, 24),     # HW = 64: the Pooling route must stay on avepool_fwd
    (2, 65, 1, 8),     # HW = 65: first shape on gap_fwd
    (2, 5, 5, 12),     # C % 8 != 0: scalar path
    (2, 9, 8, 40),     # ragged channel tile
    (1, 4, 4, 520),    # more than one channel-group block
    (2, 13, 5, 520),   # added: two slabs (33 + 32 rows) at two channel-group blocks
    (3, 41, 25, 16),   # HW = 1025: several slabs with a ragged last one (561 rows are not split)
)
LARGEST = CASES[-1]
HW64, HW65 = CASES[4], CASES[5]
FP32_CASES = (CASES[3], CASES[6], CASES[-1])  # also run with fp32 tensors
IDS = ["x".join(map(str, c)) for c in CASES]

U32 = 2.0 ** -24
U16 = 2.0 ** -8
PREFILL = 7.0
F64 = torch.float64
BF16 = torch.bfloat16


@functools.lru_cache(maxsize=None)
def inputs(case, learned=False) -> dict:
    """x, dy, r [N,H,W,C] in bf16; s, b [N,C] in fp32 (bf16-representable unless ``learned``)."""
    N, H, W, C = case
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    rn = lambda *shape: torch.randn(*shape, generator=g)
    out = {k: rn(N, H, W, C).to(BF16) for k in ("x", "dy", "r")}
    s, b = torch.sigmoid(rn(N, C)), rn(N, C)
    if not learned:
        s, b = s.to(BF16).float(), b.to(BF16).float()
    out["s"], out["b"] = s, b
    return out


def _coef(v, shape, absolute, gate0):
    N, H, W, C = shape
    v = v.to(F64).reshape(N, 1, 1, C)
    if gate0:
        v = v[:1].expand(N, 1, 1, C)
    return v.abs() if absolute else v


def forward64(x, s=None, b=None, r=None, *, absolute=False, gate0=False, drop_r=False):
    """fp64 ``x s + b + r``, NHWC.  Mutants: the gate (and bias) of image 0 used for every image;
    r dropped."""
    y = x.to(F64)
    if absolute:
        y = y.abs()
    if s is not None:
        y = y * _coef(s, x.shape, absolute, gate0)
    if b is not None:
        y = y + _coef(b, x.shape, absolute, gate0)
    if r is not None and not drop_r:
        y = y + (r.to(F64).abs() if absolute else r.to(F64))
    return y


def backward64(dy, x, s, *, absolute=False, skip_last=False, gate0=False, no_x=False):
    """fp64 (dx [N,H,W,C], ds [N,C], db [N,C]).  Mutants: the last pixel left out of both
    reductions; the gate of image 0 used for every image; ds computed without x."""
    N, H, W, C = dy.shape
    g, xv = dy.to(F64), x.to(F64)
    if absolute:
        g, xv = g.abs(), xv.abs()
    dx = g * _coef(s, dy.shape, absolute, gate0)
    gr, xr = g.reshape(N, H * W, C), xv.reshape(N, H * W, C)
    if skip_last:
        gr, xr = gr[:, :-1], xr[:, :-1]
    ds = gr.sum(1) if no_x else (gr * xr).sum(1)
    return dx, ds, gr.sum(1)


def pool64(x, *, absolute=False, skip_last=False, div_plus_one=False):
    """fp64 mean over HW, [N,C].  Mutants: the last pixel left out; the sum divided by M + 1."""
    N, H, W, C = x.shape
    v = x.to(F64).reshape(N, H * W, C)
    if absolute:
        v = v.abs()
    M = H * W
    return (v[:, :-1] if skip_last else v).sum(1) / (M + 1 if div_plus_one else M)


# --- bounds ---------------------------------------------------------------------------------

def forward_bound(case, learned=False, use=("s", "b", "r"), fp32=False):
    """(ref, bound) of the forward with the operands named in ``use``."""
    i = inputs(case, learned)
    kw = {k: i[k] for k in use}
    ref = forward64(i["x"], **kw)
    A = forward64(i["x"], **kw, absolute=True)
    return ref, (0.0 if fp32 else U16) * ref.abs() + 8 * U32 * A


def backward_bound(case, learned=False, prefill=None, bf16_store=False, fp32=False):
    """((dx ref, bound), (ds ref, bound), (db ref, bound)); prefill: the value the gradient
    buffers held when the sums were accumulated onto them (None: stored); bf16_store: the sums
    are then rounded into a bf16 bottom[1]."""
    i = inputs(case, learned)
    M = case[1] * case[2]
    dx, ds, db = backward64(i["dy"], i["x"], i["s"])
    _, Ss, Sb = backward64(i["dy"], i["x"], i["s"], absolute=True)
    if prefill is not None:
        ds, db, Ss, Sb, M = ds + prefill, db + prefill, Ss + abs(prefill), Sb + abs(prefill), M + 1
    extra = U16 if bf16_store else 0.0
    return ((dx, ((0.0 if fp32 else U16) + 4 * U32) * dx.abs()),
            (ds, 1.01 * (M + 1) * U32 * Ss + extra * ds.abs()),
            (db, 1.01 * (M + 1) * U32 * Sb + extra * db.abs()))


def pool_bound(case):
    i = inputs(case)
    M = case[1] * case[2]
    ref = pool64(i["x"])
    return ref, U16 * ref.abs() + 1.01 * (M + 3) * U32 * pool64(i["x"], absolute=True)


def worst(got, ref, bound) -> float:
    """Largest |got - ref| / bound over the elements (0 where both vanish): <= 1 passes."""
    d = (got.detach().to(F64).cpu().reshape(ref.shape) - ref).abs()
    ratio = torch.where(d == 0, torch.zeros_like(d), d / bound)
    return float(ratio.max()) if ratio.numel() else 0.0
