"""Shared cases, inputs, fp64 oracles, mutants and error bounds of tests/test_pool_lrn_oracle.py
(CPU) and tests/test_pool_lrn_oracle_gpu.py (csrc/kernels/pool.hip, lrn.hip and pool_lrn.hip:
max / average pooling, cross-channel and within-channel LRN, and the three fused pool / LRN
kernels).

Nothing here calls the code under test.  The oracles are vectorised torch in float64 on float64
copies of the very bf16 values the code under test reads.  Pooling windows are ``unfold`` views
of an explicitly padded tensor; the cross-channel LRN window is a C x C membership matrix and the
within-channel one an ``unfold`` box, and the LRN backward is written out (not autograd), so
that every mutant below is one changed argument of the same computation.

Pooling cases ``(N, H, W, C, kh, kw, sh, sw, ph, pw)`` run for MAX and AVE; the comment on each
names the kernel or template instance of pool.hip it is there for.  x is ``relu(randn - 0.5)``
(many ties and all-zero windows; run gated and ungated) or plain ``randn``; dy ~ N(0, 1).
Geometry is Caffe's ceil mode (``PoolSpec.P`` / ``PoolSpec.Q``); no case has an empty window
(asserted below).  The argmax mask is the uint8 offset ``(h - hs) * kw + (w - ws)`` of the first
maximum in row-major order from the unclipped window origin, 255 where ``gate`` is set and the
window maximum is not > 0; an ungated all-zero window points at its first in-range element.

LRN cases ``(kind, N, H, W, C, size)`` with the hyperparameters of ``HYPER``: x ~ 2 N(0, 1),
dy ~ N(0, 1), alpha a power of two (exact in fp32, as the kernels receive it) such that
alpha/size * sum x^2 is of the order of k, so the normalisation is as large as the signal:
``k <= s <= 8 k`` on every case (asserted below).  The within-channel kernels have k = 1 built in.

Error bounds (from the number formats and the summation shapes, never from a kernel output).
U32 = 2^-24 and U16 = 2^-8 are the unit roundoffs of fp32 and bf16, and "A" is the abs-oracle: the
same computation with every term replaced by its absolute value.  Every result is rounded to
bf16 once (the ``U16 |ref|`` term); the second term covers the fp32 arithmetic before that, as
``c U32 A`` with c twice the number of fp32 roundings on the longest path (twice: each rounding
is relative to a computed, not the exact, value, and the final rounding sees the perturbed
number).

* MAX forward: equal as numbers to the oracle (the maximum of bf16 values is exact; ``==``, as
  the sign of a zero may differ): a bound of zero.  The mask: equal to the oracle.
* MAX backward: ``U16 |ref| + 2 T U32 A`` with ``T = ceil(kh/sh) ceil(kw/sw)`` the most windows
  that cover one pixel, summed in fp32, and A the same routing applied to |dy|.
* AVE forward: ``U16 |ref| + 2 (kh kw + 2) U32 A``: kh kw window terms added in fp32, the
  reciprocal of the divisor, the multiply by it.  A = sum |x| / divisor.  The divisor is
  ``(min(hs+kh, H+ph) - hs) (min(ws+kw, W+pw) - ws)``, forward and backward.
* AVE backward: ``U16 |ref| + 2 (T + 2) U32 A``: per term the reciprocal and the multiply (one
  path through them), then T adds.  A = sum |dy| / divisor over the covering windows.
* LRN: ``U16 |ref| + (c U32 + n EPOW) A``.  A = |ref| in the forward; in the backward
  ``|dy| s^-beta + ratio |x| sum_j |dy_j x_j| s_j^(-beta-1)`` over the same window.  n counts the
  ``s^-beta`` factors on a path: 1 forward, 2 backward (``s^(-beta-1)`` is ``s^-beta s^-1``).
  Roundings, cross-channel with window ``size``: forward alpha/size (1), the square sum (size; a
  product of two bf16 numbers is exact), the scale fma (1), the multiply (1): c = 2 (size + 3).
  Backward: a neighbour's scale (size + 2 roundings, amplified by beta + 1 <= 2 in the power),
  its product with the power (1), the window sum (size), the ratio 2 alpha beta / size (2), its
  product with x (1), the final fma (1): c = 2 (3 size + 9).  Within-channel, with ``size^2`` box
  terms in place of ``size`` and two more roundings for ``1 + a sum`` as a multiply and an add
  and for the unfused last line: forward c = 2 (size^2 + 4), backward c = 2 (3 size^2 + 13).
  EPOW = 2^-16 caps the relative error of ``sn_powneg``, ``exp2(-beta log2 s)`` on the hardware
  approximations, whose accuracy neither the project nor its guides state.  With 1-ulp
  instructions and s <= 16 (log2 s <= 4, exponent at most 1.75 x 4 = 7) the error is about
  ln 2 (7 x 2^-24 + 1.75 x 4 x 2^-23) + 2^-23, roughly 2^-20: a supposition.  EPOW is tied to the
  output format instead: 1/256 of the bf16 rounding that follows, so it cannot hide anything that
  is visible in bf16.

``worst(got, ref, bound)`` is the largest ``|got - ref| / bound`` (0 where they agree, inf where
they differ under a zero bound); <= 1 passes.

Largest worst / bound observed on an MI355X (tests/test_pool_lrn_oracle_gpu.py prints them):
pooling 0.996 (a max-pool dx), cross-channel LRN 0.991 (0.983 unfused; the larger is an LRN stage
of the fused chains), within-channel LRN 0.980.  Values this close to 1 are the final bf16
rounding alone (half an ulp of a number just above a power of two is 2^-8 of it); the U32 and EPOW
terms were not needed beyond it, and EPOW stays at 2^-16.
"""
import functools
import zlib
from typing import NamedTuple

import torch
import torch.nn.functional as F

from sparknet_amd.ops.spec import POOL_AVE, POOL_MAX, PoolSpec

U32 = 2.0 ** -24
U16 = 2.0 ** -8
EPOW = 2.0 ** -16
F64 = torch.float64
BF16 = torch.bfloat16

# --- pooling cases ----------------------------------------------------------------------------

POOL_CASES = (
    (1, 1, 1, 8, 3, 3, 2, 2, 1, 1),     # a single pixel; maxpool_fwd_k<3,3>, pool_bwd_k3s2, avepool_fwd<true>
    (2, 8, 9, 16, 3, 3, 2, 2, 0, 0),    # pool_bwd_k3s2<MAX / AVE>; the last window clipped by ceil mode
    (2, 9, 8, 8, 3, 3, 2, 2, 2, 1),     # pool_bwd_k3s2 with pads 2 and 1
    (2, 6, 7, 8, 2, 2, 2, 2, 0, 0),     # maxpool_fwd_k<2,2>, pool_bwd_k<1,1,*>; odd width
    (2, 7, 7, 8, 2, 2, 3, 3, 0, 0),     # stride above kernel: uncovered pixels get dx = 0 (pool_bwd_k<1,1,*>)
    (2, 9, 8, 8, 3, 2, 2, 1, 1, 0),     # everything non-square; maxpool_fwd<true>, pool_bwd_k<2,2,*>
    (2, 8, 8, 8, 5, 3, 2, 2, 2, 1),     # nh = 3, nw = 2: the generic pool_bwd<true,*>; maxpool_fwd<true>
    (2, 7, 7, 16, 7, 7, 1, 1, 0, 0),    # global pooling: the 49-term average, its tail batch of one; pool_bwd<true,*>
    (2, 6, 6, 8, 3, 3, 1, 1, 2, 2),     # output larger than input; pool_bwd_k<3,3,*>
    (3, 5, 6, 3, 2, 2, 2, 2, 0, 0),     # scalar: maxpool_fwd<false>, avepool_fwd<false>, pool_bwd<false,*>
    (2, 6, 5, 20, 3, 3, 2, 2, 1, 1),    # scalar paths, 3x3 / stride 2 with a pad
    (1, 5, 5, 520, 3, 3, 2, 2, 0, 0),   # 65 channel chunks
    (2, 30, 9, 64, 3, 3, 2, 2, 0, 0),   # several workgroups (4 max forward, 15 average forward, 5 backward): fewer
                                        # than the 16 at which xcd_block remaps, which the next two cases reach
    # 17 or more workgroups, the count not a multiple of 8: xcd_block's remap with a remainder
    # (tests/test_pool_lrn_oracle.py derives the counts from the launch formulas)
    (2, 33, 35, 64, 3, 3, 2, 2, 0, 0),  # maxpool_fwd_k<3,3> 17, avepool_fwd<true> 68, pool_bwd_k3s2 20 workgroups
    (2, 34, 33, 64, 2, 2, 2, 2, 0, 0),  # maxpool_fwd_k<2,2> 19, avepool_fwd<true> 73, pool_bwd_k<1,1,*> 71 workgroups
)
POOL_IDS = ["x".join(map(str, c)) for c in POOL_CASES]
NON_SQUARE = POOL_CASES[5]
STRIDE_ABOVE_KERNEL = POOL_CASES[4]
XCD_REMAP = POOL_CASES[13:15]
VARIANTS = ("relu", "randn")
METHODS = (POOL_MAX, POOL_AVE)


def pool_spec(case, method=POOL_MAX) -> PoolSpec:
    return PoolSpec(*case, method)


def _origins(s: PoolSpec):
    return torch.arange(s.P) * s.sh - s.ph, torch.arange(s.Q) * s.sw - s.pw


def _divisor(s: PoolSpec, in_image=False):
    """[P, Q] float64.  in_image (a mutant): only the elements inside the image are counted."""
    hs, ws = _origins(s)
    if in_image:
        dh = torch.clamp(hs + s.kh, max=s.H) - torch.clamp(hs, min=0)
        dw = torch.clamp(ws + s.kw, max=s.W) - torch.clamp(ws, min=0)
    else:
        dh = torch.clamp(hs + s.kh, max=s.H + s.ph) - hs
        dw = torch.clamp(ws + s.kw, max=s.W + s.pw) - ws
    return (dh[:, None] * dw[None, :]).to(F64)


def _covered(s: PoolSpec):
    """[H, W] bool: the pixel lies in at least one window."""
    hs, ws = _origins(s)
    h, w = torch.arange(s.H), torch.arange(s.W)
    ch = ((h[:, None] >= hs[None, :]) & (h[:, None] < hs[None, :] + s.kh)).any(1)
    cw = ((w[:, None] >= ws[None, :]) & (w[:, None] < ws[None, :] + s.kw)).any(1)
    return ch[:, None] & cw[None, :]


for _c in POOL_CASES:  # no empty window: every window holds at least one pixel of the image
    _s = pool_spec(_c)
    assert bool((_divisor(_s, in_image=True) > 0).all()), _c
    assert _s.kh * _s.kw <= 254, _c
assert not bool(_covered(pool_spec(STRIDE_ABOVE_KERNEL)).all())


@functools.lru_cache(maxsize=None)
def pool_inputs(case, variant) -> dict:
    """x [N,H,W,C] and dy [N,P,Q,C] in bf16."""
    s = pool_spec(case)
    g = torch.Generator().manual_seed(zlib.crc32(repr(("pool", case, variant)).encode()))
    x = torch.randn(s.N, s.H, s.W, s.C, generator=g)
    if variant == "relu":
        x = torch.relu(x - 0.5)
    return {"x": x.to(BF16), "dy": torch.randn(s.N, s.P, s.Q, s.C, generator=g).to(BF16)}


def _nchw(t):
    return t.to(F64).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _windows(xn, s: PoolSpec, fill):
    """[N, C, P, Q, kh*kw] windows of NCHW xn on the explicitly padded input."""
    Hp, Wp = (s.P - 1) * s.sh + s.kh, (s.Q - 1) * s.sw + s.kw
    xp = F.pad(xn, (s.pw, max(Wp - s.W - s.pw, 0), s.ph, max(Hp - s.H - s.ph, 0)), value=fill)[:, :, :Hp, :Wp]
    win = xp.unfold(2, s.kh, s.sh).unfold(3, s.kw, s.sw)
    assert win.shape[2:4] == (s.P, s.Q)
    return win.reshape(*win.shape[:4], s.kh * s.kw)


def max_forward64(x, s: PoolSpec, gate=False, *, last=False, offset_kw=None, ignore_gate=False,
                  skip_last_row=False):
    """fp64 (y, mask) in NHWC; the mask as int64.  The keyword mutants: the last maximum instead of
    the first; the offset's row pitch (kh in place of kw); the gate ignored; the last output row
    left at zero."""
    win = _windows(_nchw(x), s, float("-inf"))
    m = win.max(-1).values
    K = s.kh * s.kw
    idx = torch.arange(K).expand(win.shape)
    eq = win == m[..., None]
    j = torch.where(eq, idx, -1).max(-1).values if last else torch.where(eq, idx, K).min(-1).values
    off = (j // s.kw) * (s.kw if offset_kw is None else offset_kw) + j % s.kw
    if gate and not ignore_gate:
        off = torch.where(m > 0, off, torch.full_like(off, 255))
    if skip_last_row:
        m, off = m.clone(), off.clone()
        m[:, :, -1], off[:, :, -1] = 0.0, 0
    return _nhwc(m), _nhwc(off)


def fit(t, P, Q, fill=0):
    """NHWC t cropped or padded with `fill` to P x Q: the leading block of a gradient or mask as a
    backward with another geometry (a mutant) would index it."""
    t = t[:, :P, :Q]
    return F.pad(t, (0, 0, 0, Q - t.shape[2], 0, P - t.shape[1]), value=fill)


def max_backward64(dy, mask, s: PoolSpec, *, absolute=False, uncovered=0.0, strict=True):
    """fp64 dx, NHWC: dy routed by the mask.  uncovered (a mutant): the value left in pixels that
    no window covers.  strict off (mutants with another geometry): an offset that leaves the image
    routes nothing."""
    dyn = _nchw(dy)
    if absolute:
        dyn = dyn.abs()
    mk = mask.permute(0, 3, 1, 2).long()
    valid = mk != 255
    hs, ws = _origins(s)
    h = hs[None, None, :, None] + mk // s.kw
    w = ws[None, None, None, :] + mk % s.kw
    inside = (h >= 0) & (h < s.H) & (w >= 0) & (w < s.W)
    assert not strict or bool((~valid | inside).all())
    valid = valid & inside
    lin = torch.where(valid, h * s.W + w, torch.zeros_like(h))
    dx = torch.zeros(s.N, s.C, s.H * s.W, dtype=F64)
    dx.scatter_add_(2, lin.flatten(2), (dyn * valid).flatten(2))
    dx = dx.reshape(s.N, s.C, s.H, s.W)
    if uncovered:
        dx = torch.where(_covered(s), dx, torch.full_like(dx, uncovered))
    return _nhwc(dx)


def ave_forward64(x, s: PoolSpec, *, absolute=False, in_image_divisor=False, skip_last_row=False):
    xn = _nchw(x)
    y = _windows(xn.abs() if absolute else xn, s, 0.0).sum(-1) / _divisor(s, in_image_divisor)
    if skip_last_row:
        y[:, :, -1] = 0.0
    return _nhwc(y)


def ave_backward64(dy, s: PoolSpec, *, absolute=False, in_image_divisor=False, uncovered=0.0):
    dyn = _nchw(dy)
    g = (dyn.abs() if absolute else dyn) / _divisor(s, in_image_divisor)
    K = s.kh * s.kw
    Hp, Wp = (s.P - 1) * s.sh + s.kh, (s.Q - 1) * s.sw + s.kw
    cols = g[:, :, None].expand(s.N, s.C, K, s.P, s.Q).reshape(s.N, s.C * K, s.P * s.Q)
    dxp = F.fold(cols, (Hp, Wp), (s.kh, s.kw), stride=(s.sh, s.sw))
    dxp = F.pad(dxp, (0, max(s.pw + s.W - Wp, 0), 0, max(s.ph + s.H - Hp, 0)))
    dx = dxp[:, :, s.ph:s.ph + s.H, s.pw:s.pw + s.W]
    if uncovered:
        dx = torch.where(_covered(s), dx, torch.full_like(dx, uncovered))
    return _nhwc(dx)


def _terms(s: PoolSpec) -> int:
    return -(-s.kh // s.sh) * -(-s.kw // s.sw)


def pool_forward_bound_of(x, s: PoolSpec, gate=False):
    """(y ref, y bound, mask ref or None) for the input x."""
    if s.method == POOL_MAX:
        y, mask = max_forward64(x, s, gate)
        return y, torch.zeros_like(y), mask
    y, A = ave_forward64(x, s), ave_forward64(x, s, absolute=True)
    return y, U16 * y.abs() + 2 * (s.kh * s.kw + 2) * U32 * A, None


def pool_backward_bound_of(dy, x, s: PoolSpec, gate=False):
    """(dx ref, dx bound) for the inputs dy and x.  AVE with a gate: dx zeroed where x <= 0."""
    if s.method == POOL_MAX:
        mask = max_forward64(x, s, gate)[1]
        dx, A = max_backward64(dy, mask, s), max_backward64(dy, mask, s, absolute=True)
        return dx, U16 * dx.abs() + 2 * _terms(s) * U32 * A
    dx, A = ave_backward64(dy, s), ave_backward64(dy, s, absolute=True)
    if gate:
        keep = x.to(F64) > 0
        dx, A = dx * keep, A * keep
    return dx, U16 * dx.abs() + 2 * (_terms(s) + 2) * U32 * A


@functools.lru_cache(maxsize=None)
def pool_forward_bound(case, method, variant, gate=False):
    return pool_forward_bound_of(pool_inputs(case, variant)["x"], pool_spec(case, method), gate)


@functools.lru_cache(maxsize=None)
def pool_backward_bound(case, method, variant, gate=False):
    i = pool_inputs(case, variant)
    return pool_backward_bound_of(i["dy"], i["x"], pool_spec(case, method), gate)


def pool_runs():
    """(variant, gate) combinations every pooling case runs with."""
    return (("relu", False), ("relu", True), ("randn", False))


# --- LRN cases --------------------------------------------------------------------------------

class Hyper(NamedTuple):
    within: bool
    size: int
    alpha: float
    beta: float
    k: float


ACROSS, WITHIN = "across", "within"
LRN_CASES = (
    # cross-channel, the vector kernels lrn_across_fwd<SIZE> / lrn_across_bwd<SIZE>
    (ACROSS, 2, 3, 3, 8, 9),     # <9>: one chunk, every neighbour chunk outside [0, C)
    (ACROSS, 2, 3, 4, 16, 9),    # <9>: two chunks, each with one neighbour
    (ACROSS, 2, 3, 4, 24, 7),    # <7>: a middle chunk with neighbours on both sides
    (ACROSS, 2, 4, 3, 40, 3),    # <3>: the vectorised size-3 kernels
    (ACROSS, 1, 5, 5, 96, 5),    # <5>: more than one block (300 threads)
    # cross-channel, lrn_across_fwd_scalar / lrn_across_bwd_scalar
    (ACROSS, 2, 3, 3, 20, 3),    # C % 8 != 0
    (ACROSS, 2, 3, 3, 12, 5),    # C % 8 != 0
    (ACROSS, 2, 3, 3, 16, 11),   # a size without a template instance
    # within-channel: lrn_within_fwd, lrn_within_bwd_u, lrn_within_bwd_dx
    (WITHIN, 2, 5, 5, 16, 9),    # window wider than the image
    (WITHIN, 2, 6, 7, 8, 3),
    (WITHIN, 2, 9, 8, 20, 5),    # more than one block
    (WITHIN, 1, 1, 1, 8, 5),     # a single pixel
)
LRN_IDS = ["x".join(map(str, c)) for c in LRN_CASES]
#            alpha, beta, k
_HYPER = {
    LRN_CASES[0]: (0.125, 0.75, 1.0),
    LRN_CASES[1]: (0.25, 0.75, 2.0),
    LRN_CASES[2]: (0.125, 0.5, 1.0),
    LRN_CASES[3]: (0.125, 0.75, 1.0),
    LRN_CASES[4]: (0.25, 0.75, 2.0),
    LRN_CASES[5]: (0.25, 0.75, 2.0),
    LRN_CASES[6]: (0.125, 0.75, 1.0),
    LRN_CASES[7]: (0.125, 0.75, 1.0),
    LRN_CASES[8]: (0.5, 0.75, 1.0),
    LRN_CASES[9]: (0.125, 0.75, 1.0),
    LRN_CASES[10]: (0.125, 0.5, 1.0),
    LRN_CASES[11]: (4.0, 0.75, 1.0),
}


def hyper(case) -> Hyper:
    return Hyper(case[0] == WITHIN, case[5], *_HYPER[case])


@functools.lru_cache(maxsize=None)
def lrn_inputs(case) -> dict:
    """x ~ 2 N(0, 1) and dy ~ N(0, 1), [N,H,W,C] in bf16."""
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    shape = case[1:5]
    return {"x": (2.0 * torch.randn(*shape, generator=g)).to(BF16), "dy": torch.randn(*shape, generator=g).to(BF16)}


class Window(NamedTuple):
    """The geometry of an LRN window; the defaults are the kernels', every other value a mutant."""
    shift: int = 0            # cross-channel: the window shifted by this many channels
    drop_far: bool = False    # cross-channel: the farthest neighbour c + post dropped
    chunk_zero: bool = False  # cross-channel: neighbours in another 8-channel chunk read as zero
    clip_short: bool = False  # within-channel: the image's last row and column are never read


def window_matrix(C, size, win=Window()):
    """[C, C] float64, M[c, c'] = 1 where c' lies in the window of c: c - pre <= c' <= c + post."""
    pre = (size - 1) // 2
    post = size - pre - 1
    c = torch.arange(C)
    d = c[None, :] - c[:, None]
    M = (d >= -pre + win.shift) & (d <= post + win.shift)
    if win.drop_far:
        M &= d != post
    if win.chunk_zero:
        M &= (c[None, :] // 8) == (c[:, None] // 8)
    return M.to(F64)


def _box(t, size, win=Window()):
    """size x size box sums (zero outside the image) of NHWC t."""
    pre = (size - 1) // 2
    tn = t.permute(0, 3, 1, 2)
    if win.clip_short:
        tn = tn.clone()
        tn[:, :, -1, :] = 0.0
        tn[:, :, :, -1] = 0.0
    tp = F.pad(tn, (pre, size - 1 - pre, pre, size - 1 - pre))
    return _nhwc(tp.unfold(2, size, 1).unfold(3, size, 1).sum((-1, -2)))


def _gather(t, h: Hyper, win: Window, transposed=False):
    """Window sums of t: within-channel a box; cross-channel over the window of each channel, or
    (transposed) over the channels whose window holds it."""
    if h.within:
        return _box(t, h.size, win)
    M = window_matrix(t.shape[-1], h.size, win)
    return t @ (M if transposed else M.T)


def lrn_scale64(x, h: Hyper, win=Window(), *, alpha_undivided=False, divisor_size=False):
    """(s, a): s = k + a sum x^2 over the window, a = alpha / size (size^2 within a channel).  The
    mutants: alpha in place of alpha / size; within a channel, size in place of size^2."""
    xd = x.to(F64)
    a = h.alpha / (h.size * h.size if h.within and not divisor_size else h.size)
    if alpha_undivided:
        a = h.alpha
    return h.k + a * _gather(xd * xd, h, win), a


def lrn_forward64(x, h: Hyper, win=Window(), *, identity=False, **scale):
    """y = x s^-beta.  identity (a mutant): y = x."""
    xd = x.to(F64)
    if identity:
        return xd
    s, _ = lrn_scale64(x, h, win, **scale)
    return xd * s.pow(-h.beta)


def lrn_backward64(dy, x, h: Hyper, gate=False, win=Window(), *, absolute=False, passthrough=False,
                   no_neighbours=False, ignore_gate=False, **scale):
    """dx = dy s^-beta - 2 a beta x sum_j dy_j x_j s_j^(-beta-1), the sum over the j whose window
    holds the element; zeroed where x <= 0 under a gate.  The mutants: dy passed through; the
    neighbour term dropped; the gate ignored; and those of Window and lrn_scale64."""
    xd, dyd = x.to(F64), dy.to(F64)
    if passthrough:
        return dyd
    s, a = lrn_scale64(x, h, win, **scale)
    ratio = 0.0 if no_neighbours else 2.0 * a * h.beta
    r = dyd * xd * s.pow(-h.beta - 1.0)
    if absolute:
        dx = dyd.abs() * s.pow(-h.beta) + ratio * xd.abs() * _gather(r.abs(), h, win, transposed=True)
    else:
        dx = dyd * s.pow(-h.beta) - ratio * xd * _gather(r, h, win, transposed=True)
    if gate and not ignore_gate:
        dx = dx * (xd > 0)
    return dx


def _roundings(h: Hyper, backward: bool) -> int:
    if h.within:
        return 2 * (3 * h.size ** 2 + 13) if backward else 2 * (h.size ** 2 + 4)
    return 2 * (3 * h.size + 9) if backward else 2 * (h.size + 3)


def lrn_forward_bound_of(x, h: Hyper):
    ref = lrn_forward64(x, h)
    return ref, U16 * ref.abs() + (_roundings(h, False) * U32 + EPOW) * ref.abs()


def lrn_backward_bound_of(dy, x, h: Hyper, gate=False):
    ref = lrn_backward64(dy, x, h, gate)
    A = lrn_backward64(dy, x, h, gate, absolute=True)
    return ref, U16 * ref.abs() + (_roundings(h, True) * U32 + 2 * EPOW) * A


@functools.lru_cache(maxsize=None)
def lrn_forward_bound(case):
    return lrn_forward_bound_of(lrn_inputs(case)["x"], hyper(case))


@functools.lru_cache(maxsize=None)
def lrn_backward_bound(case, gate=False):
    i = lrn_inputs(case)
    return lrn_backward_bound_of(i["dy"], i["x"], hyper(case), gate)


def scale_range(x, h: Hyper):
    s, _ = lrn_scale64(x, h)
    return float(s.min()), float(s.max())


for _c in LRN_CASES:  # the normalisation is visible and the power's argument stays in [k, 8k]
    _h = hyper(_c)
    assert _h.alpha == float(torch.tensor(_h.alpha, dtype=torch.float32)) and not (_h.within and _h.k != 1.0), _c
    _lo, _hi = scale_range(lrn_inputs(_c)["x"], _h)
    assert _h.k <= _lo and 1.5 * _h.k <= _hi <= 8 * _h.k, (_c, _lo, _hi)
assert {hyper(c).beta for c in LRN_CASES} == {0.5, 0.75} and {hyper(c).k for c in LRN_CASES} == {1.0, 2.0}

# --- the fused pool / LRN kernels: 3x3 / stride-2 max pooling and a cross-channel LRN ----------

FUSED_CASES = (  # N, H, W, C, pad, LRN size (the pooling input's shape)
    (2, 30, 9, 64, 0, 5),    # lrn_pool_bwd tile: cg = 4 of 8 chunks (two channel groups), three row blocks
    (2, 8, 10, 96, 1, 5),    # three channel groups: the middle one has neighbours on both sides; a pad
    (1, 13, 13, 8, 0, 9),    # one chunk: every neighbour chunk outside [0, C)
    (2, 9, 12, 24, 2, 7),    # size 7, pad 2
    (3, 14, 15, 40, 1, 3),   # size 3, odd sizes
)
FUSED_IDS = ["x".join(map(str, c)) for c in FUSED_CASES]
FUSED_HYPER = (0.125, 0.75, 1.0)  # alpha, beta, k


def fused_spec(case) -> PoolSpec:
    N, H, W, C, pad, _ = case
    return PoolSpec(N, H, W, C, 3, 3, 2, 2, pad, pad, POOL_MAX)


def fused_hyper(case) -> Hyper:
    return Hyper(False, case[5], *FUSED_HYPER)


@functools.lru_cache(maxsize=None)
def fused_inputs(case) -> dict:
    """x [N,H,W,C] ~ 2 N(0, 1) and dy [N,P,Q,C] ~ N(0, 1) in bf16."""
    s = fused_spec(case)
    g = torch.Generator().manual_seed(zlib.crc32(repr(("fused", case)).encode()))
    return {"x": (2.0 * torch.randn(s.N, s.H, s.W, s.C, generator=g)).to(BF16),
            "dy": torch.randn(s.N, s.P, s.Q, s.C, generator=g).to(BF16)}


def fused_x(case, gate):
    """The pooling / LRN input: under a gate, the in-place ReLU output the gate stands for."""
    x = fused_inputs(case)["x"]
    return x.clamp_min(0) if gate else x


for _c in FUSED_CASES:  # the LRN's input is the pooled tensor (pool -> LRN) or x itself (LRN -> pool)
    _h = fused_hyper(_c)
    for _gate in (False, True):
        _pooled = max_forward64(fused_x(_c, _gate), fused_spec(_c), _gate)[0]
        for _t in (_pooled, fused_x(_c, _gate)):
            _lo, _hi = scale_range(_t, _h)
            assert _h.k <= _lo and 1.5 * _h.k <= _hi <= 8 * _h.k, (_c, _gate, _lo, _hi)


# --- image chunking: N = 5 as 2 + 2 + 1 images ------------------------------------------------

CHUNK_CASES = (
    (5, 6, 7, 8, 2, 2, 2, 2, 0, 0),     # fp8 side output forward (maxpool_fwd_k<2,2>) and backward (pool_bwd_k<1,1>)
    (5, 8, 9, 16, 3, 3, 2, 2, 0, 0),    # fp8 side output forward (maxpool_fwd_k<3,3>); pool_bwd_k3s2 has none
    (5, 9, 8, 8, 3, 2, 2, 1, 1, 0),     # generic forward: no side output
)
CHUNK_IDS = ["x".join(map(str, c)) for c in CHUNK_CASES]


def chunk_limit(case) -> int:
    """The element limit at which the case's 5 images run as 2 + 2 + 1."""
    s = pool_spec(case)
    return 2 * s.H * s.W * s.C + 1


def worst(got, ref, bound) -> float:
    """Largest |got - ref| / bound over the elements (0 where they agree, inf where they differ
    under a zero bound): <= 1 passes."""
    d = (got.detach().to(F64).cpu().reshape(ref.shape) - ref).abs()
    ratio = torch.where(d == 0, torch.zeros_like(d), d / bound)
    return float(ratio.max()) if ratio.numel() else 0.0


def exact(got, ref) -> float:
    """worst() under a zero bound: 0 where equal as numbers, inf otherwise."""
    ref = ref.to(F64)
    return worst(got, ref, torch.zeros_like(ref))
