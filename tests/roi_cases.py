"""Shared cases, inputs, oracle and error bounds of tests/test_roi.py and tests/test_roi_gpu.py (csrc/kernels/roi.hip:
ROIPooling, ROIAlign).  Nothing here calls the code under test.

The oracle is plain loops: bin edges and sample positions in float32 in the kernels' order of operations (they
define the result: fp32 3 * (7 / 3) is 7 + 2^-21, whose ceil is 8), values and sums in float64 on the very bf16
values the kernels read.  Box coordinates are multiples of 1/8, so that sample positions are exact or far from
the -1 / H cut-offs (tests/test_roi.py asserts the distance).

ROIPooling's forward is a selection: output and argmax must match exactly.  The other bounds come from the
number formats (u32 = 2^-24, u16 = 2^-8; A: the same sum over absolute values): ``u16 |ref| + 2 D u32 A``, one
rounding to bf16 plus an fp32 sum of depth D, doubled for the higher-order terms.  D is the number of terms plus
one for the ROIPooling backward; for ROIAlign the number of (sample, corner) terms plus ``2 G + 8`` with G the
largest sampling grid: the weights are differences, products and sums of up to G fp32 values per axis, divided
by the count.
"""
import functools
import math
import typing
import zlib

import numpy as np
import torch

from conv_dw_cases import BF16, F64, U16, U32, worst  # noqa: F401

F32 = np.float32
CHUNK = 256  # ROIs per staged table chunk of the backward kernels (hip.ROI_CHUNK)


class Case(typing.NamedTuple):
    name: str
    N: int
    H: int
    W: int
    C: int
    PH: int
    PW: int
    scale: float
    rois: tuple       # (image, x1, y1, x2, y2) rows, or an int: that many seeded ROIs
    plateau: bool = False


CASES = (
    Case("one_vector", 1, 6, 6, 8, 2, 2, 1.0, ((0, 0, 0, 5, 5),)),
    Case("ragged", 2, 5, 7, 21, 3, 2, 0.5, (
        (1, 0, 0, 8, 6), (1, 2, 2, 10, 8),    # overlapping: the backward sums across ROIs
        (0, 4, 4, 4, 4),                      # one pixel: every bin picks it; narrower than a pixel for ROIAlign
        (0, 8, 6, 20, 16),                    # hangs off the bottom right: clipped windows, empty bins
        (1, 20, 20, 30, 30),                  # wholly outside
        (0, 0, -6, 6, 6),                     # rows -3 .. 3, height 7 over 3 bins: ceil(3 * bin) is 8, so row 4 counts
        (2, 0, 0, 4, 4))),                    # batch index N: ignored
    Case("tiles", 1, 14, 14, 40, 7, 7, 1.0, ((0, 0, 0, 13, 13), (0, 2, 3, 9, 12), (0, 5.5, 1.25, 12.5, 8.75))),
    Case("chunks", 2, 4, 4, 8, 2, 2, 1.0, CHUNK + 3),
    Case("plateau", 1, 6, 6, 8, 2, 2, 1.0, ((0, 0, 0, 5, 5), (0, 1, 2, 4, 3)), True),
)
IDS = [c.name for c in CASES]


@functools.lru_cache(maxsize=None)
def inputs(case) -> dict:
    """x [N,H,W,C] and dy [R,PH,PW,C] in bf16, rois [R,5] in fp32."""
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    rois = case.rois
    if isinstance(rois, int):  # corners on the 1/8 grid in [0, 3], x1 <= x2, y1 <= y2, a third of the batch indices N
        p = torch.randint(0, 25, (rois, 2, 2), generator=g).sort(dim=1).values / 8.0
        n = torch.randint(0, case.N + 1, (rois, 1), generator=g).float()
        rois = torch.cat([n, p[:, 0], p[:, 1]], 1).tolist()
    x = torch.randn(case.N, case.H, case.W, case.C, generator=g)
    if case.plateau:
        x = x[:, :1, :1].expand(-1, case.H, case.W, -1).contiguous()
    return {"x": x.to(BF16), "rois": torch.tensor(rois, dtype=torch.float32),
            "dy": torch.randn(len(rois), case.PH, case.PW, case.C, generator=g).to(BF16)}


def _scaled(case, roi):
    """(image, x1, y1, x2, y2) scaled in float32, or None for an ignored ROI."""
    return (int(roi[0]), *(F32(v) * F32(case.scale) for v in roi[1:])) if 0 <= roi[0] < case.N else None


def _f64(case):
    i = inputs(case)
    return i["x"].to(F64).numpy(), i["dy"].to(F64).numpy(), i["rois"].numpy()


@functools.lru_cache(maxsize=None)
def pool_oracle(case):
    """y, argmax, and for the backward (dx, A, terms per element)."""
    x, dy, rois = _f64(case)
    rnd = lambda v: int(math.copysign(math.floor(abs(float(v)) + 0.5), float(v)))
    y, am = np.zeros(dy.shape), np.full(dy.shape, -1, dtype=np.int64)
    dx, A, D = (np.zeros((case.N, case.H * case.W, case.C)) for _ in range(3))
    chan = np.arange(case.C)
    for r, roi in enumerate(rois):
        box = _scaled(case, roi)
        if box is None:
            continue
        n, ws, hs, we, he = box[0], *(rnd(v) for v in box[1:])
        bh, bw = F32(max(he - hs + 1, 1)) / F32(case.PH), F32(max(we - ws + 1, 1)) / F32(case.PW)
        edge = lambda p, b, s, L: (min(max(math.floor(F32(p) * b) + s, 0), L), min(max(math.ceil(F32(p + 1) * b) + s, 0), L))
        for ph in range(case.PH):
            h0, h1 = edge(ph, bh, hs, case.H)
            for pw in range(case.PW):
                w0, w1 = edge(pw, bw, ws, case.W)
                if h1 <= h0 or w1 <= w0:
                    continue
                m, a = np.full(case.C, -np.inf), np.full(case.C, -1, dtype=np.int64)
                for h in range(h0, h1):
                    for w in range(w0, w1):
                        gt = x[n, h, w] > m  # strict: the first maximum in scan order wins
                        m[gt], a[gt] = x[n, h, w][gt], h * case.W + w
                y[r, ph, pw], am[r, ph, pw] = m, a
                for acc, v in ((dx, dy[r, ph, pw]), (A, np.abs(dy[r, ph, pw])), (D, 1.0)):
                    np.add.at(acc[n], (a, chan), v)
    shape = (case.N, case.H, case.W, case.C)
    D += 1
    return y, am, tuple(torch.from_numpy(t.reshape(shape)) for t in (dx, A, D))


def _axis(start, size, P, grid, L):
    """Per sample of an axis: (bin, float32 coordinate, ((index, weight), ...)), no corners for a zero sample."""
    out = []
    for p in range(P):
        for i in range(grid):
            v = start + F32(p) * size + (F32(i) + F32(0.5)) * size / F32(grid)
            if v < -1 or v > L:
                out.append((p, v, ()))
                continue
            c = max(v, F32(0))
            lo = int(c)
            wh = float(c) - lo
            out.append((p, v, ((L - 1, 1.0),) if lo >= L - 1 else ((lo, 1.0 - wh), (lo + 1, wh))))
    return out


def align_axes(case, sampling):
    """Per served ROI: (r, image, row samples, column samples, samples per bin, largest grid)."""
    for r, roi in enumerate(inputs(case)["rois"].numpy()):
        box = _scaled(case, roi)
        if box is not None:
            n, x1, y1, x2, y2 = box
            rw, rh = max(x2 - x1, F32(1)), max(y2 - y1, F32(1))
            gh = sampling or math.ceil(rh / F32(case.PH))
            gw = sampling or math.ceil(rw / F32(case.PW))
            yield (r, n, _axis(y1, rh / F32(case.PH), case.PH, gh, case.H),
                   _axis(x1, rw / F32(case.PW), case.PW, gw, case.W), gh * gw, max(gh, gw))


@functools.lru_cache(maxsize=None)
def align_oracle(case, sampling):
    """((y, A, D), (dx, A, D)) in float64."""
    x, dy, _ = _f64(case)
    fwd, bwd = [np.zeros(dy.shape) for _ in range(3)], [np.zeros(x.shape) for _ in range(3)]
    G = 1
    for r, n, ys, xs, count, g in align_axes(case, sampling):
        G = max(G, g)
        for p, _, yc in ys:
            for q, _, xc in xs:
                for h, wy in yc:
                    for w, wx in xc:
                        k = wy * wx / count
                        for acc, v in zip(fwd, (k * x[n, h, w], k * np.abs(x[n, h, w]), 1.0)):
                            acc[r, p, q] += v
                        for acc, v in zip(bwd, (k * dy[r, p, q], k * np.abs(dy[r, p, q]), 1.0)):
                            acc[n, h, w] += v
    for t in (fwd, bwd):
        t[2] += 2 * G + 8
    return tuple(torch.from_numpy(t) for t in fwd), tuple(torch.from_numpy(t) for t in bwd)


def bound(ref, A, D):
    return ref, U16 * ref.abs() + 2 * D * U32 * A


L1_CASES = [(sigma, nb) for sigma in (1.0, 3.0) for nb in (2, 3, 4)]  # (sigma, bottoms)


@functools.lru_cache(maxsize=None)
def smooth_l1(sigma, nb, lw=0.75):
    """SmoothL1Loss on [6, 12]: the operands (pred bf16; target, inside, outside weights fp32, None when absent;
    with three bottoms the third is both weights) and in float64 the loss with its bound — an fp32 sum of 72
    terms of a few operations each — and the gradient to pred for loss weight ``lw`` (elementwise: one bf16
    rounding and 8 fp32 ones).  |d| falls on both sides of 1 / sigma^2."""
    g = torch.Generator().manual_seed(int(10 * sigma) + nb)
    pred, target = (2 * torch.randn(6, 12, generator=g)).to(BF16), torch.randn(6, 12, generator=g)
    in_w = (torch.rand(6, 12, generator=g) > 0.3).float() * 1.5 if nb > 2 else None
    out_w = torch.rand(6, 12, generator=g) if nb > 3 else in_w
    one = torch.ones(6, 12, dtype=F64)
    iw, ow = (one if t is None else t.to(F64) for t in (in_w, out_w))
    d, s2 = iw * (pred.to(F64) - target.to(F64)), sigma * sigma
    assert (d.abs() < 1 / s2).any() and (d.abs() > 1 / s2).any()
    f = torch.where(d.abs() < 1 / s2, 0.5 * s2 * d * d, d.abs() - 0.5 / s2)
    loss, A = (ow * f).sum() / 6, (ow * (f.abs() + 0.5 / s2)).sum() / 6
    grad = lw / 6 * iw * ow * torch.where(d.abs() < 1 / s2, s2 * d, torch.sign(d))
    return (pred, target, in_w, out_w), (loss, 2 * (72 + 8) * U32 * A), (grad, (U16 + 8 * U32) * grad.abs())
