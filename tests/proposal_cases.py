"""Shared cases, inputs, oracle and bounds of tests/test_proposal.py and tests/test_proposal_gpu.py (the Proposal
layer: csrc/kernels/proposal.hip, ops.ref.proposal).  Nothing here calls the code under test.

The oracle works in float64 on the bf16-rounded scores and deltas: decode, clip, filter, a stable rank by score,
greedy NMS in a loop, padding.  It also returns its two decision margins: the smallest |extent - min_size scale|
over the boxes and the smallest |IoU - nms_thresh| over the pairs (kept box, any lower-ranked box).  The tests
assert them to be at least 1e-3 pixel and 1e-4: conditions on the inputs, so that an fp32 rounding cannot flip a
decision and membership, order and count must match exactly.  With nms_thresh = 1 nothing can be suppressed in
either arithmetic (fp32 inter / (a + b - inter) never exceeds 1: a + b >= 2 inter survives each rounding), so
that margin is infinite.

Coordinates.  With zero deltas every quantity of the decode is a small integer or half-integer and exp(0) = 1:
exact.  Otherwise, per axis with u = 2^-24, e and c = lo + 0.5 e are exact (integers / halves), pc = d e + c
takes two roundings, u (|d e| + |pc|), pe = exp(dl) e one ulp = 2 u of the device exp (the documented bound of
the OCML expf) and one rounding, 3 u pe, and pc -+ 0.5 pe one more, u (|pc| + 0.5 pe): in all at most
u (|d e| + 2 |pc| + 2 pe) <= 3 u (|c| + |d e| + pe).  Clipping does not expand it.  BOUND takes 4 u for the
higher-order terms.
"""
import functools
import typing
import zlib

import numpy as np
import torch

from conv_dw_cases import BF16, F64, U32, worst  # noqa: F401

M_EXTENT, M_IOU = 1e-3, 1e-4


class Case(typing.NamedTuple):
    name: str
    N: int
    H: int
    W: int
    ratios: tuple
    scales: tuple
    min_size: float
    pre: int
    post: int
    thresh: float
    im_info: tuple
    deltas: float      # standard deviation of the deltas; 0: none
    scores: str        # "random", "eight" distinct values, "narrow" (a few neighbouring bf16 values), "descending"
    exact: bool = False
    seed: int = 0      # chosen on the CPU so that the margins hold


R3, S3 = (0.5, 1, 2), (8, 16, 32)
CASES = (
    Case("decode", 2, 5, 7, R3, S3, 16, 315, 315, 1.0, ((80, 112, 1), (64, 100, 1.5)), 0.5, "random"),
    Case("select_ties", 2, 5, 7, R3, S3, 15.5, 100, 100, 1.0, ((80, 112, 1), (90, 100, 1)), 0, "eight", True),
    Case("select_passes", 1, 24, 32, R3, S3, 16, 3000, 50, 0.8, ((384, 512, 1),), 0.3, "narrow", seed=1),
    Case("nms_chain", 1, 3, 70, (1,), (4,), 15.5, 200, 200, 0.5, ((120, 1200, 1),), 0, "descending", True),
    Case("few", 1, 5, 7, R3, S3, 44, 200, 60, 0.5, ((80, 112, 1),), 0.5, "random", seed=3),
    # 16641 boxes, 16384 of them sorted: the select's and the scan's LDS both pass 64 KB
    Case("lds_limit", 1, 43, 43, R3, S3, 15.5, 16384, 12, 0.69, ((688, 688, 1),), 0, "random", True),
    Case("empty", 3, 5, 7, R3, S3, 16, 100, 20, 0.7, ((80, 112, 100), (float("nan"), 112, 1), (80, 112, 1)), 0.5, "random"),
)
IDS = [c.name for c in CASES]


def anchors(ratios, scales):
    """The public generate_anchors for base_size 16 (centre 7.5), written out independently of ops.ref: ratios
    outermost, numpy's roundings."""
    out = []
    for r in ratios:
        w = np.round(np.sqrt(256 / r))
        h = np.round(w * r)
        for s in scales:
            out.append([7.5 - 0.5 * (w * s - 1), 7.5 - 0.5 * (h * s - 1), 7.5 + 0.5 * (w * s - 1), 7.5 + 0.5 * (h * s - 1)])
    return np.array(out, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def inputs(case) -> dict:
    """scores [N, H, W, 2A] and deltas [N, H, W, 4A] in bf16, im_info [N, 3] and the base anchors [A, 4] in fp32."""
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()) + case.seed)
    A = len(case.ratios) * len(case.scales)
    shape = (case.N, case.H, case.W, A)
    if case.scores == "random":
        fg = torch.rand(shape, generator=g)
    elif case.scores == "eight":
        fg = torch.randint(1, 9, shape, generator=g) / 8.0
    elif case.scores == "narrow":  # 0.5 + k / 256, k < 6: bf16 neighbours, their keys share the 13 leading bits
        fg = 0.5 + torch.randint(0, 6, shape, generator=g) / 256.0
    else:  # distinct bf16 values, descending in box order: 1 - 2^-8, the next one down, ...
        bits = 0x3F7F - torch.arange(case.N * case.H * case.W * A, dtype=torch.int32)
        fg = bits.to(torch.int16).view(BF16).float().reshape(shape)
    scores = torch.cat([1 - fg, fg], 3).to(BF16)
    deltas = (case.deltas * torch.randn(case.N, case.H, case.W, 4 * A, generator=g)).to(BF16)
    return {"scores": scores, "deltas": deltas, "im_info": torch.tensor(case.im_info, dtype=torch.float32),
            "anchors": torch.from_numpy(anchors(case.ratios, case.scales))}


class Expected(typing.NamedTuple):
    rois: torch.Tensor    # [N post, 5] float64
    scores: torch.Tensor  # [N post, 1]
    count: torch.Tensor   # [N]
    bound: torch.Tensor   # [N post, 5]: 0 for the image column and the padding rows
    m_extent: float
    m_iou: float


def oracle(scores, deltas, im_info, base, stride, min_size, pre, post, thresh) -> Expected:
    N, H, W, A = *scores.shape[:3], scores.shape[3] // 2
    sc = scores[..., A:].to(F64).reshape(N, -1).numpy()
    d = deltas.to(F64).reshape(N, -1, 4).numpy()
    info, base = im_info.to(F64).numpy(), base.to(F64).numpy()
    shift = np.array([[w, h, w, h] for h in range(H) for w in range(W)], dtype=np.float64) * stride
    anc = (shift[:, None, :] + base[None]).reshape(-1, 4)
    rois, out_sc, bound = np.zeros((N, post, 5)), np.zeros((N, post, 1)), np.zeros((N, post, 5))
    rois[..., 0], count, m_extent, m_iou = -1, np.zeros(N, dtype=np.int64), np.inf, np.inf
    for n in range(N):
        if not (np.isfinite(info[n]).all() and (info[n] > 0).all()):
            continue
        box, err = np.zeros((len(anc), 4)), np.zeros((len(anc), 4))
        with np.errstate(over="ignore", invalid="ignore"):
            for k in (0, 1):  # x, then y
                e = anc[:, k + 2] - anc[:, k] + 1
                c = anc[:, k] + 0.5 * e
                pc, pe = d[n, :, k] * e + c, np.exp(d[n, :, k + 2]) * e
                box[:, k], box[:, k + 2] = pc - 0.5 * pe, pc + 0.5 * pe
                err[:, k] = err[:, k + 2] = 4 * U32 * (np.abs(c) + np.abs(d[n, :, k] * e) + pe)
        finite = np.isfinite(box).all(1)
        box = np.clip(box, 0, [info[n, 1] - 1, info[n, 0] - 1] * 2)
        extent = np.stack([box[:, 2] - box[:, 0] + 1, box[:, 3] - box[:, 1] + 1], 1)
        lim = float(np.float32(min_size) * np.float32(info[n, 2]))
        m_extent = min(m_extent, np.abs(extent[finite] - lim).min())
        keep = np.nonzero(finite & (extent >= lim).all(1) & ~np.isnan(sc[n]))[0]
        order = keep[np.argsort(-sc[n, keep], kind="stable")][:pre if pre else None]
        b = box[order]
        area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
        gone, kept = np.zeros(len(b), dtype=bool), []
        for i in range(len(b)):
            if gone[i]:
                continue
            kept.append(i)
            if len(kept) == post:
                break
            for j in range(i + 1, len(b)):
                iw = max(0.0, min(b[i, 2], b[j, 2]) - max(b[i, 0], b[j, 0]) + 1)
                ih = max(0.0, min(b[i, 3], b[j, 3]) - max(b[i, 1], b[j, 1]) + 1)
                iou = iw * ih / (area[i] + area[j] - iw * ih)
                if thresh < 1:
                    m_iou = min(m_iou, abs(iou - thresh))
                gone[j] |= iou > thresh
        k = count[n] = len(kept)
        rois[n, :k, 0], rois[n, :k, 1:], bound[n, :k, 1:] = n, b[kept], err[order[kept]]
        out_sc[n, :k, 0] = sc[n, order[kept]]
    t = torch.from_numpy
    return Expected(t(rois).reshape(-1, 5), t(out_sc).reshape(-1, 1), t(count), t(bound).reshape(-1, 5),
                    float(m_extent), float(m_iou))


@functools.lru_cache(maxsize=None)
def expected(case) -> Expected:
    i = inputs(case)
    return oracle(i["scores"], i["deltas"], i["im_info"], i["anchors"], 16, case.min_size, case.pre, case.post,
                  case.thresh)


def check(got, want: Expected, exact=False):
    """Membership, order, batch indices, padding rows, scores and count exactly; coordinates exactly
    (``exact``) or within the bound.  ``got``: (rois, scores, count).  Returns worst error / bound."""
    rois, scores, count = (t.detach().cpu() for t in got)
    assert want.m_extent >= M_EXTENT and want.m_iou >= M_IOU, (want.m_extent, want.m_iou)
    assert rois.dtype == scores.dtype == torch.float32 and count.dtype == torch.int32
    assert torch.equal(count.long(), want.count), (count, want.count)
    assert torch.equal(rois[:, 0].double(), want.rois[:, 0]) and torch.equal(scores.double(), want.scores)
    live = want.rois[:, 0] >= 0
    assert torch.equal(rois[~live].double(), want.rois[~live])
    if exact:
        assert torch.equal(rois.double(), want.rois)
        return 0.0
    # a clipped coordinate (0 or the image edge) is exact in both: the bound covers the rest
    return worst(rois[live], want.rois[live], want.bound[live].clamp(min=1e-300))
