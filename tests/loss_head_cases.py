"""Shared inputs, oracles and error bounds of tests/test_loss_head.py (CPU) and
tests/test_loss_head_gpu.py (HIP kernels of csrc/kernels/softmax.hip).

Nothing here calls the code under test.  The top-k oracle sorts (score, class index) pairs
the way the reference's AccuracyLayer does (caffe/src/caffe/layers/accuracy_layer.cpp:
partial_sort with std::greater<pair>); the loss oracle is fp64 ``log_softmax`` with explicit
masking.

Error bounds (derived from the number formats, never from a kernel's output):

* fp32 probabilities: ``exp(a)`` evaluated as ``exp2(a * log2(e))`` carries the rounding of
  the product, a relative error of about ``|a| * 2^-24`` (4e-6 at ``|a| = 64``); the row sum
  and the reciprocal add a few ulp.  Allowed: 4e-5 relative (8x margin) plus 1e-37 absolute
  for values flushed below the normal range.
* loss: 4e-5 relative plus 2^-22 (a few ulp of a probability near 1) per contributing row,
  scaled by 1 / normaliser.
* bf16 outputs: one round-to-nearest of an fp32 value, ``2^-7 * |ref|`` plus the fp32 error
  of the value that is rounded (given at each use).
"""
import functools
import math
import zlib

import torch

FLT_MIN = 1.1754943508222875e-38          # smallest normal fp32: the clamp of the label probability
NLL_MAX = -math.log(FLT_MIN)              # 87.3365...: the row loss under the clamp
P_REL, P_ABS = 4e-5, 1e-37                # fp32 probability bound
ROW_ABS = 2.0 ** -22                      # per-row loss term
BF16_REL = 2.0 ** -7                      # one bf16 rounding

# (M, C): smallest input; C below one wave; either side of one wave; two strides + 1; many
# strides; second and third trip of the 1024-thread reduce loop with M % 4 = 1 and 3
GRID = [(1, 2), (3, 10), (5, 63), (6, 64), (7, 65), (9, 129), (130, 1000), (1029, 10), (2051, 3)]
IGNORES = [None, 0, "C+5", -1]


def grid_id(mc):
    return f"{mc[0]}x{mc[1]}"


def resolve_ignore(ignore, C):
    return C + 5 if ignore == "C+5" else ignore


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def make_labels(M, C, ignore=None, all_ignored=False, seed=0):
    """Random labels in [0, C); with an ignore label about a quarter of the rows (every row
    with index % 4 == 1) carry it."""
    lab = torch.randint(0, C, (M,), generator=_gen("lab", M, C, seed)).float()
    if ignore is not None:
        lab[1::4] = float(ignore)
        if all_ignored:
            lab[:] = float(ignore)
    return lab


def make_logits(M, C, regime="randn", labels=None, seed=0):
    """bf16 logits.  ``randn``: N(0, 4).  The other regimes clip the background to [-4, 4],
    put the row maximum at class (label + 1) % C and set the label's score:
    ``saturated``  60 below the row maximum (8 / -52): p ~ e^-60, still a normal fp32;
    ``clamped``    100 below it (8 / -92): p < FLT_MIN, the clamp of the label probability applies;
    ``confident``  20 above every other score (24 / 4): p within 1e-8 * C of 1."""
    x = torch.randn(M, C, generator=_gen("x", M, C, seed)) * 2
    if regime != "randn":
        lab = labels.long().clamp(0, C - 1)
        other = (lab + 1) % C
        r = torch.arange(M)
        x = x.clamp(-4, 4)
        hi, lo = {"saturated": (8.0, -52.0), "clamped": (8.0, -92.0), "confident": (4.0, 24.0)}[regime]
        x[r, other] = hi
        x[r, lab] = lo
    return x.bfloat16()


# --------------------------------------------------------------------------------------
# fp64 SoftmaxWithLoss / Softmax oracles
# --------------------------------------------------------------------------------------

def xent_ref64(x, labels, ignore=None, normalize=True, outer_num=None, loss_weight=1.0):
    """fp64 SoftmaxWithLoss of bf16 logits: dict with loss, prob, norm (python number), count of
    valid rows, per-row nll and dx = (prob - onehot) * valid * loss_weight / norm."""
    x64 = x.double()
    M, C = x64.shape
    lab = labels.reshape(-1).to(torch.int64)
    valid = torch.ones(M, dtype=torch.bool) if ignore is None else lab != int(ignore)
    logp = torch.log_softmax(x64, dim=-1)
    prob = torch.softmax(x64, dim=-1)
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    nll = -logp.gather(1, safe[:, None])[:, 0]
    nll = torch.clamp(nll, max=NLL_MAX)                      # -log(max(p, FLT_MIN))
    nll = torch.where(valid, nll, torch.zeros_like(nll))
    count = int(valid.sum())
    norm = float(max(count if normalize else (outer_num if outer_num is not None else M), 1))
    onehot = torch.zeros_like(prob)
    onehot[torch.arange(M), safe] = 1.0
    lw = float(torch.tensor(loss_weight, dtype=torch.float32))   # the kernel reads an fp32 weight
    dx = (prob - onehot) * valid[:, None].double() * (lw / norm)
    return dict(loss=float(nll.sum() / norm), prob=prob, norm=norm, count=count, nll=nll, dx=dx,
                valid=valid, scale=lw / norm)


def loss_bound(ref):
    return P_REL * abs(ref["loss"]) + ROW_ABS * ref["count"] / ref["norm"]


def prob_bound(ref):
    return P_REL * ref["prob"] + P_ABS


def xent_dx_bound(ref):
    """bf16 rounding of (prob - onehot) * scale: the fp32 error of prob, times the scale."""
    return BF16_REL * ref["dx"].abs() + (P_REL * ref["prob"] * abs(ref["scale"]) + P_ABS)


def softmax_y_bound(y64):
    return BF16_REL * y64 + (P_REL * y64 + P_ABS)


def softmax_bwd_ref64(dy, y):
    y64, d64 = y.double(), dy.double()
    return y64 * (d64 - (d64 * y64).sum(-1, keepdim=True))


def softmax_bwd_bound(dy, y, dx64):
    """dx = y * (dy - sum(dy * y)): the bf16 products are exact in fp32; a sum of depth
    ceil(C / 64) (per lane) + 6 (wave shuffles) errs by at most depth * 2^-24 * sum|dy * y|
    (2x margin taken: 2^-23); the subtraction and the product add 2^-24 relative each."""
    C = y.shape[1]
    depth = -(-C // 64) + 8
    s_abs = (dy.double() * y.double()).abs().sum(-1, keepdim=True)
    a = y.double().abs() * depth * 2.0 ** -23 * s_abs + 2.0 ** -22 * dx64.abs() + P_ABS
    return BF16_REL * dx64.abs() + a


# --------------------------------------------------------------------------------------
# top-k oracle: the reference's sort of (score, class index) pairs
# --------------------------------------------------------------------------------------

def _pair_lt(a, b):
    """Lexicographic a < b of (score, index) pairs built from ``<`` alone, as std::pair's."""
    return a[0] < b[0] or (not (b[0] < a[0]) and a[1] < b[1])


def _pair_desc(a, b):
    return -1 if _pair_lt(b, a) else (1 if _pair_lt(a, b) else 0)


@functools.lru_cache(maxsize=None)
def _ranking(row):
    pairs = [(s, i) for i, s in enumerate(row)]
    if any(s != s for s in row):   # NaN: tuples would compare by identity; use the pair order
        pairs.sort(key=functools.cmp_to_key(_pair_desc))
    else:
        pairs.sort(reverse=True)
    return tuple(i for _, i in pairs)


def topk_oracle(x, labels, k, ignore=None):
    """(hits, n_valid): rows whose label is among the first k of the descending sort of
    (score, index) pairs; rows carrying the ignore label are skipped."""
    rows = x.float().tolist()
    labs = [int(v) for v in labels.reshape(-1).tolist()]
    hits = n = 0
    for row, lab in zip(rows, labs):
        if ignore is not None and lab == int(ignore):
            continue
        n += 1
        hits += lab in _ranking(tuple(row))[:k]
    return hits, n


def check_accuracy(acc, x, labels, k, ignore=None):
    """Exact: bf16 / fp32 scores compare exactly, acc = hits / max(n_valid, 1) in fp32."""
    hits, n = topk_oracle(x, labels, k, ignore)
    acc = float(acc)
    if n == 0:
        assert acc == 0.0, acc
    else:
        assert round(acc * n) == hits and abs(acc - hits / n) < 1e-6, (acc, hits, n)
    return hits, n


def half_logits(M, C, seed=0):
    """Scores rounded to multiples of 0.5 (exact in bf16): ties in most rows."""
    x = torch.randn(M, C, generator=_gen("half", M, C, seed)) * 2
    return (torch.round(x * 2) / 2).bfloat16()


def accuracy_cases():
    """{name: (x bf16 [M, C], labels [M] float, top_k tuple, ignore_label or None)}"""
    cases = {}
    cases["zeros_37x10"] = (torch.zeros(37, 10).bfloat16(), make_labels(37, 10), (1, 5, 10), None)
    xh = half_logits(203, 10)
    cases["half_203x10"] = (xh, make_labels(203, 10), (1, 3, 5, 10), None)
    cases["randn_203x1000"] = (make_logits(203, 1000), make_labels(203, 1000), (1, 5), None)
    # all-NaN rows among normal rows: every class ties, the label's rank is C - 1 - label
    xn = half_logits(9, 10, seed=1).float()
    ln = make_labels(9, 10, seed=1)
    xn[2], xn[5], xn[8] = float("nan"), float("nan"), float("nan")
    ln[2], ln[5], ln[8] = 9.0, 4.0, 7.0
    cases["nan_rows_9x10"] = (xn.bfloat16(), ln, (1, 3, 5, 6), None)
    for ig in (0, 255, -1):
        cases[f"ignore_{ig}_203x10"] = (xh, make_labels(203, 10, ignore=ig), (1, 3), ig)
        cases[f"all_ignored_{ig}_37x10"] = (half_logits(37, 10, seed=2),
                                            make_labels(37, 10, ignore=ig, all_ignored=True), (1, 5), ig)
    # label at index 0 tied with index 64: the tie sits in lane 0's second stride
    xt = -1.0 - torch.rand(6, 65, generator=_gen("tie65"))
    xt[:, 0] = 1.0
    xt[:, 64] = 1.0
    cases["tie_0_vs_64_6x65"] = (xt.bfloat16(), torch.zeros(6), (1, 2), None)
    # label at index 63 of 64: nothing has a higher index, so a tie never outranks it
    xl = half_logits(6, 64, seed=3).float()
    xl[0] = 0.0
    xl[1:, 63] = xl[1:].max(dim=1).values
    cases["label_last_6x64"] = (xl.bfloat16(), torch.full((6,), 63.0), (1, 2), None)
    return cases


ACCURACY_CASES = accuracy_cases()
