"""ctypes wrappers of ``csrc/kernels/layers.hip``: the non-hot Caffe layer families on the
GPU (neurons, PReLU, Eltwise, BatchNorm / MVN, axis copies, layout changes, row gathers /
scatter-adds, Reduction, ArgMax, Caffe-ordered Im2col, the loss family) and of
``csrc/kernels/bn_scale.hip`` (fused BatchNorm -> Scale -> ReLU, per-channel Scale / Bias) and
``csrc/kernels/se.hip`` (global average pool, per-image per-channel affine: Axpy, (N, C) Scale / Bias).

Every function launches HIP kernels on torch's current stream (graph-capturable); torch is
used only to allocate outputs.  Tensors must be contiguous bf16 or fp32 device tensors.
Shapes are described as ``[B][outer][A][inner]`` decompositions of the PHYSICAL layout.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

call = _lib.call

NEURON = {"Sigmoid": 0, "TanH": 1, "AbsVal": 2, "BNLL": 3, "Exp": 4, "Log": 5, "Power": 6, "Threshold": 7}
RED_SUM, RED_DOT, RED_SQ, RED_PRELU, RED_ABS, RED_CSQ = 0, 1, 2, 3, 4, 5
LOSS = {"Euclidean": 0, "HingeL1": 1, "HingeL2": 2, "Multinomial": 3, "Infogain": 4, "SigmoidXent": 5,
        "Contrastive": 6}


def dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return 1
    if t.dtype == torch.bfloat16:
        return 0
    raise TypeError(f"layers_hip: unsupported dtype {t.dtype}")


def _c(t):
    if t is None:
        return None
    return t if t.is_contiguous() else t.contiguous()


# -- neurons -------------------------------------------------------------------------------
def neuron_fwd(kind: str, x, out_dtype=None, a=0.0, b=0.0, c=0.0):
    x = _c(x)
    y = torch.empty(x.shape, dtype=out_dtype or x.dtype, device=x.device)
    call("neuron_fwd", NEURON[kind], x, y, x.numel(), dt(x), dt(y), float(a), float(b), float(c))
    return y


def neuron_bwd(kind: str, x, y, dy, a=0.0, b=0.0, c=0.0):
    dy = _c(dy)
    dx = torch.empty_like(dy)
    call("neuron_bwd", NEURON[kind], _c(x), _c(y), dy, dx, dy.numel(), dt(x) if x is not None else 0,
         dt(y) if y is not None else 0, dt(dy), float(a), float(b), float(c))
    return dx


def prelu_fwd(x, slope, C_, inner, out_dtype=None):
    x = _c(x)
    y = torch.empty(x.shape, dtype=out_dtype or x.dtype, device=x.device)
    call("prelu_fwd", x, _c(slope), y, x.numel(), C_, inner, dt(x), dt(y))
    return y


def prelu_bwd(x, dy, slope, C_, inner):
    """dx in dy's dtype; x may be in another dtype (an fp32 2-D Input blob)."""
    dy = _c(dy)
    dx = torch.empty_like(dy)
    call("prelu_bwd", _c(x), dy, _c(slope), dx, dy.numel(), C_, inner, dt(x), dt(dy))
    return dx


# -- deterministic reductions --------------------------------------------------------------
def axis_reduce(mode, p, q, B, outer, A, inner, out=None, scale=1.0, acc=False):
    """out[b*A + a] (+)= scale * sum over (outer, inner) of f(p, q) (fp32, deterministic)."""
    p = _c(p)
    q = _c(q)
    k = _lib.kernels()
    k.sn_axis_reduce_splits.restype = C.c_longlong
    splits = int(k.sn_axis_reduce_splits(C.c_longlong(B), C.c_longlong(outer), C.c_longlong(A),
                                         C.c_longlong(inner)))
    part = torch.empty(splits * B * A, dtype=torch.float32, device=p.device)
    if out is None:
        out = torch.empty(B * A, dtype=torch.float32, device=p.device)
        acc = False
    call("axis_reduce", mode, p, q, dt(p), dt(q) if q is not None else 0, B, outer, A, inner, part, out,
         float(scale), int(acc))
    return out


def stats_finalize(s1, s2, count, eps, mode):
    n = s1.numel()
    mean = torch.empty(n, dtype=torch.float32, device=s1.device)
    var = torch.empty_like(mean)
    inv = torch.empty_like(mean)
    call("stats_finalize", s1, s2, n, 1.0 / max(count, 1), float(eps), mode, mean, var, inv)
    return mean, var, inv


def mean_var(x, B, outer, A, inner, eps, mode):
    """Per-(b, a) mean, variance and inverse scale of x over (outer, inner) in two
    deterministic passes: the mean, then the CENTRED second moment E[(x - mean)^2]
    (Caffe's batch_norm_layer.cu:50-59 / mvn_layer.cu:31-36 order, no E[x^2] - EX^2
    cancellation).  mode as stats_finalize: 0 BatchNorm, 1 MVN."""
    count = outer * inner
    s1 = axis_reduce(RED_SUM, x, None, B, outer, A, inner)
    mean, _, _ = stats_finalize(s1, None, count, eps, 2)
    s2 = axis_reduce(RED_CSQ, x, mean, B, outer, A, inner)
    return stats_finalize(s1, s2, count, eps, mode | 4)


def chan_affine(x, mean, inv, outer, A, inner, out_dtype=None):
    x = _c(x)
    y = torch.empty(x.shape, dtype=out_dtype or x.dtype, device=x.device)
    call("chan_affine", x, y, x.numel(), outer, A, inner, mean, inv, dt(x), dt(y))
    return y


def norm_bwd(dy, xhat, m1, m2, inv, outer, A, inner):
    dy = _c(dy)
    dx = torch.empty_like(dy)
    call("norm_bwd", dy, _c(xhat), dx, dy.numel(), outer, A, inner, m1, m2, inv, dt(dy),
         dt(xhat) if xhat is not None else 0)
    return dx


def bn_running(mean, var, factor, bmean, bvar, frac, unbias):
    call("bn_running", mean, var, factor, bmean, bvar, mean.numel(), float(frac), float(unbias))


def bn_global(rm, rv, factor, eps):
    Cn = rm.numel()
    mean = torch.empty(Cn, dtype=torch.float32, device=rm.device)
    inv = torch.empty_like(mean)
    call("bn_global", rm, rv, factor, Cn, float(eps), mean, inv)
    return mean, inv


# -- fused BatchNorm -> Scale -> ReLU, per-channel Scale / Bias (csrc/kernels/bn_scale.hip) ----
# x / y / dy / dx: contiguous [R][C_] tensors of one dtype (bf16 or fp32); per-channel vectors fp32.
# ``stats`` = (mode, a, b, factor, eps): BN_NONE (no normalisation), BN_BATCH (a = mean,
# b = inv_std) or BN_GLOBAL (a / b / factor = the running blobs, scaled inside the kernels).
BN_NONE, BN_BATCH, BN_GLOBAL = 0, 1, 2
GRAD_SKIP, GRAD_STORE, GRAD_ACC = 0, 1, 2
NO_STATS = (BN_NONE, None, None, None, 0.0)


def _bn_part(t, R, C_):
    k = _lib.kernels()
    k.sn_bn_part_floats.restype = C.c_longlong
    n = int(k.sn_bn_part_floats(C.c_longlong(R), C.c_longlong(C_), C.c_longlong(dt(t))))
    if n <= 0:
        raise ValueError(f"layers_hip: unsupported per-channel geometry R={R} C={C_}")
    return torch.empty(n, dtype=torch.float32, device=t.device), n


def bn_stats(x, R, C_, eps, running=None, frac=0.0, unbias=1.0):
    """(mean, var, inv_std) of x over its rows in one read (Welford partials, fixed-order
    merge); ``running`` = (mean, var, factor) blobs to update in the same finalize launch."""
    x = _c(x)
    part, n = _bn_part(x, R, C_)
    mean = torch.empty(C_, dtype=torch.float32, device=x.device)
    var = torch.empty_like(mean)
    inv = torch.empty_like(mean)
    rm, rv, rf = running if running is not None else (None, None, None)
    call("bn_stats", x, dt(x), R, C_, part, n, float(eps), mean, var, inv, rm, rv, rf, float(frac), float(unbias))
    return mean, var, inv


def bn_fwd(x, R, C_, stats, gamma=None, beta=None, relu=False):
    """y = relu?(gamma (x - mean) inv_std + beta), one launch."""
    x = _c(x)
    mode, a, b, f, eps = stats
    y = torch.empty_like(x)
    call("bn_fwd", x, y, dt(x), R, C_, a, b, f, float(eps), mode, gamma, beta, int(bool(relu)))
    return y


def bn_bwd_reduce(dy, x, y, R, C_, stats, relu, dgamma=None, gflag=GRAD_SKIP, dbeta=None, bflag=GRAD_SKIP,
                  want_coef=True):
    """Pass 1 of the backward: dbeta (+)= sum g, dgamma (+)= sum g xhat with g = dy [y > 0];
    returns the [2][C_] coefficients of bn_bwd_dx (None unless ``want_coef``)."""
    dy = _c(dy)
    mode = stats[0]
    need_x = gflag != GRAD_SKIP or mode == BN_BATCH
    part, n = _bn_part(dy, R, C_)
    coef = torch.empty(2 * C_, dtype=torch.float32, device=dy.device) if want_coef else None
    call("bn_bwd_reduce", dy, _c(x) if need_x else None, _c(y) if relu else None, dt(dy), R, C_, stats[1], stats[2],
         stats[3], float(stats[4]), mode, int(bool(relu)), int(need_x), part, n, dgamma, gflag, dbeta, bflag, coef)
    return coef


def bn_bwd_dx(dy, x, y, R, C_, stats, relu, gamma, coef):
    """Pass 2: dx = gamma inv_std (g - sum g / M - xhat sum g xhat / M); without batch
    statistics dx = g gamma inv_std."""
    dy = _c(dy)
    mode = stats[0]
    dx = torch.empty_like(dy)
    call("bn_bwd_dx", dy, _c(x) if mode == BN_BATCH else None, _c(y) if relu else None, dx, dt(dy), R, C_, stats[1],
         stats[2], stats[3], float(stats[4]), mode, int(bool(relu)), gamma, coef)
    return dx


def axis_scale_bias(x, s, b, A, inner):
    """y = x * s[a] + b[a] over [outer][A][inner] (s / b fp32 vectors, either may be None)."""
    x = _c(x)
    y = torch.empty_like(x)
    call("axis_scale_bias", x, y, x.numel(), A, inner, s, b, dt(x))
    return y


def cast(x, dtype):
    """Copy of x in another supported dtype."""
    return neuron_fwd("Power", x, dtype, 1.0, 1.0, 0.0)


# -- squeeze-and-excitation: global average pool, per-(image, channel) affine (csrc/kernels/se.hip) ----
# x / r / y / dy / dx: contiguous [N][HW][C_] tensors of one dtype (bf16 or fp32); the coefficients
# s / b and the gradients ds / db are fp32 [N][C_] (any shape of N * C_ elements).
def _nc_part(t, N, HW, C_):
    k = _lib.kernels()
    k.sn_nc_part_floats.restype = C.c_longlong
    n = int(k.sn_nc_part_floats(C.c_longlong(N), C.c_longlong(HW), C.c_longlong(C_), C.c_longlong(dt(t))))
    if n < 0:
        raise ValueError(f"layers_hip: unsupported per-image geometry N={N} HW={HW} C={C_}")
    return (torch.empty(n, dtype=torch.float32, device=t.device) if n else None), n


def _nc_vec(v, N, C_, out=False):
    if v is None:
        return None
    if v.dtype != torch.float32 or v.numel() != N * C_ or (out and not v.is_contiguous()):
        raise ValueError(f"layers_hip: an (N, C) coefficient must be {'contiguous ' if out else ''}fp32 with "
                         f"{N * C_} elements, got {v.dtype} {tuple(v.shape)}")
    return _c(v)


def gap_fwd(x, N, HW, C_):
    """y[n, c] = mean over the HW rows of image n, accumulated in fp32: (N, 1, 1, C_) in x's dtype."""
    x = _c(x)
    part, n = _nc_part(x, N, HW, C_)
    y = torch.empty((N, 1, 1, C_), dtype=x.dtype, device=x.device)
    call("gap_fwd", x, y, dt(x), N, HW, C_, part, n)
    return y


def nc_affine_fwd(x, N, HW, C_, s=None, b=None, r=None):
    """y = x * s[n, c] + b[n, c] + r in one pass (each of s, b, r may be None)."""
    x = _c(x)
    if r is not None and (r.dtype != x.dtype or r.numel() != x.numel()):
        raise ValueError("layers_hip: nc_affine_fwd's r must match x in dtype and size")
    y = torch.empty_like(x)
    call("nc_affine_fwd", x, _c(r), y, dt(x), N, HW, C_, _nc_vec(s, N, C_), _nc_vec(b, N, C_))
    return y


def nc_affine_bwd(dy, N, HW, C_, s=None, x=None, want_dx=True, ds=None, sflag=GRAD_SKIP, db=None, bflag=GRAD_SKIP):
    """One pass over dy (and x when ``sflag``): returns dx = dy * s (None unless ``want_dx``);
    ds (+)= sum over HW of dy * x and db (+)= sum over HW of dy under the GRAD_* flags."""
    dy = _c(dy)
    if sflag != GRAD_SKIP and (x is None or x.dtype != dy.dtype or x.numel() != dy.numel()):
        raise ValueError("layers_hip: nc_affine_bwd's ds needs x in dy's dtype and size")
    if want_dx and s is None:
        raise ValueError("layers_hip: nc_affine_bwd's dx needs s (without a scale dx is dy itself)")
    part, n = _nc_part(dy, N, HW, C_) if (sflag != GRAD_SKIP or bflag != GRAD_SKIP) else (None, 0)
    dx = torch.empty_like(dy) if want_dx else None
    call("nc_affine_bwd", dy, _c(x) if sflag != GRAD_SKIP else None, dx, dt(dy), N, HW, C_, _nc_vec(s, N, C_), part, n,
         _nc_vec(ds, N, C_, True) if sflag != GRAD_SKIP else None, sflag,
         _nc_vec(db, N, C_, True) if bflag != GRAD_SKIP else None, bflag)
    return dx


# -- eltwise -------------------------------------------------------------------------------
def _ptrs(xs):
    arr = (C.c_void_p * len(xs))(*[t.data_ptr() for t in xs])
    return arr


def eltwise_fwd(op, xs, coeffs):
    xs = [_c(x) for x in xs]
    y = torch.empty_like(xs[0])
    mask = torch.empty(xs[0].shape, dtype=torch.int32, device=y.device) if op == 2 else None
    co = (C.c_float * len(xs))(*[float(c) for c in coeffs])
    call("eltwise_fwd", _ptrs(xs), co, len(xs), op, y, mask, y.numel(), dt(y))
    return y, mask


def eltwise_bwd(op, xs, coeffs, which, stable, y, dy, mask):
    xs = [_c(x) for x in xs]
    dy = _c(dy)
    dx = torch.empty_like(dy)
    co = (C.c_float * len(xs))(*[float(c) for c in coeffs])
    call("eltwise_bwd", _ptrs(xs), co, len(xs), op, which, int(stable), _c(y), dy, mask, dx, dy.numel(), dt(dy))
    return dx


# -- copies / layout -----------------------------------------------------------------------
def axis_copy(src, dst, outer, srcA, dstA, inner, src_off, dst_off, cnt, acc=False):
    call("axis_copy", _c(src), dst, outer, srcA, dstA, inner, src_off, dst_off, cnt, dt(src), dt(dst), int(acc))


def tile_bwd(src, outer, A, inner, tiles, out_shape):
    dst = torch.empty(out_shape, dtype=src.dtype, device=src.device)
    call("tile_bwd", _c(src), dst, outer, A, inner, tiles, dt(src))
    return dst


def transpose(src, N, R, Ccols, out_shape=None, out_dtype=None):
    """[N][R][Ccols] -> [N][Ccols][R] (NHWC <-> NCHW with R = HW / C)."""
    dst = torch.empty(out_shape if out_shape is not None else (N, Ccols, R), dtype=out_dtype or src.dtype,
                      device=src.device)
    call("transpose", _c(src), dst, N, R, Ccols, dt(src), dt(dst))
    return dst


def nhwc_to_nchw(t, out_dtype=None):
    N, H, W, Cn = t.shape
    return transpose(t, N, H * W, Cn, (N, Cn, H, W), out_dtype)


def nchw_to_nhwc(t, N, Cn, H, W, out_dtype=None):
    return transpose(t, N, Cn, H * W, (N, H, W, Cn), out_dtype)


# -- gathers / scatter-adds ----------------------------------------------------------------
def gather_rows(src, idx, rows, row_len, out_shape, bias=None, out_dtype=None):
    idx = _c(idx)
    dst = torch.empty(out_shape, dtype=out_dtype or src.dtype, device=src.device)
    call("gather_rows", _c(src), idx, int(idx.dtype == torch.int32), dst, rows, row_len, bias, dt(src), dt(dst))
    return dst


def index_add_rows(src, idx, n_dst, row_len, dst, acc):
    idx = _c(idx)
    call("index_add_rows", _c(src), idx, int(idx.dtype == torch.int32), idx.numel(), dst, n_dst, row_len,
         dt(src), dt(dst), int(acc))
    return dst


# -- Reduction / ArgMax / Im2col ------------------------------------------------------------
def reduction_bwd(x, dy, segs, L, op, coeff):
    x = _c(x)
    dx = torch.empty_like(x)
    call("reduction_bwd", x, _c(dy), dx, segs, L, op, float(coeff), dt(x))
    return dx


def topk(x, outer, A, inner, k, out_max_val, axis_mode, out_shape):
    out = torch.empty(out_shape, dtype=torch.float32, device=x.device)
    call("topk", _c(x), outer, A, inner, k, int(out_max_val), int(axis_mode), out, dt(x))
    return out


def im2col_caffe(x, g, out_shape):
    col = torch.empty(out_shape, dtype=x.dtype, device=x.device)
    call("im2col_caffe", _c(x), col, *g, dt(x))
    return col


def col2im_caffe(dcol, g, out_shape):
    dx = torch.empty(out_shape, dtype=dcol.dtype, device=dcol.device)
    call("col2im_caffe", _c(dcol), dx, *g, dt(dcol))
    return dx


# -- losses --------------------------------------------------------------------------------
def loss_rows_fwd(kind, x, t, label, H, M, C_, margin=0.0, legacy=False):
    """Per-row loss terms [M] (and d2 [M] for Contrastive) -> (row_loss, workspace)."""
    x = _c(x)
    ws = torch.empty(3 * M, dtype=torch.float32, device=x.device)
    call("loss_rows_fwd", LOSS[kind], x, _c(t), _c(label), _c(H), M, C_, dt(x), dt(t) if t is not None else 0,
         float(margin), int(legacy), ws)
    return ws


def loss_sum(ws, M, scale):
    """0-d fp32 loss = scale * sum(ws[:M]) (device, no host sync)."""
    out = torch.empty((), dtype=torch.float32, device=ws.device)
    call("vsum", ws, M, out, float(scale), 0)
    return out


def loss_rows_bwd(kind, x, t, label, H, M, C_, loss_weight, scale, sign=1.0, ws=None, margin=0.0, legacy=False):
    x = _c(x)
    dx = torch.empty_like(x)
    d2 = ws[M:2 * M] if ws is not None else None
    call("loss_rows_bwd", LOSS[kind], x, _c(t), _c(label), _c(H), M, C_, dt(x), dt(t) if t is not None else 0,
         float(margin), int(legacy), _c(loss_weight.reshape(-1).float()), float(scale), float(sign), d2, dx)
    return dx


# -- stochastic pooling ----------------------------------------------------------------------
def stopool(x, s, rng_state, stream, train):
    """(y, mask): mask holds the sampled window offset (train) for the max-pool backward."""
    x = _c(x)
    y = torch.empty((s.N, s.P, s.Q, s.C), dtype=x.dtype, device=x.device)
    mask = torch.empty((s.N, s.P, s.Q, s.C), dtype=torch.uint8, device=x.device) if train else None
    call("stopool", x, y, mask, s.N, s.H, s.W, s.C, s.P, s.Q, s.kh, s.kw, s.sh, s.sw, rng_state, int(stream),
         int(train))
    return y, mask
