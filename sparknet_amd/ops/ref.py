"""PyTorch fp32 reference implementations of every op (CPU path and test oracle).

Each function mirrors the Caffe CPU/GPU semantics of the corresponding layer (file:line
cited per function) on NHWC tensors.  Complex backward passes are obtained with
autograd on the forward formula, which gives the exact analytic gradient that the
reference's hand-written backward kernels implement.  These run on the CPU reference
path (``device='cpu'``) and serve as the oracle for the HIP kernel tests.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from .spec import POOL_AVE, POOL_MAX, ConvNdSpec, ConvSpec, PoolSpec


def nchw(x):
    return x.permute(0, 3, 1, 2)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _w_oihw(w, s: ConvSpec):
    return w.reshape(s.K, s.R, s.S, s.Cg).permute(0, 3, 1, 2)


# --- convolution (base_conv_layer.cpp:312-376, conv_layer.cpp) -----------------------

def conv_forward(x, w, b, s: ConvSpec, relu=False, ws=None, folded=None):
    y = F.conv2d(nchw(x.float()), _w_oihw(w.float(), s), b.float() if b is not None else None,
                 stride=(s.sh, s.sw), padding=(s.ph, s.pw), dilation=(s.dh, s.dw), groups=s.groups)
    if relu:
        y = F.relu(y)
    return nhwc(y).to(x.dtype)


# --- N-d convolution (base_conv_layer.cpp:16-40, im2col.cpp im2col_nd_cpu) ------------

def im2col_nd(x, s: ConvNdSpec, g: int = 0):
    """[num][C][ins] -> col [num * P][Cg * T] of channel group g (Caffe's (c, taps) order)."""
    xp = F.pad(x[:, g * s.Cg:(g + 1) * s.Cg], [p for d in reversed(s.pd) for p in (d, d)])
    taps = []
    import itertools
    for kk in itertools.product(*[range(k) for k in s.ks]):
        idx = [slice(None), slice(None)] + [slice(k0, k0 + st * (o - 1) + 1, st)
                                            for k0, st, o in zip(kk, s.st, s.outs)]
        taps.append(xp[tuple(idx)])
    col = torch.stack(taps, 2)  # [num][Cg][T][outs]
    return col.reshape(s.num, s.Cg * s.T, s.P).transpose(1, 2).reshape(s.num * s.P, s.Cg * s.T)


def conv_nd_forward(x, w, b, s: ConvNdSpec):
    """x [num][C][ins], w [K][Cg][ks] (Caffe layout) -> y [num][K][outs]."""
    x, w = x.float(), w.float()
    ys = []
    for g in range(s.groups):
        col = im2col_nd(x, s, g)
        wg = w[g * s.Kg:(g + 1) * s.Kg].reshape(s.Kg, -1)
        ys.append((col @ wg.t()).reshape(s.num, s.P, s.Kg).transpose(1, 2))
    y = torch.cat(ys, 1)
    if b is not None:
        y = y + b.float().view(1, -1, 1)
    return y.reshape((s.num, s.K) + s.outs)


def conv_nd_backward(dy, x, w, s: ConvNdSpec, need_dx: bool, dw=None, db=None):
    """Gradients of conv_nd_forward by autograd on the same formula; dw / db accumulate
    (Caffe's Backward adds into the param diffs).  x may be None when dw is None (the data
    gradient alone: a Deconvolution forward)."""
    if x is None:
        assert dw is None
        x = torch.zeros((s.num, s.C) + tuple(s.ins), dtype=dy.dtype)
    xr = x.float().detach().requires_grad_(need_dx)
    wr = w.float().detach().requires_grad_(dw is not None)
    y = conv_nd_forward(xr, wr, None, s)
    ins = [t for t in (xr, wr) if t.requires_grad]
    grads = torch.autograd.grad(y, ins, dy.float()) if ins else ()
    gi = iter(grads)
    dx = next(gi) if need_dx else None
    if dw is not None:
        dw += next(gi).reshape(dw.shape)
    if db is not None:
        db += dy.float().reshape(s.num, s.K, -1).sum((0, 2))
    return dx.to(x.dtype) if dx is not None else None


def _gated(dx, gate):
    """Backward of a slope-0 ReLU whose output is ``gate`` (fused into the producer)."""
    return dx if gate is None else dx * (gate > 0).to(dx.dtype)


def _acc(dst, val, accumulate):
    if accumulate:
        dst += val
    else:
        dst.copy_(val)


def conv_backward(dy, x, w, s: ConvSpec, need_dx: bool, dw=None, db=None, gate=None, ws=None,
                  dw_acc=True, db_acc=True):
    dyn = nchw(dy.float())
    xn = nchw(x.float())
    wo = _w_oihw(w.float(), s)
    dx = None
    if need_dx:
        dx = torch.nn.grad.conv2d_input(xn.shape, wo, dyn, stride=(s.sh, s.sw), padding=(s.ph, s.pw),
                                        dilation=(s.dh, s.dw), groups=s.groups)
        dx = _gated(nhwc(dx).to(x.dtype), gate)
    if dw is not None:
        gw = torch.nn.grad.conv2d_weight(xn, wo.shape, dyn, stride=(s.sh, s.sw), padding=(s.ph, s.pw),
                                         dilation=(s.dh, s.dw), groups=s.groups)
        _acc(dw, gw.permute(0, 2, 3, 1).reshape(dw.shape), dw_acc)
    if db is not None:
        _acc(db, dyn.sum(dim=(0, 2, 3)), db_acc)
    return dx


# --- deconvolution (deconv_layer.cpp): conv with roles of fwd/dgrad swapped ------------

def deconv_forward(x, w, b, s: ConvSpec):
    """x: [N,H,W,C=num_input]; w internal (C, R, S, K/g) i.e. Caffe (C, K/g, R, S) permuted."""
    wo = w.float().reshape(s.C, s.R, s.S, s.Kg).permute(0, 3, 1, 2)
    y = F.conv_transpose2d(nchw(x.float()), wo, b.float() if b is not None else None,
                           stride=(s.sh, s.sw), padding=(s.ph, s.pw), dilation=(s.dh, s.dw),
                           groups=s.groups)
    return nhwc(y).to(x.dtype)


# --- inner product (inner_product_layer.cpp) ------------------------------------------

def linear_forward(x2, w, b, relu=False):
    y = x2.float() @ w.float().t()
    if b is not None:
        y = y + b.float()
    if relu:
        y = F.relu(y)
    return y.to(x2.dtype)


def linear_backward(dy2, x2, w, need_dx, dw=None, db=None, gate=None, dw_acc=True, db_acc=True):
    dyf = dy2.float()
    if dw is not None:
        _acc(dw, dyf.t() @ x2.float(), dw_acc)
    if db is not None:
        _acc(db, dyf.sum(0), db_acc)
    if not need_dx:
        return None
    return _gated((dyf @ w.float()).to(x2.dtype), gate.reshape(x2.shape) if gate is not None else None)


# --- pooling (pooling_layer.cpp / .cu) -------------------------------------------------

def _pool_windows(x, s: PoolSpec, fill):
    """Padded NCHW input and its [N, C, P, Q, kh*kw] window view."""
    P, Q = s.P, s.Q
    Hp = (P - 1) * s.sh + s.kh
    Wp = (Q - 1) * s.sw + s.kw
    xn = nchw(x)
    pad_b = Hp - s.H - s.ph
    pad_r = Wp - s.W - s.pw
    xp = F.pad(xn, (s.pw, max(pad_r, 0), s.ph, max(pad_b, 0)), value=fill)
    xp = xp[:, :, :Hp, :Wp]
    win = xp.unfold(2, s.kh, s.sh).unfold(3, s.kw, s.sw)  # N,C,P,Q,kh,kw
    return win.reshape(*win.shape[:4], s.kh * s.kw)


def _ave_divisor(s: PoolSpec, device):
    P, Q = s.P, s.Q
    hs = torch.arange(P, device=device) * s.sh - s.ph
    ws = torch.arange(Q, device=device) * s.sw - s.pw
    he = torch.clamp(hs + s.kh, max=s.H + s.ph)
    we = torch.clamp(ws + s.kw, max=s.W + s.pw)
    return ((he - hs)[:, None] * (we - ws)[None, :]).float()


def _pool_fwd_f32(x, s: PoolSpec):
    if s.method == POOL_MAX:
        return _pool_windows(x, s, float("-inf")).max(dim=-1).values
    win = _pool_windows(x, s, 0.0)
    return win.sum(dim=-1) / _ave_divisor(s, x.device)


def pool_forward(x, s: PoolSpec):
    y = _pool_fwd_f32(x.float(), s)
    return nhwc(y).to(x.dtype)


def pool_backward(dy, x, s: PoolSpec, gate=False):
    xf = x.float().detach().requires_grad_(True)
    y = _pool_fwd_f32(xf, s)
    (g,) = torch.autograd.grad(y, xf, nchw(dy.float()))
    return _gated(g.to(x.dtype), x if gate else None)


# --- LRN (lrn_layer.cpp / .cu) -------------------------------------------------------

def _lrn_across_f32(x, size, alpha, beta, k):
    pre = (size - 1) // 2
    post = size - pre - 1
    sq = x * x
    sq = F.pad(sq, (pre, post))  # pad the channel (last) axis
    win = sq.unfold(-1, size, 1).sum(-1)
    scale = k + alpha / size * win
    return x * scale.pow(-beta)


def _lrn_within_f32(x, size, alpha, beta):
    pre = (size - 1) // 2
    s = PoolSpec(x.shape[0], x.shape[1], x.shape[2], x.shape[3], size, size, 1, 1, pre, pre, POOL_AVE)
    pooled = nhwc(_pool_fwd_f32(x * x, s))
    return x * (1 + alpha * pooled).pow(-beta)


def lrn_forward(x, size, alpha, beta, k, within=False):
    xf = x.float()
    y = _lrn_within_f32(xf, size, alpha, beta) if within else _lrn_across_f32(xf, size, alpha, beta, k)
    return y.to(x.dtype)


def lrn_backward(dy, x, size, alpha, beta, k, within=False, y=None):
    xf = x.float().detach().requires_grad_(True)
    y = _lrn_within_f32(xf, size, alpha, beta) if within else _lrn_across_f32(xf, size, alpha, beta, k)
    (g,) = torch.autograd.grad(y, xf, dy.float())
    return g.to(x.dtype)


# --- neurons (relu/sigmoid/tanh/... layers) --------------------------------------------

def shuffle_channels(x, groups: int):
    """Channel shuffle on the channels-last storage: ``y[..., j * groups + i] = x[..., i * (C // groups) + j]``
    (the reshape (groups, C / groups) -> transpose -> flatten of the ShuffleNet release)."""
    Cc = x.shape[-1]
    if groups < 1 or Cc % groups != 0:
        raise ValueError(f"shuffle_channels: {Cc} channels do not split into {groups} groups")
    return x.reshape(*x.shape[:-1], groups, Cc // groups).transpose(-1, -2).reshape(x.shape).contiguous()


def crop_window(x, offsets, shape):
    """The window of ``x`` at ``offsets`` with ``shape``, one entry per stored axis (crop_layer.cpp)."""
    return x[tuple(slice(o, o + n) for o, n in zip(offsets, shape))].contiguous()


def crop_window_backward(dy, offsets, shape):
    """Gradient of crop_window for a source of ``shape``: dy inside the window, zero outside."""
    dx = torch.zeros(tuple(shape), dtype=dy.dtype, device=dy.device)
    dx[tuple(slice(o, o + n) for o, n in zip(offsets, dy.shape))] = dy
    return dx


# --- region-of-interest layers (roi_pooling_layer.cu of the Fast R-CNN fork; Caffe2's RoIAlign) -------------
# x [N, H, W, C] of any float dtype, rois [R, 5] = (batch index, x1, y1, x2, y2) in image coordinates, y
# [R, PH, PW, C].  Bin edges and sample positions are computed in float32 in the order of operations of
# csrc/kernels/roi.hip, which defines them.  A ROI whose batch index is not in [0, N), or with a scaled
# coordinate that is not finite or beyond 2^20, is ignored: zeros, argmax -1, no gradient.  These functions
# read the ROIs on the host, so they cannot be captured into a graph.

ROI_COORD_MAX, ROI_ALIGN_MAX_GRID = float(1 << 20), 64


def _roi_coords(roi, N, scale):
    """(image, x1, y1, x2, y2) scaled in float32, or None for an ignored ROI."""
    c = [roi[k] * np.float32(scale) for k in range(1, 5)]
    if not 0 <= roi[0] < N or not all(abs(v) <= ROI_COORD_MAX for v in c):
        return None
    return (int(roi[0]), *c)


def _roi_round(v) -> int:  # half away from zero
    return int(math.copysign(math.floor(abs(float(v)) + 0.5), float(v)))


def _roi_pool_box(roi, N, PH, PW, scale):
    """(image, first row, first column, bin height, bin width) or None."""
    c = _roi_coords(roi, N, scale)
    if c is None:
        return None
    n, ws, hs, we, he = c[0], *(_roi_round(v) for v in c[1:])
    return n, hs, ws, np.float32(max(he - hs + 1, 1)) / np.float32(PH), np.float32(max(we - ws + 1, 1)) / np.float32(PW)


def _roi_pool_bin(p, size, start, L):
    """Bin p of an axis, [lo, hi) clipped to [0, L]."""
    lo = int(math.floor(np.float32(p) * size)) + start
    hi = int(math.ceil(np.float32(p + 1) * size)) + start
    return min(max(lo, 0), L), min(max(hi, 0), L)


def roi_pool_forward(x, rois, ph, pw, scale):
    """ROIPooling: (y, argmax [R, PH, PW, C] int32 holding h * W + w of the maximum, or -1); an empty bin
    gives 0 / -1, the first maximum in (h, w) order wins a tie."""
    N, H, W, C = x.shape
    table = rois.detach().float().cpu().numpy()
    y = torch.zeros((len(table), ph, pw, C), dtype=x.dtype, device=x.device)
    am = torch.full((len(table), ph, pw, C), -1, dtype=torch.int32, device=x.device)
    for r, roi in enumerate(table):
        box = _roi_pool_box(roi, N, ph, pw, scale)
        if box is None:
            continue
        n, hs, ws, bh, bw = box
        for i in range(ph):
            h0, h1 = _roi_pool_bin(i, bh, hs, H)
            for j in range(pw):
                w0, w1 = _roi_pool_bin(j, bw, ws, W)
                if h1 <= h0 or w1 <= w0:
                    continue
                win = x[n, h0:h1, w0:w1].reshape(-1, C)
                m = win.max(0).values
                first = ((win == m).int().cumsum(0) == 0).sum(0)  # entries before the first maximum
                y[r, i, j] = m
                am[r, i, j] = ((h0 + first // (w1 - w0)) * W + w0 + first % (w1 - w0)).int()
    return y, am


def roi_pool_backward(dy, rois, argmax, x_shape, ph, pw, scale):
    """Gradient of roi_pool_forward to x: dy added at the stored argmax, in (ROI, ph, pw) order."""
    N, H, W, C = x_shape
    table = rois.detach().float().cpu().numpy()
    dx = torch.zeros((N, H * W, C), dtype=torch.float32, device=dy.device)
    for r, roi in enumerate(table):
        box = _roi_pool_box(roi, N, ph, pw, scale)
        if box is None:
            continue
        idx = argmax[r].reshape(-1, C).long()
        dx[box[0]].scatter_add_(0, idx.clamp(min=0), dy[r].reshape(-1, C).float() * (idx >= 0))
    return dx.reshape(N, H, W, C).to(dy.dtype)


def _roi_align_axis(start, size, P, grid, L):
    """[P, L] float32: the weight each position of an axis of length L has in each of the P bins, summed
    over the bin's ``grid`` samples (bilinear; zero outside [-1, L], clamped to 0 and L - 1)."""
    m = np.zeros((P, L), dtype=np.float32)
    for p in range(P):
        for i in range(grid):
            v = start + np.float32(p) * size + (np.float32(i) + np.float32(0.5)) * size / np.float32(grid)
            if v < -1 or v > L:
                continue
            v = max(v, np.float32(0))
            lo = int(v)
            if lo >= L - 1:
                lo = hi = L - 1
                v = np.float32(lo)
            else:
                hi = lo + 1
            wh = v - np.float32(lo)
            m[p, lo] += np.float32(1) - wh
            m[p, hi] += wh
    return m


def _roi_align_weights(roi, x_shape, ph, pw, scale, sampling_ratio, device):
    """(image, Wy [PH, H], Wx [PW, W], samples per bin) or None: the bilinear weights are separable."""
    N, H, W, _ = x_shape
    c = _roi_coords(roi, N, scale)
    if c is None:
        return None
    n, x1, y1, x2, y2 = c
    rw, rh = max(x2 - x1, np.float32(1)), max(y2 - y1, np.float32(1))
    bh, bw = rh / np.float32(ph), rw / np.float32(pw)
    gh = sampling_ratio if sampling_ratio > 0 else int(math.ceil(rh / np.float32(ph)))
    gw = sampling_ratio if sampling_ratio > 0 else int(math.ceil(rw / np.float32(pw)))
    gh, gw = min(gh, ROI_ALIGN_MAX_GRID), min(gw, ROI_ALIGN_MAX_GRID)
    wy, wx = _roi_align_axis(y1, bh, ph, gh, H), _roi_align_axis(x1, bw, pw, gw, W)
    return n, torch.from_numpy(wy).to(device), torch.from_numpy(wx).to(device), gh * gw


def roi_align_forward(x, rois, ph, pw, scale, sampling_ratio=0):
    """ROIAlign (aligned = false): the mean of ``sampling_ratio`` (0: ceil(roi / pooled)) squared bilinear
    samples per bin; coordinates scaled and not rounded, the ROI at least one pixel wide and high."""
    table = rois.detach().float().cpu().numpy()
    y = torch.zeros((len(table), ph, pw, x.shape[3]), dtype=torch.float32, device=x.device)
    for r, roi in enumerate(table):
        wts = _roi_align_weights(roi, x.shape, ph, pw, scale, sampling_ratio, x.device)
        if wts is not None:
            n, wy, wx, count = wts
            y[r] = torch.einsum("ph,hwc,qw->pqc", wy, x[n].float(), wx) / count
    return y.to(x.dtype)


def roi_align_backward(dy, rois, x_shape, ph, pw, scale, sampling_ratio=0):
    """Gradient of roi_align_forward to x."""
    table = rois.detach().float().cpu().numpy()
    dx = torch.zeros(tuple(x_shape), dtype=torch.float32, device=dy.device)
    for r, roi in enumerate(table):
        wts = _roi_align_weights(roi, x_shape, ph, pw, scale, sampling_ratio, dy.device)
        if wts is not None:
            n, wy, wx, count = wts
            dx[n] += torch.einsum("ph,pqc,qw->hwc", wy, dy[r].float(), wx) / count
    return dx.to(dy.dtype)


def _smooth_l1_diff(pred, target, in_w):
    d = pred.float() - target.float().reshape(pred.shape)
    return d if in_w is None else d * in_w.float().reshape(pred.shape)


def smooth_l1_forward(pred, target, in_w=None, out_w=None, sigma=1.0):
    """SmoothL1Loss (smooth_L1_loss_layer.cu of the Fast R-CNN fork): d = in_w (pred - target), f(d) = 0.5
    sigma^2 d^2 below 1 / sigma^2, else |d| - 0.5 / sigma^2; sum(out_w f) / pred.shape[0] as a 0-d fp32."""
    d, s2 = _smooth_l1_diff(pred, target, in_w), float(sigma) ** 2
    f = torch.where(d.abs() < 1.0 / s2, 0.5 * s2 * d * d, d.abs() - 0.5 / s2)
    if out_w is not None:
        f = f * out_w.float().reshape(pred.shape)
    return (f.sum() / pred.shape[0]).reshape(())


def smooth_l1_backward(pred, target, in_w, out_w, sigma, loss_weight, need_target=False):
    """(gradient to pred in its dtype, gradient to target in fp32 or None): loss_weight / num in_w out_w f'(d)
    and its negative."""
    d, s2 = _smooth_l1_diff(pred, target, in_w), float(sigma) ** 2
    g = torch.where(d.abs() < 1.0 / s2, s2 * d, torch.sign(d)) * (loss_weight.float() / pred.shape[0])
    for wgt in (in_w, out_w):
        if wgt is not None:
            g = g * wgt.float().reshape(pred.shape)
    return g.to(pred.dtype), (-g).reshape(target.shape) if need_target else None


# --- proposal layer (rpn/proposal_layer.py, generate_anchors.py, nms of the public Faster R-CNN code) --------

def proposal_anchors(base_size=16, ratios=(0.5, 1, 2), scales=(8, 16, 32)):
    """The public generate_anchors: [len(ratios) len(scales), 4] float32 base anchors (x1, y1, x2, y2) around a
    ``base_size`` square at the origin, ratios outermost, with numpy's roundings."""
    ratios, scales = np.asarray(ratios, dtype=np.float64), np.asarray(scales, dtype=np.float64)

    def centred(ws, hs, cx, cy):
        return np.stack([cx - 0.5 * (ws - 1), cy - 0.5 * (hs - 1), cx + 0.5 * (ws - 1), cy + 0.5 * (hs - 1)], 1)

    centre = 0.5 * (base_size - 1)
    ws = np.round(np.sqrt(base_size * base_size / ratios))
    hs = np.round(ws * ratios)
    out = []
    for x1, y1, x2, y2 in centred(ws, hs, centre, centre):
        w, h = x2 - x1 + 1, y2 - y1 + 1
        out.append(centred(w * scales, h * scales, x1 + 0.5 * (w - 1), y1 + 0.5 * (h - 1)))
    return np.concatenate(out).astype(np.float32)


def _proposal_axis(lo, hi, d, dl):
    e = hi - lo + 1
    c = lo + 0.5 * e
    pc, pe = d * e + c, torch.exp(dl) * e
    return pc - 0.5 * pe, pc + 0.5 * pe


def proposal(scores, deltas, im_info, anchors, feat_stride, min_size, pre_nms_topn, post_nms_topn, nms_thresh):
    """The proposal layer of Faster R-CNN's RPN on the stored layout, the semantics of csrc/kernels/proposal.hip
    in fp32: ``scores`` [N, H, W, 2A] (foreground: channels A ..), ``deltas`` [N, H, W, 4A], ``im_info`` [N, 3] =
    (height, width, scale), ``anchors`` [A, 4]; box ``i = (h W + w) A + a``.  Decode, clip, drop boxes below
    ``min_size`` scale (and NaN scores, non-finite boxes, images whose im_info is NaN or not positive), rank by
    score with the lower index first among equals, keep ``pre_nms_topn`` (0: all), greedy NMS at IoU >
    ``nms_thresh``.  Returns (rois [N post, 5] fp32 as (image, x1, y1, x2, y2), scores [N post, 1] fp32, count
    [N] int32); an image's unused rows are (-1, 0, 0, 0, 0) with score 0.  The boxes are read on the host for
    the NMS loop, so this route cannot be captured into a graph."""
    N, H, W, A2 = scores.shape
    A, dev, f32 = A2 // 2, scores.device, torch.float32
    sc = scores[..., A:].float().reshape(N, -1) + 0.0  # -0 ranks, and is reported, as +0
    d = deltas.float().reshape(N, -1, 4)
    ws = torch.arange(W, dtype=f32, device=dev) * feat_stride
    hs = torch.arange(H, dtype=f32, device=dev) * feat_stride
    shift = torch.stack([ws.expand(H, W), hs[:, None].expand(H, W)] * 2, -1)
    anc = (torch.as_tensor(anchors, dtype=f32, device=dev) + shift[:, :, None, :]).reshape(-1, 4)
    info = im_info.float()
    good = ((info > 0) & torch.isfinite(info)).all(1)
    x1, x2 = _proposal_axis(anc[:, 0], anc[:, 2], d[..., 0], d[..., 2])
    y1, y2 = _proposal_axis(anc[:, 1], anc[:, 3], d[..., 1], d[..., 3])
    raw = torch.stack([x1, y1, x2, y2], -1)
    top = torch.stack([info[:, 1] - 1, info[:, 0] - 1] * 2, -1)[:, None, :]
    boxes = torch.maximum(torch.minimum(raw, top), torch.zeros((), dtype=f32, device=dev))
    lim = (min_size * info[:, 2])[:, None]
    keep = (torch.isfinite(raw).all(-1) & good[:, None] & ~torch.isnan(sc)
            & (boxes[..., 2] - boxes[..., 0] + 1 >= lim) & (boxes[..., 3] - boxes[..., 1] + 1 >= lim))
    rois = torch.zeros((N, post_nms_topn, 5), dtype=f32)
    rois[..., 0] = -1
    out_sc = torch.zeros((N, post_nms_topn, 1), dtype=f32)
    count = torch.zeros(N, dtype=torch.int32)
    boxes, sc, keep = boxes.cpu(), sc.cpu(), keep.cpu()
    for n in range(N):
        idx = torch.nonzero(keep[n]).flatten()
        order = idx[torch.sort(-sc[n, idx], stable=True).indices]
        if pre_nms_topn > 0:
            order = order[:pre_nms_topn]
        b = boxes[n, order].numpy()
        area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
        gone, kept = np.zeros(len(b), dtype=bool), []
        for i in range(len(b)):
            if gone[i]:
                continue
            kept.append(i)
            if len(kept) == post_nms_topn:
                break
            w = np.maximum(np.float32(0), np.minimum(b[i, 2], b[i + 1:, 2]) - np.maximum(b[i, 0], b[i + 1:, 0]) + 1)
            h = np.maximum(np.float32(0), np.minimum(b[i, 3], b[i + 1:, 3]) - np.maximum(b[i, 1], b[i + 1:, 1]) + 1)
            inter = w * h
            gone[i + 1:] |= inter / (area[i] + area[i + 1:] - inter) > np.float32(nms_thresh)
        k = len(kept)
        rois[n, :k, 0], rois[n, :k, 1:] = n, torch.from_numpy(b[kept].reshape(k, 4))
        out_sc[n, :k, 0] = sc[n, order[kept]]
        count[n] = k
    return rois.reshape(-1, 5).to(dev), out_sc.reshape(-1, 1).to(dev), count.to(dev)


# --- LSTM (upstream lstm_layer.cpp / lstm_unit_layer.cpp / recurrent_layer.cpp) -------------------------------

def lstm_forward(x2, cont, w_xc, b_c, w_hc, h0, c0, xs=None, w_xs=None, train=True):
    """The LSTM layer in fp32, a loop over t (the semantics of csrc/kernels/lstm.hip): pre = W_xc x_t + b_c
    (+ W_xs xs) + W_hc (cont_t h_{t-1}); i, f, o = sigmoid, g = tanh over the 4H axis in that order; c_t = cont_t
    f c_{t-1} + i g; h_t = o tanh(c_t).  ``x2`` [T N, D], ``cont`` [T, N], state ``h0`` / ``c0`` [N, H], overwritten by
    h_T / c_T.  Returns (h [T, N, H] in h0's dtype, saved = (cells [T + 1, N, H], gates [T, N, 4H], cont_t h_{t-1}
    [T, N, H]), all fp32)."""
    (T, N), H = cont.shape, w_hc.shape[1]
    cont, w_hc = cont.float(), w_hc.float()
    xg = (x2.float() @ w_xc.float().t() + b_c.float()).reshape(T, N, 4 * H)
    if xs is not None:
        xg = xg + xs.float() @ w_xs.float().t()
    h, cells, gates, hcs = h0.float(), [c0.float().clone()], [], []
    hs = []
    for t in range(T):
        hc = cont[t, :, None] * h
        pre = xg[t] + hc @ w_hc.t()
        a = torch.cat([torch.sigmoid(pre[:, :3 * H]), torch.tanh(pre[:, 3 * H:])], 1)
        c = cont[t, :, None] * a[:, H:2 * H] * cells[-1] + a[:, :H] * a[:, 3 * H:]
        h = a[:, 2 * H:3 * H] * torch.tanh(c)
        hs.append(h), cells.append(c), gates.append(a), hcs.append(hc)
    h0.copy_(h)
    c0.copy_(cells[-1])
    return torch.stack(hs).to(h0.dtype), (torch.stack(cells), torch.stack(gates), torch.stack(hcs))


def lstm_backward(dh, x2, cont, w_xc, w_hc, saved, need_dx, dw_xc=None, db=None, dw_hc=None, xs=None, w_xs=None,
                  dw_xs=None, need_dxs=False, acc=(True, True, True, True)):
    """Backward of lstm_forward for the top gradient ``dh`` [T, N, H]; ``acc``: accumulate or store into (dw_xc,
    db, dw_xs, dw_hc).  No gradient reaches the state a forward started from.  Returns (dx [T N, D], dxs)."""
    cells, gates, hcs = saved
    (T, N), H = cont.shape, w_hc.shape[1]
    cont, w_hc, dh = cont.float(), w_hc.float(), dh.float().reshape(T, N, H)
    dg = torch.zeros((T, N, 4 * H), dtype=torch.float32, device=dh.device)
    dc = torch.zeros((N, H), dtype=torch.float32, device=dh.device)
    for t in range(T - 1, -1, -1):
        d = dh[t] + (cont[t + 1, :, None] * (dg[t + 1] @ w_hc) if t < T - 1 else 0)
        i, f, o, g = gates[t].float().split(H, 1)
        ct, tc = cont[t, :, None], torch.tanh(cells[t + 1])
        dc = dc + d * o * (1 - tc * tc)
        dg[t] = torch.cat([dc * g * i * (1 - i), dc * ct * cells[t] * f * (1 - f), d * tc * o * (1 - o),
                           dc * i * (1 - g * g)], 1)
        dc = dc * ct * f
    dg2 = dg.reshape(T * N, 4 * H)
    if dw_hc is not None:
        _acc(dw_hc, dg2.t() @ hcs.float().reshape(T * N, H), acc[3])
    dx = linear_backward(dg2, x2.float(), w_xc, need_dx, dw_xc, db, dw_acc=acc[0], db_acc=acc[1])
    dxs = None
    if xs is not None and (dw_xs is not None or need_dxs):
        dxs = linear_backward(dg.sum(0), xs.float(), w_xs, need_dxs, dw_xs, None, dw_acc=acc[2])
    return dx, dxs


def relu_forward(x, slope=0.0):
    xf = x.float()
    return torch.where(xf > 0, xf, xf * slope).to(x.dtype)


def relu_backward(dy, x, slope=0.0):
    xf = x.float()
    return (dy.float() * torch.where(xf > 0, torch.ones_like(xf), torch.full_like(xf, slope))).to(dy.dtype)


# --- dropout (dropout_layer.cpp:14-18, .cu): keep iff u32 > UINT_MAX*p -----------------

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = 0xFFFFFFFF


def philox_u32(n: int, seed: int, counter: int, stream: int) -> torch.Tensor:
    """Dropout words for element indices 0..n-1: element e takes word e % 4 of
    Philox4x32-10 at counter e // 4 — bit-identical to the HIP kernels
    (csrc/kernels/common.h dropout_bits4) so CPU and GPU dropout masks agree."""
    n4 = -(-n // 4)
    return _philox4(n4, seed, counter, stream).reshape(-1)[:n]


def _philox4(n4: int, seed: int, counter: int, stream: int) -> torch.Tensor:
    """[n4, 4] Philox4x32-10 output words for counters 0..n4-1."""
    idx = torch.arange(n4, dtype=torch.int64)
    c0 = idx & _MASK32
    c1 = (idx >> 32) & _MASK32
    c1 = c1 | ((stream & 0xFFFF) << 16)
    c2 = torch.full_like(idx, counter & _MASK32)
    c3 = torch.full_like(idx, (counter >> 32) & _MASK32)
    k0 = seed & _MASK32
    k1 = (seed >> 32) & _MASK32
    for _ in range(10):
        p0 = c0 * _M0
        p1 = c2 * _M1
        hi0, lo0 = (p0 >> 32) & _MASK32, p0 & _MASK32
        hi1, lo1 = (p1 >> 32) & _MASK32, p1 & _MASK32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + _W0) & _MASK32
        k1 = (k1 + _W1) & _MASK32
    return torch.stack([c0, c1, c2, c3], dim=1)


def philox4_counters(seed: int, c0, c1: int, c2: int, c3: int) -> torch.Tensor:
    """Philox4x32-10 of arbitrary counters (c0 a tensor, c1..c3 scalars): [len(c0), 4]."""
    c0 = torch.as_tensor(c0, dtype=torch.int64) & _MASK32
    c1 = torch.full_like(c0, c1 & _MASK32)
    c2 = torch.full_like(c0, c2 & _MASK32)
    c3 = torch.full_like(c0, c3 & _MASK32)
    k0, k1 = seed & _MASK32, (seed >> 32) & _MASK32
    for _ in range(10):
        p0 = c0 * _M0
        p1 = c2 * _M1
        hi0, lo0 = (p0 >> 32) & _MASK32, p0 & _MASK32
        hi1, lo1 = (p1 >> 32) & _MASK32, p1 & _MASK32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + _W0) & _MASK32
        k1 = (k1 + _W1) & _MASK32
    return torch.stack([c0, c1, c2, c3], dim=1)


def augment_params(N: int, seed: int, counter: int, Hs: int, Ws: int, crop_h: int, crop_w: int, mirror: bool):
    """Per-image (row offset, column offset, mirror) of a training crop — the draw of the
    augment / augment_s2d kernels (csrc/kernels/augment.hip: Philox(seed) at counter
    (n, 0xA5A50000, counter)), so a CPU feeder reproduces the device crops exactly."""
    u = philox4_counters(seed, torch.arange(N), 0xA5A50000, counter & _MASK32, (counter >> 32) & _MASK32)
    ho = (u[:, 0] % (Hs - crop_h + 1)).tolist()
    wo = (u[:, 1] % (Ws - crop_w + 1)).tolist()
    mir = (u[:, 2] & 1).tolist() if mirror else [0] * N
    return list(zip(ho, wo, [bool(m) for m in mir]))


def dropout_mask(shape, ratio, seed, counter, stream, device):
    n = math.prod(shape)
    u = philox_u32(n, seed, counter, stream)
    thr = int(_MASK32 * ratio)
    return (u > thr).reshape(shape).to(device)


def dropout_forward(x, ratio, seed, counter, stream):
    scale = 1.0 / (1.0 - ratio)
    m = dropout_mask(x.shape, ratio, seed, counter, stream, x.device)
    return (x.float() * m * scale).to(x.dtype)


def dropout_backward(dy, ratio, seed, counter, stream, gate=None):
    return _gated(dropout_forward(dy, ratio, seed, counter, stream), gate)


# --- softmax / softmax-with-loss (softmax_loss_layer.cpp / .cu) ------------------------

def softmax_forward(x2):
    return torch.softmax(x2.float(), dim=-1).to(x2.dtype)


def softmax_backward(dy2, y2):
    y = y2.float()
    d = dy2.float()
    return (y * (d - (d * y).sum(-1, keepdim=True))).to(dy2.dtype)


def softmax_loss_forward(x2, labels, ignore_label=None, normalize=True, outer_num=None):
    """SoftmaxWithLoss forward (softmax_loss_layer.cpp:Forward_cpu).
    Returns (loss, prob, normalizer): loss = -sum log(max(p_label, FLT_MIN)) / normalizer,
    normalizer = #valid labels if ``normalize`` else outer_num."""
    prob = torch.softmax(x2.float(), dim=-1)
    lab = labels.reshape(-1).long()
    valid = torch.ones_like(lab, dtype=torch.bool)
    if ignore_label is not None:
        valid = lab != ignore_label
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    p = prob.gather(1, safe[:, None])[:, 0].clamp_min(torch.finfo(torch.float32).tiny)
    nll = torch.where(valid, -torch.log(p), torch.zeros_like(p))
    if normalize:
        norm = valid.sum().float()
    else:
        norm = torch.tensor(float(outer_num if outer_num is not None else x2.shape[0]))
    norm = torch.clamp(norm, min=1.0)
    return nll.sum() / norm, prob, norm


def softmax_loss_backward(prob, labels, loss_weight, norm, ignore_label=None, dtype=torch.float32):
    lab = labels.reshape(-1).long()
    g = prob.clone()
    valid = torch.ones_like(lab, dtype=torch.bool)
    if ignore_label is not None:
        valid = lab != ignore_label
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    g.scatter_add_(1, safe[:, None], torch.where(valid, -1.0, 0.0)[:, None])
    g = g * valid[:, None].float()
    lw = loss_weight.reshape(-1)[0].float() if torch.is_tensor(loss_weight) else loss_weight
    g = g * (lw / norm)
    return g.to(dtype)


def accuracy(x2, labels, top_k=1, ignore_label=None):
    lab = labels.reshape(-1).long()
    xf = x2.float()
    # accuracy_layer.cpp sorts (score, class index) pairs in descending order and looks for the
    # label among the first top_k: a class ranks ahead of the label when it scores strictly
    # higher, or when it does not compare below the label's score (a tie; NaN against NaN)
    # and has the higher index.
    lc = lab.clamp(0, xf.shape[1] - 1)[:, None]
    lab_score = xf.gather(1, lc)
    idx = torch.arange(xf.shape[1], device=xf.device)[None, :]
    ahead = (xf > lab_score) | (~(lab_score > xf) & (idx > lc))
    hit = (ahead.sum(1) < top_k).float()
    valid = torch.ones_like(hit, dtype=torch.bool)
    if ignore_label is not None:
        valid = lab != ignore_label
    n = valid.sum().float()
    return (hit * valid).sum() / torch.clamp(n, min=1.0)


# --- solver (sgd_solver.cpp:102-239) ----------------------------------------------------

def sgd_update(data, diff, hist, lr_vec, decay_vec, momentum, l1: bool, clip_scale: float):
    """In-place fused SGD on flat fp32 buffers; lr_vec/decay_vec are per-element
    (lr*lr_mult, wd*decay_mult)."""
    g = diff * clip_scale if clip_scale != 1.0 else diff.clone()
    if l1:
        g += decay_vec * torch.sign(data)
    else:
        g += decay_vec * data
    hist.mul_(momentum).add_(lr_vec * g)
    diff.copy_(hist)
    data.sub_(hist)


def solver_update_ref(kind, data, diff, hist, lr_mult, decay_mult, h, l1, clip):
    """Reference for every solver kind on flat fp32 buffers (CPU).  ``h`` = hyper list.
    Order: clip (global L2 of raw diffs) -> 1/iter_size -> L1/L2 decay -> update rule."""
    lr, mom, wd, clipv, norm, delta, mom2, rms, corr = h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8]
    scale = norm
    if clip and clipv > 0:
        l2 = float(torch.sqrt((diff.double() ** 2).sum()))
        if l2 > clipv:
            scale *= clipv / l2
    g = diff * scale
    w = data
    if l1:
        g = g + (wd * decay_mult) * torch.sign(w)
    else:
        g = g + (wd * decay_mult) * w
    rate = lr * lr_mult
    if kind == 0:      # SGD
        hist[0].mul_(mom).add_(rate * g)
        upd = hist[0]
    elif kind == 1:    # Nesterov
        prev = hist[0].clone()
        hist[0].mul_(mom).add_(rate * g)
        upd = (1 + mom) * hist[0] - mom * prev
    elif kind == 2:    # AdaGrad
        hist[0].add_(g * g)
        upd = rate * g / (torch.sqrt(hist[0]) + delta)
    elif kind == 3:    # RMSProp
        hist[0].mul_(rms).add_((1 - rms) * g * g)
        upd = rate * g / (torch.sqrt(hist[0]) + delta)
    elif kind == 4:    # AdaDelta
        hist[0].mul_(mom).add_((1 - mom) * g * g)
        u = g * torch.sqrt((hist[1] + delta) / (hist[0] + delta))
        hist[1].mul_(mom).add_((1 - mom) * u * u)
        upd = rate * u
    elif kind == 5:    # Adam
        hist[0].mul_(mom).add_((1 - mom) * g)
        hist[1].mul_(mom2).add_((1 - mom2) * g * g)
        upd = rate * corr * hist[0] / (torch.sqrt(hist[1]) + delta)
    else:
        raise ValueError(kind)
    diff.copy_(upd)
    data.sub_(upd)
