"""Device-dispatching op layer.

Every op has two implementations with identical semantics:

* :mod:`.hip` — hand-written HIP/CDNA4 kernels from ``libsn_kernels.so`` (used for every
  tensor on a ROCm device; there is NO silent PyTorch fallback on the GPU — if the
  native library is missing the call raises);
* :mod:`.ref` — PyTorch fp32 reference (CPU tensors; also the test oracle).
"""
from __future__ import annotations

import contextlib
import threading

import torch

from . import ref
from .spec import POOL_AVE, POOL_MAX, POOL_STOCHASTIC, ConvNdSpec, ConvSpec, PoolSpec  # noqa: F401

_hip = None
_state = threading.local()


def _hipmod():
    global _hip
    if _hip is None:
        from . import hip as _h
        _hip = _h
    return _hip


def f32_active() -> bool:
    """Inside ``precision(torch.float32)``: GPU tensors take the fp32 device path."""
    return getattr(_state, "f32", False)


@contextlib.contextmanager
def precision(dtype):
    """Net forward / backward of a ``dtype`` net: fp32 nets on the GPU route every op to
    :mod:`.f32dev` (fp32 MFMA products + the reference formulas), bf16 nets to :mod:`.hip`."""
    prev = f32_active()
    _state.f32 = dtype == torch.float32
    try:
        yield
    finally:
        _state.f32 = prev


def _gpu(t: torch.Tensor) -> bool:
    """The bf16 HIP engine serves this tensor (a GPU tensor outside the fp32 device mode)."""
    return t.is_cuda and not f32_active()


def _impl(t: torch.Tensor):
    if not t.is_cuda:
        return ref
    if f32_active():
        from . import f32dev
        return f32dev
    return _hipmod()


def _dispatch(name):
    def fn(first, *args, **kwargs):
        return getattr(_impl(first), name)(first, *args, **kwargs)
    fn.__name__ = name
    return fn


conv_forward = _dispatch("conv_forward")
conv_backward = _dispatch("conv_backward")
conv_nd_forward = _dispatch("conv_nd_forward")
conv_nd_backward = _dispatch("conv_nd_backward")
linear_forward = _dispatch("linear_forward")
linear_backward = _dispatch("linear_backward")
pool_forward = _dispatch("pool_forward")
lrn_forward = _dispatch("lrn_forward")
lrn_backward = _dispatch("lrn_backward")
relu_forward = _dispatch("relu_forward")
relu_backward = _dispatch("relu_backward")
shuffle_channels = _dispatch("shuffle_channels")
softmax_forward = _dispatch("softmax_forward")
softmax_backward = _dispatch("softmax_backward")
accuracy = _dispatch("accuracy")


def deconv_dw_forward(x, w, bias, s):
    """Depthwise Deconvolution forward with the bias inside (``s``: the convolution top -> bottom).  bf16
    GPU tensors run conv_updw_fwd; the CPU and the fp32 device mode keep the data-gradient route."""
    if _gpu(x):
        return _hipmod().deconv_dw_forward(x, w, bias, s)
    zeros = torch.zeros((s.N, s.H, s.W, s.C), dtype=x.dtype, device=x.device)
    y = conv_backward(x, zeros, w, s, True, None, None)
    return y if bias is None else (y.float() + bias.float()).to(y.dtype)


def deconv_dw_backward(dy, x, w, s, need_dx, dw=None, db=None, dw_acc=True, db_acc=True):
    """Backward of deconv_dw_forward: dw, db (stored or accumulated) and the bottom gradient or None."""
    if _gpu(dy):
        return _hipmod().deconv_dw_backward(dy, x, w, s, need_dx, dw, db, dw_acc, db_acc)
    if db is not None:
        g = dy.float().reshape(-1, s.C).sum(0)
        db.copy_(db + g if db_acc else g)
    if dw is not None:
        conv_backward(x, dy, w, s, False, dw, None, dw_acc=dw_acc)
    return conv_forward(dy, w, None, s) if need_dx else None


def crop_window(x, offsets, shape):
    """Crop forward on the stored layout: ``x[o0:o0 + s0, o1:o1 + s1, ...]`` (crop_k for 4-D bf16 GPU blobs)."""
    if _gpu(x) and x.dim() == 4 and x.dtype == torch.bfloat16:
        return _hipmod().crop_window(x, offsets, shape)
    return ref.crop_window(x, offsets, shape)


def crop_window_backward(dy, offsets, shape):
    """Gradient of crop_window for a source of ``shape``: dy inside the window, zero outside."""
    if _gpu(dy) and dy.dim() == 4 and dy.dtype == torch.bfloat16:
        return _hipmod().crop_window_backward(dy, offsets, shape)
    return ref.crop_window_backward(dy, offsets, shape)


def _roi_hip(x, rois) -> bool:
    """The ROI kernels (csrc/kernels/roi.hip) serve these tensors; otherwise ops.ref, which reads the ROIs on
    the host (the CPU, the fp32 device mode, other dtypes, SN_FEATURES=roi_kernels=0)."""
    return _gpu(x) and _hipmod().roi_ok(x, rois)


def roi_pool_forward(x, rois, ph, pw, scale):
    """ROIPooling forward on the stored layout: (y [R, PH, PW, C], int32 argmax)."""
    return (_hipmod() if _roi_hip(x, rois) else ref).roi_pool_forward(x, rois, ph, pw, scale)


def roi_pool_backward(dy, rois, argmax, x_shape, ph, pw, scale):
    impl = _hipmod() if _roi_hip(dy, rois) else ref
    return impl.roi_pool_backward(dy, rois, argmax, x_shape, ph, pw, scale)


def roi_align_forward(x, rois, ph, pw, scale, sampling_ratio=0):
    return (_hipmod() if _roi_hip(x, rois) else ref).roi_align_forward(x, rois, ph, pw, scale, sampling_ratio)


def roi_align_backward(dy, rois, x_shape, ph, pw, scale, sampling_ratio=0):
    impl = _hipmod() if _roi_hip(dy, rois) else ref
    return impl.roi_align_backward(dy, rois, x_shape, ph, pw, scale, sampling_ratio)


def smooth_l1_forward(pred, target, in_w=None, out_w=None, sigma=1.0):
    """SmoothL1Loss as a 0-d fp32 tensor (smooth_l1_fwd for GPU tensors outside the fp32 device mode)."""
    return (_hipmod() if _gpu(pred) else ref).smooth_l1_forward(pred, target, in_w, out_w, sigma)


def smooth_l1_backward(pred, target, in_w, out_w, sigma, loss_weight, need_target=False):
    impl = _hipmod() if _gpu(pred) else ref
    return impl.smooth_l1_backward(pred, target, in_w, out_w, sigma, loss_weight, need_target)


def proposal(scores, deltas, im_info, anchors, feat_stride, min_size, pre_nms_topn, post_nms_topn, nms_thresh):
    """The RPN's proposal layer on the stored layout: (rois [N post, 5], scores [N post, 1], count [N]).  The
    kernels of csrc/kernels/proposal.hip where hip.proposal_ok accepts the operands; otherwise ops.ref, which
    reads the boxes on the host (the CPU, the fp32 device mode, other dtypes, larger problems,
    SN_FEATURES=proposal_kernels=0)."""
    use = _gpu(scores) and _hipmod().proposal_ok(scores, deltas, im_info, pre_nms_topn, post_nms_topn, nms_thresh)
    return (_hipmod() if use else ref).proposal(scores, deltas, im_info, anchors, feat_stride, min_size,
                                                pre_nms_topn, post_nms_topn, nms_thresh)


def _lstm_hip(x2, cont, w_hc) -> bool:
    """The step kernels (csrc/kernels/lstm.hip) serve these operands; otherwise ops.ref's fp32 loop over t (the
    CPU, the fp32 device mode, H not a multiple of 8, SN_FEATURES=lstm_kernels=0)."""
    return _gpu(x2) and _hipmod().lstm_ok(x2, cont, w_hc)


def lstm_forward(x2, cont, w_xc, b_c, w_hc, h0, c0, xs=None, w_xs=None, train=True):
    """The LSTM layer's forward over all T steps: (h [T, N, H], saved); h0 / c0 are replaced by h_T / c_T."""
    impl = _hipmod() if _lstm_hip(x2, cont, w_hc) else ref
    return impl.lstm_forward(x2, cont, w_xc, b_c, w_hc, h0, c0, xs, w_xs, train)


def lstm_backward(dh, x2, cont, w_xc, w_hc, saved, need_dx, dw_xc=None, db=None, dw_hc=None, xs=None, w_xs=None,
                  dw_xs=None, need_dxs=False, acc=(True, True, True, True)):
    """Backward of lstm_forward by the route that ran it (only ops.ref saves the cont_t h_{t-1} rows in fp32; the
    kernels save them in bf16, or not at all after a forward with train=False, which hip.lstm_backward refuses)."""
    impl = ref if saved[2] is not None and saved[2].dtype == torch.float32 else _hipmod()
    return impl.lstm_backward(dh, x2, cont, w_xc, w_hc, saved, need_dx, dw_xc, db, dw_hc, xs, w_xs, dw_xs, need_dxs,
                              acc)


def pool_backward(dy, x, s, aux=None, y=None, gate=False):
    """gate=True: x is a slope-0 in-place ReLU output whose backward is fused here (MAX
    pooling on the GPU encodes it in the forward's argmax mask)."""
    if _gpu(dy):
        return _hipmod().pool_backward(dy, x, s, aux, y, gate)
    if dy.is_cuda:  # fp32 device mode
        from . import f32dev
        return f32dev.pool_backward(dy, x, s, aux, y, gate)
    return ref.pool_backward(dy, x, s, gate)


def pool_forward_aux(x, s, gate=False):
    """Forward returning (y, aux) where aux is the GPU argmax mask (None on CPU)."""
    if _gpu(x):
        return _hipmod().pool_forward_mask(x, s, gate)
    if x.is_cuda:  # fp32 device mode
        from . import f32dev
        return f32dev.pool_forward_aux(x, s, gate)
    return ref.pool_forward(x, s), None


def dropout_forward(x, ratio, rng_state, stream):
    if _gpu(x):
        return _hipmod().dropout_forward(x, ratio, rng_state, stream)
    if x.is_cuda:
        from . import f32dev
        return f32dev.dropout_forward(x, ratio, rng_state, stream)
    seed, counter = (int(v) for v in rng_state.tolist())
    return ref.dropout_forward(x, ratio, seed, counter, stream)


def dropout_backward(dy, ratio, rng_state, stream, gate=None):
    if _gpu(dy):
        return _hipmod().dropout_backward(dy, ratio, rng_state, stream, gate)
    if dy.is_cuda:
        from . import f32dev
        return f32dev.dropout_backward(dy, ratio, rng_state, stream, gate)
    seed, counter = (int(v) for v in rng_state.tolist())
    return ref.dropout_backward(dy, ratio, seed, counter, stream, gate)


def softmax_loss_forward(x2, labels, ignore_label=None, normalize=True, outer_num=None):
    return _impl(x2).softmax_loss_forward(x2, labels, ignore_label, normalize, outer_num)


def softmax_loss_backward(prob, labels, loss_weight, norm, ignore_label=None, dtype=torch.float32):
    return _impl(prob).softmax_loss_backward(prob, labels, loss_weight, norm, ignore_label, dtype)


def sum_bf16(tensors):
    """Elementwise sum of same-shape bf16 device tensors (fp32 accumulation)."""
    return _hipmod().sum_bf16([t.contiguous() for t in tensors])


def cast_f32_to_bf16(src: torch.Tensor, dst: torch.Tensor) -> None:
    if src.is_cuda:
        _hipmod().cast_f32_to_bf16(src, dst)
    else:
        dst.copy_(src)


def advance_rng(rng_state: torch.Tensor) -> None:
    """Bump the Philox counter once per iteration (device-side, graph-capturable)."""
    if rng_state.is_cuda:
        _hipmod().advance_rng(rng_state)
    else:
        rng_state[1] += 1


def solver_tables(segments, total: int, device, slab_chunks=None) -> dict:
    """Per-element multipliers (CPU reference) or the chunk table of the fused HIP update
    (``slab_chunks``: gradients read from split-K slabs, GPU only)."""
    device = torch.device(device)
    if device.type == "cuda":
        return _hipmod().solver_tables(segments, total, device, slab_chunks)
    assert not slab_chunks
    lr = torch.zeros(max(total, 1))
    dc = torch.zeros(max(total, 1))
    for off, cnt, lm, dm in segments:
        lr[off:off + cnt] = lm
        dc[off:off + cnt] = dm
    return {"lr": lr, "decay": dc}


def solver_update(kind, data, diff, history, compute, tables, hyper, l1: bool, clip: bool,
                  grid_limit: int = 0) -> None:
    if data.is_cuda:
        _hipmod().solver_update(kind, data, diff, history, compute, tables, hyper, l1, clip, grid_limit)
        return
    h = hyper.tolist()
    ref.solver_update_ref(kind, data, diff, history, tables["lr"], tables["decay"], h, l1, clip)
    if compute is not None and compute is not data:
        compute.copy_(data)
