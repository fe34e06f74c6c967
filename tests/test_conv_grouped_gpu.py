"""The narrow-group 3x3 kernels (csrc/kernels/conv_grouped.hip) through ``hip.conv_forward`` and
``hip.conv_backward``, held elementwise to the fp64 oracle and the derived bounds of
tests/conv_grouped_cases.py on every case; which launches are used (a spy on the native calls and
on the GEMM), the ``conv_grouped=0`` path as the reference point, determinism, and the
fall-backs: a misaligned view, a channel-slice view, C = 24."""
import contextlib
import os

import pytest
import torch

import conv_grouped_cases as gc
from sparknet_amd.ops.spec import ConvSpec

pytestmark = pytest.mark.gpu

NEW = {"conv_grouped_fwd", "conv_grouped_wgrad", "conv_grouped_dgrad"}


@contextlib.contextmanager
def features(value):
    old = os.environ.get("SN_FEATURES")
    if value is None:
        os.environ.pop("SN_FEATURES", None)
    else:
        os.environ["SN_FEATURES"] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SN_FEATURES", None)
        else:
            os.environ["SN_FEATURES"] = old


@pytest.fixture
def spy(gpu, monkeypatch):
    """Names of the native launches made, in order; a GEMM is recorded as "gemm"."""
    from sparknet_amd.ops import _lib, hip
    names = []
    native, gemm = _lib.call, hip.gemm

    def call(name, *args):
        names.append(name)
        return native(name, *args)

    def spied_gemm(*args, **kw):
        names.append("gemm")
        return gemm(*args, **kw)
    monkeypatch.setattr(hip, "call", call)
    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(hip, "gemm", spied_gemm)
    return names


def _dev(case, gpu):
    return {k: v.to(gpu) for k, v in gc.inputs(case).items()}


def _grads(s, gpu, fill=gc.PREFILL):
    return (torch.full((s.K, 3, 3, s.Cg), fill, dtype=torch.float32, device=gpu),
            torch.full((s.K,), fill, dtype=torch.float32, device=gpu))


def _check_forward(case, gpu, hip, c=gc.C_SUM):
    i, s = _dev(case, gpu), gc.spec(case)
    worst = 0.0
    for bias in (True, False):
        for relu in (True, False):
            y = hip.conv_forward(i["x"], i["w"], i["bias"] if bias else None, s, relu=relu)
            assert tuple(y.shape) == (s.N, s.P, s.Q, s.C) and y.dtype == torch.bfloat16
            r = gc.worst(y, *gc.forward_bound(case, bias, relu, c))
            print("forward", case, "bias", bias, "relu", relu, "worst / bound", r)
            worst = max(worst, r)
    return worst


def _check_backward(case, gpu, hip, c=gc.C_SUM):
    """gate on + store onto 7.0; gate off + accumulate onto 7.0; need_dx False with db None;
    dw None with the bias gradient alone.  Returns the worst ratios (dx, dw, db)."""
    i, s = _dev(case, gpu), gc.spec(case)
    worst = [0.0, 0.0, 0.0]
    for gate, acc in ((True, False), (False, True)):
        dw, db = _grads(s, gpu)
        dx = hip.conv_backward(i["dy"], i["x"], i["w"], s, True, dw, db, i["gate"] if gate else None,
                               dw_acc=acc, db_acc=acc)
        assert tuple(dx.shape) == (s.N, s.H, s.W, s.C) and dx.dtype == torch.bfloat16
        bw, bb = gc.wgrad_bound(case, gc.PREFILL if acc else None, c)
        r = (gc.worst(dx, *gc.dgrad_bound(case, gate, c)), gc.worst(dw, *bw), gc.worst(db, *bb))
        print("backward", case, "gate", gate, "acc", acc, "worst / bound (dx, dw, db)", r)
        worst = [max(a, b) for a, b in zip(worst, r)]
    dw, _ = _grads(s, gpu)
    assert hip.conv_backward(i["dy"], i["x"], i["w"], s, False, dw, None, None, dw_acc=False) is None
    worst[1] = max(worst[1], gc.worst(dw, *gc.wgrad_bound(case, None, c)[0]))
    _, db = _grads(s, gpu)
    hip.conv_backward(i["dy"], i["x"], i["w"], s, False, None, db, None, db_acc=False)
    worst[2] = max(worst[2], gc.worst(db, *gc.wgrad_bound(case, None, c)[1]))
    print("backward", case, "worst / bound over the four requests (dx, dw, db)", worst)
    return worst


@pytest.mark.parametrize("case", gc.CASES, ids=gc.IDS)
def test_forward(case, gpu, spy):
    from sparknet_amd.ops import hip
    with features(None):
        assert _check_forward(case, gpu, hip) <= 1.0
    assert spy == ["conv_grouped_fwd"] * 4, spy


@pytest.mark.parametrize("case", gc.CASES, ids=gc.IDS)
def test_backward(case, gpu, spy):
    from sparknet_amd.ops import hip
    with features(None):
        assert max(_check_backward(case, gpu, hip)) <= 1.0
    # the bias gradient stays a column sum
    assert spy == ["colsum_bf16", "conv_grouped_wgrad", "conv_grouped_dgrad"] * 2 + ["conv_grouped_wgrad",
                                                                                   "colsum_bf16"], spy


@pytest.mark.parametrize("case", gc.CASES, ids=gc.IDS)
def test_switch_off_is_the_parent_path_and_meets_the_bounds(case, gpu, spy):
    """SN_FEATURES=conv_grouped=0: the implicit grouped GEMM (Cg = 8, 16; its stride-2 data
    gradient through an fp32 dcol and col2im) or one im2col + GEMM per group (Cg = 4)."""
    from sparknet_amd.ops import hip
    with features("conv_grouped=0"):
        assert _check_forward(case, gpu, hip) <= 1.0
        assert max(_check_backward(case, gpu, hip)) <= 1.0
    assert spy and not NEW & set(spy), sorted(set(spy))
    assert "gemm" in spy and (case[4] != 4 or ("im2col" in spy and "col2im" in spy))


def test_weight_gradient_is_bitwise_reproducible(gpu, spy):
    from sparknet_amd.ops import _lib, hip
    case = gc.LARGEST
    i, s = _dev(case, gpu), gc.spec(case)
    runs = []
    with features(None):
        for _ in range(3):
            dw, _ = _grads(s, gpu)
            hip.conv_backward(i["dy"], i["x"], i["w"], s, False, dw, None, None, dw_acc=False)
            runs.append(dw.clone())
    assert spy == ["conv_grouped_wgrad"] * 3
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    # several slabs of partials went into that sum
    k = _lib.kernels()
    k.sn_conv_grouped_part_floats.restype = _lib.C.c_longlong
    n = int(k.sn_conv_grouped_part_floats(*(_lib.C.c_longlong(v) for v in (s.N, s.P, s.Q, s.C, s.Cg))))
    per = s.K * 9 * s.Cg
    assert n % per == 0 and n // per > 1, n


def _all_products(i, x, s, gpu, hip):
    y = hip.conv_forward(x, i["w"], i["bias"], s, relu=False)
    dw, db = _grads(s, gpu)
    dx = hip.conv_backward(i["dy"], x, i["w"], s, True, dw, db, i["gate"], dw_acc=False, db_acc=False)
    return y, dx, dw, db


def _ratios(case, y, dx, dw, db):
    bw, bb = gc.wgrad_bound(case)
    return (gc.worst(y, *gc.forward_bound(case, True, False)), gc.worst(dx, *gc.dgrad_bound(case, True)),
            gc.worst(dw, *bw), gc.worst(db, *bb))


def test_misaligned_view_falls_back_and_is_correct(gpu, spy):
    """A contiguous view at a storage offset of 2 elements starts 4 bytes into a 16-byte lane."""
    from sparknet_amd.ops import hip
    case = gc.CASES[2]  # Cg = 4: the per-group path takes any alignment
    i, s = _dev(case, gpu), gc.spec(case)
    buf = torch.zeros(i["x"].numel() + 8, dtype=torch.bfloat16, device=gpu)
    assert buf.data_ptr() % 16 == 0
    x = buf[2:2 + i["x"].numel()].view(i["x"].shape)
    x.copy_(i["x"])
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    with features(None):
        out = _all_products(i, x, s, gpu, hip)
    assert "conv_grouped_fwd" not in spy and "conv_grouped_wgrad" not in spy, spy
    assert spy.count("conv_grouped_dgrad") == 1  # dy, w, gate and dx are aligned
    r = _ratios(case, *out)
    print("misaligned: worst / bound (y, dx, dw, db)", r)
    assert max(r) <= 1.0, r


def test_channel_slice_view_falls_back_and_is_correct(gpu, spy):
    """x as channels [16, 32) of a 48-channel tensor: made dense for a grouped layer; a sliced
    dx_out is written by the path that can write it in place (stride 1) and equals the dense one."""
    from sparknet_amd.ops import hip
    case = gc.CASES[4]
    i, s = _dev(case, gpu), gc.spec(case)
    wide = torch.zeros((s.N, s.H, s.W, 48), dtype=torch.bfloat16, device=gpu)
    x = wide[..., 16:32]
    x.copy_(i["x"])
    dx_wide, gate = torch.zeros_like(wide), torch.zeros_like(wide)[..., 16:32]  # the gate shares dx's layout
    gate.copy_(i["gate"])
    with features(None):
        y = hip.conv_forward(x, i["w"], i["bias"], s, relu=False)
        dw, db = _grads(s, gpu)
        dx = hip.conv_backward(i["dy"], x, i["w"], s, True, dw, db, gate, dw_acc=False, db_acc=False,
                               dx_out=dx_wide[..., 16:32])
    assert "conv_grouped_dgrad" not in spy, spy
    assert dx.data_ptr() == dx_wide[..., 16:32].data_ptr()
    assert float(dx_wide[..., :16].abs().max()) == 0.0 and float(dx_wide[..., 32:].abs().max()) == 0.0
    r = _ratios(case, y, dx, dw, db)
    print("channel slice: worst / bound (y, dx, dw, db)", r)
    assert max(r) <= 1.0, r


def test_c24_falls_back_and_is_correct(gpu, spy):
    """C = 24 with Cg = 4 is not whole bundles: the per-group path, against torch in fp64."""
    import torch.nn.functional as F
    from sparknet_amd.ops import hip
    s = ConvSpec(2, 6, 6, 24, 24, 3, 3, 1, 1, 1, 1, 1, 1, 6)
    g = torch.Generator().manual_seed(24)
    x = torch.randn(2, 6, 6, 24, generator=g).to(torch.bfloat16)
    w = (0.2 * torch.randn(24, 3, 3, 4, generator=g)).to(torch.bfloat16)
    with features(None):
        y = hip.conv_forward(x.to(gpu), w.to(gpu), None, s, relu=False)
    assert spy and not NEW & set(spy), spy
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), padding=1, groups=6)
    A = F.conv2d(x.double().abs().permute(0, 3, 1, 2), w.double().abs().permute(0, 3, 1, 2), padding=1, groups=6)
    ref, A = ref.permute(0, 2, 3, 1), A.permute(0, 2, 3, 1)
    assert gc.worst(y, ref, gc.U16 * ref.abs() + gc.C_SUM * 37 * gc.U32 * A) <= 1.0
