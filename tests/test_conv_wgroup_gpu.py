"""The 32-wide grouped 3x3 kernels (csrc/kernels/conv_wgroup.hip) through ``hip.conv_forward`` and
``hip.conv_backward``, held elementwise to the fp64 oracle and the derived bounds of
tests/conv_grouped_cases.py on the cases of tests/conv_wgroup_cases.py; which launches are used,
the ``conv_wgroup=0`` path under the same bounds, reproducibility, and the fall-backs.  The request
mixes, the spy and the helpers are those of tests/test_conv_grouped_gpu.py."""
import pytest
import torch

import conv_grouped_cases as gc
import conv_wgroup_cases as wc
import test_conv_grouped_gpu as tg
from test_conv_grouped_gpu import spy  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

FWD, WGRAD, DGRAD = "conv_wgroup_fwd", "conv_wgroup_wgrad", "conv_wgroup_dgrad"
cases = pytest.mark.parametrize("case", wc.CASES, ids=wc.IDS)


@cases
def test_forward(case, gpu, spy):
    from sparknet_amd.ops import hip
    with tg.features(None):
        assert tg._check_forward(case, gpu, hip) <= 1.0
    assert spy == [FWD] * 4, spy


@cases
def test_backward(case, gpu, spy):
    from sparknet_amd.ops import hip
    with tg.features(None):
        assert max(tg._check_backward(case, gpu, hip)) <= 1.0
    assert spy == ["colsum_bf16", WGRAD, DGRAD] * 2 + [WGRAD, "colsum_bf16"], spy


@cases
def test_switch_off_is_the_parent_path_and_meets_the_bounds(case, gpu, spy):
    from sparknet_amd.ops import hip
    with tg.features("conv_wgroup=0"):
        assert tg._check_forward(case, gpu, hip) <= 1.0
        assert max(tg._check_backward(case, gpu, hip)) <= 1.0
    assert "gemm" in spy and not {FWD, WGRAD, DGRAD} & set(spy), sorted(set(spy))


def test_weight_gradient_is_bitwise_reproducible(gpu, spy):
    from sparknet_amd.ops import hip
    i, s = tg._dev(wc.LARGEST, gpu), gc.spec(wc.LARGEST)
    runs = []
    with tg.features(None):
        for _ in range(3):
            dw, _ = tg._grads(s, gpu)
            hip.conv_backward(i["dy"], i["x"], i["w"], s, False, dw, None, None, dw_acc=False)
            runs.append(dw.clone())
    assert spy == [WGRAD] * 3
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    n, per = hip._wgroup_part(s, gpu)[1], s.K * 9 * 32
    assert n % per == 0 and n // per > 1, n  # several slabs of partials went into that sum


def test_misaligned_view_falls_back_and_is_correct(gpu, spy):
    """A contiguous dy at a storage offset of 2 elements starts 4 bytes into a 16-byte lane.  At Cg = 32
    the implicit GEMM needs aligned activations as well, so the product that can fall back is the
    stride-2 data gradient: its generic route copies dy group by group."""
    from sparknet_amd.ops import hip
    case = wc.CASES[3]
    i, s = tg._dev(case, gpu), gc.spec(case)
    buf = torch.zeros(i["dy"].numel() + 8, dtype=torch.bfloat16, device=gpu)
    dy = buf[2:2 + i["dy"].numel()].view(i["dy"].shape)
    dy.copy_(i["dy"])
    assert dy.is_contiguous() and dy.data_ptr() % 16 == 4
    with tg.features(None):
        dx = hip.conv_backward(dy, i["x"], i["w"], s, True, None, None, i["gate"])
    assert DGRAD not in spy and "col2im" in spy, spy
    assert gc.worst(dx, *gc.dgrad_bound(case, True)) <= 1.0


def test_channel_slice_dx_out_falls_back_and_is_correct(gpu, spy):
    """dx_out as channels [32, 96) of a 128-channel tensor is written in place by the implicit GEMM."""
    from sparknet_amd.ops import hip
    case = wc.CASES[2]
    i, s = tg._dev(case, gpu), gc.spec(case)
    dx_wide, gate = (torch.zeros((s.N, s.H, s.W, 128), dtype=torch.bfloat16, device=gpu) for _ in range(2))
    gate = gate[..., 32:96]
    gate.copy_(i["gate"])
    with tg.features(None):
        y = hip.conv_forward(i["x"], i["w"], i["bias"], s, relu=False)
        dw, db = tg._grads(s, gpu)
        dx = hip.conv_backward(i["dy"], i["x"], i["w"], s, True, dw, db, gate, dw_acc=False, db_acc=False,
                               dx_out=dx_wide[..., 32:96])
    assert DGRAD not in spy and FWD in spy and WGRAD in spy, spy
    assert dx.data_ptr() == dx_wide[..., 32:96].data_ptr()
    assert float(dx_wide[..., :32].abs().max()) == 0.0 and float(dx_wide[..., 96:].abs().max()) == 0.0
    assert max(tg._ratios(case, y, dx, dw, db)) <= 1.0
