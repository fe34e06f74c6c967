"""The grouped pointwise kernels (csrc/kernels/conv_gpw.hip) through ``hip.conv_forward`` and
``hip.conv_backward``, held elementwise to the fp64 oracle and the bounds of tests/conv_gpw_cases.py
with a spy on the launches; the isolation of one group from non-finite values in the others; the
channel shuffle against the reshape / transpose."""
import pytest
import torch

import conv_gpw_cases as gc

pytestmark = pytest.mark.gpu


@pytest.fixture
def spy(gpu, monkeypatch):
    """Names of the native launches ops/hip.py makes, in order; the switches at their defaults."""
    from sparknet_amd.ops import _lib, hip
    names = []

    def call(name, *args):
        names.append(name)
        return _lib.call(name, *args)
    monkeypatch.delenv("SN_FEATURES", raising=False)
    monkeypatch.setattr(hip, "call", call)
    return names


@pytest.mark.parametrize("case", gc.CASES, ids=gc.IDS)
def test_forward(case, gpu, spy):
    from sparknet_amd.ops import hip
    i, s = {k: v.to(gpu) for k, v in gc.inputs(case).items()}, gc.spec(case)
    for on in (True, False):  # bias + ReLU, neither
        y = hip.conv_forward(i["x"], i["w"], i["bias"] if on else None, s, relu=on)
        assert tuple(y.shape) == (s.N, s.H, s.W, s.K) and y.dtype == torch.bfloat16
        r = gc.worst(y, *gc.forward_bound(case, on, on))
        print("forward", case, "bias + relu", on, "worst / bound", r)
        assert r <= 1.0, (on, r)
    assert spy == [hip.GPW_FWD] * 2, spy


@pytest.mark.parametrize("case", gc.CASES, ids=gc.IDS)
def test_backward(case, gpu, spy):
    """gate on + store onto 7.0; gate off + accumulate onto 7.0."""
    from sparknet_amd.ops import hip
    i, s = {k: v.to(gpu) for k, v in gc.inputs(case).items()}, gc.spec(case)
    for gate, acc in ((True, False), (False, True)):
        dw = torch.full((s.K, 1, 1, s.Cg), gc.PREFILL, dtype=torch.float32, device=gpu)
        db = torch.full((s.K,), gc.PREFILL, dtype=torch.float32, device=gpu)
        dx = hip.conv_backward(i["dy"], i["x"], i["w"], s, True, dw, db, i["gate"] if gate else None,
                               dw_acc=acc, db_acc=acc)
        assert tuple(dx.shape) == (s.N, s.H, s.W, s.C) and dx.dtype == torch.bfloat16
        bw, bb = gc.wgrad_bound(case, gc.PREFILL if acc else None)
        r = (gc.worst(dx, *gc.dgrad_bound(case, gate)), gc.worst(dw, *bw), gc.worst(db, *bb))
        print("backward", case, "gate", gate, "acc", acc, "worst / bound (dx, dw, db)", r)
        assert max(r) <= 1.0, (gate, acc, r)
    assert [n for n in spy if n.startswith("conv")] == [hip.GPW_WGRAD, hip.GPW_WGRAD_FINALIZE, hip.GPW_DGRAD] * 2, spy


def test_a_group_is_isolated_from_the_others(gpu, spy):
    """Inf in every channel outside group 0 of x (of dy in the data gradient) leaves group 0's
    outputs as they are bit for bit: the neighbouring group's columns are masked when staged."""
    from sparknet_amd.ops import hip
    i, s = {k: v.to(gpu) for k, v in gc.inputs(gc.ISOLATION).items()}, gc.spec(gc.ISOLATION)
    x, dy = i["x"].clone(), i["dy"].clone()
    x[..., s.Cg:] = float("inf")
    dy[..., s.Kg:] = float("inf")
    y0, y1 = (hip.conv_forward(t, i["w"], i["bias"], s, relu=True) for t in (i["x"], x))
    d0, d1 = (hip.conv_backward(t, i["x"], i["w"], s, True, gate=i["gate"]) for t in (i["dy"], dy))
    assert spy == [hip.GPW_FWD] * 2 + [hip.GPW_DGRAD] * 2, spy
    assert torch.equal(y0[..., :s.Kg], y1[..., :s.Kg]) and torch.isfinite(y1[..., :s.Kg]).all()
    assert torch.equal(d0[..., :s.Cg], d1[..., :s.Cg]) and torch.isfinite(d1[..., :s.Cg]).all()


@pytest.mark.parametrize("shape, G", [((2, 3, 5, 24), 3), ((1, 1, 1, 8), 2), ((3, 7, 7, 240), 3), ((2, 4, 4, 12), 3),
                                      ((70, 1, 1, 1000), 8)])  # the last: C % 8 == 0 rows in more than one run
def test_shuffle_channels(shape, G, gpu):
    from sparknet_amd.ops import hip, ref
    x = torch.randn(shape, generator=torch.Generator().manual_seed(G)).to(torch.bfloat16)
    y = hip.shuffle_channels(x.to(gpu), G)
    assert torch.equal(y.cpu(), ref.shuffle_channels(x, G))
    assert torch.equal(y.cpu(), x.reshape(*shape[:3], G, shape[3] // G).transpose(3, 4).reshape(shape))
    assert torch.equal(hip.shuffle_channels(y, shape[3] // G).cpu(), x)  # the backward pass undoes it
