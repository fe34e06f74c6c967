"""The pooling and LRN kernels (csrc/kernels/pool.hip, lrn.hip, pool_lrn.hip) through ops.hip, held
elementwise to the fp64 oracles and the derived bounds of tests/pool_lrn_cases.py on every case:
values, the argmax mask itself and the gradients; which launches are made (a spy on the native
call); the fused pool / LRN kernels bitwise against the unfused chain, each stage of which meets
the oracle on the inputs it actually received; and the image-chunked launches against one launch.
Every check prints its worst / bound ratio."""
import pytest
import torch

import pool_lrn_cases as pc
from sparknet_amd.ops.spec import POOL_MAX

pytestmark = pytest.mark.gpu


@pytest.fixture
def spy(gpu, monkeypatch):
    """Names of the native launches ops/hip.py makes, in order."""
    from sparknet_amd.ops import _lib, hip
    names = []

    def call(name, *args):
        names.append(name)
        return _lib.call(name, *args)
    monkeypatch.setattr(hip, "call", call)
    return names


def _held(what, got, ref, bound):
    r = pc.worst(got, ref, bound)
    print(what, "worst / bound", r)
    assert r <= 1.0, (what, r)


def _same(what, got, ref):
    r = pc.exact(got, ref)
    print(what, "worst / bound", r)
    assert r == 0.0, what


@pytest.mark.parametrize("method", pc.METHODS, ids=["max", "ave"])
@pytest.mark.parametrize("case", pc.POOL_CASES, ids=pc.POOL_IDS)
def test_pool(case, method, gpu, spy):
    from sparknet_amd.ops import hip
    s = pc.pool_spec(case, method)
    runs = pc.pool_runs()
    for variant, gate in runs:
        i = {k: v.to(gpu) for k, v in pc.pool_inputs(case, variant).items()}
        tag = f"pool {case} {'max' if method == POOL_MAX else 'ave'} {variant} gate {gate}:"
        y, mask = hip.pool_forward_mask(i["x"], s, gate)
        assert tuple(y.shape) == (s.N, s.P, s.Q, s.C) and y.dtype == torch.bfloat16
        yr, yb, mr = pc.pool_forward_bound(case, method, variant, gate)
        _held(tag + " y", y, yr, yb)
        if method == POOL_MAX:
            assert mask.dtype == torch.uint8 and tuple(mask.shape) == tuple(y.shape)
            _same(tag + " mask", mask, mr)
        else:
            assert mask is None
        ref, bound = pc.pool_backward_bound(case, method, variant, gate)
        for m in (mask, None):  # the forward's mask, and the mask recomputed from x
            dx = hip.pool_backward(i["dy"], i["x"], s, m, gate=gate)
            assert tuple(dx.shape) == (s.N, s.H, s.W, s.C) and dx.dtype == torch.bfloat16
            _held(tag + f" dx ({'mask' if m is not None else 'mask=None'})", dx, ref, bound)
    assert spy.count("pool_fwd") == len(runs) * (2 if method == POOL_MAX else 1), spy
    assert spy.count("pool_bwd") == 2 * len(runs), spy


@pytest.mark.parametrize("case", pc.LRN_CASES, ids=pc.LRN_IDS)
def test_lrn(case, gpu, spy):
    from sparknet_amd.ops import hip
    i, h = {k: v.to(gpu) for k, v in pc.lrn_inputs(case).items()}, pc.hyper(case)
    kind = "within-channel" if h.within else "cross-channel"
    y = hip.lrn_forward(i["x"], h.size, h.alpha, h.beta, h.k, h.within)
    assert y.shape == i["x"].shape and y.dtype == torch.bfloat16
    _held(f"lrn {kind} {case}: y", y, *pc.lrn_forward_bound(case))
    for gate in (False, True):
        dx = hip.lrn_backward(i["dy"], i["x"], h.size, h.alpha, h.beta, h.k, h.within, gate=gate)
        assert dx.shape == i["x"].shape and dx.dtype == torch.bfloat16
        _held(f"lrn {kind} {case} gate {gate}: dx", dx, *pc.lrn_backward_bound(case, gate))
    name = "lrn_within" if h.within else "lrn_across"
    assert spy.count(name + "_fwd") == 1 and spy.count(name + "_bwd") == 2, spy


def _fused_setup(case, gate, gpu):
    i = {k: v.to(gpu) for k, v in pc.fused_inputs(case).items()}
    i["x"] = pc.fused_x(case, gate).to(gpu)
    return i, pc.fused_spec(case), pc.fused_hyper(case)


def _scale_in_range(x, h):
    lo, hi = pc.scale_range(x.cpu(), h)
    assert h.k <= lo and hi <= 8 * h.k, (lo, hi)


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("case", pc.FUSED_CASES, ids=pc.FUSED_IDS)
def test_fused_pool_then_lrn(case, gate, gpu, spy):
    """pool_lrn_fwd and lrn_pool_bwd are bitwise the unfused launches, and those meet the oracle."""
    from sparknet_amd.ops import hip
    i, s, h = _fused_setup(case, gate, gpu)
    hy = (h.size, h.alpha, h.beta, h.k)
    assert hip.pool_lrn_eligible(s, h.size, False)
    pooled, mask, y = hip.pool_lrn_forward(i["x"], s, gate, *hy)
    p_ref, m_ref = hip.pool_forward_mask(i["x"], s, gate)
    y_ref = hip.lrn_forward(p_ref, *hy)
    assert torch.equal(pooled, p_ref) and torch.equal(mask, m_ref) and torch.equal(y, y_ref)
    dx = hip.lrn_pool_backward(i["dy"], pooled, mask, s, *hy)
    dp = hip.lrn_backward(i["dy"], p_ref, *hy)
    dx_ref = hip.pool_backward(dp, i["x"], s, m_ref, gate=gate)
    assert torch.equal(dx, dx_ref)
    assert spy == ["pool_lrn_fwd", "pool_fwd", "lrn_across_fwd", "lrn_pool_bwd", "lrn_across_bwd", "pool_bwd"], spy
    tag = f"pool -> lrn {case} gate {gate}:"
    xc, pooled_c, dpc = i["x"].cpu(), p_ref.cpu(), dp.cpu()
    _scale_in_range(pooled_c, h)
    pr, pb, mr = pc.pool_forward_bound_of(xc, s, gate)
    _held(tag + " pooled", p_ref, pr, pb)
    _same(tag + " mask", m_ref, mr)
    _held(tag + " y", y_ref, *pc.lrn_forward_bound_of(pooled_c, h))
    _held(tag + " dp", dp, *pc.lrn_backward_bound_of(i["dy"].cpu(), pooled_c, h))
    _held(tag + " dx", dx_ref, *pc.pool_backward_bound_of(dpc, xc, s, gate))


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("case", pc.FUSED_CASES, ids=pc.FUSED_IDS)
def test_fused_lrn_then_pool_backward(case, gate, gpu, spy):
    """pool_lrn_bwd_rev is bitwise pool_bwd_k3s2 then lrn_across_bwd, and those meet the oracle."""
    from sparknet_amd.ops import hip
    i, s, h = _fused_setup(case, gate, gpu)
    hy = (h.size, h.alpha, h.beta, h.k)
    assert hip.pool_lrn_rev_eligible(s, h.size, False)
    y = hip.lrn_forward(i["x"], *hy)
    _, mask = hip.pool_forward_mask(y, s, False)
    dl = hip.pool_backward(i["dy"], y, s, mask)
    dx_ref = hip.lrn_backward(dl, i["x"], *hy, gate=gate)
    dx = hip.pool_lrn_backward_rev(i["dy"], mask, i["x"], s, *hy, gate)
    assert torch.equal(dx, dx_ref)
    assert spy == ["lrn_across_fwd", "pool_fwd", "pool_bwd", "lrn_across_bwd", "pool_lrn_bwd_rev"], spy
    tag = f"lrn -> pool {case} gate {gate}:"
    xc, yc, dlc = i["x"].cpu(), y.cpu(), dl.cpu()
    _scale_in_range(xc, h)
    _held(tag + " y", y, *pc.lrn_forward_bound_of(xc, h))
    _same(tag + " mask", mask, pc.max_forward64(yc, s, False)[1])
    _held(tag + " dl", dl, *pc.pool_backward_bound_of(i["dy"].cpu(), yc, s, False))
    _held(tag + " dx", dx_ref, *pc.lrn_backward_bound_of(dlc, xc, h, gate))


def _side(shape, gpu):
    """An initialised delayed-scaling slot and an fp8 side output over a fresh tensor of `shape`."""
    from sparknet_amd.ops import gemm as G, hip
    sc = hip.Fp8Scales(1, gpu)
    sc.slots[0, 0], sc.slots[0, 2], sc.slots[0, 3] = 37.0, 1 / 37.0, 1.0
    return sc, G.Fp8Side(torch.empty(shape, dtype=torch.bfloat16, device=gpu), sc.slot(0), False)


@pytest.mark.parametrize("method", pc.METHODS, ids=["max", "ave"])
@pytest.mark.parametrize("case", pc.CHUNK_CASES, ids=pc.CHUNK_IDS)
def test_image_chunked_launches_equal_one_launch(case, method, gpu, spy, monkeypatch):
    """N = 5 as 2 + 2 + 1 images: values, mask, gradients, and (where the kernels have one) the fp8
    side bytes and the folded amax are those of the single launch."""
    from sparknet_amd.ops import hip
    s = pc.pool_spec(case, method)
    gate = method == POOL_MAX
    i = {k: v.to(gpu) for k, v in pc.pool_inputs(case, "relu").items()}

    def run():
        out = {}
        out["y"], out["mask"] = hip.pool_forward_mask(i["x"], s, gate)
        out["dx"] = hip.pool_backward(i["dy"], i["x"], s, out["mask"], gate=gate)
        if hip.pool_side_ok(s, False):
            sc, side = _side((s.N, s.P, s.Q, s.C), gpu)
            y, mask = hip.pool_forward_mask(i["x"], s, gate, side=side)
            assert torch.equal(y, out["y"]) and torch.equal(mask, out["mask"])
            out["fwd q"], out["fwd amax"] = side.q, sc.slots[0, 1].clone()
            assert float(out["fwd amax"]) == float(y.float().abs().max()) > 0
        if hip.pool_side_ok(s, True):
            sc, side = _side((s.N, s.H, s.W, s.C), gpu)
            dx = hip.pool_backward(i["dy"], i["x"], s, out["mask"], gate=gate, side=side)
            assert torch.equal(dx, out["dx"])
            out["bwd q"], out["bwd amax"] = side.q, sc.slots[0, 1].clone()
            assert float(out["bwd amax"]) == float(dx.float().abs().max()) > 0
        return out

    whole = run()
    launches = spy.count("pool_fwd") + spy.count("pool_bwd")
    del spy[:]
    monkeypatch.setattr(hip, "_MAX_ELEMS", pc.chunk_limit(case))
    assert hip._pool_images(s) == 2
    chunked = run()
    assert spy.count("pool_fwd") + spy.count("pool_bwd") == 3 * launches, spy
    assert set(chunked) == set(whole)
    for k, v in whole.items():
        assert (chunked[k] is None and v is None) or torch.equal(chunked[k], v), k
    # and the single launch meets the oracle
    yr, yb, mr = pc.pool_forward_bound_of(i["x"].cpu(), s, gate)
    _held(f"chunk {case} y", whole["y"], yr, yb)
    if mr is not None:
        _same(f"chunk {case} mask", whole["mask"], mr)
    _held(f"chunk {case} dx", whole["dx"], *pc.pool_backward_bound_of(i["dy"].cpu(), i["x"].cpu(), s, gate))
