"""The fused HIP solver update (csrc/kernels/solver.hip: solver_update_kernel, chunk_grad,
sumsq_pass1/2, scale_shadow) against the fp64 oracle of tests/solver_update_cases.py, at its
edges: every (kind, L1, CLIP, SHADOW) instance, segments of 1 .. 20000 parameters (several
chunks, a short last chunk), all lr_mult / decay_mult values, +-0 weights under L1, clips that
bite and clips that do not, the grid-stride loop over the chunk table, gradients summed from
split-K slabs on every path of chunk_grad, and scale_shadow on its vector, tail and scalar
paths.  Bounds are derived in the cases module; tests/test_solver_update.py shows on the CPU
that a correct fp32 update uses under a quarter of them and that an update with any one
ingredient wrong misses them by a factor of 500 on a fifth of the elements.
"""
import ctypes as C

import pytest
import torch

import solver_update_cases as sc
from test_solver_update import VARIANTS, variant_id

pytestmark = pytest.mark.gpu

DEV = "cuda"
INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def _hip():
    from sparknet_amd.ops import hip
    return hip


def _bits(t):
    return t.contiguous().view(INT[t.dtype])


def _same_bits(a, b, mask=None):
    a, b = _bits(a), _bits(b)
    return torch.equal(a, b) if mask is None else torch.equal(a[mask], b[mask])


def _run(c, hyper, l1, clip, shadow=True, grid_limit=0, tabs=None, g=None):
    """One update of clones of the case's inputs on the device -> outputs on the CPU."""
    hip = _hip()
    w, h0, h1 = (t.clone().to(DEV) for t in (c.w, c.h0, c.h1))
    g = c.g.clone().to(DEV) if g is None else g
    g_before = g.clone()
    sh = torch.full((c.total,), sc.SENTINEL, dtype=torch.bfloat16, device=DEV) if shadow else None
    tabs = hip.solver_tables(c.segs, c.total, DEV) if tabs is None else tabs
    hip.solver_update(c.kind, w, g, [h0, h1], sh, tabs, hyper.clone().to(DEV), l1, clip, grid_limit)
    torch.cuda.synchronize()
    assert _same_bits(g, g_before), "the update modified the gradient"
    return dict(w=w.cpu(), h0=h0.cpu(), h1=h1.cpu(), shadow=None if sh is None else sh.cpu())


def _check(out, c, refs, bnds, what):
    """Outputs within the bound on the updated range, the shadow the bf16 rounding of the
    stored weight, everything else bitwise as it was."""
    names = ("w", "h0", "h1") if c.kind >= 4 else ("w", "h0")
    for name, r, b in zip(names, refs, bnds):
        err = (out[name].double() - r).abs()[c.upd]
        over = err - b[c.upd]
        print(what, name, "max error", float(err.max()), "max error / bound", float((err / b[c.upd]).max()))
        assert bool((over <= 0).all()), (what, name, "max error", float(err.max()), "worst excess", float(over.max()),
                                         "elements over", int((over > 0).sum()))
    if c.kind < 4:
        assert _same_bits(out["h1"], c.h1), "h1 written by a one-history solver"
    for name, src in (("w", c.w), ("h0", c.h0), ("h1", c.h1)):
        assert _same_bits(out[name], src, c.gap), f"{name}: a gap element was written"
    if out["shadow"] is not None:
        assert _same_bits(out["shadow"], out["w"].to(torch.bfloat16), c.upd), "shadow != bf16(stored weight)"
        assert bool((out["shadow"][c.gap] == sc.SENTINEL).all()), "shadow: a gap element was written"


def _equal_outputs(a, b, mask=None):
    return all((a[k] is None and b[k] is None) or _same_bits(a[k], b[k], mask) for k in ("w", "h0", "h1", "shadow"))


@pytest.mark.parametrize("variant", VARIANTS, ids=variant_id)
@pytest.mark.parametrize("kind", range(6), ids=sc.KINDS)
def test_every_instance_against_fp64(gpu, kind, variant):
    """6 kinds x {L2, L1} x {no clip, clip at half the norm}, plus a clip above the norm and
    clip = -1 through the clipping instance: both must give the unclipped update."""
    l1, clip, mode = variant
    c = sc.case(kind)
    hyper = c.hyper(mode)
    refs, bnds = sc.case_bounds(c, hyper, l1, clip, clipped=mode == "half")
    out = _run(c, hyper, l1, clip)
    _check(out, c, refs, bnds, f"{sc.KINDS[kind]} {variant_id(variant)}")
    if mode in ("above", "negative"):   # the same arithmetic as the instance without clipping
        assert _equal_outputs(out, _run(c, c.hyper("none"), l1, False))


@pytest.mark.parametrize("kind", range(6), ids=sc.KINDS)
def test_without_shadow(gpu, kind):
    """shadow = None (the SHADOW = false instances): same weights and histories, bitwise."""
    c = sc.case(kind)
    l1, clip = bool(kind & 1), kind >= 3
    hyper = c.hyper("half" if clip else "none")
    refs, bnds = sc.case_bounds(c, hyper, l1, clip, clipped=clip)
    out = _run(c, hyper, l1, clip, shadow=False)
    _check(out, c, refs, bnds, f"{sc.KINDS[kind]} no shadow")
    with_shadow = _run(c, hyper, l1, clip)
    assert all(_same_bits(out[k], with_shadow[k]) for k in ("w", "h0", "h1"))


@pytest.mark.parametrize("kind", [1, 5], ids=["Nesterov", "Adam"])
def test_grid_stride_loop_is_bitwise_neutral(gpu, kind):
    """A grid smaller than the chunk table (the overlapped update on a side stream) loops
    over it; a larger limit is ignored."""
    c = sc.case(kind)
    n = c.nchunks()
    assert _hip().solver_tables(c.segs, c.total, DEV)["n"] == n == 11
    hyper = c.hyper("half")
    full = _run(c, hyper, True, True)
    refs, bnds = sc.case_bounds(c, hyper, True, True, clipped=True)
    _check(full, c, refs, bnds, "grid_limit 0")
    for limit in (1, 3, n - 1, n, n + 5):
        assert _equal_outputs(_run(c, hyper, True, True, grid_limit=limit), full), f"grid_limit {limit}"


@pytest.mark.parametrize("kind", [0, 4], ids=["SGD", "AdaDelta"])
def test_clipped_update_is_deterministic(gpu, kind):
    c = sc.case(kind)
    hyper = c.hyper("half")
    assert _equal_outputs(_run(c, hyper, False, True), _run(c, hyper, False, True))


# --------------------------------------------------------------------------------------
# gradients summed from split-K slabs (chunk_grad)
# --------------------------------------------------------------------------------------

def _reduced_flat_gradient(s, ws):
    """The flat gradient the unfused path would have produced: ops/gemm.py's splitk_reduce
    call in mode 1 (fp32 store), the bias (ones) column going to the ``extra`` vector."""
    from sparknet_amd.ops import _lib
    G, M, N, ldw = sc.SLAB_G, sc.SLAB_M, sc.SLAB_N, sc.SLAB_LDW
    g = s.g.clone().to(DEV)
    out, bias_grad = g[sc.SLAB_OFF_W:], g[sc.SLAB_OFF_B:]
    _lib.call("splitk_reduce", ws, s.splits, M * ldw, M, N + 1, ldw, out, N, 1, None, 0,
              G, s.splits * M * ldw, M * N, None, bias_grad, N, 0, M,
              C.c_void_p(0), 0, 0.0, 1.0)
    torch.cuda.synchronize()
    return g


@pytest.mark.parametrize("splits", sc.SPLITS)
def test_slab_gradients(gpu, splits):
    """Serial order below 16 splits (4-at-a-time body and tail), the 16-lane order from 16 on
    (its 64-stride body from 49), each for weight rows (es = 1) and the strided bias column:
    (a) against the oracle fed the fp64 sum of the slabs, (b) bitwise against the update of
    the flat gradient that splitk_reduce_kernel / splitk_reduce_wide write."""
    hip = _hip()
    for kind in (0, 5):
        s = sc.slab_case(kind, splits)
        ws = s.ws.to(DEV)
        ws_before = ws.clone()
        tabs = hip.solver_tables(s.segs, s.total, DEV, s.slab_chunks(ws.data_ptr()))
        assert tabs["src"] is not None and tabs["n"] == sc.SLAB_G * sc.SLAB_M + sc.SLAB_G + 1
        fused = _run(s, s.hyper(), False, False, tabs=tabs)      # flat g holds noise on the slab ranges
        assert torch.equal(ws, ws_before)
        refs, bnds = s.bounds(s.hyper())
        _check(fused, s, refs, bnds, f"slabs {splits} {sc.KINDS[kind]}")
        g = _reduced_flat_gradient(s, ws)
        gc = g.cpu()
        assert bool(((gc.double() - s.g64).abs() <= s.g_abs)[s.slab].all()), "splitk_reduce against the fp64 sum"
        assert _same_bits(gc, s.g, ~s.slab), "splitk_reduce wrote outside the weight and bias gradients"
        flat = _run(s, s.hyper(), False, False, g=g)
        assert _equal_outputs(fused, flat, s.upd), f"summation order differs from the reduce kernel at {splits} splits"


def test_clipping_with_slab_tables_is_refused(gpu):
    """Clipping needs every gradient in the flat buffer: status 9, nothing launched."""
    from sparknet_amd.ops import _lib
    hip = _hip()
    s = sc.slab_case(0, 4)
    ws = s.ws.to(DEV)
    tabs = hip.solver_tables(s.segs, s.total, DEV, s.slab_chunks(ws.data_ptr()))
    w, g, h0, h1 = (t.clone().to(DEV) for t in (s.w, s.g, s.h0, s.h1))
    sh = torch.full((s.total,), sc.SENTINEL, dtype=torch.bfloat16, device=DEV)
    hyper = sc.hyper_vector(1.0).to(DEV)
    with pytest.raises(RuntimeError, match="code 9"):
        _lib.call("solver_update", 0, w, g, h0, h1, sh, tabs["pos"], tabs["mult"], tabs["n"], hyper, 0, 1,
                  tabs["part"], tabs["part"].numel(), tabs["total"], 0, tabs["src"])
    torch.cuda.synchronize()
    assert _same_bits(w.cpu(), s.w) and _same_bits(h0.cpu(), s.h0) and bool((sh == sc.SENTINEL).all())


# --------------------------------------------------------------------------------------
# scale_shadow
# --------------------------------------------------------------------------------------

def _scale_case(vals, scale, w_off, s_off, shadow=True):
    """w (and shadow) are views ``w_off`` (``s_off``) elements into sentinel-filled buffers:
    an offset of one element breaks the 16-byte (8-byte) alignment of the vector path."""
    hip = _hip()
    n = vals.numel()
    wbuf = torch.full((n + 12,), sc.SENTINEL, device=DEV)
    sbuf = torch.full((n + 12,), sc.SENTINEL, dtype=torch.bfloat16, device=DEV)
    wbuf[w_off:w_off + n] = vals.to(DEV)
    w = wbuf[w_off:w_off + n]
    sh = sbuf[s_off:s_off + n] if shadow else None
    assert w.data_ptr() % 16 == 4 * w_off and (sh is None or sh.data_ptr() % 8 == 2 * s_off)
    hip.scale_shadow(w, sh, scale)
    torch.cuda.synchronize()
    want = vals * torch.tensor(scale, dtype=torch.float32)          # the one fp32 product
    wb, sb = wbuf.cpu(), sbuf.cpu()
    what = (n, scale, w_off, s_off, shadow)
    assert _same_bits(wb[w_off:w_off + n], want), what
    outside = torch.ones(n + 12, dtype=torch.bool)
    outside[w_off:w_off + n] = False
    assert bool((wb[outside] == sc.SENTINEL).all()), what
    outside[:] = True
    if shadow:
        assert _same_bits(sb[s_off:s_off + n], want.to(torch.bfloat16)), what
        outside[s_off:s_off + n] = False
    assert bool((sb[outside] == sc.SENTINEL).all()), what


@pytest.mark.parametrize("n", sc.SCALE_NS)
def test_scale_shadow(gpu, n):
    """16-byte body + scalar tail (n % 4 != 0, n < 4), the scalar fallback for a misaligned w
    or shadow, and a null shadow."""
    vals = torch.randn(n, generator=sc._gen("scale", n)) * 3
    for scale in (1.0 / 3.0, 0.125):
        for w_off, s_off in ((0, 0), (1, 1), (0, 1), (1, 0)):
            _scale_case(vals, scale, w_off, s_off)
        for w_off in (0, 1):
            _scale_case(vals, scale, w_off, 0, shadow=False)


def test_scale_shadow_rounds_to_nearest_even(gpu):
    """scale = 1 on exact bf16 ties of both parities, +-0 and +-inf: w unchanged, shadow the
    torch cast, bit for bit, on the vector and the scalar path."""
    vals = sc.bf16_edge_vector()
    assert vals.numel() % 4 == 0 and not bool(torch.isnan(vals).any())
    low = _bits(vals)[:-4] & 0xFFFF
    assert bool((low == 0x8000).all())
    for off in (0, 1):
        _scale_case(vals, 1.0, off, off)
