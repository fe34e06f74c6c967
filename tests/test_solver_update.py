"""The solver update on the CPU, with no kernel involved (tests/test_solver_update_gpu.py runs
the HIP kernel against the same oracle and bounds, tests/solver_update_cases.py holds them):

* the project's fp32 formula (``ops.ref.solver_update_ref``, also through the CPU dispatch
  ``ops.solver_update``) stays within a quarter of the bound against the fp64 oracle, so the
  chosen inputs keep a correct fp32 implementation well inside the bound;
* every ingredient of the update is visible: an oracle with one ingredient wrong moves at
  least 20 % of the elements of some output by more than 500 x the tolerance, so an
  implementation that passes the bound cannot have dropped it;
* the chunk table of the HIP kernel (``ops.hip.solver_tables``, pure Python) tiles exactly
  the padded segments.
"""
import pytest
import torch

from sparknet_amd import ops
from sparknet_amd.ops import ref

import solver_update_cases as sc

# (l1, clip instance, clip mode): the four template instances plus the two no-op clips
VARIANTS = [(False, False, "none"), (True, False, "none"), (False, True, "half"), (True, True, "half"),
            (False, True, "above"), (True, True, "negative")]


def variant_id(v):
    return f"{'l1' if v[0] else 'l2'}-{'clip' if v[1] else 'noclip'}-{v[2]}"


def _quarter(got, refs, bnds, mask, what):
    for name, o, r, b in zip(("w", "h0", "h1"), got, refs, bnds):
        err = (o.double() - r).abs()[mask]
        over = err - 0.25 * b[mask]
        assert bool((over <= 0).all()), (what, name, "max error", float(err.max()), "worst excess", float(over.max()))


@pytest.mark.parametrize("variant", VARIANTS, ids=variant_id)
@pytest.mark.parametrize("kind", range(6), ids=sc.KINDS)
def test_fp32_reference_within_quarter_bound(kind, variant):
    l1, clip, mode = variant
    c = sc.case(kind)
    hyper = c.hyper(mode)
    refs, bnds = sc.case_bounds(c, hyper, l1, clip, clipped=mode == "half")
    if mode != "half":      # a clip that does not bite is the unclipped update
        for a, b in zip(refs, sc.case_oracle(c, c.hyper("none"), l1, False)):
            assert torch.equal(a[c.upd], b[c.upd])
    # the formula on per-element multipliers over the padded ranges
    w, g, hist = c.w.clone(), c.g.clone(), [c.h0.clone(), c.h1.clone()]
    ref.solver_update_ref(kind, w, g, hist, c.lr, c.dc, hyper.tolist(), l1, clip)
    _quarter((w, hist[0], hist[1] if kind >= 4 else c.h1), refs, bnds, c.upd, "solver_update_ref")
    # the CPU dispatch with its own tables (multipliers on the parameters themselves)
    w, g, hist = c.w.clone(), c.g.clone(), [c.h0.clone(), c.h1.clone()]
    shadow = torch.empty_like(w)
    tabs = ops.solver_tables(c.segs, c.total, device="cpu")
    ops.solver_update(kind, w, g, hist, shadow, tabs, hyper, l1, clip)
    _quarter((w, hist[0], hist[1] if kind >= 4 else c.h1), refs, bnds, c.real, "ops.solver_update")
    assert torch.equal(shadow[c.real], w[c.real])
    if kind < 4:
        assert torch.equal(hist[1], c.h1)


@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
@pytest.mark.parametrize("kind", range(6), ids=sc.KINDS)
def test_every_ingredient_is_visible(kind, l1):
    """With clipping at half the norm (the case the GPU test runs), each applicable mutant is
    more than 500 x the tolerance away from the oracle on at least 20 % of the updated
    elements of at least one output."""
    c = sc.case(kind)
    hyper = c.hyper("half")
    refs = sc.case_oracle(c, hyper, l1, True)
    tried = 0
    for mutant in sc.MUTANTS:
        if not sc.mutant_applies(mutant, kind, True):
            continue
        tried += 1
        frac = sc.moved_fraction(sc.case_oracle(c, hyper, l1, True, mutant=mutant), refs, c.upd)
        assert frac >= 0.20, (sc.KINDS[kind], mutant, "moves only", frac)
    assert tried == 6 + (kind >= 2) + (kind == 5) + (kind in (3, 5)) + (kind >= 4)


def test_mutants_without_clipping_and_gradient_error_terms():
    """The unclipped instances see the same ingredients; the clipping term of the bound stays
    within 10 x the tolerance, far below the sensitivity threshold (no mutant hides in it)."""
    for kind in range(6):
        c = sc.case(kind)
        hyper = c.hyper("none")
        refs = sc.case_oracle(c, hyper, False, False)
        for mutant in sc.MUTANTS:
            if mutant != "no_clip" and sc.mutant_applies(mutant, kind, False):
                assert sc.moved_fraction(sc.case_oracle(c, hyper, False, False, mutant=mutant), refs, c.upd) >= 0.20
        refs, bnds = sc.case_bounds(c, c.hyper("half"), False, True, clipped=True)
        for r, b in zip(refs, bnds):
            assert bool((b[c.upd] <= 10 * sc.TOL * r.abs().clamp(min=1.0)[c.upd]).all())


def test_case_layout():
    segs, total = sc.layout()
    assert [cnt for _, cnt, _, _ in segs] == [1, 4, 63, 64, 1000, 8192, 8192 + 64, 20000]
    assert {lm for _, _, lm, _ in segs} == {1.0, 2.0, 0.5, 0.0} and {dm for _, _, _, dm in segs} == {1.0, 0.0, 3.0}
    assert sc.padded(20000) == 20032 and total <= 41000
    c = sc.case(0)
    assert all(off % 4 == 0 for off, _, _, _ in segs) and bool(c.gap.any())
    assert float(c.g[c.gap].abs().max()) == 0.0 and bool((c.w[c.gap] == sc.SENTINEL).all())
    zeros = c.w[c.upd] == 0
    assert 0.03 < float(zeros.float().mean()) < 0.09
    assert bool(torch.signbit(c.w[c.upd][zeros]).any()) and not bool(torch.signbit(c.w[c.upd][zeros]).all())
    assert bool((c.h0[c.upd] < 0).any()) and bool((c.h0[c.upd] > 0).any())
    assert float(sc.case(5).h0[c.upd].min()) >= 0.1
    assert c.nchunks() == 4 + 1 + 1 + 2 + 3


# --------------------------------------------------------------------------------------
# chunk table of the HIP kernel (pure Python)
# --------------------------------------------------------------------------------------

def _hip():
    return pytest.importorskip("sparknet_amd.ops.hip")


def _covered(pos):
    out = set()
    for start, count in pos:
        rng = set(range(start, start + count))
        assert not (out & rng), "chunks overlap"
        out |= rng
    return out


def test_chunk_table_tiles_the_padded_segments():
    hip = _hip()
    assert hip.CHUNK == sc.CHUNK
    c = sc.case(0)
    t = hip.solver_tables(c.segs, c.total, "cpu")
    pos, mult = t["pos"].tolist(), t["mult"].tolist()
    assert t["n"] == len(pos) == len(mult) == c.nchunks() and t["src"] is None and t["total"] == c.total
    assert all(s % 4 == 0 and n % 4 == 0 and 0 < n <= hip.CHUNK for s, n in pos)
    want = set()
    for off, cnt, _, _ in c.segs:
        want |= set(range(off, off + sc.padded(cnt)))
    assert _covered(pos) == want == set(torch.nonzero(c.upd).flatten().tolist())
    for (s, n), (lm, dm) in zip(pos, mult):
        assert bool((c.lr[s:s + n] == lm).all()) and bool((c.dc[s:s + n] == dm).all())
    # the last segment: 20000 pads to 20032 = 8192 + 8192 + 3648
    assert [n for s, n in pos[-3:]] == [8192, 8192, 3648]
    assert 1 <= t["part"].numel() <= 1024 and t["part"].numel() * 256 * 16 >= c.total
    empty = hip.solver_tables([], 0, "cpu")
    assert empty["n"] == 0 and empty["pos"].shape == (1, 2)


def test_chunk_table_slab_variant():
    hip = _hip()
    s = sc.slab_case(0, 5)
    base = 1 << 20
    chunks = s.slab_chunks(base)
    t = hip.solver_tables(s.segs, s.total, "cpu", chunks)
    pos, mult, src = t["pos"].tolist(), t["mult"].tolist(), t["src"].tolist()
    G, M, N, ldw = sc.SLAB_G, sc.SLAB_M, sc.SLAB_N, sc.SLAB_LDW
    assert t["n"] == len(pos) == len(src) == G * M + G + 1
    assert _covered(pos) == set(torch.nonzero(s.upd).flatten().tolist())
    assert all(st % 4 == 0 and n % 4 == 0 for st, n in pos)
    for i in range(G * M):
        g, m = divmod(i, M)
        assert pos[i] == [sc.SLAB_OFF_W + i * N, N] and mult[i] == [1.0, 1.0]
        assert src[i] == [base + 4 * ((g * 5 + 0) * M * ldw + m * ldw), M * ldw, 5, 1]
    for g in range(G):
        i = G * M + g
        assert pos[i] == [sc.SLAB_OFF_B + g * M, M] and mult[i] == [2.0, 0.0]
        assert src[i] == [base + 4 * (g * 5 * M * ldw + N), M * ldw, 5, ldw]
    assert pos[-1] == [sc.SLAB_OFF_F, sc.padded(sc.SLAB_FLAT)] and src[-1] == [0, 0, 0, 0] and mult[-1] == [0.5, 3.0]
    # a slab chunk longer than CHUNK is cut; each piece's slab address advances by 4 * s * es bytes
    for es in (1, 24):
        n = 2 * hip.CHUNK + 100
        t = hip.solver_tables([(64, n, 1.0, 1.0)], 64 + n, "cpu", {64: [(64, n, base, 7 * n * es, 3, es)]})
        assert t["pos"].tolist() == [[64, 8192], [64 + 8192, 8192], [64 + 16384, 100]]
        assert t["src"].tolist() == [[base + 4 * k * 8192 * es, 7 * n * es, 3, es] for k in range(3)]
