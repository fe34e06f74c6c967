"""Pooling and LRN, CPU side (tests/test_pool_lrn_oracle_gpu.py holds the HIP kernels to the same
oracles and bounds; tests/pool_lrn_cases.py has them): the bounds admit a correct fp32
implementation (ops.ref) on every case, every mutant of the oracles violates them by at least 10x,
and the host-side predicates of the fp8 side output and of the LRN -> pool backward fusion on the
new shapes."""
import dataclasses

import pytest
import torch

import pool_lrn_cases as pc
from sparknet_amd.ops import ref
from sparknet_amd.ops.spec import POOL_AVE, POOL_MAX


# --- the bounds admit ops.ref -------------------------------------------------------------------

@pytest.mark.parametrize("method", pc.METHODS, ids=["max", "ave"])
@pytest.mark.parametrize("case", pc.POOL_CASES, ids=pc.POOL_IDS)
def test_pool_bounds_admit_the_fp32_reference(case, method):
    s = pc.pool_spec(case, method)
    for variant, gate in pc.pool_runs():
        i = pc.pool_inputs(case, variant)
        y = ref.pool_forward(i["x"], s)
        assert y.dtype == torch.bfloat16 and tuple(y.shape) == (s.N, s.P, s.Q, s.C)
        yr, yb, _ = pc.pool_forward_bound(case, method, variant, gate)
        assert pc.worst(y, yr, yb) <= 1.0, (variant, gate)
        dx = ref.pool_backward(i["dy"], i["x"], s, gate=gate)
        assert pc.worst(dx, *pc.pool_backward_bound(case, method, variant, gate)) <= 1.0, (variant, gate)


@pytest.mark.parametrize("case", pc.LRN_CASES, ids=pc.LRN_IDS)
def test_lrn_bounds_admit_the_fp32_reference(case):
    i, h = pc.lrn_inputs(case), pc.hyper(case)
    y = ref.lrn_forward(i["x"], h.size, h.alpha, h.beta, h.k, h.within)
    assert y.dtype == torch.bfloat16
    assert pc.worst(y, *pc.lrn_forward_bound(case)) <= 1.0
    dx = ref.lrn_backward(i["dy"], i["x"], h.size, h.alpha, h.beta, h.k, h.within)
    assert pc.worst(dx, *pc.lrn_backward_bound(case, False)) <= 1.0
    assert pc.worst(ref.relu_backward(dx, i["x"]), *pc.lrn_backward_bound(case, True)) <= 1.0


def test_the_oracle_mask_matches_a_loop_over_one_case():
    """The vectorised mask against the definition, window by window, on the non-square case."""
    case = pc.NON_SQUARE
    s, x = pc.pool_spec(case), pc.pool_inputs(case, "relu")["x"].double()
    for gate in (False, True):
        y, mask = pc.max_forward64(x, s, gate)
        for p in range(s.P):
            for q in range(s.Q):
                hs, ws = p * s.sh - s.ph, q * s.sw - s.pw
                best = torch.full((s.N, s.C), float("-inf"), dtype=torch.float64)
                arg = torch.zeros((s.N, s.C), dtype=torch.int64)
                for h in range(max(hs, 0), min(hs + s.kh, s.H)):
                    for w in range(max(ws, 0), min(ws + s.kw, s.W)):
                        better = x[:, h, w] > best
                        best = torch.where(better, x[:, h, w], best)
                        arg = torch.where(better, torch.full_like(arg, (h - hs) * s.kw + (w - ws)), arg)
                if gate:
                    arg = torch.where(best > 0, arg, torch.full_like(arg, 255))
                assert torch.equal(y[:, p, q], best) and torch.equal(mask[:, p, q], arg), (gate, p, q)


# --- every mutant violates its bound ------------------------------------------------------------

def _overlap(*ts):
    p, q = min(t.shape[1] for t in ts), min(t.shape[2] for t in ts)
    return [t[:, :p, :q] for t in ts]


def _ave_forward_mutant(case, variant="randn", geometry=None, **kw):
    s = pc.pool_spec(case, POOL_AVE)
    yr, yb, _ = pc.pool_forward_bound(case, POOL_AVE, variant)
    got = pc.ave_forward64(pc.pool_inputs(case, variant)["x"], dataclasses.replace(s, **(geometry or {})), **kw)
    return pc.worst(*_overlap(got, yr, yb))  # another geometry: compared where both outputs exist


def _ave_backward_mutant(case, geometry=None, **kw):
    """geometry: a backward that places dy's leading rows and columns with another stride or pad."""
    s, i = pc.pool_spec(case, POOL_AVE), pc.pool_inputs(case, "randn")
    m = dataclasses.replace(s, **(geometry or {}))
    got = pc.ave_backward64(pc.fit(i["dy"], m.P, m.Q), m, **kw)
    return pc.worst(got, *pc.pool_backward_bound(case, POOL_AVE, "randn"))


def _max_backward_geometry_mutant(case, geometry):
    """The true mask and dy, routed by a backward with another stride or pad."""
    s, i = pc.pool_spec(case, POOL_MAX), pc.pool_inputs(case, "randn")
    m = dataclasses.replace(s, **geometry)
    mask = pc.fit(pc.max_forward64(i["x"], s)[1], m.P, m.Q, fill=255)
    got = pc.max_backward64(pc.fit(i["dy"], m.P, m.Q), mask, m, strict=False)
    return pc.worst(got, *pc.pool_backward_bound(case, POOL_MAX, "randn"))


def _max_forward_mutant(case, gate=False, geometry=None, **kw):
    """(value, mask): inf where the mutant differs from the oracle at all."""
    s = pc.pool_spec(case, POOL_MAX)
    yr, _, mr = pc.pool_forward_bound(case, POOL_MAX, "relu", gate)
    y, m = pc.max_forward64(pc.pool_inputs(case, "relu")["x"], dataclasses.replace(s, **(geometry or {})), gate, **kw)
    y, yr, m, mr = _overlap(y, yr, m, mr)
    return pc.exact(y, yr), pc.exact(m, mr)


def _max_backward_mutant(case, gate=False, uncovered=0.0, **kw):
    """dx routed by a mutant's mask, against the bound of the backward."""
    s, i = pc.pool_spec(case, POOL_MAX), pc.pool_inputs(case, "relu")
    mask = pc.max_forward64(i["x"], s, gate, **kw)[1]
    return pc.worst(pc.max_backward64(i["dy"], mask, s, uncovered=uncovered),
                    *pc.pool_backward_bound(case, POOL_MAX, "relu", gate))


def _swap(s, a, b):
    return {a: getattr(s, b), b: getattr(s, a)}


def _sw(case, a, b):
    return _swap(pc.pool_spec(case), a, b)


POOL_MUTANTS = {
    "ave forward: sh and sw swapped": lambda c: _ave_forward_mutant(c, geometry=_sw(c, "sh", "sw")),
    "ave forward: ph and pw swapped": lambda c: _ave_forward_mutant(c, geometry=_sw(c, "ph", "pw")),
    "ave forward: divisor counts in-image elements only": lambda c: _ave_forward_mutant(c, in_image_divisor=True),
    "ave forward: the last output row skipped": lambda c: _ave_forward_mutant(c, skip_last_row=True),
    "ave backward: divisor counts in-image elements only": lambda c: _ave_backward_mutant(c, in_image_divisor=True),
    "ave backward: uncovered pixels left non-zero": lambda c: _ave_backward_mutant(c, uncovered=1.0),
    "ave backward: sh and sw swapped": lambda c: _ave_backward_mutant(c, geometry=_sw(c, "sh", "sw")),
    "ave backward: ph and pw swapped": lambda c: _ave_backward_mutant(c, geometry=_sw(c, "ph", "pw")),
    "max backward: sh and sw swapped": lambda c: _max_backward_geometry_mutant(c, _sw(c, "sh", "sw")),
    "max backward: ph and pw swapped": lambda c: _max_backward_geometry_mutant(c, _sw(c, "ph", "pw")),
    "max forward: sh and sw swapped": lambda c: _max_forward_mutant(c, geometry=_sw(c, "sh", "sw"))[0],
    "max forward: ph and pw swapped": lambda c: _max_forward_mutant(c, geometry=_sw(c, "ph", "pw"))[0],
    "max forward: the last output row skipped": lambda c: _max_forward_mutant(c, skip_last_row=True)[0],
    "mask: offsets with kh in place of kw": lambda c: _max_forward_mutant(c, offset_kw=pc.pool_spec(c).kh)[1],
    "mask: the last maximum instead of the first": lambda c: _max_forward_mutant(c, last=True)[1],
    "mask: the gate ignored": lambda c: _max_forward_mutant(c, gate=True, ignore_gate=True)[1],
    "max backward: the last maximum instead of the first": lambda c: _max_backward_mutant(c, last=True),
    "max backward: the gate ignored": lambda c: _max_backward_mutant(c, gate=True, ignore_gate=True),
    "max backward: uncovered pixels left non-zero": lambda c: _max_backward_mutant(c, uncovered=1.0),
}
# the case that must hold the difference, where only one can
DESIGNATED = {
    "ave forward: sh and sw swapped": pc.NON_SQUARE,
    "max forward: sh and sw swapped": pc.NON_SQUARE,
    "mask: offsets with kh in place of kw": pc.NON_SQUARE,
    "ave backward: sh and sw swapped": pc.NON_SQUARE,
    "ave backward: ph and pw swapped": pc.NON_SQUARE,
    "max backward: sh and sw swapped": pc.NON_SQUARE,
    "max backward: ph and pw swapped": pc.NON_SQUARE,
    "ave backward: uncovered pixels left non-zero": pc.STRIDE_ABOVE_KERNEL,
    "max backward: uncovered pixels left non-zero": pc.STRIDE_ABOVE_KERNEL,
}


@pytest.mark.parametrize("name", sorted(POOL_MUTANTS))
def test_every_pool_mutant_violates_its_bound(name):
    if name in DESIGNATED:
        assert POOL_MUTANTS[name](DESIGNATED[name]) >= 10.0
        return
    ratios = {c: POOL_MUTANTS[name](c) for c in pc.POOL_CASES}
    assert max(ratios.values()) >= 10.0, ratios


def test_swapped_pads_show_on_every_case_where_they_differ():
    for c in pc.POOL_CASES:
        s = pc.pool_spec(c)
        if s.ph != s.pw:
            assert POOL_MUTANTS["ave forward: ph and pw swapped"](c) >= 10.0, c
            assert POOL_MUTANTS["max forward: ph and pw swapped"](c) >= 10.0, c


def _lrn_forward_mutant(case, **kw):
    return pc.worst(pc.lrn_forward64(pc.lrn_inputs(case)["x"], pc.hyper(case), **kw), *pc.lrn_forward_bound(case))


def _lrn_backward_mutant(case, gate=False, **kw):
    i = pc.lrn_inputs(case)
    return pc.worst(pc.lrn_backward64(i["dy"], i["x"], pc.hyper(case), gate, **kw), *pc.lrn_backward_bound(case, gate))


def _both(**kw):
    """A mutant of the window geometry (pc.Window) or of the scale, forward and backward."""
    win = {k: kw.pop(k) for k in list(kw) if k in pc.Window._fields}
    kw["win"] = pc.Window(**win)
    return {"forward": lambda c: _lrn_forward_mutant(c, **kw), "backward": lambda c: _lrn_backward_mutant(c, **kw)}


_ANY, _ACROSS, _WITHIN = (pc.ACROSS, pc.WITHIN), (pc.ACROSS,), (pc.WITHIN,)
LRN_MUTANTS = {  # name: (the kinds of case it applies to, the ratio of a case)
    "forward: the identity": (_ANY, lambda c: _lrn_forward_mutant(c, identity=True)),
    "backward: dy passed through": (_ANY, lambda c: _lrn_backward_mutant(c, passthrough=True)),
    "backward: the neighbour term dropped": (_ANY, lambda c: _lrn_backward_mutant(c, no_neighbours=True)),
    "backward: the gate ignored": (_ANY, lambda c: _lrn_backward_mutant(c, gate=True, ignore_gate=True)),
    "forward: window shifted by one channel": (_ACROSS, _both(shift=1)["forward"]),
    "backward: window shifted by one channel": (_ACROSS, _both(shift=1)["backward"]),
    "forward: farthest neighbour dropped": (_ACROSS, _both(drop_far=True)["forward"]),
    "backward: farthest neighbour dropped": (_ACROSS, _both(drop_far=True)["backward"]),
    "forward: neighbours in another chunk read as zero": (_ACROSS, _both(chunk_zero=True)["forward"]),
    "backward: neighbours in another chunk read as zero": (_ACROSS, _both(chunk_zero=True)["backward"]),
    "forward: alpha / size as alpha": (_ACROSS, _both(alpha_undivided=True)["forward"]),
    "backward: alpha / size as alpha": (_ACROSS, _both(alpha_undivided=True)["backward"]),
    "forward: within-channel divisor size, not size^2": (_WITHIN, _both(divisor_size=True)["forward"]),
    "backward: within-channel divisor size, not size^2": (_WITHIN, _both(divisor_size=True)["backward"]),
    "forward: within-channel box one short at the image edge": (_WITHIN, _both(clip_short=True)["forward"]),
    "backward: within-channel box one short at the image edge": (_WITHIN, _both(clip_short=True)["backward"]),
}
# mutants that no case may hide: every case of the kind has to show them (the single pixel has no
# neighbours and no edge to clip; one chunk has no other chunk)
EVERY_CASE = {"forward: the identity", "backward: dy passed through", "backward: the gate ignored",
              "forward: window shifted by one channel", "backward: window shifted by one channel",
              "forward: farthest neighbour dropped", "backward: farthest neighbour dropped",
              "forward: alpha / size as alpha", "backward: alpha / size as alpha",
              "forward: within-channel divisor size, not size^2", "backward: within-channel divisor size, not size^2"}


@pytest.mark.parametrize("name", sorted(LRN_MUTANTS))
def test_every_lrn_mutant_violates_its_bound(name):
    kinds, fn = LRN_MUTANTS[name]
    ratios = {c: fn(c) for c in pc.LRN_CASES if c[0] in kinds}
    assert max(ratios.values()) >= 10.0, ratios
    if name in EVERY_CASE:
        assert min(ratios.values()) >= 10.0, ratios


def test_every_kernel_kind_sees_the_neighbour_term():
    """The neighbour term of the backward shows at >= 10x in each of the three families: the vector
    and the scalar cross-channel kernels and the within-channel ones."""
    fn = LRN_MUTANTS["backward: the neighbour term dropped"][1]
    for cases in (pc.LRN_CASES[:5], pc.LRN_CASES[5:8], pc.LRN_CASES[8:11]):
        for c in cases:
            assert fn(c) >= 10.0, c


# --- workgroup counts: which cases reach xcd_block's remap ----------------------------------------

def _grids(s):
    """(forward, backward) workgroup counts of sn_pool_fwd / sn_pool_bwd (csrc/kernels/pool.hip),
    from the launch formulas: 256-thread blocks over one thread per 8-channel chunk (per channel
    when C % 8) of an output pixel, of an input pixel, or of a 2x2 input block for 3x3 / stride 2;
    64-thread blocks for an average forward below 256 * 1024 threads.  Every one of these kernels
    maps its block through xcd_block, which is the identity below 16 workgroups."""
    blocks = lambda n, per: max(1, -(-n // per))
    vec = s.C % 8 == 0
    cv = s.C // 8 if vec else s.C
    total = s.N * s.P * s.Q * cv
    fwd = blocks(total, 256) if s.method == POOL_MAX else blocks(total, 64 if total < 256 * 1024 else 256)
    if vec and (s.kh, s.kw, s.sh, s.sw) == (3, 3, 2, 2):
        bwd = blocks(s.N * ((s.H + s.ph + 1) // 2) * ((s.W + s.pw + 1) // 2) * cv, 256)
    else:
        bwd = blocks(s.N * s.H * s.W * cv, 256)
    return fwd, bwd


def test_workgroup_counts_reach_the_xcd_remap_with_a_remainder():
    remapped = lambda g: g >= 17 and g % 8 != 0
    for case in pc.XCD_REMAP:
        for method in pc.METHODS:
            fwd, bwd = _grids(pc.pool_spec(case, method))
            assert remapped(fwd) and remapped(bwd), (case, method, fwd, bwd)
    assert [_grids(pc.pool_spec(c, m)) for c in pc.XCD_REMAP for m in pc.METHODS] == \
        [(17, 20), (68, 20), (19, 71), (73, 71)]
    # the counts the case comments state for the issue's last case: below the remap
    assert [_grids(pc.pool_spec(pc.POOL_CASES[12], m)) for m in pc.METHODS] == [(4, 5), (15, 5)]
    # between them the remapped cases take the vector fixed-window forwards, the vector average
    # forward, the 3x3 / stride-2 blocked backward and the pool_bwd_k gather
    assert {c[4:8] for c in pc.XCD_REMAP} == {(3, 3, 2, 2), (2, 2, 2, 2)} and all(c[3] % 8 == 0 for c in pc.XCD_REMAP)


# --- host-side predicates on the new shapes ------------------------------------------------------

def test_pool_side_ok_truth_table():
    from sparknet_amd.ops.hip import pool_side_ok
    table = {  # case: (MAX forward, MAX backward, AVE forward, AVE backward)
        pc.POOL_CASES[0]: (True, False, False, False),    # 3x3 / stride 2: the blocked backward has no side output
        pc.POOL_CASES[1]: (True, False, False, False),
        pc.POOL_CASES[2]: (True, False, False, False),
        pc.POOL_CASES[3]: (True, True, False, True),      # 2x2 / stride 2: nh = nw = 1
        pc.POOL_CASES[4]: (True, True, False, True),      # stride above kernel: nh = nw = 1
        pc.POOL_CASES[5]: (False, True, False, True),     # 3x2 forward is generic; nh = nw = 2
        pc.POOL_CASES[6]: (False, False, False, False),   # nh = 3, nw = 2
        pc.POOL_CASES[7]: (False, False, False, False),   # 7x7 / stride 1: nh = 7
        pc.POOL_CASES[8]: (True, True, False, True),      # 3x3 / stride 1: nh = nw = 3
        pc.POOL_CASES[9]: (False, False, False, False),   # C % 8
        pc.POOL_CASES[10]: (False, False, False, False),  # C % 8
        pc.POOL_CASES[11]: (True, False, False, False),
        pc.POOL_CASES[12]: (True, False, False, False),
        pc.POOL_CASES[13]: (True, False, False, False),
        pc.POOL_CASES[14]: (True, True, False, True),
    }
    assert set(table) == set(pc.POOL_CASES)
    for case, want in table.items():
        got = tuple(pool_side_ok(pc.pool_spec(case, m), b) for m in (POOL_MAX, POOL_AVE) for b in (False, True))
        assert got == want, (case, got)
    side = [(pool_side_ok(pc.pool_spec(c), False), pool_side_ok(pc.pool_spec(c), True)) for c in pc.CHUNK_CASES]
    assert side == [(True, True), (True, False), (False, True)]


def test_pool_lrn_rev_eligible_truth_table():
    from sparknet_amd.ops.hip import pool_lrn_rev_eligible
    for case in pc.FUSED_CASES:
        s = pc.fused_spec(case)
        assert pool_lrn_rev_eligible(s, case[5], False), case
        assert not pool_lrn_rev_eligible(s, case[5], True)
        assert not pool_lrn_rev_eligible(s, 11, False) and not pool_lrn_rev_eligible(s, 4, False)
        assert not pool_lrn_rev_eligible(dataclasses.replace(s, method=POOL_AVE), case[5], False)
        assert not pool_lrn_rev_eligible(dataclasses.replace(s, C=s.C + 4), case[5], False)
        assert not pool_lrn_rev_eligible(dataclasses.replace(s, ph=3, pw=3), case[5], False)
    # of the pooling cases: the 3x3 / stride-2 ones with whole 8-channel chunks, pads 2 and 1 included
    got = {c: pool_lrn_rev_eligible(pc.pool_spec(c), 5, False) for c in pc.POOL_CASES}
    want = {c: (c[4:8] == (3, 3, 2, 2) and c[3] % 8 == 0) for c in pc.POOL_CASES}
    assert got == want, got
