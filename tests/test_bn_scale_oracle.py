"""The fp64 oracle of the fused BatchNorm / Scale / ReLU kernels, CPU side
(tests/test_bn_scale_oracle_gpu.py holds csrc/kernels/bn_scale.hip to it; tests/bn_scale_cases.py
has the cases, the oracle and the bounds): the oracle agrees with torch's batch_norm, relu and
autograd in float64, every mutant of it violates a bound by at least 10x on some case while the
oracle recomputed from fp32-rounded coefficients stays inside, the case list reaches every path of
the launch plan it claims, and no ReLU gate of a case is ambiguous."""
import pytest
import torch
import torch.nn.functional as F

import bn_scale_cases as bc

SMALL = [p for p in bc.PARAMS if p[0].R * p[0].C <= 100000]


# --- the oracle against torch --------------------------------------------------------------------

def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


@pytest.mark.parametrize("global_stats", (False, True), ids=("batch", "global"))
@pytest.mark.parametrize("relu", (False, True))
def test_oracle_agrees_with_torch(global_stats, relu):
    case = bc.BY_NAME["144x136"]
    i = bc.inputs(case, bc.F32)
    x = i.x.to(bc.F64).requires_grad_()
    gamma, beta = i.gamma.to(bc.F64).requires_grad_(), i.beta.to(bc.F64).requires_grad_()
    dy = i.dy.to(bc.F64)
    if global_stats:
        rf = bc.f32(3.7)
        t = F.batch_norm(x, i.grm.to(bc.F64) / rf, i.grv.to(bc.F64) / rf, gamma, beta, False, 0.0, i.eps)
        mu, inv = bc.coef64(bc.BN_GLOBAL, i.grm, i.grv, torch.tensor([rf]), i.eps, case.C)
    else:
        t = F.batch_norm(x, None, None, gamma, beta, True, 0.0, i.eps)
        mu, var, inv = bc.stats64(i.x, i.eps)
        xd = i.x.to(bc.F64)
        assert _rel(mu, xd.mean(0)) <= 1e-12 and _rel(var, xd.var(0, unbiased=False)) <= 1e-12
    if relu:
        t = F.relu(t)
    t.backward(dy)
    z = bc.fwd64(i.x, mu, inv, i.gamma, i.beta)
    assert _rel(bc.fwd64(i.x, mu, inv, i.gamma, i.beta, relu), t.detach()) <= 1e-12
    dx, dgamma, dbeta, _, _ = bc.bwd64(i.dy, i.x, mu, inv, i.gamma, z if relu else None, not global_stats)
    assert _rel(dx, x.grad) <= 1e-12 and _rel(dgamma, gamma.grad) <= 1e-12 and _rel(dbeta, beta.grad) <= 1e-12
    _, dga, dba, _, _ = bc.bwd64(i.dy, i.x, mu, inv, i.gamma, z if relu else None, not global_stats, prefill=bc.PREFILL)
    assert torch.equal(dga, dgamma + bc.PREFILL) and torch.equal(dba, dbeta + bc.PREFILL)


def test_running64_is_caffes_update():
    rm, rv, rf = bc.running64(torch.tensor([2.0]), torch.tensor([3.0]), torch.tensor([4.0]), torch.tensor([0.5]),
                              torch.tensor([0.25]), 0.5, 2.0)
    assert (float(rm), float(rv), float(rf)) == (1.5, 2.0, 3.0)


def test_axis64_is_a_broadcast():
    x, s, b = bc.axis_inputs(3, 5, 7, bc.F32)
    ref = x.to(bc.F64) * s.to(bc.F64).reshape(1, 5, 1) + b.to(bc.F64).reshape(1, 5, 1)
    assert torch.equal(bc.axis64(x, s, b, 5, 7), ref.reshape(-1))


# --- mutants ----------------------------------------------------------------------------------------

MUTANTS = {  # name: the keyword argument (a function of the case where it depends on R)
    "eps left out": dict(no_eps=True),
    "eps added after the square root": dict(eps_outside=True),
    "unbias = 1": dict(unbias_is=1.0),
    "unbias = R / (R + 1)": lambda c: dict(unbias_is=c.R / (c.R + 1)),
    "frac treated as 0": dict(frac_zero=True),
    "factor without its + 1": dict(no_plus_one=True),
    "s = 1 instead of 1 / rf": dict(s_one=True),
    "rf == 0 treated as s = 1": dict(zero_factor_s_one=True),
    "variance divided by R - 1": dict(div_rm1=True),
    "last row left out of the statistics": dict(stat_skip_last=True),
    "last row of the last slab left out of both backward sums": dict(sum_skip_last=True),
    "sum g / R term dropped from dx": dict(no_mean_term=True),
    "xhat sum (g xhat) / R term dropped from dx": dict(no_proj_term=True),
    "gamma left out of dx": dict(no_gamma=True),
    "ReLU gate taken from dy": dict(gate_dy=True),
    "gate z >= 0 instead of z > 0": dict(gate_ge=True),
    "GRAD_ACC treated as a store": dict(acc_as_store=True),
    "channel c reading the coefficient of c XOR 1": dict(xor1=True),
}


def _ratio(param, name):
    case, dtype, cfg = param
    kw = MUTANTS[name]
    mut = bc.evaluate(case, dtype, cfg, **(kw(case) if callable(kw) else kw))
    ref = bc.reference(case, dtype, cfg)
    return max(bc.worst(getattr(mut, q), getattr(ref, q), ref.bound[q])
               for q in bc.QUANTITIES if ref.bound[q] is not None)


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_every_mutant_violates_a_bound(name):
    ratios = {bc.PARAM_IDS[bc.PARAMS.index(p)]: _ratio(p, name) for p in SMALL}
    assert max(ratios.values()) >= 10.0, ratios


def test_the_largest_cases_see_a_dropped_row():
    """The two largest cases exist for their slab plans: a row left out of the last slab's sums, or
    of the statistics, is beyond the bound there too."""
    for case in bc.DET_CASES:
        p = (case, bc.BF16, "batch-relu")
        assert _ratio(p, "last row left out of the statistics") >= 10.0
        assert _ratio(p, "last row of the last slab left out of both backward sums") >= 10.0


def test_axis_mutant_violates_its_bound():
    ratios = []
    for inner in (1, 3, 49):
        x, s, b = bc.axis_inputs(2, 5, inner, bc.BF16)
        ratios.append(bc.worst(bc.axis64(x, s, b, 5, inner, mod_index=True), *bc.axis_bound(x, s, b, 5, inner, bc.BF16)))
    assert ratios[0] == 0.0 and min(ratios[1:]) >= 10.0, ratios  # inner = 1: e % A is the index


PER_CHANNEL = ("mean", "var", "inv", "rm", "rv", "rf", "dgamma", "dbeta", "dgamma_acc", "dbeta_acc", "c1", "c2")


@pytest.mark.parametrize("param", bc.PARAMS, ids=bc.PARAM_IDS)
def test_the_bounds_admit_fp32_coefficients(param):
    """No bound is below what the formats can give: the oracle meets its own bounds exactly, and
    still meets them when mu, inv, c1 and c2 are rounded to fp32 before the elementwise results
    are computed and every per-channel result is rounded to fp32."""
    ref = bc.reference(*param)
    r32 = bc.evaluate(*param, round32=True)
    for q in bc.QUANTITIES:
        if ref.bound[q] is None:
            continue
        assert bool((ref.bound[q] >= 0).all()), q
        assert bc.worst(getattr(ref, q), getattr(ref, q), ref.bound[q]) == 0.0
        got = getattr(r32, q)
        if q in PER_CHANNEL:
            got = got.float().to(bc.F64)
        elif param[1] == bc.F32:
            got = got.float().to(bc.F64)
        else:
            got = got.to(bc.BF16).to(bc.F64)
        assert bc.worst(got, getattr(ref, q), ref.bound[q]) <= 1.0, q


# --- the launch plan ------------------------------------------------------------------------------------

def _plans():
    """(case, dtype, plan at the lane width the case runs at)."""
    return [(c, d, bc.plan(c.R, c.C, 1 if c.view else bc.vec(c, d))) for c in bc.CASES for d in c.dtypes]


def _rows(p, n):
    return n in p.lane_rows or n in p.last_lane_rows


PATHS = {
    "one row, 255 empty row lanes": lambda c, d, p: c.R == 1 and p.TY == 256 and p.lane_rows.count(0) == 255,
    "R below the row lanes": lambda c, d, p: 1 < c.R < p.TY,
    "inactive channel lane": lambda c, d, p: p.TX * p.gx > p.CG,
    "scalar lanes, bf16": lambda c, d, p: p.V == 1 and d == bc.BF16,
    "scalar lanes, fp32": lambda c, d, p: p.V == 1 and d == bc.F32,
    "V = 8 bf16": lambda c, d, p: p.V == 8 and d == bc.BF16,
    "V = 4 fp32": lambda c, d, p: p.V == 4 and d == bc.F32,
    "V = 4 fp32 at more than one channel-group block": lambda c, d, p: p.V == 4 and p.gx > 1,
    "pick_v falls back although C % 8 == 0, x misaligned": lambda c, d, p: c.view == "x" and c.C % 8 == 0 and p.V == 1,
    "pick_v falls back although C % 8 == 0, dy misaligned": lambda c, d, p: c.view == "dy" and c.C % 8 == 0 and p.V == 1,
    "ragged channel tile of vector lanes": lambda c, d, p: p.V > 1 and p.CG % p.TX != 0,
    "several slabs, the last one short": lambda c, d, p: p.slabs > 1 and p.last < p.rps,
    "finalize chunk > 1": lambda c, d, p: p.chunk > 1,
    "want clamped to cap at gx > 1": lambda c, d, p: p.asked > p.cap == p.want and p.gx > 1,
    "finalize lane without slabs next to lanes with several": lambda c, d, p: p.chunk > 1 and 0 in p.fin,
    "a lane of 3 rows": lambda c, d, p: _rows(p, 3),
    "a lane of 4 rows": lambda c, d, p: _rows(p, 4),
    "a lane of 5 rows": lambda c, d, p: _rows(p, 5),
    "a lane of 1 row next to lanes of 2": lambda c, d, p: _rows(p, 1) and _rows(p, 2),
    "large mean": lambda c, d, p: c.mean == 1000.0,
}


@pytest.mark.parametrize("path", sorted(PATHS))
def test_the_cases_reach(path):
    assert any(PATHS[path](c, d, p) for c, d, p in _plans()), path


def test_the_plans_are_the_ones_the_case_table_states():
    P = lambda name, V: bc.plan(bc.BY_NAME[name].R, bc.BY_NAME[name].C, V)
    p = P("1x8", 8)
    assert (p.TX, p.TY, p.slabs, p.lane_rows[:2]) == (1, 256, 1, [1, 0])
    p = P("2x3", 1)
    assert (p.TX, p.TY, p.CG, p.gx, p.slabs) == (4, 64, 3, 1, 1)
    assert bc.f32(16 / 15) - 1 == pytest.approx(0.067, abs=1e-3)
    p = P("30x20", 1)
    assert (p.TY, sorted(set(p.lane_rows))) == (8, [3, 4])
    for V in (8, 4):
        p = P("19x512", V)
        assert (p.TY, p.slabs, p.lane_rows) == (4, 1, [5, 5, 5, 4])
    p = P("144x136", 8)
    assert (p.CG, p.TX, p.gx, p.slabs, p.rps, p.last) == (17, 32, 1, 3, 48, 48)
    p = P("2200x512", 8)
    assert (p.gx, p.slabs, p.rps, p.last, p.chunk) == (1, 35, 63, 58, 2)
    assert [k for k in range(32) if p.fin[k] == 0] == list(range(18, 32)) and p.fin[17] == 1
    p = P("2200x512", 4)
    assert (p.V, p.gx, p.slabs, p.rps, p.last, p.chunk) == (4, 2, 35, 63, 58, 2)
    p = P("22000x130", 1)
    assert (p.gx, p.asked, p.cap, p.want, p.slabs, p.rps, p.last, p.chunk) == (3, 344, 341, 341, 339, 65, 30, 11)
    assert [k for k in range(32) if p.fin[k] == 0] == [31] and p.fin[30] == 9
    for name in ("64x16-view-x", "64x16-view-dy"):
        assert bc.BY_NAME[name].C % 8 == 0 and bc.vec(bc.BY_NAME[name], bc.BF16) == 8
    assert max(c.R * c.C for c in bc.CASES) == 22000 * 130
    assert sum(c.eps == bc.CASES[4].eps == 0.25 for c in bc.CASES) == 2


# --- the ReLU gate -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("param", [p for p in bc.PARAMS if bc.CONFIGS[p[2]].relu],
                         ids=[i for i, p in zip(bc.PARAM_IDS, bc.PARAMS) if bc.CONFIGS[p[2]].relu])
def test_no_relu_gate_is_ambiguous(param):
    ref = bc.reference(*param)
    assert bc.ambiguous(ref) == 0
    if bc.CONFIGS[param[2]].zeros and param[0].R * param[0].C >= 30:  # the exact zeros z >= 0 would let through
        assert int((ref.z == 0).sum()) > 0
