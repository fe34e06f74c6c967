"""Shared cases, inputs, fp64 oracle, mutants, launch-plan replica and error bounds of
tests/test_bn_scale_oracle.py (CPU) and tests/test_bn_scale_oracle_gpu.py (csrc/kernels/bn_scale.hip:
the Welford statistics with Caffe's running-blob update, the fused forward
``y = relu?(gamma (x - mu) inv + beta)``, the two backward passes and the general per-axis
Scale / Bias).

Nothing here calls the code under test.  The oracle is plain float64 torch on ``[R][C]`` tensors
and reads float64 copies of exactly the values the kernels read: x and dy as stored (bf16 values
for the bf16 cases, plain fp32 values for the fp32 cases), the fp32 per-channel vectors, and the
scalars eps, frac and unbias after their conversion to fp32.  With batch statistics the forward and
backward kernels read the fp32 vectors ``mean`` and ``inv_std``; the oracle (and the GPU test)
gives them the fp32 rounding of ``stats64``, so each kernel is held to the oracle of what it reads,
and one further GPU test runs the forward on the statistics kernel's own output with the
propagated bound.  Each mutant is one keyword argument.

Cases are ``(R, C)`` plus the tensor types, the smallest shapes that reach each path of
``make_plan`` and of the finalize kernels; ``plan`` below is a transcription of ``make_plan`` and
tests/test_bn_scale_oracle.py asserts with it, by name, that every path is reached:

=================  ==========  ==================================================================
(1, 8)             bf16 fp32   one row: var 0, inv = rsqrt(eps), unbias = 1; TY = 256, 255 empty
                               row lanes
(2, 3)             bf16        scalar lanes, TX = 4 with an inactive channel lane, R < TY = 64
(16, 10)           bf16 fp32   the 2-D blob of the older tests; unbias - 1 = 6.7 %
(98, 3) (30, 20)   bf16        the older scalar-tail shapes; (30, 20) has lanes of 4 and of 3 rows
(19, 512)          bf16 fp32   TY = 4, lanes of 5, 5, 5, 4 rows: the U = 4 loop and the two-row
                               loops run with and without a tail
(144, 136)         bf16 fp32   vector lanes, ragged channel tile (17 of 32 lanes), 3 slabs of 48
(2200, 512)        bf16 fp32   35 slabs of 63 rows, the last of 58; finalize chunk = 2, lanes
                               18 - 31 empty; fp32: V = 4 and gx = 2
(22000, 130)       bf16        scalar lanes, gx = 3, want clamped from 344 to cap = 341; 339 slabs
                               of 65 rows, the last of 30; chunk = 11, finalize lane 31 empty
(64, 16) view      bf16 fp32   a view one element into a larger buffer: pick_v falls back to
                               V = 1 although C % 8 == 0; once x, once dy misaligned
(128, 64) + 1000   bf16 fp32   x = 1000 + randn: Welford against cancellation, under the same bound
=================  ==========  ==================================================================

Configurations (``CONFIGS``): batch statistics with ReLU, gamma and beta; batch statistics bare;
global statistics (factor 3.7) with ReLU; global statistics with factor 0 and no beta; no
normalisation with gamma and a ReLU on an x with exact zeros (the only place where ``z > 0`` and
``z >= 0`` differ); no normalisation with beta alone (the Bias layer's call, need_x = 0).  The two
largest cases and the large-mean case run a subset (``configs``).  (30, 20) and (144, 136) use
eps = 0.25 on an x of variance 0.1, so that leaving eps out or adding it outside the root is
visible; the running blobs of the batch cases start at non-zero values with frac = 0.9.

Inputs are seeded by (case, type).  The kernels gate the backward on the stored ``y > 0``, the
oracle on ``z64 > 0``; the two can differ only where ``|z64|`` is within the forward bound (before
the rounding to bf16) of zero.  That set must be empty, which the CPU test asserts for every case
with a ReLU; where the bound itself is 0 (x = 0 without normalisation) the kernel's z is exactly 0
and nothing is ambiguous.  ``SEED_STEP`` records, per (case, type), the first step added to the
seed at which the set is empty.

Error bounds
------------
From the number formats and the shape of each summation, never from a kernel output.
u32 = 2^-24 and u16 = 2^-8 are the unit roundoffs of fp32 and bf16; ``A`` / ``S`` stand for the
oracle's expression on absolute values (every input replaced by its magnitude, every subtraction
by an addition).

Depth.  No kernel sums R terms in a row.  A row lane walks ``ceil(rps / TY)`` rows, its block
merges the TY lanes in order, a finalize lane merges ``chunk`` slabs and lane 0 merges the 32
lanes: ``D = ceil(rps / TY) + TY + chunk + 32`` steps on the longest path.  The lane width V is 1
for a misaligned view whichever tensor is misaligned for one entry only, so D is the larger of the
two plans' depths.

* mean: ``1.01 (D + 8) u32 mean|x|``.  A Welford step ``m += (x - m) / k`` rounds the difference,
  the reciprocal (``rcpf`` in ``welford()``: 1 ulp = 2 u32, on a term that is divided by k), the
  product and the sum; the sum's error ``u32 |m_k|`` dominates and enters the result with weight
  k / n, so n steps cost at most ``n u32 mean|x|``; the other three, each a few u32 of ``|x - m| / k``,
  add up to at most ``8 u32 mean|x|`` over a lane.  A Chan merge is one such step.
* var: ``1.01 (D + 8) u32 kappa var`` with ``kappa = sqrt(1 + R mean^2 / M2) = sqrt(1 + mean^2 / var)``,
  the condition number of the variance: the bound of Chan, Golub and LeVeque (1983) for the
  updating algorithms, n u kappa, with n the depth.  The error of the running mean, ``D u32 |mean|``,
  enters M2 through ``d (x - m)`` relative to the deviation, which is what kappa measures; this is
  what holds the large-mean case (kappa = 1000 in fp32, 650 in bf16) to a bound and not to a
  waiver.  The division by R is one of the 8.  R = 1: var = 0 exactly.
* inv_std: ``inv (0.5 B_var / (var + eps) + 4 u32)``: the propagated error of the radicand, its own
  rounding and ``rsqrtf`` (1 ulp).
* running blobs: factor ``2 u32 (|frac f| + 1)``; mean ``2 u32 (|frac m| + |mean|) + B_mean``;
  variance ``3 u32 (|frac v| + unbias var) + unbias B_var``.
* coefficients computed inside a kernel (global statistics): ``s = 1 / f`` and the product give
  ``d_mu = 3 u32 |mu|``; the radicand's two roundings and rsqrtf give ``d_inv = 5 u32 inv``.  Batch
  statistics and no normalisation: both 0, the kernel reads the very values the oracle reads.
* forward, before it is stored: ``B_z = |gamma| (inv d_mu + |x - mu| d_inv) + 4 u32 A`` with
  ``A = |gamma| (|x| + |mu|) inv + |beta|`` (the difference, ``gamma inv``, the fma; one spare).
  Stored as bf16: ``u16 |ref|`` more; as fp32 the last rounding is among the four.
* dbeta: ``1.01 (D + 2) u32 S``, ``S = sum |g|``.  dgamma: ``1.01 (D + 6) u32 S``,
  ``S = sum |g| (|x| + |mu|) inv`` (each term carries the roundings of xhat), plus
  ``sum |g| (inv d_mu + |x - mu| d_inv)``.  Accumulated onto the prefill of 7.0: one more term, on
  ``S + 7``.
* the coefficients of pass 2, ``c = sum / R``: the sum's bound over R, plus ``2 u32 |c|`` (``1 / R``
  and the product).
* dx, batch statistics: ``u16 |ref| + 8 u32 A + |gamma| inv (B_c1 + |xhat| B_c2)`` with
  ``A = |gamma| inv (|g| + |c1| + (|x| + |mu|) inv |c2|)`` (seven roundings; the GPU test feeds
  pass 2 the coefficients pass 1 produced, so their error propagates).  Otherwise
  ``(u16 + 3 u32) |ref| + |g gamma| d_inv``.  fp32 tensors: without the u16 term.
* axis_scale_bias: ``u16 |ref| + 2 u32 (|x| |s| + |b|)``.
"""
import functools
import math
import zlib
from collections import namedtuple
from types import SimpleNamespace

import torch

U32 = 2.0 ** -24
U16 = 2.0 ** -8
PREFILL = 7.0
F64 = torch.float64
BF16 = torch.bfloat16
F32 = torch.float32
BN_NONE, BN_BATCH, BN_GLOBAL = 0, 1, 2
BOTH = (BF16, F32)

Case = namedtuple("Case", "name R C dtypes eps view mean", defaults=(1e-5, None, 0.0))
CASES = (
    Case("1x8", 1, 8, BOTH),
    Case("2x3", 2, 3, (BF16,)),
    Case("16x10", 16, 10, BOTH),
    Case("98x3", 98, 3, (BF16,)),
    Case("30x20", 30, 20, (BF16,), eps=0.25),
    Case("19x512", 19, 512, BOTH),
    Case("144x136", 144, 136, BOTH, eps=0.25),
    Case("2200x512", 2200, 512, BOTH),
    Case("22000x130", 22000, 130, (BF16,)),
    Case("64x16-view-x", 64, 16, BOTH, view="x"),
    Case("64x16-view-dy", 64, 16, BOTH, view="dy"),
    Case("128x64-mean1000", 128, 64, BOTH, mean=1000.0),
)
BY_NAME = {c.name: c for c in CASES}
DET_CASES = (BY_NAME["2200x512"], BY_NAME["22000x130"])  # two runs must be bitwise equal

Config = namedtuple("Config", "mode relu gamma beta factor zeros", defaults=(None, False))
CONFIGS = {
    "batch-relu": Config(BN_BATCH, True, True, True),
    "batch-bare": Config(BN_BATCH, False, False, False),
    "global-relu": Config(BN_GLOBAL, True, True, True, 3.7),
    "global-factor0": Config(BN_GLOBAL, False, True, False, 0.0),
    "none-relu": Config(BN_NONE, True, True, False, zeros=True),
    "none-bias": Config(BN_NONE, False, False, True),
}


def configs(case):
    if case.mean:  # |z| reaches the forward bound on 8192 elements: no ReLU here
        return ("batch-bare", "global-factor0", "none-bias")
    if case.R * case.C > 500000:
        return ("batch-relu", "global-factor0")
    return tuple(CONFIGS)


def dname(dtype):
    return "bf16" if dtype == BF16 else "fp32"


PARAMS = [(c, d, k) for c in CASES for d in c.dtypes for k in configs(c)]
PARAM_IDS = [f"{c.name}-{dname(d)}-{k}" for c, d, k in PARAMS]

# first step added to crc32(name, type) at which no ReLU gate of the case is ambiguous; a pair that
# is not listed needs none (at the two largest cases the smallest |z| is 2.4, 7.4 and 71 bounds
# away from zero as seeded)
SEED_STEP = {}


# --- the launch plan ---------------------------------------------------------------------------

def vec(case, dtype):
    """Lane width of the kernels when every tensor is aligned."""
    return (8 if dtype == BF16 else 4) if case.C % 8 == 0 else 1


def plan(R, C, V):
    """make_plan of bn_scale.hip and the finalize kernels' split of the slabs over 32 lanes."""
    CG = C // V
    txlog = 0
    while (1 << txlog) < 64 and (1 << txlog) < CG:
        txlog += 1
    TX, TY = 1 << txlog, 256 >> txlog
    gx = -(-CG // TX)
    cap = max(1024 // gx, 1)
    min_rows = max(TY * 8, 64)
    asked = -(-R // min_rows)
    want = max(min(asked, cap), 1)
    rps = -(-R // want)
    slabs = -(-R // rps)
    chunk = -(-slabs // 32)
    lane_rows = lambda rows: [(-(-(rows - k) // TY) if rows > k else 0) for k in range(TY)]
    return SimpleNamespace(
        V=V, CG=CG, TX=TX, TY=TY, gx=gx, cap=cap, asked=asked, want=want, rps=rps, slabs=slabs, chunk=chunk,
        last=R - (slabs - 1) * rps, lane_rows=lane_rows(min(rps, R)), last_lane_rows=lane_rows(R - (slabs - 1) * rps),
        fin=[max(0, min(slabs, (k + 1) * chunk) - k * chunk) for k in range(32)],
        depth=-(-rps // TY) + TY + chunk + 32)


def part_floats(case, dtype):
    s = plan(case.R, case.C, 1).slabs
    if case.C % 8 == 0:
        s = max(s, plan(case.R, case.C, vec(case, dtype)).slabs)
    return 2 * case.C * s


def depth(case, dtype):
    return max(plan(case.R, case.C, 1).depth, plan(case.R, case.C, vec(case, dtype)).depth)


# --- inputs --------------------------------------------------------------------------------------

def f32(v):
    """The value a C float argument holds."""
    return float(torch.tensor(v, dtype=F32))


def seed_of(case, dtype, step=None):
    key = (case.name, dname(dtype))
    return zlib.crc32(repr(key).encode()) + (SEED_STEP.get(key, 0) if step is None else step)


def _inputs(case, dtype, step=None):
    R, C = case.R, case.C
    g = torch.Generator().manual_seed(seed_of(case, dtype, step))
    rn = lambda *shape: torch.randn(*shape, generator=g)
    std = math.sqrt(0.1) if case.eps == 0.25 else 1.0
    x = (case.mean + std * rn(R, C)).to(dtype)
    dy = rn(R, C).to(dtype)
    i = SimpleNamespace(x=x, dy=dy, eps=f32(case.eps), frac=f32(0.9), unbias=f32(R / max(R - 1, 1)))
    i.gamma, i.beta = 0.5 + torch.rand(C, generator=g), 0.5 * rn(C)
    i.x0 = torch.where(torch.rand(R, C, generator=g) < 0.1, torch.zeros_like(x), x)  # exact zeros
    i.rm0, i.rv0, i.rf0 = 0.5 * rn(C), 0.5 + torch.rand(C, generator=g), torch.tensor([2.5])
    i.grm = 3.7 * (case.mean + 0.3 * rn(C))  # running sums of a factor of 3.7
    i.grv = 3.7 * std * std * (0.5 + torch.rand(C, generator=g))
    return i


inputs = functools.lru_cache(maxsize=4)(_inputs)


# --- the oracle ------------------------------------------------------------------------------------

def _v(t, absolute=False):
    t = t.to(F64)
    return t.abs() if absolute else t


def _inv(var, eps, no_eps=False, eps_outside=False):
    if no_eps:
        return 1.0 / var.sqrt()
    if eps_outside:
        return 1.0 / (var.sqrt() + eps)
    return 1.0 / (var + eps).sqrt()


def stats64(x, eps, *, absolute=False, no_eps=False, eps_outside=False, div_rm1=False, stat_skip_last=False, **_):
    """(mean, biased variance, 1 / sqrt(var + eps)) over the rows.  Mutants: eps left out; eps added
    after the root; the variance divided by R - 1; the last row left out."""
    v = _v(x, absolute)
    if stat_skip_last and v.shape[0] > 1:
        v = v[:-1]
    n = v.shape[0]
    mean = v.mean(0)
    var = ((v - mean) ** 2).sum(0) / (max(n - 1, 1) if div_rm1 else n)
    return mean, var, _inv(var, eps, no_eps, eps_outside)


def running64(rm, rv, rf, mean, var, frac, unbias, *, absolute=False, unbias_is=None, frac_zero=False,
              no_plus_one=False, **_):
    """Caffe's update (rm', rv', rf').  Mutants: unbias replaced (by 1, by R / (R + 1)); frac taken as
    0; the factor without its + 1."""
    if unbias_is is not None:
        unbias = unbias_is
    if frac_zero:
        frac = 0.0
    rm, rv, rf, mean, var = (_v(t, absolute) for t in (rm, rv, rf, mean, var))
    return frac * rm + mean, frac * rv + unbias * var, frac * rf + (0.0 if no_plus_one else 1.0)


def coef64(mode, a, b, rf, eps, C, *, absolute=False, round32=False, no_eps=False, eps_outside=False, s_one=False,
           zero_factor_s_one=False, xor1=False, **_):
    """(mu, inv) of the three modes: BN_BATCH reads them, BN_GLOBAL scales the running sums by
    s = 0 if rf == 0 else 1 / rf, BN_NONE is (0, 1).  Mutants: the eps pair; s = 1; s = 1 where
    rf == 0; channel c reading the coefficients of c XOR 1."""
    if mode == BN_NONE:
        mu, inv = torch.zeros(C, dtype=F64), torch.ones(C, dtype=F64)
    elif mode == BN_BATCH:
        mu, inv = _v(a), _v(b)
    else:
        f = float(rf)
        s = (1.0 if zero_factor_s_one else 0.0) if f == 0 else 1.0 / f
        if s_one:
            s = 1.0
        mu = _v(a) * s
        inv = _inv(_v(b) * s + 0.0, eps, no_eps, eps_outside)
    if xor1:
        idx = (torch.arange(C) ^ 1).clamp(max=C - 1)
        mu, inv = mu[idx], inv[idx]
    if round32:
        mu, inv = mu.float().to(F64), inv.float().to(F64)
    return (mu.abs() if absolute else mu), inv


def fwd64(x, mu, inv, gamma=None, beta=None, relu=False, *, absolute=False):
    """z = gamma (x - mu) inv + beta; max(z, 0) when relu."""
    x, mu = _v(x, absolute), _v(mu, absolute)
    z = ((x + mu) if absolute else (x - mu)) * inv
    if gamma is not None:
        z = z * _v(gamma, absolute)
    if beta is not None:
        z = z + _v(beta, absolute)
    return z.clamp(min=0) if relu else z


def bwd64(dy, x, mu, inv, gamma, z, batch, *, prefill=None, absolute=False, round32=False, sum_skip_last=False,
          no_mean_term=False, no_proj_term=False, no_gamma=False, gate_dy=False, gate_ge=False, acc_as_store=False,
          **_):
    """(dx, dgamma, dbeta, c1, c2) with g = dy [z > 0] (z None: no gate; the gate is always taken
    from the signed z).  prefill: the sums are accumulated onto it.  Mutants: the last row left out
    of both sums; the sum g / R term and the xhat sum (g xhat) / R term dropped from dx; gamma left
    out of dx; the gate taken from dy, or as z >= 0; accumulate treated as store."""
    R = dy.shape[0]
    g, xv, mu = _v(dy, absolute), _v(x, absolute), _v(mu, absolute)
    if z is not None:
        gate = (_v(dy) > 0) if gate_dy else (z >= 0) if gate_ge else (z > 0)
        g = g * gate
    xhat = ((xv + mu) if absolute else (xv - mu)) * inv
    gs, gx = (g[:-1], (g * xhat)[:-1]) if sum_skip_last and R > 1 else (g, g * xhat)
    sg, sgx = gs.sum(0), gx.sum(0)
    dgamma, dbeta = sgx, sg
    if prefill is not None and not acc_as_store:
        p = abs(prefill) if absolute else prefill
        dgamma, dbeta = sgx + p, sg + p
    gi = inv if gamma is None or no_gamma else _v(gamma, absolute) * inv
    c1, c2 = sg / R, sgx / R
    if round32:
        c1, c2 = c1.float().to(F64), c2.float().to(F64)
    if not batch:
        return g * gi, dgamma, dbeta, torch.zeros_like(c1), torch.zeros_like(c2)
    t1 = 0.0 if no_mean_term else c1
    t2 = 0.0 if no_proj_term else xhat * c2
    return gi * ((g + t1 + t2) if absolute else (g - t1 - t2)), dgamma, dbeta, c1, c2


def axis64(x, s, b, A, inner, *, absolute=False, mod_index=False):
    """x s[a] + b[a] over [outer][A][inner], flat.  Mutant: the index taken as e % A."""
    v = _v(x, absolute).reshape(-1)
    e = torch.arange(v.numel())
    a = (e % A) if mod_index else (e // inner) % A
    if s is not None:
        v = v * _v(s, absolute)[a]
    if b is not None:
        v = v + _v(b, absolute)[a]
    return v


# --- one configuration of one case: every output, then its bound ---------------------------------

QUANTITIES = ("mean", "var", "inv", "rm", "rv", "rf", "y", "dgamma", "dbeta", "dgamma_acc", "dbeta_acc", "c1", "c2",
              "dx")


def evaluate(case, dtype, cfg, step=None, **mut):
    """Every output of the configuration as the oracle computes it; ``mut`` holds at most one mutant."""
    k = CONFIGS[cfg]
    i = inputs(case, dtype) if step is None else _inputs(case, dtype, step)
    o = SimpleNamespace(i=i, k=k, x=i.x0 if k.zeros else i.x)
    o.gamma, o.beta = (i.gamma if k.gamma else None), (i.beta if k.beta else None)
    if k.mode == BN_BATCH:
        o.mean, o.var, o.inv = stats64(o.x, i.eps, **mut)
        o.rm, o.rv, o.rf = running64(i.rm0, i.rv0, i.rf0, o.mean, o.var, i.frac, i.unbias, **mut)
        o.sa, o.sb, o.sf = o.mean.float(), o.inv.float(), None  # what the next kernels read
    elif k.mode == BN_GLOBAL:
        o.sa, o.sb, o.sf = i.grm, i.grv, torch.tensor([k.factor])
    else:
        o.sa = o.sb = o.sf = None
    o.mu, o.cinv = coef64(k.mode, o.sa, o.sb, o.sf, i.eps, case.C, **mut)
    o.z = fwd64(o.x, o.mu, o.cinv, o.gamma, o.beta)
    o.y = o.z.clamp(min=0) if k.relu else o.z
    gate = o.z if k.relu else None
    batch = k.mode == BN_BATCH
    o.dx, o.dgamma, o.dbeta, o.c1, o.c2 = bwd64(i.dy, o.x, o.mu, o.cinv, o.gamma, gate, batch, **mut)
    _, o.dgamma_acc, o.dbeta_acc, _, _ = bwd64(i.dy, o.x, o.mu, o.cinv, o.gamma, gate, batch, prefill=PREFILL, **mut)
    return o


def _reference(case, dtype, cfg, step=None):
    """evaluate() without a mutant, with ``bound`` (a dict over QUANTITIES, None where the
    configuration has no such output), ``bz`` (the forward bound before the store) and ``own``
    (what a forward on the statistics kernel's own output may differ by, on top)."""
    o = evaluate(case, dtype, cfg, step)
    i, k = o.i, o.k
    R, D = case.R, depth(case, dtype)
    st = 0.0 if dtype == F32 else U16  # the rounding of a stored tensor beyond fp32's
    B = dict.fromkeys(QUANTITIES)
    batch = k.mode == BN_BATCH
    if batch:
        amean = stats64(o.x, i.eps, absolute=True)[0]
        B["mean"] = 1.01 * (D + 8) * U32 * amean
        B["var"] = 1.01 * (D + 8) * U32 * (o.var * (o.var + o.mean ** 2)).sqrt()
        B["inv"] = o.inv * (0.5 * B["var"] / (o.var + i.eps) + 4 * U32)
        arm, arv, arf = running64(i.rm0, i.rv0, i.rf0, o.mean, o.var, i.frac, i.unbias, absolute=True)
        B["rm"] = 2 * U32 * arm + B["mean"]
        B["rv"] = 3 * U32 * arv + i.unbias * B["var"]
        B["rf"] = 2 * U32 * arf
    glob = k.mode == BN_GLOBAL
    d_mu = (3 * U32 if glob else 0.0) * o.mu.abs()
    d_inv = (5 * U32 if glob else 0.0) * o.cinv
    ag = o.gamma.to(F64).abs() if o.gamma is not None else torch.ones(case.C, dtype=F64)
    xc = (o.x.to(F64) - o.mu).abs()
    amu = o.mu.abs()
    o.bz = ag * (o.cinv * d_mu + xc * d_inv) + 4 * U32 * fwd64(o.x, amu, o.cinv, o.gamma, o.beta, absolute=True)
    B["y"] = o.bz + st * o.y.abs()
    if batch:  # more, for a forward on the statistics kernel's own mean / inv_std (the oracle reads their roundings)
        o.own = ag * (o.cinv * (B["mean"] + U32 * amu) + xc * (B["inv"] + U32 * o.cinv))
    gate = o.z if k.relu else None
    adx, sgx, sg, _, _ = bwd64(i.dy, o.x, amu, o.cinv, o.gamma, gate, batch, absolute=True)
    prop = (sg.new_zeros(()) if not glob else
            ((i.dy.to(F64).abs() * (gate > 0 if gate is not None else 1.0)) * (o.cinv * d_mu + xc * d_inv)).sum(0))
    B["dbeta"] = 1.01 * (D + 2) * U32 * sg
    B["dgamma"] = 1.01 * (D + 6) * U32 * sgx + prop
    B["dbeta_acc"] = 1.01 * (D + 3) * U32 * (sg + PREFILL)
    B["dgamma_acc"] = 1.01 * (D + 7) * U32 * (sgx + PREFILL) + prop
    if batch:
        B["c1"] = B["dbeta"] / R + 2 * U32 * o.c1.abs()
        B["c2"] = B["dgamma"] / R + 2 * U32 * o.c2.abs()
        xhat = xc * o.cinv
        B["dx"] = st * o.dx.abs() + 8 * U32 * adx + ag * o.cinv * (B["c1"] + xhat * B["c2"])
    else:
        B["dx"] = (st + 3 * U32) * o.dx.abs() + (i.dy.to(F64) * ag).abs() * d_inv
    o.bound = B
    return o


reference = functools.lru_cache(maxsize=2)(_reference)


def ambiguous(o):
    """Elements whose ReLU gate the kernels may take the other way: |z64| within the forward bound."""
    return int(((o.z.abs() <= o.bz) & (o.bz > 0)).sum())


def axis_inputs(outer, A, inner, dtype):
    g = torch.Generator().manual_seed(zlib.crc32(repr((outer, A, inner, dname(dtype))).encode()))
    return (torch.randn(outer, A, inner, generator=g).to(dtype), 0.5 + torch.rand(A, generator=g),
            torch.randn(A, generator=g))


def axis_bound(x, s, b, A, inner, dtype):
    ref = axis64(x, s, b, A, inner)
    return ref, (0.0 if dtype == F32 else U16) * ref.abs() + 2 * U32 * axis64(x, s, b, A, inner, absolute=True)


def worst(got, ref, bound) -> float:
    """Largest |got - ref| / bound over the elements (0 where both vanish): <= 1 passes."""
    d = (got.detach().to(F64).cpu().reshape(ref.shape) - ref).abs()
    bound = torch.as_tensor(bound, dtype=F64).expand_as(d)
    ratio = torch.where(d == 0, torch.zeros_like(d), d / bound)
    ratio = torch.where(torch.isnan(d), torch.full_like(d, math.inf), ratio)
    return float(ratio.max()) if ratio.numel() else 0.0
