"""Shared inputs, fp64 oracle, mutants and error bounds of tests/test_solver_update.py (CPU)
and tests/test_solver_update_gpu.py (csrc/kernels/solver.hip: solver_update_kernel with
chunk_grad, sumsq_pass1/2, scale_shadow).

Nothing here calls the code under test.  The oracle follows the reference's order
(caffe/src/caffe/solvers/sgd_solver.cpp ApplyUpdate: ClipGradients -> Normalize -> Regularize ->
ComputeUpdateValue -> Blob::Update, and the five sibling solvers): clip by the global L2 norm
of the raw gradient, scale by H_NORM = 1 / iter_size, add L1 / L2 decay times decay_mult, run
the rule with rate = lr * lr_mult.  It computes in fp64 on fp64 copies of the fp32 inputs and
of the fp32 hyper-parameter vector (``1 - mom2`` of the *rounded* 0.999 is what any fp32
implementation sees; in fp32 that subtraction is exact).

Inputs.  Segments of 1, 4, 63, 64, 1000, 8192, 8192 + 64 and 20000 parameters lie in one flat
buffer, each padded to a multiple of 64 as the chunk table pads it, with gaps between them.
The update covers the padded ranges; the gaps hold a sentinel in w / h0 / h1 / shadow and
must come back bitwise intact.  Hyper-parameters are chosen so that every ingredient moves
the result by far more than the tolerance (tests/test_solver_update.py proves it with the
mutants below): lr 0.1, momentum 0.9, weight decay 0.5, 1 / iter_size 0.5, momentum2 0.999,
rms_decay 0.98, Adam correction 0.7, delta 0.05, gradients of N(0, 4^2), clip at half the
gradient norm.

Error bounds (from the number formats and the summation shapes, never from a kernel output),
elementwise on each of w, h0, h1:

    |got - ref64| <= TOL * max(1, |ref64|) + (width of the oracle under the gradient error)

* ``TOL = 2e-6``.  Every output is the result of at most about a dozen fp32 roundings
  (2^-24 = 6e-8 relative each) of quantities between O(1) and O(10): the scale, the decay
  product and sum, two or three products and a sum for a history, sqrt, divide, the rate
  product and the final subtraction.  A dozen roundings of terms up to a few times the
  result: 12 * 3 * 6e-8 = 2.1e-6.  tests/test_solver_update.py measures the project's
  fp32 formula on these very inputs and requires it to stay within a quarter of the bound,
  so the bound is not tighter than fp32 allows; FMA contraction on the device removes
  roundings, it adds none.
* Clipping multiplies the gradient by ``clip / sqrt(sumsq)``; sqrt, divide and product are
  three of the dozen roundings above, the sum of squares is not.  Its summation shape
  (sumsq_pass1 with ``nparts = ceil(total / 4096)`` blocks of 256 threads, sumsq_pass2 with
  one block of 1024): 1 rounding of the square, at most 16 serial adds per thread
  (``total / (256 * nparts) <= 16``), 6 levels of the wave tree, 4 serial adds over the
  waves of the block; in pass 2 one add per thread (``nparts <= 1024``), 6 levels, 16 serial
  adds over the waves: 1 + 16 + 6 + 4 + 1 + 6 + 16 = 50 roundings on the path of any term.
  All terms are non-negative, so the sum errs by at most ``50 * 2^-24`` relative and the norm
  by half that: ``CLIP_REL = 25 * 2^-24 = 1.49e-6`` relative on the scaled gradient term.
  The bound adds the full width ``|oracle(g * (1 + CLIP_REL)) - oracle(g * (1 - CLIP_REL))|``:
  to first order twice ``CLIP_REL * |g * scale|`` times the rule's own derivative, the factor
  two covering curvature.
* Gradients summed from split-K slabs: a sum of ``splits`` fp32 terms in any order errs by at
  most ``splits * 2^-24 * sum_s |slab_s|`` (absolute, per element); it enters like the
  clipping term, as the width of the oracle under ``g +- that``.
* bf16 shadow and ``scale_shadow``: exact.  The shadow is round-to-nearest-even of the fp32
  weight that was stored, the scaled weight is the single fp32 product.
"""
import functools
import zlib

import torch

N_HYPER = 16                       # lr, mom, wd, clip, norm, delta, mom2, rms, corr; [15]: the kernel's sum of squares
KINDS = ("SGD", "Nesterov", "AdaGrad", "RMSProp", "AdaDelta", "Adam")
CHUNK = 8192                       # parameters per workgroup of the update kernel

TOL = 2e-6
CLIP_REL = 25 * 2.0 ** -24
SENSITIVITY = 500                  # a mutant must move the oracle by more than SENSITIVITY * TOL

SENTINEL = -7.25                   # exact in bf16; nothing the update produces by accident
G_STD = 4.0

HYPER = dict(lr=0.1, mom=0.9, wd=0.5, norm=0.5, delta=0.05, mom2=0.999, rms=0.98, corr=0.7)

# (count, lr_mult, decay_mult): every multiplier of {1, 2, 0.5, 0} x {1, 0, 3}; the three
# large segments carry (2, 0), (0.5, 3) and (1, 1) so each multiplier matters on > 20 %
SEGMENT_SPECS = [(1, 1.0, 1.0), (4, 2.0, 0.0), (63, 0.5, 3.0), (64, 0.0, 1.0), (1000, 0.0, 3.0),
                 (8192, 2.0, 0.0), (8192 + 64, 0.5, 3.0), (20000, 1.0, 1.0)]
GAPS = [8, 64, 4, 128, 12, 64, 20, 36, 28]      # before each segment and after the last; multiples of 4


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def padded(count):
    return -(-count // 64) * 64


def layout():
    """(segments [(offset, count, lr_mult, decay_mult)], total): 16-byte aligned offsets."""
    segs, off = [], 0
    for (cnt, lm, dm), gap in zip(SEGMENT_SPECS, GAPS):
        off += gap
        segs.append((off, cnt, lm, dm))
        off += padded(cnt)
    return segs, off + GAPS[-1]


def hyper_vector(clip=-1.0, **over):
    """The fp32 hyper-parameter vector the kernel reads (core.solver.hyper_values layout)."""
    p = dict(HYPER, **over)
    h = torch.zeros(N_HYPER, dtype=torch.float32)
    h[:9] = torch.tensor([p["lr"], p["mom"], p["wd"], clip, p["norm"], p["delta"], p["mom2"], p["rms"], p["corr"]])
    return h


class Case:
    """fp32 CPU inputs of one update; never modified (every user clones)."""

    def __init__(self, kind, segs, total, seed=0):
        self.kind, self.segs, self.total = kind, segs, total
        g = _gen("solver", kind, total, seed)
        self.upd = torch.zeros(total, dtype=torch.bool)          # what the kernel updates
        self.real = torch.zeros(total, dtype=torch.bool)         # the parameters themselves
        self.lr = torch.zeros(total)
        self.dc = torch.zeros(total)
        for off, cnt, lm, dm in segs:
            self.upd[off:off + padded(cnt)] = True
            self.real[off:off + cnt] = True
            self.lr[off:off + padded(cnt)] = lm
            self.dc[off:off + padded(cnt)] = dm
        self.gap = ~self.upd
        self.w = torch.randn(total, generator=g)
        z = torch.rand(total, generator=g)
        self.w[z < 0.03] = 0.0                                    # L1: sign(+-0) = 0
        self.w[z > 0.97] = -0.0
        # the clip norm sums the whole flat gradient, gaps included: they hold zero
        self.g = torch.randn(total, generator=g) * G_STD
        self.h0 = torch.rand(total, generator=g) + 0.1
        if kind in (0, 1):
            self.h0 -= 0.6                                        # momentum of both signs
        self.h1 = torch.rand(total, generator=g) + 0.1
        self.g[self.gap] = 0.0
        for t in (self.w, self.h0, self.h1):
            t[self.gap] = SENTINEL
        self.gnorm = float(self.g.double().square().sum().sqrt())

    def nchunks(self):
        return sum(-(-padded(cnt) // CHUNK) for _, cnt, _, _ in self.segs)

    def hyper(self, clip_mode="none", **over):
        """``half``: clip at half the gradient norm; ``above``: twice the norm (no-op);
        ``negative``: clip = -1 (disabled although the clipping instance runs)."""
        clip = {"none": -1.0, "negative": -1.0, "half": 0.5 * self.gnorm, "above": 2.0 * self.gnorm}[clip_mode]
        return hyper_vector(clip, **over)


@functools.lru_cache(maxsize=None)
def case(kind):
    segs, total = layout()
    return Case(kind, segs, total)


# --------------------------------------------------------------------------------------
# fp64 oracle and its one-ingredient-wrong variants
# --------------------------------------------------------------------------------------

MUTANTS = ("no_decay", "swap_l1_l2", "lr_mult_1", "decay_mult_1", "no_norm", "no_clip", "delta_0", "corr_1",
           "swap_mom2_rms", "h1_stale")


def mutant_applies(mutant, kind, clip):
    return {"no_clip": clip, "delta_0": kind >= 2, "corr_1": kind == 5, "swap_mom2_rms": kind in (3, 5),
            "h1_stale": kind >= 4}.get(mutant, True)


def oracle(kind, w, g, h0, h1, lr_mult, decay_mult, hyper, l1, clip, mutant=None, g_rel=0.0, g_abs=None):
    """fp64 update of flat buffers -> (w, h0, h1), inputs untouched.  ``g`` is the raw
    gradient; ``g_rel`` / ``g_abs`` perturb it after the clip norm was taken (error bounds)."""
    assert mutant is None or mutant in MUTANTS
    w, g, h0, h1 = w.double(), g.double(), h0.double(), h1.double()
    lr_mult, decay_mult = lr_mult.double(), decay_mult.double()
    lr, mom, wd, clipv, norm, delta, mom2, rms, corr = [float(v) for v in hyper.double()[:9]]
    if mutant == "no_decay":
        wd = 0.0
    if mutant == "swap_l1_l2":
        l1 = not l1
    if mutant == "lr_mult_1":
        lr_mult = torch.ones_like(lr_mult)
    if mutant == "decay_mult_1":
        decay_mult = torch.ones_like(decay_mult)
    if mutant == "no_norm":
        norm = 1.0
    if mutant == "delta_0":
        delta = 0.0
    if mutant == "corr_1":
        corr = 1.0
    if mutant == "swap_mom2_rms":
        mom2, rms = rms, mom2
    scale = norm
    if clip and mutant != "no_clip" and clipv > 0:
        l2 = float(g.square().sum().sqrt())
        if l2 > clipv:
            scale *= clipv / l2
    g = g * (1.0 + g_rel)
    if g_abs is not None:
        g = g + g_abs
    gg = g * scale + wd * decay_mult * (torch.sign(w) if l1 else w)
    rate = lr * lr_mult
    a, b = h0, h1
    if kind == 0:
        a = mom * h0 + rate * gg
        upd = a
    elif kind == 1:
        a = mom * h0 + rate * gg
        upd = (1.0 + mom) * a - mom * h0
    elif kind == 2:
        a = h0 + gg * gg
        upd = rate * gg / (a.sqrt() + delta)
    elif kind == 3:
        a = rms * h0 + (1.0 - rms) * gg * gg
        upd = rate * gg / (a.sqrt() + delta)
    elif kind == 4:
        a = mom * h0 + (1.0 - mom) * gg * gg
        u = gg * ((h1 + delta) / (a + delta)).sqrt()
        b = mom * h1 + (1.0 - mom) * u * u
        upd = rate * u
    elif kind == 5:
        a = mom * h0 + (1.0 - mom) * gg
        b = mom2 * h1 + (1.0 - mom2) * gg * gg
        if mutant == "h1_stale":
            b = h1
        upd = rate * corr * a / (b.sqrt() + delta)
    else:
        raise ValueError(kind)
    if mutant == "h1_stale":
        b = h1
    return w - upd, a, b


def case_oracle(c, hyper, l1, clip, **kw):
    return oracle(c.kind, c.w, c.g, c.h0, c.h1, c.lr, c.dc, hyper, l1, clip, **kw)


def base_bound(ref64):
    return TOL * ref64.abs().clamp(min=1.0)


def bounds(kind, w, g, h0, h1, lr_mult, decay_mult, hyper, l1, clip, g_rel=0.0, g_abs=None):
    """(refs, bounds) for w, h0, h1: ``TOL * max(1, |ref|)`` plus the width of the oracle
    under a gradient known to ``g * (1 +- g_rel) +- g_abs`` (module docstring)."""
    args = (kind, w, g, h0, h1, lr_mult, decay_mult, hyper, l1, clip)
    refs = oracle(*args)
    bnd = [base_bound(r) for r in refs]
    if g_rel or g_abs is not None:
        hi = oracle(*args, g_rel=g_rel, g_abs=g_abs)
        lo = oracle(*args, g_rel=-g_rel, g_abs=None if g_abs is None else -g_abs)
        bnd = [b + (h - l).abs() for b, h, l in zip(bnd, hi, lo)]
    return refs, bnd


def case_bounds(c, hyper, l1, clip, clipped):
    """``clipped``: whether the clip actually scales (the summation error of the norm enters)."""
    return bounds(c.kind, c.w, c.g, c.h0, c.h1, c.lr, c.dc, hyper, l1, clip, g_rel=CLIP_REL if clipped else 0.0)


def moved_fraction(mut, ref, mask):
    """Largest share, over the outputs, of the masked elements that a mutant moves by more
    than SENSITIVITY * TOL * max(1, |ref|)."""
    best = 0.0
    for m, r in zip(mut, ref):
        far = (m - r).abs() > SENSITIVITY * TOL * r.abs().clamp(min=1.0)
        best = max(best, float(far[mask].double().mean()))
    return best


# --------------------------------------------------------------------------------------
# split-K slabs (the weight gradient of a grouped convolution before its reduce)
# --------------------------------------------------------------------------------------

SPLITS = (1, 2, 3, 4, 5, 7, 15, 16, 17, 31, 63, 64, 65, 80, 128, 130)
SLAB_G, SLAB_M, SLAB_N, SLAB_LDW = 2, 8, 72, 80       # ones (bias) column at SLAB_N
SLAB_OFF_W, SLAB_OFF_B, SLAB_OFF_F, SLAB_FLAT, SLAB_TOTAL = 16, 1232, 1344, 100, 1536


class SlabCase:
    """A weight [G * M, N] and a bias [G * M] whose gradients are ``splits`` fp32 slabs
    ``ws[G][splits][M][ldw]`` (bias in column N, junk in the padding columns), and one
    ordinary flat-gradient segment of 100 parameters, in a flat buffer with sentinel gaps."""

    def __init__(self, kind, splits):
        G, M, N, ldw = SLAB_G, SLAB_M, SLAB_N, SLAB_LDW
        self.kind, self.splits, self.total = kind, splits, SLAB_TOTAL
        self.segs = [(SLAB_OFF_W, G * M * N, 1.0, 1.0), (SLAB_OFF_B, G * M, 2.0, 0.0),
                     (SLAB_OFF_F, SLAB_FLAT, 0.5, 3.0)]
        g = _gen("slab", kind, splits)
        # terms of mixed magnitude and sign: the summation order shows in the last bits
        # (scaled so that the summed gradient stays near G_STD at every split count)
        self.ws = (torch.randn(G, splits, M, ldw, generator=g) * torch.rand(G, splits, M, ldw, generator=g)
                   * (2 * G_STD / splits ** 0.5))
        w64 = self.ws.double().sum(1)
        a64 = self.ws.double().abs().sum(1)
        t = self.total
        self.upd = torch.zeros(t, dtype=torch.bool)              # slab chunks are not padded
        self.lr, self.dc = torch.zeros(t), torch.zeros(t)
        for (off, cnt, lm, dm), pad in zip(self.segs, (False, False, True)):
            n = padded(cnt) if pad else cnt
            self.upd[off:off + n] = True
            self.lr[off:off + n] = lm
            self.dc[off:off + n] = dm
        self.gap = ~self.upd
        self.slab = torch.zeros(t, dtype=torch.bool)
        self.slab[SLAB_OFF_W:SLAB_OFF_W + G * M * N] = True
        self.slab[SLAB_OFF_B:SLAB_OFF_B + G * M] = True
        self.w = torch.randn(t, generator=g)
        self.h0 = torch.rand(t, generator=g) + 0.1 - (0.6 if kind in (0, 1) else 0.0)
        self.h1 = torch.rand(t, generator=g) + 0.1
        self.g = torch.randn(t, generator=g) * G_STD             # read on the flat segment alone
        self.g[self.gap] = 0.0
        for x in (self.w, self.h0, self.h1):
            x[self.gap] = SENTINEL
        # fp64 sum of the slabs laid out as the flat gradient, and the summation error bound
        self.g64 = self.g.double()
        self.g_abs = torch.zeros(t, dtype=torch.float64)
        self.g64[SLAB_OFF_W:SLAB_OFF_W + G * M * N] = w64[:, :, :N].reshape(-1)
        self.g64[SLAB_OFF_B:SLAB_OFF_B + G * M] = w64[:, :, N].reshape(-1)
        self.g_abs[SLAB_OFF_W:SLAB_OFF_W + G * M * N] = a64[:, :, :N].reshape(-1)
        self.g_abs[SLAB_OFF_B:SLAB_OFF_B + G * M] = a64[:, :, N].reshape(-1)
        self.g_abs *= splits * 2.0 ** -24

    def hyper(self):
        return hyper_vector(-1.0)

    def slab_chunks(self, base):
        """{segment offset: [(flat start, count, slab byte address, slab stride, splits,
        element stride)]} for slabs at byte address ``base``: one chunk per weight row,
        one strided chunk per group for the bias column (engine._SlabGrad.chunks)."""
        G, M, N, ldw, S = SLAB_G, SLAB_M, SLAB_N, SLAB_LDW, self.splits
        ss, gs = M * ldw, S * M * ldw
        return {SLAB_OFF_W: [(SLAB_OFF_W + (g * M + m) * N, N, base + 4 * (g * gs + m * ldw), ss, S, 1)
                             for g in range(G) for m in range(M)],
                SLAB_OFF_B: [(SLAB_OFF_B + g * M, M, base + 4 * (g * gs + N), ss, S, ldw) for g in range(G)]}

    def bounds(self, hyper, l1=False):
        return bounds(self.kind, self.w, self.g64, self.h0, self.h1, self.lr, self.dc, hyper, l1, False,
                      g_abs=self.g_abs)


@functools.lru_cache(maxsize=None)
def slab_case(kind, splits):
    return SlabCase(kind, splits)


# --------------------------------------------------------------------------------------
# scale_shadow
# --------------------------------------------------------------------------------------

SCALE_NS = (1, 3, 4, 5, 1023, 4099)


def bf16_edge_vector():
    """fp32 values halfway between two bf16 neighbours (low 16 bits 0x8000) with bit 16 clear
    and set (round-to-nearest-even goes down / up), both signs, several exponents, a carry
    into the exponent, the largest finite value (rounds to inf), denormals; +-0, +-inf."""
    bits = []
    for hi in (0x3F80, 0x3F81, 0x4000, 0x4001, 0x0080, 0x0081, 0x7F7E, 0x7F7D, 0x3FFF, 0x3FFE, 0x7F7F, 0x3F00,
               0x0000, 0x0001):
        for sign in (0, 0x8000):
            bits.append(((hi | sign) << 16) | 0x8000)
    bits += [0x00000000, 0x80000000, 0x7F800000, 0xFF800000]
    t = torch.tensor(bits, dtype=torch.int64)
    t = torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32)
    return t.view(torch.float32)
