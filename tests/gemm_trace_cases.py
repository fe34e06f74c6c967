"""Cases and recorder of tests/test_gemm_launch_trace.py: which native launches, with which arguments,
ops.gemm issues for a product.

Everything between ``gemm()``'s keywords and the ``SnGemmArgs`` handed to the kernel library is plain
Python, so with ``_lib.kernels`` / ``_lib.stream_ptr`` / ``_lib.call`` replaced and CPU bf16 / uint8 /
fp32 tensors as operands it runs anywhere in milliseconds.  A trace is the ordered list of what one
case did:

* ``["sn_gemm", {field: value}]``: every field of the SnGemmArgs (both SnOperands included, their
  geometry as the list of SnConvGeom's fields); a field that is 0 / null is left out;
* ``[kernel, arg, ...]`` for a ``_lib.call`` (splitk_reduce, colsum_bf16, fp8_fold_amax);
* ``["raise", text]`` for an assertion of the front-end, ``["result", ...]`` for what a helper
  returned or left behind, ``["sink.*", ...]`` for the defer_reduce protocol, ``["side", ...]`` for
  an Fp8Side's state after its block;
* last, ``["misses", [...]]``: the tune keys (as strings) the case left in ``tune_misses()``.

A pointer is ``"buffer+byte offset"``: the buffer is the name of the operand whose storage it lies
in (x, w, y, ...) or ``t<n>`` for the n-th temporary in order of first appearance.  Never a raw
address.  (ops.gemm sees a ``torch`` whose ``empty`` / ``zeros`` keep what they return alive and
zero it, so that an address names one buffer for the whole case and the torch fallbacks compute on
defined values.)

``python tests/gemm_trace_cases.py`` rewrites the fixture, tests/gemm_launch_trace.json.  The
committed fixture was written by this module at the commit BEFORE ops.gemm described a launch by a
typed GemmCall: the module only goes through what both sides have (``gemm()`` and the helpers
around it), except ``_cands``, which calls the candidate lists with that commit's positional
signature when there is no GemmCall.
"""
import contextlib
import ctypes as C
import json
import pathlib
import sys

import torch

if __name__ == "__main__":  # under pytest, tests/conftest.py has done this
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
from sparknet_amd.ops import _lib, gemm as G

FIXTURE = pathlib.Path(__file__).with_name("gemm_launch_trace.json")
DB = pathlib.Path(G.__file__).with_name("gemm_tuned.json")
BF16, U8, F32 = torch.bfloat16, torch.uint8, torch.float32
STREAM = 0x5EA0  # what _lib.stream_ptr() answers; sn_gemm must be handed exactly this
SLAB_FIELDS = ("ws", "splits", "M", "N", "ldw", "groups", "ones", "ldc", "c_gstride")


class _Torch:
    """The ``torch`` of ops.gemm while a case runs (see the module docstring)."""

    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, name):
        fn = getattr(torch, name)
        if name not in ("empty", "zeros", "empty_like", "zeros_like"):
            return fn
        fn = getattr(torch, name.replace("empty", "zeros"))

        def alloc(*a, **k):
            t = fn(*a, **k)
            self._rec.own(t)
            return t
        return alloc


class Kernels:
    """Stands for libsn_kernels.so."""

    def __init__(self, rec):
        self.rec = rec

    def sn_gemm(self, args, stream):
        assert stream.value == STREAM, stream
        self.rec.trace.append(["sn_gemm", self.rec.struct(args._obj)])
        return 0


class Recorder:
    def __init__(self):
        self.trace = []
        self.bufs = []  # [first byte, past the last, name or None, storage (kept alive)]

    def own(self, t, name=None):
        """Know ``t``'s storage as ``name`` (None: a temporary, numbered when a launch first uses it)."""
        st = t.untyped_storage()
        if st.nbytes() == 0:
            return t
        for b in self.bufs:
            if b[0] == st.data_ptr():
                b[2] = name or b[2]
                return t
        self.bufs.append([st.data_ptr(), st.data_ptr() + st.nbytes(), name, st])
        return t

    def buf(self, name, *shape, dtype=BF16, fill=0):
        return self.own(torch.full(shape, fill, dtype=dtype), name)

    def ptr(self, addr):
        if isinstance(addr, torch.Tensor):
            addr = addr.data_ptr()
        if not addr:
            return 0
        for b in self.bufs:
            if b[0] <= addr < b[1]:
                if b[2] is None:
                    b[2] = f"t{sum(o[2] is not None and o[2][0] == 't' and o[2][1:].isdigit() for o in self.bufs)}"
                return f"{b[2]}+{addr - b[0]}"
        raise LookupError(f"address {addr:#x} lies in no known buffer")

    def struct(self, s):
        out = {}
        for f, typ in s._fields_:
            v = getattr(s, f)
            if isinstance(v, _lib.SnConvGeom):
                v = [getattr(v, g) for g, _ in v._fields_]
                v = v if any(v) else 0
            elif isinstance(v, C.Structure):
                v = self.struct(v)
            elif typ is C.c_void_p:
                v = self.ptr(v)
            if v:
                out[f] = v
        return out

    def arg(self, v):
        if isinstance(v, torch.Tensor):
            return self.ptr(v)
        if isinstance(v, C.c_void_p):
            return self.ptr(v.value)
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        raise TypeError(f"launch argument {v!r}")

    def call(self, kernel, *args):
        self.trace.append([kernel, *map(self.arg, args)])

    def result(self, what, v):
        if isinstance(v, torch.Tensor):
            v = f"{self.ptr(v)}:{str(v.dtype)[6:]}{list(v.shape)}/{list(v.stride())}".replace(" ", "")
        self.trace.append(["result", what, v])

    def raises(self, fn, *a, **k):
        try:
            fn(*a, **k)
        except AssertionError as e:
            self.trace.append(["raise", str(e)])
        else:
            self.trace.append(["raise", None])

    def side(self, side):
        self.trace.append(["side", {"ok": side.ok, "launches": side.launches, "complete": side.complete}])


@contextlib.contextmanager
def patch(**attrs):
    saved = {k: getattr(G, k) for k in attrs}
    try:
        for k, v in attrs.items():
            setattr(G, k, v)
        yield
    finally:
        for k, v in saved.items():
            setattr(G, k, v)


@contextlib.contextmanager
def recording(rec):
    """ops.gemm with its import-time switches at their defaults, an empty tuning cache, and the native
    library replaced by ``rec``."""
    lib = {"kernels": lambda: Kernels(rec), "stream_ptr": lambda device=None: STREAM, "call": rec.call,
           "DEBUG_SYNC": False}
    saved = {k: getattr(_lib, k) for k in lib}
    try:
        for k, v in lib.items():
            setattr(_lib, k, v)
        with patch(torch=_Torch(rec), _FORCE_TILE=-1, _AUTOTUNE=False, _THIN=True, _LDS_EPI=True, _SIDE_FRAG=True,
                   _TUNED={}, _MISSES=set(), _SIDE=None, _DEFER_SINK=None, SIDE_STATS={"used": 0, "missed": 0}):
            yield
    finally:
        for k, v in saved.items():
            setattr(_lib, k, v)


CASES = {}


def case(name):
    def add(fn):
        assert name not in CASES, name
        CASES[name] = fn
        return fn
    return add


def run(name) -> list:
    rec = Recorder()
    with recording(rec):
        CASES[name](rec)
        rec.trace.append(["misses", [G._key_to_str(k) for k in G.tune_misses()]])
    return rec.trace


# --- the dense helpers -------------------------------------------------------------------------

def _xwb(rec, M, N, K):
    return rec.buf("x", M, K), rec.buf("w", N, K), rec.buf("b", N, dtype=F32)


def _dense(rec, M, N, K, **kw):
    """gemm() of x [M, K] and w [N, K] into a bf16 y [M, N]."""
    x, w = rec.buf("x", M, K), rec.buf("w", N, K)
    y = kw.pop("y", None)
    if y is None:
        y = rec.buf("y", M, N)
    G.gemm(M, N, K, G.Dense(x, K, True), G.Dense(w, K, True), y, y.stride(0), epi=kw.pop("epi", G.EPI_BF16), **kw)


@case("linear_fwd 64x10x4096: split-K reduce, bias, relu")
def _(rec):
    x, w, b = _xwb(rec, 64, 10, 4096)
    rec.result("y", G.linear_fwd(x, w, b, relu=True))


@case("linear_fwd 77x96x368, x a column slice: one _pad8 copy")
def _(rec):
    _, w, b = _xwb(rec, 77, 96, 368)
    rec.result("y", G.linear_fwd(rec.buf("x_wide", 77, 400)[:, :368], w, b, relu=True))


@case("linear_fwd 77x96x363, K % 8: both _pad8 copies")
def _(rec):
    x, w, b = _xwb(rec, 77, 96, 363)
    rec.result("y", G.linear_fwd(x, w, b, relu=True, out=rec.buf("y", 77, 96)))


@case("linear_fwd dropout, unsplit")
def _(rec):
    x, w, b = _xwb(rec, 64, 96, 64)
    rec.result("y", G.linear_fwd(x, w, b, relu=True, dropout=(rec.buf("rng", 2, dtype=torch.int64), 7, 0.25)))


@case("gemm dropout, splits=3: dropout in splitk_reduce")
def _(rec):
    _dense(rec, 64, 96, 512, bias=rec.buf("b", 96, dtype=F32), relu=True, splits=3,
           dropout=(rec.buf("rng", 2, dtype=torch.int64), 9, 0.5))


@case("linear_dgrad plain")
def _(rec):
    rec.result("dx", G.linear_dgrad(rec.buf("dy", 40, 24), rec.buf("w", 24, 64)))


@case("linear_dgrad gate, gate_scale")
def _(rec):
    rec.result("dx", G.linear_dgrad(rec.buf("dy", 40, 24), rec.buf("w", 24, 64), gate=rec.buf("gate", 40, 64),
                                    gate_scale=2.0))


@case("linear_dgrad K % 8 with a gate: torch fallback")
def _(rec):
    dx = G.linear_dgrad(rec.buf("dy", 40, 24), rec.buf("w", 24, 60), gate=rec.buf("gate", 40, 60, fill=1),
                        gate_scale=2.0)
    rec.trace.append(["result", "dx", list(dx.shape), float(dx.float().sum())])
    out = rec.buf("dx", 40, 60, fill=1)
    got = G.linear_dgrad(rec.buf("dy", 40, 24), rec.buf("w", 24, 60), out=out, gate=rec.buf("gate", 40, 60, fill=1))
    rec.trace.append(["result", "dx", got is out, float(out.float().sum())])


@case("linear_dgrad out= given, padding needed")
def _(rec):
    out = rec.buf("dx", 40, 60, fill=1)
    got = G.linear_dgrad(rec.buf("dy", 40, 20), rec.buf("w", 20, 60), out=out)
    rec.trace.append(["result", "dx", got is out, float(out.float().sum())])
    out = rec.buf("dx2", 40, 64, fill=1)
    got = G.linear_dgrad(rec.buf("dy", 40, 20), rec.buf("w2", 20, 64), out=out)  # only dy and w are padded
    rec.trace.append(["result", "dx2", got is out, float(out.float().sum())])


def _wgrad(rec, M, N, K):
    return (rec.buf("dy", M, N), rec.buf("x", M, K), rec.buf("dw", N, K, dtype=F32, fill=1),
            rec.buf("db", N, dtype=F32, fill=1))


@case("linear_wgrad fused db: accumulate / overwrite, odd-N slabs")
def _(rec):
    dy, x, dw, db = _wgrad(rec, 4096, 64, 96)
    rec.result("fused", G.linear_wgrad(dy, x, dw, accumulate=True, db=db, db_acc=False))
    rec.result("fused", G.linear_wgrad(dy, x, dw, accumulate=False, db=db, db_acc=True))
    rec.result("fused", G.linear_wgrad(dy, x, dw, accumulate=False))
    rec.result("fused", G.linear_wgrad(dy, x, dw, db=db.double()))


@case("linear_wgrad N % 8: temporary, add_ / copy_")
def _(rec):
    dy, x, dw, db = _wgrad(rec, 512, 60, 96)
    rec.result("fused", G.linear_wgrad(dy, x, dw, accumulate=True, db=db))
    rec.result("dw sum", float(dw.sum()))
    rec.result("fused", G.linear_wgrad(dy, x, dw, accumulate=False, db=db))
    rec.result("dw sum", float(dw.sum()))


def _sgd(rec, N, K):
    return {"w": rec.buf("sgd.w", N, K, dtype=F32), "h": rec.buf("sgd.h", N, K, dtype=F32),
            "shadow": rec.buf("sgd.shadow", N, K), "hyper": rec.buf("sgd.hyper", 8, dtype=F32),
            "lr_mult": 1.5, "decay_mult": 0.25, "flags": 5}


@case("linear_wgrad_sgd: EPI_SGD, unsplit, no miss")
def _(rec):
    dy, x, _, db = _wgrad(rec, 8192, 64, 96)
    rec.result("fused", G.linear_wgrad_sgd(dy, x, _sgd(rec, 64, 96), db=db, db_acc=False))
    rec.result("fused", G.linear_wgrad_sgd(dy, x, _sgd(rec, 64, 96)))
    with patch(_FORCE_TILE=10):  # not an EPI_SGD tile: 0
        rec.result("fused", G.linear_wgrad_sgd(dy, x, _sgd(rec, 64, 96), db=db))
    with patch(_FORCE_TILE=3):
        rec.result("fused", G.linear_wgrad_sgd(dy, x, _sgd(rec, 64, 96), db=db))


@case("colsum 5000x96, 77x13")
def _(rec):
    G.colsum(rec.buf("x", 5000, 96), rec.buf("out", 96, dtype=F32))
    G.colsum(rec.buf("x2", 80, 16)[:77, :13], rec.buf("out2", 13, dtype=F32), accumulate=False)


@case("M == 0 or N == 0: no launch")
def _(rec):
    y = G.linear_fwd(torch.zeros((0, 64), dtype=BF16), rec.buf("w", 8, 64))
    rec.result("y shape", list(y.shape))
    _dense(rec, 8, 0, 64, y=rec.buf("y", 8, 8))


# --- operands ------------------------------------------------------------------------------------

def _conv_fwd(rec, x, ctot):
    """A grouped 3x3 convolution, 2 x 6 x 6 x 32 -> 64 in two groups, as ops.hip launches it."""
    geom = G.ConvGeom(2, 6, 6, ctot, 6, 6, 3, 3, 1, 1, 1, 1, 1, 1, 16)
    w, y = rec.buf("w", 64, 144), rec.buf("y", 2, 6, 6, 64)
    G.gemm(72, 32, 144, G.Im2col(x, geom, True, gstride=16), G.Dense(w, 144, True, gstride=32 * 144), y, 64,
           epi=G.EPI_BF16, groups=2, c_gstride=32, bias=rec.buf("b", 64, dtype=F32), relu=True)


@case("grouped Im2col x Dense, c_gstride")
def _(rec):
    _conv_fwd(rec, rec.buf("x", 2, 6, 6, 32), 32)


@case("Im2col on a channel slice")
def _(rec):
    _conv_fwd(rec, rec.buf("x", 2, 6, 6, 80)[..., 16:48], 80)


@case("Im2col MC x Dense MC: grouped weight gradient, bias column, c_gstride")
def _(rec):
    geom = G.ConvGeom(2, 6, 6, 32, 6, 6, 3, 3, 1, 1, 1, 1, 1, 1, 16)
    G.gemm(32, 144, 72, G.Dense(rec.buf("dy", 72, 64), 64, False, gstride=32),
           G.Im2col(rec.buf("x", 2, 6, 6, 32), geom, False, gstride=16), rec.buf("dw", 64, 144, dtype=F32), 144,
           epi=G.EPI_F32_ACC, groups=2, c_gstride=32 * 144, bias_grad=rec.buf("db", 64, dtype=F32), bias_acc=True)


@case("FlipW dgrad, gate")
def _(rec):
    g2 = G.ConvGeom(2, 6, 6, 64, 6, 6, 3, 3, 1, 1, 1, 1, 1, 1, 32)
    G.gemm(72, 16, 288, G.Im2col(rec.buf("dy", 2, 6, 6, 64), g2, True, gstride=32),
           G.FlipW(rec.buf("w", 64, 3, 3, 16), 32, 3, 3, 16), rec.buf("dx", 2, 6, 6, 32), 32, epi=G.EPI_BF16, groups=2,
           c_gstride=16, gate=rec.buf("gate", 2, 6, 6, 32))


@case("_operand refuses")
def _(rec):
    y, w = rec.buf("y", 64, 64), G.Dense(rec.buf("w", 64, 64), 64, True)
    x = rec.buf("x", 2, 4, 4, 64)

    def geom(**kw):
        return G.ConvGeom(**{**dict(N=2, H=4, W=4, C=64, P=4, Q=4, R=1, S=1, Cg=64), **kw})

    def refuse(A, B=w, **kw):
        rec.raises(G.gemm, 64, 64, 64, A, B, y, 64, **{"epi": G.EPI_BF16, **kw})
    refuse(G.Dense(rec.buf("x2", 65, 64).view(-1)[1:4097].view(64, 64), 64, True))  # pointer
    refuse(G.Dense(rec.buf("x3", 64, 60), 60, True))                                # leading dimension
    refuse(G.Dense(rec.buf("x4", 64, 64, dtype=F32), 64, True))                     # dtype
    refuse(G.Dense(rec.buf("x5", 64, 64), 64, True), deq=(rec.buf("da", 1, dtype=F32), rec.buf("db", 1, dtype=F32)))
    refuse(G.Im2col(rec.buf("x6", 2, 4, 4, 64, dtype=F32), geom(), True))
    refuse(G.Im2col(x.permute(0, 2, 1, 3), geom(), True))                           # not NHWC
    refuse(G.Im2col(rec.buf("x7", 2, 4, 4, 80)[..., :64], geom(C=72), True))        # slice, wrong pixel stride
    refuse(G.Im2col(x, geom(Cg=60), True))
    refuse(G.Im2col(x, geom(C=68), True))
    refuse(G.Im2col(rec.buf("xq", 2, 4, 4, 64, dtype=U8), geom(Cg=24), True),       # fp8: channels % 16
           deq=(rec.buf("da", 1, dtype=F32), rec.buf("db", 1, dtype=F32)))
    refuse(G.Im2col(x, geom(N=1 << 12, P=64, Q=64), True))                          # 2^24 output pixels
    refuse(G.Im2col(x, geom(N=1 << 12, H=64, W=64), True))                          # 2^24 input pixels
    refuse(G.Im2col(x, geom(N=1 << 11, H=64, W=64, C=256), True))                   # 2^31 elements
    refuse(G.Im2col(x, geom(N=1 << 11, H=64, W=64, C=248), True))                   # just below: launches
    refuse(G.Im2col(rec.buf("x8", 2 * 4 * 4 * 64 + 8)[4:2052].view(2, 4, 4, 64), geom(), True))  # pointer
    refuse(w, G.FlipW(rec.buf("w2", 64, 1, 1, 12), 64, 1, 1, 12))
    refuse(w, G.FlipW(rec.buf("w3", 64, 1, 1, 16, dtype=F32), 64, 1, 1, 16))
    # bias_grad: a K-contiguous B, the wrong length
    refuse(w, bias_grad=rec.buf("bg", 64, dtype=F32), epi=G.EPI_F32)
    refuse(G.Dense(rec.buf("x5", 64, 64), 64, False), G.Dense(rec.buf("w", 64, 64), 64, False),
           bias_grad=rec.buf("bg2", 63, dtype=F32), epi=G.EPI_F32)
    refuse(w, bias=rec.buf("bb", 64))
    refuse(w, gate=rec.buf("gate", 64, 64), epi=G.EPI_F32)
    refuse(w, dropout=(rec.buf("rng", 2, dtype=torch.int64), 1, 0.5), epi=G.EPI_F32)
    refuse(w, epi=G.EPI_SGD)


# --- fp8 -----------------------------------------------------------------------------------------

def _deq(rec):
    return rec.buf("deq_a", 1, dtype=F32), rec.buf("deq_b", 1, dtype=F32)


def _fp8(rec, M, N, K, deq, kc=True, **kw):
    xq = rec.buf("xq", *((M, K) if kc else (K, M)), dtype=U8)
    wq = rec.buf("wq", *((N, K) if kc else (K, N)), dtype=U8)
    y = rec.buf("y", M, N, dtype=kw.pop("dtype", BF16))
    G.gemm(M, N, K, G.Dense(xq, K if kc else M, kc), G.Dense(wq, K if kc else N, kc), y, N,
           epi=kw.pop("epi", G.EPI_BF16), deq=deq, **kw)


@case("fp8 deq 2-tuple, 3-tuples of either format: one key for format 1")
def _(rec):
    da, db = _deq(rec)
    b = rec.buf("b", 64, dtype=F32)
    _fp8(rec, 128, 64, 256, (da, db), bias=b, relu=True)
    _fp8(rec, 128, 64, 256, (da, db, 1), bias=b, relu=True)
    _fp8(rec, 128, 64, 256, (da, db, 2), bias=b, relu=True)


@case("fp8 dropout, gate")
def _(rec):
    _fp8(rec, 128, 64, 256, _deq(rec), dropout=(rec.buf("rng", 2, dtype=torch.int64), 3, 0.5))
    _fp8(rec, 128, 64, 256, _deq(rec), gate=rec.buf("gate", 128, 64), gate_scale=4.0)


@case("fp8 MC weight gradient, bias_grad, N % 16")
def _(rec):
    db = rec.buf("db", 64, dtype=F32)
    _fp8(rec, 64, 32, 16384, (*_deq(rec), 2), kc=False, epi=G.EPI_F32, dtype=F32, bias_grad=db, bias_acc=False)
    _fp8(rec, 64, 32, 256, (*_deq(rec), 2), kc=False, epi=G.EPI_F32_ACC, dtype=F32, bias_grad=db)
    rec.raises(_fp8, rec, 64, 24, 256, _deq(rec), kc=False, epi=G.EPI_F32, dtype=F32, bias_grad=db)


@case("fp8 kchunk: multiples of 128")
def _(rec):
    _fp8(rec, 128, 128, 16384, _deq(rec))
    _fp8(rec, 128, 128, 1024, _deq(rec), splits=3)
    _fp8(rec, 128, 128, 1024, _deq(rec), splits=1)
    _fp8(rec, 128, 128, 64, _deq(rec), splits=1)  # K below one K-step: kchunk 128


@case("fp8 _FORCE_TILE")
def _(rec):
    for tile in (11, 16, 3):
        with patch(_FORCE_TILE=tile):
            _fp8(rec, 256, 256, 4096, _deq(rec))                                # K-contiguous: 11 and 16 kept
            _fp8(rec, 256, 256, 4096, _deq(rec), kc=False, epi=G.EPI_F32, dtype=F32)  # MC: tile 0


# --- the choice of tile and splits ---------------------------------------------------------------

@case("splits forced: 1, 3, 100")
def _(rec):
    for splits in (1, 3, 100):
        _dense(rec, 96, 200, 1000, splits=splits, bias=rec.buf("b", 200, dtype=F32))
    _dense(rec, 96, 200, 1000, splits=3, epi=G.EPI_F32, y=rec.buf("yf", 96, 200, dtype=F32))
    _dense(rec, 96, 200, 1000, splits=3, epi=G.EPI_F32_ACC, y=rec.buf("yf", 96, 200, dtype=F32))


@case("_FORCE_TILE: every tile")
def _(rec):
    for tile in G.TILES:
        with patch(_FORCE_TILE=tile):
            _dense(rec, 300, 200, 1024)


def _from_key(rec, key):
    """Run the product that the tune key ``key`` (of Dense operands) describes."""
    M, N, K, groups, a_mc, a_mode, b_mc, b_mode, epi, gate, bias_grad, drop, ga, gb = key[:14]
    assert (a_mode, b_mode, groups, gate, bias_grad) == (0, 0, 1, False, False) and key[14:-1] in ((), ("fp8",)), key
    fp8 = key[14:-1] == ("fp8",)
    a = rec.buf("a", *((K, M) if a_mc else (M, K)), dtype=U8 if fp8 else BF16)
    b = rec.buf("b", *((K, N) if b_mc else (N, K)), dtype=U8 if fp8 else BF16)
    G.gemm(M, N, K, G.Dense(a, ga[0], not a_mc), G.Dense(b, gb[0], not b_mc), rec.buf("out", M, N, dtype=key[-1]), N,
           epi=epi, deq=_deq(rec) if fp8 else None,
           dropout=(rec.buf("rng", 2, dtype=torch.int64), 1, 0.5) if drop else None)


DB_KEYS = (
    "(100, 10, 1024, 1, 0, 0, 0, 0, 0, False, False, False, (1024, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), "
    "(1024, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), 'bfloat16')",
    "(128, 1024, 2048, 1, 0, 0, 0, 0, 0, False, False, True, (2048, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), "
    "(2048, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), 'bfloat16')",
    "(2048, 1000, 4096, 1, 0, 0, 0, 0, 0, False, False, False, (4096, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), "
    "(4096, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), 'fp8', 'bfloat16')",
)


@case("database hits: no miss; the same products on the cost model")
def _(rec):
    db = json.loads(DB.read_text())
    for ks in DB_KEYS:
        key = G._key_from_str(ks)
        with patch(_TUNED={key: tuple(db[ks])}):
            _from_key(rec, key)
        rec.result("misses so far", len(G.tune_misses()))
        _from_key(rec, key)
        rec.result("misses so far", len(G.tune_misses()))


# --- derived fields ------------------------------------------------------------------------------

@case("raster_n: 1 < tn <= 8 and tm >= 8 tn")
def _(rec):
    for M, N in ((2048, 200), (1920, 200), (2048, 128), (8192, 1025), (9216, 1025)):
        _dense(rec, M, N, 64, splits=1)


@case("lds_store")
def _(rec):
    _dense(rec, 64, 128, 64)                                                     # tile 0, ldc % 8 == 0: on
    _dense(rec, 64, 128, 64, y=rec.buf("y_wide", 64, 132)[:, :128])              # ldc % 8
    _dense(rec, 64, 128, 64, y=rec.buf("y_flat", 64 * 128 + 8)[4:-4].view(64, 128))  # out not 16-B aligned
    _dense(rec, 64, 128, 64, epi=G.EPI_F32, y=rec.buf("yf", 64, 128, dtype=F32))
    with patch(_FORCE_TILE=2):                                                   # not an LDS-epilogue tile
        _dense(rec, 64, 128, 64)
    with patch(_LDS_EPI=False):
        _dense(rec, 64, 128, 64)
    geom = G.ConvGeom(2, 6, 6, 32, 6, 6, 3, 3, 1, 1, 1, 1, 1, 1, 16)              # c_gstride % 8
    G.gemm(72, 12, 144, G.Im2col(rec.buf("xc", 2, 6, 6, 32), geom, True, gstride=16),
           G.Dense(rec.buf("wc", 24, 144), 144, True, gstride=12 * 144), rec.buf("yc", 72, 24), 24, epi=G.EPI_BF16,
           groups=2, c_gstride=12)


# --- Fp8Side -------------------------------------------------------------------------------------

def _side(rec, base, **kw):
    side = G.Fp8Side(base, rec.buf("slot", 4, dtype=F32), part=rec.buf("part", 8, dtype=F32), **kw)
    rec.own(side.q, "side.q")
    return side


@case("Fp8Side: covered unsplit launches store, then fold")
def _(rec):
    base = rec.buf("base", 128, 64)
    with G.fp8_side_output(_side(rec, base)) as side:
        assert G._SIDE is side
        _dense(rec, 64, 64, 64, y=base[:64])
        _dense(rec, 64, 64, 64, y=base[64:])  # at an offset inside base
        _dense(rec, 64, 64, 64)               # not covered: left alone
        rec.side(side)
    assert G._SIDE is None
    rec.side(side)
    rec.result("matches", [side.matches(base), side.matches(base[:64]), side.covers(base[64:]),
                           side.covers(base.view(torch.int16))])


@case("Fp8Side: e5m2, its own partials, dropout epilogue, a grouped output")
def _(rec):
    base = rec.buf("base", 72, 64)
    side = G.Fp8Side(base, rec.buf("slot", 4, dtype=F32), e5m2=True)
    rec.own(side.q, "side.q")
    rec.own(side.part, "side.part")
    rec.result("part", list(side.part.shape))
    with G.fp8_side_output(side):
        _dense(rec, 72, 64, 64, y=base, dropout=(rec.buf("rng", 2, dtype=torch.int64), 2, 0.5))
        _conv_fwd(rec, rec.buf("xc", 2, 6, 6, 32), 32)  # y is not covered
        geom = G.ConvGeom(2, 6, 6, 32, 6, 6, 3, 3, 1, 1, 1, 1, 1, 1, 16)
        G.gemm(72, 32, 144, G.Im2col(rec.buf("xc", 2, 6, 6, 32), geom, True, gstride=16),
               G.Dense(rec.buf("w", 64, 144), 144, True, gstride=32 * 144), base, 64, epi=G.EPI_BF16, groups=2,
               c_gstride=32)
    rec.side(side)


def _refusal(rec, base, y, M, N, K, **kw):
    with G.fp8_side_output(_side(rec, base)) as side:
        _dense(rec, M, N, K, y=y, **kw)
    rec.side(side)  # nothing stored: no fp8_fold_amax before this line


@case("Fp8Side refuses: split-K")
def _(rec):
    base = rec.buf("base", 64, 64)
    _refusal(rec, base, base, 64, 64, 512, splits=2)


@case("Fp8Side refuses: tiles 6 and 7")
def _(rec):
    base = rec.buf("base", 64, 64)
    for tile in (6, 7):
        with patch(_FORCE_TILE=tile):
            _refusal(rec, base, base, 64, 64, 64)


@case("Fp8Side refuses: N % 8, ldc % 8, c_gstride % 8, an fp32 epilogue")
def _(rec):
    base = rec.buf("base", 64, 16)
    _refusal(rec, base, base[:, :12], 64, 12, 64)
    base = rec.buf("base12", 64, 12)
    _refusal(rec, base, base[:, :8], 64, 8, 64)
    base = rec.buf("basec", 72, 24)
    with G.fp8_side_output(_side(rec, base)) as side:
        geom = G.ConvGeom(2, 6, 6, 32, 6, 6, 3, 3, 1, 1, 1, 1, 1, 1, 16)
        G.gemm(72, 8, 144, G.Im2col(rec.buf("xc", 2, 6, 6, 32), geom, True, gstride=16),
               G.Dense(rec.buf("wc", 16, 144), 144, True, gstride=8 * 144), base, 24, epi=G.EPI_BF16, groups=2,
               c_gstride=12)
    rec.side(side)


@case("Fp8Side: _SIDE_FRAG off stores only through the LDS epilogue")
def _(rec):
    base = rec.buf("base", 64, 64)
    with patch(_SIDE_FRAG=False):
        _refusal(rec, base, base, 64, 64, 64)  # tile 0 stores through LDS: kept
        with patch(_FORCE_TILE=2):
            _refusal(rec, base, base, 64, 64, 64)
    with patch(_FORCE_TILE=2):
        _refusal(rec, base, base, 64, 64, 64)  # the per-fragment epilogue stores it


@case("side_bytes: used / missed")
def _(rec):
    base = rec.buf("base", 64, 64)
    with G.fp8_side_output(_side(rec, base)) as side:
        _dense(rec, 64, 64, 64, y=base)
    got = [G.side_bytes(None, base), G.side_bytes(side, base), G.side_bytes(side, base, e5m2=True),
           G.side_bytes(side, rec.buf("other", 64, 64)), G.side_bytes(side, base[:32])]
    rec.result("side_bytes", [g if g is None else g is side.q for g in got])
    rec.result("SIDE_STATS", dict(G.SIDE_STATS))
    side.ok = False
    rec.result("side_bytes", G.side_bytes(side, base))
    rec.result("SIDE_STATS", dict(G.SIDE_STATS))


# --- defer_reduce --------------------------------------------------------------------------------

class Sink:
    """The defer_reduce protocol, recorded."""

    def __init__(self, rec, accept):
        self.rec, self.accept = rec, accept

    def begin(self):
        self.rec.trace.append(["sink.begin"])

    def end(self):
        self.rec.trace.append(["sink.end"])

    def accepts(self, out, bias_grad):
        self.rec.trace.append(["sink.accepts", self.rec.arg(out), self.rec.arg(bias_grad), self.accept])
        return self.accept

    def slab(self, numel, device):
        self.rec.trace.append(["sink.slab", numel, str(device)])
        return self.rec.buf("slab", numel + 16, dtype=F32)[16:]

    def record(self, d):
        get = d.__getitem__ if isinstance(d, dict) else (lambda k: getattr(d, k))
        desc = {k: get(k) for k in SLAB_FIELDS}
        desc["ws"] = f"{self.rec.ptr(desc['ws'])}:{list(desc['ws'].shape)}".replace(" ", "")
        self.rec.trace.append(["sink.record", desc])


def _deferred(rec, accept, M=4096, **kw):
    dy, x, dw, db = _wgrad(rec, M, 64, 96)
    with G.defer_reduce(Sink(rec, accept)) as sink:
        assert G._DEFER_SINK is sink
        rec.result("fused", G.linear_wgrad(dy, x, dw, db=db, **kw))
    assert G._DEFER_SINK is None


@case("defer_reduce: the sink accepts")
def _(rec):
    _deferred(rec, True, accumulate=False, db_acc=False)


@case("defer_reduce: the sink accepts, grouped, no bias column")
def _(rec):
    geom = G.ConvGeom(2, 32, 32, 32, 32, 32, 3, 3, 1, 1, 1, 1, 1, 1, 16)
    with G.defer_reduce(Sink(rec, True)):
        G.gemm(32, 144, 2048, G.Dense(rec.buf("dy", 2048, 64), 64, False, gstride=32),
               G.Im2col(rec.buf("x", 2, 32, 32, 32), geom, False, gstride=16), rec.buf("dw", 64, 144, dtype=F32), 144,
               epi=G.EPI_F32, groups=2, c_gstride=32 * 144)


@case("defer_reduce: the sink refuses")
def _(rec):
    _deferred(rec, False, accumulate=False, db_acc=False)


@case("defer_reduce: EPI_F32_ACC is never deferred")
def _(rec):
    _deferred(rec, True, accumulate=True, db_acc=False)


@case("defer_reduce: an accumulated bias_grad is not deferred")
def _(rec):
    _deferred(rec, True, accumulate=False, db_acc=True)


@case("defer_reduce: fp8 is not deferred")
def _(rec):
    with G.defer_reduce(Sink(rec, True)):
        _fp8(rec, 64, 32, 16384, _deq(rec), kc=False, epi=G.EPI_F32, dtype=F32)


@case("defer_reduce: an unsplit product, begin / end alone")
def _(rec):
    _deferred(rec, True, M=64, accumulate=False, db_acc=False)


# --- pure tables ---------------------------------------------------------------------------------

def _cands(M, N, K, groups, b_kc_dense, epi, fp8=False, drop=False, mc=False):
    if not hasattr(G, "GemmCall"):  # the commit before: positional
        return (G._candidates_fp8(M, N, K, groups, epi, (int(drop),), mc) if fp8
                else G._candidates(M, N, K, groups, b_kc_dense, epi))
    a, b = (G.Operand(_lib.SnOperand(), int(m), G.OP_DENSE) for m in (mc, mc or not b_kc_dense))
    call = G.GemmCall(M, N, K, groups, a, b, epi, None, 0, dropout=(None, 0, 0.5) if drop else None,
                      fp8_format=int(fp8))
    return G._candidates_fp8(call) if fp8 else G._candidates(call)


@case("choose_tile, choose_splits")
def _(rec):
    for kc in (False, True):
        rec.result(f"choose_tile, M 64 128 256 1000 x N 10 48 64 96 112 128 192 200, b_kcontig={kc}",
                   [G.choose_tile(M, N, kc) for M in (64, 128, 256, 1000) for N in (10, 48, 64, 96, 112, 128, 192, 200)])
    for tile in (0, 1, 6, 10, 14, 22):
        rec.result(f"choose_splits, tile {tile}",
                   [[M, N, K, g, *G.choose_splits(M, N, K, g, tile)]
                    for M, N, K, g in ((64, 10, 4096, 1), (96, 433, 774400, 1), (32, 201, 102400, 1), (4096, 4096, 4096, 1),
                                       (128, 1153, 16771328, 1), (192, 1728, 43264, 2), (8192, 8192, 100000, 4),
                                       (100, 70, 200, 1), (256, 256, 256, 1), (1000, 1000, 1000, 3))])


CANDIDATES = [  # M, N, K, groups, b_kc_dense, epi
    (512, 512, 1024, 1, True, G.EPI_BF16), (512, 384, 1024, 1, False, G.EPI_F32), (512, 192, 4096, 1, False, G.EPI_BF16),
    (512, 160, 4096, 1, False, G.EPI_BF16), (256, 96, 512, 1, True, G.EPI_BF16), (256, 48, 512, 2, False, G.EPI_BF16),
    (192, 96, 20000, 1, True, G.EPI_F32), (192, 288, 20000, 2, False, G.EPI_F32_ACC), (64, 64, 100000, 1, False, G.EPI_F32),
    (32, 201, 102400, 1, False, G.EPI_F32), (128, 100, 64, 1, False, G.EPI_BF16), (512, 512, 1024, 1, False, G.EPI_SGD),
    (64, 64, 8192, 1, False, G.EPI_SGD), (4096, 4096, 4096, 4, True, G.EPI_BF16), (8192, 8192, 640, 1, False, G.EPI_F32),
]
CANDIDATES_FP8 = [  # M, N, K, groups, epi, dropout, MC operands
    (512, 512, 1024, 1, G.EPI_BF16, False, False), (512, 512, 1024, 1, G.EPI_BF16, True, False),
    (512, 512, 1024, 1, G.EPI_F32, False, False), (512, 512, 1024, 1, G.EPI_F32_ACC, False, False),
    (128, 1153, 16771328, 1, G.EPI_F32, False, True), (128, 64, 16384, 1, G.EPI_BF16, False, False),
    (8192, 8192, 1024, 2, G.EPI_BF16, False, False), (8192, 8192, 100000, 1, G.EPI_F32, False, True),
]


@case("_candidates, _candidates_fp8")
def _(rec):
    for c in CANDIDATES:
        rec.result(f"candidates {c}", [list(x) for x in _cands(*c)])
    with patch(_THIN=False):
        rec.result(f"candidates, no thin tiles {CANDIDATES[9]}", [list(x) for x in _cands(*CANDIDATES[9])])
    for M, N, K, g, epi, drop, mc in CANDIDATES_FP8:
        rec.result(f"candidates_fp8 {(M, N, K, g, epi, drop, mc)}",
                   [list(x) for x in _cands(M, N, K, g, not mc, epi, fp8=True, drop=drop, mc=mc)])


def dumps(traces: dict) -> str:
    """JSON, one launch per line."""
    cases = []
    for name, trace in traces.items():
        lines = ",\n".join("  " + json.dumps(launch, separators=(",", ":")) for launch in trace)
        cases.append(f" {json.dumps(name)}: [\n{lines}\n ]")
    return "{\n" + ",\n".join(cases) + "\n}\n"


if __name__ == "__main__":
    FIXTURE.write_text(dumps({name: run(name) for name in CASES}))
    print(f"{FIXTURE}: {len(CASES)} cases, {FIXTURE.stat().st_size} bytes")
