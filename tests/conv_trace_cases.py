"""Cases and recorder of tests/test_conv_launch_trace.py: which launches, with which arguments,
ops.hip.conv_forward + conv_backward issue for a geometry and a set of requests.

The dispatch is plain Python, so with the launchers replaced by a recorder (``hip.call``,
``_lib.call``, ``hip.gemm``, ``hip.colsum``, ``hip._dw_part``) and CPU bf16 tensors as operands
it runs anywhere in milliseconds.  A trace is the ordered list of launches of one case:

* ``[kernel, arg, ...]`` for a ``call``: scalars as they are, tensors as below;
* ``["gemm", M, N, K, A, B, out, ldc, {keyword: value}]`` with the operands as
  ``["Dense", t, ld, kcontig, gstride]``, ``["Im2col", t, [every ConvGeom field], kcontig,
  gstride]`` or ``["FlipW", t, Kg, R, S, Cg]``; ``"side": true`` among the keywords where the
  active fp8 side output covers ``out`` (the epilogue would store its fp8 bytes too);
* ``["colsum", t, out, accumulate]``, ``["dw_part", N, P, Q, C]``;
* ``["raise", text]`` where conv_backward refuses to read a bf16 output gradient that was never
  written, ``["result", ...]`` for what the calls returned.

A tensor is ``"buffer:dtype[shape]/[strides]+offset"``: the buffer is the name of the operand
whose storage it lies in (x, w, dy, ...) or ``t<n>`` for the n-th temporary in order of first
appearance, the offset is in elements from that storage's start.  Never a raw pointer.

``python tests/conv_trace_cases.py`` rewrites the fixture, tests/conv_launch_trace.json.  The
committed fixture was written by this module at the commit BEFORE ops.hip's workspace became a
typed ConvScratch: ``_scratch`` / ``_side_out`` build and read the plain dict of that commit when
ops.hip has no ConvScratch, so the module runs unchanged on both sides of that change.
"""
import contextlib
import dataclasses
import json
import os
import pathlib
import sys

import torch

if __name__ == "__main__":  # under pytest, tests/conftest.py has done this
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
from sparknet_amd.ops import _lib, gemm as G, hip
from sparknet_amd.ops.spec import ConvSpec

FIXTURE = pathlib.Path(__file__).with_name("conv_launch_trace.json")
BF16 = torch.bfloat16


def conv(N, H, W, C, K, r, stride=1, pad=0, groups=1) -> ConvSpec:
    return ConvSpec(N, H, W, C, K, r, r, stride, stride, pad, pad, 1, 1, groups)


@dataclasses.dataclass
class Case:
    spec: ConvSpec
    dw: bool = True
    db: bool = True
    gate: bool = True
    need_dx: bool = True
    dw_acc: bool = True
    db_acc: bool = True
    wt: bool = False           # the flipped weights come pre-computed (FlipBatch)
    x_in: tuple = None         # (Ctot, c0): x is the channel slice [c0, c0 + C) of a wider tensor
    y_in: tuple = None         # forward ``out=`` and dy, likewise
    dx_in: tuple = None        # ``dx_out=``, likewise; (C, 0) is a dense destination
    folded: bool = False       # the forward gets the folded input from upstream (fused augment + fold)
    stale: bool = False        # x is written between forward and backward: the cached fold is stale
    chunk: bool = False        # hip._MAX_PIX lowered so that the batch runs as chunks of two images
    fp8: tuple = None          # (formats, weight gradient too, dy_side): "e4m3" | "e5m2";
    #                            dy_side None | "covers" | "misses" | "only" | "only-misses"
    dx_side: bool = False      # request the fp8 copy of dx (the layer below's dy_side)
    patch: dict = dataclasses.field(default_factory=dict)  # attributes of ops.hip
    features: str = ""         # SN_FEATURES


C64 = conv(2, 16, 16, 64, 64, 3, pad=1)            # direct c64 (VGG conv1_2); e4m3: the fp8 direct kernel
C32 = conv(2, 8, 8, 32, 32, 3, pad=1)              # plain implicit GEMM, fp8-eligible both ways
CAFFENET1 = conv(2, 19, 19, 3, 96, 11, stride=4)   # folds to 48 -> 96, 3x3
GOOGLENET1 = conv(2, 8, 8, 3, 64, 7, stride=2, pad=3)  # folds to 16 -> 64, 4x4
VGG1 = conv(2, 8, 8, 3, 64, 3, pad=1)              # folds to 8 -> 64, 3x3
DW32 = ConvSpec(2, 8, 8, 32, 32, 3, 3, 2, 2, 1, 1, 1, 1, 32)
STRIDED = conv(2, 8, 8, 64, 128, 1, stride=2)

CASES = {
    # one per route
    "direct c64": Case(C64),
    "direct k96, packed off": Case(conv(2, 8, 8, 48, 96, 3), patch={"_PACKED": False}),
    "packed 3x3 via the fold": Case(CAFFENET1),
    "packed 4x4 via the fold": Case(GOOGLENET1),
    "packed k64 via the fold": Case(VGG1),
    "packed 1x1": Case(conv(2, 8, 8, 64, 64, 1), patch={"_PACKED11": True}),
    "direct96 split": Case(conv(2, 8, 8, 64, 192, 3, pad=1)),
    "grouped implicit": Case(conv(2, 6, 6, 96, 256, 5, pad=2, groups=2)),
    "depthwise": Case(DW32),
    "depthwise off": Case(DW32, features="conv_depthwise=0"),
    "explicit im2col": Case(conv(2, 9, 9, 5, 7, 3, stride=2)),
    "strided implicit": Case(STRIDED),
    # every route behind a switch, with the switch off
    "c64, direct off": Case(C64, patch={"_DIRECT_C64": False}),
    "k96, direct and packed off": Case(conv(2, 8, 8, 48, 96, 3), patch={"_PACKED": False, "_DIRECT_K96": False}),
    "caffenet conv1, packed off": Case(CAFFENET1, patch={"_PACKED": False}),
    "googlenet conv1, packed44 off": Case(GOOGLENET1, patch={"_PACKED44": False}),
    "vgg conv1_1, packed k64 off": Case(VGG1, patch={"_PACKED_K64": False}),
    "1x1, packed11 off": Case(conv(2, 8, 8, 64, 64, 1)),
    "64 -> 192, direct96 off": Case(conv(2, 8, 8, 64, 192, 3, pad=1), patch={"_DIRECT96": False}),
    # gradient requests
    "implicit, overwrite dw": Case(C32, dw_acc=False),
    "implicit, overwrite db": Case(C32, db_acc=False),
    "fold, overwrite both": Case(CAFFENET1, dw_acc=False, db_acc=False),
    "depthwise, overwrite both": Case(DW32, dw_acc=False, db_acc=False),
    "explicit, overwrite both": Case(conv(2, 9, 9, 5, 7, 3, stride=2), dw_acc=False, db_acc=False),
    "implicit, no dx": Case(C32, need_dx=False),
    "fold, no dx": Case(VGG1, need_dx=False),
    "implicit, db without dw": Case(C32, dw=False),
    "depthwise, db without dw": Case(DW32, dw=False),
    "implicit, dw without db": Case(C32, db=False),
    "implicit, dx alone, no gate": Case(C32, dw=False, db=False, gate=False),
    "strided, no gate": Case(STRIDED, gate=False),
    "fold, stale cache": Case(GOOGLENET1, stale=True),
    # the flipped weights
    "implicit, inplace weights": Case(C32, patch={"DGRAD_INPLACE_WEIGHTS": True}),
    "c64, inplace weights": Case(C64, patch={"DGRAD_INPLACE_WEIGHTS": True}),
    "implicit, pre-flipped": Case(C32, wt=True),
    "c64, pre-flipped": Case(C64, wt=True),
    "grouped, pre-flipped": Case(conv(2, 6, 6, 96, 256, 5, pad=2, groups=2), wt=True),
    # channel slices of a wider NHWC tensor
    "implicit, sliced x": Case(C32, x_in=(80, 16)),
    "implicit, sliced y": Case(C32, y_in=(96, 32)),
    "implicit, sliced dx": Case(C32, dx_in=(72, 8)),
    "implicit, dense dx_out": Case(C32, dx_in=(32, 0)),
    "implicit, all sliced": Case(C32, x_in=(80, 16), y_in=(96, 32), dx_in=(80, 16)),
    "c64, sliced x": Case(C64, x_in=(128, 64)),
    "c64, sliced dx": Case(C64, dx_in=(128, 0)),
    "strided, sliced x and dx": Case(STRIDED, x_in=(128, 64), dx_in=(128, 64)),  # col2im: dx by a copy
    "grouped, sliced x and dx": Case(conv(2, 6, 6, 96, 256, 5, pad=2, groups=2), x_in=(192, 96), dx_in=(192, 0)),
    "depthwise, sliced x and dx": Case(DW32, x_in=(64, 32), dx_in=(64, 0)),
    "fold, dense dx_out": Case(VGG1, dx_in=(3, 0)),
    # image chunks
    "chunked implicit": Case(dataclasses.replace(C32, N=3), chunk=True),
    "chunked implicit, overwrite, sliced dx": Case(dataclasses.replace(C32, N=3), chunk=True, dw_acc=False,
                                                   db_acc=False, dx_in=(64, 32)),
    "chunked fold": Case(dataclasses.replace(CAFFENET1, N=3), chunk=True),
    "chunked fused fold": Case(dataclasses.replace(CAFFENET1, N=3), chunk=True, folded=True),
    "chunked fused fold, stale": Case(dataclasses.replace(CAFFENET1, N=3), chunk=True, folded=True, stale=True),
    "fused fold": Case(CAFFENET1, folded=True),
    # the fp8 backward
    "fp8 dgrad e4m3, c64": Case(C64, fp8=("e4m3", False, None)),
    "fp8 dgrad e4m3, c64, direct fp8 off": Case(C64, fp8=("e4m3", False, None), patch={"_DIRECT_FP8": False}),
    "fp8 dgrad e5m2, c64": Case(C64, fp8=("e5m2", False, None), wt=True),
    "fp8 both e4m3": Case(C32, fp8=("e4m3", True, None)),
    "fp8 both e5m2, pre-flipped": Case(C32, fp8=("e5m2", True, None), wt=True),
    "fp8 both, side covers": Case(C32, fp8=("e4m3", True, "covers")),
    "fp8 both e5m2, side covers": Case(C32, fp8=("e5m2", True, "covers")),
    "fp8 dgrad, side covers": Case(C32, fp8=("e4m3", False, "covers")),
    "fp8 both, side misses": Case(C32, fp8=("e4m3", True, "misses")),
    "fp8 both, separate bias": Case(C32, fp8=("e4m3", True, None), patch={"FP8_WGRAD_BIAS": False}),
    "fp8 both, overwrite": Case(C32, fp8=("e4m3", True, "covers"), dw_acc=False, db_acc=False),
    "fp8 both, no dx": Case(C32, fp8=("e4m3", True, None), need_dx=False),
    "fp8 both, sliced dx": Case(C32, fp8=("e4m3", True, None), dx_in=(64, 0)),
    "fp8 both, strided": Case(conv(2, 8, 8, 32, 32, 3, stride=2, pad=1), fp8=("e4m3", True, None)),
    "fp8 both, chunked": Case(dataclasses.replace(C32, N=3), fp8=("e4m3", True, None), chunk=True),
    "fp8 both, chunked, side covers": Case(dataclasses.replace(C32, N=3), fp8=("e5m2", True, "covers"), chunk=True),
    "fp8 only": Case(C32, fp8=("e4m3", True, "only")),
    "fp8 only, c64, dx alone": Case(C64, fp8=("e4m3", False, "only"), dw=False, db=False),
    "fp8 only, separate bias raises": Case(C32, fp8=("e4m3", True, "only"), patch={"FP8_WGRAD_BIAS": False}),
    "fp8 only, bf16 wgrad raises": Case(C32, fp8=("e4m3", False, "only")),
    "fp8 only, side misses, raises": Case(C32, fp8=("e4m3", True, "only-misses")),
    "fp8 only, chunked, side misses, raises": Case(dataclasses.replace(C32, N=3), fp8=("e4m3", True, "only-misses"),
                                                   chunk=True),
    "fp8 only, strided dgrad raises": Case(conv(2, 8, 8, 32, 32, 3, stride=2, pad=1), fp8=("e4m3", False, "only"),
                                           dw=False, db=False),
    "fp8 only, bf16 flip dgrad raises": Case(conv(2, 8, 8, 32, 24, 3, pad=1), fp8=("e4m3", False, "only"),
                                             dw=False, db=False),
    "dx side": Case(C32, dx_side=True),
    "dx side, c64": Case(C64, dx_side=True),  # the direct kernel has no side output: the GEMM runs
    "dx side, sliced dx": Case(C32, dx_side=True, dx_in=(64, 0)),
    "dx side, dense dx_out": Case(C32, dx_side=True, dx_in=(32, 0)),
    "dx side, no dx": Case(C32, dx_side=True, need_dx=False),
    "dx side, strided": Case(STRIDED, dx_side=True),
    "dx side, depthwise": Case(DW32, dx_side=True),
    "dx side, chunked": Case(dataclasses.replace(C32, N=3), dx_side=True, chunk=True),
    "dx side, fp8 both": Case(C32, dx_side=True, fp8=("e4m3", True, "covers")),
    "dx side, fp8 dgrad, c64": Case(C64, dx_side=True, fp8=("e4m3", False, None)),
}


# --- the workspace, on both sides of the ConvScratch change ----------------------------------

def _scratch(**fields):
    """The forward -> backward workspace holding ``fields``."""
    if not hasattr(hip, "ConvScratch"):
        return fields  # the commit before: a dict under the same names, the requests plain tuples
    if "fp8_dgrad" in fields:
        fields["fp8_dgrad"] = hip.Fp8Dgrad(*fields["fp8_dgrad"])
    if "fp8_wgrad" in fields:
        fields["fp8_wgrad"] = hip.Fp8Wgrad(*fields["fp8_wgrad"])
    return hip.ConvScratch(**fields)


def _set(ws, **fields):
    other = _scratch(**fields)
    for k in fields:
        if isinstance(ws, dict):
            ws[k] = other[k]
        else:
            setattr(ws, k, getattr(other, k))


def _side_out(ws):
    """(was the fp8 copy of dx reported?, the Fp8Side or None)."""
    if isinstance(ws, dict):
        return "fp8_dx_side_out" in ws, ws.get("fp8_dx_side_out")
    return ws.fp8_dx_side_out is not None, ws.fp8_dx_side_out


# --- the recorder ----------------------------------------------------------------------------

class Scales:
    """Stands for the delayed-scaling table (engine.enable_fp8): slot i is e5m2 if listed."""

    def __init__(self, e5m2=()):
        self.e5m2 = set(e5m2)
        self.slots = [torch.zeros(4) for _ in range(4)]
        self.deqs = [torch.zeros(1) for _ in range(4)]

    def slot(self, i):
        return self.slots[i]

    def deq(self, i):
        return self.deqs[i]

    def is_e5m2(self, i):
        return i in self.e5m2

    def names(self):
        return {**{f"slot{i}": t for i, t in enumerate(self.slots)}, **{f"deq{i}": t for i, t in enumerate(self.deqs)}}


class Recorder:
    def __init__(self, named):
        self.trace = []
        self.names = {}
        self.keep = []  # storages stay alive, so that an address names one buffer for the whole case
        for name, t in named.items():
            self.name(t, name)

    def name(self, t, name=None):
        st = t.untyped_storage()
        if st.data_ptr() not in self.names:
            self.keep.append(st)
            self.names[st.data_ptr()] = name or f"t{sum(n[0] == 't' and n[1:].isdigit() for n in self.names.values())}"
        return self.names[st.data_ptr()]

    def arg(self, v):
        if isinstance(v, torch.Tensor):
            return (f"{self.name(v)}:{str(v.dtype)[6:]}{list(v.shape)}/{list(v.stride())}+{v.storage_offset()}"
                    .replace(" ", ""))
        if isinstance(v, (tuple, list)):
            return [self.arg(e) for e in v]
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        raise TypeError(f"launch argument {v!r}")

    def operand(self, op):
        if isinstance(op, G.Dense):
            return ["Dense", self.arg(op.t), op.ld, op.kcontig, op.gstride]
        if isinstance(op, G.Im2col):
            return ["Im2col", self.arg(op.x), list(dataclasses.astuple(op.geom)), op.kcontig, op.gstride]
        assert isinstance(op, G.FlipW), op
        return ["FlipW", self.arg(op.w), op.Kg, op.R, op.S, op.Cg]

    def call(self, kernel, *args):
        self.trace.append([kernel, *map(self.arg, args)])

    def gemm(self, M, N, K, A, B, out, ldc, **kw):
        kw = {k: self.arg(v) for k, v in sorted(kw.items())}
        if G._SIDE is not None and G._SIDE.covers(out):
            G._SIDE.launches += 1
            kw["side"] = True
        self.trace.append(["gemm", M, N, K, self.operand(A), self.operand(B), self.arg(out), ldc, kw])

    def colsum(self, x, out, accumulate=True):
        self.trace.append(["colsum", self.arg(x), self.arg(out), accumulate])

    def dw_part(self, s, device):
        self.trace.append(["dw_part", s.N, s.P, s.Q, s.C])
        return torch.zeros(8), 8


@contextlib.contextmanager
def _patched(rec, case, max_pix):
    attrs = {"call": rec.call, "gemm": rec.gemm, "colsum": rec.colsum, "_dw_part": rec.dw_part, **case.patch}
    if max_pix:
        attrs["_MAX_PIX"] = max_pix
    saved = {k: getattr(hip, k) for k in attrs}
    lib_call, env = _lib.call, os.environ.get("SN_FEATURES")
    try:
        for k, v in attrs.items():
            setattr(hip, k, v)
        _lib.call = rec.call
        os.environ["SN_FEATURES"] = case.features
        yield
    finally:
        for k, v in saved.items():
            setattr(hip, k, v)
        _lib.call = lib_call
        if env is None:
            del os.environ["SN_FEATURES"]
        else:
            os.environ["SN_FEATURES"] = env


def _nhwc(N, H, W, C, view=None):
    """A zero [N, H, W, C] bf16 tensor (dense, or the channel slice ``view`` = (Ctot, c0) of a wider
    one) and the tensor that owns its storage."""
    ctot, c0 = view or (C, 0)
    base = torch.zeros((N, H, W, ctot), dtype=BF16)
    return (base if ctot == C else base[..., c0:c0 + C]), base


def run(case: Case, backwards: int = 1) -> list:
    """The launch trace of conv_forward (bias + ReLU) and conv_backward for one case (``backwards``: that many
    backward calls, each with the layer's requests set anew on the one workspace)."""
    s = case.spec
    x, x_base = _nhwc(s.N, s.H, s.W, s.C, case.x_in)
    y, y_base = _nhwc(s.N, s.P, s.Q, s.K, case.y_in)
    dy, dy_base = _nhwc(s.N, s.P, s.Q, s.K, case.y_in)
    dx, dx_base = _nhwc(s.N, s.H, s.W, s.C, case.dx_in)
    named = {"x": x_base, "dy": dy_base, "w": torch.zeros((s.K, s.R, s.S, s.Cg), dtype=BF16), "b": torch.zeros(s.K),
             "dw": torch.zeros((s.K, s.R, s.S, s.Cg)), "db": torch.zeros(s.K),
             "w_flipped": torch.zeros((s.groups, s.Cg, s.R, s.S, s.Kg), dtype=BF16)}
    if case.y_in:
        named["y"] = y_base
    if case.dx_in:
        named["dx"] = dx_base
    plan = hip._s2d_plan(s)
    max_pix = 0
    if case.chunk:  # chunks of two images, counted as hip._image_chunk counts them
        per = max(s.H * s.W, s.P * s.Q, plan[4].H * plan[4].W if plan else 1)
        max_pix = 2 * per + 1
    folded = None
    if case.folded:
        s2 = plan[4]
        folded = named["folded"] = torch.zeros((s.N, s2.H, s2.W, s2.C), dtype=BF16)
    requests = {}
    if case.wt:
        requests.update(wt=named["w_flipped"])
    if case.fp8:
        fmt, wgrad, dy_side = case.fp8
        sc = Scales(e5m2=(1,) if fmt == "e5m2" else ())  # slots: 0 x, 1 dy, 2 flipped w, 3 the layer below's dy
        named.update(sc.names())
        side = None
        if dy_side:
            covered = dy if "misses" not in dy_side else torch.zeros_like(dy)
            side = G.Fp8Side(covered, sc.slot(1), sc.is_e5m2(1), torch.zeros(8))
            side.launches, side.only = 1, "only" in dy_side
            named["dy_side.q"] = side.q
        requests.update(fp8_dgrad=(sc, 1, 2) if side is None else (sc, 1, 2, side))
        if wgrad:
            named["xq"] = torch.zeros(x.shape, dtype=torch.uint8)
            requests.update(fp8_wgrad=(sc, 0, named["xq"], 1))
    if case.dx_side:
        named["dx_side.slot"], named["dx_side.part"] = torch.zeros(4), torch.zeros(8)
        requests.update(fp8_dx_side=(named["dx_side.slot"], False, named["dx_side.part"]))
    rec = Recorder(named)
    ws = _scratch()
    with _patched(rec, case, max_pix):
        out = hip.conv_forward(x, named["w"], named["b"], s, relu=True, ws=ws, folded=folded,
                               out=y if case.y_in else None)
        rec.trace.append(["result", "y", rec.arg(out)])
        if case.stale:
            x.add_(1)
        for _ in range(backwards):
            _set(ws, **requests)
            try:
                got = hip.conv_backward(dy, x, named["w"], s, case.need_dx, named["dw"] if case.dw else None,
                                        named["db"] if case.db else None, x if case.gate else None, ws,
                                        dw_acc=case.dw_acc, db_acc=case.db_acc, dx_out=dx if case.dx_in else None)
            except RuntimeError as e:
                if not str(e).startswith("conv backward: "):
                    raise
                rec.trace.append(["raise", str(e)])
                break
            else:
                rec.trace.append(["result", "dx", None if got is None else rec.arg(got)])
                reported, side = _side_out(ws)
                if reported:
                    rec.trace.append(["result", "fp8 side of dx",
                                      side and [rec.arg(side.base), rec.arg(side.q), side.launches, side.complete]])
    return rec.trace


def dumps(traces: dict) -> str:
    """JSON, one launch per line."""
    cases = []
    for name, trace in traces.items():
        cases.append(f" {json.dumps(name)}: [\n" + ",\n".join("  " + json.dumps(launch) for launch in trace) + "\n ]")
    return "{\n" + ",\n".join(cases) + "\n}\n"


if __name__ == "__main__":
    FIXTURE.write_text(dumps({name: run(case) for name, case in CASES.items()}))
    print(f"{FIXTURE}: {len(CASES)} cases, {FIXTURE.stat().st_size} bytes")
