"""The squeeze-and-excitation kernels (csrc/kernels/se.hip) on the GPU against the fp64 oracle and
the format-derived bounds of tests/se_cases.py: the three wrappers on every case, the Pooling and
Axpy layers with the launches they make, the same layer checks on the se_kernels=0 routes, and
bitwise repeatability."""
import pytest
import torch

import se_cases as sc
from sparknet_amd import proto
from sparknet_amd.core.net import Net
from test_se import run_axpy

pytestmark = pytest.mark.gpu

NEW = ("gap_fwd", "nc_affine_fwd", "nc_affine_bwd")
USES = (("s", "b", "r"), ("b", "r"), ("s", "r"), ("s", "b"), ("s",), ("b",), ("r",))  # each operand absent in turn


def _dev(i, gpu, fp32=False):
    return {k: (v.float() if fp32 else v).to(gpu) for k, v in i.items()}


def _geom(case):
    N, H, W, C = case
    return N, H * W, C


def _forms(case):
    return [(learned, fp32) for learned in (False, True) for fp32 in ((False, True) if case in sc.FP32_CASES else (False,))]


# --- the wrappers -----------------------------------------------------------------------------

@pytest.mark.parametrize("case", sc.CASES, ids=sc.IDS)
def test_gap_fwd(gpu, case):
    from sparknet_amd.ops import layers_hip as lh
    N, HW, C = _geom(case)
    y = lh.gap_fwd(sc.inputs(case)["x"].to(gpu), N, HW, C)
    assert y.shape == (N, 1, 1, C) and y.dtype == torch.bfloat16
    w = sc.worst(y, *sc.pool_bound(case))
    print("gap_fwd", case, w)
    assert w <= 1.0


@pytest.mark.parametrize("case", sc.CASES, ids=sc.IDS)
def test_nc_affine_fwd(gpu, case):
    from sparknet_amd.ops import layers_hip as lh
    N, HW, C = _geom(case)
    for learned, fp32 in _forms(case):
        d = _dev(sc.inputs(case, learned), gpu, fp32)
        for use in USES:
            y = lh.nc_affine_fwd(d["x"], N, HW, C, **{k: d[k] for k in use})
            assert y.dtype == d["x"].dtype and y.shape == d["x"].shape
            w = sc.worst(y, *sc.forward_bound(case, learned, use, fp32))
            print("nc_affine_fwd", case, learned, fp32, use, w)
            assert w <= 1.0, (learned, fp32, use)


@pytest.mark.parametrize("case", sc.CASES, ids=sc.IDS)
def test_nc_affine_bwd(gpu, case):
    from sparknet_amd.ops import layers_hip as lh
    N, HW, C = _geom(case)
    for learned, fp32 in _forms(case):
        d = _dev(sc.inputs(case, learned), gpu, fp32)
        for flag, prefill in ((lh.GRAD_STORE, None), (lh.GRAD_ACC, sc.PREFILL)):
            bx, bs, bb = sc.backward_bound(case, learned, prefill, fp32=fp32)
            ds = torch.full((N, C), sc.PREFILL, device=gpu)
            db = torch.full((N, C), sc.PREFILL, device=gpu)
            dx = lh.nc_affine_bwd(d["dy"], N, HW, C, s=d["s"], x=d["x"], ds=ds, sflag=flag, db=db, bflag=flag)
            ws = (sc.worst(dx, *bx), sc.worst(ds, *bs), sc.worst(db, *bb))
            print("nc_affine_bwd", case, learned, fp32, prefill, ws)
            assert dx.dtype == d["dy"].dtype and max(ws) <= 1.0, (learned, fp32, prefill, ws)
            # each output absent in turn: the others do not change, a skipped buffer is not written
            ds2, db2 = torch.full_like(ds, sc.PREFILL), torch.full_like(db, sc.PREFILL)
            assert lh.nc_affine_bwd(d["dy"], N, HW, C, x=d["x"], want_dx=False, ds=ds2, sflag=flag, db=db2,
                                    bflag=flag) is None
            assert torch.equal(ds2, ds) and torch.equal(db2, db)
            ds3, db3 = torch.full_like(ds, sc.PREFILL), torch.full_like(db, sc.PREFILL)
            dx3 = lh.nc_affine_bwd(d["dy"], N, HW, C, s=d["s"], db=db3, bflag=flag)
            assert torch.equal(dx3, dx) and torch.equal(db3, db)
            dx4 = lh.nc_affine_bwd(d["dy"], N, HW, C, s=d["s"], x=d["x"], ds=ds3, sflag=flag)
            assert torch.equal(dx4, dx) and torch.equal(ds3, ds)
            assert torch.equal(lh.nc_affine_bwd(d["dy"], N, HW, C, s=d["s"]), dx)


def test_wrappers_reject_what_the_kernels_cannot_take(gpu):
    from sparknet_amd.ops import layers_hip as lh
    d = _dev(sc.inputs(sc.CASES[3]), gpu)
    N, HW, C = _geom(sc.CASES[3])
    with pytest.raises(ValueError):
        lh.nc_affine_fwd(d["x"], N, HW, C, s=d["s"].bfloat16())
    with pytest.raises(ValueError):
        lh.nc_affine_fwd(d["x"], N, HW, C, r=d["r"].float())
    with pytest.raises(ValueError):
        lh.nc_affine_bwd(d["dy"], N, HW, C)  # dx without a scale is dy itself
    with pytest.raises(ValueError):
        lh.nc_affine_bwd(d["dy"], N, HW, C, want_dx=False, ds=torch.empty(N, C, device=gpu), sflag=lh.GRAD_STORE)


# --- the layers ---------------------------------------------------------------------------------

class _Recorder:
    """Names of the native launches made through ops.layers_hip.call / ops.hip.call."""

    def __enter__(self):
        from sparknet_amd.ops import _lib, hip, layers_hip
        self.names = []

        def call(name, *args):
            self.names.append(name)
            return _lib.call(name, *args)
        hip.call = layers_hip.call = call
        return self

    def __exit__(self, *exc):
        from sparknet_amd.ops import _lib, hip, layers_hip
        hip.call = layers_hip.call = _lib.call

    def new(self):
        return [n for n in self.names if n in NEW]


def _switch(monkeypatch, on):
    if on:
        monkeypatch.delenv("SN_FEATURES", raising=False)
    else:
        monkeypatch.setenv("SN_FEATURES", "se_kernels=0")


def _pool_layer(case, gpu):
    N, H, W, C = case
    net = Net(proto.parse_prototxt(
        f'name: "g" force_backward: true\n'
        f'layer {{ name: "in" type: "Input" top: "x" java_data_param {{ shape {{ dim: {N} dim: {C} dim: {H} dim: {W} }} }} }}\n'
        'layer { name: "L" type: "Pooling" bottom: "x" top: "y" pooling_param { pool: AVE global_pooling: true } }'),
        phase=proto.TRAIN, seed=3, device=gpu)
    return net.layers[-1], net.bottom_vecs[-1], net.top_vecs[-1]


@pytest.mark.parametrize("on", (True, False), ids=("se_kernels", "se_kernels=0"))
@pytest.mark.parametrize("case", sc.CASES, ids=sc.IDS)
def test_global_average_pooling_layer(gpu, monkeypatch, case, on):
    """Within the pool bound on both routes; gap_fwd exactly where H W > 64 and the switch is on
    (64 positions stay on avepool_fwd, whose entry is pool_fwd); the backward stays on pool_bwd:
    dy / M at every position, one rounding."""
    _switch(monkeypatch, on)
    N, H, W, C = case
    i = sc.inputs(case)
    layer, bvec, tvec = _pool_layer(case, gpu)
    bvec[0].data = i["x"].to(gpu)
    with _Recorder() as rec:
        layer.forward(bvec, tvec)
        tvec[0].diff = i["dy"][:, :1, :1].contiguous().to(gpu)
        layer.backward(tvec, [True], bvec)
    assert rec.names == (["gap_fwd", "pool_bwd"] if on and H * W > 64 else ["pool_fwd", "pool_bwd"]), rec.names
    if case in (sc.HW64, sc.HW65):
        assert rec.names[0] == ("gap_fwd" if on and case == sc.HW65 else "pool_fwd")
    w = sc.worst(tvec[0].data, *sc.pool_bound(case))
    print("Pooling", case, on, w)
    assert tvec[0].data.dtype == torch.bfloat16 and w <= 1.0
    ref = (i["dy"][:, :1, :1].to(sc.F64) / (H * W)).expand(N, H, W, C)
    assert sc.worst(bvec[0].diff, ref, (sc.U16 + 4 * sc.U32) * ref.abs()) <= 1.0


@pytest.mark.parametrize("on", (True, False), ids=("se_kernels", "se_kernels=0"))
@pytest.mark.parametrize("case", sc.CASES, ids=sc.IDS)
def test_axpy_layer(gpu, monkeypatch, case, on):
    """top, dx and da within the bounds on both routes (the gate's gradient is rounded into a bf16
    blob when the gate is an image blob), dy exactly dtop; one nc_affine_fwd and one nc_affine_bwd
    and no layout copy with the switch on, none of the new launches with it off."""
    _switch(monkeypatch, on)
    for image_gate in (False, True):
        with _Recorder() as rec:
            top, (da, dx, dy) = run_axpy(case, gpu, image_gate)
        if on:
            assert rec.new() == ["nc_affine_fwd", "nc_affine_bwd"], rec.names
            assert not {"transpose", "axis_scale_bias", "axis_reduce", "eltwise_fwd"} & set(rec.names), rec.names
        else:
            assert rec.new() == [] and {"transpose", "axis_scale_bias", "axis_reduce", "eltwise_fwd"} <= set(rec.names)
        assert top.dtype == torch.bfloat16 and dx.dtype == torch.bfloat16
        assert image_gate <= (da.dtype == torch.bfloat16)  # an image blob is bf16 on the device
        bx, ba, _ = sc.backward_bound(case, bf16_store=da.dtype == torch.bfloat16)
        ws = (sc.worst(top, *sc.forward_bound(case, use=("s", "r"))), sc.worst(dx, *bx), sc.worst(da, *ba))
        print("Axpy", case, on, image_gate, ws)
        assert max(ws) <= 1.0, (image_gate, ws)
        assert torch.equal(dy.cpu(), sc.inputs(case)["dy"])


@pytest.mark.parametrize("propagate", [(True, False, False), (False, True, False), (False, False, True)])
def test_axpy_layer_honours_propagate_down(gpu, monkeypatch, propagate):
    _switch(monkeypatch, True)
    _, ref = run_axpy(sc.CASES[3], gpu)
    with _Recorder() as rec:
        _, got = run_axpy(sc.CASES[3], gpu, propagate=propagate)  # asserts that the others are untouched
    for g, r, p in zip(got, ref, propagate):
        assert not p or torch.equal(g, r)
    assert rec.new() == (["nc_affine_fwd"] if propagate[2] else ["nc_affine_fwd", "nc_affine_bwd"])


# --- determinism --------------------------------------------------------------------------------

def test_two_runs_are_bitwise_equal(gpu, monkeypatch):
    from sparknet_amd.ops import layers_hip as lh
    _switch(monkeypatch, True)
    case = sc.LARGEST
    N, HW, C = _geom(case)
    d = _dev(sc.inputs(case), gpu)

    def run():
        ds, db = torch.empty(N, C, device=gpu), torch.empty(N, C, device=gpu)
        dx = lh.nc_affine_bwd(d["dy"], N, HW, C, s=d["s"], x=d["x"], ds=ds, sflag=lh.GRAD_STORE, db=db,
                              bflag=lh.GRAD_STORE)
        return (lh.gap_fwd(d["x"], N, HW, C), lh.nc_affine_fwd(d["x"], N, HW, C, d["s"], d["b"], d["r"]), dx, ds, db,
                *run_axpy(case, gpu)[1])
    a, b = run(), run()
    assert len(a) == 8 and all(torch.equal(x, y) for x, y in zip(a, b))
