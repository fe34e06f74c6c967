"""LSTM / LRCN on the CPU: ``ops.ref`` against tests/lstm_cases.py at fp32 accuracy, the layer from upstream prototxt."""
import pytest
import torch

import lstm_cases as lc
from sparknet_amd import models, proto
from sparknet_amd.core.net import Net
from sparknet_amd.ops import ref


def run(impl, case, conv=lambda k, t: t):
    """The case through ``impl``: the outputs of lstm_cases.oracle.  ``conv(name, tensor)`` places an input."""
    i = {k: conv(k, v) for k, v in lc.inputs(case).items()}
    x2, h0, c0 = i["x"].reshape(case.T * case.N, case.D), i["h0"].clone(), i["c0"].clone()
    st = (i["xs"], i["w_xs"]) if case.static else (None, None)
    for cont in ([i["cont_first"]] if case.twice else []) + [i["cont"]]:
        h, saved = impl.lstm_forward(x2, cont, i["w_xc"], i["b_c"], i["w_hc"], h0, c0, *st)
    z = lambda t: torch.zeros(t.shape, dtype=torch.float32, device=t.device)
    out = {"h": h, "c": c0, "dw_xc": z(i["w_xc"]), "db": z(i["b_c"]), "dw_hc": z(i["w_hc"])}
    if case.static:
        out["dw_xs"] = z(i["w_xs"])
    out["dx"], dxs = impl.lstm_backward(i["dh"], x2, i["cont"], i["w_xc"], i["w_hc"], saved, True, out["dw_xc"], out["db"],
                                        out["dw_hc"], *st, out.get("dw_xs"), bool(case.static))
    if case.static:
        out["dxs"] = dxs
    return out


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.name)
def test_ref_lstm(case):
    plain, eps = lc.expected(case)[0], lc.eps32(case.T, case.D, case.H)
    assert lc.worst_ratio(run(ref, case), plain, dict.fromkeys(plain, eps), case.name) <= 1.0


def test_recurrence_matters():
    """A kernel that dropped W_hc or cont would miss the bound on h at least tenfold, in every case."""
    for case in lc.CASES:
        i, (plain, bound) = lc.inputs(case), lc.expected(case)
        other = torch.zeros_like(i["cont"]) if case.twice else torch.ones_like(i["cont"])
        cont = lc.distance(lc.oracle(i, cont=other)["h"], plain["h"]) / bound["h"]
        none = lc.distance(lc.oracle(i, w_hc=torch.zeros_like(i["w_hc"]))["h"], plain["h"]) / bound["h"]
        print(case.name, "W_hc = 0:", none, "other cont:", cont)
        assert cont >= 10 and (none >= 10 or case.cont == "zeros"), (case.name, none, cont)


UPSTREAM = """name: "lstm"
layer { name: "x" type: "Input" top: "x" java_data_param { shape { dim: 3 dim: 2 dim: 5 } } }
layer { name: "cont" type: "Input" top: "cont" java_data_param { shape { dim: 3 dim: 2 } } }
layer { name: "lstm1" type: "LSTM" bottom: "x" bottom: "cont" top: "lstm1"
  recurrent_param { num_output: 8 weight_filler { type: "uniform" min: -0.5 max: 0.5 } bias_filler { type: "constant" value: 0.1 } } }
"""


def test_lstm_prototxt():
    """Blob order; the forward is the op; the second forward continues the first; reset(); expose_hidden refused."""
    net = Net(proto.parse_prototxt(UPSTREAM), phase=proto.TRAIN, device="cpu", seed=3)
    layer, top = net.layer_by_name("lstm1"), net.blob_by_name("lstm1")
    assert [p.caffe_shape for p in layer.params] == [(32, 5), (32,), (32, 8)] and tuple(top.shape) == (3, 2, 8)
    x, cont = torch.randn(3, 2, 5, generator=torch.Generator().manual_seed(1)), torch.tensor([[0.0, 0.0], [1.0, 1.0], [1.0, 0.0]])
    net.blob_by_name("x").data.copy_(x)
    w_xc, b_c, w_hc = (p.data for p in layer.params)
    h0, c0 = torch.zeros(2, 8), torch.zeros(2, 8)
    for cont_t in (cont, torch.ones(3, 2), None):
        if cont_t is None:  # after reset() the all-ones forward starts from zero again
            layer.reset(), h0.zero_(), c0.zero_()
            cont_t = torch.ones(3, 2)
        net.blob_by_name("cont").data.copy_(cont_t)
        net.forward()
        want, _ = ref.lstm_forward(x.reshape(6, 5), cont_t, w_xc, b_c, w_hc, h0, c0)
        assert torch.equal(top.data, want) and float(want.abs().max()) > 0
    with pytest.raises(ValueError, match="expose_hidden"):
        Net(proto.parse_prototxt(UPSTREAM.replace("num_output: 8", "num_output: 8 expose_hidden: true")), phase=proto.TRAIN,
            device="cpu")


def test_lrcn_builds():
    net = Net(models.lrcn(width=0.125, size=96, T=3, N=2), phase=proto.TRAIN, device="cpu")
    size = lambda name: tuple(net.blob_by_name(name).shape)
    assert size("fc6") == (6, 512) and size("fc6-reshape") == (3, 2, 512) and size("lstm1") == (3, 2, 32)
    assert size("fc8-final") == (3, 2, 101) and size("score") == (6, 101) and size("label-flat") == (6, 1)
    assert [p.caffe_shape for p in net.layer_by_name("lstm1").params] == [(128, 512), (128,), (128, 32)]
    assert models.solver_for("lrcn", width=0.125, size=96, T=3, N=2).stepsize == 10000
