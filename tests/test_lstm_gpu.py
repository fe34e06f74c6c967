"""csrc/kernels/lstm.hip through ``hip.lstm_forward`` / ``lstm_backward`` against tests/lstm_cases.py, launch names
spied; lrcn(width=0.125, size=96, T=3, N=2), kernels on and off, against the fp32 CPU engine from lstm1's bottom on."""
import pytest
import torch

import lstm_cases as lc
from test_lstm import run
from sparknet_amd import models, proto
from sparknet_amd.core.net import Net

pytestmark = pytest.mark.gpu
CONT = torch.tensor([[0.0, 0.0], [1.0, 1.0], [1.0, 0.0]])


def spy(mp, names):
    from sparknet_amd.ops import _lib, hip
    mp.setattr(hip, "call", lambda name, *args: (names.append(name), _lib.call(name, *args))[1])


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.name)
def test_lstm_kernels(case, gpu, monkeypatch):
    """Every output within its bound; two runs bitwise equal; exactly T launches per forward and per backward."""
    from sparknet_amd.ops import hip
    names = []
    monkeypatch.delenv("SN_FEATURES", raising=False)
    spy(monkeypatch, names)
    place = lambda k, t: t.to(gpu) if k in ("cont", "cont_first", "c0", "b_c") else t.to(gpu, torch.bfloat16)
    got, again = run(hip, case, place), run(hip, case, place)
    assert lc.worst_ratio(got, *lc.expected(case), case.name) <= 1.0 and all(torch.equal(got[k], again[k]) for k in got)
    steps = [n for n in names if n.startswith("lstm_step")]
    assert steps == (["lstm_step_fwd"] * case.T * (2 if case.twice else 1) + ["lstm_step_bwd"] * case.T) * 2


def outputs(net, names=()):
    net.blob_by_name("clip_markers").data.copy_(CONT)
    net.forward_backward()
    layer, li = net.layer_by_name("lstm1"), net.layer_names.index("lstm1")
    return {"loss": net.blob_by_name("loss").data.float().clone(), "h": net.top_vecs[li][0].data.clone(),
            "dx": net.bottom_vecs[li][0].diff.clone(), "dw_xc": layer.w_xc.diff.clone(), "db": layer.b_c.diff.clone(),
            "dw_hc": layer.w_hc.diff.clone(), "names": [n for n in names if "lstm" in n]}


@pytest.fixture(scope="module")
def nets(gpu):
    """Loss, lstm1's top, bottom and parameter gradients of LRCN on the GPU ("on" / "off") and of the CPU engine on
    lrcn(trunk=False) with the GPU net's lstm1 bottom and bf16 weights; bounds from the oracle forms with fc8-final
    and the loss (scores, their gradient and dh rounded to bf16) as their tail."""
    out, names, mp = {}, [], pytest.MonkeyPatch()
    g = torch.Generator().manual_seed(4)
    data, label = 50 * torch.randn(6, 3, 96, 96, generator=g), torch.randint(0, 101, (3, 2), generator=g).float()
    kw = dict(width=0.125, T=3, N=2, drop=0.0)
    try:
        spy(mp, names)
        for key, feat in (("on", ""), ("off", "lstm_kernels=0")):
            mp.setenv("SN_FEATURES", feat)
            net = Net(models.lrcn(size=96, **kw), phase=proto.TRAIN, device=torch.device(gpu), seed=5)
            for p in net.layer_by_name("lstm1").params[::2]:  # weights at which the recurrence matters at 32 units
                p.data.mul_(30)
            net.sync_compute()
            net.blob_by_name("data").set_nchw(data)
            net.blob_by_name("label").data.copy_(label)
            del names[:]
            out[key] = outputs(net, names)
    finally:
        mp.undo()
    param = models.lrcn(trunk=False, **kw)
    param.force_backward = True
    cpu = Net(param, phase=proto.TRAIN, device="cpu")
    w = {}
    for name in ("lstm1", "fc8-final"):  # the GPU net's bf16 shadows of the weights, its fp32 biases
        for pc, pg in zip(cpu.layer_by_name(name).params, net.layer_by_name(name).params):
            pc.data.copy_((pg.compute if pg.data.dim() > 1 else pg.data).float().cpu())
            w[name, len(w)] = pc.data.double()
    cpu.sync_compute()
    x = net.blob_by_name("fc6-reshape").data.float().cpu()
    cpu.blob_by_name("fc6-reshape").data.copy_(x)
    cpu.blob_by_name("label").data.copy_(label)
    out["cpu"] = outputs(cpu)
    (w_xc, b_c, w_hc, w8, b8), rows = w.values(), torch.arange(6)

    def tail(h, rb):
        s = rb(h.reshape(6, -1) @ w8.t() + b8)
        p = torch.softmax(s, 1)
        onehot = torch.nn.functional.one_hot(label.reshape(6).long(), 101).double()
        return rb(rb((p - onehot) / 6) @ w8).reshape(h.shape), {"loss": -torch.log(p[rows, label.reshape(6).long()]).mean()}

    i = {"x": x, "w_xc": w_xc, "b_c": b_c, "w_hc": w_hc, "h0": torch.zeros(2, 32), "c0": torch.zeros(2, 32), "cont": CONT}
    plain, rnd = lc.oracle(i, tail=tail), lc.oracle(i, True, tail=tail)
    del plain["c"], rnd["c"]
    out["bound"] = lc.bounds(plain, rnd, lc.eps32(3, 512, 32))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("key", ["on", "off"])
def test_lrcn_against_cpu_engine(nets, key):
    assert lc.worst_ratio(nets[key], nets["cpu"], nets["bound"], "lrcn " + key) <= 1.0


def test_lrcn_launches(nets):
    assert (nets["on"]["names"], nets["off"]["names"]) == (["lstm_step_fwd"] * 3 + ["lstm_transpose"] + ["lstm_step_bwd"] * 3, [])
