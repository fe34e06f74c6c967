"""The loss / accuracy head on the CPU: ``ops.ref`` (the fp32 reference that the GPU tests
and the CPU engine lean on) against independent oracles.

* Accuracy follows the reference's AccuracyLayer (caffe/src/caffe/layers/accuracy_layer.cpp):
  a descending sort of (score, class index) pairs, so a class tying the label's score ranks
  ahead of it when its index is higher, and a row of equal (or all-NaN) scores is a hit only
  for the labels within top_k of the highest index.  Counting strictly higher scores alone
  reports 100 % for a collapsed or diverged net.
* SoftmaxWithLoss forward / backward against fp64 ``log_softmax`` with explicit masking on the
  shape grid of tests/test_loss_head_gpu.py.
"""
import pytest
import torch

from sparknet_amd import proto
from sparknet_amd.core.net import Net
from sparknet_amd.ops import ref

import loss_head_cases as lh


@pytest.mark.parametrize("name", sorted(lh.ACCURACY_CASES))
def test_accuracy_matches_pair_sort_oracle(name):
    x, labels, ks, ignore = lh.ACCURACY_CASES[name]
    for k in ks:
        acc = ref.accuracy(x, labels, k, ignore)
        hits, n = lh.check_accuracy(acc, x, labels, k, ignore)
        if k == x.shape[1] and n:
            assert float(acc) == 1.0          # k = C: every valid row is a hit
        if name.startswith("all_ignored"):
            assert n == 0 and float(acc) == 0.0


def test_accuracy_tie_and_nan_expectations():
    """The figures themselves, not only agreement with the oracle."""
    x, labels, _, _ = lh.ACCURACY_CASES["zeros_37x10"]
    for k in (1, 5):   # all scores equal: a hit iff the label is one of the k highest indices
        want = float((labels >= 10 - k).sum()) / 37
        assert abs(float(ref.accuracy(x, labels, k)) - want) < 1e-6
        assert want < 1.0
    x, labels, _, _ = lh.ACCURACY_CASES["tie_0_vs_64_6x65"]
    assert float(ref.accuracy(x, labels, 1)) == 0.0 and float(ref.accuracy(x, labels, 2)) == 1.0
    x, labels, _, _ = lh.ACCURACY_CASES["label_last_6x64"]
    assert float(ref.accuracy(x, labels, 1)) == 1.0
    # all-NaN rows behave like all-tied rows: labels 9 / 4 / 7 rank 0 / 5 / 2
    nan = torch.full((3, 10), float("nan"))
    lab = torch.tensor([9.0, 4.0, 7.0])
    for k, want in ((1, 1), (2, 1), (3, 2), (5, 2), (6, 3)):
        assert round(float(ref.accuracy(nan, lab, k)) * 3) == want, k


def test_accuracy_reads_labels_as_int_of_float():
    x = lh.half_logits(8, 10, seed=5)
    lab = lh.make_labels(8, 10, seed=5)
    assert float(ref.accuracy(x, lab + 0.75, 1)) == float(ref.accuracy(x, lab, 1))
    lh.check_accuracy(ref.accuracy(x, lab + 0.75, 1), x, lab, 1)


def _zero_ip_net(device="cpu", dtype=None):
    n = proto.parse_prototxt("""
      name: "collapsed"
      layer { name: "data" type: "Input" top: "data" java_data_param { shape { dim: 37 dim: 6 dim: 1 dim: 1 } } }
      layer { name: "label" type: "Input" top: "label" java_data_param { shape { dim: 37 } } }
      layer { name: "ip" type: "InnerProduct" bottom: "data" top: "ip"
              inner_product_param { num_output: 10 weight_filler { type: "constant" value: 0 }
                                    bias_filler { type: "constant" value: 0 } } }
      layer { name: "acc" type: "Accuracy" bottom: "ip" bottom: "label" top: "acc" accuracy_param { top_k: 1 } }
    """)
    return Net(n, phase=proto.TEST, device=device, dtype=dtype)


def collapsed_net_accuracy(device="cpu", dtype=None):
    """(accuracy of a net whose scores are all zero, fraction of labels equal to 9)"""
    net = _zero_ip_net(device, dtype)
    g = torch.Generator().manual_seed(11)
    labels = torch.randint(0, 10, (37,), generator=g).float()
    net.blob_by_name("data").set_nchw(torch.randn(37, 6, 1, 1, generator=g))
    net.blob_by_name("label").set_nchw(labels)
    net.forward()
    assert float(net.blob_by_name("ip").data.float().abs().max()) == 0.0
    return float(net.blob_by_name("acc").data.reshape(-1)[0]), float((labels == 9).float().mean())


def test_collapsed_net_reports_chance_not_100_percent():
    acc, want = collapsed_net_accuracy()
    assert 0.0 < want < 0.5
    assert abs(acc - want) < 1e-6, (acc, want)


@pytest.mark.parametrize("ignore", lh.IGNORES, ids=lambda v: f"ignore_{v}")
@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "nonorm"])
@pytest.mark.parametrize("mc", lh.GRID, ids=lh.grid_id)
def test_ref_softmax_loss_vs_fp64(mc, normalize, ignore):
    M, C = mc
    ignore = lh.resolve_ignore(ignore, C)
    outer = None if normalize else (M // 3 or 1)
    labels = lh.make_labels(M, C, ignore)
    x = lh.make_logits(M, C)
    loss, prob, norm = ref.softmax_loss_forward(x, labels, ignore, normalize, outer)
    for lw in (1.0, 0.3):
        r = lh.xent_ref64(x, labels, ignore, normalize, outer, lw)
        assert float(norm) == r["norm"]
        assert abs(float(loss) - r["loss"]) <= lh.loss_bound(r)
        assert bool(((prob.double() - r["prob"]).abs() <= lh.prob_bound(r)).all())
        dx = ref.softmax_loss_backward(prob, labels, torch.tensor(lw), norm, ignore, torch.bfloat16)
        assert bool(((dx.double() - r["dx"]).abs() <= lh.xent_dx_bound(r)).all())
        assert float(dx[~r["valid"]].float().abs().sum()) == 0.0


@pytest.mark.parametrize("ignore", [0, 255, -1])
def test_ref_all_rows_ignored(ignore):
    labels = lh.make_labels(37, 10, ignore, all_ignored=True)
    x = lh.make_logits(37, 10)
    for normalize in (True, False):
        loss, prob, norm = ref.softmax_loss_forward(x, labels, ignore, normalize, 12)
        assert float(loss) == 0.0
        assert float(norm) == (1.0 if normalize else 12.0)   # normaliser: max(count, 1)
        dx = ref.softmax_loss_backward(prob, labels, torch.tensor(0.3), norm, ignore)
        assert float(dx.abs().max()) == 0.0


@pytest.mark.parametrize("regime", ["saturated", "clamped", "confident"])
@pytest.mark.parametrize("mc", lh.GRID, ids=lh.grid_id)
def test_ref_softmax_loss_regimes(mc, regime):
    M, C = mc
    labels = lh.make_labels(M, C)
    x = lh.make_logits(M, C, regime, labels)
    r = lh.xent_ref64(x, labels)
    loss, prob, norm = ref.softmax_loss_forward(x, labels)
    assert abs(float(loss) - r["loss"]) <= lh.loss_bound(r)
    assert bool(((prob.double() - r["prob"]).abs() <= lh.prob_bound(r)).all())
    assert float(loss) >= 0.0
    if regime == "clamped":
        assert bool((r["nll"] == lh.NLL_MAX).all())
    if regime == "confident":
        assert r["loss"] < 1e-7 * C


def test_ref_softmax_vs_fp64():
    for M, C in lh.GRID:
        x = lh.make_logits(M, C)
        y64 = torch.softmax(x.double(), -1)
        y = ref.softmax_forward(x)
        assert y.dtype == torch.bfloat16
        assert bool(((y.double() - y64).abs() <= lh.softmax_y_bound(y64)).all())
        yb = y64.bfloat16()
        dy = lh.make_logits(M, C, seed=7)
        dx64 = lh.softmax_bwd_ref64(dy, yb)
        dx = ref.softmax_backward(dy, yb)
        assert bool(((dx.double() - dx64).abs() <= lh.softmax_bwd_bound(dy, yb, dx64)).all())
