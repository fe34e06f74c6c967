"""Host-side pieces of the fused loss head and the solver tail launch (no GPU): the index
maps the tail gathers / scatters through, and the predicate that decides whether a
SoftmaxWithLoss forward may also write its input gradient."""
import pytest
import torch

from sparknet_amd.ops import hip
from sparknet_amd.ops.spec import ConvSpec


def _conv(N, H, W, C, K, r, stride=1, pad=0, groups=1) -> ConvSpec:
    return ConvSpec(N, H, W, C, K, r, r, stride, stride, pad, pad, 1, 1, groups)


# conv1 of CaffeNet, GoogLeNet and VGG at the small sizes of tests/conv_trace_cases.py
FOLDS = {
    "caffenet": _conv(2, 19, 19, 3, 96, 11, stride=4),       # 11x11/4 -> 3x3 on 48 channels: taps 11 zero
    "googlenet": _conv(2, 8, 8, 3, 64, 7, stride=2, pad=3),  # 7x7/2 -> 4x4 on 16 channels
    "vgg": _conv(2, 8, 8, 3, 64, 3, pad=1),                  # f = 1: channels padded 3 -> 8
}


@pytest.mark.parametrize("name", FOLDS)
def test_fold_and_unfold_maps_are_inverse(name):
    s = FOLDS[name]
    f, cp, rf, sf, s2 = hip.s2d_plan(s)
    fold, unfold = hip.s2d_fold_map(s), hip.s2d_unfold_map(s)
    n, n2 = s.K * s.R * s.S * s.C, s.K * rf * sf * s2.C
    assert fold.dtype == unfold.dtype == torch.int32
    assert fold.numel() == n2 and unfold.numel() == n and n2 > n  # every geometry here pads
    # unfold is injective into the folded tensor, and fold undoes it
    u = unfold.long()
    assert int(u.min()) >= 0 and int(u.max()) < n2 and u.unique().numel() == n
    assert torch.equal(fold.long()[u], torch.arange(n))
    # fold's real entries are a permutation of the weights, and unfold undoes it; the rest is padding
    real = fold >= 0
    assert int(real.sum()) == n and int(fold.max()) < n
    assert torch.equal(u[fold[real].long()], torch.nonzero(real).reshape(-1))
    assert bool((fold[~real] == -1).all())
    # the scatter the tail does (w2[unfold[i]] = w[i] over zeros) is the fold itself
    w = torch.arange(1, n + 1, dtype=torch.float32)
    w2 = torch.zeros(n2).index_put_((u,), w)
    assert torch.equal(w2, torch.where(real, w[fold.clamp_min(0).long()], torch.zeros(n2)))


def test_fold_map_matches_the_folded_convolution():
    """The fold the maps describe is the one the space-to-depth plan means: a stride-f conv
    equals the stride-1 conv of the folded input with the folded weights."""
    s = FOLDS["caffenet"]
    f, cp, rf, sf, s2 = hip.s2d_plan(s)
    g = torch.Generator().manual_seed(0)
    w = torch.randn(s.K, s.R, s.S, s.C, generator=g)
    x = torch.randn(s.N, s.H, s.W, s.C, generator=g)
    fold = hip.s2d_fold_map(s).long()
    w2 = torch.where(fold >= 0, w.reshape(-1)[fold.clamp_min(0)], torch.zeros(())).reshape(s.K, rf, sf, s2.C)
    x2 = torch.zeros(s.N, s2.H, s2.W, s2.C)
    for dy in range(f):
        for dx in range(f):
            for c in range(s.C):
                src = x[:, dy::f, dx::f, c][:, :s2.H, :s2.W]
                x2[:, :src.shape[1], :src.shape[2], (dy * f + dx) * cp + c] = src
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=f)
    y2 = torch.nn.functional.conv2d(x2.permute(0, 3, 1, 2), w2.permute(0, 3, 1, 2))
    assert y.shape == y2.shape
    assert torch.allclose(y, y2, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("G,Kg,R,S,Cg", [(2, 128, 5, 5, 48), (1, 24, 3, 3, 40), (2, 8, 1, 1, 8)])
def test_flip_map_is_the_flip_transpose(G, Kg, R, S, Cg):
    m = hip.flip_map(G, Kg, R, S, Cg).long()
    n = G * Kg * R * S * Cg
    assert m.unique().numel() == n and int(m.min()) == 0 and int(m.max()) == n - 1
    w = torch.arange(n, dtype=torch.float32).reshape(G, Kg, R, S, Cg)
    wt = torch.empty(n).index_put_((m,), w.reshape(-1)).reshape(G, Cg, R, S, Kg)
    assert torch.equal(wt, w.flip(2, 3).permute(0, 4, 2, 3, 1))


def test_loss_head_predicate():
    ok = hip.loss_head_norm
    # no ignore_label, constant weight: the normaliser is M (normalize) or outer_num, at least 1
    assert ok(256, 256, None, True, True) == 256.0
    assert ok(12, 3, None, False, True) == 3.0
    assert ok(12, 0, None, False, True) == 1.0
    assert ok(1, 1, None, True, True) == 1.0
    # ignore_label: the valid count (normalize) and the zeroed rows are data
    assert ok(256, 256, 255, True, True) is None
    assert ok(256, 256, 0, True, True) is None     # label 0 ignored is still an ignore_label
    assert ok(256, 256, 255, False, True) is None
    # a loss weight that is not the constant the net wrote
    assert ok(256, 256, None, True, False) is None
    # float(M) must be exact
    assert ok(1 << 24, 1, None, True, True) is None
    assert ok((1 << 24) - 1, 1, None, True, True) == float((1 << 24) - 1)


def test_net_reports_a_constant_loss_weight_only_while_it_holds():
    """Net.constant_loss_diff: the loss top's diff counts as the constant loss weight only
    after prefill_loss_diffs wrote it and until anything writes it again."""
    from sparknet_amd import models, proto
    from sparknet_amd.core.net import Net
    n = models.lenet(train_batch=2, test_batch=2)
    net = Net(n, phase=proto.TRAIN, seed=1, device="cpu")
    (top, w), = net._loss_tops
    assert net.constant_loss_diff(top) is None          # nothing written yet
    net.prefill_loss_diffs()
    d = net.constant_loss_diff(top)
    assert d is top.diff and float(d) == w
    top.diff.fill_(0.25)                                 # a user's own loss weight
    assert net.constant_loss_diff(top) is None
    net.prefill_loss_diffs()
    assert net.constant_loss_diff(top) is top.diff
    stamp = net.weights_stamp()
    net.learnable_params[0].data[0] += 1.0               # a user's write to a weight blob
    assert net.weights_stamp() != stamp
    stamp = net.weights_stamp()
    net.sync_compute()
    assert net.weights_stamp() != stamp
