"""The fused loss head (softmax_xent_fwd_bwd) and the solver tail launch (sn_solver_tail)
against the separate launches they replace, bitwise, and a small net through GraphStep with
both switches on and off, with and without a weight write between steps (the stale-copy
test: the copies the tail keeps must be rebuilt after any change it did not make)."""
import pytest
import torch

from sparknet_amd import models, proto
from sparknet_amd.dsl import (ConvolutionLayer, InnerProductLayer, NetParam, PoolingLayer, ReLULayer,
                              SoftmaxWithLoss)
from sparknet_amd.ops import hip
from sparknet_amd.ops.spec import ConvSpec

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


# ------------------------------------------------------------------------------------------
# 1. fused loss kernel vs softmax_xent_fwd + xent_reduce + softmax_xent_bwd
# ------------------------------------------------------------------------------------------

SHAPES = [(1, 2), (3, 5), (4, 64), (5, 65), (7, 1000), (256, 1000)]


def _logits(M, C, dev):
    g = torch.Generator().manual_seed(100 * M + C)
    x = (torch.randn(M, C, generator=g) * 4).to(BF16)
    lab = torch.randint(0, C, (M,), generator=g)
    lab[0] = 0                      # class 0
    lab[-1] = C - 1                 # class C - 1 (M = 1: the one row)
    if M > 2:
        x[1] = 1.5                  # a row whose logits are all equal
    return x.to(dev), lab.float().to(dev)


@pytest.mark.parametrize("lw", [1.0, 0.3])
@pytest.mark.parametrize("M,C", SHAPES)
def test_fused_loss_head_matches_three_launches(gpu, M, C, lw):
    x, lab = _logits(M, C, gpu)
    w = torch.full((), lw, dtype=torch.float32, device=gpu)
    for normalize, outer in ((True, M), (False, max(1, M // 2))):
        loss0, prob0, norm0 = hip.softmax_loss_forward(x, lab, None, normalize, outer)
        dx0 = hip.softmax_loss_backward(prob0, lab, w, norm0, None, BF16)
        loss1, prob1, norm1, dx1, rows = hip.softmax_loss_forward_backward(x, lab, w, normalize, outer)
        assert float(norm1) == hip.loss_head_norm(M, outer, None, normalize, True)
        assert torch.equal(prob0, prob1)
        assert torch.equal(loss0, loss1) and torch.equal(norm0, norm1)
        assert torch.equal(dx0.view(torch.int16), dx1.view(torch.int16))
        # the row losses, through the sum the solver tail's block 0 runs in xent_reduce's place
        loss2, _, norm2, dx2, rows2 = hip.softmax_loss_forward_backward(x, lab, w, normalize, outer, reduce=False)
        assert torch.equal(rows, rows2) and torch.equal(dx1.view(torch.int16), dx2.view(torch.int16))
        _tail_only_loss(gpu, (rows2, M, normalize, outer, loss2, norm2))
        assert torch.equal(loss0, loss2) and torch.equal(norm0, norm2)
    assert torch.isfinite(prob1).all() and torch.isfinite(dx1.float()).all()


def _tail_only_loss(dev, loss, rng=None):
    """A tail launch with no parameters: only block 0's loss sum (and RNG advance)."""
    t = hip.solver_tail_tables([], 0, dev)
    z = torch.zeros(64, dtype=torch.float32, device=dev)
    hip.solver_tail(0, z, z.clone(), [z.clone()], torch.zeros(64, dtype=BF16, device=dev), t,
                    torch.zeros(16, dtype=torch.float32, device=dev), False, rng, loss)


def test_tail_loss_sum_past_one_pass_of_xent_reduce(gpu):
    """More rows than xent_reduce's 1024 threads: its threads loop, and so must the tail's."""
    M, C = 2500, 3
    x, lab = _logits(M, C, gpu)
    w = torch.ones((), dtype=torch.float32, device=gpu)
    loss0, _, norm0 = hip.softmax_loss_forward(x, lab, None, True, M)
    loss1, _, norm1, _, rows = hip.softmax_loss_forward_backward(x, lab, w, True, M, reduce=False)
    _tail_only_loss(gpu, (rows, M, True, M, loss1, norm1))
    assert torch.equal(loss0, loss1) and torch.equal(norm0, norm1)


def test_ignore_label_takes_the_unfused_path(gpu):
    """A SoftmaxWithLoss layer with ignore_label, offered the fused head, keeps its three
    launches and matches a layer that was never offered it."""
    from sparknet_amd.core.net import Net
    from sparknet_amd.engine import fuse_loss_head

    def run(fuse, ignore):
        loss = SoftmaxWithLoss("loss", ["ip", "label"])
        if ignore is not None:
            loss.loss_param.ignore_label = ignore
        n = NetParam("t", *models.zoo.data_layers(5, 5, 3, 4, 4),
                     InnerProductLayer("ip", ["data"], 9, weight_filler={"type": "gaussian", "std": 0.5}), loss)
        net = Net(n, phase=proto.TRAIN, seed=4, device=gpu)
        head = fuse_loss_head(net) if fuse else None
        g = torch.Generator().manual_seed(2)
        net.blob_by_name("data").set_nchw(torch.randn(5, 3, 4, 4, generator=g))
        net.blob_by_name("label").set_nchw(torch.tensor([[0.0], [8.0], [3.0], [3.0], [1.0]]))
        layer = net.layers[-1]
        out = []
        for _ in range(2):  # the first pass fills the loss weight; the second may fuse
            net.clear_param_diffs()
            l = net.forward()
            taken = layer._dx is not None
            net.backward()
            out.append((l.clone(), net.blob_by_name("ip").diff.clone(), taken))
        return head, out

    _, ref = run(False, 3)
    head, got = run(True, 3)
    assert head is not None and not got[0][2] and not got[1][2]
    for (l0, d0, _), (l1, d1, _) in zip(ref, got):
        assert torch.equal(l0, l1) and torch.equal(d0.view(torch.int16), d1.view(torch.int16))
    # without ignore_label the same net does fuse, from the pass after the loss weight is in place
    _, ref = run(False, None)
    _, got = run(True, None)
    assert [t for _, _, t in got] == [False, True]
    for (l0, d0, _), (l1, d1, _) in zip(ref, got):
        assert torch.equal(l0, l1) and torch.equal(d0.view(torch.int16), d1.view(torch.int16))


# ------------------------------------------------------------------------------------------
# 2. sn_solver_tail vs s2d_weight_grad + solver_update + s2d_weight + flip_weights_multi + advance_rng
# ------------------------------------------------------------------------------------------

CONV1 = ConvSpec(2, 19, 19, 3, 96, 11, 11, 4, 4, 0, 0, 1, 1, 1)     # folds with zero-padded taps
CONV2 = ConvSpec(2, 9, 9, 96, 256, 5, 5, 1, 1, 2, 2, 1, 1, 2)       # grouped 5x5
CONV3 = ConvSpec(2, 5, 5, 40, 24, 3, 3, 1, 1, 1, 1, 1, 1, 1)        # 8640 weights: not a multiple of 4 * 256


def _align(n):
    return -(-n // 64) * 64


@pytest.mark.parametrize("kind,l1", [(0, False), (1, False), (0, True), (1, True)])
def test_solver_tail_matches_separate_launches(gpu, kind, l1):
    dev = gpu
    specs = [CONV1, CONV2, CONV3]
    segs, off = [], 0
    for s in specs:
        n = s.K * s.R * s.S * s.Cg
        segs.append((off, n, 1.0, 1.0))
        off += _align(n)
        segs.append((off, s.K, 2.0, 0.0))  # bias: lr_mult / decay_mult != 1
        off += _align(s.K)
    total = off
    assert segs[4][1] % 1024 != 0
    g = torch.Generator().manual_seed(5 + kind)
    real = torch.zeros(total, dtype=torch.bool)
    for o, n, _, _ in segs:
        real[o:o + n] = True
    master = torch.where(real, torch.randn(total, generator=g) * 0.05, torch.zeros(())).to(dev)
    hist = torch.where(real, torch.randn(total, generator=g) * 0.01, torch.zeros(())).to(dev)
    diff = torch.where(real, torch.randn(total, generator=g) * 0.1, torch.zeros(())).to(dev)
    hyper = torch.zeros(16, dtype=torch.float32)
    hyper[0], hyper[1], hyper[2], hyper[4] = 0.01, 0.9, 5e-4, 1.0  # rate, momentum, decay, 1 / iter_size
    hyper = hyper.to(dev)
    f, cp, rf, sf, s2 = hip.s2d_plan(CONV1)
    k2 = rf * sf * s2.C
    dw2 = (torch.randn(CONV1.K, k2, generator=g) * 0.1).to(dev)
    n1 = segs[0][1]

    def flip_items(shadow, wts):
        items = []
        for (o, n, _, _), s, wt in zip(segs[2::2], specs[1:], wts):
            items.append((shadow[o:o + n].view(s.K, s.R, s.S, s.Cg), wt, s.groups, s.Kg, s.R, s.S, s.Cg))
        return items

    def new_wts(fill):
        return [torch.full((s.groups, s.Cg, s.R, s.S, s.Kg), fill, dtype=BF16, device=dev) for s in specs[1:]]

    # the separate launches
    m0, h0, d0 = master.clone(), hist.clone(), diff.clone()
    sh0 = m0.to(BF16)
    rng0 = torch.tensor([1234, 7], dtype=torch.int64, device=dev)
    hip.call("s2d_weight_grad", dw2, d0[:n1], CONV1.K, CONV1.R, CONV1.S, CONV1.C, f, cp, rf, sf, 0)
    hip.advance_rng(rng0)
    hip.solver_update(kind, m0, d0, [h0], sh0, hip.solver_tables(segs, total, dev), hyper, l1, False)
    w2_0 = torch.empty((CONV1.K, rf, sf, s2.C), dtype=BF16, device=dev)
    hip.call("s2d_weight", sh0[:n1], w2_0, CONV1.K, CONV1.R, CONV1.S, CONV1.C, f, cp, rf, sf)
    wt0 = new_wts(3.0)
    hip.FlipBatch(flip_items(sh0, wt0), dev).run()

    # one tail launch: conv1's flat gradient is never read (poisoned), its w2 starts from zeros
    m1, h1, d1 = master.clone(), hist.clone(), diff.clone()
    d1[:n1] = float("nan")
    sh1 = m1.to(BF16)
    rng1 = torch.tensor([1234, 7], dtype=torch.int64, device=dev)
    w2_1 = torch.zeros((CONV1.K, rf, sf, s2.C), dtype=BF16, device=dev)
    wt1 = new_wts(-5.0)
    extras = {segs[0][0]: (hip.s2d_unfold_map(CONV1), dw2, w2_1)}
    for (o, n, _, _), s, wt in zip(segs[2::2], specs[1:], wt1):
        extras[o] = (hip.flip_map(s.groups, s.Kg, s.R, s.S, s.Cg), None, wt)
    t = hip.solver_tail_tables(segs, total, dev, extras)
    assert t["n"] > hip.solver_tables(segs, total, dev)["n"]  # the mapped segments run as smaller chunks
    hip.solver_tail(kind, m1, d1, [h1], sh1, t, hyper, l1, rng1, None)
    torch.cuda.synchronize()

    assert torch.equal(m0, m1) and torch.equal(h0, h1)
    assert torch.equal(sh0.view(torch.int16), sh1.view(torch.int16))
    assert torch.equal(w2_0.view(torch.int16), w2_1.view(torch.int16))
    for a, b in zip(wt0, wt1):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert rng0.tolist() == rng1.tolist() == [1234, 8]
    assert not torch.equal(m1, master) and torch.isfinite(m1).all()


# ------------------------------------------------------------------------------------------
# 3. conv1 -> relu -> pool -> grouped conv -> fc -> loss through GraphStep, switches on / off
# ------------------------------------------------------------------------------------------

def _small_net():
    gs = lambda std: {"type": "gaussian", "std": std}  # noqa: E731
    wb = [(1.0, 1.0), (2.0, 0.0)]
    return NetParam("tail", *models.zoo.data_layers(2, 2, 3, 35, 35),
                    ConvolutionLayer("conv1", ["data"], (11, 11), 96, stride=4, weight_filler=gs(0.05), param=wb),
                    ReLULayer("relu1", ["conv1"], in_place=True),
                    PoolingLayer("pool1", ["conv1"], kernel=(3, 3), stride=(2, 2)),
                    ConvolutionLayer("conv2", ["pool1"], (5, 5), 32, pad=2, group=2, weight_filler=gs(0.05),
                                     param=wb),
                    ReLULayer("relu2", ["conv2"], in_place=True),
                    InnerProductLayer("fc", ["conv2"], 16, weight_filler=gs(0.05), param=wb),
                    SoftmaxWithLoss("loss", ["fc", "label"]))


OFF = "solver_tail=0,fuse_loss_head=0"
ALL = "solver_tail_flips=1"  # the tail with the weight flips too (opt-in); "": the defaults


def _train(monkeypatch, feats: str, write: str | None, solver_type="SGD"):
    from sparknet_amd.core.net import Net
    from sparknet_amd.core.solver import Solver
    from sparknet_amd.engine import GraphStep, fuse_relu
    monkeypatch.setenv("SN_FEATURES", feats)
    sp = models.zoo._solver(_small_net(), base_lr=0.005, lr_policy="fixed", momentum=0.9, weight_decay=5e-3,
                            max_iter=100, type=solver_type)
    solver = Solver(sp, device=torch.device("cuda:0"), seed=3, build_test_nets=False)
    net = solver.net
    fuse_relu(net)
    g = torch.Generator().manual_seed(1)
    batches = [(torch.randn(2, 3, 35, 35, generator=g), torch.tensor([[1.0], [13.0]])) for _ in range(6)]
    it = iter(batches)

    def pre():
        x, y = next(it)
        net.blob_by_name("data").set_nchw(x)
        net.blob_by_name("label").set_nchw(y)

    step = GraphStep(solver, warmup=1, pre=pre, overlap=False, fuse_fc=True)
    losses = []
    for k in range(3):  # warm-up, capture + replay, replay
        if k == 2 and write == "copy_from":
            other = Net(_small_net(), phase=proto.TRAIN, seed=77, device="cpu")
            net.copy_trained_layers_from(other.to_proto())
        elif k == 2 and write == "blob":
            net.layer_by_name("conv1").weight.data.mul_(0.5)  # a user's write to a blob ...
            net.layer_by_name("conv2").weight.data.add_(0.01)
            net.sync_compute()                                # ... made visible to the bf16 kernels
        losses.append(step.step().clone())
    torch.cuda.synchronize()
    return solver, step, torch.stack(losses)


@pytest.mark.parametrize("feats", ["", ALL])
@pytest.mark.parametrize("write", [None, "copy_from", "blob"])
def test_graph_step_with_and_without_the_tail(gpu, monkeypatch, write, feats):
    s0, st0, l0 = _train(monkeypatch, OFF, write)
    s1, st1, l1 = _train(monkeypatch, feats, write)
    assert st0.tail is None and getattr(s0.net, "_loss_head", None) is None
    tail = st1.tail
    assert tail is not None and len(tail.folds) == 1 and tail.folds[0][2] is not None
    assert tail.head.defer_to is s1.net.layers[-1]
    assert (tail.flip_batch is not None and len(tail.flip_batch.items) == 1) if feats == ALL else tail.flip_batch is None
    assert tail.refreshes == (1 if write is None else 2)  # at set-up, and after the outside write
    assert torch.isfinite(l0).all() and len(set(l0.tolist())) == 3
    assert torch.equal(l0, l1)
    assert torch.equal(s0.net.flat_data, s1.net.flat_data)
    assert torch.equal(s0.history[0], s1.history[0])
    assert torch.equal(s0.net.flat_compute.view(torch.int16), s1.net.flat_compute.view(torch.int16))
    assert s0.net.ctx.rng_state.tolist() == s1.net.ctx.rng_state.tolist()
    # the copies the tail keeps are the fold / flip of the weights as they are now
    layer, w2, _, s = tail.folds[0]
    fold = hip.s2d_fold_map(s).to(gpu).long()
    w = layer.weight.compute.reshape(-1)
    want = torch.where(fold >= 0, w[fold.clamp_min(0)], torch.zeros((), dtype=BF16, device=gpu))
    assert torch.equal(w2.reshape(-1).view(torch.int16), want.view(torch.int16))
    if tail.flip_batch is not None:
        w, wt, G, Kg, R, S, Cg = tail.flip_batch.items[0]
        want = torch.empty_like(wt).reshape(-1)
        want[hip.flip_map(G, Kg, R, S, Cg).to(gpu).long()] = w.reshape(-1)
        assert torch.equal(wt.reshape(-1).view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("feats", ["", ALL])
def test_a_missed_invalidation_would_show(gpu, monkeypatch, feats):
    """The stale-copy test has teeth: with the staleness check blinded after set-up, the same
    weight write leaves the step on the old folded / flipped weights and the results differ."""
    from sparknet_amd.engine import SolverTail
    s0, _, l0 = _train(monkeypatch, OFF, "blob")
    monkeypatch.setattr(SolverTail, "stale", lambda self: self.stamp is None)
    s1, st1, l1 = _train(monkeypatch, feats, "blob")
    assert st1.tail.refreshes == 1
    assert torch.equal(l0[:2], l1[:2]) and not torch.equal(s0.net.flat_data, s1.net.flat_data)


def test_graph_step_tail_nesterov(gpu, monkeypatch):
    s0, _, l0 = _train(monkeypatch, OFF, None, "Nesterov")
    s1, st1, l1 = _train(monkeypatch, ALL, None, "Nesterov")
    assert st1.tail is not None
    assert torch.equal(l0, l1) and torch.equal(s0.net.flat_data, s1.net.flat_data)
    assert torch.equal(s0.history[0], s1.history[0])


def test_eager_iteration_between_replays_marks_the_copies_stale(gpu, monkeypatch):
    """A plain solver iteration outside the captured step changes the weights without the tail:
    the next replay must rebuild the copies first."""
    s1, st1, _ = _train(monkeypatch, ALL, None)
    n = st1.tail.refreshes
    s1.net.blob_by_name("data").set_nchw(torch.ones(2, 3, 35, 35))
    s1.iteration()
    assert st1.tail.stale()
    st1.step()
    torch.cuda.synchronize()
    assert st1.tail.refreshes == n + 1 and not st1.tail.stale()
