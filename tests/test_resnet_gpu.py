"""Net-level checks of the fused BatchNorm -> Scale -> ReLU path on resnet_cifar(n=1), batch 8:
the bf16 loss trajectory against the fp32 CPU engine, hipGraph replay against the eager step,
BranchStreams against the sequential order (the shortcut branch around the fused blob), and the
TEST-phase net (global statistics: the one-launch forward) against the CPU TEST net."""
import pytest
import torch

from sparknet_amd import models, proto

pytestmark = pytest.mark.gpu

B, STEPS = 8, 20


def _solver(dev, w0=None, fuse=True):
    from sparknet_amd.core.solver import Solver
    from sparknet_amd.engine import fuse_relu
    sp = models.solver_for("resnet_cifar", n=1, train_batch=B, test_batch=B)
    sp.base_lr = 0.01
    solver = Solver(sp, device=torch.device(dev), seed=8, build_test_nets=False)
    net = solver.net
    if w0 is not None:
        net.flat_data.copy_(w0.to(net.flat_data.device))
        net.sync_compute()
    if fuse and net.device.type == "cuda":
        fuse_relu(net)
    return solver


def _batches(n=2, seed=4):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, 3, 32, 32, generator=g), torch.randint(0, 10, (B, 1), generator=g).float())
            for _ in range(n)]


def _feed(net, batch):
    net.blob_by_name("data").set_nchw(batch[0])
    net.blob_by_name("label").set_nchw(batch[1])


def _trajectory(solver, batches):
    out = []
    for it in range(STEPS):
        _feed(solver.net, batches[it % len(batches)])
        solver.stage_hyper()
        out.append(float(solver.iteration()))
        solver.iter += 1
    return out


@pytest.fixture(scope="module")
def runs(gpu):
    """CPU, fused GPU and unfused GPU (fuse_bn_scale=0) trajectories from identical weights and
    batches, computed once for the module."""
    import os
    batches = _batches()
    cpu = _solver("cpu")
    w0 = cpu.net.flat_data.detach().clone()
    out = {"w0": w0, "cpu": _trajectory(cpu, batches)}
    fused = _solver(gpu, w0)
    out["n_fused"] = fused.net.bn_scale_fused
    out["fused"] = _trajectory(fused, batches)
    out["w_fused"] = fused.net.flat_data.detach().float().cpu().clone()
    old = os.environ.get("SN_FEATURES")
    os.environ["SN_FEATURES"] = "fuse_bn_scale=0"
    try:
        unfused = _solver(gpu, w0)
        out["n_unfused"] = unfused.net.bn_scale_fused
        out["unfused"] = _trajectory(unfused, batches)
    finally:
        if old is None:
            del os.environ["SN_FEATURES"]
        else:
            os.environ["SN_FEATURES"] = old
    torch.cuda.synchronize()
    return out


def test_loss_trajectory_matches_fp32_cpu(runs):
    """Per step within max(5 %, 1.5 x the unfused GPU run's largest deviation) of the CPU run;
    5 % is the window of tests/test_training_gpu.py."""
    assert runs["n_fused"] == 9 and runs["n_unfused"] == 0
    lc, lf, lu = runs["cpu"], runs["fused"], runs["unfused"]
    dev = lambda a, b: abs(a - b) / max(1.0, abs(a))
    d_unfused = max(dev(a, b) for a, b in zip(lc, lu))
    bound = max(0.05, 1.5 * d_unfused)
    print("cpu", lc, "\nfused", lf, "\nunfused", lu, "\nd_unfused", d_unfused)
    for i, (a, b) in enumerate(zip(lc, lf)):
        assert dev(a, b) <= bound, (i, a, b, bound)
    assert min(lc[-4:]) < lc[0] and min(lf[-4:]) < lf[0], (lc, lf)


def test_graph_replay_matches_eager(gpu, runs):
    """GraphStep capture of the fused net vs the eager fused step: flat weights (running
    statistics included) after 10 steps agree to 1e-5 of the largest weight."""
    from sparknet_amd.engine import LocalSGDTrainer, fuse_fc_updates
    batch = _batches(1, seed=6)[0]
    out = []
    for graph in (True, False):
        solver = _solver(gpu, runs["w0"])
        assert solver.net.bn_scale_fused == 9
        _feed(solver.net, batch)
        tr = LocalSGDTrainer(solver, None, tau=1000, use_graph=graph)
        if not graph:
            fuse_fc_updates(solver)
        while solver.iter < 10:
            tr.local_step()
        torch.cuda.synchronize()
        out.append(solver.net.flat_data.detach().clone())
    assert not torch.equal(out[1], runs["w0"].to(out[1].device))
    scale = out[1].abs().max().item()
    assert (out[0] - out[1]).abs().max().item() <= 1e-5 * scale


def test_branch_streams_match_sequential(gpu, runs):
    """3 streams: weights bitwise equal to the sequential order after 3 steps.  All three layers
    of a fused chain name one blob, so the blob lists alone order the shortcut branch."""
    from sparknet_amd.engine import BranchStreams
    batch = _batches(1, seed=7)[0]
    out = []
    for streams in (0, 3):
        solver = _solver(gpu, runs["w0"])
        net = solver.net
        _feed(net, batch)
        fb = net.forward_backward
        if streams:
            bs = BranchStreams(net, streams, star=True)
            assert bs.streams_used() > 1 and bs.streams_used(backward=True) > 1
            fb = bs.forward_backward
        for _ in range(3):
            solver.stage_hyper()
            net.clear_param_diffs(lazy=True)
            fb()
            net.finish_param_diffs()
            solver.update_params()
            solver.iter += 1
        torch.cuda.synchronize()
        out.append(net.flat_data.detach().clone())
    assert not torch.equal(out[0], runs["w0"].to(out[0].device))
    assert torch.equal(out[0], out[1])


def test_overlapped_update_waits_for_the_batchnorm(gpu, runs):
    """The per-layer update plan groups a fused Scale's params under its BatchNorm, the layer
    whose backward writes their gradients (it runs after the Scale layer's no-op backward)."""
    solver = _solver(gpu, runs["w0"])
    net = solver.net
    groups, _ = solver.overlap_plan(1)
    where = {seg[0]: li for li, segs in groups.items() for seg in segs}
    fused = [(li, l) for li, l in enumerate(net.layers) if l.type_name == "Scale" and l.fused_into is not None]
    assert len(fused) == 9
    for li, sc in fused:
        assert net.layers[li - 1] is sc.fused_into
        assert [where[p.offset] for p in sc.params] == [li - 1, li - 1]


def test_test_phase_net_matches_cpu(gpu, runs):
    from sparknet_amd.core.net import Net
    from sparknet_amd.engine import fuse_relu
    param = models.resnet_cifar(n=1, train_batch=B, test_batch=B)
    batch = _batches(1, seed=9)[0]
    logits = {}
    for dev in ("cpu", "cuda"):
        net = Net(param, phase=proto.TEST, device=dev)
        net.flat_data.copy_(runs["w_fused"].to(net.flat_data.device))
        net.sync_compute()
        if dev == "cuda":
            fuse_relu(net)
            bns = [l for l in net.layers if l.type_name == "BatchNorm"]
            assert len(bns) == 9 and all(l.use_global and l.fused_scale is not None for l in bns)
        _feed(net, batch)
        net.forward()
        logits[dev] = net.blob_by_name("fc").nchw().float().cpu().clone()
    a, b = logits["cuda"], logits["cpu"]
    assert (a - b).abs().max().item() / (b.abs().max().item() + 1e-6) < 3e-2
