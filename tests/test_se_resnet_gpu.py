"""Net-level checks of the squeeze-and-excitation kernels on se_resnet(reps=(1, 1, 1, 1), crop=32,
classes=10), batch 8: which launches its SE tails make, the bf16 loss trajectory against the fp32
CPU engine with the se_kernels=0 run as the yardstick, hipGraph replay against the eager step, and
the TEST-phase net against the CPU TEST net.

Launches per step.  The net has four blocks, one per stage, each with one Axpy: 4 nc_affine_fwd and
4 nc_affine_bwd (the gate and the block output both take a gradient).  At crop 32 conv1 (stride 2)
leaves 16 x 16 and pool1 (3 x 3 / 2) 8 x 8, so the SE pools see 8 x 8 = 64, 4 x 4, 2 x 2 and 1 x 1
positions and pool5 one: none has more than 64, every one stays on avepool_fwd and gap_fwd is not
launched at all.  At crop 64 the stage-2 pool sees 16 x 16 = 256 positions and is the only one on
gap_fwd (stage 3 has 8 x 8 = 64)."""
import os

import pytest
import torch

from sparknet_amd import models, proto
from sparknet_amd.models import zoo

pytestmark = pytest.mark.gpu

B, STEPS = 8, 10
NET = dict(reps=(1, 1, 1, 1), crop=32, classes=10, train_batch=B, test_batch=B)
BLOCKS = 4
NEW = ("gap_fwd", "nc_affine_fwd", "nc_affine_bwd")


def _solver(dev, w0=None):
    from sparknet_amd.core.solver import Solver
    from sparknet_amd.engine import fuse_relu
    sp = zoo.se_resnet50_solver(models.se_resnet(**NET))
    sp.base_lr = 0.01
    solver = Solver(sp, device=torch.device(dev), seed=8, build_test_nets=False)
    net = solver.net
    if w0 is not None:
        net.flat_data.copy_(w0.to(net.flat_data.device))
        net.sync_compute()
    if net.device.type == "cuda":
        fuse_relu(net)
    return solver


def _batches(n=2, seed=4, crop=32, batch=B):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(batch, 3, crop, crop, generator=g), torch.randint(0, 10, (batch, 1), generator=g).float())
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


class _Names:
    """Counts the native launches made through ops.hip.call / ops.layers_hip.call by name."""

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
        return {n: self.names.count(n) for n in NEW if n in self.names}


@pytest.fixture(scope="module")
def runs(gpu):
    """CPU, SE-kernel GPU and parent-path GPU (se_kernels=0) trajectories from identical weights
    and batches, computed once for the module; the native launches are counted by name."""
    batches = _batches()
    cpu = _solver("cpu")
    w0 = cpu.net.flat_data.detach().clone()
    out = {"w0": w0, "cpu": _trajectory(cpu, batches)}
    old = os.environ.get("SN_FEATURES")
    try:
        for key, feat in (("new", None), ("old", "se_kernels=0")):
            if feat is None:
                os.environ.pop("SN_FEATURES", None)
            else:
                os.environ["SN_FEATURES"] = feat
            with _Names() as names:
                solver = _solver(gpu, w0)
                out["n_fused_" + key] = solver.net.bn_scale_fused
                out[key] = _trajectory(solver, batches)
            out["launches_" + key] = names.new()
            out["pools_" + key] = names.names.count("pool_fwd")
            out["w_" + key] = solver.net.flat_data.detach().float().cpu().clone()
    finally:
        if old is None:
            os.environ.pop("SN_FEATURES", None)
        else:
            os.environ["SN_FEATURES"] = old
    torch.cuda.synchronize()
    return out


def test_se_tails_run_the_se_kernels(runs):
    """Four Axpy layers x 10 steps each way; no pool of this net has more than 64 positions, so all
    (pool1, four SE pools, pool5) run pool_fwd and none gap_fwd; nothing new with the switch off."""
    assert runs["launches_new"] == {"nc_affine_fwd": BLOCKS * STEPS, "nc_affine_bwd": BLOCKS * STEPS}, runs["launches_new"]
    assert runs["launches_old"] == {}
    assert runs["pools_new"] == runs["pools_old"] == (BLOCKS + 2) * STEPS
    assert runs["n_fused_new"] == runs["n_fused_old"] > 0


def test_only_the_pools_over_more_than_64_positions_run_gap_fwd(gpu, monkeypatch):
    """Crop 64: stage 2 pools 16 x 16 positions (gap_fwd), stage 3 8 x 8 = 64 and the rest fewer
    (pool_fwd); one forward-backward, and none with the switch off."""
    from sparknet_amd.core.net import Net
    param = models.se_resnet(**{**NET, "crop": 64, "train_batch": 2})
    batch = _batches(1, seed=3, crop=64, batch=2)[0]
    for feat, want in ((None, {"gap_fwd": 1, "nc_affine_fwd": BLOCKS, "nc_affine_bwd": BLOCKS}), ("se_kernels=0", {})):
        if feat is None:
            monkeypatch.delenv("SN_FEATURES", raising=False)
        else:
            monkeypatch.setenv("SN_FEATURES", feat)
        net = Net(param, phase=proto.TRAIN, device=gpu, seed=2)
        _feed(net, batch)
        with _Names() as names:
            net.forward()
            net.backward()
        assert names.new() == want, names.new()
        assert net.blob_by_name("res2a_se_pool").shape == (2, 256, 1, 1)
        assert names.names.count("pool_fwd") == BLOCKS + 2 - (1 if want else 0)
    torch.cuda.synchronize()


def test_loss_trajectory_matches_fp32_cpu(runs):
    """Per step within max(5 %, 1.5 x the se_kernels=0 run's largest deviation) of the CPU run;
    5 % is the window of tests/test_training_gpu.py."""
    lc, ld, lg = runs["cpu"], runs["new"], runs["old"]
    dev = lambda a, b: abs(a - b) / max(1.0, abs(a))
    d_old = max(dev(a, b) for a, b in zip(lc, lg))
    bound = max(0.05, 1.5 * d_old)
    print("cpu", lc, "\nse kernels", ld, "\nse_kernels=0", lg, "\nd_old", d_old)
    for i, (a, b) in enumerate(zip(lc, ld)):
        assert dev(a, b) <= bound, (i, a, b, bound)


def test_graph_replay_matches_eager(gpu, runs):
    """GraphStep capture vs the eager step: flat weights after 10 steps agree to 1e-5 of the
    largest weight."""
    from sparknet_amd.engine import LocalSGDTrainer, fuse_fc_updates
    batch = _batches(1, seed=6)[0]
    out = []
    for graph in (True, False):
        solver = _solver(gpu, runs["w0"])
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


def test_test_phase_net_matches_cpu(gpu, runs):
    from sparknet_amd.core.net import Net
    from sparknet_amd.engine import fuse_relu
    param = models.se_resnet(**NET)
    batch = _batches(1, seed=9)[0]
    logits = {}
    for dev in ("cpu", "cuda"):
        net = Net(param, phase=proto.TEST, device=dev)
        net.flat_data.copy_(runs["w_new"].to(net.flat_data.device))
        net.sync_compute()
        if dev == "cuda":
            fuse_relu(net)
            assert all(l.use_global for l in net.layers if l.type_name == "BatchNorm")
        _feed(net, batch)
        net.forward()
        logits[dev] = net.blob_by_name("fc10").nchw().float().cpu().clone()
    a, b = logits["cuda"], logits["cpu"]
    assert (a - b).abs().max().item() / (b.abs().max().item() + 1e-6) < 3e-2
