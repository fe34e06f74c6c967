"""Net-level checks of the narrow-group kernels on resnext(reps=(1, 1, 1, 1), crop=32, classes=10),
batch 8: which launches its grouped 3x3 layers make, the bf16 loss trajectory against the fp32 CPU
engine with the conv_grouped=0 run as the yardstick, hipGraph replay against the eager step, and
the TEST-phase net against the CPU TEST net."""
import os

import pytest
import torch

from sparknet_amd import models, proto
from sparknet_amd.models import zoo

pytestmark = pytest.mark.gpu

B, STEPS = 8, 10
NET = dict(reps=(1, 1, 1, 1), crop=32, classes=10, train_batch=B, test_batch=B)
ROUTED = 3  # the grouped 3x3 of stages 2 to 4: Cg = 4, 8, 16; stage 5 has Cg = 32, which is not routed


def _solver(dev, w0=None):
    from sparknet_amd.core.solver import Solver
    from sparknet_amd.engine import fuse_relu
    sp = zoo.resnext50_solver(models.resnext(**NET))
    sp.base_lr = 0.01
    solver = Solver(sp, device=torch.device(dev), seed=8, build_test_nets=False)
    net = solver.net
    if w0 is not None:
        net.flat_data.copy_(w0.to(net.flat_data.device))
        net.sync_compute()
    if net.device.type == "cuda":
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
def runs(gpu, request):
    """CPU, grouped-kernel GPU and parent-path GPU (conv_grouped=0) trajectories from identical
    weights and batches, computed once for the module; the native launches are counted by name."""
    from sparknet_amd.ops import _lib, hip
    batches = _batches()
    cpu = _solver("cpu")
    w0 = cpu.net.flat_data.detach().clone()
    out = {"w0": w0, "cpu": _trajectory(cpu, batches)}
    old = os.environ.get("SN_FEATURES")
    names = []

    def call(name, *args):
        names.append(name)
        return _lib.call(name, *args)
    try:
        for key, feat in (("new", None), ("old", "conv_grouped=0")):
            if feat is None:
                os.environ.pop("SN_FEATURES", None)
            else:
                os.environ["SN_FEATURES"] = feat
            del names[:]
            hip.call = call
            solver = _solver(gpu, w0)
            out["n_fused_" + key] = solver.net.bn_scale_fused
            out[key] = _trajectory(solver, batches)
            out["launches_" + key] = {n: names.count(n) for n in set(names) if n.startswith("conv_grouped")}
            out["w_" + key] = solver.net.flat_data.detach().float().cpu().clone()
    finally:
        hip.call = _lib.call
        if old is None:
            os.environ.pop("SN_FEATURES", None)
        else:
            os.environ["SN_FEATURES"] = old
    torch.cuda.synchronize()
    return out


def test_grouped_layers_run_the_grouped_kernels(runs):
    """Three routed layers x 10 steps, each with a weight and a data gradient; none with the switch off."""
    assert runs["launches_new"] == {"conv_grouped_fwd": ROUTED * STEPS, "conv_grouped_wgrad": ROUTED * STEPS,
                                    "conv_grouped_dgrad": ROUTED * STEPS}, runs["launches_new"]
    assert runs["launches_old"] == {}
    assert runs["n_fused_new"] == runs["n_fused_old"] > 0


def test_loss_trajectory_matches_fp32_cpu(runs):
    """Per step within max(5 %, 1.5 x the conv_grouped=0 run's largest deviation) of the CPU
    run; 5 % is the window of tests/test_training_gpu.py."""
    lc, ld, lg = runs["cpu"], runs["new"], runs["old"]
    dev = lambda a, b: abs(a - b) / max(1.0, abs(a))
    d_group = max(dev(a, b) for a, b in zip(lc, lg))
    bound = max(0.05, 1.5 * d_group)
    print("cpu", lc, "\ngrouped kernels", ld, "\nconv_grouped=0", lg, "\nd_group", d_group)
    for i, (a, b) in enumerate(zip(lc, ld)):
        assert dev(a, b) <= bound, (i, a, b, bound)


def test_graph_replay_matches_eager(gpu, runs):
    """GraphStep capture (the weight-gradient workspace is allocated inside it) vs the eager
    step: flat weights after 10 steps agree to 1e-5 of the largest weight."""
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
    param = models.resnext(**NET)
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
