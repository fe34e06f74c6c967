"""Net-level checks of the wide-window depthwise kernels on mnasnet(alpha=0.25, crop=32, classes=10),
batch 8: the bf16 loss trajectory against the fp32 CPU engine with the conv_depthwise_wide=0 run as
the yardstick (the rule of tests/test_mobilenet_gpu.py), and the launches of the 5x5 layers."""
import pytest
import torch

from sparknet_amd import models

pytestmark = pytest.mark.gpu

B, STEPS = 8, 10
NET = dict(alpha=0.25, crop=32, classes=10, train_batch=B, test_batch=B)


def _trajectory(dev, batches, w0=None):
    from sparknet_amd.core.solver import Solver
    from sparknet_amd.engine import fuse_relu
    sp = models.solver_for("mnasnet", **NET)
    sp.base_lr = 0.01
    solver = Solver(sp, device=torch.device(dev), seed=8, build_test_nets=False)
    net = solver.net
    if w0 is not None:
        net.flat_data.copy_(w0.to(net.flat_data.device))
        net.sync_compute()
        fuse_relu(net)
    start, out = net.flat_data.detach().cpu().clone(), []
    for it in range(STEPS):
        net.blob_by_name("data").set_nchw(batches[it % len(batches)][0])
        net.blob_by_name("label").set_nchw(batches[it % len(batches)][1])
        solver.stage_hyper()
        out.append(float(solver.iteration()))
        solver.iter += 1
    return start, out


@pytest.fixture(scope="module")
def runs(gpu):
    """CPU, wide-kernel GPU and per-group GPU (conv_depthwise_wide=0) trajectories from identical weights
    and batches, computed once for the module; the native launches of the GPU runs by name."""
    from sparknet_amd.ops import _lib, hip
    g = torch.Generator().manual_seed(4)
    batches = [(torch.randn(B, 3, 32, 32, generator=g), torch.randint(0, 10, (B, 1), generator=g).float())
               for _ in range(2)]
    w0, cpu = _trajectory("cpu", batches)
    out, names = {"cpu": cpu}, []
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(hip, "call", lambda name, *args: (names.append(name), _lib.call(name, *args))[1])
        for key, feat in (("wide", ""), ("group", "conv_depthwise_wide=0")):
            mp.setenv("SN_FEATURES", feat)
            del names[:]
            out[key] = _trajectory(gpu, batches, w0)[1]
            out["launches_" + key] = {n: names.count(n) for n in set(names) if n.startswith("conv_xdw")}
    finally:
        mp.undo()
    torch.cuda.synchronize()
    return out


def test_5x5_layers_run_the_wide_kernels(runs):
    """10 depthwise 5x5 layers x 10 steps, each with a bottom gradient; none with the switch off."""
    assert runs["launches_wide"] == {"conv_xdw_fwd": 10 * STEPS, "conv_xdw_wgrad": 10 * STEPS,
                                     "conv_xdw_dgrad": 10 * STEPS}, runs["launches_wide"]
    assert runs["launches_group"] == {}


def test_loss_trajectory_matches_fp32_cpu(runs):
    """Per step within max(5 %, 1.5 x the conv_depthwise_wide=0 run's largest deviation) of the CPU run."""
    lc, lw, lg = runs["cpu"], runs["wide"], runs["group"]
    dev = lambda a, b: abs(a - b) / max(1.0, abs(a))
    bound = max(0.05, 1.5 * max(dev(a, b) for a, b in zip(lc, lg)))
    print("cpu", lc, "\nwide kernels", lw, "\nconv_depthwise_wide=0", lg, "\nbound", bound)
    for i, (a, b) in enumerate(zip(lc, lw)):
        assert dev(a, b) <= bound, (i, a, b, bound)
