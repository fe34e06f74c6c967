"""One solver step of shufflenet(groups=3, scale=0.25, crop=64, classes=10) at batch 4 (stage widths 48 /
144 / 240: 4 to 20 channels per group in the grouped 1x1 layers) on the GPU against the fp32 CPU engine,
with the conv_gpw=0 run as the yardstick (the rule of tests/test_mnasnet_gpu.py: within max(5 %, 1.5 x
the switch-off run's largest deviation), deviations relative to max(1, |cpu|)), for the loss and for
every learnable parameter after the update; and the launches of the grouped 1x1 layers."""
import pytest
import torch

from sparknet_amd import models

pytestmark = pytest.mark.gpu

B = 4
NET = dict(groups=3, scale=0.25, crop=64, classes=10, train_batch=B, test_batch=B)


def _step(dev, batch, w0=None):
    from sparknet_amd.core.solver import Solver
    from sparknet_amd.engine import fuse_relu
    sp = models.solver_for("shufflenet", **NET)
    sp.base_lr = 0.01
    solver = Solver(sp, device=torch.device(dev), seed=8, build_test_nets=False)
    net = solver.net
    if w0 is not None:
        net.flat_data.copy_(w0.to(net.flat_data.device))
        net.sync_compute()
        fuse_relu(net)
    start = net.flat_data.detach().cpu().clone()
    net.blob_by_name("data").set_nchw(batch[0])
    net.blob_by_name("label").set_nchw(batch[1])
    solver.stage_hyper()
    loss = float(solver.iteration())
    grouped = sum(l.type_name == "Convolution" and l.lp.convolution_param.group == NET["groups"] for l in net.layers)
    return start, loss, net.flat_data.detach().float().cpu().clone(), grouped


@pytest.fixture(scope="module")
def runs(gpu):
    from sparknet_amd.ops import _lib, hip
    g = torch.Generator().manual_seed(4)
    batch = (torch.randn(B, 3, 64, 64, generator=g), torch.randint(0, 10, (B, 1), generator=g).float())
    w0, *cpu = _step("cpu", batch)
    out, names = {"cpu": cpu}, []
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(hip, "call", lambda name, *args: (names.append(name), _lib.call(name, *args))[1])
        for key, feat in (("gpw", ""), ("off", "conv_gpw=0")):
            mp.setenv("SN_FEATURES", feat)
            del names[:]
            out[key] = _step(gpu, batch, w0)[1:]
            out["launches_" + key] = {n: names.count(n) for n in set(names) if n.startswith("conv_gpw")}
    finally:
        mp.undo()
    torch.cuda.synchronize()
    return out


def test_grouped_pointwise_layers_run_the_gpw_kernels(runs):
    """31 grouped 1x1 layers (two per unit, the first unit's first ungrouped), each with a bottom gradient."""
    n = runs["gpw"][2]
    assert n == 31
    assert runs["launches_gpw"] == {"conv_gpw_fwd": n, "conv_gpw_wgrad": n, "conv_gpw_wgrad_finalize": n,
                                    "conv_gpw_dgrad": n}, runs["launches_gpw"]
    assert runs["launches_off"] == {}


def test_one_step_matches_fp32_cpu(runs):
    (lc, wc, _), (lg, wg, _), (lo, wo, _) = runs["cpu"], runs["gpw"], runs["off"]
    dev = lambda a, b: abs(a - b) / max(1.0, abs(a))
    devs = lambda a, b: float(((a - b).abs() / a.abs().clamp(min=1.0)).max())
    bound_l, bound_w = max(0.05, 1.5 * dev(lc, lo)), max(0.05, 1.5 * devs(wc, wo))
    print("loss cpu", lc, "gpw", lg, "conv_gpw=0", lo, "bound", bound_l,
          "\nparameters: gpw", devs(wc, wg), "conv_gpw=0", devs(wc, wo), "bound", bound_w)
    assert dev(lc, lg) <= bound_l and devs(wc, wg) <= bound_w
