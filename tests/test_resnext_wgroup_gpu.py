"""Net-level check of the 32-wide grouped kernels on resnext(reps=(1, 1, 1, 1), crop=32, classes=10),
batch 8: res5a_branch2b (Cg = 32, stride 2) makes one launch of each per step, none with
conv_wgroup=0, and the bf16 loss trajectory stays as close to the fp32 CPU engine as
tests/test_resnext_gpu.py asks of the narrow-group kernels, with the conv_wgroup=0 run as the yardstick."""
import os

import pytest
import torch

import test_resnext_gpu as rg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs(gpu):
    from sparknet_amd.ops import _lib, hip
    batches = rg._batches()
    cpu = rg._solver("cpu")
    w0 = cpu.net.flat_data.detach().clone()
    out = {"cpu": rg._trajectory(cpu, batches)}
    old = os.environ.get("SN_FEATURES")
    names = []

    def call(name, *args):
        names.append(name)
        return _lib.call(name, *args)
    try:
        for key, feat in (("new", ""), ("old", "conv_wgroup=0")):
            os.environ["SN_FEATURES"] = feat
            del names[:]
            hip.call = call
            out[key] = rg._trajectory(rg._solver(gpu, w0), batches)
            out["launches_" + key] = {n: names.count(n) for n in set(names) if n.startswith("conv_wgroup")}
    finally:
        hip.call = _lib.call
        if old is None:
            os.environ.pop("SN_FEATURES", None)
        else:
            os.environ["SN_FEATURES"] = old
    torch.cuda.synchronize()
    return out


def test_stage5_runs_the_wgroup_kernels(runs):
    assert runs["launches_new"] == {"conv_wgroup_fwd": rg.STEPS, "conv_wgroup_wgrad": rg.STEPS,
                                    "conv_wgroup_dgrad": rg.STEPS}, runs["launches_new"]
    assert runs["launches_old"] == {}


def test_loss_trajectory_matches_fp32_cpu(runs):
    """Per step within max(5 %, 1.5 x the conv_wgroup=0 run's largest deviation) of the CPU run."""
    lc, ln, lo = runs["cpu"], runs["new"], runs["old"]
    dev = lambda a, b: abs(a - b) / max(1.0, abs(a))
    bound = max(0.05, 1.5 * max(dev(a, b) for a, b in zip(lc, lo)))
    print("cpu", lc, "\nwgroup kernels", ln, "\nconv_wgroup=0", lo)
    for i, (a, b) in enumerate(zip(lc, ln)):
        assert dev(a, b) <= bound, (i, a, b, bound)
