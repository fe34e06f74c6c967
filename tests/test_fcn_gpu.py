"""The Crop kernel bitwise against the slice, and one forward / backward of fcn8s(width=0.125, crop=64) at
batch 2 on the GPU: its launches and its loss against the fp32 CPU engine."""
import pytest
import torch

from sparknet_amd import models, proto

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("C, c, oc", [(16, 8, 8), (21, 21, 0), (21, 5, 3)])  # the 16-byte path, and not
def test_crop_kernel_is_the_slice(C, c, oc, gpu):
    from sparknet_amd.ops import hip
    x = torch.randn(2, 9, 11, C).to(torch.bfloat16).to(gpu)
    offsets, shape = (0, 2, 3, oc), (2, 5, 7, c)
    window = tuple(slice(o, o + n) for o, n in zip(offsets, shape))
    y = hip.crop_window(x, offsets, shape)
    assert torch.equal(y, x[window])
    dy = torch.randn(shape).to(torch.bfloat16).to(gpu)
    want = torch.zeros_like(x)
    want[window] = dy
    assert torch.equal(hip.crop_window_backward(dy, offsets, tuple(x.shape)), want)


def _run(dev, w0, data, label):
    from sparknet_amd.core.net import Net
    net = Net(models.fcn8s(width=0.125, crop=64, train_batch=2), phase=proto.TRAIN, device=torch.device(dev), seed=5)
    if w0 is not None:
        net.flat_data.copy_(w0.to(net.flat_data.device))
        net.sync_compute()
    start = net.flat_data.detach().cpu().clone()
    net.blob_by_name("data").set_nchw(data)
    net.blob_by_name("label").set_nchw(label)
    loss = float(net.forward())
    net.backward()
    return start, loss


@pytest.fixture(scope="module")
def runs(gpu):
    from sparknet_amd.ops import _lib, hip
    g = torch.Generator().manual_seed(6)
    data, label = torch.randn(2, 3, 64, 64, generator=g), torch.randint(0, 21, (2, 1, 64, 64), generator=g).float()
    label[:, :, :5] = 255
    w0, cpu = _run("cpu", None, data, label)
    out, names = {"cpu": cpu}, []
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(hip, "call", lambda name, *args: (names.append(name), _lib.call(name, *args))[1])
        for key, feat in (("updw", ""), ("off", "deconv_dw=0")):
            mp.setenv("SN_FEATURES", feat)
            del names[:]
            out[key] = _run(gpu, w0, data, label)[1]
            out["launches_" + key] = {n: names.count(n) for n in set(names) if n.startswith("conv_updw")}
    finally:
        mp.undo()
    torch.cuda.synchronize()
    return out


def test_fcn8s_launches(runs):
    """Three upsampling layers forward; each has learnable layers below it, so each propagates a bottom
    gradient; upscore8 has lr_mult 0, so only two weight gradients."""
    assert runs["launches_updw"] == {"conv_updw_fwd": 3, "conv_updw_dgrad": 3, "conv_updw_wgrad": 2}, runs["launches_updw"]
    assert runs["launches_off"] == {}


def test_fcn8s_loss_matches_fp32_cpu(runs):
    """The yardstick is the deconv_dw=0 run's deviation from the fp32 CPU loss; the new route gets twice
    that, both being bf16 storage error of the same net with differently ordered sums.  Measured on an
    MI355X: CPU loss 74178.77, both GPU runs 74144.12, so both deviations are 34.65."""
    lc, lg, lo = runs["cpu"], runs["updw"], runs["off"]
    print("loss cpu", lc, "updw", lg, "deconv_dw=0", lo, "deviations", abs(lg - lc), abs(lo - lc))
    assert abs(lg - lc) <= 2 * abs(lo - lc)
