"""Convolution with ``bias_term: false`` on the GPU against the fp32 CPU engine — the building
blocks of a Caffe ResNet that no 2-D GPU test reached: a bias-free 3x3, a 1x1 with stride 2 and
a 7x7 / stride 2 / pad 3 stem on 3 channels.  Forward, dx and dW at the bound of the
convolution tests (tests/test_kernels_gpu.py: 2e-2, max-abs error over max-abs reference)."""
import pytest
import torch

from sparknet_amd import proto
from sparknet_amd.core.net import Net

pytestmark = pytest.mark.gpu

TOL = 2e-2

CASES = {
    # name: (N, C, H, W), num_output, kernel, stride, pad
    "3x3_pad1": ((2, 16, 8, 8), 16, 3, 1, 1),
    "1x1_stride2": ((2, 16, 8, 8), 32, 1, 2, 0),
    "7x7_stride2_pad3": ((2, 3, 20, 20), 16, 7, 2, 3),
}


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-6)


def _run(device, case, x, w, dy):
    shape, k, ks, stride, pad = CASES[case]
    dims = " ".join(f"dim: {d}" for d in shape)
    net = Net(proto.parse_prototxt(
        f'name: "c" force_backward: true\n'
        f'layer {{ name: "in" type: "Input" top: "x" java_data_param {{ shape {{ {dims} }} }} }}\n'
        f'layer {{ name: "conv" type: "Convolution" bottom: "x" top: "y" convolution_param {{ num_output: {k} '
        f'kernel_size: {ks} stride: {stride} pad: {pad} bias_term: false }} }}'), phase=proto.TRAIN, seed=3,
        device=device)
    layer, bvec, tvec = net.layers[-1], net.bottom_vecs[-1], net.top_vecs[-1]
    assert len(layer.params) == 1
    layer.params[0].set_caffe(w)
    net.sync_compute()
    net.flat_diff.zero_()
    bvec[0].set_nchw(x)
    layer.forward(bvec, tvec)
    top = tvec[0].nchw().float().cpu().clone()
    tvec[0].set_nchw(dy, diff=True)
    layer.backward(tvec, [True], bvec)
    return top, bvec[0].nchw(diff=True).float().cpu().clone(), layer.params[0].to_caffe(layer.params[0].diff).cpu()


@pytest.mark.parametrize("case", sorted(CASES))
def test_bias_free_convolution_matches_cpu(gpu, case):
    shape, k, ks, stride, pad = CASES[case]
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g).bfloat16().float()
    x = rnd(*shape)
    w = (0.2 * rnd(k, shape[1], ks, ks)).bfloat16().float()
    out = (shape[2] + 2 * pad - ks) // stride + 1
    dy = rnd(shape[0], k, out, out)
    ref = _run("cpu", case, x, w, dy)
    got = _run("cuda", case, x, w, dy)
    for name, a, b in zip(("top", "dx", "dW"), got, ref):
        assert a.shape == b.shape and _rel(a, b) < TOL, (name, _rel(a, b))
