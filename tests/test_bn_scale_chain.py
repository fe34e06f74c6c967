"""The CPU chain BatchNorm -> Scale -> ReLU against torch.nn.functional.batch_norm + relu and
its autograd gradients (batch statistics and use_global_stats).

``run_chain`` is shared with tests/test_bn_scale_relu_gpu.py, where the same chain runs through
the fused kernels on the GPU and is compared against this CPU engine."""
import pytest
import torch
import torch.nn.functional as F

from sparknet_amd import proto
from sparknet_amd.core.net import Net

EPS = 1e-5
FACTOR = 3.7  # moving-average factor of the global-statistics cases


def chain_text(shape, *, relu=True, bias_term=True, global_stats=False, bn_inplace=False, scale_txt=None):
    blob = "x" if bn_inplace else "y"
    dims = " ".join(f"dim: {d}" for d in shape)
    stats = "true" if global_stats else "false"
    scale = scale_txt or (f'layer {{ name: "sc" type: "Scale" bottom: "{blob}" top: "{blob}" '
                          f'scale_param {{ bias_term: {"true" if bias_term else "false"} }} }}')
    return (f'name: "chain" force_backward: true\n'
            f'layer {{ name: "in" type: "Input" top: "x" java_data_param {{ shape {{ {dims} }} }} }}\n'
            f'layer {{ name: "bn" type: "BatchNorm" bottom: "x" top: "{blob}" '
            f'batch_norm_param {{ use_global_stats: {stats} eps: {EPS} }} }}\n{scale}\n'
            + (f'layer {{ name: "relu" type: "ReLU" bottom: "{blob}" top: "{blob}" }}\n' if relu else ""))


def chain_inputs(shape, seed=0, large_mean=False):
    """x = 2 randn + 0.5 and dy = randn rounded to bf16, gamma = 0.5 + 0.5 |randn|,
    beta = 0.5 randn, and running statistics for the global-statistics cases."""
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    x = torch.randn(shape, generator=g)
    x = (1000.0 + x) if large_mean else (2.0 * x + 0.5)
    return dict(x=x.bfloat16().float(), dy=torch.randn(shape, generator=g).bfloat16().float(),
                gamma=0.5 + 0.5 * torch.randn(C, generator=g).abs(), beta=0.5 * torch.randn(C, generator=g),
                rmean=FACTOR * (0.5 + 0.3 * torch.randn(C, generator=g)),
                rvar=FACTOR * 4.0 * (0.5 + torch.rand(C, generator=g)))


def run_chain(device, shape, *, relu=True, bias_term=True, global_stats=False, bn_inplace=False, propagate=True,
              grads="zero", dtype=None, fuse=False, inputs=None, text=None):
    """One forward + backward of the chain, layer by layer.  grads: "zero" (accumulate into
    zeros), "acc" (accumulate into ones) or "lazy" (Net.clear_param_diffs(lazy=True) over
    garbage: the first write must store).  Returns fp32 CPU tensors and the fused-chain count."""
    from sparknet_amd import engine
    inp = inputs or chain_inputs(shape)
    net = Net(proto.parse_prototxt(text or chain_text(shape, relu=relu, bias_term=bias_term,
                                                      global_stats=global_stats, bn_inplace=bn_inplace)),
              phase=proto.TRAIN, seed=3, device=device, dtype=dtype)
    fused = engine.fuse_bn_scale_relu(net) if fuse else 0
    bn = net.layers[net.layer_names.index("bn")]
    sc = net.layers[net.layer_names.index("sc")]
    dev = net.flat_data.device
    if global_stats:
        bn.mean.data.copy_(inp["rmean"].to(dev))
        bn.var.data.copy_(inp["rvar"].to(dev))
        bn.factor.data.fill_(FACTOR)
    if sc.scale is not None:
        sc.scale.data.copy_(inp["gamma"].to(dev))
    if sc.bias is not None:
        sc.bias.data.copy_(inp["beta"].to(dev))
    net.sync_compute()
    if grads == "lazy":
        net.flat_diff.fill_(7.0)
        net.clear_param_diffs(lazy=True)
    else:
        net.flat_diff.fill_(1.0 if grads == "acc" else 0.0)
    net.blob_by_name("x").set_nchw(inp["x"])
    first = net.layer_names.index("bn")
    for li in range(first, len(net.layers)):
        net.layers[li].forward(net.bottom_vecs[li], net.top_vecs[li])
    top_blob = net.top_vecs[-1][0]
    top = top_blob.nchw().float().cpu().clone()
    top_blob.set_nchw(inp["dy"], diff=True)
    for li in range(len(net.layers) - 1, first - 1, -1):
        pd = [propagate] if li == first else net.bottom_need_backward[li]
        net.layers[li].backward(net.top_vecs[li], pd, net.bottom_vecs[li])
    if grads == "lazy":
        net.finish_param_diffs()
    out = dict(top=top, fused=fused, net=net,
               dx=net.blob_by_name("x").nchw(diff=True).float().cpu().clone() if propagate else None,
               dgamma=sc.scale.diff.float().cpu().clone() if sc.scale is not None else None,
               dbeta=sc.bias.diff.float().cpu().clone() if sc.bias is not None else None,
               running=[p.data.float().cpu().clone() for p in (bn.mean, bn.var, bn.factor)])
    return out


def torch_oracle(shape, *, relu, bias_term, global_stats, inputs=None):
    inp = inputs or chain_inputs(shape)
    x = inp["x"].clone().requires_grad_(True)
    gamma = inp["gamma"].clone().requires_grad_(True)
    beta = inp["beta"].clone().requires_grad_(True) if bias_term else None
    if global_stats:
        y = F.batch_norm(x, inp["rmean"] / FACTOR, inp["rvar"] / FACTOR, gamma, beta, training=False, eps=EPS)
    else:
        y = F.batch_norm(x, None, None, gamma, beta, training=True, eps=EPS)
    z = y
    if relu:
        y = F.relu(y)
    (y * inp["dy"]).sum().backward()
    return dict(top=y.detach(), z=z.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad if bias_term else None)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-6)


@pytest.mark.parametrize("shape", [(4, 5, 6, 3), (16, 10)])
@pytest.mark.parametrize("global_stats", [False, True])
@pytest.mark.parametrize("relu,bias_term,bn_inplace", [(True, True, False), (False, True, True), (True, False, True)])
def test_cpu_chain_matches_torch(shape, global_stats, relu, bias_term, bn_inplace):
    got = run_chain("cpu", shape, relu=relu, bias_term=bias_term, global_stats=global_stats, bn_inplace=bn_inplace)
    ref = torch_oracle(shape, relu=relu, bias_term=bias_term, global_stats=global_stats)
    for key in ("top", "dx", "dgamma", "dbeta"):
        if ref[key] is not None:
            assert rel(got[key], ref[key]) < 1e-5, (key, rel(got[key], ref[key]))
    inp = chain_inputs(shape)
    if global_stats:  # the running blobs are read, not updated
        assert torch.equal(got["running"][0], inp["rmean"]) and float(got["running"][2]) == pytest.approx(FACTOR)
    else:  # one update from zero: factor 1, the batch mean, the unbiased batch variance
        dims = [d for d in range(len(shape)) if d != 1]
        assert float(got["running"][2]) == 1.0
        assert rel(got["running"][0], inp["x"].mean(dim=dims)) < 1e-5
        assert rel(got["running"][1], inp["x"].var(dim=dims, unbiased=True)) < 1e-5
