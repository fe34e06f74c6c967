"""Scale and Bias on the GPU (csrc/kernels/bn_scale.hip, HIP only) against the fp32 CPU engine:
every configuration of tests/test_scale_bias_layers.py with bf16 blobs, and four of them with
fp32 device tensors (the fp32 device mode runs the same wrappers on fp32 tensors).  Inputs are
bf16-representable, so both devices read identical values."""
import pytest
import torch

from test_scale_bias_layers import CONFIGS, compare, cpu_result, rel, run_config

pytestmark = pytest.mark.gpu

BF16_TOL = 3e-2  # the bound of tests/test_layers_gpu.py
FP32_TOL = 1e-3  # the project's fp32 device-mode bound


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_bf16_matches_cpu(gpu, cfg):
    compare(run_config(cfg, "cuda"), cpu_result(cfg), BF16_TOL)


# a direct per-channel case on the vector path, an NCHW-copy case, a two-bottom case, the whole shape
@pytest.mark.parametrize("cfg", ["channel8_inplace", "middle_ch", "two_channel_bias_inplace", "eltwise"])
def test_fp32_tensors_match_cpu(gpu, cfg):
    compare(run_config(cfg, "cuda", dtype=torch.float32), cpu_result(cfg), FP32_TOL)


@pytest.mark.parametrize("cfg", ["channel8_inplace", "middle_ch", "bias_channel"])
def test_param_diffs_accumulate(gpu, cfg):
    ref = cpu_result(cfg)
    got = run_config(cfg, "cuda", accumulate=True)
    for a, b in zip(got["pdiff"], ref["pdiff"]):
        assert rel(a, b + 1.0) < BF16_TOL


def test_deterministic(gpu):
    a, b = run_config("channel8_inplace", "cuda"), run_config("channel8_inplace", "cuda")
    assert torch.equal(a["top"], b["top"]) and torch.equal(a["bdiff"][0], b["bdiff"][0])
    assert all(torch.equal(x, y) for x, y in zip(a["pdiff"], b["pdiff"]))
