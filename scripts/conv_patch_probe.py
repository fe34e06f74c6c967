#!/usr/bin/env python3
"""The patch-resident 5x5 data gradient (csrc/kernels/conv_patch.hip) against the implicit grouped
GEMM (``SN_FEATURES=conv_patch=0``) on CaffeNet's conv2: 27 x 27, two groups of 128 -> 48 channels,
batch 256.  Both paths run through ``hip.conv_backward`` with pre-flipped weights, a gate and a
destination buffer, as the training step calls them; they alternate on the same build and each
figure is the median of several passes of device events over random operands.  TF/s counts the
2 M N K of the product; the L2 -> LDS rate is what the GEMM's im2col operand must move (every dy
byte once per tap), which the patch kernel replaces by one staged copy per band.

    python scripts/conv_patch_probe.py [--batch 256] [--rounds 5]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def timed(fn, reps, passes=3):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(passes):
        torch.cuda._sleep(1 << 18)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=27)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the two paths")
    args = ap.parse_args()
    from sparknet_amd.ops import hip
    from sparknet_amd.ops.spec import ConvSpec
    dev = torch.device("cuda", 0)
    B, H, bf = args.batch, args.size, torch.bfloat16
    s = ConvSpec(B, H, H, 96, 256, 5, 5, 1, 1, 2, 2, 1, 1, 2)
    assert hip.patch_dgrad_ok(s), s
    dy = torch.randn(B, H, H, 256, device=dev).to(bf)
    x = torch.randn(B, H, H, 96, device=dev).to(bf)
    w = (0.05 * torch.randn(256, 5, 5, 48, device=dev)).to(bf)
    dx = torch.empty_like(x)
    ws = hip.ConvScratch(wt=hip._flipped(w, s, None))

    def run():
        hip.conv_backward(dy, x, w, s, True, None, None, x, ws, dx_out=dx)
    t = {"": [], "conv_patch=0": []}
    outs = {}
    for _ in range(args.rounds):
        for feat in t:
            os.environ["SN_FEATURES"] = feat
            t[feat].append(timed(run, args.reps))
            outs[feat] = dx.clone()
    os.environ.pop("SN_FEATURES", None)
    flop = 2.0 * B * H * H * 96 * 25 * 128
    stream = B * H * H * 256 * 2 * 25
    print(f"conv2 dgrad B={B} {H}x{H}: {flop / 1e9:.1f} GFLOP, im2col operand {stream / 1e9:.2f} GB, "
          f"dy {stream / 25e6:.1f} MB; outputs bitwise equal: {torch.equal(outs[''], outs['conv_patch=0'])}")
    for feat, v in t.items():
        m = statistics.median(v)
        print(f"  {feat or 'conv_patch (new)':18s} {m:8.1f} us  {flop / m / 1e6:7.1f} TF/s  "
              f"im2col stream {stream / m / 1e6:5.1f} TB/s  (" + " ".join(f"{q:.1f}" for q in v) + ")")
    print(f"  ratio {statistics.median(t['conv_patch=0']) / statistics.median(t['']):.2f}x")


if __name__ == "__main__":
    main()
