#!/usr/bin/env python3
"""The depthwise 3x3 kernels (csrc/kernels/conv_dw.hip) at MobileNet v1's 13 depthwise shapes
(9 distinct; conv5_1 .. conv5_5 share one): forward, data gradient and weight / bias gradient
timed in isolation, with the effective HBM rate of the bytes each must move (activations read
once and written once; weights, bias and slab partials are not counted), next to a device copy
of the same number of bytes.

    python scripts/dw_probe.py [--batch 64]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def timed(fn, reps=10, passes=5):
    fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(passes):
        torch.cuda._sleep(1 << 18)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        best.append(e0.elapsed_time(e1) * 1e3 / reps)
    best.sort()
    return best[len(best) // 2]


SHAPES = [("conv2_1/dw", 112, 32, 1), ("conv2_2/dw", 112, 64, 2), ("conv3_1/dw", 56, 128, 1),
          ("conv3_2/dw", 56, 128, 2), ("conv4_1/dw", 28, 256, 1), ("conv4_2/dw", 28, 256, 2),
          ("conv5_1..5/dw (x5)", 14, 512, 1), ("conv5_6/dw", 14, 512, 2), ("conv6/dw", 7, 1024, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--only", default="", help="comma-separated substrings of the shape names to run")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    from sparknet_amd.ops import _lib
    from sparknet_amd.ops import hip
    from sparknet_amd.ops.spec import ConvSpec
    dev = torch.device("cuda", 0)
    B = args.batch
    shapes = [sh for sh in SHAPES if not args.only or any(o in sh[0] for o in args.only.split(","))]
    bf = torch.bfloat16
    for name, H, C, st in shapes:
        s = ConvSpec(B, H, H, C, C, 3, 3, st, st, 1, 1, 1, 1, C)
        geo = (s.N, s.H, s.W, s.C, s.sh, s.sw, s.ph, s.pw)
        x = torch.randn(B, H, H, C, device=dev).to(bf)
        w = (0.2 * torch.randn(C, 3, 3, 1, device=dev)).to(bf)
        y = torch.empty(B, s.P, s.Q, C, device=dev, dtype=bf)
        dy = torch.randn(B, s.P, s.Q, C, device=dev).to(bf)
        dx = torch.empty_like(x)
        dw = torch.zeros(C, 3, 3, 1, device=dev)
        db = torch.zeros(C, device=dev)
        part, n = hip._dw_part(s, dev)

        def fwd():
            _lib.call("conv_dw_fwd", x, w, None, y, *geo, 0)

        def dgrad():
            _lib.call("conv_dw_dgrad", dy, w, None, dx, *geo)

        def wgrad():
            _lib.call("conv_dw_wgrad", dy, x, part, n, dw, 1, db, 1, *geo)
        nbytes = (x.numel() + y.numel()) * 2  # the same for all three: one input-sized and one output-sized tensor
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        tc = timed(lambda: dst.copy_(src), args.reps)
        out = [f"{name:19s} B={B} {H}x{H}x{C} /{st}: {nbytes / 1e6:7.1f} MB  copy {tc:7.1f} us {nbytes / tc / 1e6:5.2f} TB/s"]
        for label, fn in (("fwd", fwd), ("dgrad", dgrad), ("wgrad", wgrad)):
            t = timed(fn, args.reps)
            out.append(f"{label} {t:7.1f} us {nbytes / t / 1e6:5.2f} TB/s")
        print(" | ".join(out), flush=True)
        del x, y, dy, dx, src, dst, part


if __name__ == "__main__":
    main()
