#!/usr/bin/env python3
"""The grouped pointwise kernels (csrc/kernels/conv_gpw.hip) at the eleven distinct routed shapes of
ShuffleNet 1x g=3 (31 layers): forward, data gradient and weight gradient through ``hip.conv_forward`` /
``hip.conv_backward``, new kernels against SN_FEATURES=conv_gpw=0 in the same build (the implicit
grouped GEMM where Cg and Kg are multiples of 8, one im2col + GEMM per group otherwise) in alternating
rounds, next to a device copy of the bytes each must move (one input-sized and one output-sized tensor;
weights and slab partials are not counted).  Each figure is the median over the rounds of a median of
event-timed passes; the spread of the rounds is printed for both routes.

    python scripts/gpw_probe.py [--batch 64] [--rounds 3]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

OFF = "conv_gpw=0"
G = 3
# (layers, H = W, C, K)
SHAPES = [("resx1_conv3", 28, 60, 216), ("resx2..4_conv1 (x3)", 28, 240, 60), ("resx2..4_conv3 (x3)", 28, 60, 240),
          ("resx5_conv1", 28, 240, 120), ("resx5_conv3", 14, 120, 240), ("resx6..12_conv1 (x7)", 14, 480, 120),
          ("resx6..12_conv3 (x7)", 14, 120, 480), ("resx13_conv1", 14, 480, 240), ("resx13_conv3", 7, 240, 480),
          ("resx14..16_conv1 (x3)", 7, 960, 240), ("resx14..16_conv3 (x3)", 7, 240, 960)]


def timed(fn, reps, passes=3):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(passes):
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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from sparknet_amd.ops import hip
    from sparknet_amd.ops.spec import ConvSpec
    dev, bf, B = torch.device("cuda", 0), torch.bfloat16, args.batch
    for name, H, C, K in SHAPES:
        s = ConvSpec(B, H, H, C, K, 1, 1, groups=G)
        assert hip.gpw_ok(s), s
        x = torch.randn(B, H, H, C, device=dev).to(bf)
        w = (0.2 * torch.randn(K, 1, 1, s.Cg, device=dev)).to(bf)
        dy = torch.randn(B, H, H, K, device=dev).to(bf)
        dw = torch.zeros(K, 1, 1, s.Cg, device=dev)
        products = {"fwd": lambda: hip.conv_forward(x, w, None, s),
                    "dgrad": lambda: hip.conv_backward(dy, x, w, s, True, None, None, None),
                    "wgrad": lambda: hip.conv_backward(dy, x, w, s, False, dw, None, None, dw_acc=False)}
        nbytes = (x.numel() + dy.numel()) * 2
        src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        t = {(p, f): [] for p in products for f in ("", OFF)}
        for _ in range(args.rounds):
            for feat in ("", OFF):  # alternating: new, off, new, off, ...
                os.environ["SN_FEATURES"] = feat
                for p, fn in products.items():
                    t[p, feat].append(timed(fn, args.reps))
        os.environ.pop("SN_FEATURES", None)
        tc = timed(lambda: dst.copy_(src), args.reps)
        out = [f"{name:22s} B={B} {H}x{H} {s.Cg}->{s.Kg} x{G}: {nbytes / 1e6:6.1f} MB (x2 = {2 * nbytes / 2 ** 20:4.0f} MiB "
               f"touched) copy {tc:6.1f} us {nbytes / tc / 1e6:5.2f} TB/s"]
        for p in products:
            new, off = statistics.median(t[p, ""]), statistics.median(t[p, OFF])
            out.append(f"{p} {new:6.1f} us {nbytes / new / 1e6:5.2f} TB/s (rounds {min(t[p, '']):.1f}-{max(t[p, '']):.1f}; "
                       f"off {off:7.1f} us, rounds {min(t[p, OFF]):.1f}-{max(t[p, OFF]):.1f}; x{off / new:5.2f})")
        print(" | ".join(out), flush=True)
        del x, dy, src, dst


if __name__ == "__main__":
    main()
