#!/usr/bin/env python3
"""The wide-window depthwise kernels (csrc/kernels/conv_xdw.hip) at MnasNet-B1's six distinct 5x5
depthwise shapes (ten layers): forward, data gradient and weight / bias gradient through
``hip.conv_forward`` / ``hip.conv_backward``, new kernels against SN_FEATURES=conv_depthwise_wide=0
(one im2col + GEMM per channel) in alternating rounds, next to a device copy of the bytes each must
move (one input-sized and one output-sized tensor; weights, bias and slab partials are not counted).
Each figure is the median over the rounds of a median of event-timed passes.

    python scripts/xdw_probe.py [--batch 64] [--rounds 3] [--extra]

``--extra`` adds a 7x7, a dilated 3x3 and a 1x7 shape (no MnasNet layers; new kernels only).
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

OFF = "conv_depthwise_wide=0"
# (name, H = W, C, window, stride, dilation)
SHAPES = [("block2_1/dw", 56, 72, 5, 2, 1), ("block2_2..3/dw (x2)", 28, 120, 5, 1, 1), ("block3_1/dw", 28, 240, 5, 2, 1),
          ("block3_2..3/dw (x2)", 14, 480, 5, 1, 1), ("block5_1/dw", 14, 576, 5, 2, 1),
          ("block5_2..4/dw (x3)", 7, 1152, 5, 1, 1)]
EXTRA = [("7x7", 28, 240, 7, 1, 1), ("7x7 / 2", 28, 240, 7, 2, 1), ("3x3 dilated 2", 28, 240, 3, 1, 2),
         ("1x7", 14, 480, (1, 7), 1, 1)]


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
    ap.add_argument("--extra", action="store_true")
    args = ap.parse_args()
    from sparknet_amd.ops import hip
    from sparknet_amd.ops.spec import ConvSpec
    dev, bf, B = torch.device("cuda", 0), torch.bfloat16, args.batch
    for name, H, C, k, st, dil in SHAPES + (EXTRA if args.extra else []):
        R, S = k if isinstance(k, tuple) else (k, k)
        s = ConvSpec(B, H, H, C, C, R, S, st, st, dil * (R - 1) // 2, dil * (S - 1) // 2, dil, dil, C)
        x = torch.randn(B, H, H, C, device=dev).to(bf)
        w = (0.2 * torch.randn(C, R, S, 1, device=dev)).to(bf)
        dy = torch.randn(B, s.P, s.Q, C, device=dev).to(bf)
        dw, db = torch.zeros(C, R, S, 1, device=dev), torch.zeros(C, device=dev)
        products = {"fwd": lambda: hip.conv_forward(x, w, None, s),
                    "dgrad": lambda: hip.conv_backward(dy, x, w, s, True, None, None, None),
                    "wgrad": lambda: hip.conv_backward(dy, x, w, s, False, dw, db, None, dw_acc=False, db_acc=False)}
        nbytes = (x.numel() + dy.numel()) * 2
        src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        routes = ("", OFF) if (name, H, C, k, st, dil) in SHAPES else ("",)
        t = {(p, f): [] for p in products for f in routes}
        for _ in range(args.rounds):
            for feat in routes:  # alternating: new, off, new, off, ...
                os.environ["SN_FEATURES"] = feat
                for p, fn in products.items():
                    t[p, feat].append(timed(fn, args.reps if not feat else 2))
        os.environ.pop("SN_FEATURES", None)
        tc = timed(lambda: dst.copy_(src), args.reps)
        out = [f"{name:20s} B={B} {H}x{H}x{C} {R}x{S}/{st} d{dil}: {nbytes / 1e6:6.1f} MB (x2 = {2 * nbytes / 2 ** 20:5.0f} MiB "
               f"touched) copy {tc:7.1f} us {nbytes / tc / 1e6:5.2f} TB/s"]
        for p in products:
            new = statistics.median(t[p, ""])
            line = f"{p} {new:7.1f} us {nbytes / new / 1e6:5.2f} TB/s"
            if OFF in routes:
                off = statistics.median(t[p, OFF])
                line += f" (off {off:9.1f} us, x{off / new:6.1f}; rounds new {min(t[p, '']):.1f}-{max(t[p, '']):.1f})"
            out.append(line)
        print(" | ".join(out), flush=True)
        del x, dy, src, dst


if __name__ == "__main__":
    main()
