#!/usr/bin/env python3
"""The phase-decomposed stride-2 data gradient (csrc/kernels/conv_tstride.hip) against the route it
replaces, on the same build: the isolated data gradient through ``hip.conv_backward`` (gate on, dense
``dx_out``) with the new kernel and with ``SN_FEATURES=conv_tstride=0`` (fp32 dcol GEMM + col2im +
relu_backward + copy), in alternation, at ResNet-50's six strided 1x1 layers, three 3x3 / 2 shapes, a
2x2 / 2 up-convolution and a 4x4 / 2 upsampler.  Times are medians of several passes of device events
per round; every round is printed, so the spread between rounds of one route is the A/B noise of the
run.  "copy floor" is a device copy that moves as many bytes as the product must (dy and the gate
read once, dx written once): a floor, not a target.  The two results are also compared elementwise.

    python scripts/tstride_probe.py [--batch 64]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def timed(fn, reps=100, passes=5):
    for _ in range(3):
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


# (name, input H = W, input channels C, output channels K, window, pad): x [B, H, H, C] -> y [B, P, P, K]
SHAPES = [("res3a_branch2a", 56, 256, 128, 1, 0), ("res3a_branch1", 56, 256, 512, 1, 0),
          ("res4a_branch2a", 28, 512, 256, 1, 0), ("res4a_branch1", 28, 512, 1024, 1, 0),
          ("res5a_branch2a", 14, 1024, 512, 1, 0), ("res5a_branch1", 14, 1024, 2048, 1, 0),
          ("3x3/2 56 64->128", 56, 64, 128, 3, 1), ("3x3/2 28 128->256", 28, 128, 256, 3, 1),
          ("3x3/2 14 256->512", 14, 256, 512, 3, 1), ("2x2/2 up 14->28 512->256", 28, 256, 512, 2, 0),
          ("4x4/2 up 16->32 256->128", 32, 128, 256, 4, 1)]
OFF = "conv_tstride=0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--only", default="", help="comma-separated substrings of the shape names to run")
    ap.add_argument("--reps", type=int, default=100, help="calls per timed window (2 to 30 ms at batch 64)")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the two routes")
    args = ap.parse_args()
    from sparknet_amd.ops import hip
    from sparknet_amd.ops.spec import ConvSpec
    dev = torch.device("cuda", 0)
    B, bf = args.batch, torch.bfloat16
    for name, H, C, K, r, pad in [sh for sh in SHAPES if not args.only or any(o in sh[0] for o in args.only.split(","))]:
        s = ConvSpec(B, H, H, C, K, r, r, 2, 2, pad, pad, 1, 1, 1)
        os.environ.pop("SN_FEATURES", None)
        assert hip.tstride_ok(s), s
        x = torch.randn(B, H, H, C, device=dev).to(bf)
        w = (0.05 * torch.randn(K, r, r, C, device=dev)).to(bf)
        dy = torch.randn(B, s.P, s.Q, K, device=dev).to(bf)
        dx = {f: torch.empty_like(x) for f in ("", OFF)}
        run = lambda f: hip.conv_backward(dy, x, w, s, True, None, None, x, dx_out=dx[f])
        nbytes = (2 * x.numel() + dy.numel()) * 2
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        tcopy = timed(lambda: dst.copy_(src), args.reps)  # moves nbytes in all: half read, half written
        t = {"": [], OFF: []}
        for _ in range(args.rounds):
            for f in ("", OFF):
                os.environ["SN_FEATURES"] = f
                t[f].append(timed(lambda: run(f), args.reps, passes=3))
        os.environ.pop("SN_FEATURES", None)
        torch.cuda.synchronize()
        diff = (dx[""].float() - dx[OFF].float()).abs().max().item()
        scale = dx[OFF].float().abs().max().item()
        med = {f: sorted(v)[len(v) // 2] for f, v in t.items()}
        fmt = lambda v: " ".join(f"{q:.1f}" for q in v)
        print(f"{name:26s} B={B} x {H}x{H}x{C} K={K} {r}x{r}/2 pad {pad}: {nbytes / 1e6:6.1f} MB, copy floor {tcopy:6.1f} us | "
              f"new {med['']:8.1f} us ({fmt(t[''])}) | {OFF} {med[OFF]:8.1f} us ({fmt(t[OFF])}) | "
              f"x{med[OFF] / med['']:.2f} | max |new - old| {diff:.3g} of {scale:.3g}", flush=True)
        del x, dy, dx, src, dst


if __name__ == "__main__":
    main()
