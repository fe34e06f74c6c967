#!/usr/bin/env python3
"""The narrow-group 3x3 kernels (csrc/kernels/conv_grouped.hip) at ResNeXt-50 32x4d's grouped
shapes: the four stage shapes and the three stride-2 first blocks.  Forward, data gradient and
weight gradient are timed through ``hip.conv_forward`` / ``hip.conv_backward`` with the new kernels
and with ``SN_FEATURES=conv_grouped=0`` (the implicit grouped GEMM, or one im2col + GEMM per group
at Cg = 4) in alternation on the same build, and the new launches once more on their own
(``call``: no dispatch, no allocation).  Times are medians of several passes of device events;
TB/s is the effective rate of the bytes each product must move (one input-sized and one
output-sized activation; weights and slab partials are not counted), next to a device copy of the
same number of bytes.  Every tensor here is below the 256 MiB Infinity Cache and the launches repeat
on the same buffers, so the copy runs above the HBM stream rate and the kernels may be served from
the cache as well: the TB/s column compares the two, it is not an HBM rate.  Cg = 32 (stage 5) has
no instance: its rows show the parent path only.

    python scripts/grouped_probe.py [--batch 64]
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


# (name, input H = W, channels, channels per group, stride)
SHAPES = [("res2x_branch2b", 56, 128, 4, 1), ("res3a_branch2b", 56, 256, 8, 2), ("res3x_branch2b", 28, 256, 8, 1),
          ("res4a_branch2b", 28, 512, 16, 2), ("res4x_branch2b", 14, 512, 16, 1), ("res5a_branch2b", 14, 1024, 32, 2),
          ("res5x_branch2b", 7, 1024, 32, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--only", default="", help="comma-separated substrings of the shape names to run")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2, help="alternations of the two paths")
    args = ap.parse_args()
    from sparknet_amd.ops import _lib, hip
    from sparknet_amd.ops.spec import ConvSpec
    dev = torch.device("cuda", 0)
    B = args.batch
    bf = torch.bfloat16
    for name, H, C, cg, st in [sh for sh in SHAPES if not args.only or any(o in sh[0] for o in args.only.split(","))]:
        s = ConvSpec(B, H, H, C, C, 3, 3, st, st, 1, 1, 1, 1, C // cg)
        geo = (s.N, s.H, s.W, s.C, s.Cg, s.sh, s.sw, s.ph, s.pw)
        x = torch.randn(B, H, H, C, device=dev).to(bf)
        w = (0.2 * torch.randn(C, 3, 3, cg, device=dev)).to(bf)
        y = torch.empty(B, s.P, s.Q, C, device=dev, dtype=bf)
        dy = torch.randn(B, s.P, s.Q, C, device=dev).to(bf)
        dx = torch.empty_like(x)
        dw = torch.zeros(C, 3, 3, cg, device=dev)
        products = {"fwd": lambda: hip.conv_forward(x, w, None, s, relu=True),
                    "dgrad": lambda: hip.conv_backward(dy, x, w, s, True, None, None, x, dx_out=dx),
                    "wgrad": lambda: hip.conv_backward(dy, x, w, s, False, dw, None, None, dw_acc=False)}
        nbytes = (x.numel() + y.numel()) * 2
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        tc = timed(lambda: dst.copy_(src), args.reps)
        print(f"{name} B={B} {H}x{H}x{C} Cg={cg} /{st}: {nbytes / 1e6:.1f} MB  copy {tc:.1f} us "
              f"{nbytes / tc / 1e6:.2f} TB/s", flush=True)
        routed = cg in hip.GROUPED_WIDTHS
        t = {}
        for rnd in range(args.rounds):
            for feat in ("", "conv_grouped=0") if routed else ("conv_grouped=0",):
                os.environ["SN_FEATURES"] = feat
                reps = args.reps if (feat == "" or cg != 4) else 2  # the per-group loop takes milliseconds
                for label, fn in products.items():
                    t.setdefault((feat, label), []).append(timed(fn, reps, passes=3))
        os.environ.pop("SN_FEATURES", None)
        if routed:
            part, n = hip._grouped_part(s, dev)
            direct = {"fwd": lambda: _lib.call("conv_grouped_fwd", x, w, None, y, *geo, 1),
                      "dgrad": lambda: _lib.call("conv_grouped_dgrad", dy, w, x, dx, *geo),
                      "wgrad": lambda: _lib.call("conv_grouped_wgrad", dy, x, part, n, dw, 0, *geo)}
        tot = {"": 0.0, "conv_grouped=0": 0.0}
        for label in products:
            row = [f"  {label:5s}"]
            if routed:
                td = timed(direct[label], args.reps)
                row.append(f"call {td:8.1f} us {nbytes / td / 1e6:5.2f} TB/s")
            for feat in ("", "conv_grouped=0") if routed else ("conv_grouped=0",):
                v = sorted(t[(feat, label)])
                m = v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
                tot[feat] += m
                row.append(f"{feat or 'new':14s} {m:9.1f} us (" + " ".join(f"{q:.1f}" for q in t[(feat, label)]) + ")")
            print(" | ".join(row), flush=True)
        print(f"  sum   new {tot['']:9.1f} us | conv_grouped=0 {tot['conv_grouped=0']:9.1f} us", flush=True)
        del x, y, dy, dx, src, dst


if __name__ == "__main__":
    main()
