#!/usr/bin/env python3
"""The 32-wide grouped 3x3 kernels (csrc/kernels/conv_wgroup.hip) at ResNeXt-50 32x4d's stage 5:
res5a (14x14x1024, stride 2) and res5b / res5c (7x7x1024, stride 1).  Forward, data gradient and
weight gradient are timed through ``hip.conv_forward`` / ``hip.conv_backward`` with the new kernels
and with ``SN_FEATURES=conv_wgroup=0`` (the implicit grouped GEMM; at stride 2 the per-group fp32 dcol
GEMM + col2im data gradient) in alternating rounds on the same build; every round's figure is
printed, and their spread per route is the noise a difference has to exceed.  A device copy of the
bytes each product must move (one input-sized and one output-sized activation) is the floor; every
tensor here is below the 256 MiB Infinity Cache, so that copy runs above the HBM stream rate.  The
two routes' results on the same inputs are compared elementwise in the same run.  ``--sweep`` times
the weight gradient over targets for its number of blocks (sn_conv_wgroup_tune).

    python scripts/wgroup_probe.py [--batch 64] [--rounds 3] [--sweep 32,64,128,256,512]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from grouped_probe import timed  # noqa: E402

SHAPES = [("res5a_branch2b", 14, 1024, 2), ("res5x_branch2b", 7, 1024, 1)]  # name, input H = W, channels, stride
OFF = "conv_wgroup=0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the two routes")
    ap.add_argument("--sweep", default="", help="comma-separated weight-gradient block targets to time")
    args = ap.parse_args()
    from sparknet_amd.ops import _lib, hip
    from sparknet_amd.ops.spec import ConvSpec
    dev = torch.device("cuda", 0)
    B, bf = args.batch, torch.bfloat16
    tune = _lib.kernels().sn_conv_wgroup_tune
    tune.restype = None
    for name, H, C, st in SHAPES:
        s = ConvSpec(B, H, H, C, C, 3, 3, st, st, 1, 1, 1, 1, C // 32)
        x = torch.randn(B, H, H, C, device=dev).to(bf)
        w = (0.2 * torch.randn(C, 3, 3, 32, device=dev)).to(bf)
        dy = torch.randn(B, s.P, s.Q, C, device=dev).to(bf)
        dx = torch.empty_like(x)
        dw = torch.zeros(C, 3, 3, 32, device=dev)

        def wgrad():
            hip.conv_backward(dy, x, w, s, False, dw, None, None, dw_acc=False)
            return dw
        products = {"fwd": lambda: hip.conv_forward(x, w, None, s, relu=True),
                    "dgrad": lambda: hip.conv_backward(dy, x, w, s, True, None, None, x, dx_out=dx),
                    "wgrad": wgrad}
        nbytes = (x.numel() + dy.numel()) * 2
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        tc = timed(lambda: dst.copy_(src), args.reps)
        print(f"{name} B={B} {H}x{H}x{C} Cg=32 /{st}: {nbytes / 1e6:.1f} MB  copy {tc:.1f} us", flush=True)
        t, res = {}, {}
        for rnd in range(args.rounds):
            for feat in ("", OFF):
                os.environ["SN_FEATURES"] = feat
                for label, fn in products.items():
                    if rnd == 0:
                        res[(feat, label)] = fn().float().clone()
                    t.setdefault((feat, label), []).append(timed(fn, args.reps, passes=3))
        os.environ.pop("SN_FEATURES", None)
        for label in products:
            row = [f"  {label:5s}"]
            for feat in ("", OFF):
                v = sorted(t[(feat, label)])
                row.append(f"{feat or 'new':13s} median {v[len(v) // 2]:8.1f} us, rounds " + " ".join(f"{q:.1f}" for q in t[(feat, label)]))
            a, b = res[("", label)], res[(OFF, label)]
            row.append(f"max |new - old| {float((a - b).abs().max()):.3g} of max |old| {float(b.abs().max()):.3g}")
            print(" | ".join(row), flush=True)
        for blocks in [int(v) for v in args.sweep.split(",") if v]:
            tune(_lib.C.c_longlong(blocks))
            n = hip._wgroup_part(s, dev)[1]
            print(f"  wgrad at {blocks:4d} blocks aimed at: {n // (C * 288):3d} slabs, {timed(wgrad, args.reps):8.1f} us", flush=True)
        tune(_lib.C.c_longlong(0))
        del x, dy, dx, src, dst


if __name__ == "__main__":
    main()
