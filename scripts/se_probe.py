#!/usr/bin/env python3
"""The squeeze-and-excitation kernels (csrc/kernels/se.hip) at SE-ResNet-50's four block shapes:
56 x 56 x 256, 28 x 28 x 512, 14 x 14 x 1024 and 7 x 7 x 2048 at batch 64.

Per shape, each timed in isolation with device events (medians of several passes, the two sides in
alternation on the same build):

* squeeze   gap_fwd against avepool_fwd (``hip.pool_forward`` under ``SN_FEATURES=se_kernels=0``).
  At 7 x 7 the Pooling layer keeps avepool_fwd whatever the timing says (the H W > 64 threshold
  keeps the bits of the existing 7 x 7 heads); the row shows both all the same.
* excite    nc_affine_fwd(x, s, r) against the plain-Caffe spelling on the parent routes in bf16:
  Scale with an (N, C) bottom on an NCHW copy (transpose, axis_scale_bias, transpose back), then
  Eltwise SUM.  The Axpy layer's own se_kernels=0 path is timed too: it keeps the product in fp32
  between the launches (one rounding, as in the kernel), so it is slower than that spelling.
* backward  nc_affine_bwd (dx and the gate's gradient in one pass) against the parent routes: the
  Eltwise SUM gradient, a transposed dy, axis_reduce, axis_scale_bias and the transpose back.  The
  shortcut's gradient (one eltwise_bwd on either side) is left out of both.

TB/s is the effective rate of the bytes the computation must move (squeeze: x; excite: x, r and
y; backward: dy, x and dx; the [N][C] vectors and slab partials are not counted), next to a device
copy of as many bytes.  Three of the four activations (51, 26 and 13 MB; stage 2 has 103 MB) and
every launch's working set but stage 2's excite / backward (308 MB) are below the 256 MiB Infinity
Cache and the launches repeat on the same buffers, so these rates are not HBM rates: the column
compares a kernel with the copy, nothing more.

    python scripts/se_probe.py [--batch 64]
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


# (name, H = W, channels) of the output of scale{stage}x_branch2c
SHAPES = [("res2x", 56, 256), ("res3x", 28, 512), ("res4x", 14, 1024), ("res5x", 7, 2048)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--only", default="", help="comma-separated substrings of the shape names to run")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2, help="alternations of the two sides")
    args = ap.parse_args()
    from sparknet_amd.ops import hip, layers_hip as lh
    from sparknet_amd.ops.spec import POOL_AVE, PoolSpec
    dev = torch.device("cuda", 0)
    N, bf, f32 = args.batch, torch.bfloat16, torch.float32
    for name, H, C in [sh for sh in SHAPES if not args.only or any(o in sh[0] for o in args.only.split(","))]:
        HW = H * H
        x = torch.randn(N, H, H, C, device=dev).to(bf)
        r = torch.randn(N, H, H, C, device=dev).to(bf)
        dy = torch.randn(N, H, H, C, device=dev).to(bf)
        s = torch.sigmoid(torch.randn(N, C, device=dev))
        ds = torch.empty(N, C, device=dev)
        xl = lh.nhwc_to_nchw(x)  # the Scale layer keeps its NCHW input for the backward
        ps = PoolSpec(N, H, H, C, H, H, 1, 1, 0, 0, POOL_AVE)

        def to_nhwc(t):
            return lh.nchw_to_nhwc(t.reshape(N, C, HW), N, C, H, H)

        def old_excite():
            t = to_nhwc(lh.axis_scale_bias(lh.nhwc_to_nchw(x), s.view(-1), None, N * C, HW))
            return lh.eltwise_fwd(1, [t, r], [1.0, 1.0])[0]

        def old_axpy_layer():
            t = to_nhwc(lh.axis_scale_bias(lh.nhwc_to_nchw(x, f32), s.view(-1), None, N * C, HW))
            return lh.cast(lh.eltwise_fwd(1, [t, lh.cast(r, f32)], [1.0, 1.0])[0], bf)

        def old_backward():
            g = lh.nhwc_to_nchw(lh.eltwise_bwd(1, [x, r], [1.0, 1.0], 0, False, x, dy, None))
            lh.axis_reduce(lh.RED_DOT, g, xl, 1, 1, N * C, HW, out=ds)
            return to_nhwc(lh.axis_scale_bias(g, s.view(-1), None, N * C, HW))

        def old_squeeze():
            os.environ["SN_FEATURES"] = "se_kernels=0"
            try:
                return hip.pool_forward(x, ps)
            finally:
                os.environ.pop("SN_FEATURES", None)

        rows = {
            "squeeze": (1, lambda: lh.gap_fwd(x, N, HW, C), {"avepool_fwd": old_squeeze}),
            "excite": (3, lambda: lh.nc_affine_fwd(x, N, HW, C, s=s, r=r),
                       {"Scale + Eltwise": old_excite, "Axpy se_kernels=0": old_axpy_layer}),
            "backward": (3, lambda: lh.nc_affine_bwd(dy, N, HW, C, s=s, x=x, ds=ds, sflag=lh.GRAD_STORE),
                         {"parent routes": old_backward}),
        }
        print(f"{name} B={N} {H}x{H}x{C}: activation {x.numel() * 2 / 1e6:.1f} MB"
              f"{'' if HW > 64 else '  (H W <= 64: the Pooling layer stays on avepool_fwd)'}", flush=True)
        tot = {"new": 0.0, "old": 0.0}
        for label, (tensors, new, olds) in rows.items():
            nbytes = tensors * x.numel() * 2
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            tc = timed(lambda: dst.copy_(src), args.reps)
            del src, dst
            t = {}
            for rnd in range(args.rounds):
                for key, fn in (("new", new), *olds.items()):
                    t.setdefault(key, []).append(timed(fn, args.reps, passes=3))
            med = {k: (sorted(v)[len(v) // 2] if len(v) % 2 else 0.5 * (sorted(v)[len(v) // 2 - 1] + sorted(v)[len(v) // 2]))
                   for k, v in t.items()}
            tot["new"] += med["new"]
            tot["old"] += med[next(iter(olds))]
            cells = [f"{k:18s} {m:8.1f} us {nbytes / m / 1e6:5.2f} TB/s (" + " ".join(f"{q:.1f}" for q in t[k]) + ")"
                     for k, m in med.items()]
            print(f"  {label:8s} {nbytes / 1e6:6.1f} MB  copy {tc:7.1f} us {nbytes / tc / 1e6:5.2f} TB/s | " + " | ".join(cells),
                  flush=True)
        print(f"  sum      new {tot['new']:8.1f} us | parent {tot['old']:8.1f} us", flush=True)
        del x, r, dy, xl


if __name__ == "__main__":
    main()
