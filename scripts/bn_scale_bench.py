"""Isolated effective bandwidth of the fused BatchNorm -> Scale -> ReLU kernels
(csrc/kernels/bn_scale.hip) on an MI355X: device-event timing of each of the four launches at
ResNet-50 activation shapes, bytes counted from the shapes (what the algorithm must move:
x for the statistics; x + y forward; dy + y + x for pass 1; dy + y + x + dx for pass 2).

    python scripts/bn_scale_bench.py [--shapes 64x256x56x56,64x2048x7x7] [--iters 200]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters, warmup=20):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x256x56x56,64x2048x7x7")
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bn_scale_bench: no GPU")
    from sparknet_amd.ops import _lib, layers_hip as lh
    _lib.kernels()
    for shape in args.shapes.split(","):
        N, C, H, W = (int(v) for v in shape.split("x"))
        R = N * H * W
        g = torch.Generator().manual_seed(0)
        x = (2 * torch.randn(R, C, generator=g) + 0.5).to("cuda", torch.bfloat16)
        dy = torch.randn(R, C, generator=g).to("cuda", torch.bfloat16)
        gamma = (0.5 + 0.5 * torch.randn(C, generator=g).abs()).cuda()
        beta = (0.5 * torch.randn(C, generator=g)).cuda()
        rm, rv, rf = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(1, device="cuda")
        dg, db = torch.empty_like(gamma), torch.empty_like(beta)
        mean, _, inv = lh.bn_stats(x, R, C, 1e-5, (rm, rv, rf), 0.999, R / (R - 1))
        stats = (lh.BN_BATCH, mean, inv, None, 1e-5)
        y = lh.bn_fwd(x, R, C, stats, gamma, beta, True)
        coef = lh.bn_bwd_reduce(dy, x, y, R, C, stats, True, dg, lh.GRAD_STORE, db, lh.GRAD_STORE)
        n = R * C * 2  # bytes of one bf16 activation
        cases = {
            "stats": (lambda: lh.bn_stats(x, R, C, 1e-5, (rm, rv, rf), 0.999, R / (R - 1)), n),
            "forward": (lambda: lh.bn_fwd(x, R, C, stats, gamma, beta, True), 2 * n),
            "backward_reduce": (lambda: lh.bn_bwd_reduce(dy, x, y, R, C, stats, True, dg, lh.GRAD_STORE, db,
                                                         lh.GRAD_STORE), 3 * n),
            "backward_dx": (lambda: lh.bn_bwd_dx(dy, x, y, R, C, stats, True, gamma, coef), 4 * n),
        }
        for name, (fn, nbytes) in cases.items():
            t = timed(fn, args.iters)
            print(json.dumps({"shape": shape, "kernel": name, "us": round(t * 1e6, 2), "bytes": nbytes,
                              "TB_per_s": round(nbytes / t / 1e12, 3)}), flush=True)


if __name__ == "__main__":
    main()
