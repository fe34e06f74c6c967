#!/usr/bin/env python3
"""Re-time a model's GEMM products one at a time, on an idle GPU, against every tuner
candidate (ops.gemm._candidates: tile x split-K), and write the winners into a tuning
database.

Why: the first-call tuner times its candidates inside the warm-up steps, and on a model whose
Inception towers run on four branch streams the other streams' kernels share the CUs while a
candidate is timed — GoogLeNet's database held choices up to 1.6x slower than the best tile in
isolation (conv2/3x3 forward: tile 15 at 340 TF/s vs tile 17 at 522, scripts/conv_probe.py).
Every product here is timed with the real operands and epilogue (the launch recorded from one
eager step), median of 5 passes; a candidate must beat the current choice by 3 % to replace it
and must reproduce the current choice's output (max relative error 1e-2).  fp8 and EPI_SGD
products keep their entries.

    python scripts/retune_isolated.py --model googlenet --out gpurun_out/gemm_tuned_gn.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def timed(fn, reps, passes=5):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="googlenet")
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--out", required=True)
    ap.add_argument("--margin", type=float, default=0.97)
    ap.add_argument("--wide", action="store_true", help="also try split-K 1-256 (powers of 2 and x1.5) on every tile")
    ap.add_argument("--tiles", default="", help="only try these candidate tiles (comma-separated), e.g. 21,22")
    args = ap.parse_args()
    import bench
    from sparknet_amd import models
    from sparknet_amd.core.solver import Solver
    from sparknet_amd.data.prefetch import DeviceFeeder, SyntheticSource
    from sparknet_amd.engine import LocalSGDTrainer, fuse_input_fold, fuse_relu
    from sparknet_amd.ops import gemm as G

    dev = torch.device("cuda", 0)
    B, C, HW, crop, classes, mean, in_scale = bench.DEFAULTS[args.model]
    B = args.batch or B
    kw = dict(train_batch=B, test_batch=max(1, min(B, 50)))
    if args.model in ("caffenet", "alexnet", "googlenet", "vgg16"):
        kw["crop"] = crop
    solver = Solver(models.solver_for(args.model, **kw), device=dev, seed=1701, build_test_nets=False)
    net = solver.net
    fuse_relu(net)
    src = SyntheticSource(B, C, HW, HW, classes=classes, pool=3, seed=0)
    feeder = DeviceFeeder(src, net.blob_by_name("data"), net.blob_by_name("label"), crop=crop, mean=mean,
                          scale=in_scale, mirror=True, train=True, rng_state=net.ctx.rng_state, device=dev)
    fuse_input_fold(net, feeder)
    trainer = LocalSGDTrainer(solver, None, tau=50, feeder=feeder, use_graph=False)
    trainer.local_step()
    torch.cuda.synchronize()

    where = ["?"]
    for layer in net.layers:
        f, b = layer.forward, layer.backward

        def fw(*a, _f=f, _n=layer.name):
            where[0] = _n + ":fwd"
            return _f(*a)

        def bw(*a, _b=b, _n=layer.name):
            where[0] = _n + ":bwd"
            return _b(*a)
        layer.forward, layer.backward = fw, bw
    rec = []
    orig = G._launch

    def spy(call, tile, splits, kchunk):
        rec.append((where[0], call, tile, splits, kchunk))
        return orig(call, tile, splits, kchunk)
    G._launch = spy
    trainer.local_step()
    torch.cuda.synchronize()
    G._launch = orig

    updates = {}
    tot_old = tot_new = 0.0
    seen = set()
    for name, call, tile, splits, kchunk in rec:
        M, N, K, groups, out, bias_grad = call.M, call.N, call.K, call.groups, call.out, call.bias_grad
        key = call.key
        if call.fp8 or call.epi == G.EPI_SGD or key in seen:
            continue
        seen.add(key)
        fl = 2.0 * M * N * K * groups
        reps = max(2, min(40, int(2e12 / fl)))
        saved = out.clone()
        bsaved = bias_grad.clone() if bias_grad is not None else None

        def restore():
            out.copy_(saved)
            if bias_grad is not None:
                bias_grad.copy_(bsaved)

        def run(t, s, kc):
            orig(call, t, s, kc)
        restore()
        run(tile, splits, kchunk)
        ref = out.float().clone()
        scale = ref.abs().max().item() + 1e-6
        t_old = timed(lambda: run(tile, splits, kchunk), reps)
        best = (t_old, tile, splits, kchunk)
        cands = G._candidates(call)
        if args.wide:
            extra = []
            for t in dict.fromkeys(c[0] for c in cands):
                for s in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256):
                    kc = G._kchunk(K, s, G.BK)
                    s2 = max(1, -(-K // kc))
                    if s2 > 1 and s2 * M * N * groups * 4 > (256 << 20):
                        continue
                    extra.append((t, s2, kc))
            cands = list(dict.fromkeys(cands + extra))
        if args.tiles:
            only = {int(v) for v in args.tiles.split(",")}
            cands = [c for c in cands if c[0] in only]
        for t, s, kc in cands:
            if (t, s) == (tile, splits):
                continue
            try:
                restore()
                run(t, s, kc)
            except RuntimeError:
                continue
            err = (out.float() - ref).abs().max().item() / scale
            if err > 1e-2:
                continue
            us = timed(lambda: run(t, s, kc), reps)
            if us < best[0]:
                best = (us, t, s, kc)
        restore()
        tot_old += t_old
        chosen = best if best[0] < args.margin * t_old else (t_old, tile, splits, kchunk)
        tot_new += chosen[0]
        if (chosen[1], chosen[2]) != (tile, splits):
            updates[G._key_to_str(key)] = [chosen[1], chosen[2], chosen[3]]
        print(f"{name:30s} {M:7d} {N:5d} {K:6d} {groups}  {tile:3d}/{splits:<3d} {t_old:8.1f} -> "
              f"{chosen[1]:3d}/{chosen[2]:<3d} {chosen[0]:8.1f}", flush=True)
    db = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            db = json.load(f)
    db.update(updates)
    with open(args.out, "w") as f:
        json.dump(dict(sorted(db.items())), f, indent=0)
    print(f"total GEMM (distinct products): {tot_old:.1f} -> {tot_new:.1f} us; {len(updates)} entries changed -> {args.out}")


if __name__ == "__main__":
    main()
