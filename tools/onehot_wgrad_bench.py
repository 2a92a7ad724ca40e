#!/usr/bin/env python3
"""Weight gradient over one-hot stoch columns: the dense TN product against the segment sum (MI355X only).

    python tools/onehot_wgrad_bench.py [--reps 50] [--whole]

Per shape class of the update (rows R, layer width U; S x D = 32 x 32): device time per launch of
ops.gemm(dY, onehot, gW, transA=True, accumulate=True) and of ops.onehot_wgrad -- `reps` launches captured into one
hipGraph ON the 128-CU side lane (engine.Lanes), so that both pick what they pick inside the pipelined update (the
GEMM its lane tile, the segment sum its row splits), HIP events around the replay.  --whole: on the whole-chip stream.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dreamerv3-torch_amd"))
import torch  # noqa: E402

from dv3hip import engine, ops  # noqa: E402

SHAPES = [(14336, 512, "value / actor layer 0 (behaviour)"), (1024, 4096, "decoder Linear"),
          (1024, 512, "reward / cont layer 0 (world model)")]
S, D = 32, 32


def timed(fn, reps, stream):
    with torch.cuda.stream(stream):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        for _ in range(reps):
            fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = None
    for _ in range(3):
        with torch.cuda.stream(stream):
            a.record()
            g.replay()
            b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / reps
        best = us if best is None else min(best, us)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--whole", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lanes = engine.Lanes.get(dev)
    lane = "whole" if args.whole else "side"
    stream = lanes.streams[lane]
    print(f"{args.reps} launches in one hipGraph on the {lane} lane ({lanes.cus[lane]} CUs), us per launch (best of 3 replays)")
    print(f"{'R':>6s} {'U':>5s} {'dense':>8s} {'segsum':>8s} {'splits':>6s}  note")
    for R, U, note in SHAPES:
        torch.manual_seed(R + U)
        dY = torch.randn(R, U, device=dev)
        idx = torch.randint(0, D, (R, S), device=dev, dtype=torch.int32)
        x1 = torch.zeros(R, S * D, device=dev)
        x1.view(R, S, D).scatter_(2, idx.long().unsqueeze(-1), 1.0)
        gW = torch.zeros(U, S * D + 512, device=dev)  # (the .grad layout of a [stoch | deter] layer)
        part = torch.empty(ops.onehot_wgrad_partials(R, U, S, D), device=dev)
        dense = timed(lambda: ops.gemm(dY, x1, gW[:, :S * D], transA=True, transB=False, accumulate=True), args.reps, stream)
        seg = timed(lambda: ops.onehot_wgrad(dY, idx, D, gW[:, :S * D], part), args.reps, stream)
        print(f"{R:6d} {U:5d} {dense:8.1f} {seg:8.1f} {ops.onehot_wgrad_splits(R, U, lanes.cus[lane]):6d}  {note}", flush=True)


if __name__ == "__main__":
    main()
