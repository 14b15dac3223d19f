#!/usr/bin/env python3
"""Wall time of the capped ball query (ops.ball_query_capped) next to the bounded one (ops.ball_query_bounded) on the
same inputs: one 65 k-point cloud against itself at mean degree 32, and the level 0 / level 1 pair of the DFaust-sized
workload (the neighbourhoods of its first down- and last up-convolution).  Every figure is the median of `--rounds` rounds of `--reps` back-to-back
calls, with the spread (min .. max over the rounds) beside it.  `--bounded-only` times the bounded query alone (what a
build without the capped entry points can run too: the A/B of the shared kernels against an older commit).

    python tools/time_capped_query.py [--cap 16] [--bounded-only]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import se3conv3d_amd as amd  # noqa: E402
from se3conv3d_amd import workloads as W  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cap", type=int, default=16)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--bounded-only", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")


def timed(fn):
    for _ in range(5):
        fn()
    rounds = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) / args.reps * 1e3)
    return f"{statistics.median(rounds):.3f} ms ({min(rounds):.3f} .. {max(rounds):.3f})"


def case(name, src, dst, r):
    q = (src.pts_, dst.pts_, src.batch_ids_, dst.batch_ids_, r)
    nb_b = src.num_batches()
    _, ends, info = amd.ops.ball_query_bounded(*q, capacity=1, n_batches=nb_b)
    e, n_dst = int(info[0]), dst.pts_.shape[0]
    print(f"{name}: {src.pts_.shape[0]} sources, {n_dst} samples, {nb_b} batch element(s), r = {r:.4f}, {e} edges "
          f"(mean degree {e / n_dst:.1f})")
    print(f"  bounded, capacity = E                      {timed(lambda: amd.ops.ball_query_bounded(*q, capacity=e, n_batches=nb_b))}")
    if args.bounded_only:
        return
    m = args.cap
    res = amd.ops.ball_query_capped(*q, m, 1, capacity=n_dst * m, n_batches=nb_b, want_degrees=True)
    kept, share = int(res[2][0]), float((res[3] > m).float().mean())
    print(f"  capped at {m}, capacity = samples x {m}        {timed(lambda: amd.ops.ball_query_capped(*q, m, 1, capacity=n_dst * m, n_batches=nb_b))}"
          f"   {kept} edges kept, {share:.2f} of the samples capped")
    print(f"  capped entry point without a cap (m = 0)   {timed(lambda: amd.ops.ball_query_capped(*q, 0, 1, capacity=e, n_batches=nb_b))}")


torch.manual_seed(0)
n = 65536
cloud = amd.pc.Pointcloud(torch.rand(n, 3, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), num_batches=1)
case("65 k cloud against itself", cloud, cloud, W.radius_for_degree(n, 32))
lo, hi, r_down, r_up = W.build_level_pair(W.WORKLOADS["dfaust_f2"], dev, 0)
case("DFaust-sized level 0 -> 1 (down)", lo, hi, r_down)
case("DFaust-sized level 1 -> 0 (up)", hi, lo, r_up)
