#!/usr/bin/env python3
"""Forward + backward time of the clouds' global pooling through the torch path (`scatter_reduce` over an [N * F] copy of the
batch ids: the default route) and through `p_native=True` (`se3_global_pool` / `se3_global_unpool`,
include/se3conv_global_pool.h), eager and as replays of a captured graph, at three shapes:

    ScanNet network, coarsest level     6 scenes,  238 points in all, F = 1, C = 320  (profiles/r06_scannet_network_convs.txt)
    DFaust batch                       32 bodies x 2 200 points,      F = 2, C = 256  (every row of a batch: the largest pool
                                                                                       a head could be asked for)
    ModelNet-like, coarsest level      32 models x 16 points,         F = 2, C = 512  (32 x 1 024 points after four grid levels
                                                                                       of the classification network's five)

per shape `global_pooling` in avg and max mode and `global_pooling_specific_feature_pooling("avg", "max")`, on ordinary
clouds with sorted ids.  Times are per call of forward + backward: HIP events around a loop of eager calls (which includes
the host's launch work) and around a loop of graph replays.  Nothing here is asserted or thresholded; the native result is
compared with the torch result and the largest difference printed.  Needs a GPU; no CPU fallback.

    python tools/time_global_pool.py [--out profiles/global_pool.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import se3conv3d_amd as amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=0.3, help="keep repeating a measurement for this long")
ap.add_argument("--calls", type=int, default=20, help="calls (or replays) per timed window")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_pool.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tools/time_global_pool.py needs a GPU")
dev = torch.device("cuda:0")
lines = []
SHAPES = (("ScanNet network, coarsest level", [40, 40, 40, 40, 39, 39], 1, 320),
          ("DFaust batch, 32 x 2 200", [2200] * 32, 2, 256),
          ("ModelNet-like 32 x 1 024, coarsest level", [16] * 32, 2, 512))


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def window(fn):
    """ms per call of `fn` over windows of `args.calls` calls: (median, min, max, windows)."""
    times = []
    while sum(times) * args.calls < args.seconds * 1e3 or len(times) < 3:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / args.calls)
    return statistics.median(times), min(times), max(times), len(times)


def captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        fn()
    return graph


say("global pooling, forward + backward: the torch path (default) against p_native=True (se3_global_pool / se3_global_unpool)")
say(f"device: {torch.cuda.get_device_name(0)}; ms per call, median (min .. max) over windows of {args.calls} calls (HIP events)")
say(f"SE3_GLOBAL_POOL_CHUNK = {amd._lib.GLOBAL_POOL_CHUNK} points")
say()
lib = amd._lib.load()
for name, sizes, f, c in SHAPES:
    nb, n = len(sizes), sum(sizes)
    g = torch.Generator().manual_seed(n)
    ids = torch.repeat_interleave(torch.arange(nb, dtype=torch.int32), torch.tensor(sizes)).to(dev)
    pc = amd.pc.PointcloudRotEquiv.from_frames(torch.rand(n, 3, generator=g).to(dev), ids,
                                               torch.eye(3).reshape(1, 1, 9).repeat(n, f, 1).to(dev), num_batches=nb)
    x = torch.randn(n * f, c, generator=g).to(dev).requires_grad_(True)
    up = torch.randn(nb, c, generator=g).to(dev)
    ws = lib.se3_global_pool_workspace_bytes(n, f, nb, c)
    say(f"{name}: {nb} elements, {n} points, F = {f}, C = {c} ({n * f * c * 4 / 1e6:.2f} MB of features); "
        f"workspace {ws} bytes")
    calls = (("global_pooling avg", lambda native: pc.global_pooling(x, "avg", p_native=native)),
             ("global_pooling max", lambda native: pc.global_pooling(x, "max", p_native=native)),
             ("specific (avg, max)", lambda native: pc.global_pooling_specific_feature_pooling(x, "avg", "max", p_native=native)))
    for what, call in calls:
        res = {}

        def step(native):
            x.grad = None
            y = call(native)
            y.backward(up)
            res[native] = (y.detach(), x.grad)

        row = []
        for native in (False, True):
            step(native)
            torch.cuda.synchronize()
            eager = window(lambda: step(native))
            graph = captured(lambda: step(native))
            row.append((eager, window(graph.replay)))
            del graph
        step(False), step(True)
        d_y = float((res[True][0] - res[False][0]).abs().max())
        d_g = float((res[True][1] - res[False][1]).abs().max())
        for label, (eager, replay) in zip(("torch path", "p_native  "), row):
            say(f"    {what:20s} {label}  eager {eager[0]:8.4f} ({eager[1]:.4f} .. {eager[2]:.4f})   "
                f"graph replay {replay[0]:8.4f} ({replay[1]:.4f} .. {replay[2]:.4f})")
        say(f"    {'':20s} largest difference native - torch: output {d_y:.2e}, gradient {d_g:.2e}")
    say()

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("wrote", args.out)
