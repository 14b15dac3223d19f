#!/usr/bin/env python3
"""Wall time of a DFaust step's GEOMETRY -- level-0 PCA frames (16-NN), 3 grid sub-samples with PCA frames on every level, and
the ball-query neighbourhoods the network's calls use between levels 0 .. 3 -- three ways:

  (a) the trimmed build: `PointHierarchyRotEquiv` level after level and the two-phase ball query (a read-back per level and
      per neighbourhood), eager;
  (b) the padded build (`p_padded=True`, neighbourhoods with `p_capacity`: include/se3conv_padded.h), eager, no read-back;
  (c) the padded build captured once and replayed as a HIP graph,

(b) and (c) with level capacities "input" and with 1.25 x the true level sizes; edge capacities are 1.25 x the true counts.
Every variant also asks each neighbourhood between two levels for its source-major list (`source_major()`: a second,
role-swapped query where the segments are long), as a step's backward does.  (c-) is (c) captured with `ops.SHARED_GRIDS`
off: every query of the capture sorts its source cloud itself.
Needs a GPU; there is no CPU fallback.  The variants run in one process, in turn, every call timed by the host clock around
the call and a device synchronise, after a warm-up, until every variant has run for `--seconds` and `--min-reps` calls.
Reported: the median and min .. max per variant.

    python tools/time_padded_geometry.py [--out profiles/padded_geometry.txt]
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
ap.add_argument("--seconds", type=float, default=1.0)
ap.add_argument("--min-reps", type=int, default=30)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "padded_geometry.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tools/time_padded_geometry.py needs a GPU")
dev = torch.device("cuda:0")
ops, pc = amd.ops, amd.pc
lines = []
CFG = {"pca": True, "n_frames": 2, "fixed_axis": False, "neigh_method": "knn", "neigh_kwargs": {"neigh_k": 16}}
RADII = [0.05, 0.1, 0.2]


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def run(variants):
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    while any(sum(t) < args.seconds * 1e3 or len(t) < args.min_reps for t in times.values()):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return times


raw_pts, raw_bid = W.faust_raw_batch(dev)
raw = pc.Pointcloud(raw_pts, raw_bid)
init = pc.GridSubSample(raw, 0.04)
pts = init.__subsample_tensor__(raw.pts_, "avg").contiguous()
bid = init.__subsample_tensor__(raw.batch_ids_, "max").to(torch.int32).contiguous()
n, nb = pts.shape[0], raw.num_batches()
calls = W.faust_network_calls(os.path.join(ROOT, "tests", "golden", "network_faust_calls.npz"))
keys = []
for c in calls:
    k = (c["level_in"], c["level_out"], c["radius"])
    if max(k[0], k[1]) <= len(RADII) and k not in keys:
        keys.append(k)


def trimmed():
    """(a): the trimmed levels and their two-phase queries, a read-back each."""
    pc0 = pc.PointcloudRotEquiv(pts, bid, CFG, num_batches=nb)
    hier = pc.PointHierarchyRotEquiv(pc0, len(RADII), "grid_avg", grid_radii=RADII)
    nbhs = {}
    for k in keys:
        nbhs[k] = pc.BQNeighborhood(hier.pcs_[k[0]], hier.pcs_[k[1]], k[2])
        if k[0] != k[1]:
            nbhs[k].source_major()
    return hier, nbhs


hier0, nbhs0 = trimmed()
sizes = [p.pts_.shape[0] for p in hier0.pcs_]
edges = {k: v.num_edges() for k, v in nbhs0.items()}
edge_caps = {k: int(e * 1.25) + 1 for k, e in edges.items()}
word = torch.tensor([n], dtype=torch.int32, device=dev)


def padded(level_caps):
    pc0 = pc.PointcloudRotEquiv(pts, bid, CFG, p_n_valid=word, num_batches=nb)
    hier = pc.PointHierarchyRotEquiv(pc0, len(RADII), "grid_avg", p_capacities=level_caps, p_padded=True, grid_radii=RADII)
    nbhs = {}
    for k in keys:
        nbhs[k] = pc.BQNeighborhood(hier.pcs_[k[0]], hier.pcs_[k[1]], k[2], p_capacity=edge_caps[k])
        if k[0] != k[1]:
            nbhs[k].source_major()
    return hier, nbhs


def captured(level_caps, shared=True):
    held = []
    ops.SHARED_GRIDS = shared
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        padded(level_caps)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        held.append(padded(level_caps))
    ops.SHARED_GRIDS = True
    return graph, held


say(f"tools/time_padded_geometry.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
say("per-call host time, each call ended by a device synchronise; variants alternate in one process")
say(f"DFaust-like step: {n} points in {nb} bodies, PCA frames from 16-NN (F = 2) on every level, grid sub-samples {RADII}")
say(f"  level sizes {sizes}; {len(keys)} ball-query neighbourhoods (levels in -> out, radius: edges):")
say("  " + ", ".join(f"{k[0]}->{k[1]} r={k[2]:g}: {edges[k]}" for k in keys))
caps125 = [int(s * 1.25) + 1 for s in sizes[1:]]
graphs = {"input": captured("input"), "1.25x": captured(caps125)}
unshared = captured(caps125, shared=False)
variants = {
    "(a) trimmed levels, two-phase queries, eager": trimmed,
    "(b) padded, eager, level capacities 'input'": lambda: padded("input"),
    f"(b) padded, eager, level capacities 1.25 x {caps125}": lambda: padded(caps125),
    "(c) padded, graph replay, level capacities 'input'": graphs["input"][0].replay,
    "(c) padded, graph replay, level capacities 1.25 x": graphs["1.25x"][0].replay,
    "(c-) the same, captured without shared source grids": unshared[0].replay,
}
for name, t in run(variants).items():
    say(f"  {name:<72} median {statistics.median(t):7.3f} ms  ({min(t):.3f} .. {max(t):.3f}), {len(t)} calls")
# what the replays built is what the trimmed build holds
ok = True
for tag, (graph, held) in graphs.items():
    graph.replay()
    torch.cuda.synchronize()
    hier, nbhs = held[0]
    ok = ok and hier.level_sizes() == sizes and not hier.overflowed()
    ok = ok and all(torch.equal(a.pts_[:m], b.pts_) for a, b, m in zip(hier.pcs_, hier0.pcs_, sizes))
    ok = ok and all(nbhs[k].num_edges() == edges[k] and not nbhs[k].overflowed() for k in keys)
say(f"  replayed level sizes, level points and edge counts equal the trimmed build's: {ok}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
