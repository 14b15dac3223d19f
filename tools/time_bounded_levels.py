#!/usr/bin/env python3
"""Wall time of the hierarchy build, level after level with one read-back each (the `PointHierarchy` of today) against
the bounded build (`ops.grid_levels_bounded`: all levels in one library call, sizes on the device, ONE read-back in
`trim()`), eager and as a replayed HIP graph.  Two clouds: the DFaust step's raw batch (32 x 4 096 points, initial
sub-sample 0.04, then the four grid sub-samples `workloads.faust_clouds` uses) and the headline cloud (65 536 uniform
points, 3 sub-sampling levels).  Needs a GPU; there is no CPU fallback.

The variants run in one process, in turn (a, b, ... a, b, ...), every call timed by the host clock around the call and a
device synchronise, after a warm-up, until every variant has run for `--seconds` and `--min-reps` calls.  Reported: the
median and min .. max per variant, and the kernel nodes of the captured bounded call.

    python tools/time_bounded_levels.py [--out profiles/bounded_levels.txt]
"""
import argparse
import ctypes as C
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
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--min-reps", type=int, default=30)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bounded_levels.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tools/time_bounded_levels.py needs a GPU")
dev = torch.device("cuda:0")
ops, pc = amd.ops, amd.pc
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def node_count(graph):
    """(all nodes, memset nodes) of a captured graph (the walk of tests/test_gpu_graph_nodes.py)."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    raw, n = C.c_void_p(graph.raw_cuda_graph()), C.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, C.byref(n)) == 0
    nodes = (C.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(raw, nodes, C.byref(n)) == 0
    memsets = 0
    for i in range(n.value):
        t = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(t)) == 0
        memsets += t.value == 2
    return n.value, memsets


def run(variants):
    """name -> list of per-call milliseconds, the variants taking turns."""
    for fn in variants.values():
        for _ in range(5):
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


def case(title, pts, bid, radii):
    n, n_levels = pts.shape[0], len(radii)
    cloud = pc.Pointcloud(pts, bid)
    n_batches = cloud.num_batches()
    sizes = [p.pts_.shape[0] for p in pc.PointHierarchy(cloud, n_levels, "grid_avg", grid_radii=radii).pcs_[1:]]
    caps = [int(s * 1.25) + 1 for s in sizes]
    say(f"{title}: {n} points, {n_batches} batch element(s), cells {radii}")
    say(f"  level sizes {sizes}, capacities (1.25 x) {caps}")

    def unbounded_ops():
        p, b = pts, bid
        for r in radii:
            c = ops.grid_subsample(p, b, r, n_batches)
            p, b = c.pts, c.batch_ids

    # (c): one captured call on the very buffers, replayed; the read-back stays outside the graph
    held = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.grid_levels_bounded(pts, bid, radii, caps, n_batches)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        held.append(ops.grid_levels_bounded(pts, bid, radii, caps, n_batches))
    nodes, memsets = node_count(graph)

    def replay():
        graph.replay()
        held[0].trim()

    variants = {
        "(a)  PointHierarchy, level after level (today)": lambda: pc.PointHierarchy(cloud, n_levels, "grid_avg", grid_radii=radii),
        "(a-) ops.grid_subsample chain, no cloud objects": unbounded_ops,
        "(b)  PointHierarchy(p_capacities), eager + trim()": lambda: pc.PointHierarchy(cloud, n_levels, "grid_avg", grid_radii=radii,
                                                                                      p_capacities=caps),
        "(b-) ops.grid_levels_bounded + trim(), no cloud objects": lambda: ops.grid_levels_bounded(pts, bid, radii, caps, n_batches).trim(),
        "(c)  graph replay + trim(), no cloud objects": replay,
    }
    for name, t in run(variants).items():
        say(f"  {name:<58} median {statistics.median(t):7.3f} ms  ({min(t):.3f} .. {max(t):.3f}), {len(t)} calls")
    say(f"  captured bounded call: {nodes} nodes for {n_levels} levels ({nodes / n_levels:.1f} per level), {memsets} memset nodes; "
        "se3_grid_subsample issues the same kernels per level (the stages are one shared function) and ops.grid_subsample "
        "adds a torch.zeros fill and the read-back")
    same = all(torch.equal(a.pts_, b.pts_) for a, b in zip(
        pc.PointHierarchy(cloud, n_levels, "grid_avg", grid_radii=radii).pcs_,
        pc.PointHierarchy(cloud, n_levels, "grid_avg", grid_radii=radii, p_capacities=caps).pcs_))
    say(f"  level points of (a) and (b) bit-identical: {same}")
    say()


say(f"tools/time_bounded_levels.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
say("per-call host time, each call ended by a device synchronise; variants alternate in one process")
say()
raw_pts, raw_bid = W.faust_raw_batch(dev)
raw = pc.Pointcloud(raw_pts, raw_bid)
init = pc.GridSubSample(raw, 0.04)
case("DFaust step (raw batch 32 x 4096, initial sub-sample 0.04)", init.__subsample_tensor__(raw.pts_, "avg").contiguous(),
     init.__subsample_tensor__(raw.batch_ids_, "max").contiguous(), [0.05, 0.1, 0.2, 0.4])
torch.manual_seed(0)
n = W.WORKLOADS["headline"]["points"]
r0 = W.radius_for_degree(n, W.WORKLOADS["headline"]["degree"])
case("headline cloud", torch.rand(n, 3, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), [r0 * 2 ** i for i in range(3)])
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
