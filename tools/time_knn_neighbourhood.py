#!/usr/bin/env python3
"""Wall time of a k-NN neighbourhood of a cloud against itself on TRIMMED clouds, two ways:

  (a) the mask-and-cumsum build of `KnnNeighborhood(pc, pc, k)`: the `[N * k, 2]` list with its empty slots, a boolean-mask
      index (a device read-back of the edge count) and a cumsum of the mask;
  (b) the capacity-bounded build `KnnNeighborhood(pc, pc, k, p_capacity=N * k)` (`se3_knn_edges_bounded`,
      include/se3conv_knn_edges.h): count, scan and store on the device, no read-back,

and of a convolution's forward + FIRST backward over each list (32 -> 32 channels, F = 2), which includes the transposition
of the list the backward reads (`se3_csr_transpose_bounded`, for (b) on the device-side edge count).  The id table is the
cloud's cached one in both builds (`_self_knn_ids`), so the search itself is outside both timings.
Shapes: 65 536 points, k = 16, and 32 x 2 200 points, k = 16.
Needs a GPU; there is no CPU fallback.  The variants run in one process, in turn, every call timed by the host clock around
the call and a device synchronise, after a warm-up, until every variant has run for `--seconds` and `--min-reps` calls.
Reported: the median and min .. max per variant.

    python tools/time_knn_neighbourhood.py [--out profiles/knn_edges.txt]
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

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=1.0)
ap.add_argument("--min-reps", type=int, default=30)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_edges.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tools/time_knn_neighbourhood.py needs a GPU")
dev = torch.device("cuda:0")
pc = amd.pc
lines = []
K, F, C = 16, 2, 32


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


say(f"tools/time_knn_neighbourhood.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
say("per-call host time, each call ended by a device synchronise; variants alternate in one process")
for label, sizes in (("65 536 points in one element", [65536]), ("32 x 2 200 points", [2200] * 32)):
    g = torch.Generator().manual_seed(0)
    n = sum(sizes)
    pts = torch.rand(n, 3, generator=g).to(dev)
    bid = torch.repeat_interleave(torch.arange(len(sizes), dtype=torch.int32), torch.tensor(sizes)).to(dev)
    cloud = pc.PointcloudRotEquiv(pts, bid, {"pca": False, "n_frames": F, "fixed_axis": False}, num_batches=len(sizes))
    conv = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu").create_conv_layer(C, C).to(dev)
    conv.norm_neigh_dist_.fill_(float(n / len(sizes)) ** (1.0 / 3.0)), conv.norm_num_neighs_.fill_(1.0 / K)
    x = torch.randn(n * F, C, device=dev, requires_grad=True)
    go = torch.randn(n * F, C, device=dev)
    build = {"(a) mask + cumsum": lambda: pc.KnnNeighborhood(cloud, cloud, K),
             "(b) bounded, capacity N * k": lambda: pc.KnnNeighborhood(cloud, cloud, K, p_capacity=n * K)}

    def step(make):
        nbh = make()                                # a fresh list: its transposition is built by this backward
        x.grad = None
        conv(p_pc_in=cloud, p_pc_out=cloud, p_in_features=x, p_neighborhood=nbh).backward(go)

    a, b = build["(a) mask + cumsum"](), build["(b) bounded, capacity N * k"]()
    e = a.num_edges()
    same = b.num_edges() == e and torch.equal(b.neighbors_i32_[:e], a.neighbors_) and torch.equal(b.start_ids_, a.start_ids_)
    say(f"{label}, k = {K}: {e} edges; the two builds hold the same list: {same}")
    variants = {f"build {name}": fn for name, fn in build.items()}
    variants.update({f"build + convolution forward + first backward, {name}": (lambda fn=fn: step(fn)) for name, fn in build.items()})
    for name, t in run(variants).items():
        say(f"  {name:<72} median {statistics.median(t):7.3f} ms  ({min(t):.3f} .. {max(t):.3f}), {len(t)} calls")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
