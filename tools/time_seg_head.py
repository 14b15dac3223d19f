#!/usr/bin/env python3
"""Time of the loss and metrics head (`ops.seg_loss` with tallies + backward, include/se3conv_seg_head.h) beside the recipe it
replaces, at the two shapes of the reference's tasks:

    segmentation      99 000 rows x 21 classes (a ScanNet batch), class 0 masked, 10 % unlabelled
    classification        32 rows x 40 classes (a ModelNet40 batch)

The recipe: `cross_entropy(logits, labels, ignore_index=-100, reduction="sum") / mask.sum().clamp(min=1)` forward + backward
(INTEGRATION.md, step 3), and the reference-style metrics update, `SemSegMetrics.update_metrics(logits.cpu().numpy(),
labels.cpu().numpy())` on the compacted rows -- a device-to-host copy of the logits and a synchronisation, which no graph can
hold, so it is timed eagerly only.  Each side is timed eagerly (host clock around `--iters` steps and a synchronise) and as a
replayed graph (HIP events), the sides taking turns; the kernel nodes of each graph are counted.  Nothing here is asserted or
thresholded.  Needs a GPU; no CPU fallback.

    python tools/time_seg_head.py [--out profiles/seg_head.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import se3conv3d_amd as amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200, help="steps per timed window")
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_head.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tools/time_seg_head.py needs a GPU")
dev = torch.device("cuda:0")
SHAPES = (("segmentation, 99 000 x 21", 99000, 21, (0,), 0.1), ("classification, 32 x 40", 32, 40, (), 0.0))
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def node_types(graph):
    hip = C.CDLL("libamdhip64.so")
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    raw, n = C.c_void_p(graph.raw_cuda_graph()), C.c_size_t(0)
    hip.hipGraphGetNodes(raw, None, C.byref(n))
    nodes = (C.c_void_p * n.value)()
    hip.hipGraphGetNodes(raw, nodes, C.byref(n))
    out = []
    for i in range(n.value):
        t = C.c_int(-1)
        hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(t))
        out.append(t.value)
    return out


def captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        fn()
    return graph


def eager_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / args.iters


def replay_ms(graph):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.iters):
        graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.iters


say(f"tools/time_seg_head.py on {torch.cuda.get_device_name(0)}: {args.windows} windows of {args.iters} steps per row, medians; "
    "ms per step")
for name, rows, classes, masked, unlabelled in SHAPES:
    g = torch.Generator().manual_seed(rows)
    logits = (torch.randn(rows, classes, generator=g) * 3.0).to(dev).requires_grad_(True)
    labels = torch.randint(0, classes, (rows,), generator=g)
    labels[torch.rand(rows, generator=g) < unlabelled] = -100
    labels = labels.to(dev)
    one = torch.ones((), device=dev)
    metrics = amd.SemSegMetrics(classes, list(masked), device=dev)
    # what the parent's loop does: labels of masked classes become ignore_index once per batch (its compaction, without the
    # read-back), the loss is sum / count, the metrics take the compacted rows on the host
    lab_recipe = labels.clone()
    for c in masked:
        lab_recipe[labels == c] = -100
    keep = lab_recipe != -100
    host = amd.SemSegMetrics(classes, list(masked))

    def head():
        loss = metrics.loss(logits, labels, 0.1)
        return torch.autograd.grad(loss, logits, one)[0]

    def recipe_loss():
        loss = torch.nn.functional.cross_entropy(logits, lab_recipe, ignore_index=-100, reduction="sum", label_smoothing=0.1) / keep.sum().clamp(min=1)
        return torch.autograd.grad(loss, logits, one)[0]

    def recipe_metrics():
        host.update_metrics(logits.detach()[keep].cpu().numpy(), labels[keep].cpu().numpy())

    def recipe():
        recipe_loss()
        recipe_metrics()

    d = (head() - recipe_loss()).abs().max().item()
    graphs = {"head": captured(head), "recipe, loss alone": captured(recipe_loss)}
    kinds = {k: node_types(v) for k, v in graphs.items()}
    times = {k: [] for k in ("head, eager", "head, graph", "recipe loss, eager", "recipe loss, graph", "recipe metrics, eager",
                             "recipe loss + metrics, eager")}
    for _ in range(args.windows):
        times["head, eager"].append(eager_ms(head))
        times["recipe loss, eager"].append(eager_ms(recipe_loss))
        times["recipe metrics, eager"].append(eager_ms(recipe_metrics))
        times["recipe loss + metrics, eager"].append(eager_ms(recipe))
        times["head, graph"].append(replay_ms(graphs["head"]))
        times["recipe loss, graph"].append(replay_ms(graphs["recipe, loss alone"]))
    med = {k: statistics.median(v) for k, v in times.items()}
    say()
    say(f"{name} (largest |difference| of the two gradients {d:.2e})")
    for k, v in med.items():
        say(f"  {k:32s} {v:9.4f}   (min {min(times[k]):.4f}, max {max(times[k]):.4f})")
    for k, v in kinds.items():
        say(f"  graph of {k}: {v.count(0)} kernel, {v.count(1)} memcpy, {v.count(2)} memset nodes")
    say(f"  head / recipe loss alone, graph replay:           {med['head, graph'] / med['recipe loss, graph']:.2f}")
    say(f"  head, graph / recipe loss + metrics, eager:       {med['head, graph'] / med['recipe loss + metrics, eager']:.3f}")
    say(f"  head, eager / recipe loss + metrics, eager:       {med['head, eager'] / med['recipe loss + metrics, eager']:.3f}")
    moved = rows * classes * 4
    say(f"  logits: {moved / 1e6:.2f} MB; the head reads them twice and writes them once")

with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
