#!/usr/bin/env python3
"""Time of `AugPipeline.augment_batch` (include/se3conv_augment.h) against the same steps written with torch ops, one batch
element at a time, on the same device -- a stand-in for the reference's loader path (`Dataset.__getitem__` augments one scene
at a time; the reference is not needed here) -- at two shapes:

    ScanNet training list (tests/augment_configs.py SCANNET: the reference's list without its elastic step)   6 x 120 000 points
    DFaust training list  (DFAUST)                                                                           32 x   4 096 points

Per shape: 10 timed runs after 3 warm-up runs, each a host clock around the call that ends in a device synchronise (the eager
call includes the host's launch work, which is most of it at the small shape); median, minimum and maximum; the same for
replays of the captured call; and the number of graph nodes of the captured call (its launches and copies).  The stand-in
draws its parameters on the host (no read-back) but its point crop indexes with a boolean mask, as the reference does: that is
its one synchronisation per element.  Nothing here is asserted or thresholded.  Needs a GPU; no CPU fallback.

The ScanNet call carries the four extra tensors its list flags (normals, colours, labels, ids: the first is rotated and
mirrored with the points, all four are cropped); the stand-in moves the same four.  The result replaces the block between the
two marker lines of profiles/augment.txt (or is appended to it).

    python tools/time_augment.py [--out profiles/augment.txt]
"""
import argparse
import math
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import augment_configs as CFG  # noqa: E402
from se3conv3d_amd import augment  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tools/time_augment.py needs a GPU")
dev = torch.device("cuda:0")
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def axis_matrix(axis, angle):
    c, s = math.cos(angle), math.sin(angle)
    m = {0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    return torch.tensor(m, dtype=torch.float32, device=dev)


def torch_element(cfgs, pts, extras):
    """One element through the list with torch ops, parameters drawn on the host; `extras` follow their flags."""
    extras = list(extras)
    for c in cfgs:
        name = c["name"]
        flags = list(c["p_apply_extra_tensors"]) + [False] * len(extras)
        if name == "CenterAug":
            axes = torch.tensor(c.get("p_axes", [True, True, True]), device=dev)
            pts = pts - pts.mean(0) * axes
        elif name == "MirrorAug":
            flip = [a and random.random() > c["p_mirror_prob"] for a in c["p_axes"]]
            vec = torch.tensor([-1.0 if f else 1.0 for f in flip], device=dev)
            pts = pts * vec
            extras = [e * vec if f else e for e, f in zip(extras, flags)]
        elif name == "RotationAug":
            rot = axis_matrix(c["p_axis"], random.random() * (c["p_max_angle"] - c["p_min_angle"]) + c["p_min_angle"])
            pts = pts @ rot
            extras = [e @ rot if f else e for e, f in zip(extras, flags)]
        elif name == "LinearAug":
            pts = pts * (random.random() * (c["p_max_a"] - c["p_min_a"]) + c["p_min_a"]) + (random.random() * (c["p_max_b"] - c["p_min_b"]) + c["p_min_b"])
        elif name == "NoiseAug":
            pts = pts + torch.clip(torch.randn_like(pts) * c["p_stddev"], -c["p_clip"], c["p_clip"])
        elif name == "CropPtsAug":
            n = pts.shape[0]
            m = min(c["p_max_pts"] if c["p_max_pts"] > 0 else n, int(n * c["p_crop_ratio"]))
            if n > m:
                order = torch.argsort(((pts - pts[random.randrange(n)]) ** 2).sum(1))
                mask = torch.ones(n, dtype=torch.bool, device=dev)
                mask[order[m:]] = False
                pts = pts[mask]
                extras = [e[mask] if f else e for e, f in zip(extras, flags)]
        elif name == "TranslationAug":
            ratio = torch.as_tensor(c["p_max_aabb_ratio"], dtype=torch.float32, device=dev)
            u = torch.tensor([random.random() for _ in range(3)], device=dev)
            pts = pts + (pts.amax(0) - pts.amin(0)) / 2.0 * ((u * 2.0 - 1.0) * ratio)
        else:
            raise KeyError(name)
    return pts, extras


BEGIN, END = "== times (tools/time_augment.py) ==", "== end of times =="

for title, cfgs, nb, per in (("ScanNet list, 6 x 120 000 points", CFG.SCANNET, 6, 120000), ("DFaust list, 32 x 4 096 points", CFG.DFAUST, 32, 4096)):
    g = torch.Generator(device="cpu").manual_seed(1)
    pts = (torch.rand(nb * per, 3, generator=g) * torch.tensor([8.0, 6.0, 3.0])).to(dev)
    ids = torch.arange(nb, dtype=torch.int32).repeat_interleave(per).to(dev)
    word = torch.tensor([nb * per], dtype=torch.int32, device=dev)
    seed_word = torch.zeros(1, dtype=torch.int32, device=dev)
    draws = torch.rand(len(cfgs), nb, augment.AUG_DRAWS, device=dev)
    pipe = augment.AugPipeline()
    pipe.create_pipeline(cfgs)
    held = {}
    n_extra = len(cfgs[0]["p_apply_extra_tensors"])
    extras = [torch.randn(nb * per, 3, generator=g).to(dev), torch.rand(nb * per, 3, generator=g).to(dev),
              torch.randint(0, 20, (nb * per,), generator=g).to(dev), torch.arange(nb * per, dtype=torch.int32).to(dev)][:n_extra]

    def library():
        held["res"] = pipe.augment_batch(pts, ids, nb, extras, n_valid=word, seed=7, seed_tensor=seed_word, draws=draws)

    def stand_in():
        held["ref"] = [torch_element(cfgs, pts[b * per:(b + 1) * per], [e[b * per:(b + 1) * per] for e in extras])[0] for b in range(nb)]

    eager, ref = timed(library), timed(stand_in)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        library()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        library()
    replay = timed(graph.replay)
    try:
        from test_gpu_graph_nodes import node_types
        nodes = len(node_types(graph))
    except Exception as exc:  # the count is a convenience of the test helpers
        nodes = f"not counted ({exc})"
    kept = int(held["res"].n_valid_) if held["res"].n_valid_ is not None else nb * per
    say(f"{title}, {n_extra} extra tensors")
    say(f"  library, eager call      median {eager[0]:8.3f} ms   min {eager[1]:8.3f}   max {eager[2]:8.3f}   ({args.runs} runs)")
    say(f"  library, graph replay    median {replay[0]:8.3f} ms   min {replay[1]:8.3f}   max {replay[2]:8.3f}   graph nodes: {nodes}")
    say(f"  torch ops per element    median {ref[0]:8.3f} ms   min {ref[1]:8.3f}   max {ref[2]:8.3f}")
    say(f"  rows kept by the library: {kept} of {nb * per}; by the stand-in: {sum(p.shape[0] for p in held['ref'])}")
    say()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
old = open(args.out).read() if os.path.exists(args.out) else ""
block = "\n".join([BEGIN] + lines + [END]) + "\n"
if BEGIN in old and END in old:
    text = old[:old.index(BEGIN)] + block + old[old.index(END) + len(END):].lstrip("\n")
else:
    text = old + block
with open(args.out, "w") as fh:
    fh.write(text)
