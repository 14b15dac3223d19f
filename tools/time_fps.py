#!/usr/bin/env python3
"""Device time of farthest-point sampling (`ops.fps` -> se3_fps, include/se3conv_fps.h) at three batch shapes, ratio 0.25:

    32 x 2 200 points    (a DFaust-like batch: register-resident form, 32 of 256 CUs busy)
    16 x 6 900 points    (register-resident form, 16 CUs busy)
     1 x 150 000 points  (one scene: streaming form, ONE CU busy -- the known cost of exact FPS without grid barriers)

and beside each a plain-torch loop of the same contract on the same GPU (all elements of the batch advanced together,
one pick per iteration: subtract, square, add, minimum, mask, argmax), whose ids are compared with the library's.
HIP events around the calls, after a warm-up; nothing here is asserted or thresholded.  Needs a GPU; no CPU fallback.

    python tools/time_fps.py [--out profiles/fps.txt]
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
ap.add_argument("--seconds", type=float, default=0.5, help="keep repeating the library call for this long")
ap.add_argument("--min-reps", type=int, default=3)
ap.add_argument("--ratio", type=float, default=0.25)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fps.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tools/time_fps.py needs a GPU")
dev = torch.device("cuda:0")
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def torch_fps(pts, m):
    """The contract on [B, n, 3] equal-sized elements starting at each element's first row: ids [B, m] inside the
    elements.  No host synchronisation inside the loop."""
    b, n, _ = pts.shape
    mind = torch.full((b, n), float("inf"), device=pts.device)
    marked = torch.zeros((b, n), dtype=torch.bool, device=pts.device)
    ids = torch.empty((b, m), dtype=torch.int64, device=pts.device)
    p = torch.zeros((b, 1), dtype=torch.int64, device=pts.device)
    rows = torch.arange(b, device=pts.device)
    for j in range(m):
        ids[:, j] = p[:, 0]
        marked[rows, p[:, 0]] = True
        if j + 1 == m:
            break
        d = pts - pts[rows, p[:, 0]][:, None, :]
        d = d * d
        mind = torch.minimum(mind, (d[..., 0] + d[..., 1]) + d[..., 2])
        p = torch.argmax(mind.masked_fill(marked, -1.0), dim=1, keepdim=True)
    return ids


say(f"farthest-point sampling, ratio {args.ratio}: se3_fps against a plain-torch loop of the same contract")
say(f"device: {torch.cuda.get_device_name(0)}; times in ms (HIP events)")
say()
for n_el, n_pts in ((32, 2200), (16, 6900), (1, 150000)):
    g = torch.Generator().manual_seed(n_el)
    pts = torch.rand(n_el * n_pts, 3, generator=g).to(dev)
    bid = torch.arange(n_el, dtype=torch.int32).repeat_interleave(n_pts).to(dev)
    call = lambda: amd.ops.fps(pts, bid, args.ratio, n_el)
    call()
    torch.cuda.synchronize()
    times, res = [], None
    while sum(times) < args.seconds * 1e3 or len(times) < args.min_reps:
        ms, res = timed(call)
        times.append(ms)
    ids, d2, starts = res.trim()
    m = int(starts[1])
    form = "resident" if n_pts <= amd._lib.FPS_RESIDENT_MAX else "streaming"
    say(f"{n_el:3d} x {n_pts:6d} points -> {n_el} x {m} samples ({form} form)")
    say(f"    se3_fps     median {statistics.median(times):10.3f}   min {min(times):10.3f}   max {max(times):10.3f}   "
        f"({len(times)} calls; {statistics.median(times) * 1e3 / m:.2f} us per pick)")
    cube = pts.reshape(n_el, n_pts, 3)
    if n_el * n_pts <= 100000:
        torch_fps(cube, min(m, 20))  # warm-up of the ops' first launches
    t_ms, t_ids = timed(lambda: torch_fps(cube, m))
    same = torch.equal((t_ids + torch.arange(n_el, device=dev)[:, None] * n_pts).reshape(-1), ids.to(torch.int64))
    say(f"    torch loop         {t_ms:10.3f}   (1 call; {t_ms * 1e3 / m:.2f} us per pick; ids {'equal' if same else 'DIFFER'})")
    say()

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("wrote", args.out)
