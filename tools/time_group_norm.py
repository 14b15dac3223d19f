#!/usr/bin/env python3
"""Forward and backward time of the point-cloud group norm (`se3_group_norm_fwd` / `se3_group_norm_bwd`,
include/se3conv_group_norm.h) beside training batch norm (`se3_bn_fwd` / `se3_bn_bwd`, include/se3conv.h) on the same rows,
through the C entry points themselves (no autograd, no allocation inside the timed region), at two shapes:

    headline level      8 scenes,  65 536 points in all, F = 2, C =  64, G = 8
    DFaust level       32 bodies x 2 200 points,         F = 2, C = 128, G = 8

Batch norm is the yardstick: it makes the same passes over `x` and `dy` (one that sums, one that writes) but keeps one table
per channel, where group norm keeps one per (chunk, element, channel).  Each entry point is captured as a graph of `--calls`
calls and the replays are timed with HIP events, the four entry points taking turns window by window; ids are sorted (a
batch as the library's levels hold it) and, for group norm, also shuffled.  Nothing here is asserted or thresholded.  Needs a
GPU; no CPU fallback.

    python tools/time_group_norm.py [--out profiles/group_norm.txt] [--sweep 32,64,256,512]

`--sweep`: after the run on the library as built, one child process per value on the variant library
`lib/libse3conv_hip_gn<K>.so` (SE3_LIB_SUFFIX=_gn<K>: a build of a tree that differs in SE3_GROUP_NORM_CHUNK alone), and a table
of all of them with the workspace sizes -- how the constant was chosen."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import se3conv3d_amd as amd  # noqa: E402
from se3conv3d_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=0.5, help="timed replays per entry point and shape, in all")
ap.add_argument("--calls", type=int, default=20, help="calls per captured graph")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_norm.txt"))
ap.add_argument("--sweep", default="", help="comma-separated chunk sizes whose variant libraries exist")
ap.add_argument("--json", action="store_true", help="(child of --sweep) print one JSON line of medians, write no file")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tools/time_group_norm.py needs a GPU")
dev = torch.device("cuda:0")
SHAPES = (("headline level, 8 x 8 192", [8192] * 8, 2, 64, 8),
          ("DFaust level, 32 x 2 200", [2200] * 32, 2, 128, 8))
lines = []


def say(text=""):
    if not args.json:
        print(text, flush=True)
    lines.append(text)


def captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        for _ in range(args.calls):
            fn()
    return graph


def take_turns(graphs):
    """ms per call of every graph of `graphs` (name -> graph of `args.calls` calls): one replay each in turn, until every one
    has run for `args.seconds`; (median, min, max, windows)."""
    times = {k: [] for k in graphs}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    while min(sum(v) for v in times.values()) * args.calls < args.seconds * 1e3 or min(len(v) for v in times.values()) < 5:
        for k, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / args.calls)
    return {k: (statistics.median(v), min(v), max(v), len(v)) for k, v in times.items()}


def measure():
    lib = _lib.load()
    p = lambda v: v.data_ptr()
    result = {}
    for name, sizes, f, c, groups in SHAPES:
        nb, n = len(sizes), sum(sizes)
        gen = torch.Generator().manual_seed(n)
        rows = n * f
        x, dy = torch.randn(rows, c, generator=gen).to(dev), torch.randn(rows, c, generator=gen).to(dev)
        gamma, beta = (torch.rand(c, generator=gen) + 0.5).to(dev), torch.rand(c, generator=gen).to(dev)
        sorted_ids = torch.repeat_interleave(torch.arange(nb, dtype=torch.int32), torch.tensor(sizes))
        ids = {"sorted ids": sorted_ids.to(dev), "shuffled ids": sorted_ids[torch.randperm(n, generator=gen)].to(dev)}
        y, dx = torch.empty_like(x), torch.empty_like(x)
        mean, invstd = torch.empty(nb, groups, device=dev), torch.empty(nb, groups, device=dev)
        dgamma, dbeta = torch.empty(c, device=dev), torch.empty(c, device=dev)
        need = lib.se3_group_norm_workspace_bytes(n, f, nb, c, groups)
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        bn_mean, bn_invstd = torch.empty(c, device=dev), torch.empty(c, device=dev)
        run_mean, run_var = torch.zeros(c, device=dev), torch.ones(c, device=dev)
        bn_need = lib.se3_glue_workspace_bytes(c)
        bn_ws = torch.empty(max(bn_need, 256), dtype=torch.uint8, device=dev)

        def gn_fwd(which):
            _lib.check(lib.se3_group_norm_fwd(p(x), p(gamma), p(beta), p(ids[which]), n, f, None, nb, c, groups, 1e-8, p(y), p(mean),
                                              p(invstd), p(ws), ws.numel(), amd.ops._stream(dev)), "se3_group_norm_fwd")

        def gn_bwd(which):
            _lib.check(lib.se3_group_norm_bwd(p(dy), p(x), p(gamma), p(mean), p(invstd), p(ids[which]), n, f, None, nb, c, groups,
                                              p(dx), p(dgamma), p(dbeta), p(ws), ws.numel(), amd.ops._stream(dev)), "se3_group_norm_bwd")

        def bn_fwd():
            _lib.check(lib.se3_bn_fwd(p(x), p(gamma), p(beta), rows, c, 1e-5, 0.2, p(run_mean), p(run_var), None, p(y), p(bn_mean),
                                      p(bn_invstd), p(bn_ws), bn_ws.numel(), amd.ops._stream(dev)), "se3_bn_fwd")

        def bn_bwd():
            _lib.check(lib.se3_bn_bwd(p(dy), p(x), p(bn_mean), p(bn_invstd), p(gamma), rows, c, p(dx), p(dgamma), p(dbeta), p(bn_ws),
                                      bn_ws.numel(), amd.ops._stream(dev)), "se3_bn_bwd")

        graphs = {"se3_bn_fwd": captured(bn_fwd), "se3_bn_bwd": captured(bn_bwd)}
        for which in ids:
            gn_fwd(which)                                                  # (the backward call reads the saved statistics)
            graphs[f"se3_group_norm_fwd, {which}"] = captured(lambda w=which: gn_fwd(w))
            graphs[f"se3_group_norm_bwd, {which}"] = captured(lambda w=which: gn_bwd(w))
        got = take_turns(graphs)
        say(f"{name}: {nb} elements, {n} points, F = {f}, C = {c}, G = {groups} ({rows * c * 4 / 1e6:.2f} MB of features); "
            f"group-norm workspace {need} bytes, batch-norm workspace {bn_need} bytes")
        for k, (med, lo, hi, windows) in got.items():
            say(f"    {k:36s} {med:8.4f} ({lo:.4f} .. {hi:.4f})   {windows} windows")
        say()
        result[name] = {"workspace": need, **{k: v[0] for k, v in got.items()}}
    return result


suffix = os.environ.get("SE3_LIB_SUFFIX", "")
chunk = suffix[3:] if suffix.startswith("_gn") and suffix[3:].isdigit() else str(_lib.GROUP_NORM_CHUNK)
say("group norm beside training batch norm, through the C entry points: ms per call, median (min .. max) over windows of "
    f"{args.calls} calls replayed as one graph (HIP events), the entry points taking turns")
say(f"device: {torch.cuda.get_device_name(0)}; SE3_GROUP_NORM_CHUNK = {chunk} points")
say()
res = measure()
if args.json:
    print(json.dumps({"chunk": int(chunk), "result": res}), flush=True)
    sys.exit(0)
if args.sweep:
    table = {int(chunk): res}
    for k in [int(v) for v in args.sweep.split(",")]:
        env = dict(os.environ, SE3_LIB_SUFFIX=f"_gn{k}")
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--json", "--seconds", str(args.seconds), "--calls",
                              str(args.calls)], env=env, capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            say(f"chunk {k}: the variant run failed ({out.stderr.strip().splitlines()[-1:]})")
            continue
        table[k] = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])["result"]
    ks = sorted(table, reverse=True)
    say("The sweep of SE3_GROUP_NORM_CHUNK: the same measurement on builds that differ in the constant alone, one process each;")
    say("ms per call (median), and the workspace of one call")
    say()
    say(f"    {'CHUNK (points)':57s}" + "".join(f"{k:>9d}" for k in ks))
    for name, *_ in SHAPES:
        for key in [k for k in table[ks[0]][name] if k != "workspace"]:
            say(f"    {name[:22]:22s} {key:34s}" + "".join(f"{table[k][name][key]:9.4f}" for k in ks))
        say(f"    {name[:22]:22s} {'workspace (MB)':34s}" + "".join(f"{table[k][name]['workspace'] / 1e6:9.1f}" for k in ks))
    say()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("wrote", args.out)
