#!/usr/bin/env python3
"""Time of the ScanNet training list with and without its ElasticDistortionAug step (include/se3conv_elastic.h), at the shape of
profiles/augment.txt: 6 x 120 000 points in a box of 8 x 6 x 3 and the four extra tensors the list flags.

The method of tools/time_augment.py: per measurement 10 timed runs after 3 warm-up runs, each a host clock around the call
that ends in a device synchronise; median, minimum and maximum; eager calls and replays of the captured call.  Every
measurement runs in a child process of its own, and the children alternate between this tree and a checkout of the parent
commit (`--parent`, with its library built), `--rounds` times over: the parent's call WITHOUT the step is the yardstick, this
tree's call without the step shows that the default path did not move, this tree's call with the step is the new number.
Also written: the graph node count, the grid cells and bytes the step writes, the share of generated cells that are halo
recomputation, and the CPU time of the same step written with torch ops (conv3d + grid_sample, one element at a time) -- a
stand-in for the reference's host path, which is not needed here.  Nothing is asserted or thresholded.  Needs a GPU.

    python tools/time_elastic.py --parent <checkout of the parent commit> [--out profiles/elastic.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "elastic.txt"))
ap.add_argument("--worker", choices=["with", "without", "cpu"], default=None, help="(internal) one measurement, printed as JSON")
ap.add_argument("--tree", default=ROOT, help="(internal) the tree whose package the worker imports")
args = ap.parse_args()
NB, PER = 6, 120000


def worker():
    sys.path.insert(0, args.tree)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch

    import augment_configs as CFG

    g = torch.Generator(device="cpu").manual_seed(1)
    host_pts = torch.rand(NB * PER, 3, generator=g) * torch.tensor([8.0, 6.0, 3.0])

    def timed(fn, sync):
        for _ in range(3):
            fn()
        sync()
        times = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            fn()
            sync()
            times.append((time.perf_counter() - t0) * 1e3)
        return [statistics.median(times), min(times), max(times)]

    if args.worker == "cpu":   # the step alone with torch ops on the host, one element at a time
        import torch.nn.functional as fn

        cfg = CFG.SCANNET_ELASTIC

        def element(x):
            lo, hi = x.amin(0), x.amax(0)
            c = x.clone()
            for gran, mag in zip(cfg["p_granularity"], cfg["p_magnitude"]):
                dims = [int(v) + 3 for v in torch.floor((hi - lo) / gran).tolist()]
                field = torch.randn(1, 3, *dims)
                for _ in range(2):
                    for axis in range(3):
                        shape = [3, 1, 1, 1, 1]
                        shape[2 + axis] = 3
                        field = fn.conv3d(field, torch.full(shape, 1.0 / 3.0), padding="same", groups=3)
                at = ((c - lo) / (hi - lo) * 2.0 - 1.0).flip(1).reshape(1, -1, 1, 1, 3)   # grid_sample's x is the LAST grid axis
                c = c + fn.grid_sample(field, at, align_corners=True, padding_mode="border")[0, :, :, 0, 0].t() * mag
            return c

        out = {"cpu": timed(lambda: [element(host_pts[b * PER:(b + 1) * PER]) for b in range(NB)], lambda: None), "threads": torch.get_num_threads()}
        print("RESULT " + json.dumps(out))
        return
    from se3conv3d_amd import augment

    dev = torch.device("cuda:0")
    pts = host_pts.to(dev)
    ids = torch.arange(NB, dtype=torch.int32).repeat_interleave(PER).to(dev)
    word = torch.tensor([NB * PER], dtype=torch.int32, device=dev)
    seed_word = torch.zeros(1, dtype=torch.int32, device=dev)
    extras = [torch.randn(NB * PER, 3, generator=g).to(dev), torch.rand(NB * PER, 3, generator=g).to(dev),
              torch.randint(0, 20, (NB * PER,), generator=g).to(dev), torch.arange(NB * PER, dtype=torch.int32).to(dev)]
    out, kw, held = {}, {}, {}
    if args.worker == "with":
        cfgs = CFG.SCANNET[:6] + [CFG.SCANNET_ELASTIC] + CFG.SCANNET[6:]
        pipe = augment.AugPipeline(p_elastic=True)
        pipe.create_pipeline(cfgs)
        kw["grid_capacity"] = out["capacity"] = pipe.elastic_capacity((8.0, 6.0, 3.0), NB)
    else:
        cfgs = CFG.SCANNET
        pipe = augment.AugPipeline()
        pipe.create_pipeline(cfgs)
    draws = torch.rand(len(cfgs), NB, augment.AUG_DRAWS, generator=g).to(dev)
    draws[:, :, 0] = 0.5   # every gate open: the elastic step on all six elements

    def library():
        held["res"] = pipe.augment_batch(pts, ids, NB, extras, n_valid=word, seed=7, seed_tensor=seed_word, draws=draws, **kw)

    out["eager"] = timed(library, torch.cuda.synchronize)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        library()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        library()
    out["replay"] = timed(graph.replay, torch.cuda.synchronize)
    from test_gpu_graph_nodes import node_types
    out["nodes"] = len(node_types(graph))
    out["kept"] = int(held["res"].n_valid_)
    if args.worker == "with":
        import elastic_reference as E

        out["overflow"] = int(held["res"].overflow_)
        # the step's own plan, once more by hand on the cloud as it stands in front of the step
        head = augment.AugPipeline()
        head.create_pipeline(cfgs[:6])
        mid = head.augment_batch(pts, ids, NB, [], n_valid=word, seed=7, seed_tensor=seed_word, draws=draws[:6])
        counts, stats = augment.aug_stats(mid.pts_, ids, NB, None, word)
        table = augment.aug_elastic_plan(counts, stats, draws[6], 0.95, CFG.SCANNET_ELASTIC["p_granularity"], out["capacity"])[0].cpu().numpy()
        out["dims"] = table[:, :, 0:3].tolist()
        out["cells"] = int(sum(int(e[0] * e[1] * e[2]) for e in table.reshape(-1, 4) if e[3] >= 0))
        out["generated"], out["halo"] = (int(v) for v in E.halo_share(table))
    print("RESULT " + json.dumps(out))


def child(tree, what):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", what, "--tree", tree, "--runs", str(args.runs)]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if done.returncode != 0:
        sys.exit(f"{' '.join(cmd)} failed ({done.returncode}):\n{done.stdout[-2000:]}\n{done.stderr[-4000:]}")
    return json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    series = {"parent, without the step": [], "this tree, without the step": [], "this tree, with the step": []}
    for _ in range(args.rounds):   # alternating: one child each per round
        if args.parent:
            series["parent, without the step"].append(child(os.path.abspath(args.parent), "without"))
        series["this tree, without the step"].append(child(ROOT, "without"))
        series["this tree, with the step"].append(child(ROOT, "with"))
    say(f"ScanNet training list, {NB} x {PER} points, 4 extra tensors; {args.rounds} alternating rounds of child processes, {args.runs} timed runs each.")
    say("Per line: the median over the rounds of the per-child medians, and the smallest and largest single run of any round (ms).")
    for name, runs in series.items():
        if not runs:
            continue
        for key in ("eager", "replay"):
            meds = [r[key][0] for r in runs]
            say(f"  {name:30s} {key:6s}  median {statistics.median(meds):8.3f}   per round {' '.join(f'{m:.3f}' for m in meds)}   "
                f"min {min(r[key][1] for r in runs):8.3f}   max {max(r[key][2] for r in runs):8.3f}   graph nodes {runs[0]['nodes']}")
    w = series["this tree, with the step"][0]
    say(f"  rows kept: {w['kept']} of {NB * PER}; overflow word {w['overflow']}; grid_capacity {w['capacity']} cells ({w['capacity'] * 16 / 2 ** 20:.1f} MiB allocated)")
    say(f"  grid dims per element and octave: {w['dims'][0]} ... ; cells written {w['cells']} = {w['cells'] * 16 / 2 ** 20:.2f} MiB of 16-byte stores")
    say(f"  cells generated in LDS {w['generated']}, of which halo recomputation {w['halo']} ({100.0 * w['halo'] / max(w['generated'], 1):.1f} %)")
    cpu = child(ROOT, "cpu")
    say(f"  STAND-IN, not the reference: the step alone with torch ops on the host (conv3d + grid_sample per element, {cpu['threads']} threads): "
        f"median {cpu['cpu'][0]:.1f} ms   min {cpu['cpu'][1]:.1f}   max {cpu['cpu'][2]:.1f}")
    begin, end = "== times (tools/time_elastic.py) ==", "== end of times =="
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    old = open(args.out).read() if os.path.exists(args.out) else ""
    block = "\n".join([begin] + lines + [end]) + "\n"
    text = old[:old.index(begin)] + block + old[old.index(end) + len(end):].lstrip("\n") if begin in old and end in old else old + block
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    worker() if args.worker else main()
