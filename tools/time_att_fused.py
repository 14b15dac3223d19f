#!/usr/bin/env python3
"""What profiles/att_fused.txt records for the entry points of include/se3conv_att_fused.h and the layers with `p_fused=True`.
Needs a GPU; no CPU fallback; nothing here is asserted or thresholded.

  1. Error ratios: observed error / bound per tensor, over the cases of tests/att_fused_reference.py (the per-element float64
     restatement; the bound is 8 x its float32 emulation) -- the figures tests/test_gpu_att_fused.py asserts to be <= 1.
  2. Time of one step, forward + backward (eager autograd, device events around each step after a warm-up), at the shape of
     profiles/att_layers.txt: N = 65 536 points in 8 batch elements, 32 nearest neighbours per point, C_in = C_out = V = 64,
     K = 32, 4 heads.  MultiHeadAttLayer and LoRAttConvLayer, each with `p_fused=False` and `p_fused=True` IN ONE PROCESS on one
     box, the two settings alternating step by step over the same weights, cloud and input; median, min .. max and spread of
     `--steps` steps; the peak of the allocator over the steps of each setting; and the two settings' out, dx and parameter
     gradients against each other at that size (whole-tensor rel_err).
  3. The fused layers' time kernel by kernel, from the library's timing hooks (se3_profile_*), in steps of their own: the
     hooks put events around every launch and are not part of the timed steps.

    python tools/time_att_fused.py [--out profiles/att_fused.txt] [--points 65536] [--steps 10]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import att_fused_reference as R  # noqa: E402
import se3conv3d_amd as amd  # noqa: E402
from se3conv3d_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "att_fused.txt"))
ap.add_argument("--points", type=int, default=65536)
ap.add_argument("--neighbours", type=int, default=32)
ap.add_argument("--channels", type=int, default=64)
ap.add_argument("--basis", type=int, default=32)
ap.add_argument("--heads", type=int, default=4)
ap.add_argument("--steps", type=int, default=10)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tools/time_att_fused.py needs a GPU")
dev = torch.device("cuda:0")
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
n_ = lambda a: a.detach().cpu().numpy()
rel_err = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))


# ----------------------------------------------------------------------------------------------------------- error ratios
def ratios():
    b = R.bounds()
    say("observed error / bound (bound = 8 x the float32 emulation: " + ", ".join(f"{k} {v:.3g}" for k, v in b.items()) + ")")
    say(f"{'case':44s} " + " ".join(f"{name:>7s}" for name in R.ENTRIES))
    for i, (n, v, h, k, deg, hub, kind) in enumerate(R.CASES):
        case = R.case(500 + i, n, v, h, k, deg, hub, kind)
        phi, x, pe = (t(case[name]).requires_grad_(True) for name in ("phi", "x", "pe"))
        out = amd.ops.FusedBasisAttention.apply(phi, x, pe, t(case["neighbors"]), t(case["ends"]), h)
        att = out.grad_fn.saved_tensors[5]
        out.backward(t(case["grad_out"]))
        got = {"att": att, "out": out, "dphi": phi.grad, "dx": x.grad, "dpe": pe.grad}
        want, scale = R.both(case)
        say(f"{f'N={n} V={v} H={h} K={k} deg<={deg} hub={hub} {kind}':44s} " +
            " ".join(f"{R.worst(n_(got[name]), want[name], scale[name]) / b[name]:7.3f}" for name in R.ENTRIES))


# ------------------------------------------------------------------------------------------------------------------ time
def profile_table(lib):
    buf = C.create_string_buffer(1 << 16)
    lib.se3_profile_tags(buf, len(buf))
    table = {}
    for tag in filter(None, buf.value.decode().split(",")):
        ms, cnt = C.c_double(0), C.c_int64(0)
        lib.se3_profile_read(tag.encode(), C.byref(ms), C.byref(cnt))
        if cnt.value:
            table[tag] = (ms.value, cnt.value)
    return table


def times():
    torch.manual_seed(0)
    lib = _lib.load()
    npts, nn, c, kb, heads = args.points, args.neighbours, args.channels, args.basis, args.heads
    pts = torch.rand(npts, 3, device=dev)
    ids = torch.arange(npts, device=dev, dtype=torch.int32) // (npts // 8)
    pc = amd.pc.Pointcloud(pts, ids)
    nbh = amd.pc.KnnNeighborhood(pc, pc, nn)
    e = nbh.neighbors_.shape[0]
    say(f"N = {npts} points in 8 batch elements, {nn} nearest neighbours each: E = {e}; C_in = C_out = V = {c}, K = {kb}, {heads} heads; "
        f"forward + backward, eager, ms: median (min .. max; spread = max - min) of {args.steps} steps per setting, the settings alternating")
    x = torch.randn(npts, c, device=dev, requires_grad=True)
    g = torch.randn(npts, c, device=dev)
    diff = pts[nbh.neighbors_[:, 1].long()] - pts[nbh.neighbors_[:, 0].long()]
    rho = 1.0 / (2.0 * float(diff.norm(dim=1).mean()))
    for name, factory in (("MultiHeadAttLayer", amd.MultiHeadAttLayerFactory), ("LoRAttConvLayer", amd.LoRAttConvLayerFactory)):
        convs = {fused: factory(3, kb, "single", heads, p_fused=fused).create_conv_layer(c, c).to(dev) for fused in (False, True)}
        convs[True].load_state_dict(convs[False].state_dict())
        for conv in convs.values():
            with torch.no_grad():
                conv.norm_neigh_dist_.fill_(rho), conv.norm_num_neighs_.fill_(npts / e)

        def step(conv):
            for p in (x, *conv.parameters()):
                p.grad = None
            out = conv(pc, pc, x, nbh)
            out.backward(g)
            return out

        results, ms, peak = {}, {False: [], True: []}, {}
        for fused in (False, True):                       # warm-up, the results of both settings, and the peak of each alone
            step(convs[fused])
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = step(convs[fused])
            torch.cuda.synchronize()
            peak[fused] = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
            results[fused] = {"out": out.detach().clone(), "dx": x.grad.clone(),
                              **{n: p.grad.clone() for n, p in convs[fused].named_parameters()}}
            del out
        for _ in range(args.steps):
            for fused in (False, True):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                step(convs[fused])
                b.record()
                torch.cuda.synchronize()
                ms[fused].append(a.elapsed_time(b))
        stat = {f: (statistics.median(v), min(v), max(v)) for f, v in ms.items()}
        for fused in (False, True):
            med, lo, hi = stat[fused]
            say(f"  {name:18s} p_fused={str(fused):5s} {med:9.3f} ({lo:.3f} .. {hi:.3f}; spread {hi - lo:.3f}), "
                f"peak memory of a step above what was held before it {peak[fused]:.2f} GiB")
        gap, spreads = stat[False][0] - stat[True][0], sum(s[2] - s[1] for s in stat.values())
        say(f"  {name:18s} unfused / fused = {stat[False][0] / stat[True][0]:.2f}; the gap of the medians {gap:.3f} ms against the sum "
            f"of the two spreads {spreads:.3f} ms")
        errs = {n: rel_err(results[True][n], results[False][n]) for n in results[True]}
        say(f"  {name:18s} fused against unfused at this size, rel_err: " + ", ".join(f"{n} {v:.1e}" for n, v in errs.items()))
        lib.se3_profile_reset(), lib.se3_profile_enable(1)
        for _ in range(3):
            step(convs[True])
        torch.cuda.synchronize()
        lib.se3_profile_enable(0)
        table = profile_table(lib)
        say(f"  {name:18s} p_fused=True, kernels with a timing hook, ms per step (launches per step): " +
            ", ".join(f"{tag} {v[0] / 3:.3f} ({v[1] // 3})" for tag, v in sorted(table.items(), key=lambda kv: -kv[1][0])))
        del convs, results


ratios()
say()
times()
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
