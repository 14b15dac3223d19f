#!/usr/bin/env python3
"""What profiles/att_layers.txt records for the entry points of include/se3conv_basis_att.h and the layers on them.  Needs a GPU;
no CPU fallback; nothing here is asserted or thresholded.

  1. Error ratios: observed error / bound per tensor, over the cases of tests/basis_att_reference.py (the per-element float64
     restatement; the bound is 8 x its float32 emulation) -- the figures tests/test_gpu_basis_att.py asserts to be <= 1.
  2. Time of one step, forward + backward (eager autograd, device events around `--steps` steps after a warm-up), at
     N = 65 536 points in 8 batch elements, 32 nearest neighbours per point, C_in = C_out = V = 64, K = 32, 4 heads:
       (a) MultiHeadAttLayer and LoRAttConvLayer ('single' kernel points);
       (b) the attention stage alone, `ops.BasisAttention` on a T [N, 2V, K] of that shape;
       (c) the same stage written in the reference's torch ops (the transposes, `+ pe_`, two einsums, softmax) on the same T.
  3. The rate of (b) -- the bytes its kernels move by design (forward: T once; backward: T once, dT once, the query half of dT
     once more for dpe) over its time -- against the rate of a device-to-device copy of T measured in the same process.

    python tools/time_att_layers.py [--out profiles/att_layers.txt] [--points 65536] [--steps 10]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import basis_att_reference as R  # noqa: E402
import se3conv3d_amd as amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "att_layers.txt"))
ap.add_argument("--points", type=int, default=65536)
ap.add_argument("--neighbours", type=int, default=32)
ap.add_argument("--channels", type=int, default=64)
ap.add_argument("--basis", type=int, default=32)
ap.add_argument("--heads", type=int, default=4)
ap.add_argument("--steps", type=int, default=10)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tools/time_att_layers.py needs a GPU")
dev = torch.device("cuda:0")
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
n_ = lambda a: a.detach().cpu().numpy()


# ----------------------------------------------------------------------------------------------------------- error ratios
def ratios():
    b = R.bounds()
    say("observed error / bound (bound = 8 x the float32 emulation: " + ", ".join(f"{k} {v:.3g}" for k, v in b.items()) + ")")
    say(f"{'case':32s} " + " ".join(f"{name:>7s}" for name in R.ENTRIES))
    for i, (n, v, h, k, kind) in enumerate(R.CASES):
        case = R.case(300 + i, n, v, h, k, kind)
        T, key, pe = (t(case[x]).requires_grad_(True) for x in ("T", "key", "pe"))
        out = amd.ops.BasisAttention.apply(T, key, pe, h)
        att = out.grad_fn.saved_tensors[3]
        out.backward(t(case["grad_out"]))
        got = {"att": att, "out": out, "dT": T.grad, "dkey": key.grad, "dpe": pe.grad}
        want, scale = R.both(case)
        say(f"{f'N={n} V={v} H={h} K={k} {kind}':32s} " +
            " ".join(f"{R.worst(n_(got[name]), want[name], scale[name]) / b[name]:7.3f}" for name in R.ENTRIES))


# ------------------------------------------------------------------------------------------------------------------ time
def timed(step):
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def torch_attention(T, key, pe, heads):
    """layers/MultiHeadAttLayer.py:136-147 of the reference, on torch ops."""
    n, v2, k = T.shape
    v = v2 // 2
    d = v // heads
    agg_v = T[:, :v, :].transpose(1, 2)
    agg_q = T[:, v:, :].transpose(1, 2) + pe
    att = torch.einsum("nkhi,nkhi->nkh", agg_q.reshape(n, k, heads, d), key.reshape(n, 1, heads, d))
    att = torch.nn.functional.softmax(att, 1)
    return torch.einsum("nkhi,nkhi->nhi", agg_v.reshape(n, k, heads, d), att.reshape(n, k, heads, 1)).reshape(n, v)


def times():
    torch.manual_seed(0)
    npts, nn, c, kb, heads = args.points, args.neighbours, args.channels, args.basis, args.heads
    pts = torch.rand(npts, 3, device=dev)
    ids = torch.arange(npts, device=dev, dtype=torch.int32) // (npts // 8)
    pc = amd.pc.Pointcloud(pts, ids)
    nbh = amd.pc.KnnNeighborhood(pc, pc, nn)
    e = nbh.neighbors_.shape[0]
    say(f"N = {npts} points in 8 batch elements, {nn} nearest neighbours each: E = {e}; C_in = C_out = V = {c}, K = {kb}, {heads} heads; "
        f"median (min .. max) of {args.steps} eager steps, forward + backward, ms")
    x = torch.randn(npts, c, device=dev, requires_grad=True)
    g = torch.randn(npts, c, device=dev)
    diff = pts[nbh.neighbors_[:, 1].long()] - pts[nbh.neighbors_[:, 0].long()]
    rho = 1.0 / (2.0 * float(diff.norm(dim=1).mean()))
    for name, factory in (("MultiHeadAttLayer", amd.MultiHeadAttLayerFactory), ("LoRAttConvLayer", amd.LoRAttConvLayerFactory)):
        conv = factory(3, kb, "single", heads).create_conv_layer(c, c).to(dev)
        with torch.no_grad():
            conv.norm_neigh_dist_.fill_(rho), conv.norm_num_neighs_.fill_(npts / e)

        def step(conv=conv):
            for p in (x, *conv.parameters()):
                p.grad = None
            conv(pc, pc, x, nbh).backward(g)
        med, lo, hi = timed(step)
        say(f"  (a) {name:18s} {med:9.3f} ({lo:.3f} .. {hi:.3f})")
    del conv
    T = torch.randn(npts, 2 * c, kb, device=dev, requires_grad=True)
    wide = torch.randn(npts, 3 * c, device=dev)
    key = wide[:, 2 * c:].requires_grad_(True)
    pe = (torch.rand(1, kb, c, device=dev) - 0.5).requires_grad_(True)

    def stage(fn):
        def step():
            T.grad = key.grad = pe.grad = None
            fn(T, key, pe, heads).backward(g)
        return step

    hip = timed(stage(amd.ops.BasisAttention.apply))
    say(f"  (b) the attention stage, ops.BasisAttention      {hip[0]:9.3f} ({hip[1]:.3f} .. {hip[2]:.3f})")
    torch.cuda.reset_peak_memory_stats()
    ref = timed(stage(torch_attention))
    say(f"  (c) the same stage, the reference's torch ops    {ref[0]:9.3f} ({ref[1]:.3f} .. {ref[2]:.3f}), peak memory "
        f"{torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    say(f"  (c) / (b) = {ref[0] / hip[0]:.2f}; the spreads: (b) {hip[2] - hip[1]:.3f} ms, (c) {ref[2] - ref[1]:.3f} ms")
    with torch.no_grad():
        dst = torch.empty_like(T)
        copy = timed(lambda: dst.copy_(T))
    t_bytes = T.numel() * 4
    copy_rate = 2 * t_bytes / (copy[0] * 1e-3) / 1e12
    moved = 3.5 * t_bytes
    rate = moved / (hip[0] * 1e-3) / 1e12
    say(f"  T is {t_bytes / 2 ** 30:.2f} GiB; a device copy of it takes {copy[0]:.3f} ms = {copy_rate:.2f} TB/s read + write; (b) moves "
        f"3.5 x T = {moved / 2 ** 30:.2f} GiB by design (T, T, dT, the query half of dT) = {rate:.2f} TB/s, {100 * rate / copy_rate:.0f} % of the copy rate "
        f"(the step also holds autograd's host time and the small att, out, dkey, dpe)")


ratios()
say()
times()
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
