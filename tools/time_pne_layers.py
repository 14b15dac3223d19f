#!/usr/bin/env python3
"""What profiles/pne_layers.txt records for the entry points of include/se3conv_pne.h and the layers on them.  Needs a GPU; no
CPU fallback; nothing here is asserted or thresholded.

  1. Error ratios: observed error / bound per tensor and kind, over the cases of tests/pne_reference.py (the per-element
     float64 restatement; the bound is 8 x its float32 emulation) -- the figures tests/test_gpu_pne.py asserts to be <= 1.
  2. Time of one layer step, forward + backward (eager autograd, device events around `--steps` steps after a warm-up), at
     N = 65 536 points in 8 batch elements, 32 nearest neighbours per point (E = 2 097 152), C_in = C_out = 64, K = 32:
     PNEConvLayer 'kp_gauss' with 'max' and with 'add', and 'mlp_gelu' + 'add' (the fused operator) for scale.
  3. The same two steps composed from torch ops in the reference's formulation on the same GPU -- KPPNE's `[E, J, 3]`
     differences, FeatBasisProj as an index_add of `[E, C_in, K]` outer products, TransformNeighConv's `[E, C_in, C_out]` kernel
     per edge and an amax scatter -- where they fit in memory; "out of memory" where they do not.

    python tools/time_pne_layers.py [--out profiles/pne_layers.txt] [--points 65536] [--steps 10]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pne_reference as R  # noqa: E402
import se3conv3d_amd as amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pne_layers.txt"))
ap.add_argument("--points", type=int, default=65536)
ap.add_argument("--neighbours", type=int, default=32)
ap.add_argument("--channels", type=int, default=64)
ap.add_argument("--basis", type=int, default=32)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--skip-torch", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tools/time_pne_layers.py needs a GPU")
dev = torch.device("cuda:0")
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
n = lambda a: a.detach().cpu().numpy()


# ----------------------------------------------------------------------------------------------------------- error ratios
def ratios():
    b = R.bounds()
    say("observed error / bound (bound = 8 x the float32 emulation: " + ", ".join(f"{k} {v:.3g}" for k, v in b.items()) + ")")
    say(f"{'case':28s} {'phi':>7s} {'dA':>7s} {'dbeta':>7s}")
    for i, (kind, k, j) in enumerate(R.EMBED_CASES):
        case = R.embed_case(100 + i, kind, k, j)
        a, be = t(case["A"]).requires_grad_(True), t(case["beta"]).requires_grad_(True)
        phi = amd.ops.PneEmbed.apply(t(case["pts"]), t(case["samples"]), t(case["neighbors"]), a, be, float(case["rho"]), kind,
                                     None if case["kpts"] is None else t(case["kpts"]), case["sigma"])
        phi.backward(t(case["grad_phi"]))
        w_phi, s_phi, _ = R.embed_fwd(**R.embed_args(case))
        (w_dA, w_db), (s_dA, s_db) = R.embed_bwd(case["grad_phi"], **R.embed_args(case))
        got = (R.worst(n(phi), w_phi, s_phi) / b["phi"], R.worst(n(a.grad), w_dA, s_dA) / b["dA"], R.worst(n(be.grad), w_db, s_db) / b["dbeta"])
        say(f"{kind + f' K={k} J={j if R.is_kp(kind) else 3}':28s} " + " ".join(f"{v:7.3f}" for v in got))
    say(f"{'max aggregation':28s} {'out':>7s} {'dphi':>7s} {'dG':>7s}")
    for i, (k, c) in enumerate(R.MAX_CASES):
        case = R.max_case(200 + i, k, c)
        phi, g3 = t(case["phi"]).requires_grad_(True), t(case["G"]).requires_grad_(True)
        out, arg = amd.ops.NeighConvMax.apply(phi, g3, t(case["neighbors"]), t(case["ends"]), case["G"].shape[0])
        out.backward(t(case["grad_out"]))
        geo = (case["phi"], case["G"], case["neighbors"], case["ends"])
        r_out = R.hold_max_fwd(n(out), n(arg), *geo, b["out"]) / b["out"]
        (w_dphi, w_dG), (s_dphi, s_dG) = R.max_bwd(case["grad_out"], n(arg), *geo)
        say(f"{f'K={k} C_out={c}':28s} {r_out:7.3f} {R.worst(n(phi.grad), w_dphi, s_dphi) / b['dphi']:7.3f} "
            f"{R.worst(n(g3.grad), w_dG, s_dG) / b['dG']:7.3f}")


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


def layer_step(conv, pc, nbh, x, g):
    def step():
        for p in (x, *conv.parameters()):
            p.grad = None
        conv(pc, pc, x, nbh).backward(g)
    return step


def torch_step(conv, pc, nbh, x, g, agg):
    """The reference's formulation (custom_ops/PNE.py, FeatBasisProj, TransformNeighConv.py) on torch ops."""
    nb = nbh.neighbors_.long()
    smp, src = nb[:, 0], nb[:, 1]
    m = pc.pts_.shape[0]

    def step():
        for p in (x, *conv.parameters()):
            p.grad = None
        rel = (pc.pts_[src] - pc.pts_[smp]) * conv.norm_neigh_dist_
        d = torch.sqrt(((rel[:, None, :] - conv.kernel_pts_[None]) ** 2).sum(-1)) / conv.kp_sigma_
        phi = torch.exp(-(d ** 2) / 2.0) @ conv.proj_axes_ + conv.proj_biases_
        if agg == "add":
            tt = torch.zeros((m, x.shape[1], phi.shape[1]), device=dev).index_add_(0, smp, x[src][:, :, None] * phi[:, None, :])
            out = torch.einsum("nik,iko->no", tt, conv.conv_weights_)
        else:
            kernel = torch.einsum("nk,iko->nio", phi, conv.conv_weights_)
            per_edge = torch.einsum("nio,ni->no", kernel, x[src])
            out = torch.zeros((m, per_edge.shape[1]), device=dev).scatter_reduce(0, smp[:, None].expand_as(per_edge), per_edge, "amax",
                                                                                include_self=False)
        (out * conv.norm_num_neighs_).backward(g)
    return step


def times():
    torch.manual_seed(0)
    npts, k, c, kb = args.points, args.neighbours, args.channels, args.basis
    pts = torch.rand(npts, 3, device=dev)
    ids = torch.arange(npts, device=dev, dtype=torch.int32) // (npts // 8)
    pc = amd.pc.Pointcloud(pts, ids)
    nbh = amd.pc.KnnNeighborhood(pc, pc, k)
    e = nbh.neighbors_.shape[0]
    say(f"N = {npts} points in 8 batch elements, {k} nearest neighbours each: E = {e}; C_in = C_out = {c}, K = {kb}; "
        f"median (min .. max) of {args.steps} eager steps, forward + backward, ms")
    x = torch.randn(npts, c, device=dev, requires_grad=True)
    g = torch.randn(npts, c, device=dev)
    diff = pts[nbh.neighbors_[:, 1].long()] - pts[nbh.neighbors_[:, 0].long()]
    rho = 1.0 / (2.0 * float(diff.norm(dim=1).mean()))
    convs = {}
    for pne_type, agg in (("kp_gauss", "max"), ("kp_gauss", "add"), ("mlp_gelu", "max"), ("mlp_gelu", "add")):
        conv = amd.PNEConvLayerFactory(3, kb, pne_type, agg).create_conv_layer(c, c).to(dev)
        with torch.no_grad():
            conv.norm_neigh_dist_.fill_(rho), conv.norm_num_neighs_.fill_(npts / e)
        convs[pne_type, agg] = conv
        med, lo, hi = timed(layer_step(conv, pc, nbh, x, g))
        note = " (the fused operator, for scale)" if conv.fused_ else ""
        say(f"  PNEConvLayer {pne_type:9s} {agg:4s}  {med:9.3f} ({lo:.3f} .. {hi:.3f}){note}")
    if args.skip_torch:
        return
    for agg in ("max", "add"):
        conv = convs["kp_gauss", agg]
        try:
            torch.cuda.reset_peak_memory_stats()
            med, lo, hi = timed(torch_step(conv, pc, nbh, x, g, agg))
            say(f"  torch ops, reference's form, kp_gauss {agg:4s}  {med:9.3f} ({lo:.3f} .. {hi:.3f}), peak memory "
                f"{torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
        except torch.cuda.OutOfMemoryError:
            say(f"  torch ops, reference's form, kp_gauss {agg:4s}  out of memory")
        torch.cuda.empty_cache()


ratios()
say()
times()
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
