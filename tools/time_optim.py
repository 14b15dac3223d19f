#!/usr/bin/env python3
"""Time of the optimizer step (`se3conv3d_amd.AdamW.step()` = se3_optim_adamw_step, include/se3conv_optim.h) beside torch's own
path for the same three lines of the reference's loop, on the parameter shapes of the ScanNet network, and the CPU figures of
tests/test_optim_reference.py.

Parameter set: the 32 convolution calls of FPNSegUNetMLPGeluRotEqScanNet (widths recorded in
tests/golden/network_scannet_calls.npz), each call of equal widths as a `blocks.ResNetFormer` (convolution, norms, point-wise
MLP, skip), each call between widths as a convolution and a `BatchNormPC`: the tensor count and sizes of the network without
its head.

Paths, each ONE captured graph, replayed (`--iters` replays per window between two HIP events, `--windows` windows, the paths
taking turns; medians), gradients refilled by a device copy inside the graph so that every replay clips and updates:

    this call     opt.step()                         clip at 100, AdamW, table learning rate, gradients zeroed
    torch         clip_grad_norm_(foreach=True) + AdamW(fused=True, capturable=True).step() + zero_grad(set_to_none=False)
    refill alone  the copy both graphs share, to subtract

The kernel nodes of each graph are counted.  Nothing is asserted or thresholded.  Needs a GPU for the timing part; `--cpu-only`
writes the CPU figures alone.

    python tools/time_optim.py [--out profiles/optim.txt]"""
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
import se3conv3d_amd as amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50, help="replays per timed window")
ap.add_argument("--windows", type=int, default=9)
ap.add_argument("--cpu-only", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim.txt"))
args = ap.parse_args()
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


# ------------------------------------------------------------------------------------------------------- the CPU figures
import test_optim_reference as T  # noqa: E402

say("tools/time_optim.py")
say()
say("CPU: the fp32 numpy restatement of include/se3conv_optim.h against the reference's loop run with torch itself")
say("(tests/test_optim_reference.py (b): 12 iterations, tensors of 1, 3, 5, 1023, 1025 elements, gradients 1e-25 .. 1e3).")
say("Y_s: largest element error of torch's own fp32 run against the same loop in float64; ratio: the restatement's / Y_s.")
say("Columns: parameters, exp_avg, exp_avg_sq.  The bound the test asserts is ratio <= 2 at every iteration.")
for config in ("scannet", "loud"):
    for accum in (1, 3):
        Y, E, reads = T.measure(config, accum)
        say(f"  config {config}, accum {accum}: largest ratio {np.max(E / Y, axis=0).round(3).tolist()}")
        for s in range(T.ITERS):
            say(f"    iteration {s:2d}  Y_s {Y[s, 0]:.3e} {Y[s, 1]:.3e} {Y[s, 2]:.3e}   ratio {E[s, 0] / Y[s, 0]:.3f} "
                f"{E[s, 1] / Y[s, 1]:.3f} {E[s, 2] / Y[s, 2]:.3f}   clip_coef {float(reads[s]['clip_coef']):.4g} stepped {reads[s]['stepped']}")

if args.cpu_only or not torch.cuda.is_available():
    say()
    say("(no GPU: the device part was not run)")
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(0)

# ---------------------------------------------------------------------------------------------------------- the device part
dev = torch.device("cuda:0")


def scannet_parameters():
    with np.load(os.path.join(ROOT, "tests", "golden", "network_scannet_calls.npz")) as z:
        widths = [tuple(int(v) for v in z[f"c{i:02d}/meta"])[4:] for i in range(int(z["n_calls"]))]
    fact = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu")
    modules = []
    for c_in, c_out in widths:
        if c_in == c_out:
            modules.append(amd.ResNetFormer(c_in, c_out, fact, amd.BatchNormPC, 0.0))
        else:
            modules += [fact.create_conv_layer(c_in, c_out), amd.BatchNormPC(c_out)]
    return torch.nn.ModuleList(modules).to(dev)


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


def replay_ms(graph):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.iters):
        graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.iters


torch.manual_seed(0)
ours_model, theirs_model = scannet_parameters(), scannet_parameters()
theirs_model.load_state_dict(ours_model.state_dict())
ours_p = [p for p in ours_model.parameters() if p.requires_grad]
theirs_p = [p for p in theirs_model.parameters() if p.requires_grad]
numel = sum(p.numel() for p in ours_p)
table = amd.one_cycle_table(0.005, 1000, 10.0, 1000.0, 0.05)
opt = amd.AdamW(ours_p, lr_table=table, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, max_grad_norm=100.0)
source = torch.randn(opt.tables.state_len, device=dev) * 0.05       # one gradient set: norm ~ 0.05 * sqrt(numel) > 100
# torch's path gets one flat gradient buffer too, so that both refills are ONE copy of the same bytes
theirs_flat = torch.zeros_like(opt.tables.flat_grad)
for p, off in zip(theirs_p, opt.tables.offsets):
    p.grad = theirs_flat[off:off + p.numel()].view(p.shape)
theirs = torch.optim.AdamW(theirs_p, lr=torch.tensor(0.0005, device=dev), betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4,
                           fused=True, capturable=True)


def ours_step():
    opt.tables.flat_grad.copy_(source)
    opt.step()


def theirs_step():
    theirs_flat.copy_(source)
    torch.nn.utils.clip_grad_norm_(theirs_p, 100.0, foreach=True)
    theirs.step()
    theirs.zero_grad(set_to_none=False)


def refill():
    theirs_flat.copy_(source)


graphs = {"this call": captured(ours_step), "torch": captured(theirs_step), "refill alone": captured(refill)}
kinds = {k: node_types(g) for k, g in graphs.items()}
times = {k: [] for k in graphs}
for _ in range(args.windows):
    for k, g in graphs.items():
        times[k].append(replay_ms(g))
med = {k: statistics.median(v) for k, v in times.items()}
say()
say(f"Device: {torch.cuda.get_device_name(0)}; {len(ours_p)} tensors, {numel} parameters ({numel * 4 / 1e6:.1f} MB), "
    f"{opt.tables.n_chunks} chunks; {args.windows} windows of {args.iters} graph replays, medians; ms per replay")
for k, v in med.items():
    say(f"  {k:14s} {v:9.4f}   (min {min(times[k]):.4f}, max {max(times[k]):.4f})   graph: {kinds[k].count(0)} kernel, "
        f"{kinds[k].count(1)} memcpy, {kinds[k].count(2)} memset nodes")
a, b = med["this call"] - med["refill alone"], med["torch"] - med["refill alone"]
say(f"  without the refill: this call {a:.4f}, torch {b:.4f}, this call / torch {a / b:.3f}")
say(f"  launches per step: this call {kinds['this call'].count(0) - kinds['refill alone'].count(0)}, "
    f"torch {kinds['torch'].count(0) - kinds['refill alone'].count(0)} (kernel nodes beyond the refill's)")
moved = numel * 4
say(f"  bytes per step at least: read p, g, m, v + g again for the norm, write p, m, v, g = 9 x {moved / 1e6:.1f} MB; "
    f"{9 * moved / (a * 1e-3) / 1e12:.2f} TB/s at this call's time")
say(f"  after the replays: t {int(opt.t)}, it {int(opt.it)}, lr {float(opt.lr):.6g}, grad_norm {float(opt.grad_norm):.4f}, "
    f"clip_coef {float(opt.clip_coef):.4f}; torch's step {int(theirs.state[theirs_p[0]]['step'])}")

with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
