#!/usr/bin/env python3
"""Wall time of the row-wise passes on padded clouds (include/se3conv_padded_rows.h), two ways:

  (a) every padded entry point at FULL count (the word equals the row count) against its counterpart of include/se3conv.h on
      the same buffers, at 131 072 x 64 and at 6 000 x 64 feature rows (2 frames): what the word costs where nothing is absent;
  (b) the step of the test network (tests/test_gpu_network.py's MiniUNet with one ResNetFormer behind the first level,
      3 000 points, forward + masked loss + backward): ONE captured graph on padded levels (`p_padded=True,
      p_padded_rows=True`), replayed, against the eager step of the same modules on trimmed levels -- the path that existed
      before the padded glue, and the baseline.

Needs a GPU; there is no CPU fallback.  The variants of a group run in one process, in turn, every sample timed by the host
clock around `--calls` calls (the step: one) and a device synchronise, after a warm-up, until every variant has run for
`--seconds` and `--min-reps` samples.  Reported: the median and min .. max per variant; the baseline of each group is run as
two variants, whose two medians show the run-to-run spread a difference has to exceed.

    python tools/time_padded_step.py [--out profiles/padded_rows.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import se3conv3d_amd as amd  # noqa: E402
from se3conv3d_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--min-reps", type=int, default=20)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "padded_rows.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tools/time_padded_step.py needs a GPU")
dev = torch.device("cuda:0")
ops, pc = amd.ops, amd.pc
lib = _lib.load()
lines = []
F32, I32 = torch.float32, torch.int32


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def run(variants, calls):
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    while any(sum(t) * calls < args.seconds * 1e3 or len(t) < args.min_reps for t in times.values()):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / calls)
    return times


def p(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def report(group, times, base):
    """`base`: the names of the two runs of the baseline."""
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = abs(med[base[0]] - med[base[1]])
    ref = min(med[base[0]], med[base[1]])
    for name, t in times.items():
        note = ""
        if name not in base:
            d = med[name] - max(med[base[0]], med[base[1]])
            note = f"  SLOWER than its counterpart by {d * 1e3:.1f} us, more than the spread" if d > spread else "  within the spread or faster"
        say(f"  {group:<22} {name:<28} median {med[name] * 1e3:9.1f} us  ({min(t) * 1e3:.1f} .. {max(t) * 1e3:.1f}), {len(t)} samples{note}")
    say(f"  {group:<22} run-to-run spread of the baseline {spread * 1e3:.1f} us ({100 * spread / ref:.1f} %)")


# ------------------------------------------------------------------------------------------------ (a) entry points
def entry_points(rows, c, frames=2):
    n = rows // frames
    st = ops._stream(dev)
    g = torch.Generator(device="cpu").manual_seed(rows)
    x, y, dy = (torch.randn(rows, c, generator=g).to(dev) for _ in range(3))
    w, b = torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev)
    rm, rv, nbt = torch.zeros(c, device=dev), torch.ones(c, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    out, mean, invstd, dg, db = torch.empty_like(x), torch.empty(c, device=dev), torch.empty(c, device=dev), torch.empty(c, device=dev), torch.empty(c, device=dev)
    need = lib.se3_glue_workspace_bytes(c)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    word = torch.tensor([n], dtype=I32, device=dev)
    nb = 8
    rb = torch.arange(rows, device=dev, dtype=I32) * nb // rows
    gate = torch.rand(nb, device=dev)
    pooled, arg = torch.empty(n, c, device=dev), torch.empty(n, c, dtype=I32, device=dev)
    # a level of the rows as points: cells of ~4 rows
    pts = torch.rand(rows, 3, device=dev)
    bid = torch.zeros(rows, dtype=I32, device=dev)
    lv = ops.grid_levels_bounded(pts, bid, [(4.0 / rows) ** (1.0 / 3.0)], "input", 1, n_valid=torch.tensor([rows], dtype=I32, device=dev),
                                 rnd=[True]).levels[0]
    cells = int(lv["picked"].ge(0).sum())
    vals = torch.randn(rows, c, device=dev)
    picked = lv["picked"][:cells].contiguous()
    chk = lambda rc: None if rc == 0 else sys.exit(f"library call failed: {rc}")
    groups = {
        "bn_fwd": (lambda: chk(lib.se3_bn_fwd(p(x), p(w), p(b), rows, c, 1e-5, 0.2, p(rm), p(rv), p(nbt), p(out), p(mean), p(invstd), p(ws), need, st)),
                   lambda: chk(lib.se3_bn_fwd_padded(p(x), p(w), p(b), n, frames, p(word), c, 1e-5, 0.2, p(rm), p(rv), p(nbt), p(out), p(mean), p(invstd), p(ws), need, st))),
        "bn_bwd": (lambda: chk(lib.se3_bn_bwd(p(dy), p(x), p(mean), p(invstd), p(w), rows, c, p(out), p(dg), p(db), p(ws), need, st)),
                   lambda: chk(lib.se3_bn_bwd_padded(p(dy), p(x), p(mean), p(invstd), p(w), n, frames, p(word), c, p(out), p(dg), p(db), p(ws), need, st))),
        "skip_fwd": (lambda: chk(lib.se3_skip_fwd(p(x), p(y), p(w), p(gate), 0.9, p(rb), rows, c, p(out), st)),
                     lambda: chk(lib.se3_skip_fwd_padded(p(x), p(y), p(w), p(gate), 0.9, p(rb), n, frames, p(word), c, p(out), st))),
        "skip_bwd": (lambda: chk(lib.se3_skip_bwd(p(dy), p(x), p(w), p(gate), 0.9, p(rb), rows, c, p(out), p(dg), p(ws), need, st)),
                     lambda: chk(lib.se3_skip_bwd_padded(p(dy), p(x), p(w), p(gate), 0.9, p(rb), n, frames, p(word), c, p(out), p(dg), p(ws), need, st))),
        "frame_pool max": (lambda: chk(lib.se3_frame_pool(p(x), n, frames, c, 1, p(pooled), p(arg), st)),
                           lambda: chk(lib.se3_frame_pool_padded(p(x), n, frames, p(word), c, 1, p(pooled), p(arg), st))),
        "frame_unpool max": (lambda: chk(lib.se3_frame_unpool(p(pooled), p(arg), n, frames, c, 1, p(out), st)),
                             lambda: chk(lib.se3_frame_unpool_padded(p(pooled), p(arg), n, frames, p(word), c, 1, p(out), st))),
        "segment_unpool avg": (lambda: chk(lib.se3_segment_unpool(p(vals), p(lv["cell_ids"]), p(lv["cell_ends"]), None, rows, c, 0, p(out), st)),
                               lambda: chk(lib.se3_segment_unpool_padded(p(vals), p(lv["cell_ids"]), p(lv["cell_ends"]), None, rows, c, 0, p(out), st))),
        "rows_gather": (lambda: chk(lib.se3_rows_gather(p(x), p(picked), cells, c * 4, p(out), st)),
                        lambda: chk(lib.se3_rows_gather_padded(p(x), p(picked), cells, c * 4, p(out), st))),
        # the way back: zeros + scatter against the one gather
        "rows_unpick": (lambda: ops.rows_scatter(vals[:cells], picked, rows),
                        lambda: chk(lib.se3_rows_unpick_padded(p(vals), p(lv["cell_ids"]), p(lv["picked"]), rows, c * 4, p(out), st))),
    }
    say(f"(a) entry points at full count, {rows} x {c} feature rows ({frames} frames), {args.calls} calls per sample")
    for name, (plain, padded) in groups.items():
        times = run({"counterpart": plain, "counterpart (again)": plain, "padded, word = n_rows": padded}, args.calls)
        report(name, times, ("counterpart", "counterpart (again)"))
    say()


# ------------------------------------------------------------------------------------------------------- (b) step
def network_step():
    from bounded_levels_cases import cloud
    from test_gpu_network import MiniUNet

    rows, nb, f, cap, n_cls = 3000, 3, 2, 200000, 5
    cfg = {"pca": True, "n_frames": f, "fixed_axis": False, "neigh_method": "knn", "neigh_kwargs": {"neigh_k": 16}}
    cells, radii = [0.12, 0.25], [0.12, 0.25, 0.5]
    torch.manual_seed(7)
    unet = MiniUNet(amd, 3, [32, 64, 96], n_cls).to(dev).train()
    block = amd.ResNetFormer(32, 32, unet.factory, amd.BatchNormPC, 0.1).to(dev).train()
    for m in unet.modules():
        if isinstance(m, amd.PNEConvLayerRotEquiv):
            m.norm_neigh_dist_.fill_(4.0), m.norm_num_neighs_.fill_(0.05)
    block.spatial_conv_.norm_neigh_dist_.fill_(4.0), block.spatial_conv_.norm_num_neighs_.fill_(0.05)
    params = list(unet.parameters()) + list(block.parameters())
    pts, bid = cloud((1200, 800, 1000), 11)
    pts, bid = pts.to(dev), bid.to(dev)
    x = torch.randn(rows * f, 3, device=dev)
    lab = torch.randint(0, n_cls, (rows,), device=dev)
    word = torch.tensor([rows], dtype=I32, device=dev)

    def forward(levels, bq):
        h, feats = x, []
        for lv in range(3):
            h = torch.nn.functional.gelu(unet.enc_same[lv](p_pc_in=levels[lv], p_pc_out=levels[lv], p_in_features=h, p_neighborhood=bq(lv, lv)))
            if lv == 0:
                h = block(levels[0], h, bq(0, 0))
            feats.append(h)
            if lv < 2:
                h = torch.nn.functional.gelu(unet.enc_down[lv](p_pc_in=levels[lv], p_pc_out=levels[lv + 1], p_in_features=h,
                                                               p_neighborhood=bq(lv, lv + 1)))
        for lv in (1, 0):
            up = unet.dec_up[lv](p_pc_in=levels[lv + 1], p_pc_out=levels[lv], p_in_features=h, p_neighborhood=bq(lv + 1, lv))
            sk = ops.Linear.apply(feats[lv], unet.skip[lv].weight, unet.skip[lv].bias, getattr(levels[lv], "n_valid_", None), f)
            h = torch.nn.functional.gelu(up + sk)
        return unet.head(levels[0].feature_pooling(h, "avg"))

    def step(padded):
        for q in params:
            q.grad = None
        amd.PNEConvLayerRotEquiv.empty_rot_tenors_cache()
        if padded:
            pc0 = pc.PointcloudRotEquiv(pts, bid, cfg, p_n_valid=word, num_batches=nb, p_padded_rows=True)
            hier = pc.PointHierarchyRotEquiv(pc0, 2, "grid_avg", p_capacities="input", p_padded=True, p_padded_rows=True, grid_radii=cells)
        else:
            pc0 = pc.PointcloudRotEquiv(pts, bid, cfg, num_batches=nb)
            hier = pc.PointHierarchyRotEquiv(pc0, 2, "grid_avg", grid_radii=cells)
        nbhs = {}

        def bq(a, b):
            if (a, b) not in nbhs:
                nbhs[(a, b)] = pc.BQNeighborhood(hier.pcs_[a], hier.pcs_[b], radii[max(a, b)], p_capacity=cap if padded else None)
            return nbhs[(a, b)]

        logits = forward(hier.pcs_, bq)
        if padded:
            mask = pc.present_mask(pc0)
            loss = torch.nn.functional.cross_entropy(logits, lab, ignore_index=-100, reduction="sum") / mask.sum().clamp(min=1)
        else:
            loss = torch.nn.functional.cross_entropy(logits, lab)
        loss.backward()
        return loss.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        held = step(True)
    say(f"(b) the test network's step (MiniUNet [32, 64, 96] + ResNetFormer(32, 32, BatchNormPC, 0.1), {rows} points in {nb} elements, "
        f"{f} frames): geometry, forward, masked loss, backward")
    times = run({"eager, trimmed levels": lambda: step(False), "eager, trimmed (again)": lambda: step(False),
                 "eager, padded levels": lambda: step(True), "ONE graph replay, padded": graph.replay}, 1)
    report("step", times, ("eager, trimmed levels", "eager, trimmed (again)"))
    say(f"  (last replayed loss {float(held):.4f}; the eager trimmed step's {float(step(False)):.4f}: other frames and gate draws)")
    say()


say(f"tools/time_padded_step.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
say("host time per call, each sample ended by a device synchronise; the variants of a group alternate in one process")
say()
for rows_ in (131072, 6000):
    entry_points(rows_, 64)
network_step()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
