"""GPU: the loss and metrics head (include/se3conv_seg_head.h), `ops.seg_loss` / `ops.SegLoss` and `metrics.SemSegMetrics`.

1. `se3_seg_loss_fwd` / `se3_seg_loss_bwd` against the numpy contract (tests/seg_head_reference.py) within the bounds the
   header's arithmetic allows: counts and tallies exact, lse to 1e-13, the loss to one fp32 unit, the gradient to one fp32 unit
   plus the absolute error of the fp64 probabilities; exact zeros wherever a row does not count.
2. What the fixed order buys: two calls give the same bits, a padded call the bits of the trimmed one; tallies accumulate.
3. The device path of `metrics.SemSegMetrics` against the reference's fixture, the torch recipe of INTEGRATION.md, error codes.
4. Loss, counters and backward as one captured graph: no memset, no memcpy, at most four kernel nodes, replayed on two row
   counts.
5. The small padded U-Net step of tests/test_gpu_padded_rows.py with `ops.seg_loss` in place of the torch recipe."""
import functools
import os

import numpy as np
import pytest
import torch

import seg_head_reference as R
from conftest import GOLDEN
from padded_cases import DEV, word
from test_gpu_graph_nodes import HIP_GRAPH_NODE_TYPE_MEMSET, capture, node_types

pytestmark = pytest.mark.gpu
K = R.CHUNK
HIP_GRAPH_NODE_TYPE_KERNEL, HIP_GRAPH_NODE_TYPE_MEMCPY = 0, 1
ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 3 * K + 7]
CLASSES = [1, 2, 21, 40, R.TILE_CLASSES, R.TILE_CLASSES + 1]          # ..., the widest LDS tile, the first width beyond it
G = 0.7                                                                 # the gradient arriving at the loss
t = lambda a: torch.from_numpy(np.array(a, copy=True)).to(DEV)                # (a copy: the shared cases are read-only)
bits32 = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.int32)


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd as amd
    return amd


@pytest.fixture(scope="module")
def ops(amd):
    return amd.ops


def device(ops, x, y, eps=0.0, counted=None, valid=None, tallies=None, g=G, bits=64, want_lse=True, backward=True):
    """Both C entry points on prefilled outputs and a 0xFF-filled workspace of exactly the query's size:
    `dict(loss, count, lse, tallies, grad)` as numpy."""
    from se3conv3d_amd import _lib

    lib = _lib.load()
    n, c = x.shape
    xd, yd = t(x), t(np.asarray(y).astype(np.int64 if bits == 64 else np.int32))
    cd = None if counted is None else t(np.asarray(counted, dtype=np.uint8))
    w = None if valid is None else word(valid)
    loss = torch.full((1,), 9.0, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    lse = torch.full((n,), 9.0, dtype=torch.float64, device=DEV) if want_lse else None
    td = None if tallies is None else t(tallies)
    need = lib.se3_seg_head_workspace_bytes(n, c)
    assert need > 0
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    p = lambda v: None if v is None else v.data_ptr()
    s = ops._stream(torch.device(DEV))
    assert lib.se3_seg_loss_fwd(p(xd), p(yd), bits, p(cd), n, p(w), c, float(eps), p(loss), p(count), p(lse), p(td), p(ws), need, s) == 0
    out = {"loss": loss, "count": count, "lse": lse, "tallies": td, "grad": None}
    if backward:
        gd, grad = torch.tensor([g], dtype=torch.float32, device=DEV), torch.full((n, c), 9.0, device=DEV)
        assert lib.se3_seg_loss_bwd(p(xd), p(yd), bits, p(cd), p(lse), p(count), p(gd), n, p(w), c, float(eps), p(grad), s) == 0
        out["grad"] = grad
    torch.cuda.synchronize()
    out = {k: None if v is None else v.cpu().numpy() for k, v in out.items()}
    out["loss"], out["count"] = out["loss"][0], int(out["count"][0])
    return out


@functools.lru_cache(maxsize=None)
def contract(rows, classes, eps, spread=4.0):
    """The case of (rows, classes) and its reference, computed once and shared (nothing here is written to afterwards)."""
    masked = (classes - 1,) if classes > 2 else ()
    x, y = R.case(rows, classes, 1000 * rows + classes, spread=spread, masked=masked)
    counted = R.counted_of(classes, masked) if masked else None
    tallies = np.zeros((3, classes), dtype=np.int64)
    loss, count, lse, _ = R.forward(x, y, eps, counted, None, tallies)
    grad = R.backward(x, y, lse, count, G, eps, counted)
    for a in (x, y, lse, grad, tallies):
        a.setflags(write=False)
    return x, y, counted, {"loss": loss, "count": count, "lse": lse, "tallies": tallies, "grad": grad}


def assert_meets(got, want, what, g=G):
    """The bounds of the header's arithmetic (module docstring, 1.)."""
    assert got["count"] == want["count"], what
    if want["tallies"] is not None:
        assert np.array_equal(got["tallies"], want["tallies"]), what
    off = want["lse"] == 0.0
    assert not got["lse"][off].view(np.int64).any(), what                                  # 0.0 exactly where no row counts
    e_lse = np.abs(got["lse"] - want["lse"]) / np.maximum(1.0, np.abs(want["lse"]))
    e_loss = abs(float(got["loss"]) - float(want["loss"])) / R.ulp32(want["loss"])
    bound = R.ulp32(want["grad"]) + 1e-13 * abs(g) / max(want["count"], 1)
    e_grad = np.abs(got["grad"].astype(np.float64) - want["grad"].astype(np.float64)) / bound
    print(f"{what}: count {got['count']}, lse {e_lse.max(initial=0.0):.2e} (bound 1e-13), loss {e_loss:.2f} ulp32 (bound 1), "
          f"gradient {e_grad.max(initial=0.0):.2f} of its bound")
    assert e_lse.max(initial=0.0) <= 1e-13 and e_loss <= 1.0 and e_grad.max(initial=0.0) <= 1.0, what
    assert not bits32(got["grad"])[off].any(), what                                         # 0.0f exactly
    if want["count"] == 0:
        assert np.float32(got["loss"]).view(np.int32) == 0, what


# ------------------------------------------------------------------------------------------------ 1. the contract
@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("classes", CLASSES)
@pytest.mark.parametrize("rows", ROWS)
def test_kernels_meet_the_contract(ops, rows, classes, eps, bits):
    x, y, counted, want = contract(rows, classes, eps)
    if rows >= 63 and classes > 2:
        assert (y == R.IGNORE).any() and (y == classes).any() and (y == classes - 1).any() and want["count"] < rows
    got = device(ops, x, y, eps, counted, None, np.zeros((3, classes), np.int64), bits=bits)
    assert_meets(got, want, (rows, classes, eps, bits))


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("classes", [21, R.TILE_CLASSES + 1])
def test_logits_spread_over_1e4_and_first_of_tied_maxima(ops, classes, eps):
    x, y, counted, want = contract(K + 9, classes, eps, spread=4000.0)
    assert np.abs(x).max() > 1e4 and want["count"] > 100
    got = device(ops, x, y, eps, counted, None, np.zeros((3, classes), np.int64))
    assert_meets(got, want, ("1e4", classes, eps))
    # every row one tie of ALL classes: pred is class 0, whatever the label
    flat = np.full((70, classes), 2.5, dtype=np.float32)
    lab = (np.arange(70) % classes).astype(np.int64)
    got = device(ops, flat, lab, 0.0, None, None, np.zeros((3, classes), np.int64))
    assert got["tallies"][1, 0] == 70 and got["tallies"][1, 1:].sum() == 0 and got["tallies"][2].sum() == got["tallies"][2, 0] == (lab == 0).sum()


def test_no_row_counts_and_a_word_of_zero(ops):
    x, y, _, _ = contract(300, 21, 0.1)
    pre = np.arange(63, dtype=np.int64).reshape(3, 21)
    for what, labels, counted, valid in (("ignored", np.full(300, R.IGNORE), None, None), ("masked", np.full(300, 4), R.counted_of(21, (4,)), None),
                                         ("word 0", y, None, 0), ("negative word", y, None, -5)):
        got = device(ops, x, labels, 0.1, counted, valid, pre)
        assert got["count"] == 0 and np.float32(got["loss"]).view(np.int32) == 0, what
        assert not got["lse"].view(np.int64).any() and not bits32(got["grad"]).any() and np.array_equal(got["tallies"], pre), what


# ---------------------------------------------------------------------------------------- 2. repeated, padded, added
def test_two_calls_give_the_same_bits(ops):
    x, y, counted, _ = contract(3 * K + 7, 40, 0.1)
    first = device(ops, x, y, 0.1, counted, None, np.zeros((3, 40), np.int64))
    for _ in range(3):
        again = device(ops, x, y, 0.1, counted, None, np.zeros((3, 40), np.int64))
        assert np.float32(again["loss"]).view(np.int32) == np.float32(first["loss"]).view(np.int32) and again["count"] == first["count"]
        assert np.array_equal(again["lse"].view(np.int64), first["lse"].view(np.int64)) and np.array_equal(again["tallies"], first["tallies"])
        assert np.array_equal(bits32(again["grad"]), bits32(first["grad"]))


@pytest.mark.parametrize("classes", [21, R.TILE_CLASSES + 1])
@pytest.mark.parametrize("valid", [300, 177, 0])
def test_a_padded_buffer_gives_the_bits_of_the_trimmed_call(ops, valid, classes):
    x, y, counted, _ = contract(300, classes, 0.1)
    pre = np.arange(3 * classes, dtype=np.int64).reshape(3, classes)
    trimmed = device(ops, x[:valid], y[:valid], 0.1, counted, None, pre)
    xp, yp = x.copy(), y.copy()
    xp[valid:], yp[valid:] = np.nan, 3                                     # absent rows: NaN logits, labels that would count
    for bits in (64, 32):
        got = device(ops, xp, yp, 0.1, counted, valid, pre, bits=bits)
        assert np.float32(got["loss"]).view(np.int32) == np.float32(trimmed["loss"]).view(np.int32) and got["count"] == trimmed["count"]
        assert np.array_equal(got["tallies"], trimmed["tallies"])
        assert np.array_equal(got["lse"][:valid].view(np.int64), trimmed["lse"].view(np.int64)) and not got["lse"][valid:].view(np.int64).any()
        assert np.array_equal(bits32(got["grad"][:valid]), bits32(trimmed["grad"])) and not bits32(got["grad"][valid:]).any()
    # a word past the buffer is clamped
    x2, y2, counted2, want = contract(300, classes, 0.1)
    assert_meets(device(ops, x2, y2, 0.1, counted2, 309, np.zeros((3, classes), np.int64)), want, "clamped")


def test_two_calls_into_the_same_tallies_give_the_sum_and_lse_may_be_null(ops):
    x, y, counted, want = contract(257, 21, 0.0)
    x2, y2, _, want2 = contract(65, 21, 0.0)
    once = device(ops, x, y, 0.0, counted, None, np.zeros((3, 21), np.int64), want_lse=False, backward=False)
    assert once["lse"] is None and np.array_equal(once["tallies"], want["tallies"]) and once["count"] == want["count"]
    assert abs(float(once["loss"]) - float(want["loss"])) <= R.ulp32(want["loss"])
    twice = device(ops, x2, y2, 0.0, counted, None, once["tallies"], backward=False)
    assert np.array_equal(twice["tallies"], want["tallies"] + want2["tallies"])
    none = device(ops, x2, y2, 0.0, counted, None, None, backward=False)   # without tallies: the loss alone
    assert none["tallies"] is None and np.float32(none["loss"]).view(np.int32) == np.float32(twice["loss"]).view(np.int32)


# ------------------------------------------------------------------- 3. the classes, the fixture, the recipe, errors
def test_autograd_class_is_the_entry_points(ops):
    x, y, counted, _ = contract(300, 21, 0.1)
    raw = device(ops, x, y, 0.1, counted, 177, np.zeros((3, 21), np.int64), g=1.0)
    for labels in (t(y), t(y.astype(np.int32))):
        xd, tallies = t(x).requires_grad_(True), torch.zeros(3, 21, dtype=torch.int64, device=DEV)
        loss = ops.seg_loss(xd, labels, 0.1, counted=[20], n_valid=word(177), tallies=tallies)
        assert loss.shape == () and loss.dtype == torch.float32
        loss.backward()
        assert np.float32(loss.item()).view(np.int32) == np.float32(raw["loss"]).view(np.int32)
        assert np.array_equal(bits32(xd.grad), bits32(raw["grad"])) and np.array_equal(tallies.cpu().numpy(), raw["tallies"])
    with torch.no_grad():
        same = ops.seg_loss(t(x), t(y), 0.1, counted=t(counted), n_valid=word(177))
    assert np.float32(same.item()).view(np.int32) == np.float32(raw["loss"]).view(np.int32)
    with pytest.raises(ValueError, match="labels"):
        ops.seg_loss(t(x), t(y).float())
    with pytest.raises(ValueError, match="labels"):
        ops.seg_loss(t(x), t(y)[:5])
    empty = ops.seg_loss(torch.zeros(0, 21, device=DEV, requires_grad=True), torch.zeros(0, dtype=torch.int64, device=DEV))
    empty.backward()
    assert float(empty.detach()) == 0.0


def test_device_metrics_equal_the_reference_fixture(amd):
    d = np.load(os.path.join(GOLDEN, "seg_head.npz"))
    x, y, split = d["logits"], d["labels"], int(d["split"])
    m = amd.SemSegMetrics(21, [int(c) for c in d["mask_classes"]], device=DEV)
    m.update_metrics(t(x[:split]), t(y[:split]))                             # nothing compacted: masked and -100 rows do not count
    xp = np.full((300, 21), np.nan, dtype=np.float32)
    yp = np.full(300, 5, dtype=np.int64)
    xp[:300 - split], yp[:300 - split] = x[split:], y[split:]
    loss = m.loss(t(xp).requires_grad_(True), t(yp), float(d["smoothings"][1]), n_valid=word(300 - split))   # ... and a padded update
    assert np.isfinite(float(loss.detach()))
    assert np.array_equal(m.accum_gt_, d["accum_gt"]) and np.array_equal(m.accum_union_, d["accum_union"])
    assert np.array_equal(m.accum_intersection_, d["accum_intersection"])
    for name in ("per_class_acc", "per_class_iou", "class_mean_acc", "class_mean_iou", "mean_acc", "mean_iou"):
        assert np.array_equal(np.asarray(getattr(m, name)()), d[name]), name
    # the whole fixture in one pass: the loss is torch's fp64 value to one fp32 unit
    m.reset()
    assert not m.accum_gt_.any() and not m.tallies_.any()
    loss = m.loss(t(x), t(y), float(d["smoothings"][1]))
    assert abs(float(loss) - float(d["loss_1"])) <= R.ulp32(d["loss_1"])
    assert np.array_equal(m.accum_gt_, d["accum_gt"])


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_kernel_and_torch_recipe_meet_the_same_fp64_reference(ops, eps):
    """INTEGRATION.md's recipe, `cross_entropy(..., ignore_index=-100, reduction="sum") / count`, on trimmed fp32 data.  Kernel
    and recipe are each compared with the fp64 reference, not with each other: the kernel within the bounds of this module; the
    recipe, which is fp32 arithmetic throughout, within a first-order bound of that arithmetic -- (classes + 8) roundings of at
    most the largest |x - m| + log(classes) per row, log2(rows) more in the sum."""
    rows, classes = 300, 21
    rng = np.random.default_rng(77)
    x = (rng.standard_normal((rows, classes)) * 4.0).astype(np.float32)
    y = rng.integers(0, classes, rows).astype(np.int64)
    y[::9] = R.IGNORE
    loss, count, lse, _ = R.forward(x, y, eps)
    want = {"loss": loss, "count": count, "lse": lse, "tallies": None, "grad": R.backward(x, y, lse, count, 1.0, eps)}
    assert_meets(device(ops, x, y, eps, None, None, None, g=1.0), want, ("kernel", eps), g=1.0)
    xd = t(x).requires_grad_(True)
    recipe = torch.nn.functional.cross_entropy(xd, t(y), ignore_index=-100, reduction="sum", label_smoothing=float(np.float32(eps))) / count
    recipe.backward()
    u = 2.0 ** -24
    row_scale = float((x.max(1) - x.min(1)).max()) + np.log(classes)
    b_loss = (classes + 8 + np.log2(rows)) * u * row_scale
    b_grad = (classes + 8) * u / count
    e_loss = abs(float(recipe.detach()) - float(np.float64(loss)))
    e_grad = float(np.abs(xd.grad.cpu().numpy().astype(np.float64) - want["grad"]).max())
    print(f"recipe, smoothing {eps}: loss off by {e_loss:.2e} (bound {b_loss:.2e}), gradient by {e_grad:.2e} (bound {b_grad:.2e})")
    assert e_loss <= b_loss and e_grad <= b_grad
    assert not xd.grad[t(y) == R.IGNORE].any()


def test_errors_are_reported_before_any_launch(ops):
    from se3conv3d_amd import _lib

    lib = _lib.load()
    x, y = torch.zeros(8, 21, device=DEV), torch.zeros(8, dtype=torch.int64, device=DEV)
    loss, count, lse = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(8, dtype=torch.float64, device=DEV)
    g, dx = torch.ones(1, device=DEV), torch.zeros(8, 21, device=DEV)
    need = lib.se3_seg_head_workspace_bytes(8, 21)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    p, s = (lambda v: v.data_ptr()), ops._stream(torch.device(DEV))
    fwd = lambda n=8, c=21, bits=64, eps=0.1, xx=p(x), yy=p(y), lo=p(loss), co=p(count), w=p(ws), wsb=need: lib.se3_seg_loss_fwd(
        xx, yy, bits, None, n, None, c, eps, lo, co, p(lse), None, w, wsb, s)
    assert need > 0 and fwd() == 0
    assert [fwd(n=-1), fwd(c=0), fwd(bits=16), fwd(eps=-0.1), fwd(eps=1.5), fwd(eps=float("nan")), fwd(xx=None), fwd(yy=None),
            fwd(lo=None), fwd(co=None), fwd(w=None)] == [-1] * 11
    assert fwd(wsb=need - 1) == -3
    assert fwd(c=1025) == -2 and fwd(n=1 << 27) == -2
    assert fwd(n=0, xx=None, yy=None) == 0 and fwd(eps=0.0) == 0 and fwd(eps=1.0) == 0
    bwd = lambda n=8, c=21, bits=64, eps=0.1, xx=p(x), ls=p(lse), co=p(count), gg=p(g), out=p(dx): lib.se3_seg_loss_bwd(
        xx, p(y), bits, None, ls, co, gg, n, None, c, eps, out, s)
    assert bwd() == 0
    assert [bwd(n=-1), bwd(c=0), bwd(bits=8), bwd(eps=2.0), bwd(xx=None), bwd(ls=None), bwd(co=None), bwd(gg=None), bwd(out=None)] == [-1] * 9
    assert bwd(c=1025) == -2 and bwd(n=1 << 27) == -2 and bwd(n=0, xx=None, ls=None, out=None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- 4. one graph
def test_loss_counters_and_backward_capture_into_four_kernel_nodes_and_follow_the_word(amd, ops):
    rows, classes, eps = 300, 21, 0.1
    x, y, counted, _ = contract(rows, classes, eps)
    m = amd.SemSegMetrics(classes, [classes - 1], device=DEV)
    xd, yd, w, gd = t(x).requires_grad_(True), t(y), word(rows), torch.ones((), device=DEV)
    held = {}

    def step():
        loss = m.loss(xd, yd, eps, n_valid=w)
        # (autograd.grad with the gradient of the loss handed in: the walk then counts the library's nodes, not the fill that
        # makes a `1.0` nor what accumulating into `.grad` would add)
        held.update(loss=loss.detach(), dx=torch.autograd.grad(loss, xd, gd)[0])

    graph = capture(step)
    types = node_types(graph)
    assert HIP_GRAPH_NODE_TYPE_MEMSET not in types and HIP_GRAPH_NODE_TYPE_MEMCPY not in types, types
    assert 2 <= types.count(HIP_GRAPH_NODE_TYPE_KERNEL) <= 4, types
    for valid in (300, 177):
        w.fill_(valid)
        m.reset()
        graph.replay()
        torch.cuda.synchronize()
        tallies = m.tallies_.cpu().numpy().copy()
        eager = device(ops, x, y, eps, counted, valid, np.zeros((3, classes), np.int64), g=1.0)
        assert np.float32(held["loss"].item()).view(np.int32) == np.float32(eager["loss"]).view(np.int32), valid
        assert np.array_equal(bits32(held["dx"]), bits32(eager["grad"])) and np.array_equal(tallies, eager["tallies"]), valid
        want_t = np.zeros((3, classes), np.int64)
        loss, count, lse, _ = R.forward(x, y, eps, counted, valid, want_t)
        want = {"loss": loss, "count": count, "lse": lse, "tallies": want_t, "grad": R.backward(x, y, lse, count, 1.0, eps, counted, valid)}
        assert_meets(eager, want, ("replay", valid), g=1.0)
    graph.replay()                                                           # a second replay ADDS to the counters
    torch.cuda.synchronize()
    assert np.array_equal(m.tallies_.cpu().numpy(), 2 * tallies)


# ------------------------------------------------------------------------------------------------ 5. end to end
def test_a_padded_training_step_with_the_library_head(amd):
    """The step of tests/test_gpu_padded_rows.py::test_a_whole_training_step_replays_as_one_graph -- the MiniUNet of
    test_gpu_network.py with one ResNetFormer behind its first level, on static level-0 buffers of 3000 rows holding 1777
    points -- with `ops.seg_loss(..., n_valid=word)` in place of `cross_entropy(sum) / mask.sum()`: logits and parameter
    gradients against the eager step on the trimmed cloud, at that test's bound."""
    from bounded_levels_cases import cloud
    from test_gpu_network import MiniUNet

    PC = amd.pc
    rows, nb, f, cap, n_cls = 3000, 3, 2, 200000, 5
    cfg = {"pca": True, "n_frames": f, "fixed_axis": False, "neigh_method": "knn", "neigh_kwargs": {"neigh_k": 16}}
    cells, radii = [0.12, 0.25], [0.12, 0.25, 0.5]

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.unet = MiniUNet(amd, 3, [32, 64, 96], n_cls)
            self.block = amd.ResNetFormer(32, 32, self.unet.factory, amd.BatchNormPC, 0.1)

        def forward(self, hier, x, bq):
            u, feats = self.unet, []
            n_lv = len(u.enc_same)
            for lv in range(n_lv):
                x = torch.nn.functional.gelu(u.enc_same[lv](p_pc_in=hier.pcs_[lv], p_pc_out=hier.pcs_[lv], p_in_features=x,
                                                            p_neighborhood=bq(lv, lv)))
                if lv == 0:
                    x = self.block(hier.pcs_[0], x, bq(0, 0))
                feats.append(x)
                if lv + 1 < n_lv:
                    x = torch.nn.functional.gelu(u.enc_down[lv](p_pc_in=hier.pcs_[lv], p_pc_out=hier.pcs_[lv + 1],
                                                                p_in_features=x, p_neighborhood=bq(lv, lv + 1)))
            for lv in range(n_lv - 2, -1, -1):
                up = u.dec_up[lv](p_pc_in=hier.pcs_[lv + 1], p_pc_out=hier.pcs_[lv], p_in_features=x, p_neighborhood=bq(lv + 1, lv))
                pc = hier.pcs_[lv]
                sk = amd.ops.Linear.apply(feats[lv], u.skip[lv].weight, u.skip[lv].bias, getattr(pc, "n_valid_", None), f)
                x = torch.nn.functional.gelu(up + sk)
            return u.head(hier.pcs_[0].feature_pooling(x, "avg"))

    prev = amd.get_precision()
    amd.set_precision("bf16x3")
    torch.manual_seed(7)
    net = Net().to(DEV).train()
    for mod in net.modules():
        if isinstance(mod, amd.PNEConvLayerRotEquiv):
            mod.norm_neigh_dist_.fill_(4.0), mod.norm_num_neighs_.fill_(0.05)
    with torch.no_grad():
        for sk in (net.block.skip_path_1_, net.block.skip_path_2_):
            sk.gamma_.fill_(0.5)
    params = list(net.parameters())
    bn_state0 = {k: v.clone() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k}

    def with_draws(fn, feed=None):
        """`fn()` with the (nb,) gate draws of the block's skip connections kept (feed None) or replayed."""
        draws, real_rand = [], torch.rand

        def rand(*a, **k):
            out = real_rand(*a, **k)
            if tuple(out.shape) != (nb,):
                return out
            if feed is not None:
                return feed.pop(0)
            draws.append(out)
            return out

        torch.rand = rand
        try:
            return fn(), draws
        finally:
            torch.rand = real_rand

    try:
        sizes, seed = (577, 1200, 0), 12
        pts, bid = cloud(sizes, seed)
        n = sum(sizes)
        g = torch.Generator().manual_seed(seed)
        x, lab = torch.randn(n * f, 3, generator=g), torch.randint(0, n_cls, (n,), generator=g)
        lab[::13] = -100                                                    # unlabelled points among the present ones
        s_pts = torch.full((rows, 3), float("nan"), device=DEV)
        s_bid = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
        s_x = torch.zeros(rows * f, 3, device=DEV)
        s_lab = torch.full((rows,), 2, dtype=torch.int64, device=DEV)      # absent labels that WOULD count: the word keeps them out
        s_pts[:n], s_bid[:n], s_x[:n * f], s_lab[:n] = pts.to(DEV), bid.to(DEV), x.to(DEV), lab.to(DEV)
        s_word = word(n)
        tallies = torch.zeros(3, n_cls, dtype=torch.int64, device=DEV)

        amd.PNEConvLayerRotEquiv.empty_rot_tenors_cache()
        pc0 = PC.PointcloudRotEquiv(s_pts, s_bid, cfg, p_n_valid=s_word, num_batches=nb, p_padded_rows=True)
        hier = PC.PointHierarchyRotEquiv(pc0, 2, "grid_avg", p_capacities="input", p_padded=True, p_padded_rows=True, grid_radii=cells)
        nbhs = {}

        def bq(a, b):
            if (a, b) not in nbhs:
                nbhs[(a, b)] = PC.BQNeighborhood(hier.pcs_[a], hier.pcs_[b], radii[max(a, b)], p_capacity=cap)
            return nbhs[(a, b)]

        logits, draws = with_draws(lambda: net(hier, s_x, bq))
        loss = amd.ops.seg_loss(logits, s_lab, n_valid=s_word, tallies=tallies)
        loss.backward()
        level_n = hier.level_sizes()
        assert level_n[0] == n and not hier.overflowed() and not any(v.overflowed() for v in nbhs.values())
        got_logits, got_loss = logits.detach()[:n].clone(), float(loss.detach())
        got_grad = torch.cat([p.grad.reshape(-1) for p in params]).clone()
        assert len(draws) == 2 and bool(torch.isfinite(got_grad).all())

        # the eager step of the same modules and weights on the trimmed levels, with the frames and gate draws of the padded one
        net.load_state_dict(bn_state0, strict=False)
        for p in params:
            p.grad = None
        amd.PNEConvLayerRotEquiv.empty_rot_tenors_cache()
        pcs = [PC.PointcloudRotEquiv.from_frames(pc.pts_[:m_].clone(), pc.batch_ids_[:m_].clone(), pc.local_frames_[:m_].clone(),
                                                 num_batches=nb) for pc, m_ in zip(hier.pcs_, level_n)]
        eager = type("Levels", (), {"pcs_": pcs})()
        enb = {}

        def ebq(a, b):
            if (a, b) not in enb:
                enb[(a, b)] = PC.BQNeighborhood(pcs[a], pcs[b], radii[max(a, b)])
            return enb[(a, b)]

        e_logits, _ = with_draws(lambda: net(eager, x.to(DEV), ebq), feed=list(draws))
        e_loss = torch.nn.functional.cross_entropy(e_logits, lab.to(DEV), ignore_index=-100)
        e_loss.backward()
        want_grad = torch.cat([p.grad.reshape(-1) for p in params])
        e_out = float((got_logits - e_logits.detach()).norm() / e_logits.detach().norm())
        e_grad = float((got_grad - want_grad).norm() / want_grad.norm())
        print(f"{n} points: logits {e_out:.3e}, parameter gradients {e_grad:.3e} (bound 2e-4), loss {got_loss:.6f} / {float(e_loss):.6f}")
        assert e_out < 2e-4 and e_grad < 2e-4 and abs(got_loss - float(e_loss)) < 2e-4 * abs(float(e_loss))
        kept = lab != -100
        pred = e_logits.detach().argmax(1).cpu()
        assert int(tallies[0].sum()) == int(kept.sum()) and int(tallies[1].sum()) == int(kept.sum())
        assert abs(int(tallies[2].sum()) - int((pred[kept] == lab[kept]).sum())) <= 2      # (a near tie may fall the other way)
    finally:
        amd.set_precision(prev)
