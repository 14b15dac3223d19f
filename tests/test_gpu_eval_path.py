"""GPU: the evaluation path -- `eval()`, `torch.no_grad()`, `torch.inference_mode()` -- against the training path and the
float64 restatement of tests/eval_path_reference.py.

(a) every autograd class forward with gradients wanted, with none wanted, under `no_grad` and under `inference_mode` on
    inputs created inside the block: the same bits, `requires_grad` only where a gradient was asked for, no input changed.
    `SE3ConvFunction` keeps neither T nor the packed feature words when nothing needs a gradient: that forward is held row
    by row against the fp64 oracle (tests/rowwise_error.py), it allocates `out` alone outside its workspace, and it gives
    the bits of the T-keeping forward wherever `se3conv_forms` lists the same forms for both.
(b) `BatchNormPC`, `DropPathPC`, `SkipConnection` and the convolution layers in `eval()`, per element or by bits; the
    pre-process pass under `eval()` + `no_grad`.
(c) the three blocks of the reference's fixtures in `eval()` against the eval restatement, plain and on a padded cloud; the
    MiniUNet across scenes on the same module objects; one eval block captured on a padded cloud and replayed on another count.
(d) clouds, hierarchy, neighbourhoods and a convolution built inside `inference_mode`.
The last test prints every observed / bound ratio (profiles/eval_path.txt)."""
import contextlib
import math

import numpy as np
import pytest
import torch

import eval_path_reference as E
import form_coverage_table as FC
import rowwise_error as RW
from conftest import canon_edges, rel_err
from oracle import se3conv_oracle as O
from padded_cases import DEV, word

pytestmark = pytest.mark.gpu
MODES = (("fp32", 5e-6), ("bf16x3", 5e-5), ("bf16x3_t16", 5e-5))   # test_gpu_group_norm_blocks.py
RATIOS = {}
F = np.float32


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd as amd
    prev = amd.get_precision()
    yield amd
    amd.set_precision(prev)


@contextlib.contextmanager
def precision(amd, name):
    prev = amd.get_precision()
    amd.set_precision(name)
    try:
        yield
    finally:
        amd.set_precision(prev)


def same_bits(a, b):
    """Bit for bit (NaN and -0.0 would show)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.detach().contiguous().reshape(-1).view(torch.uint8).cpu(), b.detach().contiguous().reshape(-1).view(torch.uint8).cpu())


def zero_bits(t):
    return not bool(t.detach().contiguous().reshape(-1).view(torch.uint8).any())


def dev(a):
    a = np.asarray(a)
    return torch.from_numpy(a if a.ndim == 0 else np.ascontiguousarray(a)).to(DEV)


def record(name, ratio):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(ratio))


# ------------------------------------------------------------------------------------------------ (a) the grad-mode matrix
GRAD_MODES = {"grad": contextlib.nullcontext, "plain": contextlib.nullcontext, "no_grad": torch.no_grad,
              "inference": torch.inference_mode}


def _glue(seed, rows=257, c=24, batches=3):
    g = np.random.default_rng(seed)
    ids = np.sort(g.integers(0, batches, rows)).astype(np.int32)
    return g, ids


def _case_feat_basis_proj():
    import pne_reference as P
    m = P.max_case(200, 8, 24)
    g = np.random.default_rng(1)
    return ({"basis": m["phi"], "feat": g.standard_normal((40, 8)).astype(F)}, {"nb": m["neighbors"], "ends": m["ends"]},
            lambda ops, t: ops.FeatBasisProj.apply(t["basis"], t["feat"], t["nb"], t["ends"]))


def _case_pne_embed():
    import pne_reference as P
    c = P.embed_case(102, "mlp_gelu", 32)
    return ({"A": c["A"], "beta": c["beta"]}, {"pts": c["pts"], "samples": c["samples"], "nb": c["neighbors"]},
            lambda ops, t: ops.PneEmbed.apply(t["pts"], t["samples"], t["nb"], t["A"], t["beta"], float(c["rho"]), c["kind"], None, c["sigma"]))


def _case_neigh_conv_max():
    import pne_reference as P
    m = P.max_case(201, 8, 24)
    return ({"phi": m["phi"], "G": m["G"]}, {"nb": m["neighbors"], "ends": m["ends"]},
            lambda ops, t: ops.NeighConvMax.apply(t["phi"], t["G"], t["nb"], t["ends"], m["G"].shape[0]))


def _case_basis_attention():
    import basis_att_reference as B
    c = B.case(401, *B.CASES[1])
    return ({"T": c["T"], "key": c["key"], "pe": c["pe"]}, {},
            lambda ops, t: ops.BasisAttention.apply(t["T"], t["key"], t["pe"], c["heads"]))


def _case_fused_basis_attention():
    import att_fused_reference as A
    c = A.case(401, *A.CASES[1])
    return ({"phi": c["phi"], "x": c["x"], "pe": c["pe"]}, {"nb": c["neighbors"], "ends": c["ends"]},
            lambda ops, t: ops.FusedBasisAttention.apply(t["phi"], t["x"], t["pe"], t["nb"], t["ends"], c["heads"]))


def _case_group_norm():
    g, ids = _glue(3)
    x = (g.standard_normal((257 * 2, 24)) * 3 + 1).astype(F)
    return ({"x": x, "gamma": g.uniform(0.5, 1.5, (1, 24)).astype(F), "beta": g.uniform(-1, 1, (1, 24)).astype(F)}, {"ids": ids},
            lambda ops, t: ops.GroupNorm.apply(t["x"], t["gamma"], t["beta"], t["ids"], 3, 8, 1e-8, None, 2))


def _case_skip_drop_path():
    g, ids = _glue(4)
    return ({"x": g.standard_normal((257, 24)).astype(F), "y": g.standard_normal((257, 24)).astype(F),
             "gamma": g.uniform(0.5, 1.5, (1, 24)).astype(F)}, {"u": g.uniform(0, 1, 3).astype(F), "ids": ids},
            lambda ops, t: ops.SkipDropPath.apply(t["x"], t["y"], t["gamma"], t["u"], t["ids"], 0.7))


def _case_bias_gelu():
    g, _ = _glue(5)
    return ({"z": (g.standard_normal((257, 24)) * 2).astype(F), "bias": g.standard_normal(24).astype(F)}, {},
            lambda ops, t: ops.BiasGelu.apply(t["z"], t["bias"]))


def _case_linear():
    g, _ = _glue(6)
    return ({"x": g.standard_normal((257, 24)).astype(F), "w": g.standard_normal((40, 24)).astype(F), "b": g.standard_normal(40).astype(F)}, {},
            lambda ops, t: ops.Linear.apply(t["x"], t["w"], t["b"]))


def _cells(ops, t, n_cells):
    return ops.GridCells(t["cell_ids"], t["sorted_ids"], t["cell_ends"], n_cells, None, None)


def _case_grid_pool():
    import rowwise_passes_reference as REF
    n, sorted_ids, cell_ends, cell_ids = REF.segment_level()
    fixed = {"cell_ids": cell_ids, "sorted_ids": sorted_ids, "cell_ends": cell_ends}
    return ({"x": REF.pool_data(n, 7, "ties")}, fixed, lambda ops, t: ops.GridPool.apply(t["x"], _cells(ops, t, len(cell_ends)), "max"))


def _case_grid_upsample():
    import rowwise_passes_reference as REF
    n, sorted_ids, cell_ends, cell_ids = REF.segment_level()
    fixed = {"cell_ids": cell_ids, "sorted_ids": sorted_ids, "cell_ends": cell_ends}
    return ({"x": REF.pool_data(len(cell_ends), 7, "uneven", 1)}, fixed,
            lambda ops, t: ops.GridUpsample.apply(t["x"], _cells(ops, t, len(cell_ends))))


def _case_frame_pool():
    import rowwise_passes_reference as REF
    return {"x": REF.frame_data(3, 7, "uneven")}, {}, lambda ops, t: ops.FramePool.apply(t["x"], 3, "max")


def _case_global_pool():
    g, ids = _glue(7)
    return ({"x": g.standard_normal((257 * 2, 24)).astype(F)}, {"ids": ids},
            lambda ops, t: ops.GlobalPool.apply(t["x"], t["ids"], 3, "avg", 2))


def _case_global_upsample():
    g, ids = _glue(8)
    return {"x": g.standard_normal((3, 24)).astype(F)}, {"ids": ids}, lambda ops, t: ops.GlobalUpsample.apply(t["x"], t["ids"], 2)


def _case_seg_loss():
    g, _ = _glue(9)
    labels = g.integers(0, 13, 257).astype(np.int64)
    labels[::17] = -100
    return {"logits": (g.standard_normal((257, 13)) * 3).astype(F)}, {"labels": labels}, lambda ops, t: ops.SegLoss.apply(t["logits"], t["labels"], 0.1)


def _case_rows_gather():
    g, _ = _glue(10)
    return ({"x": g.standard_normal((257, 24)).astype(F)}, {"idx": g.permutation(257)[:100].astype(np.int32)},
            lambda ops, t: ops.RowsGather.apply(t["x"], t["idx"]))


def _case_rows_scatter():
    g, _ = _glue(11)
    return ({"x": g.standard_normal((100, 24)).astype(F)}, {"idx": g.permutation(257)[:100].astype(np.int32)},
            lambda ops, t: ops.RowsScatter.apply(t["x"], t["idx"], 257))


def _picked_level(seed, rows=50, present=40, capacity=20, kept=15):
    """A padded random level by hand: `cell_ids [rows]` (-1 behind the present rows), `picked [capacity]` (the row each kept
    cell picked, -1 behind the kept cells)."""
    g = np.random.default_rng(seed)
    cell_ids = np.full(rows, -1, np.int32)
    cell_ids[:present] = np.concatenate([np.arange(kept), g.integers(0, kept, present - kept)])[g.permutation(present)]
    picked = np.full(capacity, -1, np.int32)
    for j in range(kept):
        picked[j] = g.choice(np.flatnonzero(cell_ids == j))
    return g, cell_ids, picked


def _case_rows_gather_padded():
    g, cell_ids, picked = _picked_level(12)
    return ({"x": g.standard_normal((50, 24)).astype(F)}, {"cell_ids": cell_ids, "picked": picked},
            lambda ops, t: ops.RowsGatherPadded.apply(t["x"], t["cell_ids"], t["picked"]))


def _case_rows_unpick_padded():
    g, cell_ids, picked = _picked_level(13)
    return ({"x": g.standard_normal((20, 24)).astype(F)}, {"cell_ids": cell_ids, "picked": picked},
            lambda ops, t: ops.RowsUnpickPadded.apply(t["x"], t["cell_ids"], t["picked"]))


GRAD_CASES = {"FeatBasisProj": _case_feat_basis_proj, "PneEmbed": _case_pne_embed, "NeighConvMax": _case_neigh_conv_max,
              "BasisAttention": _case_basis_attention, "FusedBasisAttention": _case_fused_basis_attention,
              "GroupNorm": _case_group_norm, "SkipDropPath": _case_skip_drop_path, "BiasGelu": _case_bias_gelu, "Linear": _case_linear,
              "GridPool": _case_grid_pool, "GridUpsample": _case_grid_upsample, "FramePool": _case_frame_pool,
              "GlobalPool": _case_global_pool, "GlobalUpsample": _case_global_upsample, "SegLoss": _case_seg_loss,
              "RowsGather": _case_rows_gather, "RowsScatter": _case_rows_scatter, "RowsGatherPadded": _case_rows_gather_padded,
              "RowsUnpickPadded": _case_rows_unpick_padded}


def run_in_mode(mode, diff, fixed, call):
    """The outputs (a tuple) of `call` on fresh device tensors created inside the mode's block; the inputs must come back
    with the bits they went in with."""
    with GRAD_MODES[mode]():
        t = {k: dev(v) for k, v in {**diff, **fixed}.items()}
        if mode == "grad":
            for k in diff:
                t[k].requires_grad_(True)
        if mode == "inference":
            assert all(v.is_inference() for v in t.values())
        before = {k: v.detach().clone() for k, v in t.items()}
        out = call(t)
        outs = out if isinstance(out, tuple) else (out,)
        torch.cuda.synchronize()
        for k, v in t.items():
            assert same_bits(v, before[k]), f"{mode}: input {k} was changed"
        floats = [o for o in outs if o.is_floating_point()]
        assert floats and all(o.requires_grad == (mode == "grad") for o in floats), (mode, [o.requires_grad for o in outs])
        assert all(o.grad_fn is None for o in outs) or mode == "grad"
        return tuple(o.detach().clone() for o in outs)


def assert_same_across_modes(diff, fixed, call, what, modes=tuple(GRAD_MODES)):
    runs = {mode: run_in_mode(mode, diff, fixed, call) for mode in modes}
    first = runs[modes[0]]
    for mode in modes[1:]:
        assert len(runs[mode]) == len(first)
        for i, (a, b) in enumerate(zip(first, runs[mode])):
            assert same_bits(a, b), f"{what}: output {i} under {mode} differs from {modes[0]}"
    return runs


@pytest.mark.parametrize("name", list(GRAD_CASES))
def test_forward_bits_do_not_depend_on_the_grad_mode(amd, name):
    diff, fixed, call = GRAD_CASES[name]()
    assert_same_across_modes(diff, fixed, lambda t: call(amd.ops, t), name)


@pytest.fixture(scope="module")
def conv_cases():
    """The two smallest cases of tests/rowwise_error.py (single-wavefront forms; wave-pair kernel with two channel tiles), their
    oracle edges and the fp64 reference with its scales: computed once, never written to."""
    out = []
    for name, make in RW.rowwise_cases()[:2]:
        c = make()
        nb, ends, rho, nu = RW.graph_of(c)
        out.append((name, c, nb, ends, rho, nu, RW.reference_and_scales(c, nb, rho, nu)))
    return out


@pytest.mark.parametrize("mode", [m for m, _ in MODES])
def test_conv_forward_without_t_is_the_forward_with_t(amd, conv_cases, mode):
    import test_gpu_parity as P
    ops = amd.ops
    with precision(amd, mode):
        for name, c, nb, ends, rho, nu, (ref64, s2) in conv_cases:
            diff = {k: c[k].numpy() for k in ("x", "a", "b", "w")}
            fixed = {"pts": c["pts_in"].numpy(), "frames": c["fi"].numpy(), "nb": nb.to(torch.int32).numpy(), "ends": ends.to(torch.int32).numpy()}
            assert c["pts_out"] is c["pts_in"]

            def call(t):
                geom = ops.ConvGeometry.build(t["pts"], t["pts"], t["frames"], t["frames"], t["nb"], t["ends"])
                return ops.SE3ConvFunction.apply(t["x"], t["a"], t["b"], t["w"], geom, rho, nu)

            n, f, c_in, c_out = c["pts_in"].shape[0], c["fi"].shape[1], c["x"].shape[1], c["go"].shape[1]
            shape = (mode, n, n, int(nb.shape[0]), f, f, c_in, c_out)
            with_t, without_t = FC.lines(shape, ("fwd", 0, 0, None)), FC.lines(shape, ("fwd", 0, 0, 0))
            # the three forwards that keep nothing agree by bits whatever the forms; the T-keeping one where the forms do
            runs = assert_same_across_modes(diff, fixed, call, f"{name} {mode}", modes=("plain", "no_grad", "inference"))
            kept = run_in_mode("grad", diff, fixed, call)
            same_forms = with_t == without_t
            print(f"{name} {mode}: forward forms with T {with_t} without {without_t} -> {'bit equality asserted' if same_forms else 'forms differ'}")
            if same_forms:
                assert same_bits(kept[0], runs["no_grad"][0]), f"{name} {mode}: the same forms, other bits"
            for label, out in (("no_grad", runs["no_grad"][0]), ("grad", kept[0])):
                ratios = RW.ratios({"out": out}, ref64, s2)
                print(f"    {label}: out rowwise {ratios['out']:.3e} (bound {RW.TOLERANCES[mode]['out']:.3e}), rel_err "
                      f"{rel_err(out, ref64['out']):.3e} (bound {P.TOLS[mode]:.0e})")
                record(f"conv {name} {mode} {label} rowwise", ratios["out"] / RW.TOLERANCES[mode]["out"])
                P.assert_rowwise(ratios, mode, f"{name} {label}", skip=[e for e in RW.ENTRIES if e != "out"])
                assert rel_err(out, ref64["out"]) < P.TOLS[mode]


@pytest.mark.parametrize("mode", [m for m, _ in MODES])
def test_conv_forward_without_gradients_allocates_out_alone(amd, conv_cases, mode):
    """`ops._empty`, `ops._empty_like` and `ops._workspace` (the names tests/hostile_memory.py swaps) during a `no_grad`
    forward: one `_empty` for `out`, one workspace, nothing the size of T or of the packed feature words."""
    ops = amd.ops
    name, c, nb, ends, rho, nu, _ = conv_cases[0]
    t = {k: c[k].to(DEV) for k in ("x", "a", "b", "w")}
    geom = ops.ConvGeometry.build(c["pts_in"].to(DEV), c["pts_in"].to(DEV), c["fi"].to(DEV), c["fi"].to(DEV), nb.to(torch.int32).to(DEV), ends.to(torch.int32).to(DEV))
    calls = {"empty": [], "empty_like": [], "workspace": []}
    saved = ops._empty, ops._empty_like, ops._workspace

    def empty(*a, **k):
        out = torch.empty(*a, **k)
        calls["empty"].append((tuple(out.shape), out.dtype))
        return out

    def empty_like(x, *a, **k):
        calls["empty_like"].append((tuple(x.shape), x.dtype))
        return torch.empty_like(x, *a, **k)

    def workspace(nbytes, device):
        calls["workspace"].append(int(nbytes))
        return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)

    rows, c_in, c_out = c["x"].shape[0], c["x"].shape[1], c["go"].shape[1]
    with precision(amd, mode):
        for grad in (False, True):
            for v in calls.values():
                v.clear()
            ops._empty, ops._empty_like, ops._workspace = empty, empty_like, workspace
            try:
                if grad:
                    out = ops.SE3ConvFunction.apply(t["x"], t["a"].clone().requires_grad_(True), t["b"], t["w"].clone().requires_grad_(True), geom, rho, nu)
                else:
                    with torch.no_grad():
                        out = ops.SE3ConvFunction.apply(t["x"], t["a"], t["b"], t["w"], geom, rho, nu)
            finally:
                ops._empty, ops._empty_like, ops._workspace = saved
            torch.cuda.synchronize()
            sizes = [math.prod(s) for s, _ in calls["empty"]]
            if grad:
                # the recorder sees what the gradient-keeping forward keeps: parameter gradients alone read T here
                assert rows * c_in * 32 in sizes or (mode != "fp32" and (((rows * c_in,), torch.int32) in calls["empty"])), calls
                continue
            assert calls["empty"] == [((rows, c_out), torch.float32)], calls
            assert not calls["empty_like"] and len(calls["workspace"]) == 1, calls
            assert rows * c_in * 32 not in sizes and ((rows * c_in,), torch.int32) not in calls["empty"]
            assert not out.requires_grad


# ------------------------------------------------------------------------------------------------ (b) modules in eval()
class PlainCloud:
    """What the block glue reads of an ordinary cloud."""

    def __init__(self, ids, batches):
        self.batch_ids_ = self.batch_ids_considering_frames_ = ids
        self.batch_size_ = torch.tensor(batches)
        self.pts_ = torch.zeros(ids.shape[0], 3, device=ids.device)

    def num_batches(self):
        return int(self.batch_size_)


def padded_cloud(amd, present, rows, batches=2, frames=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    pts = torch.full((rows, 3), float("nan"), device=DEV)
    pts[:present] = torch.rand(present, 3, generator=g).to(DEV)
    bid = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    bid[:present] = (torch.arange(present) * batches // present).to(torch.int32).to(DEV)
    fr = torch.eye(3, device=DEV).reshape(1, 1, 9).repeat(rows, frames, 1)
    return amd.pc.PointcloudRotEquiv.from_frames(pts, bid, fr, p_n_valid=word(present), num_batches=batches, p_padded_rows=True)


def loaded_bn(amd, d):
    bn = amd.blocks.BatchNormPC(d["x"].shape[1]).to(DEV)
    with torch.no_grad():
        bn.layer_.weight.copy_(dev(d["weight"])), bn.layer_.bias.copy_(dev(d["bias"]))
        bn.layer_.running_mean.copy_(dev(d["running_mean"])), bn.layer_.running_var.copy_(dev(d["running_var"]))
        bn.layer_.num_batches_tracked.fill_(5)
    return bn.eval()


@pytest.mark.parametrize("c", E.BOUND_CHANNELS)
@pytest.mark.parametrize("rows", E.BOUND_ROWS)
def test_batch_norm_in_eval_per_element(amd, rows, c):
    d = E.bn_bounds_case(rows, c, 1000 * rows + c)
    bn = loaded_bn(amd, d)
    state0 = {k: v.clone() for k, v in bn.state_dict().items()}
    pc = PlainCloud(torch.zeros(rows, dtype=torch.int32, device=DEV), 1)
    x = dev(d["x"])
    with torch.no_grad():
        y = bn(x, pc)
        y2 = bn(x, pc)
    ref, scale, _, _ = E.batch_norm(**d)
    r = E.worst(y.cpu().numpy(), ref, scale) / E.bounds()["bn_eval"]
    print(f"BatchNormPC eval rows={rows} c={c}: observed / bound = {r:.3f}")
    record("bn_eval", r)
    assert r <= 1.0
    assert same_bits(y, y2) and not y.requires_grad
    for k, v in bn.state_dict().items():
        assert same_bits(v, state0[k]), f"{k} changed in eval"
    # with gradients enabled the eval form gives the same bits (and a graph through weight and bias)
    assert same_bits(bn(x, pc), y)
    # the planted mix-up would not pass: batch statistics in place of running ones
    if rows > 1:
        assert E.worst(E.batch_norm(**d, fault="batch_stats")[0], ref, scale) > 10 * E.bounds()["bn_eval"]


def test_batch_norm_in_eval_on_padded_rows(amd):
    """300 rows, 200 present, absent feature rows of 1e3: the present rows are the call on the trimmed tensor by bits, the
    absent rows finite (the row-wise torch path reads them; what follows -- a convolution, `ops.Linear` with the row-count
    word, the skip kernel -- restores the zeros, test_eval_blocks_on_a_padded_cloud), the statistics untouched."""
    d = E.bn_bounds_case(200, 24, 77)
    bn = loaded_bn(amd, d)
    state0 = {k: v.clone() for k, v in bn.state_dict().items()}
    pc = padded_cloud(amd, 200, 300)
    x = torch.full((300, 24), 1e3, device=DEV)
    x[:200] = dev(d["x"])
    with torch.no_grad():
        y = bn(x, pc)
        trimmed = bn(x[:200].clone(), PlainCloud(torch.zeros(200, dtype=torch.int32, device=DEV), 1))
    assert same_bits(y[:200], trimmed) and bool(torch.isfinite(y[200:]).all())
    ref, scale, _, _ = E.batch_norm(**d)
    r = E.worst(y[:200].cpu().numpy(), ref, scale) / E.bounds()["bn_eval"]
    record("bn_eval padded", r)
    assert r <= 1.0
    for k, v in bn.state_dict().items():
        assert same_bits(v, state0[k]), f"{k} changed in eval"


@pytest.mark.parametrize("padded", [False, True], ids=["plain", "padded"])
def test_drop_path_and_skip_connection_in_eval(amd, padded):
    c, present, rows = 24, 200, 300
    s = E.skip_bounds_case(present, c, 5)
    if padded:
        pc = padded_cloud(amd, present, rows)
        x, y = (torch.full((rows, c), 1e3, device=DEV) for _ in range(2))
        x[:present], y[:present] = dev(s["x"]), dev(s["y"])
    else:
        pc = PlainCloud((torch.arange(present) * 2 // present).to(torch.int32).to(DEV), 2)
        x, y = dev(s["x"]), dev(s["y"])
    rng0 = torch.cuda.get_rng_state()
    dp = amd.blocks.DropPathPC(0.4).eval()
    skip = amd.blocks.SkipConnection(0.4, c).to(DEV).eval()
    train0 = amd.blocks.SkipConnection(0.0, c).to(DEV).train()
    with torch.no_grad():
        skip.gamma_.copy_(dev(s["gamma"])), train0.gamma_.copy_(dev(s["gamma"]))
        out_dp = dp(x, pc)
        out = skip(x, y, pc)
        out_train0 = train0(x, y, pc)
    assert torch.equal(torch.cuda.get_rng_state(), rng0), "an eval pass drew from the generator"
    assert same_bits(out_dp, x), "DropPathPC in eval is the identity"
    ref, scale = E.skip(**s, drop_prob=0.4)
    r = E.worst(out[:present].cpu().numpy(), ref, scale) / E.bounds()["skip_eval"]
    print(f"SkipConnection eval {'padded' if padded else 'plain'}: observed / bound = {r:.3f}")
    record("skip_eval" + (" padded" if padded else ""), r)
    assert r <= 1.0
    assert same_bits(out, out_train0), "eval with drop_prob 0.4 is training with drop_prob 0"
    if padded:
        assert zero_bits(out[present:])
    for fault in ("keep_factor", "no_gamma"):
        assert E.worst(E.skip(**s, drop_prob=0.4, fault=fault)[0], ref, scale) > 10 * E.bounds()["skip_eval"]


def small_scene(amd, n, seed, frames=2, batches=2):
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(n, 3, generator=g)
    bid = (torch.arange(n) * batches // n).to(torch.int32)
    return pts, bid, O.random_frames(n, frames, g)


def _layers(amd):
    yield "PNEConvLayerRotEquiv", True, lambda: amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu").create_conv_layer(16, 24)
    yield "PNEConvLayer", False, lambda: amd.PNEConvLayerFactory(3, 32, "mlp_gelu").create_conv_layer(16, 24)
    for fused in (False, True):
        yield f"MultiHeadAttLayer fused={fused}", False, lambda f=fused: amd.MultiHeadAttLayerFactory(3, 16, "single", 2, p_fused=f).create_conv_layer(16, 24)
        yield f"LoRAttConvLayer fused={fused}", False, lambda f=fused: amd.LoRAttConvLayerFactory(3, 16, "single", 2, p_fused=f).create_conv_layer(16, 24)


def test_convolution_layers_in_eval_are_their_training_forward(amd):
    n = 300
    pts, bid, frames = small_scene(amd, n, 21)
    r = O.radius_for_degree(n / 2, 10)
    pc_rot = amd.pc.PointcloudRotEquiv.from_frames(pts.to(DEV), bid.to(DEV), frames.to(DEV))
    pc = amd.pc.Pointcloud(pts.to(DEV), bid.to(DEV))
    g = torch.Generator().manual_seed(3)
    for name, rot, make in _layers(amd):
        torch.manual_seed(11)
        conv = make().to(DEV)
        cloud = pc_rot if rot else pc
        nbh = amd.pc.BQNeighborhood(cloud, cloud, r)
        conv.norm_neigh_dist_.fill_(1.0 / r), conv.norm_num_neighs_.fill_(n / nbh.num_edges())
        x = torch.randn(n * (2 if rot else 1), 16, generator=g).to(DEV)
        state0 = {k: v.clone() for k, v in conv.state_dict().items()}
        want = conv.train()(p_pc_in=cloud, p_pc_out=cloud, p_in_features=x, p_neighborhood=nbh).detach()
        conv.eval()
        with torch.no_grad():
            got = conv(p_pc_in=cloud, p_pc_out=cloud, p_in_features=x, p_neighborhood=nbh)
        with torch.inference_mode():
            got_inf = conv(p_pc_in=cloud, p_pc_out=cloud, p_in_features=x, p_neighborhood=nbh)
        assert same_bits(got, want), f"{name}: eval + no_grad differs from the training forward"
        assert same_bits(got_inf, want), f"{name}: inference_mode differs from the training forward"
        assert not got.requires_grad and bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
        for k, v in conv.state_dict().items():
            assert same_bits(v, state0[k]), f"{name}: {k} changed"


@pytest.mark.parametrize("mode", ["no_grad", "inference_mode"])
@pytest.mark.parametrize("kind", ["ball_query", "capacity", "knn"])
def test_pre_process_pass_under_eval_and_no_grad(amd, kind, mode):
    """`start_pre_process()` + `eval()` + `no_grad`, as `pre_process()` of the reference's task scripts (and the same inside
    `inference_mode`): both buffers follow `oracle.ema_update` (a k-NN neighbourhood: half the inverse mean edge length,
    IConvLayer.py:76-97), and a training step behind it still runs -- the buffers are nothing autograd refuses to save."""
    n = 300
    pts, bid, frames = small_scene(amd, n, 22)
    r = O.radius_for_degree(n / 2, 10)
    pc = amd.pc.PointcloudRotEquiv.from_frames(pts.to(DEV), bid.to(DEV), frames.to(DEV))
    if kind == "knn":
        nbh = amd.pc.KnnNeighborhood(pc, pc, 8)
    else:
        nbh = amd.pc.BQNeighborhood(pc, pc, r, p_capacity=20000 if kind == "capacity" else None)
    torch.manual_seed(5)
    conv = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu").create_conv_layer(16, 24).to(DEV)
    x = torch.randn(n * 2, 16, device=DEV)
    n_edges = nbh.num_edges() if hasattr(nbh, "num_edges") else nbh.neighbors_.shape[0]
    if kind == "knn":
        nb = nbh.neighbors_.cpu().long()
        mean_len = float((pts[nb[:, 1]] - pts[nb[:, 0]]).double().norm(dim=1).mean())
        radius = 2.0 * mean_len                       # ema_update's 1 / radius = 1 / (2 mean length)
    else:
        radius = r
    rho, nu = torch.tensor(0.0), torch.tensor(0.0)
    conv.start_pre_process()
    conv.eval()
    params0 = [p.detach().clone() for p in conv.parameters()]
    with getattr(torch, mode)():
        for step in range(3):
            conv(p_pc_in=pc, p_pc_out=pc, p_in_features=x, p_neighborhood=nbh)
            rho, nu = O.ema_update(rho, nu, radius, nbh.start_ids_.shape[0], n_edges)
            assert math.isclose(float(conv.norm_neigh_dist_), float(rho), rel_tol=2e-6 if kind == "knn" else 1e-6), (step, kind)
            assert math.isclose(float(conv.norm_num_neighs_), float(nu), rel_tol=1e-6), (step, kind)
    conv.end_pre_process()
    assert not conv.pre_process_ and all(same_bits(p, q) for p, q in zip(conv.parameters(), params0))
    assert not conv.norm_neigh_dist_.is_inference() and not conv.norm_num_neighs_.is_inference()
    conv.train()
    xg = x.clone().requires_grad_(True)
    conv(p_pc_in=pc, p_pc_out=pc, p_in_features=xg, p_neighborhood=nbh).sum().backward()
    assert bool(torch.isfinite(xg.grad).all()) and all(bool(torch.isfinite(p.grad).all()) for p in conv.parameters())
    assert sorted(conv.state_dict()) == sorted(["conv_weights_", "norm_neigh_dist_", "norm_num_neighs_", "proj_axes_", "proj_biases_"])


# ------------------------------------------------------------------------------------------------ (c) blocks and a network
@pytest.fixture(scope="module")
def block_states():
    """Per fixture: class, the fixture, and per state (tests/eval_path_reference.py::eval_states) the float64 eval output."""
    out = {}
    for name in ("resnetformer", "resnetb", "resconvnext"):
        cls, geom, d, entries = E.eval_states(name)
        out[name] = (cls, d, [(label, norm, state, E.block_forward(cls, state, geom, d["x"], norm, drop_prob=0.1)[0])
                              for label, norm, state in entries])
    return out


def eval_block(amd, cls, d, norm, state):
    c_in, c_out = d["x"].shape[1], d["out"].shape[1]
    norm_layer = amd.BatchNormPC if norm == "batch" else amd.GroupNormPC
    blk = getattr(amd, cls)(c_in, c_out, amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu"), norm_layer, 0.1).to(DEV)
    res = blk.load_state_dict({k: dev(np.asarray(v)) for k, v in state.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return blk.eval()


@pytest.mark.parametrize("name", ["resnetformer", "resnetb", "resconvnext"])
def test_eval_blocks_against_the_restatement(amd, block_states, name):
    cls, d, entries = block_states[name]
    t = lambda k: dev(np.asarray(d[k]))
    pc = amd.pc.PointcloudRotEquiv.from_frames(t("pts"), t("batch"), t("frames"))
    nbh = amd.pc.BQNeighborhood(pc, pc, float(d["radius"]))
    for label, norm, state, want in entries:
        for mode, tol in MODES:
            with precision(amd, mode):
                blk = eval_block(amd, cls, d, norm, state)
                state0 = {k: v.clone() for k, v in blk.state_dict().items()}
                rng0 = torch.cuda.get_rng_state()
                with torch.no_grad():
                    out = blk(pc, t("x"), nbh)
                err = E.rel_err(out.cpu().numpy(), want)
                print(f"{cls} eval {label} {mode}: rel_err {err:.3e} (bound {tol:.0e})")
                record(f"{cls} eval {label} {mode}", err / tol)
                assert err < tol
                assert not out.requires_grad and torch.equal(torch.cuda.get_rng_state(), rng0)
                for k, v in blk.state_dict().items():
                    assert same_bits(v, state0[k]), f"{k} changed in eval"


@pytest.mark.parametrize("name", ["resnetformer", "resnetb", "resconvnext"])
def test_eval_blocks_on_a_padded_cloud(amd, block_states, name):
    """300 rows around the fixture's points, NaN points, id -1 and features of 1e3 behind them, fp32 mode: the present rows
    within 5e-6 of the trimmed eval run (and of the restatement), the absent output rows zero."""
    rows = 300
    cls, d, entries = block_states[name]
    t = lambda k: dev(np.asarray(d[k]))
    n, f = d["pts"].shape[0], d["frames"].shape[1]

    def buf(v, fill):
        out = torch.full((rows * (v.shape[0] // n),) + tuple(v.shape[1:]), fill, dtype=v.dtype, device=DEV)
        out[:v.shape[0]] = v
        return out

    plain = amd.pc.PointcloudRotEquiv.from_frames(t("pts"), t("batch"), t("frames"))
    plain_nbh = amd.pc.BQNeighborhood(plain, plain, float(d["radius"]))
    frames = torch.eye(3, device=DEV).reshape(1, 1, 9).repeat(rows, f, 1)
    frames[:n] = t("frames")
    pc = amd.pc.PointcloudRotEquiv.from_frames(buf(t("pts"), float("nan")), buf(t("batch"), -1), frames, p_n_valid=word(n), num_batches=2,
                                               p_padded_rows=True)
    nbh = amd.pc.BQNeighborhood(pc, pc, float(d["radius"]), p_capacity=plain_nbh.num_edges() + 100)
    assert not nbh.overflowed()
    with precision(amd, "fp32"):
        for label, norm, state, want in entries:
            blk = eval_block(amd, cls, d, norm, state)
            with torch.no_grad():
                trimmed = blk(plain, t("x"), plain_nbh)
                out = blk(pc, buf(t("x"), 1e3), nbh)
            e_trim, e_ref = rel_err(out[:n * f], trimmed), E.rel_err(out[:n * f].cpu().numpy(), want)
            print(f"{cls} eval {label} padded: against trimmed {e_trim:.3e}, against the restatement {e_ref:.3e} (bound 5e-06)")
            record(f"{cls} eval {label} padded vs trimmed", e_trim / 5e-6)
            assert e_trim < 5e-6 and e_ref < 5e-6
            assert zero_bits(out[n * f:]), "absent output rows are zero"


def unet_scene(amd, n_el, seed):
    torch.manual_seed(seed)
    pts = torch.rand(n_el * 2, 3, device=DEV)
    bid = torch.arange(2, device=DEV, dtype=torch.int32).repeat_interleave(n_el)
    x = torch.randn(n_el * 2 * 2, 3, device=DEV)
    return pts, bid, x


def unet_hierarchy(amd, pts, bid, seed):
    torch.manual_seed(seed)                                  # (the frames are drawn from torch's generator)
    pc = amd.pc.PointcloudRotEquiv(pts, bid, {"pca": True, "n_frames": 2, "fixed_axis": False, "neigh_method": "knn",
                                              "neigh_kwargs": {"neigh_k": 16}})
    return amd.pc.PointHierarchyRotEquiv(pc, 2, "grid_avg", grid_radii=[0.08, 0.16])


def unet(amd):
    from test_gpu_network import MiniUNet
    torch.manual_seed(7)
    net = MiniUNet(amd, 3, [32, 64, 96], 5).to(DEV)
    for m in net.modules():
        if isinstance(m, amd.PNEConvLayerRotEquiv):
            m.norm_neigh_dist_.fill_(4.0), m.norm_num_neighs_.fill_(0.05)
    return net


RADII = [0.08, 0.16, 0.32]


def test_mini_unet_in_eval_and_across_scenes(amd):
    """No norm and no drop path: eval and train mean the same, so the logits under `eval()` + `no_grad` and under
    `inference_mode` are the training forward's by bits; and scene A, scene B (another point count), scene A again on the same
    module and cloud objects give A's bits twice, which are those of freshly built objects."""
    net = unet(amd)
    a_pts, a_bid, a_x = unet_scene(amd, 1500, 31)
    b_pts, b_bid, b_x = unet_scene(amd, 1100, 32)
    hier_a, hier_b = unet_hierarchy(amd, a_pts, a_bid, 41), unet_hierarchy(amd, b_pts, b_bid, 42)
    want = net.train()(hier_a, RADII, a_x).detach()
    state0 = {k: v.clone() for k, v in net.state_dict().items()}
    net.eval()
    with torch.no_grad():
        first = net(hier_a, RADII, a_x)
        other = net(hier_b, RADII, b_x)
        again = net(hier_a, RADII, a_x)
    with torch.inference_mode():
        inf = net(hier_a, RADII, a_x)
    assert same_bits(first, want), "eval + no_grad differs from the training forward"
    assert same_bits(inf, want), "inference_mode differs from the training forward"
    assert same_bits(again, first), "scene A after scene B differs from scene A before it"
    assert other.shape[0] == 2200 and bool(torch.isfinite(other).all())
    fresh_net = unet(amd).eval()
    with torch.no_grad():
        fresh = fresh_net(unet_hierarchy(amd, a_pts.clone(), a_bid.clone(), 41), RADII, a_x.clone())
        fresh_b = fresh_net(unet_hierarchy(amd, b_pts.clone(), b_bid.clone(), 42), RADII, b_x.clone())
    assert same_bits(fresh, first), "freshly built objects give other bits for scene A"
    assert same_bits(fresh_b, other), "freshly built objects give other bits for scene B"
    for k, v in net.state_dict().items():
        assert same_bits(v, state0[k]), f"{k} changed"


def test_eval_block_captured_on_a_padded_cloud_follows_the_row_count(amd, block_states):
    """The ResNetFormer fixture in `eval()` + `no_grad` on static buffers of 300 rows: cloud, neighbourhood and block captured
    once at the fixture's 220 points and replayed at 170 -- the eager result on the new count, zeros behind it.  The capture
    recipe is the one of test_gpu_padded_rows.py::test_a_whole_training_step_replays_as_one_graph."""
    rows, n2 = 300, 170
    cls, d, entries = block_states["resnetformer"]
    label, norm, state, _ = entries[0]
    t = lambda k: dev(np.asarray(d[k]))
    n, f = d["pts"].shape[0], d["frames"].shape[1]
    s_pts = torch.full((rows, 3), float("nan"), device=DEV)
    s_bid = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    s_frames = torch.eye(3, device=DEV).reshape(1, 1, 9).repeat(rows, f, 1)
    s_x = torch.full((rows * f, d["x"].shape[1]), 1e3, device=DEV)
    s_word = torch.zeros(1, dtype=torch.int32, device=DEV)
    s_pts[:n], s_bid[:n], s_frames[:n], s_x[:n * f] = t("pts"), t("batch"), t("frames"), t("x")
    held = {}
    with precision(amd, "fp32"):
        blk = eval_block(amd, cls, d, norm, state)
        state0 = {k: v.clone() for k, v in blk.state_dict().items()}

        def step():
            with torch.no_grad():
                pc = amd.pc.PointcloudRotEquiv.from_frames(s_pts, s_bid, s_frames, p_n_valid=s_word, num_batches=2, p_padded_rows=True)
                nbh = amd.pc.BQNeighborhood(pc, pc, float(d["radius"]), p_capacity=20000)
                held.update(out=blk(pc, s_x, nbh), nbh=nbh)

        s_word.fill_(n)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        held.clear()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            step()
        for count in (n, n2):
            s_word.fill_(count)
            graph.replay()
            torch.cuda.synchronize()
            assert not held["nbh"].overflowed()
            got = held["out"].clone()
            captured = dict(held)
            step()                                                  # eager, on the same buffers and count
            torch.cuda.synchronize()
            eager = held["out"]
            held.update(captured)
            pc_t = amd.pc.PointcloudRotEquiv.from_frames(s_pts[:count].clone(), s_bid[:count].clone(), s_frames[:count].clone(), num_batches=2)
            with torch.no_grad():
                trimmed = blk(pc_t, s_x[:count * f].clone(), amd.pc.BQNeighborhood(pc_t, pc_t, float(d["radius"])))
            e_eager, e_trim = rel_err(got[:count * f], eager[:count * f]), rel_err(got[:count * f], trimmed)
            print(f"captured eval block at {count} points: against eager {e_eager:.3e}, against trimmed {e_trim:.3e} (bound 5e-06)")
            record(f"captured eval block {count} vs trimmed", e_trim / 5e-6)
            assert e_eager < 5e-6 and e_trim < 5e-6
            assert zero_bits(got[count * f:]) and bool(torch.isfinite(got).all())
        for k, v in blk.state_dict().items():
            assert same_bits(v, state0[k]), f"{k} changed"


# ------------------------------------------------------------------------------------------------ (d) inference_mode
PCA = {"pca": True, "n_frames": 2, "fixed_axis": False, "neigh_method": "knn", "neigh_kwargs": {"neigh_k": 16}}


def build_everything(amd, pts_cpu, bid_cpu, x_cpu, conv, r):
    """Cloud with PCA frames, hierarchy, the three neighbourhoods and a convolution, from tensors created HERE (inside whatever
    mode the caller set)."""
    torch.manual_seed(3)                                          # (the frame shuffle draws from torch's generator)
    pts, bid, x = pts_cpu.to(DEV), bid_cpu.to(DEV), x_cpu.to(DEV)
    pc = amd.pc.PointcloudRotEquiv(pts, bid, PCA)
    hier = amd.pc.PointHierarchyRotEquiv(pc, 1, "grid_avg", grid_radii=[0.1])
    bq = amd.pc.BQNeighborhood(pc, pc, r)
    bounded = amd.pc.BQNeighborhood(pc, pc, r, p_capacity=bq.num_edges() + 64)
    knn = amd.pc.KnnNeighborhood(pc, pc, 8)
    down = hier.create_neighborhood(0, 1, "ball_query", bq_radius=0.2)
    out = conv(p_pc_in=pc, p_pc_out=pc, p_in_features=x, p_neighborhood=bq)
    out_bounded = conv(p_pc_in=pc, p_pc_out=pc, p_in_features=x, p_neighborhood=bounded)
    e = bounded.num_edges()
    return {"frames": pc.local_frames_, "level1": hier.pcs_[1].pts_, "level1_frames": hier.pcs_[1].local_frames_,
            "bq": bq.neighbors_, "bq_ends": bq.start_ids_, "bounded": canon_edges(bounded.neighbors_[:e]), "bounded_ends": bounded.start_ids_,
            "knn": knn.neighbors_, "knn_ends": knn.start_ids_, "down": down.neighbors_, "down_ends": down.start_ids_,
            "out": out, "out_bounded": out_bounded}, pc


def test_everything_builds_inside_inference_mode(amd):
    """3000 points: past the size at which the ball query sorts the source cloud into a cell grid, so the per-cloud caches
    (boxes, grids, k-NN table, geometry records) are all on the path.  Before the caches stopped reading `_version` of an
    inference tensor, the first neighbourhood build raised "Inference tensors do not track version counter"."""
    n = 3000
    assert amd.ops.ball_query_needs_grid(n)
    pts, bid, _ = small_scene(amd, n, 51)
    x = torch.randn(n * 2, 16, generator=torch.Generator().manual_seed(1))
    r = O.radius_for_degree(n / 2, 12)
    torch.manual_seed(9)
    conv = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu").create_conv_layer(16, 24).to(DEV).eval()
    conv.norm_neigh_dist_.fill_(1.0 / r), conv.norm_num_neighs_.fill_(0.08)
    with torch.no_grad():
        want, _ = build_everything(amd, pts, bid, x, conv, r)
    with torch.inference_mode():
        got, pc = build_everything(amd, pts, bid, x, conv, r)
        assert pc.pts_.is_inference() and got["out"].is_inference()
        again, _ = build_everything(amd, pts, bid, x, conv, r)
    for k in want:
        assert same_bits(got[k], want[k]), f"{k}: inference_mode differs from no_grad"
        assert same_bits(again[k], want[k]), f"{k}: the second build inside inference_mode differs"
    assert float(want["out"].abs().max()) > 0 and want["bq"].shape[0] > n


def test_in_place_update_of_an_inference_cloud_reaches_every_cache(amd):
    """`pts_.copy_(other)` on a cloud created inside `inference_mode` leaves no version to notice: nothing may be cached on such
    a tensor.  The next neighbourhoods (plain, capacity-bounded, k-NN) and convolutions are those of freshly built objects."""
    n = 3000
    pts, bid, frames = small_scene(amd, n, 52)
    other = small_scene(amd, n, 53)[0]
    x = torch.randn(n * 2, 16, generator=torch.Generator().manual_seed(2))
    r = O.radius_for_degree(n / 2, 12)
    torch.manual_seed(9)
    conv = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu").create_conv_layer(16, 24).to(DEV).eval()
    conv.norm_neigh_dist_.fill_(1.0 / r), conv.norm_num_neighs_.fill_(0.08)

    def results(pc, xd):
        bq = amd.pc.BQNeighborhood(pc, pc, r)
        bounded = amd.pc.BQNeighborhood(pc, pc, r, p_capacity=bq.num_edges() + 64)
        ids = pc._self_knn_ids(8)
        e = bounded.num_edges()
        return {"bq": bq.neighbors_, "bq_ends": bq.start_ids_, "bounded": canon_edges(bounded.neighbors_[:e]), "bounded_ends": bounded.start_ids_,
                "knn_ids": ids, "aabb_min": pc.aabb()[0], "aabb_max": pc.aabb()[1],
                "out": conv(p_pc_in=pc, p_pc_out=pc, p_in_features=xd, p_neighborhood=bq),
                "out_bounded": conv(p_pc_in=pc, p_pc_out=pc, p_in_features=xd, p_neighborhood=bounded)}

    with torch.inference_mode():
        xd = x.to(DEV)
        pc = amd.pc.PointcloudRotEquiv.from_frames(pts.to(DEV), bid.to(DEV), frames.to(DEV))
        before = results(pc, xd)
        pc.pts_.copy_(other.to(DEV))
        after = results(pc, xd)
        fresh = results(amd.pc.PointcloudRotEquiv.from_frames(other.to(DEV), bid.to(DEV), frames.to(DEV)), xd)
    with torch.no_grad():
        ordinary = results(amd.pc.PointcloudRotEquiv.from_frames(other.to(DEV), bid.to(DEV), frames.to(DEV)), x.to(DEV))
    assert not same_bits(before["out"], after["out"])
    for k in fresh:
        assert same_bits(after[k], fresh[k]), f"{k}: stale after an in-place update of an inference tensor"
        assert same_bits(after[k], ordinary[k]), f"{k}: differs from the no_grad build on ordinary tensors"


def test_version_key_of_ordinary_and_inference_tensors(amd):
    ops = amd.ops
    t = torch.zeros(3, device=DEV)
    assert ops.version_key(t) == t._version == ops.version_key(t)
    t.add_(1)
    assert ops.version_key(t) == t._version == 1
    with torch.inference_mode():
        u = torch.zeros(3, device=DEV)
        with pytest.raises(RuntimeError, match="version counter"):
            u._version
        assert ops.version_key(u) != ops.version_key(u)           # equal to nothing: never a cache hit


def test_zz_error_ratios_of_this_session():
    """Prints the largest observed / bound per entry (what profiles/eval_path.txt records); every one was asserted above."""
    print({k: round(v, 3) for k, v in RATIOS.items()})
    assert all(v <= 1.0 for v in RATIOS.values())
