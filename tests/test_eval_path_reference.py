"""CPU: the float64 restatement of the evaluation forms (tests/eval_path_reference.py) is pinned to the reference's own
Python in its training form, its planted faults move the eval-form output of every block they touch by more than ten times
the bound the GPU test holds the library to, and its float32 emulation stays inside the per-element bounds taken from it."""
import numpy as np
import pytest

import eval_path_reference as E

# rel_err of the training-form restatement against `out` (and, for the first, the `after/` running statistics) of the
# fixtures, as measured (profiles/eval_path.txt): the float32 fixture's own rounding is the only error source.  Asserted at
# 4 x these, and never above the bound the fp32 kernel mode meets against the same fixtures (test_gpu_network.py).
OBSERVED = {"resnetformer": 1.32e-07, "resnetb": 8.07e-08, "resconvnext": 1.50e-07}
OBSERVED_AFTER = {"norm_1_.layer_.running_mean": 1.16e-07, "norm_1_.layer_.running_var": 3.53e-08,
                  "norm_2_.layer_.running_mean": 9.97e-08, "norm_2_.layer_.running_var": 3.26e-08}
FP32_BOUND = 5e-6     # test_gpu_network.py / test_gpu_group_norm_blocks.py: the fp32 mode against the fixtures
FAULT_FLOOR = 10 * FP32_BOUND


@pytest.fixture(scope="module")
def states():
    return {name: E.eval_states(name) for name in OBSERVED}


@pytest.mark.parametrize("name", list(OBSERVED))
def test_training_form_reproduces_the_reference_fixture(name):
    cls, state, geom, d = E.fixture(name)
    out, after = E.block_forward(cls, state, geom, d["x"], norm="batch" if cls == "ResNetFormer" else "group", train=True)
    err = E.rel_err(out, d["out"])
    print(f"{name}: out rel_err {err:.3e} (observed {OBSERVED[name]:.2e}, asserted at 4 x)")
    assert 4 * OBSERVED[name] <= FP32_BOUND
    assert err <= 4 * OBSERVED[name]
    if cls == "ResNetFormer":
        assert sorted(after) == sorted(OBSERVED_AFTER)
        for k, v in after.items():
            e = E.rel_err(v, d["after/" + k])
            print(f"    after/{k}: rel_err {e:.3e} (observed {OBSERVED_AFTER[k]:.2e})")
            assert e <= 4 * OBSERVED_AFTER[k] <= FP32_BOUND, k


def _touched(norm, label, fault):
    """Whether `fault` changes what a block in this state computes: a group norm has neither statistics nor eps of the batch
    norm; with the `after/` statistics (variances near 1) a dropped eps of 1e-5 moves the output by 2e-6, below any bound
    -- it is asserted on the drawn statistics."""
    if fault in E.BN_FAULTS:
        return norm == "batch" and not (fault == "no_eps" and label == "after")
    return True


@pytest.mark.parametrize("fault", E.FAULTS)
@pytest.mark.parametrize("name", list(OBSERVED))
def test_planted_fault_moves_the_eval_output(states, name, fault):
    """drop_prob 0.1 as in the GPU test.  The floor is 10 x the fp32 mode's bound, the sharpest of the GPU test's three; the
    figure against the split-bf16 modes' bound (5e-5) is printed beside it."""
    cls, geom, d, entries = states[name]
    asserted = 0
    for label, norm, state in entries:
        if not _touched(norm, label, fault):
            continue
        if fault == "biased_running_var":
            # a training step from `state` with the faulty update, then eval on what it left, against the same with the right one
            base = E.fixture(name)[1] if label == "after" else state
            got = E.block_forward(cls, E.after_training_step(cls, base, geom, d["x"], fault), geom, d["x"], norm, drop_prob=0.1)[0]
            ref = E.block_forward(cls, E.after_training_step(cls, base, geom, d["x"]), geom, d["x"], norm, drop_prob=0.1)[0]
        else:
            ref = E.block_forward(cls, state, geom, d["x"], norm, drop_prob=0.1)[0]
            got = E.block_forward(cls, state, geom, d["x"], norm, drop_prob=0.1, fault=fault)[0]
        moved = E.rel_err(got, ref)
        print(f"{cls} {label} {fault}: moves out by {moved:.3e} = {moved / FP32_BOUND:.0f} x the fp32 bound, "
              f"{moved / 5e-5:.1f} x the split-bf16 bound")
        assert moved > FAULT_FLOOR, (cls, label, fault, moved)
        asserted += 1
    # every block meets every fault at least once (its batch-norm form with drawn statistics), the skip's faults in every state
    assert asserted >= (1 if fault in E.BN_FAULTS else len(entries))


def test_after_statistics_sit_far_from_the_batch_statistics():
    """One step at momentum 0.2 from (0, 1): every channel of the fixture's `after/` statistics differs from the batch's own
    by far more than the bound, so eval on batch statistics cannot pass for eval on running ones."""
    cls, state, geom, d = E.fixture("resnetformer")
    inputs = {}
    E.block_forward(cls, state, geom, d["x"], train=True, norm_inputs=inputs)
    for name, (mu, var, _) in inputs.items():
        rm, rv = d[f"after/{name}.layer_.running_mean"], d[f"after/{name}.layer_.running_var"]
        sigma_shift = np.abs(np.sqrt(rv + E.EPS) / np.sqrt(var + E.EPS) - 1.0)
        mean_shift = np.abs(rm - mu) / np.sqrt(var)
        print(f"{name}: smallest sigma shift {sigma_shift.min():.3e}, smallest mean shift {mean_shift.min():.3e}")
        assert (np.maximum(sigma_shift, mean_shift) > 100 * FAULT_FLOOR).all(), name


def test_emulation_stays_within_its_bounds():
    bounds, worst = E.bounds(), E.emulated_max()
    print("emulated max", worst, "bounds", bounds)
    for k in ("bn_eval", "skip_eval"):
        assert 0.0 < worst[k] <= bounds[k] < 64 * 2.0 ** -24, k   # a handful of float32 roundings, not a loose figure
    # per element, on every shape of the GPU test
    for rows in E.BOUND_ROWS:
        for c in E.BOUND_CHANNELS:
            d = E.bn_bounds_case(rows, c, 1000 * rows + c)
            ref, scale, rm, rv = E.batch_norm(**d)
            assert (np.abs(E.batch_norm(**d, T=E.F)[0] - ref) <= bounds["bn_eval"] * scale).all(), (rows, c)
            assert np.array_equal(rm, d["running_mean"]) and np.array_equal(rv, d["running_var"])   # eval updates nothing
            s = E.skip_bounds_case(rows, c, 2000 * rows + c)
            ref, scale = E.skip(**s)
            assert (np.abs(E.skip(**s, T=E.F)[0] - ref) <= bounds["skip_eval"] * scale).all(), (rows, c)
            for p in (0.0, 0.4):
                assert np.array_equal(E.skip(**s, drop_prob=p)[0], ref)      # eval: drop_prob changes nothing
    # and the planted faults leave them
    d = E.bn_bounds_case(257, 24, 1)
    ref, scale, _, _ = E.batch_norm(**d)
    for fault in ("batch_stats",):
        assert E.worst(E.batch_norm(**d, fault=fault)[0], ref, scale) > 10 * bounds["bn_eval"]
    s = E.skip_bounds_case(257, 24, 2)
    ref, scale = E.skip(**s)
    for fault in ("keep_factor", "no_gamma"):
        assert E.worst(E.skip(**s, drop_prob=0.4, fault=fault)[0], ref, scale) > 10 * bounds["skip_eval"]


def test_cache_keys_never_read_the_version_of_an_inference_tensor():
    """The per-cloud caches key on `ops.version_key`: the version counter of an ordinary tensor, and for a tensor created under
    `torch.inference_mode()` -- which has none, and can change in place without a trace -- an object equal to nothing, so that
    every cache carrying it rebuilds.  Before, the first key built inside `inference_mode` raised "Inference tensors do not
    track version counter" (CPU tensors suffice: the keys are built before any library call)."""
    import torch

    from se3conv3d_amd import layers, ops, pc

    t = torch.zeros(4, 3)
    assert ops.version_key(t) == t._version == 0
    t.add_(1)
    assert ops.version_key(t) == t._version == 1
    with torch.inference_mode():
        pts, bid, frames = torch.rand(5, 3), torch.zeros(5, dtype=torch.int32), torch.eye(3).reshape(1, 1, 9).repeat(5, 1, 1)
        with pytest.raises(RuntimeError, match="version counter"):
            pts._version
        assert ops.version_key(pts) != ops.version_key(pts)
        word = torch.ones(1, dtype=torch.int32)
        assert ops.SourceGrids.key(pts, bid, 1, word) != ops.SourceGrids.key(pts, bid, 1, word)
        rec = ops.PreparedRecords().bind(pts, frames)
        rec.mark_filled(None)
        assert rec.filled_for(None) and not rec.bind(pts, frames).filled_for(None)      # bound again: rebuilt
        copies = [[pts, pts.clone(), ops.version_key(pts)]]
        pts.mul_(2)
        geom = type("G", (), {"pts_out": pts})()
        layers._refresh_copies(geom, copies)
        assert torch.equal(copies[0][1], pts)                                        # the in-place update reached the copy
    # ordinary tensors: the same key twice, another after an in-place update -- as before
    pts, bid, frames = torch.rand(5, 3), torch.zeros(5, dtype=torch.int32), torch.eye(3).reshape(1, 1, 9).repeat(5, 1, 1)
    key = ops.SourceGrids.key(pts, bid, 1)
    assert key == ops.SourceGrids.key(pts, bid, 1)
    rec = ops.PreparedRecords().bind(pts, frames)
    rec.mark_filled(None)
    assert rec.bind(pts, frames).filled_for(None)
    pts.add_(1)
    assert key != ops.SourceGrids.key(pts, bid, 1) and not rec.bind(pts, frames).filled_for(None)
    assert pc.Pointcloud.aabb.__code__.co_names.count("_version") == 0 and "version_key" in pc.Pointcloud.aabb.__code__.co_names


@pytest.mark.parametrize("mode", ["no_grad", "inference_mode"])
def test_pre_process_pass_leaves_buffers_autograd_can_save(mode):
    """The EMA update of `IConvLayer.forward` rebinds the two buffers.  Inside a caller's `inference_mode` block the new tensors
    would be inference tensors ("Inference tensors cannot be saved for backward" in the next training step): the update runs
    with inference mode switched off.  A stub convolution on the CPU: the update is plain torch."""
    import types

    import torch

    from oracle import se3conv_oracle as O
    from se3conv3d_amd import layers

    class Stub(layers.IConvLayer):
        def __compute_convolution__(self, p_pc_in, p_pc_out, p_in_features, p_neighborhood):
            return p_in_features * self.norm_neigh_dist_ * self.norm_num_neighs_

    conv = Stub(3, 4, 4)
    pc = types.SimpleNamespace(pts_=torch.rand(6, 3))
    nb = torch.tensor([[0, 1], [0, 2], [1, 0], [3, 4], [5, 5]])
    ball = types.SimpleNamespace(radius_=0.25, neighbors_=nb, start_ids_=torch.zeros(6, dtype=torch.int32))
    knn = types.SimpleNamespace(neighbors_=nb[:4], start_ids_=torch.zeros(6, dtype=torch.int32))
    conv.start_pre_process()
    conv.eval()
    with getattr(torch, mode)():
        conv(pc, pc, torch.ones(6, 4), ball)
        rho, nu = O.ema_update(torch.tensor(0.0), torch.tensor(0.0), 0.25, 6, 5)
        assert float(conv.norm_neigh_dist_) == float(rho) and float(conv.norm_num_neighs_) == float(nu)
        conv(pc, pc, torch.ones(6, 4), knn)
        mean_len = float((pc.pts_[nb[:4, 1]] - pc.pts_[nb[:4, 0]]).norm(dim=1).mean())
        rho, nu = O.ema_update(rho, nu, 2.0 * mean_len, 6, 4)
        assert float(conv.norm_neigh_dist_) == pytest.approx(float(rho), rel=1e-6) and float(conv.norm_num_neighs_) == float(nu)
    conv.end_pre_process()
    assert not conv.norm_neigh_dist_.is_inference() and not conv.norm_num_neighs_.is_inference()
    assert sorted(conv.state_dict()) == ["norm_neigh_dist_", "norm_num_neighs_"]
    x = torch.ones(6, 4, requires_grad=True)
    conv.train()(pc, pc, x, ball).sum().backward()          # (the product saves the buffers for backward)
    assert x.grad is not None
