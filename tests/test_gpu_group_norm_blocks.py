"""GPU: `blocks.ResNetB` and `blocks.ResConvNeXt` with `GroupNormPC` as their norm layer against the reference's own blocks
(tests/golden/resnetb_block.npz, resconvnext_block.npz: state_dict, input, output and all gradients from the reference's
Python) -- the state_dict loads key for key, output and gradients hold the tolerance of
test_gpu_network.py::test_reference_resnetformer_block_runs_unchanged in every arithmetic mode -- and the same blocks on a
`p_padded_rows` cloud against the run on the trimmed one."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_err
from padded_cases import DEV, word

pytestmark = pytest.mark.gpu
BLOCKS = [("resnetb", "ResNetB"), ("resconvnext", "ResConvNeXt")]
MODES = (("fp32", 5e-6), ("bf16x3", 5e-5), ("bf16x3_t16", 5e-5))


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd as amd
    return amd


def in_buffer(t, rows, value=float("nan")):
    out = torch.full((rows,) + tuple(t.shape[1:]), value, dtype=t.dtype, device=DEV)
    out[:t.shape[0]] = t
    return out


def loaded(amd, cls, d, t):
    blk = getattr(amd, cls)(16, 24, amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu"), amd.GroupNormPC, 0.0).to(DEV)
    state = {k[len("state/"):]: t(k) for k in d.files if k.startswith("state/")}
    res = blk.load_state_dict(state, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return blk.train()


@pytest.mark.parametrize("name,cls", BLOCKS)
def test_reference_block_with_group_norm_runs_unchanged(amd, name, cls):
    d = np.load(os.path.join(GOLDEN, f"{name}_block.npz"))
    t = lambda k: torch.from_numpy(np.asarray(d[k])).to(DEV)
    pc = amd.pc.PointcloudRotEquiv.from_frames(t("pts"), t("batch"), t("frames"))
    nbh = amd.pc.BQNeighborhood(pc, pc, float(d["radius"]))
    prev = amd.get_precision()
    try:
        for precision, tol in MODES:
            amd.set_precision(precision)
            blk = loaded(amd, cls, d, t)
            x = t("x").requires_grad_(True)
            out = blk(pc, x, nbh)
            out.backward(t("g"))
            e_out, e_dx = rel_err(out, t("out")), rel_err(x.grad, t("dx"))
            print(f"{cls} {precision}: out {e_out:.3e} dx {e_dx:.3e} (bound {tol:.0e})")
            assert e_out < tol and e_dx < tol
            for pname, p in blk.named_parameters():
                e = rel_err(p.grad, t("grad/" + pname))
                print(f"    {pname}: {e:.3e} (bound {4 * tol:.0e})")
                assert e < 4 * tol, (precision, pname)
    finally:
        amd.set_precision(prev)


@pytest.mark.parametrize("name,cls", BLOCKS)
def test_block_on_a_padded_cloud_equals_the_trimmed_run(amd, name, cls):
    """Buffers of 300 rows around the fixture's 200 points, NaN points, id -1 and features of 1000 behind them: output and gradients are the
    trimmed run's at the present rows, to fp32 rounding (the dense products cut 300 rows into other pieces than 200, the padded
    query lists a point's edges in another order), and zero behind them."""
    rows = 300
    d = np.load(os.path.join(GOLDEN, f"{name}_block.npz"))
    t = lambda k: torch.from_numpy(np.asarray(d[k])).to(DEV)
    n = d["pts"].shape[0]
    plain = amd.pc.PointcloudRotEquiv.from_frames(t("pts"), t("batch"), t("frames"))
    plain_nbh = amd.pc.BQNeighborhood(plain, plain, float(d["radius"]))
    frames = torch.eye(3, device=DEV).reshape(1, 1, 9).repeat(rows, 1, 1)
    frames[:n] = t("frames")
    pc = amd.pc.PointcloudRotEquiv.from_frames(in_buffer(t("pts"), rows), in_buffer(t("batch"), rows, -1), frames, p_n_valid=word(n),
                                               num_batches=2, p_padded_rows=True)
    nbh = amd.pc.BQNeighborhood(pc, pc, float(d["radius"]), p_capacity=plain_nbh.num_edges() + 100)
    assert not nbh.overflowed()
    prev = amd.get_precision()
    try:
        amd.set_precision("fp32")
        blk = loaded(amd, cls, d, t)
        x = t("x").requires_grad_(True)
        want = blk(plain, x, plain_nbh)
        want.backward(t("g"))
        want_grads = {k: p.grad.clone() for k, p in blk.named_parameters()}
        blk.zero_grad()
        # finite absent features, as blocks.py asks of a network's input: the linear skip of these blocks reads the block's
        # input itself, and its weight gradient multiplies every row by the (zero) gradient row
        xp = in_buffer(t("x"), rows, 1e3).requires_grad_(True)
        out = blk(pc, xp, nbh)
        out.backward(in_buffer(t("g"), rows, 0.0))                        # (the loss ignores absent rows)
        e_out, e_dx = rel_err(out[:n], want), rel_err(xp.grad[:n], x.grad)
        print(f"{cls} padded against trimmed: out {e_out:.3e} dx {e_dx:.3e}")
        assert e_out < 5e-6 and e_dx < 5e-6
        assert bool((out[n:] == 0).all()) and bool((xp.grad[n:] == 0).all())
        for k, p in blk.named_parameters():
            assert rel_err(p.grad, want_grads[k]) < 2e-5, k
        assert rel_err(out[:n], t("out")) < 5e-6 and rel_err(xp.grad[:n], t("dx")) < 5e-6
        with pytest.raises(NotImplementedError, match=cls):
            blk(pc, xp.detach().double(), nbh)
    finally:
        amd.set_precision(prev)
