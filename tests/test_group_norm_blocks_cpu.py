"""CPU: the torch formulation of `blocks.GroupNormPC` against the reference's fixture (tests/golden/group_norm.npz), and the
glue of `blocks.ResNetB` / `blocks.ResConvNeXt` around a CPU stand-in of the convolution (the oracle) against the reference's
blocks with `GroupNormPC` as the norm layer (tests/golden/resnetb_block.npz, resconvnext_block.npz) -- in the manner of
test_oracle_golden.py::test_resnetformer_block_glue_matches_reference_fixture."""
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_err
from oracle import se3conv_oracle as O
from se3conv3d_amd import blocks


@pytest.mark.parametrize("c,groups", [(16, 8), (24, 4), (8, 8)])
def test_torch_form_of_group_norm_matches_the_reference_fixture(c, groups):
    d = np.load(os.path.join(GOLDEN, "group_norm.npz"))
    p = f"c{c}_g{groups}/"
    t = lambda k: torch.from_numpy(np.asarray(d[k]))
    norm = blocks.GroupNormPC(c, groups)
    assert sorted(norm.state_dict()) == ["betas_", "gamma_"] and norm.num_groups_ == groups and norm.num_feats_ == c
    res = norm.load_state_dict({"gamma_": t(p + "gamma"), "betas_": t(p + "betas")}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    pc = types.SimpleNamespace(batch_size_=torch.tensor(3), batch_ids_=t("batch"))
    x = t(p + "x").requires_grad_(True)
    y = norm(x, pc)
    y.backward(t(p + "g"))
    for name, got in (("y", y), ("dx", x.grad), ("dgamma", norm.gamma_.grad), ("dbetas", norm.betas_.grad)):
        assert rel_err(got.reshape(-1), t(p + name).reshape(-1)) <= 2e-5, name


def test_group_norm_refuses_what_it_cannot_divide():
    with pytest.raises(ValueError, match="multiple"):
        blocks.GroupNormPC(20, 8)


@pytest.mark.parametrize("name,cls", [("resnetb", "ResNetB"), ("resconvnext", "ResConvNeXt")])
def test_block_glue_matches_the_reference_fixture(name, cls):
    path = os.path.join(GOLDEN, f"{name}_block.npz")
    assert os.path.getsize(path) < os.path.getsize(os.path.join(GOLDEN, "resnetformer_block.npz")) // 2
    d = np.load(path)
    t = lambda k: torch.from_numpy(np.asarray(d[k]))
    pts, frames, bid = t("pts"), t("frames"), t("batch")
    nb, _ = O.ball_query(pts, pts, bid, bid, float(d["radius"]))

    class OracleConv(torch.nn.Module):  # same parameter / buffer names as the layer
        def __init__(self, c_in, c_out):
            super().__init__()
            self.proj_axes_ = torch.nn.Parameter(torch.zeros(9, 32))
            self.proj_biases_ = torch.nn.Parameter(torch.zeros(32))
            self.conv_weights_ = torch.nn.Parameter(torch.zeros(c_in, 32, c_out))
            self.register_buffer("norm_neigh_dist_", torch.tensor(0.0))
            self.register_buffer("norm_num_neighs_", torch.tensor(0.0))

        def forward(self, p_pc_in, p_pc_out, p_in_features, p_neighborhood):
            return O.conv_forward(pts, pts, frames, frames, nb, p_in_features, self.proj_axes_, self.proj_biases_,
                                  self.conv_weights_, self.norm_neigh_dist_, self.norm_num_neighs_)

    factory = types.SimpleNamespace(create_conv_layer=lambda ci, co: OracleConv(ci, co))
    blk = getattr(blocks, cls)(16, 24, factory, blocks.GroupNormPC, 0.0)
    for attr in ("norm_", "linear_1_", "linear_2_", "spatial_conv_", "skip_path_", "skip_conv_"):
        assert hasattr(blk, attr), attr
    state = {k[len("state/"):]: t(k) for k in d.files if k.startswith("state/")}
    res = blk.load_state_dict(state, strict=True)  # the reference's keys, one for one
    assert not res.missing_keys and not res.unexpected_keys
    blk.train()
    pc = types.SimpleNamespace(batch_size_=torch.tensor(2), batch_ids_=bid)
    x = t("x").requires_grad_(True)
    out = blk(pc, x, None)
    out.backward(t("g"))
    assert rel_err(out, t("out")) < 5e-6 and rel_err(x.grad, t("dx")) < 5e-6
    for pname, p in blk.named_parameters():
        assert rel_err(p.grad, t("grad/" + pname)) < 2e-5, pname
