"""CPU, no library call: the constructor surface of `layers.MultiHeadAttLayer` and `layers.LoRAttConvLayer` -- state-dict keys,
shapes and sigma against the reference's (tests/golden/attention_layer_keys.json, written by tools/gen_golden.py from the
reference's own constructors), the init bounds, the kernel points as a rotation of the scaled set, the refusals and the
factories' `update_parameters` with the reference's `elif` chain."""
import json
import math
import os

import numpy as np
import pytest
import torch

import se3conv3d_amd as amd
from conftest import GOLDEN
from se3conv3d_amd import layers

with open(os.path.join(GOLDEN, "attention_layer_keys.json")) as fh:
    KEYS = json.load(fh)
FACTORIES = {"mha": "MultiHeadAttLayerFactory", "lora": "LoRAttConvLayerFactory"}
CLASSES = {"mha": "MultiHeadAttLayer", "lora": "LoRAttConvLayer"}


def test_what_failed_before_the_feature():
    """Both factories exist and construct their layers (on the parent commit `amd.MultiHeadAttLayerFactory` is an AttributeError)."""
    a = amd.MultiHeadAttLayerFactory(3, 16, "single", 2).create_conv_layer(8, 24)
    b = amd.LoRAttConvLayerFactory(3, 16, "double", 4).create_conv_layer(8, 24)
    assert type(a) is amd.MultiHeadAttLayer and type(b) is amd.LoRAttConvLayer
    assert isinstance(a, amd.IConvLayer) and isinstance(b, amd.IConvLayer)


def test_state_dict_keys_shapes_and_sigma_are_the_reference_s():
    assert sorted(KEYS) == sorted(f"{a}/{r}" for a in FACTORIES for r in ("single", "double"))
    for name, ref in KEYS.items():
        layer, res = name.split("/")
        fact = getattr(amd, FACTORIES[layer])(3, 16, res, 2)
        conv = fact.create_conv_layer(8, 24)
        assert type(conv).__name__ == CLASSES[layer] and fact.conv_list_ == [conv]
        assert {k: list(v.shape) for k, v in conv.state_dict().items()} == ref["state"], name
        assert conv.kp_sigma_ == ref["sigma"] == {"single": 0.3, "double": 0.16}[res]
        assert (conv.num_basis_, conv.kp_res_, conv.num_heads_, conv.value_size_) == (16, res, 2, 8)
        assert tuple(conv.kernel_pts_.shape) == ({"single": 13, "double": 55}[res], 3) and tuple(conv.pe_.shape) == (1, 16, 8)
        assert ("conv_weights_" in ref["state"]) == (layer == "lora")
        # a checkpoint with the reference's keys loads strictly
        conv.load_state_dict({k: torch.full(shape, 0.25) for k, shape in ref["state"].items()}, strict=True)
        assert float(conv.pe_.detach().min()) == 0.25 and float(conv.norm_num_neighs_) == 0.25


def test_init_bounds_and_dtypes():
    torch.manual_seed(3)
    for layer, res, n_kp in (("mha", "single", 13), ("lora", "double", 55)):
        conv = getattr(amd, FACTORIES[layer])(3, 64, res, 4).create_conv_layer(32, 40)
        within = lambda p, bound, frac=0.9: p.detach().abs().max() <= bound and p.detach().abs().max() > frac * bound
        assert within(conv.proj_axes_, math.sqrt(1.0 / n_kp)) and within(conv.pe_, math.sqrt(1.0 / 32))
        assert not conv.proj_biases_.detach().any()
        assert within(conv.linear_kqv_.weight, math.sqrt(1.0 / 32)) and within(conv.linear_kqv_.bias, math.sqrt(1.0 / 32), 0.7)
        assert within(conv.w_out_.weight, math.sqrt(1.0 / 32)) and tuple(conv.w_out_.weight.shape) == (40, 32)
        assert tuple(conv.linear_kqv_.weight.shape) == (96, 32)
        if layer == "lora":
            assert within(conv.conv_weights_, math.sqrt(1.0 / (32 * 64))) and tuple(conv.conv_weights_.shape) == (64, 32, 40)
        assert all(p.dtype == torch.float32 for p in conv.state_dict().values()) and all(p.requires_grad for p in conv.parameters())
        assert not conv.kernel_pts_.requires_grad and "kernel_pts_" in dict(conv.named_buffers())
        assert float(conv.norm_neigh_dist_) == 0 and float(conv.norm_num_neighs_) == 0


@pytest.mark.parametrize("res", ["single", "double"])
def test_kernel_points_are_a_rotation_of_the_scaled_set(res):
    base = layers.kernel_points({"single": "kp_gauss", "double": "kp_gauss_double"}[res])
    double = res == "double"
    radii = np.linalg.norm(base, axis=1)
    assert np.allclose(radii[:12], 0.35 if double else 0.6, atol=1e-12) and (not double or np.allclose(radii[12:54], 0.7, atol=1e-12))
    assert not base[-1].any()
    torch.manual_seed(11)
    a = amd.MultiHeadAttLayerFactory(3, 8, res, 1).create_conv_layer(4, 4).kernel_pts_.double().numpy()
    b = amd.LoRAttConvLayerFactory(3, 8, res, 1).create_conv_layer(4, 4).kernel_pts_.double().numpy()
    assert np.abs(a - b).max() > 0.05, "every layer draws its own rotation"
    for kp in (a, b):
        assert np.abs(kp @ kp.T - base @ base.T).max() < 1e-6
        rot = np.linalg.lstsq(base, kp, rcond=None)[0]
        assert np.abs(rot.T @ rot - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(rot) - 1) < 1e-6
        assert np.abs(base @ rot - kp).max() < 1e-6
    torch.manual_seed(11)
    again = amd.MultiHeadAttLayerFactory(3, 8, res, 1).create_conv_layer(4, 4).kernel_pts_.double().numpy()
    assert np.array_equal(again, a), "the rotation comes from torch's generator"


@pytest.mark.parametrize("layer", ["mha", "lora"])
def test_refusals(layer):
    make = lambda dims, k, res, heads, c_in=8: getattr(amd, FACTORIES[layer])(dims, k, res, heads).create_conv_layer(c_in, 24)
    with pytest.raises(ValueError, match="kernel-point resolution"):
        make(3, 16, "triple", 2)
    with pytest.raises(ValueError, match="heads do not divide"):
        make(3, 16, "single", 3)
    with pytest.raises(ValueError, match=r"\{8, 16, 32, 64\}"):
        make(3, 12, "single", 2)
    with pytest.raises(NotImplementedError, match="3-D"):
        make(2, 16, "single", 2)

    class Cloud:
        pts_ = torch.zeros(4, 3)

    class Bounded:
        edge_info_ = torch.zeros(2)

    conv = make(3, 16, "single", 2)
    with pytest.raises(AssertionError, match="same object"):          # the reference asserts p_pc_in == p_pc_out
        conv(Cloud(), Cloud(), torch.zeros(4, 8), None)
    pc = Cloud()
    with pytest.raises(NotImplementedError, match="a capacity-bounded neighbourhood .* cannot feed the materialised path"):
        conv(pc, pc, torch.zeros(4, 8), Bounded())
    with pytest.raises(ValueError, match="no CPU fallback"):           # CPU tensors raise, like every other op
        amd.ops.BasisAttention.apply(torch.zeros(2, 4, 8), torch.zeros(2, 2), torch.zeros(8, 2), 1)


@pytest.mark.parametrize("layer", ["mha", "lora"])
def test_update_parameters_applies_the_first_key_present_only(layer):
    """The reference's `elif` chain (MultiHeadAttLayer.py:183-188): num_basis, else kp_res, else num_heads."""
    fact = getattr(amd, FACTORIES[layer])(3, 16, "single", 2)
    fact.update_parameters(num_basis=32, kp_res="double", num_heads=4, something_else=1)
    assert (fact.num_basis_, fact.kp_res_, fact.num_heads_) == (32, "single", 2)
    fact.update_parameters(kp_res="double", num_heads=4)
    assert (fact.num_basis_, fact.kp_res_, fact.num_heads_) == (32, "double", 2)
    fact.update_parameters(num_heads=4)
    assert (fact.num_basis_, fact.kp_res_, fact.num_heads_) == (32, "double", 4)
    fact.update_parameters(something_else=1)
    conv = fact.create_conv_layer(8, 24)
    assert (conv.num_basis_, conv.kp_res_, conv.num_heads_) == (32, "double", 4) and tuple(conv.proj_axes_.shape) == (55, 32)
    assert fact.conv_list_ == [conv] and fact.dims_ == 3
