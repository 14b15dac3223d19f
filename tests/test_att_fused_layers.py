"""CPU, no library call: `p_fused` on `layers.MultiHeadAttLayer`, `layers.LoRAttConvLayer` and their factories -- a plain
attribute (`fused_`), so the state dict stays the reference's (tests/golden/attention_layer_keys.json) and a checkpoint with the
reference's keys loads strictly; the factories hand the flag on; the default is False; the fused path has a refusal of its own
for capacity-bounded neighbourhoods and raises on CPU tensors like every other op."""
import json
import os

import pytest
import torch

import se3conv3d_amd as amd
from conftest import GOLDEN

with open(os.path.join(GOLDEN, "attention_layer_keys.json")) as fh:
    KEYS = json.load(fh)
FACTORIES = {"mha": "MultiHeadAttLayerFactory", "lora": "LoRAttConvLayerFactory"}
CLASSES = {"mha": "MultiHeadAttLayer", "lora": "LoRAttConvLayer"}


def test_state_dict_keys_and_shapes_with_p_fused_are_the_reference_s():
    for name, ref in KEYS.items():
        layer, res = name.split("/")
        conv = getattr(amd, FACTORIES[layer])(3, 16, res, 2, p_fused=True).create_conv_layer(8, 24)
        assert type(conv).__name__ == CLASSES[layer] and conv.fused_ is True
        assert {k: list(v.shape) for k, v in conv.state_dict().items()} == ref["state"], name
        assert "fused_" not in dict(conv.named_buffers()) and "fused_" not in dict(conv.named_parameters())
        # a checkpoint with the reference's keys loads strictly
        conv.load_state_dict({k: torch.full(shape, 0.25) for k, shape in ref["state"].items()}, strict=True)
        assert float(conv.pe_.detach().min()) == 0.25 and float(conv.norm_num_neighs_) == 0.25 and conv.fused_ is True
        plain = getattr(amd, FACTORIES[layer])(3, 16, res, 2).create_conv_layer(8, 24)
        plain.load_state_dict(conv.state_dict(), strict=True)             # the two settings exchange checkpoints
        assert plain.fused_ is False


@pytest.mark.parametrize("layer", ["mha", "lora"])
def test_the_default_is_false_and_the_factories_hand_the_flag_on(layer):
    cls, factory = getattr(amd, CLASSES[layer]), getattr(amd, FACTORIES[layer])
    assert cls(3, 8, 24, 16, "single", 2).fused_ is False
    assert cls(3, 8, 24, 16, "single", 2, True).fused_ is True and cls(3, 8, 24, 16, "single", 2, p_fused=1).fused_ is True
    assert factory(3, 16, "single", 2).fused_ is False and factory(3, 16, "single", 2).create_conv_layer(8, 24).fused_ is False
    fact = factory(3, 16, "double", 2, p_fused=True)
    a, b = fact.create_conv_layer(8, 24), fact.create_conv_layer(24, 8)
    assert a.fused_ is True and b.fused_ is True and fact.conv_list_ == [a, b]
    fact.update_parameters(num_basis=32)
    assert fact.create_conv_layer(8, 24).fused_ is True


@pytest.mark.parametrize("layer", ["mha", "lora"])
def test_refusals_of_the_fused_path(layer):
    class Cloud:
        pts_ = torch.zeros(4, 3)

    class Bounded:
        edge_info_ = torch.zeros(2)

    conv = getattr(amd, FACTORIES[layer])(3, 16, "single", 2, p_fused=True).create_conv_layer(8, 24)
    with pytest.raises(AssertionError, match="same object"):
        conv(Cloud(), Cloud(), torch.zeros(4, 8), None)
    pc = Cloud()
    with pytest.raises(NotImplementedError, match=r"a capacity-bounded neighbourhood .* cannot feed the fused attention \(p_fused=True\)"):
        conv(pc, pc, torch.zeros(4, 8), Bounded())
    plain = getattr(amd, FACTORIES[layer])(3, 16, "single", 2).create_conv_layer(8, 24)
    with pytest.raises(NotImplementedError, match="cannot feed the materialised path"):   # the unfused wording is untouched
        plain(pc, pc, torch.zeros(4, 8), Bounded())


def test_the_operator_has_no_cpu_fallback():
    assert amd.FusedBasisAttention is amd.ops.FusedBasisAttention
    nbr, ends = torch.tensor([[0, 1], [1, 0]], dtype=torch.int32), torch.tensor([1, 2], dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU fallback"):
        amd.ops.FusedBasisAttention.apply(torch.zeros(2, 8), torch.zeros(2, 6), torch.zeros(8, 2), nbr, ends, 1)
