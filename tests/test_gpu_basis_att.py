"""GPU: the entry points of include/se3conv_basis_att.h through `ops.BasisAttention`, and the two layers on top of them.

Kernels: `att`, `out`, `dT`, `dkey`, `dpe` are held per element against the float64 restatement of tests/basis_att_reference.py and
each element's own scale; the bounds are 8 x the float32 emulation (`R.bounds()`, computed from the emulation alone).  The
shapes are the smallest that reach every path of csrc/basis_att.hip:
    (1, 6, 3, 5)                 one row, odd K (one k per lane), D = 2
    (CHUNK + 1, 32, 4, 8)        a second chunk of one point
    (2 CHUNK + 37, 64, 1, 32)    one head of 64 channels, three chunks
    (300, 72, 8, 64)             D = 9 (no multiple of the rows in flight), K at the cap
    (70, 64, 64, 16)             D = 1
    (33, 12, 2, 12)              K % 4 == 0 and no power of two: a lane of every group holds no k
    (9, 136, 8, 64)              a `pe` beyond what a workgroup stages in LDS
    (1025, 8, 2, 8)              more (point, head) pairs than one workgroup walks: several workgroups, the last one part empty.
                                 The launchers have NO grid cap (one workgroup per 4 batches of groups, at most 2^31 / 64 / 4 of them
                                 under the header's 2^31 limits), so there is no cap for a row count to cross
    (50, 16, 4, 16) large        scores to +-80: exp overflows without the maximum
    N = 0
with magnitudes that differ per point and channel, a point with T = 0 and key = 0 (att exactly 1 / K), a contiguous key and a
key that is the last third of a [N, 3V] tensor (equal by bits), a T off 16-byte alignment (one k per lane: equal by bits to the
16-byte form, as the header's tree promises), and two calls (equal by bits).

Layers: the four cases of tests/golden/attention_layers.npz (the reference's own Python) within the whole-tensor fp32
tolerance, rel_err <= 2e-5, on out, dx and every parameter gradient; LoRAtt is MultiHeadAtt plus the dense product."""
import functools
import os

import numpy as np
import pytest
import torch

import basis_att_reference as R
from conftest import GOLDEN, load_npz, rel_err
from padded_cases import DEV

pytestmark = pytest.mark.gpu
TOL = 2e-5
RATIOS = {}      # entry -> largest observed / bound of this session (printed by the last test)
CASES = [(1, 6, 3, 5, "uneven"), (R.CHUNK + 1, 32, 4, 8, "zero"), (2 * R.CHUNK + 37, 64, 1, 32, "uneven"), (300, 72, 8, 64, "uneven"),
         (70, 64, 64, 16, "zero"), (33, 12, 2, 12, "zero"), (9, 136, 8, 64, "uneven"), (1025, 8, 2, 8, "uneven"),
         (50, 16, 4, 16, "large")]
IDS = [f"N{c[0]}-V{c[1]}-H{c[2]}-K{c[3]}-{c[4]}" for c in CASES]


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd as amd
    return amd


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy()).view(np.int32)


@functools.lru_cache(maxsize=None)
def reference(i):
    """The case and its float64 values and scales: computed once, shared by the tests, never written to."""
    case = R.case(400 + i, *CASES[i])
    want, scale = R.both(case)
    return case, want, scale


def run(amd, case, key_view=False, misaligned=False):
    """att, out, dT, dkey, dpe of the library.  `key_view`: the key is the last third of a [N, 3V] tensor whose other columns
    are NaN.  `misaligned`: T starts 4 bytes past a 16-byte boundary."""
    n, v = case["key"].shape
    T = t(case["T"])
    if misaligned:
        buf = torch.empty(T.numel() + 1, device=DEV)
        buf[1:] = T.reshape(-1)
        T = buf[1:].view(T.shape)
        assert T.data_ptr() % 16 == 4 and T.is_contiguous()
    T.requires_grad_(True)
    key = t(case["key"]).requires_grad_(True)
    pe = t(case["pe"]).requires_grad_(True)
    k_in = key
    if key_view:
        k_in = torch.cat([torch.full((n, 2 * v), float("nan"), device=DEV), key], 1)[:, 2 * v:]
        assert k_in.stride() == (3 * v, 1)
    out = amd.ops.BasisAttention.apply(T, k_in, pe, case["heads"])
    att = out.grad_fn.saved_tensors[3]                 # (the op returns out alone: att is what it keeps for its backward)
    out.backward(t(case["grad_out"]))
    return {"att": att, "out": out.detach(), "dT": T.grad, "dkey": key.grad, "dpe": pe.grad}


def held(name, got, want, scale):
    r = R.worst(got.detach().cpu().numpy(), want, scale) / R.bounds()[name]
    print(f"{name}: observed / bound = {r:.3f}")
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    assert r <= 1.0, f"{name}: {r:.3f} x its bound {R.bounds()[name]:.3g}"


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_per_element_against_the_restatement(amd, i):
    case, want, scale = reference(i)
    got = run(amd, case)
    for name in R.ENTRIES:
        assert tuple(got[name].shape) == want[name].shape, name
        held(name, got[name], want[name], scale[name])
    assert all(bool(torch.isfinite(x).all()) for x in got.values())
    again = run(amd, case)
    assert all(np.array_equal(bits(got[k]), bits(again[k])) for k in got), "two calls differ"
    viewed = run(amd, case, key_view=True)
    assert all(np.array_equal(bits(got[k]), bits(viewed[k])) for k in got), "a strided key changes the result"
    if case["kind"] == "zero":
        n, k = case["T"].shape[0], case["T"].shape[2]
        assert np.array_equal(bits(got["att"][n // 2]), np.full((k, case["heads"]), np.float32(1) / np.float32(k)).view(np.int32))
        assert not bits(got["dT"][n // 2, case["key"].shape[1]:]).any(), "dTq of a point with key = 0 is +0.0"
    if case["kind"] == "large":
        s = ((case["T"][:, case["key"].shape[1]:].astype(np.float64) + case["pe"].T[None]) * case["key"][:, :, None])
        s = s.reshape(s.shape[0], case["heads"], -1, s.shape[2]).sum(2)
        assert s.max() > 89 and s.min() < -89


@pytest.mark.parametrize("i", [1, 3, 5], ids=[IDS[i] for i in (1, 3, 5)])
def test_one_k_per_lane_gives_the_bits_of_the_16_byte_form(amd, i):
    """K % 4 == 0 with T off 16-byte alignment takes the scalar kernels: the header's tree does not depend on the form."""
    case, want, scale = reference(i)
    got, off = run(amd, case), run(amd, case, misaligned=True)
    assert all(np.array_equal(bits(got[k]), bits(off[k])) for k in got)


def test_no_rows(amd):
    case = R.case(9, 0, 8, 2, 8)
    got = run(amd, case)
    assert got["out"].shape == (0, 8) and got["dT"].shape == (0, 16, 8) and got["dkey"].shape == (0, 8)
    assert got["dpe"].shape == (8, 8) and not bits(got["dpe"]).any(), "dpe of no rows is +0.0, written by the kernel"


def test_arguments(amd):
    case = R.case(10, 4, 8, 2, 8)
    T, key, pe = t(case["T"]), t(case["key"]), t(case["pe"])
    out = amd.ops.BasisAttention.apply(T, key, pe, 2)
    assert np.array_equal(bits(out), bits(amd.ops.BasisAttention.apply(T, key, pe.reshape(1, 8, 8), 2))), "pe as [1,K,V]"
    assert np.array_equal(bits(out), bits(amd.ops.BasisAttention.apply(T, key.double(), pe, 2))), "another dtype is converted"
    for bad in (lambda: amd.ops.BasisAttention.apply(T.cpu(), key, pe, 2), lambda: amd.ops.BasisAttention.apply(T, key, pe, 3),
                lambda: amd.ops.BasisAttention.apply(T, key[:, :4], pe, 2), lambda: amd.ops.BasisAttention.apply(T, key, pe[:, :4], 2)):
        with pytest.raises(ValueError):
            bad()


# --------------------------------------------------------------------------------------------------------------- layers
@pytest.fixture(scope="module")
def fixture():
    return load_npz(os.path.join(GOLDEN, "attention_layers.npz"))


def cloud(amd, d):
    pc = amd.pc.Pointcloud(d["pts"].to(DEV), d["batch"].to(DEV))
    nbh = amd.pc.BQNeighborhood(pc, pc, float(d["radius"]))
    assert torch.equal(nbh.start_ids_.cpu(), d["ends"])
    return pc, nbh


def layer_of(amd, d, layer, res, params_of=None):
    key, src = f"{layer}/{res}/", f"{params_of or layer}/{res}/"
    params = {k[len(src + "param/"):]: v for k, v in d.items() if k.startswith(src + "param/")}
    c_out, v = params["w_out_.weight"].shape
    k = params["proj_biases_"].shape[0]
    factory = {"mha": amd.MultiHeadAttLayerFactory, "lora": amd.LoRAttConvLayerFactory}[layer]
    conv = factory(3, k, res, int(d[key + "heads"])).create_conv_layer(v, c_out)
    with torch.no_grad():
        for name, p in conv.named_parameters():
            p.copy_(params[name])
        conv.kernel_pts_.copy_(d[src + "kernel_pts_"])
        conv.norm_neigh_dist_.copy_(d["rho"]), conv.norm_num_neighs_.copy_(d["nu"])
    assert abs(conv.kp_sigma_ - float(d[key + "sigma"])) < 1e-7
    return conv.to(DEV)


LAYER_CASES = [(layer, res) for layer in ("mha", "lora") for res in ("single", "double")]


@pytest.mark.parametrize("layer,res", LAYER_CASES, ids=[f"{a}-{b}" for a, b in LAYER_CASES])
def test_layer_matches_the_reference_fixture(amd, fixture, layer, res):
    d = fixture
    key = f"{layer}/{res}/"
    conv = layer_of(amd, d, layer, res)
    pc, nbh = cloud(amd, d)
    x = d["x"].to(DEV).requires_grad_(True)
    out = conv(p_pc_in=pc, p_pc_out=pc, p_in_features=x, p_neighborhood=nbh)
    assert out.shape == d[key + "out"].shape
    out.backward(d["grad_out"].to(DEV))
    errs = {"out": rel_err(out, d[key + "out"]), "dx": rel_err(x.grad, d[key + "dx"])}
    names = [n for n, _ in conv.named_parameters()]
    assert sorted(names) == sorted(k[len(key + "grad/"):] for k in d if k.startswith(key + "grad/"))
    for name, p in conv.named_parameters():
        errs[name] = rel_err(p.grad, d[key + "grad/" + name])
    print(key, {n: f"{e:.2e}" for n, e in errs.items()})
    RATIOS[f"rel_err {layer}-{res}"] = max(errs.values()) / TOL
    assert all(e <= TOL for e in errs.values()), errs


@pytest.mark.parametrize("res", ["single", "double"])
def test_lorattconv_is_multiheadatt_plus_the_dense_product(amd, fixture, res):
    d = fixture
    lora, mha = layer_of(amd, d, "lora", res), layer_of(amd, d, "mha", res, params_of="lora")
    pc, nbh = cloud(amd, d)
    x = d["x"].to(DEV)
    with torch.no_grad():
        got = lora(p_pc_in=pc, p_pc_out=pc, p_in_features=x, p_neighborhood=nbh)
        att, T = mha._attend(pc, pc, x, nbh)
        assert np.array_equal(bits(mha(p_pc_in=pc, p_pc_out=pc, p_in_features=x, p_neighborhood=nbh)), bits(att * mha.norm_num_neighs_))
        v, k = lora.value_size_, lora.num_basis_
        dense = torch.einsum("nik,kio->no", T[:, :v, :], lora.conv_weights_)
        assert rel_err(got, (att + dense) * lora.norm_num_neighs_) <= 2e-6 and float(dense.abs().max()) > 0


def test_refusals_that_need_a_neighbourhood(amd, fixture):
    d = fixture
    pc, nbh = cloud(amd, d)
    other = amd.pc.Pointcloud(d["pts"].to(DEV), d["batch"].to(DEV))
    conv = amd.MultiHeadAttLayerFactory(3, 16, "single", 2).create_conv_layer(8, 24).to(DEV)
    with pytest.raises(AssertionError, match="same object"):
        conv(other, pc, d["x"].to(DEV), nbh)
    bounded = amd.pc.BQNeighborhood(pc, pc, float(d["radius"]), p_capacity=20000)
    with pytest.raises(NotImplementedError, match="capacity-bounded"):
        conv(pc, pc, d["x"].to(DEV), bounded)


def test_zz_error_ratios_of_this_session():
    """Prints the largest observed / bound per tensor (what profiles/att_layers.txt records); every one was asserted above."""
    print({k: round(v, 3) for k, v in RATIOS.items()})
    assert all(v <= 1.0 for v in RATIOS.values())
