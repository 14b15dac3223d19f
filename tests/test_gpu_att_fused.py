"""GPU: the entry points of include/se3conv_att_fused.h, `ops.FusedBasisAttention`, and the two layers with `p_fused=True`.

Kernels: `att`, `out`, `dphi`, `dx` (dxv | dxq | dkey) and `dpe` are held per element against the float64 restatement of
tests/att_fused_reference.py and each element's own scale; the bounds are 8 x the float32 emulation (`R.bounds()`, computed from
the emulation alone).  The entry points are called directly, on buffers of this module, with the library's own transposition
(`ops.csr_transpose`).  The cases `(N, V, H, K, max degree, hub, kind)` are the smallest that reach every path of
csrc/att_fused.hip:
    (1, 8, 2, 8, 1)                 one point with one self edge
    (70, 64, 64, 16, 5)             D = 1: the scalar form, 64 heads
    (CHUNK + 1, 32, 4, 8, 9)        a second `dpe` chunk of one point; more samples than one workgroup walks (32)
    (40, 72, 8, 64, 12, hub 700)    D = 9 (scalar form), K at the cap, one sample walked in eleven slabs of 64 edges
    (300, 16, 1, 32, 8, large)      scores to +-80: exp overflows without the maximum
    (33, 12, 2, 5, 6)               K no power of two: lanes of the k group hold nothing
    (130, 64, 4, 32, 10)            D = 16, aligned: the 16-byte form -- and again with EVERY array 4 bytes off a 16-byte boundary,
                                    the scalar form: equal by bits, as the header promises
every graph with an edge-less sample, sources without incoming edges, a self edge and a source repeated inside a sample
(`R.graph`).  For each: the five outputs within bounds, `out` of edge-less samples and `dxv` / `dxq` of unreferenced sources
exactly +0.0, two calls equal by bits.  Then N = 0, E = 0, the autograd function against the direct calls, and its arguments.

Layers: the four cases of tests/golden/attention_layers.npz (the reference's own Python) with `p_fused=True` within the
whole-tensor fp32 tolerance tests/test_gpu_basis_att.py holds the unfused layers to, rel_err <= 2e-5, on out, dx and every
parameter gradient -- and at the same bound against the same layer with `p_fused=False` and copied weights."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import att_fused_reference as R
from conftest import GOLDEN, load_npz, rel_err
from padded_cases import DEV
from se3conv3d_amd import _lib

pytestmark = pytest.mark.gpu
TOL = 2e-5
RATIOS = {}      # entry -> largest observed / bound of this session (printed by the last test)
CASES = [(1, 8, 2, 8, 1, 0, "uneven"), (70, 64, 64, 16, 5, 0, "uneven"), (R.CHUNK + 1, 32, 4, 8, 9, 0, "uneven"),
         (40, 72, 8, 64, 12, 700, "uneven"), (300, 16, 1, 32, 8, 0, "large"), (33, 12, 2, 5, 6, 0, "uneven"),
         (130, 64, 4, 32, 10, 0, "uneven")]
IDS = [f"N{c[0]}-V{c[1]}-H{c[2]}-K{c[3]}-deg{c[4]}-hub{c[5]}-{c[6]}" for c in CASES]


@pytest.fixture(scope="module")
def amd(built_library):
    import se3conv3d_amd as amd
    return amd


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy()).view(np.int32)


def off16(x, off):
    """A contiguous copy of `x` that starts `off` bytes past a 16-byte boundary (4-byte elements)."""
    buf = torch.empty(x.numel() + 8, dtype=x.dtype, device=DEV)
    first = ((-buf.data_ptr()) % 16 + off) // 4
    out = buf[first:first + x.numel()].view(x.shape)
    out.copy_(x)
    assert out.numel() == 0 or out.data_ptr() % 16 == off
    return out


@functools.lru_cache(maxsize=None)
def reference(i):
    """The case and its float64 values and scales: computed once, shared by the tests, never written to."""
    case = R.case(600 + i, *CASES[i])
    want, scale = R.both(case)
    return case, want, scale


@functools.lru_cache(maxsize=None)
def transposition(i):
    """The library's own transposition of case `i`, built once: the header sums a source's entries in the order of the list it
    is handed, so runs that are compared by bits are handed the same list."""
    import se3conv3d_amd as amd

    case, _, _ = reference(i)
    return amd.ops.csr_transpose(t(case["neighbors"]), case["x"].shape[0], want_edge_ids=True)


def differing(a, b):
    """The entries of two results that are not equal by bits (`dx` by its thirds)."""
    v = a["dx"].shape[1] // 3
    parts = lambda r: {**{k: r[k] for k in r if k != "dx"}, "dxv": r["dx"][:, :v], "dxq": r["dx"][:, v:2 * v], "dkey": r["dx"][:, 2 * v:]}
    pa, pb = parts(a), parts(b)
    return [k for k in pa if not np.array_equal(bits(pa[k]), bits(pb[k]))]


def run(amd, case, off=0, tr=None):
    """att, out, dphi, dx, dpe of the library, by direct calls: every array `off` bytes past a 16-byte boundary, the outputs
    and the workspace filled with NaN beforehand.  `tr`: the transposition (None: built here)."""
    lib = _lib.load()
    f32 = torch.float32
    h = case["heads"]
    put = lambda a: off16(a if isinstance(a, torch.Tensor) else t(a), off)
    phi, x, pe, g = put(case["phi"]), put(case["x"]), put(case["pe"]), put(case["grad_out"])
    nbr, ends = put(case["neighbors"]), put(case["ends"])
    (e, k), n, v = phi.shape, x.shape[0], x.shape[1] // 3
    if e:
        ts, te, tid = (put(a) for a in (tr or amd.ops.csr_transpose(t(case["neighbors"]), n, want_edge_ids=True)))
    else:
        ts, te, tid = None, put(np.zeros(n, np.int32)), None
    nan = lambda *shape: off16(torch.full(shape, float("nan"), dtype=f32, device=DEV), off)
    att, out, dphi, dx, dpe = nan(n, k, h), nan(n, v), nan(e, k), nan(n, 3 * v), nan(k, v)
    need = lib.se3_att_fused_workspace_bytes(n, e, v, h, k)
    assert need > 0
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    p = lambda a: C.c_void_p(a.data_ptr()) if a is not None and a.numel() else None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.se3_att_fused_fwd(p(phi), p(x), p(pe), p(nbr), p(ends), n, e, v, h, k, p(att), p(out), stream)
    assert rc == 0, rc
    rc = lib.se3_att_fused_bwd(p(g), p(phi), p(x), p(pe), p(att), p(nbr), p(ends), p(ts), p(te), p(tid), n, e, v, h, k, p(dphi), p(dx),
                               p(dpe), C.c_void_p(ws.data_ptr()), need, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {"att": att, "out": out, "dphi": dphi, "dx": dx, "dpe": dpe}


def held(name, got, want, scale):
    r = R.worst(got.detach().cpu().numpy(), want, scale) / R.bounds()[name]
    print(f"{name}: observed / bound = {r:.3f}")
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    assert r <= 1.0, f"{name}: {r:.3f} x its bound {R.bounds()[name]:.3g}"


def check(case, got, want, scale):
    for name in R.ENTRIES:
        assert tuple(got[name].shape) == want[name].shape, name
        assert bool(torch.isfinite(got[name]).all()), name
        held(name, got[name], want[name], scale[name])
    n, v = case["x"].shape[0], case["x"].shape[1] // 3
    deg = np.bincount(case["neighbors"][:, 0], minlength=n)
    incoming = np.bincount(case["neighbors"][:, 1], minlength=n)
    assert not bits(got["out"])[deg == 0].any(), "out of an edge-less sample is +0.0"
    assert not bits(got["dx"])[incoming == 0, :2 * v].any(), "dxv and dxq of a source without incoming edges are +0.0"
    return deg, incoming


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_per_element_against_the_restatement(amd, i):
    case, want, scale = reference(i)
    got = run(amd, case, tr=transposition(i))
    deg, incoming = check(case, got, want, scale)
    n = deg.shape[0]
    assert n == 1 or ((deg == 0).any() and (incoming == 0).sum() >= 2), "the graph holds what the case is there for"
    again = run(amd, case, tr=transposition(i))
    assert not differing(got, again), "two calls differ"
    fresh = run(amd, case)                             # a transposition of its own: what does not read it has the same bits
    assert not set(differing(got, fresh)) - {"dxv", "dxq"}
    if case["kind"] == "large":
        nbr, v = case["neighbors"], case["x"].shape[1] // 3
        c = np.einsum("ei,ei->e", case["x"][nbr[:, 1], v:2 * v].astype(np.float64), case["x"][nbr[:, 0], 2 * v:].astype(np.float64))
        s = np.zeros((n, case["phi"].shape[1]))
        np.add.at(s, nbr[:, 0], case["phi"].astype(np.float64) * c[:, None])
        assert s.max() > 80 and s.min() < -80
    if CASES[i][5]:
        assert deg.max() == CASES[i][5] > 10 * R.SLAB


def test_every_array_off_16_byte_alignment_gives_the_bits_of_the_16_byte_form(amd):
    """D = 16 and aligned arrays take the 16-byte accesses, the same arrays 4 bytes further on the scalar form: one contract,
    the same operations in the same order, so the same bits -- and the misaligned run is held to the restatement on its own."""
    case, want, scale = reference(len(CASES) - 1)
    assert (case["x"].shape[1] // 3 // case["heads"]) % 4 == 0
    tr = transposition(len(CASES) - 1)
    got, off = run(amd, case, tr=tr), run(amd, case, off=4, tr=tr)
    check(case, off, want, scale)
    assert not differing(got, off)


def test_no_rows(amd):
    case = R.case(9, 0, 8, 2, 8, 3)
    assert case["x"].shape == (0, 24) and case["phi"].shape == (0, 8)
    got = run(amd, case)
    assert got["out"].shape == (0, 8) and got["dx"].shape == (0, 24) and got["dphi"].shape == (0, 8)
    assert got["dpe"].shape == (8, 8) and not bits(got["dpe"]).any(), "dpe of no rows is +0.0, written by the kernel"


def test_no_edges(amd):
    case = R.case(10, 37, 12, 2, 8, 0)
    assert case["phi"].shape == (0, 8) and not case["ends"].any()
    want, scale = R.both(case)
    got = run(amd, case)
    check(case, got, want, scale)
    assert not bits(got["out"]).any() and not bits(got["dx"]).any() and not bits(got["dpe"]).any(), "no edge: att alone is not zero"
    assert float(got["att"].min()) > 0 and np.allclose(got["att"].sum(1).cpu().numpy(), 1, atol=1e-5)


def through_autograd(amd, case, cache=None, nbr=None):
    phi, x, pe = (t(case[k]).requires_grad_(True) for k in ("phi", "x", "pe"))
    nbr = t(case["neighbors"]) if nbr is None else nbr
    out = amd.ops.FusedBasisAttention.apply(phi, x, pe, nbr, t(case["ends"]), case["heads"], cache)
    att = out.grad_fn.saved_tensors[5]                 # (the op returns out alone: att is what it keeps for its backward)
    out.backward(t(case["grad_out"]))
    return {"att": att, "out": out.detach(), "dphi": phi.grad, "dx": x.grad, "dpe": pe.grad}


@pytest.mark.parametrize("i", [0, 2, 5])
def test_the_autograd_function_gives_the_bits_of_the_direct_calls(amd, i):
    case, _, _ = reference(i)

    class Holder:
        pass

    cache, nbr = Holder(), t(case["neighbors"])
    auto = through_autograd(amd, case, cache, nbr)
    assert hasattr(cache, "_se3_max_transpose"), "the transposition is kept on the neighbourhood object"
    kept = cache._se3_max_transpose[1]
    again = through_autograd(amd, case, cache, nbr)
    assert cache._se3_max_transpose[1] is kept, "and used again for the same edge list"
    direct = run(amd, case, tr=kept)
    assert not differing(direct, auto) and not differing(direct, again)
    assert not set(differing(direct, through_autograd(amd, case))) - {"dxv", "dxq"}, "without a cache: a transposition per call"


def test_no_rows_and_no_edges_through_autograd(amd):
    got = through_autograd(amd, R.case(9, 0, 8, 2, 8, 3))
    assert got["out"].shape == (0, 8) and got["dx"].shape == (0, 24) and got["dpe"].shape == (8, 8) and not bits(got["dpe"]).any()
    case = R.case(10, 37, 12, 2, 8, 0)
    got, direct = through_autograd(amd, case), run(amd, case)
    assert not differing(direct, got)


def test_arguments(amd):
    case = R.case(13, 9, 8, 2, 8, 4)
    phi, x, pe, nbr, ends = (t(case[k]) for k in ("phi", "x", "pe", "neighbors", "ends"))
    F = amd.ops.FusedBasisAttention.apply
    out = F(phi, x, pe, nbr, ends, 2)
    assert np.array_equal(bits(out), bits(F(phi, x, pe.reshape(1, 8, 8), nbr, ends, 2))), "pe as [1,K,V]"
    assert np.array_equal(bits(out), bits(F(phi.double(), x.double(), pe, nbr.long(), ends.long(), 2))), "other dtypes are converted"
    for bad in (lambda: F(phi.cpu(), x, pe, nbr, ends, 2), lambda: F(phi, x, pe, nbr, ends, 3), lambda: F(phi, x[:, :23], pe, nbr, ends, 2),
                lambda: F(phi, x, pe[:, :4], nbr, ends, 2), lambda: F(phi[:-1], x, pe, nbr, ends, 2), lambda: F(phi, x, pe, nbr, ends[:-1], 2)):
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


def layer_of(amd, d, layer, res, fused):
    key = f"{layer}/{res}/"
    params = {k[len(key + "param/"):]: v for k, v in d.items() if k.startswith(key + "param/")}
    c_out, v = params["w_out_.weight"].shape
    k = params["proj_biases_"].shape[0]
    factory = {"mha": amd.MultiHeadAttLayerFactory, "lora": amd.LoRAttConvLayerFactory}[layer]
    conv = factory(3, k, res, int(d[key + "heads"]), p_fused=fused).create_conv_layer(v, c_out)
    assert conv.fused_ is fused
    with torch.no_grad():
        for name, p in conv.named_parameters():
            p.copy_(params[name])
        conv.kernel_pts_.copy_(d[key + "kernel_pts_"])
        conv.norm_neigh_dist_.copy_(d["rho"]), conv.norm_num_neighs_.copy_(d["nu"])
    return conv.to(DEV)


def forward_backward(amd, d, conv):
    pc, nbh = cloud(amd, d)
    x = d["x"].to(DEV).requires_grad_(True)
    out = conv(p_pc_in=pc, p_pc_out=pc, p_in_features=x, p_neighborhood=nbh)
    out.backward(d["grad_out"].to(DEV))
    return {"out": out.detach(), "dx": x.grad, **{name: p.grad for name, p in conv.named_parameters()}}


LAYER_CASES = [(layer, res) for layer in ("mha", "lora") for res in ("single", "double")]


@pytest.mark.parametrize("layer,res", LAYER_CASES, ids=[f"{a}-{b}" for a, b in LAYER_CASES])
def test_fused_layer_matches_the_reference_fixture_and_the_unfused_layer(amd, fixture, layer, res):
    d = fixture
    key = f"{layer}/{res}/"
    fused = forward_backward(amd, d, layer_of(amd, d, layer, res, True))
    plain = forward_backward(amd, d, layer_of(amd, d, layer, res, False))
    assert fused["out"].shape == d[key + "out"].shape
    assert sorted(set(fused) - {"out", "dx"}) == sorted(k[len(key + "grad/"):] for k in d if k.startswith(key + "grad/"))
    golden = {"out": d[key + "out"], "dx": d[key + "dx"], **{n: d[key + "grad/" + n] for n in fused if n not in ("out", "dx")}}
    errs = {n: rel_err(fused[n], golden[n]) for n in fused}
    errs_plain = {n: rel_err(fused[n], plain[n]) for n in fused}
    print(key, "against the fixture", {n: f"{e:.2e}" for n, e in errs.items()})
    print(key, "against p_fused=False", {n: f"{e:.2e}" for n, e in errs_plain.items()})
    RATIOS[f"rel_err {layer}-{res} fixture"] = max(errs.values()) / TOL
    RATIOS[f"rel_err {layer}-{res} unfused"] = max(errs_plain.values()) / TOL
    assert all(e <= TOL for e in errs.values()), errs
    assert all(e <= TOL for e in errs_plain.values()), errs_plain


def test_refusal_of_a_capacity_bounded_neighbourhood(amd, fixture):
    d = fixture
    pc, _ = cloud(amd, d)
    conv = amd.MultiHeadAttLayerFactory(3, 16, "single", 2, p_fused=True).create_conv_layer(8, 24).to(DEV)
    bounded = amd.pc.BQNeighborhood(pc, pc, float(d["radius"]), p_capacity=20000)
    with pytest.raises(NotImplementedError, match="cannot feed the fused attention"):
        conv(pc, pc, d["x"].to(DEV), bounded)


def test_zz_error_ratios_of_this_session():
    """Prints the largest observed / bound per tensor (what profiles/att_fused.txt records); every one was asserted above."""
    print({k: round(v, 3) for k, v in RATIOS.items()})
    assert all(v <= 1.0 for v in RATIOS.values())
