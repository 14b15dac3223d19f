"""CPU tests of the recipe that compiles the reference's native ops (`oracle/build_ref.py`), of their loader
(`oracle/ref_ops.py`) and of the cases of tests/reference_kernels.py.  The compile step is injected: nothing here runs the real
build, and nothing needs the reference tree.

The last group plants, in the restatements the GPU tests compare the compiled ops with, the misreadings those tests exist to
catch -- `<=` for `<` at the radius, a neighbour loop that stops at the last whole pass of the block, a window of two cells,
ties broken to the higher index -- and checks that each one is visible on the cases the GPU tests use."""
import json
import os

import numpy as np
import pytest
import torch

import api_parity_reference as REF
import reference_kernels as K
from oracle import build_ref, ref_ops
from oracle import se3conv_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_UTILS = """#pragma once
inline int keep_me(int first)
{
    return first + 1;
};

/**
 *  A helper nothing calls (our own text: only its name matters to the recipe).
 */
static float atomicMax(float* slot, float candidate)
{
    for (int turn = 0; turn < 2; ++turn) {
        if (*slot < candidate) { *slot = candidate; }
    }
    return *slot;
};

inline int keep_me_too(int second) { return second; }
"""


def fake_tree(root):
    ops = os.path.join(root, build_ref.OPS_SUBDIR)
    os.makedirs(os.path.join(ops, "sub"))
    for rel, text in (("utils.cuh", FAKE_UTILS), ("ops_list.cpp", "int a;\n"), ("sub/kernel.cu", "int b;\n"), ("sub/kernel.cuh", "int c;\n"),
                      ("notes.txt", "not a source\n")):
        with open(os.path.join(ops, rel), "w") as f:
            f.write(text)
    return ops


class FakeCompile:
    def __init__(self):
        self.calls, self.seen, self.work = 0, None, None

    def __call__(self, copy_root, work):
        self.calls += 1
        self.work = work
        self.seen = {}
        for base, _dirs, files in os.walk(work):
            for name in files:
                with open(os.path.join(base, name)) as f:
                    self.seen[os.path.relpath(os.path.join(base, name), work)] = f.read()
        so = os.path.join(work, "fake.so")
        with open(so, "wb") as f:
            f.write(b"\x7fELF fake %d" % self.calls)
        return so


def listing(path):
    return sorted((os.path.relpath(os.path.join(b, n), path), os.path.getmtime(os.path.join(b, n)), os.path.getsize(os.path.join(b, n)))
                  for b, _d, fs in os.walk(path) for n in fs) if os.path.isdir(path) else None


# ------------------------------------------------------------------------------------------------ the recipe
def test_manifest_round_trip_and_rebuild_only_when_a_hash_changes(tmp_path):
    ref, out = str(tmp_path / "ref"), str(tmp_path / "out")
    ops = fake_tree(ref)
    compile_step = FakeCompile()
    assert build_ref.build_reference(ref, out, compile_step, verbose=False) == "built" and compile_step.calls == 1
    assert sorted(os.listdir(out)) == ["manifest.json", build_ref.MODULE + ".so"]           # nothing else is kept
    man = build_ref.read_manifest(out)
    assert man["torch"] == torch.__version__ and man["arch"] == "gfx950" and man["max_jobs"] <= 16 and man["file"] == build_ref.MODULE + ".so"
    assert man["cflags"] == build_ref.CFLAGS and man["hip_cflags"] == build_ref.HIP_CFLAGS
    assert sorted(man["sources"]) == ["ref_shims/THC/THCAtomics.cuh", "reference/ops_list.cpp", "reference/sub/kernel.cu",
                                      "reference/sub/kernel.cuh", "reference/utils.cuh"]
    assert man["sources"] == build_ref.source_hashes(ops) and man == json.loads(json.dumps(man))
    assert build_ref.module_path(out) == os.path.join(out, man["file"]) and build_ref.up_to_date(ops, out)
    # the copy the compiler saw: outside the repository, the unused helper cut out, everything else as it was, our shim beside it
    assert not os.path.exists(compile_step.work) and os.path.commonpath([ROOT, os.path.realpath(compile_step.work)]) != ROOT
    utils = compile_step.seen["custom_ops/utils.cuh"]
    assert "atomicMax" not in utils and "A helper nothing calls" not in utils
    last = "    return *slot;\n};\n"
    assert utils == FAKE_UTILS[:FAKE_UTILS.index("/**")] + FAKE_UTILS[FAKE_UTILS.index(last) + len(last):]
    assert compile_step.seen["custom_ops/sub/kernel.cu"] == "int b;\n" and "Atomic.cuh" in compile_step.seen["ref_shims/THC/THCAtomics.cuh"]
    with open(os.path.join(ops, "utils.cuh")) as f:
        assert f.read() == FAKE_UTILS                                                         # the tree itself is only read
    # a second call compiles nothing; a changed source, another torch or a lost module does
    before = listing(out)
    assert build_ref.build_reference(ref, out, compile_step, verbose=False) == "current" and compile_step.calls == 1 and listing(out) == before
    with open(os.path.join(ops, "notes.txt"), "a") as f:
        f.write("still not a source\n")
    assert build_ref.build_reference(ref, out, compile_step, verbose=False) == "current"
    with open(os.path.join(ops, "sub", "kernel.cuh"), "a") as f:
        f.write("int d;\n")
    assert build_ref.build_reference(ref, out, compile_step, verbose=False) == "built" and compile_step.calls == 2
    assert build_ref.read_manifest(out)["sources"]["reference/sub/kernel.cuh"] != man["sources"]["reference/sub/kernel.cuh"]
    stale = dict(build_ref.read_manifest(out), torch="0.0.0")
    with open(os.path.join(out, "manifest.json"), "w") as f:
        json.dump(stale, f)
    assert build_ref.build_reference(ref, out, compile_step, verbose=False) == "built" and compile_step.calls == 3
    os.remove(build_ref.module_path(out))
    assert build_ref.build_reference(ref, out, compile_step, verbose=False) == "built" and compile_step.calls == 4


def test_a_failed_build_with_the_reference_present_raises_and_leaves_no_copy(tmp_path):
    ref, out = str(tmp_path / "ref"), str(tmp_path / "out")
    fake_tree(ref)
    seen = {}

    def failing(copy_root, work):
        seen["work"] = work
        raise RuntimeError("compiler said no")

    with pytest.raises(RuntimeError, match="compiler said no"):
        build_ref.build_reference(ref, out, failing, verbose=False)
    assert not os.path.exists(seen["work"]) and not os.path.exists(out)


def test_without_the_reference_nothing_is_touched(tmp_path, monkeypatch, capsys):
    ref, out = str(tmp_path / "ref"), str(tmp_path / "out")
    fake_tree(ref)
    compile_step = FakeCompile()
    build_ref.build_reference(ref, out, compile_step, verbose=False)
    before = listing(out)
    nowhere = str(tmp_path / "nowhere")
    assert build_ref.build_reference(nowhere, out, compile_step, verbose=False) == "kept"       # module present, tree absent
    assert listing(out) == before and compile_step.calls == 1
    empty = str(tmp_path / "empty_out")
    assert build_ref.build_reference(nowhere, empty, compile_step) == "absent"                  # neither: one line
    assert not os.path.exists(empty) and len(capsys.readouterr().out.strip().splitlines()) == 1
    # the real oracle/_ref/, through the environment variable build() reads
    monkeypatch.setenv(build_ref.REF_DIR_ENV, nowhere)
    assert build_ref.reference_dir() == nowhere
    real = listing(build_ref.OUT_DIR)
    assert build_ref.build_reference(compile_step=compile_step, verbose=False) in ("kept", "absent")
    assert listing(build_ref.OUT_DIR) == real and compile_step.calls == 1


def test_the_recipe_holds_no_reference_text_and_the_tree_ignores_its_output():
    with open(os.path.join(ROOT, ".gitignore")) as f:
        assert "oracle/_ref/" in f.read().split()
    with open(os.path.join(ROOT, "oracle", "ref_shims", "THC", "THCAtomics.cuh")) as f:
        code = [line for line in f.read().splitlines() if line.strip() and not line.startswith("//")]
    assert code == ["#include <ATen/cuda/Atomic.cuh>"]
    for rel in ("se3conv3d_amd", "bench.py"):                  # product code never loads the reference ops
        paths = [os.path.join(b, n) for b, _d, fs in os.walk(os.path.join(ROOT, rel)) for n in fs if n.endswith(".py")] \
            if os.path.isdir(os.path.join(ROOT, rel)) else [os.path.join(ROOT, rel)]
        for path in paths:
            with open(path) as f:
                text = f.read()
            assert "ref_ops" not in text and "build_ref" not in text, path


def test_cut_function_refuses_a_name_that_is_not_there():
    with pytest.raises(RuntimeError, match="no definition"):
        build_ref.cut_function("int f(int a) { return a; }\n", "atomicMax")
    assert build_ref.cut_function("int g() { return 1; }\nint f(int a) { if (a) { a = 2; } return a; }\nint h();\n", "f") == "int g() { return 1; }\nint h();\n"


# ------------------------------------------------------------------------------------------------ the loader
def test_load_is_none_without_a_manifest_and_raises_with_a_bad_one(tmp_path):
    assert ref_ops.load(str(tmp_path)) is None and ref_ops.load(str(tmp_path / "missing")) is None
    manifest = {"module": build_ref.MODULE, "file": build_ref.MODULE + ".so", "torch": "0.0.0+other"}
    with open(tmp_path / "manifest.json", "w") as f:
        json.dump(manifest, f)
    with pytest.raises(ref_ops.ReferenceOpsError, match="torch 0.0.0"):
        ref_ops.load(str(tmp_path))
    manifest["torch"] = torch.__version__
    with open(tmp_path / "manifest.json", "w") as f:
        json.dump(manifest, f)
    with pytest.raises(ref_ops.ReferenceOpsError, match="not there"):
        ref_ops.load(str(tmp_path))
    with open(tmp_path / manifest["file"], "wb") as f:
        f.write(b"not a shared object")
    with pytest.raises(ref_ops.ReferenceOpsError, match="does not load"):
        ref_ops.load(str(tmp_path))


def test_the_real_build_exposes_exactly_the_five_ops():
    if build_ref.read_manifest() is None:
        pytest.skip("oracle/_ref/ holds no build: build() ran without the reference tree")
    module = ref_ops.load()
    assert sorted(n for n in dir(module) if not n.startswith("_")) == sorted(ref_ops.OPS)
    man = build_ref.read_manifest()
    assert sorted(os.listdir(build_ref.OUT_DIR)) == sorted(["manifest.json", man["file"]])
    assert man["sha256"] == build_ref._sha256(build_ref.module_path()) and man["arch"] == "gfx950"


# ------------------------------------------------------------------------------------------------ the domain
def _fbp_args(k, c, n_e=6, n_feat=5, m=3):
    ends = torch.tensor([2, 2, n_e], dtype=torch.int32)[:m]
    nb = torch.stack((torch.from_numpy(REF.edge_rows(ends.numpy())).to(torch.int32), torch.arange(n_e, dtype=torch.int32) % n_feat), 1)
    return torch.zeros(n_e, k), torch.zeros(n_feat, c), nb.contiguous(), ends


def test_domain_assertions_reject_what_the_kernels_cannot_take():
    K.check_fbp_domain(*_fbp_args(32, 8), device=False)
    K.check_fbp_domain(*_fbp_args(8, 3), device=False)
    with pytest.raises(K.DomainError, match="C_in = 13"):
        K.check_fbp_domain(*_fbp_args(32, 13), device=False)
    with pytest.raises(K.DomainError, match="K = 12"):
        K.check_fbp_domain(*_fbp_args(12, 8), device=False)
    with pytest.raises(AssertionError, match="not on the device"):
        K.check_fbp_domain(*_fbp_args(32, 8))
    basis, feat, nb, ends = _fbp_args(32, 8)
    with pytest.raises(K.DomainError, match="outside the feature rows"):
        K.check_fbp_domain(basis, feat[:3].contiguous(), nb, ends, device=False)
    with pytest.raises(K.DomainError, match="ends"):
        K.check_fbp_domain(basis, feat, nb, torch.tensor([2, 1, 6], dtype=torch.int32), device=False)
    with pytest.raises(K.DomainError, match="not contiguous"):
        K.check_fbp_domain(torch.zeros(32, 6).t(), feat, nb, ends, device=False)
    with pytest.raises(K.DomainError, match="sorted by sample"):
        K.check_fbp_domain(basis, feat, nb.flip(0).contiguous(), ends, device=False)
    with pytest.raises(K.DomainError, match="grads"):
        K.check_fbp_domain(basis, feat, nb, ends, torch.zeros(3, 8, 16), device=False)
    pts, bid = K.knn_case()
    K.check_knn_domain(pts, bid, 64, device=False)
    with pytest.raises(K.DomainError, match="k = 65"):
        K.check_knn_domain(pts, bid, 65, device=False)
    with pytest.raises(K.DomainError, match="sorted"):
        K.check_knn_domain(pts, bid.flip(0).contiguous(), 8, device=False)
    c = K.ball_cases()["two_clouds_b3"]
    mn, nc, rt = K.grid_params(c["pts_src"], c["batch_src"], c["radius"])
    args = (c["pts_src"], c["pts_dst"], c["batch_src"], c["batch_dst"], mn, nc, rt)
    K.check_ball_query_domain(*args, 0, device=False)
    K.check_ball_query_domain(*args, K.CAPPED_LIMIT, c["degrees"], device=False)
    with pytest.raises(K.DomainError, match="sample 0"):
        K.check_ball_query_domain(*args, K.CAPPED_LIMIT, c["degrees"].flip(0), device=False)
    with pytest.raises(K.DomainError, match="pencil table"):
        K.check_ball_query_domain(c["pts_src"], c["pts_dst"], c["batch_src"], c["batch_dst"] + 1, mn, nc, rt, 0, device=False)
    with pytest.raises(K.DomainError, match="0 .. B-1"):
        K.check_ball_query_domain(c["pts_src"], c["pts_dst"], c["batch_src"] * 2, c["batch_dst"], mn, nc, rt, 0, device=False)
    with pytest.raises(K.DomainError, match="n >= 1"):
        K.check_keys_domain(c["pts_src"][:0], c["batch_src"][:0], mn, nc, rt, device=False)


# ------------------------------------------------------------------------------------------------ the cases
def _bytes(v):
    if isinstance(v, torch.Tensor):
        return v.numpy().tobytes()
    if isinstance(v, np.ndarray):
        return v.tobytes()
    if isinstance(v, dict):
        return b"".join(_bytes(v[key]) for key in sorted(v))
    if isinstance(v, (tuple, list)):
        return b"".join(_bytes(x) for x in v)
    return repr(v).encode()


def test_case_builders_are_deterministic():
    assert tuple(K.keys_cases()) == K.KEYS_CASES and tuple(K.ball_cases()) == K.BALL_CASES      # the names the GPU tests list
    builders = [(K.keys_cases, ()), (K.ball_cases, ()), (K.fbp_graph, ()), (K.fbp_case, (16, 8)), (K.knn_case, ())]
    first = [_bytes(f(*a)) for f, a in builders]
    for f, _a in builders:
        f.cache_clear()
    assert first == [_bytes(f(*a)) for f, a in builders]


def test_grid_arguments_and_windows_agree_with_the_oracle():
    for name, c in K.ball_cases().items():
        mn, nc, rt = K.grid_params(c["pts_src"], c["batch_src"], c["radius"])
        o_mn, o_nc = O.ball_query_grid_params(c["pts_src"], c["batch_src"], c["radius"])
        assert mn.numpy().tobytes() == o_mn.numpy().tobytes() and torch.equal(nc, o_nc) and nc.dtype == torch.int32, name
        assert rt.dtype == torch.float32 and rt.tolist() == [float(np.float32(c["radius"]))] * 3
    for name in ("boundary", "exact_radius"):       # the vectorised windows are the oracle's restatement of the grid search
        c = K.ball_cases()[name]
        nb, ends = O.ball_query_grid(c["pts_src"], c["pts_dst"], c["batch_src"], c["batch_dst"], c["radius"])
        assert torch.equal(K.sorted_edges(nb, c["pts_src"].shape[0]), c["visible"]) and torch.equal(ends, c["visible_ends"]), name
    c = K.ball_cases()["boundary"]
    assert c["full"].numel() - c["visible"].numel() == c["planted"].shape[0] == 2 * 48
    for name, args in K.keys_cases().items():
        K.check_keys_domain(*args, device=False)
    sizes = sorted(v[0].shape[0] for v in K.keys_cases().values())
    assert sizes == [1, 257, 257, 3000] and {int(v[1].max()) + 1 for v in K.keys_cases().values()} == {1, 3}


def test_float64_references_agree_with_the_oracle():
    for k, c in ((8, 4), (32, 16), (64, 8)):
        d = K.fbp_case(k, c)
        _, ref = K.fbp_reference(k, c)
        t64 = lambda a: torch.from_numpy(np.asarray(a)).double()
        nb, ends = torch.from_numpy(d["neighbors"]).long(), torch.from_numpy(d["ends"])
        want_t = O.feat_basis_proj(t64(d["basis"]), t64(d["feat"]), nb, ends).numpy()
        want_gf, want_gb = O.feat_basis_proj_grad(t64(d["basis"]), t64(d["feat"]), nb, ends, t64(d["grad_t"]))
        for kind, want in (("T", want_t), ("g_basis", want_gb.numpy()), ("g_feat", want_gf.numpy())):
            value, scale = ref[kind]
            assert REF.worst(value, want, scale)[0] < 1e-13, (k, c, kind)
        K.check_fbp_domain(*(torch.from_numpy(d[key]) for key in ("basis", "feat", "neighbors", "ends", "grad_t")), device=False)
    gr = K.fbp_graph()
    deg = np.diff(np.concatenate([[0], gr["ends"]]))
    assert deg[gr["hub"]] == 3001 and deg[gr["one_edge"]] == 1 and (deg[:3] == 0).all() and (deg[-3:] == 0).all()
    assert not np.isin(gr["unreached"], gr["src"]).any()


# ------------------------------------------------------------------------------------------------ planted misreadings
def test_the_cases_show_the_misreadings_they_are_there_for():
    # `<=` for `<` at the radius: the lattice's axis neighbours lie at exactly one radius
    c = K.ball_cases()["exact_radius"]
    d = (c["pts_dst"][:, None, :] - c["pts_src"][None, :, :]) * torch.reciprocal(torch.tensor(c["radius"], dtype=torch.float32))
    dist = torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
    assert int((dist < 1.0).sum()) == c["full"].numel() == 125 and int((dist <= 1.0).sum()) == 125 + 2 * 300
    # a window of two cells to each side would list the planted pairs; the just-outside partners are one ulp from an edge
    c = K.ball_cases()["boundary"]
    apart = K.edge_cells_apart(c["neighbors"], c["pts_src"], c["pts_dst"], c["batch_src"], c["batch_dst"], c["radius"])
    assert int((apart == 2).sum()) == c["planted"].shape[0] and int(apart.max()) == 2
    # a neighbour loop that stops at the last whole pass of the block (128 / K edges), and groups of 8 channels that drop a
    # channel count's remainder, are far outside the bound
    for k in K.FBP_K:
        d = K.fbp_case(k, 8)
        bounds, ref = K.fbp_reference(k, 8)
        per_pass = K.REF_BLOCK // k
        starts = np.concatenate([[0], d["ends"][:-1]])
        keep = np.concatenate([np.arange(s, s + (e - s) // per_pass * per_pass) for s, e in zip(starts, d["ends"])])
        ends = np.cumsum((np.diff(np.concatenate([[0], d["ends"]])) // per_pass) * per_pass)
        short, _ = REF.feat_basis_proj(d["basis"][keep], d["feat"], d["src"][keep], ends, T=np.float32)
        assert REF.worst(short, *ref["T"])[0] > 1e3 * bounds["T"], k
    # ties broken to the higher index change ids only where distances repeat: the k-NN case has no such query, so ids compare
    pts, bid = K.knn_case()
    assert all(bool(K.knn_distinct(pts, bid, k).all()) for k in K.KNN_K)
    dup = torch.cat((pts[:6], pts[:6]))
    assert not bool(K.knn_distinct(dup, torch.zeros(12, dtype=torch.int32), 2).any())
