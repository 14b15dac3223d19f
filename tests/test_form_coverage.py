"""CPU: every kernel form the fused operator can pick is run against the fp64 oracle by some table of the GPU suite.

se3conv_fwd / se3conv_bwd do not run one kernel each: every launcher picks one of several template instantiations from the
shape.  `se3conv_forms` (include/se3conv_forms.h) reports the launchers' own decisions without touching a device;
tests/form_coverage_table.py sweeps it over a grid of shapes (the universe) and over the shapes of the suite's case tables
under the requests their tests make (covered).  A form in the universe that no table reaches fails here, by name and with a
shape that reaches it: the author of a new kernel form is told which case to add to FORM_CASES (tests/test_gpu_parity.py).
The same holds under every switch environment of tests/test_gpu_variants.py, in a child process each."""
import functools

import pytest
import torch

import form_coverage_table as FC
import test_gpu_parity as P
import test_gpu_variants as V
from oracle import se3conv_oracle as O

# Forms that only a size selects, each with the full-size or variant test that runs it.  Only these size gates may appear:
# the chunk-stream edge kernels below 4096 items, the parameter-gradient kernel's per-item extent loads below 64 items per
# resident workgroup, the row-block loop of the dense products beyond 32-bit offsets.  Anything else gets a case.
VARIANT_STREAM = "tests/test_gpu_variants.py::test_variant_passes_parity_slice[SE3_DX_PATH=1,SE3_EDGE_STREAM=1]"
EXCLUSIONS = [
    # chunk-stream forms: items >= 4096 (SE3_EDGE_STREAM=1 lowers the gate to one item for the variant child's small cases)
    ("edge_t_stream_pair<tr=0>", "tests/test_gpu_parity.py::test_headline_subset_against_oracle (65 536 items, forward) and " + VARIANT_STREAM),
    ("edge_t_stream1<vw=1,fc=2,tr=0>", "tests/test_gpu_parity.py::test_dfaust_like_four_frames_batched (32-channel rows, 13 800 items) and " + VARIANT_STREAM),
    ("edge_t_stream1<vw=1,fc=2,tr=1>", VARIANT_STREAM + " (CASES seed 12: U rows of 32 channels)"),
]


@functools.lru_cache(maxsize=None)
def per_mode():
    return {p: (FC.universe((p,)), FC.covered((p,))) for p in FC.PRECISIONS}


@functools.lru_cache(maxsize=None)
def default_environment():
    universe, covered = {}, {}
    for u, c in per_mode().values():
        universe.update({k: v for k, v in u.items() if k not in universe})
        covered.update({k: v for k, v in c.items() if k not in covered})
    return universe, covered


def report(universe, covered, excluded=()):
    missing = sorted(set(universe) - set(covered) - set(excluded))
    return "\n".join(f"  {name}: reached by (precision, n_in, n_out, n_edges, F_in, F_out, C_in, C_out) = {tuple(universe[name][0])} "
                     f"under (pass, want_feat, want_params, have_t) = {tuple(universe[name][1])}" for name in missing)


def test_exclusions_are_few_size_gated_and_name_their_test(built_library):
    assert len(EXCLUSIONS) <= 12
    universe, covered = default_environment()
    for name, where in EXCLUSIONS:
        assert name.startswith(("edge_t_stream", "gemm_nn_row_blocks")) or "/loop/" in name, f"{name} is not gated by size"
        assert "::test_" in where, name
        assert name not in covered, f"{name} is run by {covered.get(name)}: drop the exclusion"


def test_every_form_of_the_universe_is_run_by_a_table(built_library):
    universe, covered = default_environment()
    counts = {p: (len(u), len(set(u) & set(c))) for p, (u, c) in per_mode().items()}
    print(f"forms in the universe: {len(universe)}; per arithmetic mode (universe, reached by the tables in that mode): {counts}")
    missing = report(universe, covered, [name for name, _ in EXCLUSIONS])
    assert not missing, "kernel forms the library can pick that no table of the GPU suite runs -- add a row to FORM_CASES:\n" + missing


@pytest.mark.parametrize("var", V.VARIANTS)
def test_every_form_under_a_switch_is_run_by_the_variant_slice(built_library, var):
    """The same under the switches of one child of tests/test_gpu_variants.py, in a child process: the universe swept in
    bf16x3 (the mode the children run: the switches act on the split-bf16 kernels) under those switches; covered: what that
    child runs, i.e. the tables of the tests its SLICE selects, in bf16x3, under the same switches -- and nothing else."""
    switches = dict((part.partition("=")[0], part.partition("=")[2] or "1") for part in var.split(","))
    child = FC.in_child(switches)
    missing = report(child["universe"], child["covered"], [name for name, _ in EXCLUSIONS])
    assert not missing, f"under {var}: forms that the child's slice does not run:\n" + missing
    if "SE3_EDGE_STREAM" in switches:   # the gate lifted: this child is where the excluded stream forms run at table sizes
        assert {name for name, _ in EXCLUSIONS if name.startswith("edge_t_stream")} <= set(child["covered"])


def test_query_pins_forms_that_read_straight_off_the_source(built_library):
    f = lambda shape, request: FC.lines(shape, request)
    # headline level 0 (65 536 points, 30 edges each, F = 2, 64 -> 64): the chunk-stream pair writes T and U
    head = ("bf16x3", 65536, 65536, 65536 * 30, 2, 2, 64, 64)
    assert "edge_t_fwd:edge_t_stream_pair<tr=0>" in f(head, ("fwd", 0, 0, 0))
    assert "edge_t_transposed:edge_t_stream_pair<tr=1>" in f(head, FC.BOTH_WITHOUT_T)
    # the class head 64 -> 13: C_out % 4 != 0 keeps T in packed words (fmt0) behind the wide kernels, and the TN product scalar
    assert "edge_t_fwd:edge_t_pair<ct=1,full=1,nf=2,p2=1,tr=0>/fmt0" in f(("bf16x3", 300, 300, 3600, 2, 2, 64, 13), ("fwd", 0, 0, 0))
    assert "edge_t_fwd:edge_t_single<vw=2,fc=1,full=1,t24=0>/p2=1" in f(("bf16x3", 300, 300, 3600, 1, 1, 64, 13), ("fwd", 0, 0, 0))
    assert "gemm_gradW:gemm_tn_bf16<fast=0,afmt=0>" in f(("bf16x3", 300, 300, 3600, 2, 2, 64, 13), FC.PARAMS_WITH_T)
    assert "gemm_gradW:gemm_tn_bf16<fast=0,afmt=0>" in f(("bf16x3", 300, 300, 3600, 1, 1, 64, 13), FC.PARAMS_WITH_T)
    # F = 3: the division forms everywhere
    for prec in FC.PRECISIONS:
        for request in FC.FORWARD + FC.BACKWARD:
            for line in f((prec, 300, 300, 3600, 3, 3, 64, 64), request):
                assert "p2=1" not in line, line
    # (64-channel rows with an odd frame count stay with the single wavefront; 128-channel rows take the pair)
    assert "edge_t_fwd:edge_t_single<vw=2,fc=1,full=1,t24=1>/p2=0" in f(("bf16x3", 300, 300, 3600, 3, 3, 64, 64), ("fwd", 0, 0, 0))
    assert "edge_t_fwd:edge_t_pair<ct=2,full=1,nf=1,p2=0,tr=-1>/fmt1" in f(("bf16x3", 300, 300, 3600, 3, 3, 128, 64), ("fwd", 0, 0, 0))
    # launch order (a split product and its reduction are two lines of one stage), K != 32 as its inner K = 32 calls
    assert f(("fp32", 300, 300, 3600, 2, 2, 64, 64), ("fwd", 0, 0, 0)) == [
        "prep:prep_batch", "edge_t_fwd:edge_t<vw=2>/p2=1", "gemm_out:gemm_nn_fast/split", "gemm_out:reduce_partials"]
    assert f(("bf16x3", 300, 120, 2000, 2, 1, 24, 40, 70), ("fwd", 0, 0, 0)) == 3 * f(("bf16x3", 300, 120, 2000, 2, 1, 24, 40, 32), ("fwd", 0, 0, 0))


# ------------------------------------------------------------------------- what keeps a division form from passing while wrong
@functools.lru_cache(maxsize=None)
def graph_of(case):
    c = P.random_case(*case)
    nb, _ = O.ball_query(c["pts_in"], c["pts_out"], c["bid_in"], c["bid_out"], c["r"])
    return torch.bincount(nb[:, 0], minlength=c["pts_out"].shape[0]), torch.bincount(nb[:, 1], minlength=c["pts_in"].shape[0])


def test_every_division_form_meets_split_chunks_and_holes(built_library):
    """Every form with p2=0 (a neighbour frame count that is no power of two: an edge's frames are found by division) is reached
    (a) by a case where, for most centres, edges x F_nb exceeds 32 without being a multiple of it -- chunk boundaries then fall
    inside an edge's frames -- and (b) by a two-cloud case with samples without a neighbour and sources without an edge."""
    universe, _ = default_environment()
    division = {name for name in universe if "p2=0" in name}
    assert len(division) >= 30
    split, holes = set(), set()
    for case in P.FORM_CASES + P.CASES:
        deg_out, deg_in = graph_of(case)
        two_clouds_with_holes = case[2] is not None and int((deg_out == 0).sum()) > 0 and int((deg_in == 0).sum()) > 0
        for prec in FC.PRECISIONS:
            shape = FC.generated_shape(case, prec)
            requests = FC.module_requests(shape) + (FC.other_requests(case, prec) if case in P.FORM_CASES else [])
            for request in requests:
                for line in FC.lines(shape, request):
                    stage, name = line.split(":", 1)
                    if name not in division:
                        continue
                    deg, f_nb = (deg_in, case[4]) if stage == "edge_t_transposed" else (deg_out, case[3])
                    fe = deg * f_nb
                    if float(((fe > 32) & (fe % 32 != 0)).float().mean()) > 0.5:
                        split.add(name)
                    if two_clouds_with_holes:
                        holes.add(name)
    assert not division - split, f"division forms never run with chunk boundaries inside an edge's frames: {sorted(division - split)}"
    assert not division - holes, f"division forms never run on a two-cloud graph with holes: {sorted(division - holes)}"


def test_form_cases_keep_the_shapes_the_table_was_asked_for():
    pairs = {(c[3], c[4]) for c in P.FORM_CASES}
    assert {(3, 2), (2, 3), (1, 3), (3, 1)} <= pairs
    assert any(c[2] is None and c[3] == c[4] == 6 for c in P.FORM_CASES)                      # F = 6 on one cloud
    assert 3 * sum(c[8] in (2, 3) for c in P.FORM_CASES) >= len(P.FORM_CASES)               # a third with 2-3 batch elements
    heads = {(c[3], c[5], c[6]) for c in P.FORM_CASES if c[3] == c[4]}
    assert {(1, 64, 13), (2, 64, 13)} <= heads and any(c[5] == 128 and c[6] == 13 for c in P.FORM_CASES)
