"""CPU: when backward's dense products share a launch (api.hip: plan_dense_shared), asked of se3conv_forms.

The line "bwd_dense_shared:one_launch" appears exactly where a call runs two or three of gemm_gradT / gemm_gradX / gemm_gradW
on a level under the row gate, in the split-bf16 modes, over rows the shared kernel has a body for; each product keeps
reporting its own form line."""
import pytest

import form_coverage_table as FC

SHARED = "bwd_dense_shared:one_launch"
DENSE = {"gemm_gradT", "gemm_gradX", "gemm_gradW"}
GATE = 32768                                                  # kDenseShareRows (common.h): rows of either side
# precision-less shapes (n_in, n_out, n_edges, F_in, F_out, C_in, C_out): under the gate, at it, beyond it, the headline's level 0
SMALL = [(37, 37, 37 * 30, 2, 2, 64, 64), (300, 300, 3600, 2, 2, 64, 64), (9207, 9207, 9207 * 27, 2, 2, 64, 64),
         (600, 150, 9000, 2, 2, 32, 64), (150, 600, 1800, 1, 3, 64, 32), (16384, 16384, 16384 * 24, 2, 2, 64, 64)]
LARGE = [(16385, 16385, 16385 * 24, 2, 2, 64, 64), (65536, 65536, 65536 * 30, 2, 2, 64, 64), (65536, 9207, 9207 * 30, 2, 2, 64, 64),
         (9207, 65536, 65536 * 4, 2, 2, 64, 64)]


def dense_stages(lines):
    return {line.split(":", 1)[0] for line in lines} & DENSE


@pytest.mark.parametrize("shape", SMALL)
def test_line_appears_exactly_for_multi_role_requests_under_the_gate(built_library, shape):
    assert max(shape[0] * shape[3], shape[1] * shape[4]) <= GATE
    shared_somewhere = False
    for request in FC.BACKWARD:
        lines = FC.lines(("bf16x3",) + shape, request)
        roles = dense_stages(lines)
        assert (SHARED in lines) == (len(roles) >= 2), (shape, request, lines)
        assert lines.count(SHARED) <= 1
        shared_somewhere |= SHARED in lines
        if SHARED in lines:  # each role reports its own form, the sharing line follows the last of them and precedes its readers
            at = lines.index(SHARED)
            assert all(lines.index(next(l for l in lines if l.startswith(r + ":"))) < at for r in roles), lines
            assert all(lines.index(l) > at for l in lines if l.startswith(("edge_dx:", "edge_param_grad:", "reductions:"))), lines
    assert shared_somewhere
    assert SHARED not in FC.lines(("bf16x3",) + shape, FC.FEAT_ONLY)      # one product
    assert SHARED not in FC.lines(("bf16x3",) + shape, ("fwd", 0, 0, 1))


@pytest.mark.parametrize("shape", LARGE)
def test_line_never_appears_beyond_the_gate(built_library, shape):
    assert max(shape[0] * shape[3], shape[1] * shape[4]) > GATE
    for precision in FC.PRECISIONS:
        for request in FC.BACKWARD:
            assert SHARED not in FC.lines((precision,) + shape, request), (precision, shape, request)


def test_headline_level_0_keeps_its_launches_and_its_stage_names(built_library):
    lines = FC.lines(("bf16x3", 65536, 65536, 65536 * 30, 2, 2, 64, 64), FC.BOTH_WITHOUT_T)   # 131 072 rows
    assert SHARED not in lines and dense_stages(lines) == DENSE


@pytest.mark.parametrize("shape", SMALL + LARGE)
def test_line_never_appears_in_fp32(built_library, shape):
    for request in FC.BACKWARD:
        assert SHARED not in FC.lines(("fp32",) + shape, request), (shape, request)


def test_t16_rows_and_wide_tiles_keep_their_own_launches(built_library):
    """Out of scope of the shared kernel: products over T16 rows (gemm_nn_t16, gemm_tn_bf16<afmt=2>) and the 128-column NN forms."""
    for precision in FC.PRECISIONS:
        for shape in SMALL + [(300, 300, 9000, 1, 1, 128, 128), (300, 300, 9000, 3, 3, 256, 64)]:
            for request in FC.BACKWARD:
                lines = FC.lines((precision,) + shape, request)
                if SHARED in lines:
                    dense = [l for l in lines if l.split(":", 1)[0] in DENSE]
                    assert not any("t16" in l or "afmt=2" in l or "nb=2" in l or "fast=0" in l for l in dense), (precision, shape, request, dense)
