"""CPU: the plans behind a fused call (se3conv3d_amd/csrc/api.hip: FwdPlan, BwdPlan) answer the host-only queries --
workspace sizes, whether backward reads T, the row formats -- exactly as recorded in tests/golden/workspace_plan.npz
(tools/gen_golden.py workspace_plan, from the library as it was before the plans replaced the layouts): callers cache
these sizes, and every decision of a call shows in one of them.  3240 shapes under each of the four environments."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from workspace_plan_table import COLUMNS, ENVIRONMENTS, shapes, table_in_child


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(GOLDEN, "workspace_plan.npz")) as z:
        return {k: z[k] for k in z.files}


def test_fixture_covers_the_grid_and_both_sides_of_every_switch(recorded):
    assert sorted(recorded) == sorted(ENVIRONMENTS)
    n = len(list(shapes()))
    assert n == 3240
    for name, tab in recorded.items():
        assert tab.shape == (n, len(COLUMNS)) and tab.dtype == np.int64, name
    differing = {k: int((recorded[k] != recorded["default"]).any(axis=1).sum()) for k in ENVIRONMENTS}
    assert differing == {"default": 0, "dx_path_0": 384, "dx_path_1": 546, "no_t24": 490}


@pytest.mark.parametrize("env", list(ENVIRONMENTS))
def test_queries_match_the_recorded_table(built_library, recorded, env):
    got = table_in_child(ENVIRONMENTS[env])
    want = recorded[env]
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    if len(bad):
        all_shapes = list(shapes())
        lines = [f"{all_shapes[r]}: {COLUMNS[c]} = {got[r, c]}, recorded {want[r, c]}" for r, c in bad[:20]]
        pytest.fail(f"{len(bad)} entries differ under {ENVIRONMENTS[env] or 'no switch'}; the first:\n" + "\n".join(lines))
