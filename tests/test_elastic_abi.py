"""CPU: include/se3conv_elastic.h against its ctypes table, the built library and its hostile-memory module -- the five checks of
tests/abi_tables.py (a to e), in the manner of tests/test_augment_abi.py -- the host-side argument checks, the constants, and
`AugPipeline(p_elastic=True)` built from the reference's ScanNet list with its elastic step."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_tables as T
import augment_configs as CFG
import augment_reference as R
import elastic_reference as E
from se3conv3d_amd import _lib, augment, build

HEADER = "se3conv_elastic.h"
NAMES = ("se3_elastic_displace", "se3_elastic_grids", "se3_elastic_plan", "se3_elastic_workspace_bytes")
HOST_ONLY = {"se3_elastic_workspace_bytes"}
PIN = T.Header("test_gpu_elastic_hostile_memory", HOST_ONLY, NAMES)
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
SCANNET_FULL = CFG.SCANNET[:6] + [CFG.SCANNET_ELASTIC] + CFG.SCANNET[6:]   # where ScanNet_DS_Aug.py has the step


@pytest.fixture
def placed(monkeypatch):
    monkeypatch.setitem(_lib.TABLES, HEADER, _lib.ELASTIC_SIGNATURES)
    monkeypatch.setitem(T.HEADERS, HEADER, PIN)
    return HEADER


def test_third_registry_holds_the_header():
    assert HEADER in _lib.EXTENSION_TABLES and _lib.EXTENSION_TABLES[HEADER] is _lib.ELASTIC_SIGNATURES
    assert HEADER not in _lib.TABLES and HEADER not in _lib.ADDED_TABLES
    assert HEADER in [os.path.basename(p) for p in build.EXTENSION_HEADERS] and os.path.exists(os.path.join(T.INCLUDE, HEADER))
    assert "elastic.hip" in build.SOURCES and build.SOURCES.index("elastic.hip") < build.SOURCES.index("api.hip")
    assert os.path.exists(os.path.join(build.CSRC, "elastic.hip")) and sorted(_lib.ELASTIC_SIGNATURES) == list(NAMES)


def test_a_header_and_table_agree(placed):
    T.check_header_and_table_agree(placed)
    assert T.declared(placed) == {"se3_elastic_workspace_bytes": 2, "se3_elastic_plan": 13, "se3_elastic_grids": 12, "se3_elastic_displace": 12}


def test_b_no_name_stands_in_any_two_tables(placed, monkeypatch):
    T.check_tables_are_disjoint()
    for header, table in list(_lib.ADDED_TABLES.items()) + [(h, t) for h, t in _lib.EXTENSION_TABLES.items() if h != placed]:
        monkeypatch.setitem(_lib.TABLES, header, table)
    T.check_tables_are_disjoint()


def test_c_library_exports_and_types_the_entry_points_inside_abi_version_6(built_library, placed):
    T.check_library_exports_and_types(placed, built_library)


def test_d_argument_counts_are_those_of_the_header(placed):
    T.check_argument_counts(placed)


def test_e_every_entry_point_with_a_device_pointer_is_covered_on_hostile_memory(placed):
    T.check_hostile_memory_coverage(placed)
    assert set(T.guard_module(placed).COVERED) == set(NAMES) - HOST_ONLY


def test_the_checks_can_fail_for_this_header(placed, monkeypatch):
    res, args = _lib.ELASTIC_SIGNATURES["se3_elastic_grids"]
    monkeypatch.setitem(_lib.ELASTIC_SIGNATURES, "se3_elastic_grids", (res, args[:-1]))
    with pytest.raises(AssertionError, match=r"se3_elastic_grids \(11 in the table, 12 in the header\)"):
        T.check_argument_counts(placed)


def test_constants_are_the_headers():
    text = open(os.path.join(T.INCLUDE, HEADER)).read()
    for name, value, restated in (("MAX_OCTAVES", _lib.ELASTIC_MAX_OCTAVES, E.MAX_OCTAVES), ("TILE", _lib.ELASTIC_TILE, E.TILE),
                                  ("MAX_QUOTIENT", _lib.ELASTIC_MAX_QUOTIENT, E.MAX_QUOTIENT)):
        assert int(re.search(r"#define SE3_ELASTIC_%s (\d+)" % name, text).group(1)) == value == restated
    assert _lib.ELASTIC_MAX_OCTAVES == 4 and len(CFG.SCANNET_ELASTIC["p_granularity"]) == 3
    source = open(os.path.join(build.CSRC, "elastic.hip")).read()
    assert "SE3_ELASTIC_TILE" in source and "fp contract(off)" in source and "atomic" not in source.replace("atomics", "")


def test_host_side_argument_checks(built_library):
    """Decided before the first launch: no GPU is touched by a refused call."""
    lib = _lib.load()
    null, p = C.c_void_p(0), C.c_void_p(16)
    oct3 = (C.c_double * 3)(0.1, 0.2, 0.4)
    nk = C.cast(null, C.POINTER(C.c_double))
    big = 1 << 20
    # the workspace query
    assert lib.se3_elastic_workspace_bytes(6, 3) >= 8 * (6 * 3 + 1)
    assert lib.se3_elastic_workspace_bytes(0, 3) == lib.se3_elastic_workspace_bytes(6, 0) == lib.se3_elastic_workspace_bytes(6, 5) == 0
    # plan

    def plan(counts=p, stats=p, draws=p, g=oct3, n_oct=3, nb=2, cap=100, table=p, over=p, ws=p, nbytes=big):
        return lib.se3_elastic_plan(counts, stats, draws, 1.0, g, n_oct, nb, cap, table, over, ws, nbytes, null)
    assert plan(n_oct=0) == plan(n_oct=5) == plan(nb=0) == plan(cap=-1) == INVALID
    assert plan(counts=null) == plan(stats=null) == plan(draws=null) == plan(g=nk) == plan(table=null) == plan(over=null) == plan(ws=null) == INVALID
    assert plan(g=(C.c_double * 3)(0.1, 0.0, 0.4)) == plan(g=(C.c_double * 3)(0.1, -1.0, 0.4)) == plan(g=(C.c_double * 3)(0.1, float("nan"), 0.4)) == INVALID
    assert plan(nbytes=lib.se3_elastic_workspace_bytes(2, 3) - 1) == WORKSPACE
    # grids

    def grids(table=p, nb=2, n_oct=3, cap=100, noise=null, grid=p, ws=p, nbytes=big):
        return lib.se3_elastic_grids(table, nb, n_oct, cap, 0, null, 0, noise, grid, ws, nbytes, null)
    assert grids(n_oct=0) == grids(n_oct=5) == grids(nb=0) == grids(cap=-1) == grids(table=null) == grids(grid=null) == grids(ws=null) == INVALID
    assert grids(nbytes=lib.se3_elastic_workspace_bytes(2, 3) - 1) == WORKSPACE
    # displace

    def displace(x=p, ids=p, n=10, nb=2, stats=p, table=p, n_oct=3, m=oct3, grid=p, y=p):
        return lib.se3_elastic_displace(x, ids, n, null, nb, stats, table, n_oct, m, grid, y, null)
    assert displace(n=-1) == displace(nb=0) == displace(n_oct=0) == displace(n_oct=5) == INVALID
    assert displace(x=null) == displace(ids=null) == displace(stats=null) == displace(table=null) == displace(m=nk) == displace(grid=null) == displace(y=null) == INVALID
    assert displace(n=1 << 31) == UNSUPPORTED
    assert displace(n=0, x=null, ids=null, y=null, grid=null) == 0                       # nothing to do: no launch


# ------------------------------------------------------------------------------------------------------------- the pipeline
def test_scannet_list_with_its_elastic_step():
    pipe = augment.AugPipeline(p_elastic=True)
    pipe.create_pipeline(SCANNET_FULL)
    assert len(pipe.pipeline_) == len(CFG.SCANNET) + 1 == 11 and [type(a).__name__ for a in pipe.pipeline_] == [c["name"] for c in SCANNET_FULL]
    assert set(pipe.aug_classes_) == set(augment.AugPipeline().aug_classes_) | {"ElasticDistortionAug"}
    for aug, cfg in zip(pipe.pipeline_, SCANNET_FULL):
        if cfg["name"] != "ElasticDistortionAug":   # the other ten: the constants of the restatement, as without the switch
            kind, consts, prob, noise, _ = R.spec_of(cfg)
            assert aug.kind_ == kind and float(aug.prob_) == prob
            if kind != "noise":
                assert np.array_equal(np.pad(np.asarray(aug._consts(), dtype=np.float64), (0, R.CONSTS))[:R.CONSTS], consts)
            continue
        assert aug.kind_ == "elastic" and aug.prob_ == 0.95 and aug.epoch_iter_ == 0
        assert aug.granularity_ == [0.1, 0.2, 0.4] and aug.magnitude_ == [0.15, 0.3, 0.6] and aug._consts() == [0.1, 0.2, 0.4, 0.15, 0.3, 0.6]
        assert list(aug.apply_extra_tensors_) == [False] * 4
        assert len(aug.granularity_) <= E.MAX_OCTAVES
    assert pipe.removes_points()
    # a bound for the grid from a box on the host: the scaled diagonal on every axis, per octave
    d = 1.25 * np.sqrt(8.0 ** 2 + 6.0 ** 2 + 3.0 ** 2)
    assert pipe.elastic_capacity((8.0, 6.0, 3.0), 6) == 6 * sum((int(d / g) + 4) ** 3 for g in (0.1, 0.2, 0.4))
    assert augment.AugPipeline().elastic_capacity((8.0, 6.0, 3.0)) == 0


def test_the_class_takes_the_references_keywords():
    aug = augment.ElasticDistortionAug()
    assert (aug.prob_, aug.granularity_, aug.magnitude_, aug.apply_extra_tensors_) == (1.0, [0.1], [0.2], [])
    for bad in ({"p_granularity": [0.1, 0.2], "p_magnitude": [0.2]}, {"p_granularity": [0.1] * 5, "p_magnitude": [0.2] * 5},
                {"p_granularity": [], "p_magnitude": []}, {"p_granularity": [0.0], "p_magnitude": [0.2]}):
        with pytest.raises(ValueError, match="ElasticDistortionAug"):
            augment.ElasticDistortionAug(**bad)


def test_the_default_pipeline_still_refuses():
    pipe = augment.AugPipeline()
    with pytest.raises(NotImplementedError, match="ElasticDistortionAug is not implemented on the device"):
        pipe.create_pipeline(SCANNET_FULL)
    assert pipe.pipeline_ == [] and "ElasticDistortionAug" not in pipe.aug_classes_ and len(pipe.aug_classes_) == 11
    assert augment.AugPipeline(p_elastic=False).elastic_ is False


def test_a_pipeline_with_the_step_needs_a_grid_capacity(monkeypatch):
    import torch
    pipe = augment.AugPipeline(p_elastic=True)
    pipe.create_pipeline([CFG.SCANNET_ELASTIC])
    monkeypatch.setattr(augment, "_cloud", lambda pts, ids, who: (pts.device, int(pts.shape[0])))   # (no GPU here: the check under test comes right behind)
    for cap in (None, -1):
        with pytest.raises(ValueError, match="grid_capacity"):
            pipe.augment_batch(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32), 1, grid_capacity=cap)
