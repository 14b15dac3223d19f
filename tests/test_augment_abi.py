"""CPU: include/se3conv_augment.h against its ctypes table, the built library and its hostile-memory module -- the five checks
of tests/abi_tables.py (a to e), in the manner of tests/test_global_pool_abi.py -- the host-side argument checks, the hash's check
vectors, and `AugPipeline` built from the reference's own config lists (tests/augment_configs.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_tables as T
import augment_configs as CFG
import augment_reference as R
from se3conv3d_amd import _lib, augment, build

HEADER = "se3conv_augment.h"
NAMES = ("se3_aug_affine_step", "se3_aug_apply", "se3_aug_compact", "se3_aug_compact_workspace_bytes", "se3_aug_keep_mask",
         "se3_aug_stats", "se3_aug_stats_workspace_bytes")
HOST_ONLY = {"se3_aug_stats_workspace_bytes", "se3_aug_compact_workspace_bytes"}
PIN = T.Header("test_gpu_augment_hostile_memory", HOST_ONLY, NAMES)
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


@pytest.fixture
def placed(monkeypatch):
    monkeypatch.setitem(_lib.TABLES, HEADER, _lib.AUGMENT_SIGNATURES)
    monkeypatch.setitem(T.HEADERS, HEADER, PIN)
    return HEADER


def test_third_registry_holds_the_header():
    assert _lib.EXTENSION_TABLES[HEADER] is _lib.AUGMENT_SIGNATURES
    assert HEADER not in _lib.TABLES and HEADER not in _lib.ADDED_TABLES
    assert list(_lib.EXTENSION_TABLES)[-1] == "se3conv_pne.h"                     # the marked line stays the last one
    assert [os.path.basename(p) for p in build.EXTENSION_HEADERS] == list(_lib.EXTENSION_TABLES) and all(os.path.exists(p) for p in build.EXTENSION_HEADERS)
    assert "augment.hip" in build.SOURCES and sorted(_lib.AUGMENT_SIGNATURES) == list(NAMES)


def test_a_header_and_table_agree(placed):
    T.check_header_and_table_agree(placed)
    assert T.declared(placed) == {"se3_aug_stats_workspace_bytes": 2, "se3_aug_stats": 11, "se3_aug_affine_step": 9, "se3_aug_apply": 18,
                                  "se3_aug_keep_mask": 15, "se3_aug_compact_workspace_bytes": 1, "se3_aug_compact": 13}


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
    res, args = _lib.AUGMENT_SIGNATURES["se3_aug_compact"]
    monkeypatch.setitem(_lib.AUGMENT_SIGNATURES, "se3_aug_compact", (res, args[:-1]))
    with pytest.raises(AssertionError, match=r"se3_aug_compact \(12 in the table, 13 in the header\)"):
        T.check_argument_counts(placed)


def test_constants_are_the_headers():
    text = open(os.path.join(T.INCLUDE, HEADER)).read()
    for name, value in (("CHUNK", _lib.AUG_CHUNK), ("DRAWS", _lib.AUG_DRAWS), ("CONSTS", _lib.AUG_CONSTS)):
        assert int(re.search(r"#define SE3_AUG_%s (\d+)" % name, text).group(1)) == value == getattr(R, name)
    body = re.search(r"enum se3_aug_kind \{(.*?)\};", text, flags=re.S).group(1)
    enum = dict((k.lower(), int(v)) for k, v in re.findall(r"SE3_AUG_(\w+) = (\d+)", body))
    assert enum == _lib.AUG_KINDS == R.KINDS


def test_hash_check_vectors():
    text = open(os.path.join(T.INCLUDE, HEADER)).read()
    vectors = re.findall(r"\((\d+),(\d+),(\d+),(\d+)\) -> (0x[0-9a-f]+)", text)
    assert len(vectors) == 3
    for seed, step, row, j, want in vectors:
        assert int(R.word(int(seed), int(step), int(row), int(j))) == int(want, 16)
    # ... and the hash underneath is the capped query's, by its own vectors (include/se3conv_capped.h)
    capped = open(os.path.join(T.INCLUDE, "se3conv_capped.h")).read()
    for seed, s, p, want in re.findall(r"`\((\w+),(\d+),(\d+)\) -> (0x[0-9a-f]+)`", capped):
        assert int(R.h(int(seed, 0), int(s), int(p))) == int(want, 16)
    u = R.uniform(np.array([0, 0xFF, 0x100, 0xFFFFFFFF], dtype=np.uint32))
    assert u.tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]


def test_host_side_argument_checks(built_library):
    """Decided before the first launch: no GPU is touched by a refused call."""
    lib = _lib.load()
    null, p = C.c_void_p(0), C.c_void_p(16)
    k = (C.c_double * _lib.AUG_CONSTS)()
    nk = C.cast(null, C.POINTER(C.c_double))
    big = 1 << 20
    # statistics
    assert lib.se3_aug_stats(p, p, -1, null, 1, null, p, p, p, big, null) == INVALID
    assert lib.se3_aug_stats(p, p, 10, null, 0, null, p, p, p, big, null) == INVALID
    assert lib.se3_aug_stats(null, p, 10, null, 1, null, p, p, p, big, null) == INVALID
    assert lib.se3_aug_stats(p, p, 10, null, 1, null, null, p, p, big, null) == INVALID
    assert lib.se3_aug_stats(p, p, 10, null, 1, null, p, p, null, big, null) == INVALID
    assert lib.se3_aug_stats(p, p, 1 << 31, null, 1, null, p, p, p, big, null) == UNSUPPORTED
    need = lib.se3_aug_stats_workspace_bytes(1000, 3)
    assert need > 0 and lib.se3_aug_stats(p, p, 1000, null, 3, null, p, p, p, need - 1, null) == WORKSPACE
    assert lib.se3_aug_stats_workspace_bytes(-1, 1) == lib.se3_aug_stats_workspace_bytes(5, 0) == lib.se3_aug_stats_workspace_bytes(1 << 31, 1) == 0
    assert lib.se3_aug_stats_workspace_bytes(0, 1) > 0
    # the affine table
    assert lib.se3_aug_affine_step(0, k, 1.0, p, null, null, 0, p, null) == INVALID
    assert lib.se3_aug_affine_step(7, k, 1.0, p, null, null, 2, p, null) == INVALID           # no such kind
    assert lib.se3_aug_affine_step(-1, k, 1.0, p, null, null, 2, p, null) == INVALID
    assert lib.se3_aug_affine_step(0, nk, 1.0, p, null, null, 2, p, null) == INVALID
    assert lib.se3_aug_affine_step(0, k, 1.0, null, null, null, 2, p, null) == INVALID
    assert lib.se3_aug_affine_step(0, k, 1.0, p, null, null, 2, null, null) == INVALID
    for kind in (2, 5, 6):                                                                    # kinds that need statistics
        assert lib.se3_aug_affine_step(kind, k, 1.0, p, null, p, 2, p, null) == INVALID
        assert lib.se3_aug_affine_step(kind, k, 1.0, p, p, null, 2, p, null) == INVALID
    k[0] = 3.0
    assert lib.se3_aug_affine_step(0, k, 1.0, p, null, null, 2, p, null) == INVALID           # axis 3
    k[0] = 0.0
    # apply
    assert lib.se3_aug_apply(p, p, -1, null, 1, null, 0, null, 0, 0, -1, 1, 0, null, 0, null, p, null) == INVALID
    assert lib.se3_aug_apply(p, p, 5, null, 0, null, 0, null, 0, 0, -1, 1, 0, null, 0, null, p, null) == INVALID
    assert lib.se3_aug_apply(null, p, 5, null, 1, null, 0, null, 0, 0, -1, 1, 0, null, 0, null, p, null) == INVALID
    assert lib.se3_aug_apply(p, p, 5, null, 1, null, 0, null, 0, 0, -1, 1, 0, null, 0, null, null, null) == INVALID
    assert lib.se3_aug_apply(p, p, 1 << 31, null, 1, null, 0, null, 0, 0, -1, 1, 0, null, 0, null, p, null) == UNSUPPORTED
    # masks
    assert lib.se3_aug_keep_mask(16, k, 1.0, p, p, -1, null, 1, p, null, 0, null, 0, p, null) == INVALID
    assert lib.se3_aug_keep_mask(15, k, 1.0, p, p, 5, null, 1, p, null, 0, null, 0, p, null) == INVALID
    assert lib.se3_aug_keep_mask(19, k, 1.0, p, p, 5, null, 1, p, null, 0, null, 0, p, null) == INVALID
    assert lib.se3_aug_keep_mask(16, nk, 1.0, p, p, 5, null, 1, p, null, 0, null, 0, p, null) == INVALID
    assert lib.se3_aug_keep_mask(16, k, 1.0, p, p, 5, null, 1, null, null, 0, null, 0, p, null) == INVALID
    assert lib.se3_aug_keep_mask(17, k, 1.0, p, p, 5, null, 1, p, null, 0, null, 0, p, null) == INVALID   # a box needs the AABB
    assert lib.se3_aug_keep_mask(16, k, 1.0, p, p, 5, null, 1, p, null, 0, null, 0, null, null) == INVALID
    assert lib.se3_aug_keep_mask(18, k, 1.0, p, p, 1 << 31, null, 1, p, null, 0, null, 0, p, null) == UNSUPPORTED
    # compaction
    assert lib.se3_aug_compact(p, p, -1, null, 1, null, p, null, p, p, p, big, null) == INVALID
    assert lib.se3_aug_compact(p, p, 5, null, 0, null, p, null, p, p, p, big, null) == INVALID
    assert lib.se3_aug_compact(null, p, 5, null, 1, null, p, null, p, p, p, big, null) == INVALID
    assert lib.se3_aug_compact(p, p, 5, null, 1, null, null, null, p, p, p, big, null) == INVALID
    assert lib.se3_aug_compact(p, p, 5, null, 1, null, p, null, null, p, p, big, null) == INVALID
    assert lib.se3_aug_compact(p, p, 5, null, 1, null, p, null, p, p, null, big, null) == INVALID
    need = lib.se3_aug_compact_workspace_bytes(1000)
    assert need >= 8000 and lib.se3_aug_compact(p, p, 1000, null, 1, null, p, null, p, p, p, need - 1, null) == WORKSPACE
    assert lib.se3_aug_compact_workspace_bytes(-1) == lib.se3_aug_compact_workspace_bytes(1 << 31) == 0
    assert b"workspace" in lib.se3_error_string(WORKSPACE)


# ------------------------------------------------------------------------------------------------------------- the pipeline
@pytest.mark.parametrize("name", ["DFAUST", "MN40", "SCANNET", "SCANNET_TEST"])
def test_pipeline_from_the_reference_config_lists(name):
    cfgs = getattr(CFG, name)
    pipe = augment.AugPipeline()
    pipe.create_pipeline(cfgs)
    assert [type(a).__name__ for a in pipe.pipeline_] == [c["name"] for c in cfgs]
    assert pipe.removes_points() == (name == "SCANNET")
    for aug, cfg in zip(pipe.pipeline_, cfgs):   # the constants the classes hand the library are those of the restatement
        kind, consts, prob, noise, keep_zeros = R.spec_of(cfg)
        assert aug.kind_ == kind and float(aug.prob_) == prob and aug.epoch_iter_ == 0
        assert list(aug.apply_extra_tensors_) == list(cfg["p_apply_extra_tensors"])
        if kind == "noise":
            assert (aug.stddev_, aug.clip_) == (cfg["p_stddev"], cfg["p_clip"])
        else:
            assert np.array_equal(np.pad(np.asarray(aug._consts(), dtype=np.float64), (0, R.CONSTS))[:R.CONSTS], consts)


def test_epoch_tables_of_the_test_time_sweep():
    pipe = augment.AugPipeline()
    pipe.create_pipeline(CFG.SCANNET_TEST)
    rot = pipe.pipeline_[1]
    for epoch in range(CFG.NUM_TEST_EPOCHS):
        assert rot.epoch_iter_ == epoch and rot._consts() == [2, CFG.SCANNET_TEST[1]["p_angle_values"][epoch], 0.0, 1.0]
        assert np.array_equal(R.spec_of(CFG.SCANNET_TEST[1], epoch)[1][:4], rot._consts())
        pipe.increase_epoch_counter()
    pipe.reset_epoch_counter()
    assert [a.epoch_iter_ for a in pipe.pipeline_] == [0, 0]
    lin = augment.LinearAug(p_a_values=[[1.0, 2.0, 3.0], 0.5], p_b_values=[0.0, [0.1, 0.2, 0.3]])
    assert lin._consts()[5:] == [1.0, 1.0, 2.0, 3.0, 0.0, 0.0, 0.0]
    lin.increase_epoch_counter()
    assert lin._consts()[5:] == [1.0, 0.5, 0.5, 0.5, 0.1, 0.2, 0.3]


def test_names_the_library_does_not_have_are_refused():
    pipe = augment.AugPipeline()
    with pytest.raises(NotImplementedError, match="ElasticDistortionAug"):
        pipe.create_pipeline(CFG.SCANNET[:6] + [CFG.SCANNET_ELASTIC] + CFG.SCANNET[6:])
    with pytest.raises(KeyError, match="unknown augmentation 'JitterAug'"):
        pipe.create_pipeline([{"name": "JitterAug"}])
    assert pipe.pipeline_ == []                                                   # a refused list leaves no half pipeline
    with pytest.raises(NotImplementedError):
        pipe.create_pipeline([{"name": "CenterAug", "p_method": "max"}])
    assert set(pipe.aug_classes_) == {"RotationAug", "RotationAug3D", "CenterAug", "LinearAug", "MirrorAug", "TranslationAug", "STDDevNormAug",
                                      "NoiseAug", "DropAug", "CropBoxAug", "CropPtsAug"}


def test_cpu_tensors_are_refused():
    import torch
    pipe = augment.AugPipeline()
    pipe.create_pipeline(CFG.DFAUST)
    with pytest.raises(ValueError, match="no CPU fallback"):
        pipe.augment_batch(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32), 1)
    with pytest.raises(ValueError, match="no CPU fallback"):
        pipe.augment(torch.zeros(4, 3))
