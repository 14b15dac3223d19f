"""The reference's own augmentation lists as plain data (a helper module, not a conftest): tasks/SemSeg/confs/dfaust/DFaust_DS_Aug.py,
tasks/Classification/confs/MN40_DS_Aug.py, tasks/SemSeg/confs/scannet/ScanNet_DS_Aug.py and ScanNet_DS_Aug_Test.py.  SCANNET is
the training list without its ElasticDistortionAug entry (kept apart as SCANNET_ELASTIC): that step is not implemented."""
import numpy as np

DFAUST = [
    {"name": "CenterAug", "p_apply_extra_tensors": []},
    {"name": "NoiseAug", "p_prob": 1.0, "p_stddev": 0.005, "p_clip": 0.02, "p_apply_extra_tensors": []},
]
MN40 = [
    {"name": "CenterAug", "p_apply_extra_tensors": [False]},
    {"name": "RotationAug3D", "p_prob": 1.0, "p_apply_extra_tensors": [True]},
    {"name": "NoiseAug", "p_prob": 1.0, "p_stddev": 0.005, "p_clip": 0.02, "p_apply_extra_tensors": [False]},
    {"name": "LinearAug", "p_prob": 1.0, "p_min_a": 0.9, "p_max_a": 1.1, "p_min_b": 0.0, "p_max_b": 0.0, "p_channel_independent": True,
     "p_apply_extra_tensors": [False]},
    {"name": "MirrorAug", "p_prob": 1.0, "p_mirror_prob": 0.5, "p_axes": [True, False, True], "p_apply_extra_tensors": [True]},
]
SCANNET_ELASTIC = {"name": "ElasticDistortionAug", "p_prob": 0.95, "p_granularity": [0.1, 0.2, 0.4], "p_magnitude": [0.15, 0.3, 0.6],
                   "p_apply_extra_tensors": [False, False, False, False]}
SCANNET = [
    {"name": "CenterAug", "p_apply_extra_tensors": [False, False, False, False]},
    {"name": "MirrorAug", "p_prob": 1.0, "p_mirror_prob": 0.5, "p_axes": [True, True, False], "p_apply_extra_tensors": [True, False, False, False]},
    {"name": "RotationAug", "p_prob": 1.0, "p_axis": 2, "p_min_angle": 0.0, "p_max_angle": 2.0 * np.pi,
     "p_apply_extra_tensors": [True, False, False, False]},
    {"name": "RotationAug", "p_prob": 1.0, "p_axis": 0, "p_min_angle": -np.pi / 24.0, "p_max_angle": np.pi / 24.0,
     "p_apply_extra_tensors": [True, False, False, False]},
    {"name": "RotationAug", "p_prob": 1.0, "p_axis": 1, "p_min_angle": -np.pi / 24.0, "p_max_angle": np.pi / 24.0,
     "p_apply_extra_tensors": [True, False, False, False]},
    {"name": "LinearAug", "p_prob": 1.0, "p_min_a": 0.75, "p_max_a": 1.25, "p_min_b": 0.0, "p_max_b": 0.0, "p_channel_independent": True,
     "p_apply_extra_tensors": [False, False, False, False]},
    {"name": "NoiseAug", "p_prob": 1.0, "p_stddev": 0.005, "p_clip": 0.02, "p_apply_extra_tensors": [False, False, False, False]},
    {"name": "CropPtsAug", "p_prob": 1.0, "p_max_pts": 120000, "p_crop_ratio": 0.8, "p_apply_extra_tensors": [True, True, True, True]},
    {"name": "CenterAug", "p_axes": [True, True, False], "p_apply_extra_tensors": [False, False, False, False]},
    {"name": "TranslationAug", "p_prob": 1.0, "p_max_aabb_ratio": np.array([0.5, 0.5, 0.0]), "p_apply_extra_tensors": [False, False, False, False]},
]
NUM_TEST_EPOCHS = 30
SCANNET_TEST = [
    {"name": "CenterAug", "p_apply_extra_tensors": [False, False, False, False]},
    {"name": "RotationAug", "p_prob": 1.0, "p_axis": 2, "p_angle_values": [(i / NUM_TEST_EPOCHS) * 2. * np.pi for i in range(NUM_TEST_EPOCHS)],
     "p_apply_extra_tensors": [True, False, False, False]},
]
