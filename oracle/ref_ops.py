"""Loader of the reference's own native module, as `oracle/build_ref.py` compiled it into `oracle/_ref/`.

TEST INFRASTRUCTURE ONLY: nothing under `se3conv3d_amd/`, `bench.py` or `smoke()` imports this file.

`load()` returns the module (`ball_query`, `compute_keys`, `feat_basis_proj`, `feat_basis_proj_grad`, `knn_query`), or
`None` when `oracle/_ref/` holds no manifest -- a checkout that was built without the reference.  With a manifest every
failure raises: a missing or unloadable shared object, another torch than the one it was built against, a missing op.  A
quiet `None` there would turn every test that holds the library to the reference's kernels into a skip.
"""
import importlib.util
import json
import os
from typing import Optional

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "_ref")
MANIFEST = "manifest.json"
OPS = ("ball_query", "compute_keys", "feat_basis_proj", "feat_basis_proj_grad", "knn_query")

_loaded = {}


class ReferenceOpsError(RuntimeError):
    """`oracle/_ref/` holds a manifest, and the module it describes cannot be used."""


def load(out_dir: Optional[str] = None):
    out_dir = OUT_DIR if out_dir is None else out_dir
    path = os.path.join(out_dir, MANIFEST)
    if not os.path.isfile(path):
        return None
    import torch  # before the module: it links against torch's libraries

    with open(path) as f:
        manifest = json.load(f)
    if manifest.get("torch") != torch.__version__:
        raise ReferenceOpsError(f"{path}: built against torch {manifest.get('torch')}, this is torch {torch.__version__}; "
                                "run build() where the reference is present")
    so = os.path.join(out_dir, str(manifest.get("file")))
    if so in _loaded:
        return _loaded[so]
    if not os.path.isfile(so):
        raise ReferenceOpsError(f"{path} names {manifest.get('file')}, which is not there")
    try:
        spec = importlib.util.spec_from_file_location(manifest["module"], so)
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
    except Exception as exc:  # ImportError, OSError, KeyError: all mean the same here
        raise ReferenceOpsError(f"{so} does not load: {exc}") from exc
    missing = [name for name in OPS if not hasattr(module, name)]
    if missing:
        raise ReferenceOpsError(f"{so} lacks {missing}")
    _loaded[so] = module
    return module
