"""Recipe for `oracle/_ref/`: the reference's own native module (`point_cloud_lib_ops`), compiled for the device.

`build_reference()` is called by `build()` after the library build.  Where a checkout of the reference is present (the
directory named by SE3_REFERENCE_DIR, default /root/reference) it copies `point_cloud_lib/custom_ops/` into a temporary
directory outside the repository, lets torch's extension builder translate and compile the copy for gfx950, and keeps two
files: the shared object and `manifest.json` (sha256 of every source file read, torch version, arch, flags).  The
temporary directory, with the source copy, the translated files and the objects, is removed.  Nothing of the reference and
nothing compiled from it is committed: `oracle/_ref/` is ignored by git; it exists so that the GPU tests of
`tests/test_gpu_reference_kernels.py` can hold the library and `oracle/se3conv_oracle.py` to the kernels they restate.

Three adjustments are made to the copy, none of which touches a kernel body or a launch:
  1. the copy's root and its sub-directories go on the include path, so that the translator also rewrites the headers;
  2. `oracle/ref_shims/` goes on the include path: `THC/THCAtomics.cuh`, which one source includes, left torch;
  3. the `static` float `atomicMax` of `utils.cuh`, which nothing calls and which collides with HIP's own overload, is cut
     out of the copy.  It is found by name at build time.

Whether a compiled module and the reference are present decides what happens:

    module   reference   action
    present  absent      keep the module as it is
    absent   absent      print one line and return
    any      present     rebuild if the manifest's hashes, torch version, arch or flags differ; a failed build raises

Product code (`se3conv3d_amd/`, `bench.py`, `smoke()`) never imports this module or `oracle/ref_ops.py`.
"""
import hashlib
import json
import os
import re
import shutil
import tempfile
from typing import Callable, Dict, Optional

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR_ENV = "SE3_REFERENCE_DIR"
REF_DIR_DEFAULT = "/root/reference"
OPS_SUBDIR = os.path.join("point_cloud_lib", "custom_ops")
OUT_DIR = os.path.join(HERE, "_ref")
SHIMS = os.path.join(HERE, "ref_shims")
MODULE = "point_cloud_lib_ops_ref"
ARCH = "gfx950"
MAX_JOBS = 16
CFLAGS = ["-O3"]
HIP_CFLAGS = ["-O3"]
SOURCE_SUFFIXES = (".cu", ".cuh", ".cpp", ".h", ".hpp")
UNUSED_HELPER = ("utils.cuh", "atomicMax")   # (file, function) cut from the copy: see the module docstring
MANIFEST = "manifest.json"


def reference_dir() -> str:
    return os.environ.get(REF_DIR_ENV, REF_DIR_DEFAULT)


def ops_dir(ref_dir: Optional[str] = None) -> str:
    return os.path.join(ref_dir if ref_dir is not None else reference_dir(), OPS_SUBDIR)


def _sha256(path: str) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 20), b""):
            h.update(block)
    return h.hexdigest()


def _tree_files(root: str):
    for base, dirs, files in os.walk(root):
        dirs.sort()
        for name in sorted(files):
            if name.endswith(SOURCE_SUFFIXES):
                full = os.path.join(base, name)
                yield os.path.relpath(full, root).replace(os.sep, "/"), full


def source_hashes(src_dir: str) -> Dict[str, str]:
    """sha256 of every source file the build reads: the reference's sources and headers, and the shim headers."""
    out = {"reference/" + rel: _sha256(full) for rel, full in _tree_files(src_dir)}
    out.update({"ref_shims/" + rel: _sha256(full) for rel, full in _tree_files(SHIMS)})
    return out


def expected_manifest(src_dir: str) -> dict:
    import torch

    return {"module": MODULE, "torch": torch.__version__, "arch": ARCH, "cflags": CFLAGS, "hip_cflags": HIP_CFLAGS,
            "max_jobs": MAX_JOBS, "sources": source_hashes(src_dir)}


def read_manifest(out_dir: str = OUT_DIR) -> Optional[dict]:
    path = os.path.join(out_dir, MANIFEST)
    if not os.path.isfile(path):
        return None
    with open(path) as f:
        return json.load(f)


def module_path(out_dir: str = OUT_DIR) -> Optional[str]:
    man = read_manifest(out_dir)
    name = man.get("file") if man else None
    if name is None and os.path.isdir(out_dir):
        found = sorted(n for n in os.listdir(out_dir) if n.startswith(MODULE) and n.endswith(".so"))
        name = found[0] if found else None
    path = os.path.join(out_dir, name) if name else None
    return path if path and os.path.isfile(path) else None


def up_to_date(src_dir: str, out_dir: str = OUT_DIR) -> bool:
    man = read_manifest(out_dir)
    if man is None or module_path(out_dir) is None:
        return False
    want = expected_manifest(src_dir)
    return all(man.get(k) == v for k, v in want.items())


def cut_function(text: str, name: str) -> str:
    """`text` without the definition of the function `name` (and the comment block right above it): from the start of the
    line that declares it to the brace that closes its body, a trailing semicolon included."""
    m = re.search(r"^[^\n;{}()/*]*\b" + re.escape(name) + r"\s*\(", text, re.M)
    if m is None:
        raise RuntimeError(f"no definition of {name} found")
    open_brace = text.index("{", m.end())
    depth, pos = 0, open_brace
    while True:
        ch = text[pos]
        depth += (ch == "{") - (ch == "}")
        pos += 1
        if depth == 0:
            break
    tail = re.match(r"[ \t]*;?[ \t]*\n?", text[pos:])
    start = m.start()
    doc = re.search(r"/\*(?:(?!\*/).)*\*/\s*\Z", text[:start], re.S)
    if doc is not None:
        start = doc.start()
    return text[:start] + text[pos + tail.end():]


def prepare_copy(src_dir: str, work: str) -> str:
    """Copy the sources and the shim headers into `work` (the translator writes next to what it reads) and cut the unused
    helper out of the copy; returns the copy's root."""
    dst = os.path.join(work, "custom_ops")
    shutil.copytree(src_dir, dst)
    shutil.copytree(SHIMS, os.path.join(work, "ref_shims"))
    for base, _dirs, files in os.walk(work):
        os.chmod(base, 0o755)
        for name in files:
            os.chmod(os.path.join(base, name), 0o644)
    fname, func = UNUSED_HELPER
    path = os.path.join(dst, fname)
    with open(path) as f:
        text = f.read()
    with open(path, "w") as f:
        f.write(cut_function(text, func))
    return dst


def compile_copy(copy_root: str, work: str) -> str:
    """Translate and compile the copy with torch's extension builder; returns the path of the shared object."""
    saved = {k: os.environ.get(k) for k in ("PYTORCH_ROCM_ARCH", "MAX_JOBS")}
    os.environ["PYTORCH_ROCM_ARCH"] = ARCH
    jobs = saved["MAX_JOBS"]
    os.environ["MAX_JOBS"] = str(min(MAX_JOBS, int(jobs)) if jobs and jobs.isdigit() and int(jobs) > 0 else MAX_JOBS)
    try:
        from torch.utils import cpp_extension

        sources = sorted(full for rel, full in _tree_files(copy_root) if rel.endswith((".cu", ".cpp")))
        subdirs = sorted(os.path.join(copy_root, d) for d in os.listdir(copy_root) if os.path.isdir(os.path.join(copy_root, d)))
        build_dir = os.path.join(work, "build")
        os.makedirs(build_dir)
        # `load` is torch's public entry to translate + ninja-build; with is_python_module=False it also maps the fresh
        # library into this process (torch.ops.load_library).  Nothing here calls into it, and the mapping outlives the
        # removal of the temporary directory without harm; the tests load the copy kept under oracle/_ref/ instead.
        cpp_extension.load(name=MODULE, sources=sources, extra_include_paths=[copy_root] + subdirs + [os.path.join(work, "ref_shims")],
                           extra_cflags=CFLAGS, extra_cuda_cflags=HIP_CFLAGS, build_directory=build_dir, verbose=False,
                           is_python_module=False)
        so = os.path.join(build_dir, MODULE + ".so")
        if not os.path.isfile(so):
            raise RuntimeError(f"the extension builder left no {MODULE}.so")
        return so
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def build_reference(ref_dir: Optional[str] = None, out_dir: str = OUT_DIR,
                    compile_step: Callable[[str, str], str] = compile_copy, verbose: bool = True) -> str:
    """See the module docstring.  Returns "absent", "kept", "current" or "built"."""
    say = print if verbose else (lambda *a, **k: None)
    src = ops_dir(ref_dir)
    if not os.path.isdir(src):
        if module_path(out_dir) is not None:
            say(f"reference ops: no reference tree at {src}; keeping {module_path(out_dir)}")
            return "kept"
        say(f"reference ops: no reference tree at {src} and no compiled module; the reference-kernel tests will skip")
        return "absent"
    if up_to_date(src, out_dir):
        say(f"reference ops: {module_path(out_dir)} is up to date")
        return "current"
    manifest = expected_manifest(src)
    work = tempfile.mkdtemp(prefix="se3_ref_ops_")
    try:
        if os.path.commonpath([os.path.realpath(work), os.path.dirname(HERE)]) == os.path.dirname(HERE):
            raise RuntimeError(f"the temporary directory {work} lies inside the repository")
        so = compile_step(prepare_copy(src, work), work)
        if os.path.isdir(out_dir):
            shutil.rmtree(out_dir)
        os.makedirs(out_dir)
        manifest["file"] = MODULE + ".so"
        shutil.copyfile(so, os.path.join(out_dir, manifest["file"]))
        manifest["sha256"] = _sha256(os.path.join(out_dir, manifest["file"]))
        with open(os.path.join(out_dir, MANIFEST), "w") as f:
            json.dump(manifest, f, indent=1, sort_keys=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    say(f"reference ops: built {os.path.join(out_dir, manifest['file'])}")
    return "built"


if __name__ == "__main__":
    build_reference()
