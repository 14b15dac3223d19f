"""CPU: the library reads its runtime switches in one place and is built one way (source scan, no library needed).

The six environment switches of the appendix of include/se3conv.h are read by `switches()` (common.h, defined in api.hip),
once per process, and by nothing else; the only macros a build may set are the timeline instrument and the degree of the
GELU polynomials."""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "se3conv3d_amd", "csrc")
SWITCHES = {"SE3_NO_T24", "SE3_NO_PAIR", "SE3_PG_SINGLE", "SE3_TR_MERGE_SORT", "SE3_DX_PATH", "SE3_EDGE_STREAM"}
BUILD_MACROS = {"SE3_TIMELINE", "SE3_GELU_POLY", "SE3_GELU_DPOLY"}
SIGNATURE = "const Switches& switches() {"


def sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert paths, "no sources found: the scan is broken"
    return {os.path.basename(p): open(p).read() for p in paths}


def code_only(text):
    return "\n".join(line.split("//")[0] for line in text.splitlines())


def switches_definition():
    """(file name, start, end) of the body of switches(): from its signature to the brace that closes it."""
    found = [(name, text.index(SIGNATURE)) for name, text in sources().items() if SIGNATURE in code_only(text)]
    assert len(found) == 1, f"switches() must be defined exactly once, found in {[n for n, _ in found]}"
    name, start = found[0]
    text = sources()[name]
    depth, pos = 0, start + len(SIGNATURE) - 1
    while True:
        depth += {"{": 1, "}": -1}.get(text[pos], 0)
        pos += 1
        if depth == 0:
            return name, start, pos


def test_the_environment_is_read_only_inside_switches():
    where, start, end = switches_definition()
    assert where == "api.hip"
    n_inside = 0
    for name, text in sources().items():
        text = code_only(text) if name != where else text
        for m in re.finditer(r"\bgetenv\s*\(", text):
            assert name == where and start <= m.start() < end, f"{name} reads the environment outside switches()"
            n_inside += 1
    assert n_inside == len(SWITCHES)


def test_switches_reads_exactly_the_six_documented_names():
    where, start, end = switches_definition()
    body = sources()[where][start:end]
    names = re.findall(r'getenv\("([A-Z0-9_]+)"\)', body)
    assert sorted(names) == sorted(SWITCHES)
    assert len(re.findall(r"\bgetenv\s*\(", body)) == len(names), "a getenv call that is not a literal name"


def test_no_build_macro_besides_timeline_and_gelu_degree():
    n_tests = 0
    for name, text in sources().items():
        for line in text.splitlines():
            m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b(.*)", line)
            if not m:
                continue
            for macro in re.findall(r"\bSE3_\w+", m.group(2).split("//")[0]):
                n_tests += 1
                assert macro in BUILD_MACROS, f"{name}: `{line.strip()}` makes the build depend on {macro}"
    assert n_tests, "no conditional found: the scan is broken"
