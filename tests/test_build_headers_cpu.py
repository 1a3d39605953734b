"""CPU: every header a HIP source under gennbv_amd/csrc/ includes is a build dependency (csrc/build.py HEADERS), so an
edit to a header alone rebuilds the library instead of reusing a stale shared object."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gennbv_amd", "csrc")


def quoted_includes():
    out = set()
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".hip", ".h", ".cpp")):
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(CSRC, fn)).read(), flags=re.M):
                out.add(os.path.normpath(os.path.join(CSRC, inc)))
    return out


def test_every_quoted_include_is_a_build_dependency():
    from gennbv_amd.csrc import build
    listed = {os.path.normpath(os.path.join(build.HERE, h)) for h in build.HEADERS}
    incs = quoted_includes()
    assert incs, "no quoted includes found"
    missing = sorted(os.path.relpath(p, ROOT) for p in incs - listed)
    assert not missing, f"included but not in csrc/build.py HEADERS: {missing}"


def test_every_hip_source_is_compiled():
    from gennbv_amd.csrc import build
    hip = sorted(fn for fn in os.listdir(CSRC) if fn.endswith(".hip"))
    assert sorted(build.SOURCES) == hip
