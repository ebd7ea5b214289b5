"""CPU: every source of the library names what it uses.  The product is one translation unit (sdf_unity.hip), but each
.hip under sedef_amd/csrc must also pass the compiler's syntax check as a translation unit of its own, so that a helper's
users can be read off the includes and not off the order of the unity file."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "sedef_amd", "csrc")


def _sources():
    return sorted(f for f in os.listdir(SRC) if f.endswith(".hip") and f != "sdf_unity.hip")


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"  # (as sedef_amd.build.build_library finds it)
    return hipcc if os.path.exists(hipcc) else None


def test_every_source_is_a_translation_unit_of_its_own():
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")

    def check(f):
        p = subprocess.run([hipcc, "-std=c++17", "-O3", "--offload-arch=gfx950", "-fsyntax-only", f], cwd=SRC,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        return f, p.returncode, p.stdout

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        results = list(pool.map(check, _sources()))
    failed = {f: out[-2000:] for f, rc, out in results if rc != 0}
    assert not failed, "\n".join("%s:\n%s" % kv for kv in failed.items())


def test_unity_file_includes_every_source_once():
    text = open(os.path.join(SRC, "sdf_unity.hip")).read()
    included = re.findall(r'^#include "([^"]+\.hip)"', text, flags=re.M)
    assert sorted(included) == _sources()
    assert len(included) == len(set(included))


def test_no_source_includes_another_source():
    """(what a file shares is in a header: a .hip that pulled in another .hip would pass the check above by compiling
    its neighbour again)"""
    for f in _sources():
        text = open(os.path.join(SRC, f)).read()
        assert not re.findall(r'^#include "[^"]+\.hip"', text, flags=re.M), f
