"""Every header of csrc/ compiles on its own: `hipcc -fsyntax-only -x hip` over the one file, with the language and
warning flags of gvamd/build.py.  A header that leans on what its includer happened to include before it fails here, so
this is the check behind the rule of the launcher headers (gv_launch_frame / _pose / _planner / _match.hpp): a kernel
file includes its family's header and each header includes what it uses.  No GPU; skipped where hipcc is absent."""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grid-vision_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "grid-vision_amd"))
from gvamd import build as gvbuild  # noqa: E402

HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".hpp"))


def _have_hipcc() -> bool:
    return any(c and os.path.exists(c) for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")))


pytestmark = pytest.mark.skipif(not _have_hipcc(), reason="hipcc not installed")


def _syntax_only(header: str):
    # build.FLAGS without what only code generation reads (-O3, -fPIC); both passes, host and gfx950
    flags = [f for f in gvbuild.FLAGS if f not in ("-O3", "-fPIC")]
    r = subprocess.run([gvbuild.hipcc(), *flags, "-Wno-pragma-once-outside-header", "-fsyntax-only", "-x", "hip",
                        os.path.join(CSRC, header)], cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return r.returncode, r.stdout


@pytest.fixture(scope="module")
def compiled():
    """{header: (exit status, compiler output)}, all headers at once in one pool"""
    with ThreadPoolExecutor(max_workers=min(8, len(HEADERS))) as ex:
        return dict(zip(HEADERS, ex.map(_syntax_only, HEADERS)))


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(compiled, header):
    status, out = compiled[header]
    assert status == 0, out


def test_no_umbrella_header_and_every_hip_is_built():
    """gv_kernels.hpp / gv_kernels.hip are gone for good, and the build takes the directory's listing: a .hip dropped
    into csrc/ is a translation unit, none is skipped"""
    assert not os.path.exists(os.path.join(CSRC, "gv_kernels.hpp")) and not os.path.exists(os.path.join(CSRC, "gv_kernels.hip"))
    assert gvbuild.SOURCES == sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
