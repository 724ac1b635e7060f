"""The host side's two shared headers without a device: maua_amd/csrc/dtype.h (bytes per element of a maua_dtype, the dispatcher over a
compile-time list of element types) and scratch.h (the one carver of 256-byte aligned workspaces), compiled alone with the host compiler
(tests/dtype_scratch_main.cpp), and the sizes the exported maua_*_workspace functions report - callers size buffers with them, so each
is pinned to the value the hand-written layouts gave before the carver replaced them."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "maua_amd" / "csrc"


def test_headers_stand_alone_with_the_host_compiler(tmp_path):
    exe = tmp_path / "dtype_scratch"
    cxx = shutil.which("g++") or shutil.which("c++") or "/opt/rocm/lib/llvm/bin/clang++"   # (the last: the host compiler hipcc drives)
    cmd = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", f"-I{CSRC}", str(ROOT / "tests" / "dtype_scratch_main.cpp"),
           "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stderr


def test_headers_include_no_hip_header():
    for name in ("dtype.h", "scratch.h"):
        includes = [line.split()[1] for line in (CSRC / name).read_text().splitlines() if line.startswith("#include")]
        assert includes and all("hip/" not in i and i != '"common.h"' for i in includes), (name, includes)


# recorded from the library as it was before the carver (hand-written layouts): one case with a dimension of 1, one that is no multiple
# of 64, one large, one a multiple of 64
WORKSPACES = {
    "maua_correlation_workspace": {(1, 1, 1): 1536, (100, 7, 3): 4608, (1000, 64, 64): 281344, (333, 12, 1): 9216},
    "maua_metrics_moments_workspace": {(1, 1): 0, (100, 37): 29696, (5000, 2048): 81920000, (64, 64): 32768},
    "maua_sqrtm_workspace": {(1,): 2816, (37,): 67328, (64,): 197888, (2048,): 201327872},
    "maua_frechet_workspace": {(1, 1, 1): 0, (100, 90, 37): 142336, (5000, 4000, 2048): 417498624, (64, 64, 64): 363008},
    "maua_kernel_distance_workspace": {(1, 1): 0, (100, 37): 59648, (1000, 2048): 32772096, (64, 64): 65792},
    "maua_prdc_workspace": {(1, 1, 1): 2048, (100, 90, 37): 86016, (5000, 4000, 2048): 156308736, (64, 1, 64): 43264},
}


@pytest.mark.parametrize("name", sorted(WORKSPACES))
def test_exported_workspace_sizes_are_pinned(name):
    from maua_amd import _lib as L
    from maua_amd.build import build
    build()
    fn = getattr(L.lib(), name)
    for args, want in WORKSPACES[name].items():
        assert fn(*args) == want, (name, args)
        assert want % 256 == 0


def test_every_exported_workspace_function_is_pinned():
    from maua_amd import _lib as L
    assert {s for s in L.declared_symbols() if s.endswith("_workspace")} == set(WORKSPACES)
