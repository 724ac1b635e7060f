"""The host side's one owner of device memory without a device: maua_amd/csrc/devbuf.h (DevBuf and the carved-set helper) compiled alone
with the host compiler against the HIP host API header only, linked to no HIP runtime - tests/devbuf_main.cpp defines the four runtime
functions it calls over malloc - and run under the address and undefined-behaviour sanitizers: live blocks after every alloc / reserve /
move / free, the empty state after a failed allocation, the placement of a carved set, and the refusal of an overflowing layout."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "maua_amd" / "csrc"
ROCM_INCLUDE = "/opt/rocm/include"


def test_devbuf_stands_alone_under_the_sanitizers(tmp_path):
    exe = tmp_path / "devbuf"
    cxx = shutil.which("g++") or shutil.which("c++") or "/opt/rocm/lib/llvm/bin/clang++"
    cmd = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM_INCLUDE}", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", f"-I{ROOT / 'include'}", f"-I{CSRC}", str(ROOT / "tests" / "devbuf_main.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stderr


def test_devbuf_includes_the_host_api_and_the_carver_only():
    includes = [line.split()[1] for line in (CSRC / "devbuf.h").read_text().splitlines() if line.startswith("#include")]
    assert includes == ["<hip/hip_runtime_api.h>", '"scratch.h"'], includes
