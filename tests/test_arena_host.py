"""The FlashSR scratch arena (csrc/egr_arena.h) on the host: no device, no library.  tools/arena_host_check.cpp drives seeded random
get / put sequences through the arena over a slab source that deals in address ranges and checks every step against a model."""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_arena_against_its_model_under_host_sanitizers(tmp_path):
    """Compiled by a host compiler with -fsanitize=address,undefined and run as a plain program (the pattern of
    tests/test_wpe_host.py::test_kernel_index_code_under_host_sanitizers)."""
    rocm_clang = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm" / "bin" / "clang++"    # the build needs ROCm, so this one exists
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or (str(rocm_clang) if rocm_clang.exists() else None)
    assert cxx is not None, "no host C++ compiler, not even ROCm's clang++: the arena check cannot run"
    exe = tmp_path / "arena_host_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        str(ROOT / "tools" / "arena_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "all sequences and refusal cases pass" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
