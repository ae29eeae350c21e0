"""The staging arena's layout (csrc/stage.h) on the CPU: tests/stage_layout_main.cpp, a stand-alone
program over malloc'd arenas of exactly the computed size, built with the host C++ compiler under
AddressSanitizer + UBSan and run as a child process.  Nothing is preloaded and nothing is loaded
into Python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_stage_layout_under_asan_ubsan(tmp_path):
    exe = tmp_path / "stage_layout"
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    os.path.join(HERE, "stage_layout_main.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "stage layout ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-4000:])
