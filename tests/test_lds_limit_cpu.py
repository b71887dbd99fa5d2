"""The (kernel, device) bookkeeping of pn2_allow_lds (csrc/pn2_device_set.h, plain C++) under ThreadSanitizer: an ordinary
child process built from tests/host/lds_limit_main.cpp, which includes the header the library itself is built with."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    for cand in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = cand and shutil.which(cand)
        if path:
            return path
    return None


def test_device_set_under_thread_sanitizer(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++) found")
    exe = str(tmp_path / "lds_limit")
    src = os.path.join(ROOT, "tests", "host", "lds_limit_main.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", src, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "ThreadSanitizer" not in run.stdout, run.stdout
