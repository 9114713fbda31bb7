"""Host, no GPU: the compaction table of the member-removal path (csrc/removal_table.hpp, used by Fast<>::task_update) against plain
"erase the listed elements in order", for all 57 cases of (n, drop).  The checks are in tests/removal_table_host.cpp, a stand-alone
program; this file builds it with the host compiler -- with AddressSanitizer and UBSan when the compiler can link them -- and runs it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "removal_table_host.cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.fail("no host C++ compiler")
    exe = tmp_path_factory.mktemp("removal_table") / "removal_table_host"
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", SRC, "-o", str(exe)]
    out = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
    sanitized = out.returncode == 0
    if not sanitized:                                   # a compiler without the sanitizer runtimes: the plain program checks the same
        out = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return str(exe), sanitized


def test_all_57_cases(program):
    exe, sanitized = program
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print("sanitized:", sanitized, out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "57 cases x 2 strides ok" in out.stdout
