"""csrc/carve.hpp on the host: tests/carve_check.cpp is compiled as plain C++17 (no HIP) and run on the CPU.

The program lays out mixed float / double / int32 / int64 arrays of 1, 3, 1025 and 0 elements in every order of the types into a
malloc-backed buffer and checks the first array at the base, 16-byte alignment, no overlap (by address and by writing every
element), total(), that a second commit into a large enough buffer allocates nothing, and that a negative count, an overflowing
byte size and one array more than the table holds are refused before the buffer is touched.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'attacking_federate_learning_amd', 'csrc')


def test_carve_on_the_host(tmp_path):
    compiler = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if compiler is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'carve_check')
    build = subprocess.run([compiler, '-std=c++17', '-O1', '-Wall', '-I', CSRC,
                            os.path.join(HERE, 'carve_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith('carve ok'), run.stdout
