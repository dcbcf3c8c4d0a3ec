"""csrc/owner_loop.hpp on the host: tests/owner_loop_check.cpp is compiled as plain C++17 (no HIP) and run on the CPU.

The program holds the ownership (row_of, owner_thread, slot_of over every row below the ceiling), FABA's removal key (its order
against the rule's own comparison over every pair of 1,000-odd (bad, s, row) samples, its unpacking, no key {0, 0}) and the fp64
total map against the sign flip faba.hip used to carry.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'attacking_federate_learning_amd', 'csrc')


def test_ownership_and_the_removal_key_on_the_host(tmp_path):
    compiler = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if compiler is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'owner_loop_check')
    build = subprocess.run([compiler, '-std=c++17', '-O1', '-Wall', '-Wno-unknown-pragmas', '-I', CSRC,
                            os.path.join(HERE, 'owner_loop_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith('owner_loop ok'), run.stdout
