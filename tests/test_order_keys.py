"""csrc/order_keys.hpp on the host: tests/order_keys_check.cpp is compiled as plain C++17 (no HIP) and run on the CPU.

The program walks every float whose low 16 bits are 0x0000, 0x0001 or 0xffff and checks the round trip of the plain map, its
order (-0.0 strictly below +0.0), the total map (every NaN to all ones behind +inf, the zeros on one key, the plain map
elsewhere) for float and double, both finiteness tests against isfinite, and the visit order with its inverse up to 2^20.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'attacking_federate_learning_amd', 'csrc')


def test_order_keys_on_the_host(tmp_path):
    compiler = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if compiler is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'order_keys_check')
    build = subprocess.run([compiler, '-std=c++17', '-O1', '-Wall', '-I', CSRC,
                            os.path.join(HERE, 'order_keys_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith('order_keys ok'), run.stdout
