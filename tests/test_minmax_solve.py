"""csrc/minmax_solve.hpp on the host: tests/minmax_solve_check.cpp is compiled as plain C++17 (no HIP) and run on the CPU, under
AddressSanitizer and UndefinedBehaviorSanitizer when the compiler links them.

The program compares the closed-form roots of the Min-Max / Min-Sum attacks with long double on a grid: b of both signs up to
1e8 times sqrt(c q), q = 0, a denormal c, the row form with and without slack and the sum form over 2 to 4000 rows.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'attacking_federate_learning_amd', 'csrc')


def test_the_roots_on_the_host(tmp_path):
    compiler = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if compiler is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'minmax_solve_check')
    base = [compiler, '-std=c++17', '-O1', '-Wall', '-Wno-unknown-pragmas', '-ffp-contract=off', '-I', CSRC,
            os.path.join(HERE, 'minmax_solve_check.cpp'), '-o', exe]
    build = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], capture_output=True, text=True)
    if build.returncode != 0:          # a compiler without the sanitizers' runtimes: the same program without them
        build = subprocess.run(base, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith('minmax_solve ok'), run.stdout
