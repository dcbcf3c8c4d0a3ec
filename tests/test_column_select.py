"""csrc/column_select.hpp's walk on the host: tests/column_select_check.cpp is compiled as plain C++17 (no HIP) and run on the CPU.

The program holds segment_sum and walk_to_digit, for 16- and 64-column tiles, to a brute-force prefix sum over a column's 256
counters: every rank of a histogram with all keys in digit 0, with all in digit 255, with one key per digit and with empty
segments before and behind the keys, the last key of each (the walk's fall-through is for ranks beyond the keys alone), and random
histograms of up to 65,535 keys read through a plain accessor and through either half of a packed word.  The rank left inside the
digit lies in 0 .. run - 1 throughout.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'attacking_federate_learning_amd', 'csrc')


def test_the_walk_to_a_ranks_digit_on_the_host(tmp_path):
    compiler = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if compiler is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'column_select_check')
    build = subprocess.run([compiler, '-std=c++17', '-O1', '-Wall', '-Wno-unknown-pragmas', '-I', CSRC,
                            os.path.join(HERE, 'column_select_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith('column_select ok'), run.stdout
