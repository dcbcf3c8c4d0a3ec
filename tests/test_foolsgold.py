"""FoolsGold without a GPU: the numpy restatement of include/byzagg.h's rule (tests/foolsgold_rule.py; tests/test_gpu_foolsgold.py
holds the device to it) against a literal transcription of the authors' loop, on the planted sybils and on the graded Grams, its
edge cases by rule number, csrc/foolsgold_rule.hpp on the host (tests/foolsgold_rule_check.cpp, built with the host sanitizers),
and the surface: header, ctypes table, build list, Python layers, documents."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.foolsgold_rule import (PLANTED_HONEST, authors_foolsgold, graded_gram, gram64, history_chain, planted_rounds,
                                  restated_foolsgold_weights, with_edge_cases, write_rule_cases)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, 'attacking_federate_learning_amd', 'csrc')
NEW_SYMBOLS = ('byz_rows_add_dev', 'byz_foolsgold_weights_dev', 'byz_foolsgold_trace_dev', 'byz_foolsgold_dev', 'byz_foolsgold_info',
               'byz_foolsgold_host')
GRADED = [(64, 8), (257, 8), (1000, 10)]


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- the restatement against the authors' loop, and what it decides ---------------------------------------------------------------
@pytest.mark.parametrize('seed', range(6))
def test_planted_sybils_get_exactly_zero_and_the_restatement_is_the_authors_loop(seed):
    for history in history_chain(planted_rounds(seed)):
        c = gram64(history)
        got = restated_foolsgold_weights(c)
        assert np.array_equal(bits64(got['weights']), bits64(authors_foolsgold(c)))          # 0 difference
        assert (got['weights'][PLANTED_HONEST:] == 0.0).all() and (got['weights'][:PLANTED_HONEST] == 1.0).all()
        assert got['usable_rows'] == c.shape[0] and not got['degenerate'] and got['divisor'] == float(c.shape[0])


@pytest.mark.parametrize('n,d', GRADED)
@pytest.mark.parametrize('seed', range(5))
def test_graded_weights_exercise_the_logit(n, d, seed):
    c = graded_gram(n, d, seed)
    got = restated_foolsgold_weights(c)
    l = got['weights']
    inside, at0, at1 = ((l > 0.0) & (l < 1.0)).mean(), (l == 0.0).mean(), (l == 1.0).mean()
    print('graded %d x %d seed %d: %.1f %% inside, %.1f %% at 0, %.1f %% at 1' % (n, d, seed, 100 * inside, 100 * at0, 100 * at1))
    assert inside >= 0.20 and at0 >= 0.05 and at1 >= 0.05
    assert (got['at_zero'], got['at_one']) == (int((l == 0).sum()), int((l == 1).sum()))
    if n <= 257:
        assert np.array_equal(bits64(l), bits64(authors_foolsgold(c)))


# ---- edge cases by rule number ---------------------------------------------------------------------------------------------------
def test_one_row_and_two_rows():
    one = restated_foolsgold_weights(np.array([[4.0]]))
    assert one['weights'].tolist() == [1.0] and one['divisor'] == 1.0 and not one['degenerate']          # (7): fewer than 2
    assert restated_foolsgold_weights(np.array([[np.nan]]))['weights'].tolist() == [0.0]
    two = restated_foolsgold_weights(np.array([[1.0, 0.0], [0.0, 4.0]]))                                   # orthogonal: both 1
    assert two['weights'].tolist() == [1.0, 1.0] and two['rescaled'].tolist() == [0.99, 0.99]
    twins = restated_foolsgold_weights(np.array([[1.0, 2.0], [2.0, 4.0]]))                                 # cs = 1: everybody's twin
    assert twins['degenerate'] and twins['weights'].tolist() == [0.0, 0.0] and twins['top'] == 0.0
    assert np.isnan(authors_foolsgold(np.array([[1.0, 2.0], [2.0, 4.0]]))).all()                           # (the authors': NaN)
    lone = restated_foolsgold_weights(np.array([[1.0, 2.0], [2.0, -4.0]]))                                 # one usable of two
    assert lone['weights'].tolist() == [1.0, 0.0] and lone['usable_rows'] == 1 and lone['divisor'] == 1.0


def test_all_rows_identical_give_zeros_not_nan():
    x = np.tile(np.random.default_rng(0).normal(size=8).astype(np.float32), (9, 1))
    got = restated_foolsgold_weights(gram64(x), normalise='sum')
    assert got['degenerate'] and not got['weights'].any() and got['divisor'] == 0.0 and got['at_zero'] == 9


@pytest.mark.parametrize('n,d', [(65, 8), (1025, 12)])
def test_the_planted_edge_cases(n, d):
    plain = graded_gram(n, d, 0)
    c = with_edge_cases(plain)
    got = restated_foolsgold_weights(c)
    assert not got['usable'][[1, 4, n - 1]].any() and got['usable'].sum() == n - 3                        # (1)
    assert got['weights'][[1, 4, n - 1]].tolist() == [0.0] * 3 and got['rescaled'][[1, 4, n - 1]].tolist() == [0.0] * 3
    assert got['usable'][6] and got['maxcs'][6] == 0.0 and got['alpha'][6] == 0.0 and got['weights'][6] == 1.0      # (2): v = 1 = top
    assert np.isfinite(got['maxcs'][[2, 9]]).all() and np.isfinite(got['weights']).all()                 # (3): a NaN cosine is 0
    assert np.isfinite(got['alpha'][[3, 11]]).all()                                                      # (5): -inf * 0 never enters
    # nobody sees an excluded row: deleting the excluded rows and columns changes no other row's numbers
    keep = np.flatnonzero(got['usable'])
    small = restated_foolsgold_weights(c[np.ix_(keep, keep)])
    for key in ('maxcs', 'alpha', 'rescaled', 'weights'):
        assert np.array_equal(bits64(small[key]), bits64(got[key][keep])), key
    assert small['divisor'] == got['divisor'] == float(n - 3)


def test_an_infinite_entry_costs_both_rows_their_weight():
    c = graded_gram(64, 8, 1)
    c[5, 7] = c[7, 5] = np.inf
    got = restated_foolsgold_weights(c)
    assert got['maxcs'][5] == np.inf and got['alpha'][5] == np.inf and got['weights'][[5, 7]].tolist() == [0.0, 0.0]
    assert np.isfinite(got['weights']).all()


def test_both_divisors_and_a_kappa_that_is_not_one():
    c = graded_gram(257, 8, 2)
    count, total = restated_foolsgold_weights(c), restated_foolsgold_weights(c, normalise='sum')
    assert np.array_equal(bits64(count['weights']), bits64(total['weights']))
    assert count['divisor'] == 257.0 and abs(total['divisor'] - count['weights'].sum()) <= 257 * 2.0 ** -53 * total['divisor']
    two = restated_foolsgold_weights(c, kappa=2.0)
    assert np.array_equal(bits64(two['rescaled']), bits64(count['rescaled']))                    # kappa enters at the logit only
    inside = (two['weights'] > 0) & (two['weights'] < 1)
    assert inside.sum() >= 20 and np.array_equal(bits64(two['weights']), bits64(authors_foolsgold(c, kappa=2.0)))
    raised = (count['weights'] > 0) & (count['weights'] < 0.5)
    assert raised.any() and (two['weights'][raised] == 2.0 * count['weights'][raised]).all()


# ---- the rule's header on the host -------------------------------------------------------------------------------------------------
def test_the_rule_header_on_the_host_under_the_sanitizers(tmp_path):
    compiler = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if compiler is None:
        pytest.skip('no host C++ compiler')
    cases = [(graded_gram(64, 8, 0), 1.0, 'count'), (graded_gram(257, 8, 1), 2.0, 'sum'), (with_edge_cases(graded_gram(65, 8, 0)), 1.0, 'sum'),
             (gram64(history_chain(planted_rounds(0))[-1]), 1.0, 'count'), (np.array([[1.0, 2.0], [2.0, 4.0]]), 1.0, 'count'),
             (np.array([[3.0]]), 1.0, 'sum'), (np.array([[1.0, 2.0], [2.0, -4.0]]), 1.0, 'sum')]
    c = graded_gram(64, 8, 1)
    c[5, 7] = c[7, 5] = np.inf
    cases.append((c, 1.0, 'count'))
    path = str(tmp_path / 'cases.txt')
    write_rule_cases(path, cases)
    exe = str(tmp_path / 'foolsgold_rule_check')
    base = [compiler, '-std=c++17', '-O1', '-g', '-Wall', '-Wno-unknown-pragmas', '-ffp-contract=off', '-I', CSRC,
            os.path.join(HERE, 'foolsgold_rule_check.cpp'), '-o', exe]
    build = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], capture_output=True, text=True)
    if build.returncode != 0 and 'sanitize' in build.stderr + build.stdout:
        build = subprocess.run(base, capture_output=True, text=True)           # (a compiler without the sanitizer runtimes)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe, path], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith('foolsgold_rule ok: %d cases' % len(cases)), run.stdout


# ---- the surface -------------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_table():
    header = open(os.path.join(ROOT, 'include', 'byzagg.h')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint %s\(' % name, header), name
    assert re.search(r'typedef struct byz_foolsgold_params \{\s*double kappa;[^}]*int64_t normalise;', header)
    for phrase in ('Usable rows', 'Pardoning', 'p_ij = (m_i < m_j) ? (cs_ij * m_i) / m_j : cs_ij', 'w_i == 1: w_i = 0.99',
                   'kappa * (log(w_i / (1 - w_i))', 'T == 0 gives the zero vector'):
        assert phrase in header, phrase
    from attacking_federate_learning_amd import _native
    for name in NEW_SYMBOLS:
        assert name in _native.EXPORTED_SYMBOLS, name
    i64, vp, f64 = ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    P = ctypes.POINTER
    params = P(_native.FoolsgoldParams)
    assert _native._PROTOTYPES['byz_rows_add_dev'] == [vp, vp, i64, vp, i64, i64, i64, i64, vp]
    assert _native._PROTOTYPES['byz_foolsgold_weights_dev'] == [vp, vp, i64, params, vp, vp, vp, vp]
    assert _native._PROTOTYPES['byz_foolsgold_dev'] == [vp, vp, i64, i64, i64, vp, i64, i64, i64, params, vp, vp, vp, vp]
    assert _native._PROTOTYPES['byz_foolsgold_info'] == [vp, P(i64), P(f64)]
    assert _native._PROTOTYPES['byz_foolsgold_host'] == [vp, vp, i64, i64, vp, i64, i64, params, vp, vp, vp]
    assert ctypes.sizeof(_native.FoolsgoldParams) == 16 and _native.FoolsgoldParams.normalise.offset == 8


def test_the_source_is_on_the_build_list():
    from attacking_federate_learning_amd import build_native
    assert 'foolsgold.hip' in build_native.SOURCES
    assert '-ffp-contract=off' in build_native.EXTRA_FLAGS['foolsgold.hip']
    text = open(os.path.join(CSRC, 'foolsgold.hip')).read()
    for kernel in ('rows_add_kernel', 'foolsgold_rowmax_kernel', 'foolsgold_pardon_kernel', 'foolsgold_weights_kernel'):
        assert kernel in text, kernel
    assert '#include "foolsgold_rule.hpp"' in text and 'atomicAdd' not in text and '__shared__ WeightsLds' in text


def test_the_report_joins_the_typed_block():
    text = open(os.path.join(CSRC, 'device_scalars.hpp')).read()
    assert re.search(r'struct FoolsgoldReport \{', text) and re.search(r'FoolsgoldReport foolsgold;', text)
    assert 'sizeof(FoolsgoldReport)' in text and 'BYZ_AT(foolsgold.top)' in text and 'BYZ_AT(foolsgold.divisor)' in text
    assert re.search(r'kReportFoolsgold\b', text)


def test_python_surface():
    from attacking_federate_learning_amd import defences
    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.server import DeviceServer
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    assert str(inspect.signature(defences.foolsgold)) == (
        "(users_grads, users_count, corrupted_count, history=None, columns=None, kappa=1.0, normalise='count', gram=None, "
        "return_info=False)")
    assert list(defences.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']
    assert defences.foolsgold not in defences.defend.values()
    doc = ' '.join(defences.foolsgold.__doc__.split())
    assert 'ONE attacker is invisible' in doc and 'IID' in doc and 'no answer to the drift attack' in doc and 'not used' in doc
    assert str(inspect.signature(Engine.foolsgold_weights)) == '(self, gram, kappa=1.0, on_device=False, like=None)'
    assert str(inspect.signature(Engine.foolsgold)) == (
        "(self, g, users_count=None, corrupted_count=None, history=None, columns=None, kappa=1.0, normalise='count', gram=None, "
        "return_info=False)")
    assert str(inspect.signature(Engine.foolsgold_info)) == '(self)' and callable(Engine.rows_add)
    assert str(inspect.signature(defences.FoolsGoldHistory.__init__)) == '(self, n, width)'
    for name in ('reset', 'numpy'):
        assert callable(getattr(defences.FoolsGoldHistory, name))
    assert str(inspect.signature(DeviceServer.defend_foolsgold)) == "(self, columns=None, kappa=1.0, normalise='count', history=True)"
    assert callable(ShardedAggregator.foolsgold) and callable(HipKernels.foolsgold_weights)
    # the rule of a pre-aggregation: called as then(matrix, users_count, corrupted_count), every other parameter defaulted
    parameters = list(inspect.signature(defences.foolsgold).parameters.values())
    assert [p.name for p in parameters[:3]] == ['users_grads', 'users_count', 'corrupted_count']
    assert all(p.default is not inspect.Parameter.empty for p in parameters[3:])


def test_the_refusals_that_need_no_gpu():
    from attacking_federate_learning_amd.engine import Engine
    p = Engine._foolsgold_params(1)
    assert (p.kappa, p.normalise) == (1.0, 0) and Engine._foolsgold_params(1 << 20, 2.5, 'sum').normalise == 1
    for n, kappa, normalise in ((0, 1.0, 'count'), (5, 0.0, 'count'), (5, -1.0, 'count'), (5, np.nan, 'count'), (5, np.inf, 'sum'),
                                (5, 1.0, 'mean')):
        with pytest.raises(ValueError):
            Engine._foolsgold_params(n, kappa, normalise)
    with pytest.raises(NotImplementedError):
        Engine._foolsgold_params((1 << 20) + 1)
    assert Engine._foolsgold_window(10, None) == (0, 10) and Engine._foolsgold_window(10, (3, 7)) == (3, 4)
    assert Engine._foolsgold_window(10, slice(2, None)) == (2, 8)
    for columns in ((-1, 4), (4, 4), (5, 3), (0, 11), slice(0, 8, 2)):
        with pytest.raises(ValueError):
            Engine._foolsgold_window(10, columns)


def test_the_dropin_shim_is_unchanged():
    import importlib.util
    path = os.path.join(ROOT, 'attacking_federate_learning_amd', 'dropin', 'defences.py')
    spec = importlib.util.spec_from_file_location('shim_defences_foolsgold', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert list(mod.defend) == ['Krum', 'TrimmedMean', 'NoDefense', 'Bulyan']


def test_the_documents_name_the_new_entry_points():
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert name in integration, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '3.4v' in design and 'byz_foolsgold_weights_dev' in design and 'feature-importance' in design
    assert 'artial participation' in design
    papers = open(os.path.join(ROOT, 'PAPERS.md')).read()
    assert 'FoolsGold' in papers and '1808.04866' in papers
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'defences.foolsgold' in readme and 'foolsgold.hip' in readme
    assert 'foolsgold_timing.md' in open(os.path.join(ROOT, 'profiles', 'INDEX.md')).read()
