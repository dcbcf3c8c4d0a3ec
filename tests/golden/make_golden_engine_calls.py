#!/usr/bin/env python3
"""The fixture of tests/test_gpu_engine_operands.py: what the engine of a given commit asks of the library, per form of the
operands.

    python tests/golden/make_golden_engine_calls.py --commit <hash>   # MI355X, on the commit whose engine is the reference

Per case and form of the test: the exception's type where the form is refused, else the ordered compute calls with their
integer and float arguments (equal lists stored once), the number of synchronising calls, and on the torch path the
ordered names of ALL library calls.  `parent_lacks_sync` lists the forms in which that
commit frees an uploaded temporary with no synchronising call behind the last kernel that read it (the test's lifetime
rule).  Nothing but the recorded calls is stored: the inputs are the test's own.  The kinds and bits the test asserts are
checked here too and printed, so that a wrong table shows at minting time; they do not enter the file.
"""
import argparse
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import test_gpu_engine_operands as t  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='the commit the engine in use is from')
    ap.add_argument('--out', default=t.GOLDEN)
    args = ap.parse_args()
    from attacking_federate_learning_amd.engine import get_engine
    eng = get_engine()
    out = {'commit': args.commit, 'forms': {}, 'parent_lacks_sync': []}
    doubts = 0
    for case in sorted(t.CASES):
        reference = None
        for m, a in t.forms_of(case):
            key = t.form_key(case, m, a)
            got = t.run_form(eng, case, m, a)
            if 'raises' in got:
                out['forms'][key] = {'raises': got['raises']}
                if t.compute_calls(got['log']):
                    doubts += 1
                    print('!! %s raised %s after %r' % (key, got['raises'], t.names_of(got['log'])), flush=True)
                continue
            out['forms'][key] = {'compute': t.jsonable(t.compute_calls(got['log'])), 'names': t.names_of(got['log'])}
            if got['violations']:
                out['parent_lacks_sync'].append(key)
            want_kinds = t.jsonable(t.CASES[case][4](m, a))
            if t.jsonable(got['kinds']) != want_kinds:
                doubts += 1
                print('!! %s kinds %r, the table says %r' % (key, got['kinds'], want_kinds), flush=True)
            if reference is None:
                reference = got['values']
            elif got['values'] != reference:
                doubts += 1
                print('!! %s differs from the first form as bits' % key, flush=True)
        print(case, {k.split('/', 1)[1]: v.get('raises', len(v.get('names', ()))) for k, v in out['forms'].items()
                     if k.startswith(case + '/')}, flush=True)
    print('parent lacks the sync:', out['parent_lacks_sync'])
    print('doubts:', doubts)
    t.write_golden(args.out, out['commit'], out['forms'], out['parent_lacks_sync'])
    print('wrote', args.out)


if __name__ == '__main__':
    main()
