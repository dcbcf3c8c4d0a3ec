"""Every byz_*_info report after every OTHER defence has run: the reports share one device block (csrc/device_scalars.hpp),
and a call may rewrite only the reports DESIGN.md 3.4 lists for it ("public call -> reports it writes").

12 rows x 96 columns, the first 3 rows one attack vector: the smallest shape at which every call below accepts its arguments
and the clusterings have something to split.  The parameters make as many reports non-zero as the data allows.  What stays
all-zero, and so cannot show an overwrite: nnm_info (no row is at a non-finite distance, so no list is short), and the
excluded / broken / inactive / norm_failed counts inside the other reports (every value is finite)."""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, ATTACKERS = 12, 96, 3

READERS = ('geometric_median_info', 'dnc_info', 'centered_clip_info', 'fltrust_info', 'nnm_info', 'robust_lr_info',
           'signguard_info', 'topk_info', 'weak_dp_info', 'flame_info', 'linkage_info', 'clipped_clustering_info',
           'multi_metrics_info', 'fang_krum_info')
# the info calls that refuse before a first call of their defence; the others report the zeroed block
REFUSING = ('flame_info', 'linkage_info', 'clipped_clustering_info', 'multi_metrics_info', 'fang_krum_info')


def bits(v):
    """A report as a hashable value, every double by its bits."""
    if isinstance(v, dict):
        return tuple((k, bits(v[k])) for k in sorted(v))
    if isinstance(v, (tuple, list)):
        return tuple(bits(x) for x in v)
    if isinstance(v, float):
        return struct.pack('<d', v)
    return v


def snapshot(e):
    snap = {}
    for name in READERS:
        try:
            snap[name] = bits(getattr(e, name)())
        except ValueError as err:                 # BYZ_E_INVALID: the report has no call behind it yet
            assert name in REFUSING and 'on this context yet' in str(err), (name, err)
            snap[name] = 'refused'
    return snap


def make_inputs():
    rng = np.random.default_rng(20240612)
    mu = rng.standard_normal(D)
    g = mu + 0.5 * rng.standard_normal((N, D))
    g[:ATTACKERS] = -2.5 * mu                     # norm about 24, the others' about 11
    g = np.ascontiguousarray(g, dtype=np.float32)
    root = np.ascontiguousarray(mu + 0.5 * rng.standard_normal(D), dtype=np.float32)
    g64 = g.astype(np.float64)
    unit = g64 / np.linalg.norm(g64, axis=1, keepdims=True)
    cosine = np.ascontiguousarray(np.maximum(1.0 - unit @ unit.T, 0.0), dtype=np.float32)
    return g, root, cosine


def build_calls(e, g, root, cosine):
    """(name, the reports DESIGN.md 3.4 lists for it, run): run() makes the call and returns what its own report must be."""
    from attacking_federate_learning_amd.engine import dnc_columns
    g64 = g.astype(np.float64)
    norms = np.linalg.norm(g64, axis=1)

    def geometric_median():
        _, info = e.geometric_median(g, max_iter=5, return_info=True)
        assert 1 <= info['iterations'] <= 5 and info['excluded_rows'] == 0 and info['objective'] > 0.0
        return {'geometric_median_info': (info['iterations'], info['excluded_rows'], info['objective'])}

    def dnc():
        _, good = e.dnc(g, ATTACKERS, dnc_columns(D, 32, n_iters=2, seed=0), return_selection=True)
        assert 1 <= good.size <= N - ATTACKERS
        return {'dnc_info': (good.size, 0)}

    def centered_clip():
        _, info = e.centered_clip(g, tau=1.0, iters=2, return_info=True)
        assert info['clipped_rows'] == N          # tau is far below every row's distance to the centre
        return {'centered_clip_info': (info['clipped_rows'], info['excluded_rows'])}

    def fltrust():
        _, info = e.fltrust(g, root, return_info=True)
        cos = (g64 @ root.astype(np.float64)) / (norms * np.linalg.norm(root.astype(np.float64)))
        assert info['trusted_rows'] == int((cos > 0).sum()) == N - ATTACKERS and info['root_ok']
        assert info['trust_sum'] == pytest.approx(cos[cos > 0].sum(), rel=1e-12)
        return {'fltrust_info': (info['trusted_rows'], info['excluded_rows'], info['root_ok'], info['trust_sum'])}

    def nnm():
        e.nnm(g, N, ATTACKERS)
        return {'nnm_info': (0, 0)}

    def robust_lr():
        theta = 8
        e.robust_lr(g, theta)
        votes = (g > 0).sum(axis=0) - (g < 0).sum(axis=0)
        flipped = int((np.abs(votes) < theta).sum())
        assert flipped > 0
        return {'robust_lr_info': flipped}

    def signguard():
        _, info = e.signguard(g, frac=0.5, return_info=True)
        assert info['kept_rows'] == int(np.count_nonzero(info['keep'])) > 0 and info['median_norm'] > 0.0
        return {'signguard_info': {k: info[k] for k in ('kept_rows', 'norm_failed_rows', 'outside_rows', 'clusters', 'seeds',
                                                        'bandwidth', 'median_norm')}}

    def topk_sparsify():
        _, _, info = e.topk_sparsify(g[5], 10, return_info=True)
        assert info['selected'] == 10 and info['ties'] >= 1 and info['threshold_key'] != 0
        return {'topk_info': info}

    def sparsefed():
        _, _, info = e.sparsefed(g, 7, clip=1.0, return_info=True)
        assert info['selected'] == 7 and info['clipped_rows'] == N
        own = {k: info[k] for k in ('selected', 'threshold_key', 'ties', 'ties_taken')}
        return {'topk_info': own, 'centered_clip_info': (info['clipped_rows'], info['excluded_rows'])}

    def weak_dp():
        _, info = e.weak_dp(g, sigma=0.01, adaptive=True, return_info=True)
        assert info['clip'] == pytest.approx(np.median(norms), rel=1e-12)
        assert info['clipped_rows'] == int((norms > np.median(norms)).sum()) == N // 2
        return {'weak_dp_info': info}

    def flame():
        _, info = e.flame(g, lam=0.001, return_info=True)
        assert info['admitted'] == info['admitted_rows'].size > 0 and info['clip'] > 0.0
        own = {k: info[k] for k in ('admitted', 'broken_rows', 'w_star', 'clip')}
        # launch_clip_scales wrote weak DP's report as well: the same clip, from the same kernel
        return {'flame_info': own, 'weak_dp_info': {'clipped_rows': N // 2, 'excluded_rows': 0, 'clip': info['clip']}}

    def linkage():
        z, usable = e.linkage(cosine)
        assert usable.all() and z.shape == (N - 1, 4)
        info = e.linkage_info()
        assert info['merges'] == N - 1 and 0 <= info['max_rescans'] <= N
        return {'linkage_info': info}

    def clipped_clustering():
        _, info = e.clipped_clustering(g, return_info=True)
        assert info['admitted'] == info['admitted_rows'].size == N - ATTACKERS and info['usable'] == N
        assert info['top_height'] >= info['second_height'] > 0.0
        own = {k: info[k] for k in ('admitted', 'usable', 'top_height', 'second_height', 'clip')}
        assert e.linkage_info()['merges'] == N - 1
        return {'clipped_clustering_info': own, 'weak_dp_info': {'clipped_rows': N // 2, 'excluded_rows': 0, 'clip': info['clip']}}

    def multi_metrics():
        _, info = e.multi_metrics(g, p=0.3, return_info=True)
        assert info['kept'] == info['chosen_rows'].size == int(0.3 * N) and info['usable'] == N
        return {'multi_metrics_info': {k: info[k] for k in ('kept', 'usable', 'degenerate', 'det')}}

    def fang_krum_attack():
        _, info = e.fang_krum_attack(g, ATTACKERS, return_info=True)
        assert info['steps'] >= 1 and info['lambda0'] >= info['lambda'] > 0.0
        return {'fang_krum_info': info}

    return [('geometric_median', {'geometric_median_info'}, geometric_median),
            ('dnc', {'dnc_info'}, dnc),
            ('centered_clip', {'centered_clip_info'}, centered_clip),
            ('fltrust', {'fltrust_info'}, fltrust),
            ('nnm', {'nnm_info'}, nnm),
            ('robust_lr', {'robust_lr_info'}, robust_lr),
            ('signguard', {'signguard_info'}, signguard),
            ('topk_sparsify', {'topk_info'}, topk_sparsify),
            ('sparsefed', {'centered_clip_info', 'topk_info'}, sparsefed),
            ('weak_dp', {'weak_dp_info'}, weak_dp),
            ('flame', {'flame_info', 'weak_dp_info'}, flame),
            ('linkage', {'linkage_info'}, linkage),
            ('clipped_clustering', {'linkage_info', 'clipped_clustering_info', 'weak_dp_info'}, clipped_clustering),
            ('multi_metrics', {'multi_metrics_info'}, multi_metrics),
            ('fang_krum_attack', {'fang_krum_info'}, fang_krum_attack)]


def test_a_call_rewrites_only_its_own_reports(eng):
    from attacking_federate_learning_amd.engine import Engine
    g, root, cosine = make_inputs()
    e = Engine()                                  # its own context: nothing has run on it
    try:
        # before any call: the zeroed block, or the refusal
        for name in READERS:
            if name in REFUSING:
                with pytest.raises(ValueError, match='on this context yet'):
                    getattr(e, name)()
            else:
                report = getattr(e, name)()
                values = report.values() if isinstance(report, dict) else report if isinstance(report, tuple) else (report,)
                assert all(v == 0 for v in values), (name, report)
        calls = build_calls(e, g, root, cosine)
        for order in (calls, calls[::-1]):
            for name, writes, run in order:
                before = snapshot(e)
                own = run()
                after = snapshot(e)
                for reader in READERS:
                    if reader not in writes:
                        assert after[reader] == before[reader], (name, reader, before[reader], after[reader])
                for reader, expected in own.items():
                    assert reader in writes and after[reader] == bits(expected), (name, reader, expected, after[reader])
    finally:
        e.close()
