"""SignGuard over two ranks through the C ABI (byz_signguard_sharded_dev), in the manner of tests/test_gpu_sharded_cabi.py:
two contexts on two threads, the all-reduce formed on the host.  Each rank counts its part of the global window -- the cut
falls inside the window, and in a second case one rank holds none of it --; exactly ONE all-reduce of 4 n doubles per rank;
the same keep set, labels and weights on both ranks; the concatenated slices within the single call's tolerance."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_signguard import close
from tests.test_signguard import MARGIN, case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('cut', [1100, 4000])
def test_two_ranks_through_the_c_abi(eng, cut):
    from attacking_federate_learning_amd import _native
    from attacking_federate_learning_amd.engine import _check, _vp
    from tests.test_gpu_sharded_cabi import Rank, TwoRankAllReduce, run_ranks
    n, d = 100, 5000
    g, _, sample, _, _, _ = case(n, d)
    window = (900, 500)                                  # cut = 1100: inside the window; cut = 4000: rank 1 holds none of it
    from tests.test_signguard import restated_signguard
    want, winfo = restated_signguard(g, window, sample)
    assert winfo['margin'] >= MARGIN
    ranks = [Rank(g[:, :cut]), Rank(g[:, cut:])]
    offsets = [0, cut]
    try:
        ar = TwoRankAllReduce(ranks)
        cbs = [ar.callback_for(k) for k in range(2)]

        def local_window(k, rank):
            lo, hi = max(window[0], offsets[k]), min(window[0] + window[1], offsets[k] + rank.d)
            return (lo - offsets[k], hi - lo) if hi > lo else (0, 0)

        def work(k, rank):
            out = rank.eng.empty((rank.d,), np.float32)
            keep = rank.eng.empty((rank.n,), np.int32)
            w = rank.eng.empty((rank.n,), np.float64)
            labels = rank.eng.empty((rank.n,), np.int32)
            dev_sample = rank.eng.to_device(sample)
            params = _native.SignGuardParams(window[0], window[1], 0.1, 3.0, 0.0, len(sample))
            start, length = local_window(k, rank)
            _check(rank.eng.lib.byz_signguard_sharded_dev(rank.eng.ctx, _vp(rank.g.ptr), rank.n, rank.d, rank.d,
                                                          ctypes.byref(params), start, length, _vp(dev_sample.ptr),
                                                          ctypes.cast(cbs[k], ctypes.c_void_p), None, _vp(out.ptr), _vp(keep.ptr),
                                                          _vp(w.ptr), _vp(labels.ptr), None))
            info = rank.eng.signguard_info()
            return out.numpy(), keep.numpy(), w.numpy(), labels.numpy(), info
        res = run_ranks(ranks, work)
        assert ar.calls[0] == ar.calls[1] == [4 * n]              # exactly one all-reduce, of 4 n doubles, per rank
        assert local_window(1, ranks[1])[1] == (300 if cut == 1100 else 0)
        for a, b in zip(res[0][1:4], res[1][1:4]):
            assert np.array_equal(a, b)                           # the same keep set, weights and labels on both ranks
        assert res[0][4] == res[1][4]
        assert np.array_equal(res[0][1], winfo['keep']) and np.array_equal(res[0][3], winfo['labels'])
        assert np.allclose(res[0][2], winfo['weights'], rtol=1e-12, atol=0.0)
        assert close(np.concatenate([res[0][0], res[1][0]]), want, g)
        if cut == 1100:
            cb = ctypes.cast(_native.ALLREDUCE_F64_FN(lambda user, buf, count, stream: 5), ctypes.c_void_p)
            out = ranks[0].eng.empty((ranks[0].d,), np.float32)
            params = _native.SignGuardParams(window[0], window[1], 0.1, 3.0, 0.5, 0)
            rc = ranks[0].eng.lib.byz_signguard_sharded_dev(ranks[0].eng.ctx, _vp(ranks[0].g.ptr), n, cut, cut, ctypes.byref(params),
                                                            900, 200, None, cb, None, _vp(out.ptr), None, None, None, None)
            assert rc == _native.E_COLLECTIVE and 'all-reduce returned 5' in _native.last_error()
            rc = ranks[0].eng.lib.byz_signguard_sharded_dev(ranks[0].eng.ctx, _vp(ranks[0].g.ptr), n, cut, cut, ctypes.byref(params),
                                                            900, 201, None, cb, None, _vp(out.ptr), None, None, None, None)
            assert rc == _native.E_INVALID                        # a local window past the slice
            ranks[0].eng.synchronize()
    finally:
        for rank in ranks:
            rank.close()
