"""SignGuard's columns-layout composition (ShardedAggregator.signguard) on CPU: world sizes 2 and 3 over gloo.

The per-rank kernels are a numpy stand-in built on the restatement of tests/test_signguard.py (TEST ONLY: the package has no
CPU implementation).  Under test: every rank draws the same window and sample, counts its own part of the window -- one rank
of three holds none of it --, ONE all-reduce of 4 N doubles makes the counts and norms whole, and the replicated selection
and the local sums put together are the unsharded restatement's result."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_sharded_gloo import free_port
from tests.test_signguard import alie, restated_census, restated_scaled_sum, restated_select, restated_signguard


class RestatedKernels:
    """numpy stand-in for HipKernels' three SignGuard methods; tensors are CPU torch tensors."""

    def row_signs(self, g_local, window_start, window_len):
        return tuple(torch.from_numpy(v) for v in restated_census(g_local.numpy(), window_start, window_len))

    def signguard_select(self, pos, zero, neg, q, window_len, lower=0.1, upper=3.0, bandwidth=None, sample=None):
        sel = restated_select(pos.numpy(), zero.numpy(), neg.numpy(), q.numpy(), window_len, lower, upper, bandwidth, sample)
        self.last = sel
        return {'keep': torch.from_numpy(sel['keep']), 'weights': torch.from_numpy(sel['weights']),
                'labels': torch.from_numpy(sel['labels']),
                'mk': torch.tensor([sel['median_norm'], float(sel['kept'])], dtype=torch.float64)}

    def scaled_rows_sum(self, g_local, weights, divisor):
        return torch.from_numpy(restated_scaled_sum(g_local.numpy(), weights.numpy(), float(divisor.reshape(-1)[0])))


def worker(rank, world, port, n, d, window, results):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from attacking_federate_learning_amd.sharded import ShardedAggregator
        kern = RestatedKernels()
        agg = ShardedAggregator(kern)
        g = alie(n, d, seed=n + d)
        lo, hi = agg.column_slices(d)[rank]
        g_local = torch.from_numpy(g[:, lo:hi].copy())
        out, info = agg.signguard(g_local, column_offset=lo, total_columns=d, seed=3, window=window, gather=True,
                                  return_info=True)
        results[rank] = {'out': out.numpy(), 'keep': info['keep'].numpy(), 'labels': info['labels'].numpy(),
                         'window': info['window'], 'comm': agg.comm_report(), 'slice': (lo, hi)}
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('world,n,d,window', [(2, 33, 2051, None), (3, 40, 900, (20, 90)), (2, 9, 1025, (1000, 25))])
def test_ranks_equal_the_unsharded_restatement(world, n, d, window):
    from attacking_federate_learning_amd.engine import signguard_sample, signguard_window
    with mp.Manager() as manager:
        results = manager.dict()
        mp.spawn(worker, args=(world, free_port(), n, d, window, results), nprocs=world, join=True)
        results = dict(results)
    g = alie(n, d, seed=n + d)
    the_window = window if window is not None else signguard_window(d, 0.1, 3)
    want, winfo = restated_signguard(g, the_window, signguard_sample(n, 50, 3))
    assert winfo['margin'] >= 1e-9                                  # q's partial sums are added in another order
    if window == (20, 90):
        lo, hi = results[2]['slice']
        assert lo >= 110                                            # the last of three ranks holds none of the window
    for rank in range(world):
        r = results[rank]
        assert tuple(r['window']) == tuple(the_window)
        assert np.array_equal(r['keep'], winfo['keep']) and np.array_equal(r['labels'], winfo['labels'])
        assert np.allclose(r['out'], want, rtol=1e-6, atol=1e-6 * float(np.abs(g).max()))
        census = r['comm']['allreduce_signguard_census']
        assert census['calls'] == 1                                 # one all-reduce, of 4 n doubles
        assert census['bytes'] == 4 * n * 8 * 2 * (world - 1) // world
