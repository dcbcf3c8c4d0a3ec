"""One rank of ShardedAggregator(HipKernels).flame over RCCL (backend "nccl"), run by tests/test_gpu_flame_sharded.py at world size
1 with BYZ_FORCE_COLLECTIVES=1: the all-reduces of the Gram and of the rows' squared norms are issued although there is nobody
else, and the result must equal the single-GPU library call on the same matrix.  Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.distributed as dist
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local_rank)
    device = torch.device('cuda', local_rank)
    dist.init_process_group('nccl', device_id=device)

    from attacking_federate_learning_amd.engine import Engine
    from attacking_federate_learning_amd.sharded import HipKernels, ShardedAggregator
    from tests.test_gpu_flame import honest_and_opposite, stable_under_the_bound
    eng = Engine(local_rank)
    agg = ShardedAggregator(HipKernels(eng))
    problems = []
    if not agg.always_collective:
        problems.append('BYZ_FORCE_COLLECTIVES=1 did not take')

    n, d = 63, 1500
    g, f = honest_and_opposite(n, d, seed=1563)
    stable, mask = stable_under_the_bound(g)
    if not stable:
        problems.append('the case is not stable under the cosine bound')
    gt = torch.from_numpy(g).to(device)
    want, winfo = eng.flame(gt, lam=0.01, seed=9, round=2, column_offset=6, return_info=True)
    got, info = agg.flame(gt, n, f, 6, lam=0.01, seed=9, round=2, return_info=True)
    if not np.array_equal(info['admitted_rows'], winfo['admitted_rows']) or not np.array_equal(info['admitted_rows'], np.flatnonzero(mask)):
        problems.append('admitted %r, the library call %r' % (info['admitted_rows'].tolist(), winfo['admitted_rows'].tolist()))
    if (info['admitted_rows'] < f).any():
        problems.append('an attacker was admitted')
    if not torch.equal(got.view(torch.int32), want.view(torch.int32)):
        problems.append('%d columns differ' % int((got.view(torch.int32) != want.view(torch.int32)).sum()))
    for key in ('admitted', 'broken_rows', 'w_star', 'clip'):
        if info[key] != winfo[key]:
            problems.append('%s: %r, the library call %r' % (key, info[key], winfo[key]))
    comm = agg.comm_report()
    eng.check()
    print(json.dumps({'ok': not problems, 'problems': problems,
                      'comm': {k: {'calls': v['calls'], 'bytes': v['bytes']} for k, v in comm.items()}}), flush=True)
    dist.destroy_process_group()
    return 0 if not problems else 1


if __name__ == '__main__':
    sys.exit(main())
