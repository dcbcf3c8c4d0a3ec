"""One rank of ShardedAggregator(HipKernels).weak_dp over RCCL (backend "nccl"), run by tests/test_gpu_weak_dp.py at world size 1
with BYZ_FORCE_COLLECTIVES=1: the all-reduce of the rows' squared norms is issued although there is nobody else, and both modes
must equal the single-GPU library call on the same matrix bit for bit.  Prints one JSON line."""
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
    from tests.test_geometric_median import attacked
    eng = Engine(local_rank)
    agg = ShardedAggregator(HipKernels(eng))
    problems = []
    if not agg.always_collective:
        problems.append('BYZ_FORCE_COLLECTIVES=1 did not take')

    n, d = 40, 4099
    g = attacked(n, d, seed=70)
    g[1] *= np.float32(40.0)
    g[n - 2, 7] = np.nan
    gt = torch.from_numpy(g).to(device)
    for adaptive, sigma in ((False, 0.05), (True, 0.01)):
        want, winfo = eng.weak_dp(gt, clip=80.0, sigma=sigma, adaptive=adaptive, seed=9, round=2, column_offset=6, return_info=True)
        got, info = agg.weak_dp(gt, n, 0, 6, clip=80.0, sigma=sigma, adaptive=adaptive, seed=9, round=2, return_info=True)
        if not torch.equal(got.view(torch.int32), want.view(torch.int32)):
            problems.append('adaptive=%r: %d columns differ' % (adaptive, int((got.view(torch.int32) != want.view(torch.int32)).sum())))
        if info != winfo:
            problems.append('adaptive=%r: info %r, the library call %r' % (adaptive, info, winfo))
        if not 0 < winfo['clipped_rows'] < n or winfo['excluded_rows'] != 1:
            problems.append('adaptive=%r: the case does not clip or exclude: %r' % (adaptive, winfo))
    comm = agg.comm_report()
    eng.check()
    print(json.dumps({'ok': not problems, 'problems': problems,
                      'comm': {k: {'calls': v['calls'], 'bytes': v['bytes']} for k, v in comm.items()}}), flush=True)
    dist.destroy_process_group()
    return 0 if not problems else 1


if __name__ == '__main__':
    sys.exit(main())
