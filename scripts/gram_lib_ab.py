"""One process of a same-box A/B of the long-K Gram between two BUILDS of the library (BYZ_LIBRARY picks the .so; unset: the
tree's own).  One warm-up call and `calls` timed calls of the Gram on a planted matrix made on the device; per call the tile
kernel's ms per launch (HIP events around the launch), the split and the reduction per call, and the SHA-256 of the N x N fp64
Gram.  Alternate processes of the two builds and compare the lines:

    BYZ_LIBRARY=/path/to/parent/libbyzagg.so python scripts/gram_lib_ab.py parent 4000 1000448
    python scripts/gram_lib_ab.py repo 4000 1000448
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    label = sys.argv[1]
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
    d = int(sys.argv[3]) if len(sys.argv) > 3 else 1000448
    calls = int(sys.argv[4]) if len(sys.argv) > 4 else 4
    import torch
    from attacking_federate_learning_amd.engine import get_engine
    eng = get_engine()
    gen = torch.Generator(device='cuda').manual_seed(4100 + n)
    g = torch.randn((n, d), generator=gen, device='cuda', dtype=torch.float32)
    g *= (1.0 + 0.5 * torch.rand((n, 1), generator=gen, device='cuda'))
    torch.cuda.synchronize()
    out = eng.gram(g)
    eng.check()
    tile, split, reduce_, launches = [], [], [], 0
    for _ in range(calls):
        eng.timing(True)
        out = eng.gram(g)
        eng.check()
        t = eng.timing_read()
        launches = t['gram_tile']['launches']
        tile.append(t['gram_tile']['total_ms'] / launches)
        split.append(t['plane_split']['total_ms'])
        reduce_.append(t.get('gram_reduce', {'total_ms': 0.0})['total_ms'])
    eng.timing(False)
    sha = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16]
    print('AB %s n=%d d=%d launches/call=%d gram_tile ms/launch %s | split ms/call %s | reduce ms/call %s | sha %s' % (
        label, n, d, launches, ' '.join('%.3f' % v for v in tile), ' '.join('%.2f' % v for v in split),
        ' '.join('%.2f' % v for v in reduce_), sha), flush=True)


if __name__ == '__main__':
    main()
