"""One call of every composition this change touched, for a rocprofv3 --kernel-trace --stats comparison (BYZ_LIBRARY picks the .so)."""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from attacking_federate_learning_amd.engine import Engine, _check, _vp
from attacking_federate_learning_amd import _native

def matrix(n, d, f, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, d)).astype(np.float32)
    g *= (1.0 + 0.5 * rng.permutation(n) / n).astype(np.float32)[:, None]
    head = g[:f]
    g[:f] = (head.mean(axis=0) - 1.5 * head.std(axis=0)).astype(np.float32)
    g[f + 3] = g[f + 7] + np.float32(1e-4) * rng.standard_normal(d).astype(np.float32)
    return g

eng = Engine(0)
res = {}
for n, d, f in ((100, 20000, 20), (2000, 8192, 400)):
    g = torch.from_numpy(matrix(n, d, f, n)).cuda()
    res['krum%d' % n] = eng.krum(g, n, f).cpu().numpy()
    res['krum_idx%d' % n] = np.asarray(eng.krum(g, n, f, return_index=True))
    res['bulyan%d' % n] = eng.bulyan(g, n, f).cpu().numpy()
    res['dist%d' % n] = eng.pairwise_distances(g).numpy()
g = torch.from_numpy(matrix(100, 20000, 20, 5)).cuda()
out, sel = eng.multi_krum(g, 100, 20, return_selection=True)
res['mk'], res['mk_sel'] = out.cpu().numpy(), sel.cpu().numpy()
g2 = torch.from_numpy(matrix(300, 4096, 60, 6)).cuda()
res['mk300'] = eng.multi_krum(g2, 300, 60).cpu().numpy()
res['geomed'] = eng.geometric_median(g).cpu().numpy()
# the sharded entry points at world size 1 (tests/test_gpu_sharded_cabi.py): the all-reduce is the identity
cb = _native.ALLREDUCE_F64_FN(lambda user, buf, count, stream: 0)
cbp = ctypes.cast(cb, ctypes.c_void_p)
for n, d, f in ((23, 3000, 5), (300, 4096, 60)):
    h = matrix(n, d, f, 7 + n)
    buf = eng.to_device(h)
    out = eng.empty((d,), np.float32)
    idx = ctypes.c_int32(-2)
    _check(eng.lib.byz_krum_sharded_dev(eng.ctx, _vp(buf.ptr), n, d, d, n, f, 1, cbp, None, _vp(out.ptr), ctypes.byref(idx), None))
    res['krum_sh%d' % n], res['krum_sh_idx%d' % n] = out.numpy(), np.asarray(idx.value)
    theta = n - 2 * f
    sel = eng.empty((theta,), np.int32)
    _check(eng.lib.byz_bulyan_sharded_dev(eng.ctx, _vp(buf.ptr), n, d, d, n, f, cbp, None, _vp(out.ptr), _vp(sel.ptr), None))
    eng.check()
    res['bul_sh%d' % n], res['bul_sh_sel%d' % n] = out.numpy(), sel.numpy()
    m = n - f
    msel = eng.empty((m,), np.int32)
    _check(eng.lib.byz_multi_krum_sharded_dev(eng.ctx, _vp(buf.ptr), n, d, d, n, f, m, 1, cbp, None, _vp(out.ptr), _vp(msel.ptr), None))
    eng.check()
    res['mk_sh%d' % n], res['mk_sh_sel%d' % n] = out.numpy(), msel.numpy()
# host paths (staging helper)
h = matrix(23, 2048, 5, 9)
res['host_krum'] = eng.krum(h.copy(), 23, 5)
res['host_bul'] = eng.bulyan(h.copy(), 23, 5)
res['host_mk'] = eng.multi_krum(h.copy(), 23, 5)
res['host_gm'] = eng.geometric_median(h.copy())
res['host_med'] = eng.coordinate_median(h.copy())
res['host_drift'] = np.stack(eng.drift_attack(h[:5].copy(), 1.5))
eng.synchronize()
if len(sys.argv) > 1:
    np.savez(sys.argv[1], **res)
eng.close()
print('launches ok', len(res))
