"""The Min-Max / Min-Sum rule of include/byzagg.h (rule D) restated in numpy, the seeded cases of its tests, exact moments by
math.fsum and the authors' halving search.  Shared by test_minmax.py (CPU) and test_gpu_minmax.py."""
import math

import numpy as np

CASES = [(20, 64, 0, 1, 0), (50, 1000, 1, 1, 0.1), (65, 257, 2, 3, 0.5), (100, 4099, 3, 0.1, 0.02), (33, 100, 4, 1, 5),
         (9, 5, 5, 1, 0.3), (8, 1025, 6, 1, 0.1)]
KINDS = ('minmax', 'minsum')
PERTURBATIONS = ('unit', 'std', 'sign')
_CACHE = {}


def matrix(n, d, seed, scale, shift):
    key = (n, d, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        g = (rng.standard_normal((n, d)) * scale + shift * rng.standard_normal(d)).astype(np.float32)
        g.setflags(write=False)
        _CACHE[key] = g
    return _CACHE[key]


def known_counts(n):
    return (n, max(2, n // 4))


def statistics(known):
    """the drift attack's mean and population std: numpy's fp32 chains down the rows"""
    mu = np.mean(known, axis=0, dtype=np.float32)
    sigma = (np.var(known, axis=0, dtype=np.float32) ** np.float32(0.5)).astype(np.float32)
    return mu, sigma


def perturbation(name, mu, sigma):
    if name == 'unit':
        nrm = math.sqrt(float(np.sum(mu.astype(np.float64) ** 2)))
        if nrm == 0.0:
            return np.zeros_like(mu)
        return (-mu.astype(np.float64) / nrm).astype(np.float32)
    if name == 'std':
        return -sigma
    if name == 'sign':
        return np.where(mu > 0, np.float32(-1), np.where(mu < 0, np.float32(1), np.float32(0))).astype(np.float32)
    raise ValueError(name)


def dmax_of(known):
    """fl32 of the largest pairwise distance, from fp64 differences"""
    k = known.astype(np.float64)
    best = 0.0
    for i in range(len(k)):
        d = ((k - k[i]) ** 2).sum(1)
        d[i] = 0.0
        best = max(best, float(d.max()))
    return np.float32(math.sqrt(best))


def root(b, c, q):
    s = math.sqrt(b * b + c * q)
    return (s - b) / c if b <= 0.0 else q / (s + b)


def vector(mu, p, gamma):
    """fl32((double)mu + fl64(gamma * (double)p)): the attacker rows"""
    return (mu.astype(np.float64) + gamma * p.astype(np.float64)).astype(np.float32)


def rule(known, kind, mu, sigma, p, dmax=None):
    """The rule on the r known rows.  Returns a dict: gamma, row, bound, c, degenerate, broken, gammas (Min-Max: every row's root)."""
    r = known.shape[0]
    x, m, pd = known.astype(np.float64), mu.astype(np.float64), p.astype(np.float64)
    with np.errstate(all='ignore'):
        diff = m - x
        a = (diff * diff).sum(1)
        b = (pd * diff).sum(1)
        c = float((pd * pd).sum())
    out = {'c': c, 'row': -1, 'degenerate': False, 'broken': False, 'gamma': float('nan'), 'gammas': None, 'a': a, 'b': b}
    if not (np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(c)):
        out['broken'] = True
        out['bound'] = float('nan')
        return out
    A = float(np.add.accumulate(a)[-1])        # in row order
    B = float(np.add.accumulate(b)[-1])
    if kind == 'minmax':
        T = float(np.float64(dmax)) ** 2
        out['bound'] = T
    else:
        amax = float(a.max())
        out['bound'] = r * amax + A
    if c == 0.0 or r == 1:
        out['degenerate'], out['gamma'] = True, 0.0
        return out
    if kind == 'minmax':
        g = np.array([root(float(b[i]), c, max(T - float(a[i]), 0.0)) for i in range(r)])
        out['gammas'] = g
        out['row'] = int(np.argmin(g))
        out['gamma'] = float(g[out['row']])
    else:
        out['row'] = int(np.argmax(a))
        out['gamma'] = root(B, r * c, r * amax)
    return out


def exact_moments(known, mu, p):
    """a_i, b_i, c by math.fsum on the fp64 images of the fp32 data"""
    m, pd = mu.astype(np.float64), p.astype(np.float64)
    a, b = [], []
    for row in known.astype(np.float64):
        diff = m - row
        a.append(math.fsum(diff * diff))
        b.append(math.fsum(pd * diff))
    return np.array(a), np.array(b), math.fsum(pd * pd)


def exact_sqdists(known, mal64):
    """|mal - g_i|^2 of every known row by math.fsum (mal64: the fp64 vector mu + gamma p)"""
    return np.array([math.fsum((mal64 - row) ** 2) for row in known.astype(np.float64)])


def halving_search(feasible, start=10.0, threshold=1e-5):
    """The authors' search (their lamda, lamda_fail, lamda_succ): the largest feasible value it visits"""
    lam, fail, succ = start, start, 0.0
    while abs(succ - lam) > threshold:
        if feasible(lam):
            succ = lam
            lam = lam + fail / 2
        else:
            lam = lam - fail / 2
        fail = fail / 2
    return succ
