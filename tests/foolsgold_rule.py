"""FoolsGold's rule (R) of include/byzagg.h in numpy, one fp64 operation at a time: the restatement the device
(tests/test_gpu_foolsgold.py) and csrc/foolsgold_rule.hpp on the host (tests/foolsgold_rule_check.cpp) are held to, a literal
transcription of the authors' published foolsgold() on a Gram, and the recipes of the matrices the tests share."""
import numpy as np

NORMALISE = {'count': 0, 'sum': 1}
LOGIT_BOUND = 4.0 * 2.0 ** -53          # |l_a - l_b| <= kappa * LOGIT_BOUND for two logs that are each within 1 ulp (see the issue)
_ROW_BLOCK = 512                        # the n x n temporaries are formed this many rows at a time


def _positive_max(x):
    """the maximum of every row from +0.0, taking a value only when it is greater: a NaN and a -0.0 never enter"""
    with np.errstate(invalid='ignore'):
        m = np.where(np.isnan(x), 0.0, x).max(axis=1)
        return np.where(m > 0.0, m, 0.0)


def _cosines(C, r, rows):
    """cs of the rows `rows` (a slice): 0 on the diagonal, against an excluded or zero-norm row, and where it is a NaN"""
    n = C.shape[0]
    part = r > 0.0
    with np.errstate(all='ignore'):
        cs = C[rows] / (r[rows, None] * r[None, :])
    valid = part[rows, None] & part[None, :]
    valid[np.arange(valid.shape[0]), np.arange(n)[rows]] = False
    return np.where(np.isnan(cs) | ~valid, 0.0, cs), valid


def restated_foolsgold_weights(C, kappa=1.0, normalise='count'):
    """(R) 1 to 8 and T on an n x n fp64 Gram.  Returns {usable (bool), r, maxcs (m), alpha (a), raw (v), top, rescaled (w),
    weights (l), divisor (T), degenerate, usable_rows, excluded_rows, at_zero, at_one}."""
    C = np.ascontiguousarray(C, dtype=np.float64)
    n = C.shape[0]
    assert C.shape == (n, n) and np.isfinite(kappa) and kappa > 0 and normalise in NORMALISE
    diag = np.diagonal(C).copy()
    usable = np.isfinite(diag) & (diag >= 0.0)
    r = np.where(usable, np.sqrt(np.where(usable, diag, 0.0)), -1.0)
    m = np.zeros(n)
    for lo in range(0, n, _ROW_BLOCK):
        rows = slice(lo, min(n, lo + _ROW_BLOCK))
        m[rows] = _positive_max(_cosines(C, r, rows)[0])
    a = np.zeros(n)
    for lo in range(0, n, _ROW_BLOCK):
        rows = slice(lo, min(n, lo + _ROW_BLOCK))
        cs, valid = _cosines(C, r, rows)
        with np.errstate(all='ignore'):
            p = np.where(m[rows, None] < m[None, :], (cs * m[rows, None]) / m[None, :], cs)
        a[rows] = _positive_max(np.where(valid, p, 0.0))
    v = np.minimum(1.0, np.maximum(0.0, 1.0 - a))
    count = int(usable.sum())
    top = float(v[usable].max()) if count else 0.0
    degenerate = count >= 2 and top == 0.0
    if count < 2:
        w = usable.astype(np.float64)
        l = w.copy()
    elif degenerate:
        w, l = np.zeros(n), np.zeros(n)
    else:
        w = v / top
        w[w == 1.0] = 0.99
        with np.errstate(all='ignore'):
            l = kappa * (np.log(w / (1.0 - w)) + 0.5)
        l = np.where(w == 0.0, 0.0, l)
        l = np.minimum(1.0, np.maximum(0.0, l))
        w, l = np.where(usable, w, 0.0), np.where(usable, l, 0.0)
    if normalise == 'count':
        total = float(count)
    else:
        total = 0.0
        for x in l.tolist():                # ascending row order, from +0.0
            total = total + x
    return dict(usable=usable, r=r, maxcs=m, alpha=a, raw=v, top=top, rescaled=w, weights=l, divisor=total, degenerate=bool(degenerate),
                usable_rows=count, excluded_rows=n - count, at_zero=int((l[usable] == 0.0).sum()), at_one=int((l[usable] == 1.0).sum()))


def authors_foolsgold(C, kappa=1.0):
    """The authors' foolsgold() (github.com/DistributedML/FoolsGold, ML/code/model_aggregator.py) with its double loop kept,
    on the cosines of a Gram whose diagonal is finite and positive: `cosine_similarity(grads) - eye` is the cosine matrix with
    its diagonal taking part as 0."""
    C = np.asarray(C, dtype=np.float64)
    n_clients = C.shape[0]
    r = np.sqrt(np.diagonal(C))
    cs = C / (r[:, None] * r[None, :])
    np.fill_diagonal(cs, 0.0)
    maxcs = np.max(cs, axis=1)
    for i in range(n_clients):
        for j in range(n_clients):
            if i == j:
                continue
            if maxcs[i] < maxcs[j]:
                cs[i][j] = cs[i][j] * maxcs[i] / maxcs[j]
    wv = 1 - (np.max(cs, axis=1))
    wv[wv > 1] = 1
    wv[wv < 0] = 0
    with np.errstate(divide='ignore', invalid='ignore'):
        wv = wv / np.max(wv)
        wv[(wv == 1)] = .99
        wv = kappa * (np.log(wv / (1 - wv)) + 0.5)
    wv[(np.isinf(wv) + wv > 1)] = 1
    wv[(wv < 0)] = 0
    return wv


def gram64(x):
    """the fp64 Gram of fp32 rows"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    return x @ x.T


# ---- the matrices the tests share ---------------------------------------------------------------------------------------------
PLANTED_HONEST, PLANTED_SYBILS, PLANTED_D, PLANTED_ROUNDS = 30, 6, 400, 4


def planted_rounds(seed, honest=PLANTED_HONEST, sybils=PLANTED_SYBILS, d=PLANTED_D, rounds=PLANTED_ROUNDS):
    """The planted sybils: honest clients c_i + N(0, 1) around a persistent c_i ~ N(0, I), sybils s + N(0, 0.3^2) around one shared
    s.  Drawn in this order: c, s, then per round the honest noise, then the sybil noise.  fp32 rows, honest first."""
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(honest, d))
    s = rng.normal(size=d)
    out = []
    for _ in range(rounds):
        h = c + rng.normal(size=(honest, d))
        y = s + rng.normal(0.0, 0.3, size=(sybils, d))
        out.append(np.vstack([h, y]).astype(np.float32))
    return out


def history_chain(rounds):
    """numpy's float32 += chain: the history after every round"""
    h = np.zeros_like(rounds[0], dtype=np.float32)
    out = []
    for g in rounds:
        h += g.astype(np.float32)
        out.append(h.copy())
    return out


def graded_gram(n, d, seed):
    """weights of every kind: many strictly inside (0, 1), some at 0, some at 1"""
    x = np.random.default_rng(1000 + seed).normal(size=(n, d)).astype(np.float32).astype(np.float64)
    return x @ x.T


def with_edge_cases(C):
    """the edge cases by rule number planted into a copy of a graded Gram of at least 16 rows: a NaN diagonal (1), a negative
    diagonal (1), an infinite diagonal (1), a zero-history row (2), a NaN and a -inf off-diagonal entry under finite diagonals (3, 5)"""
    C = np.array(C, dtype=np.float64)
    n = C.shape[0]
    assert n >= 16
    C[1, 1] = np.nan
    C[4, 4] = -1.0
    C[n - 1, n - 1] = np.inf
    C[6, :] = 0.0
    C[:, 6] = 0.0
    C[2, 9] = C[9, 2] = np.nan
    C[3, 11] = C[11, 3] = -np.inf
    return C


def write_rule_cases(path, cases):
    """The restatement's numbers for tests/foolsgold_rule_check.cpp, every double as its 16 hex digits: per case a line `n kappa
    normalise top T degenerate`, then n lines of C, then the lines usable, m, a, w, l."""
    def hexes(a):
        return ' '.join('%016x' % v for v in np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).ravel())
    with open(path, 'w') as f:
        f.write('%d\n' % len(cases))
        for C, kappa, normalise in cases:
            want = restated_foolsgold_weights(C, kappa, normalise)
            f.write('%d %s %d %s %s %d\n' % (C.shape[0], hexes([kappa]), NORMALISE[normalise], hexes([want['top']]),
                                             hexes([want['divisor']]), int(want['degenerate'])))
            for row in np.asarray(C, dtype=np.float64):
                f.write(hexes(row) + '\n')
            f.write(' '.join(str(int(u)) for u in want['usable']) + '\n')
            for key in ('maxcs', 'alpha', 'rescaled', 'weights'):
                f.write(hexes(want[key]) + '\n')
