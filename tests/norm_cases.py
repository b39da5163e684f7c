"""The RMSNorm of DESIGN.md §22 (csrc/tcsc_norm.h) restated in numpy float32, one rounded operation per step, and
the rows the norm tests use.  Shared by tests/test_norm_api.py (CPU: the restatement's order can be told from other
orders on these rows) and tests/test_gpu_norm.py (the kernels' bits against it).

The order of the sum of squares depends on K alone: 512 partials; element k belongs to partial (k >> 3) & 511; a
partial adds fl(x * x) in ascending k from +0; the partials are folded by p[c] = fl(p[c] + p[c + s]) for
s = 256, 128, .., 1.  Then mean = fl(ss / float(K)), r = fl(1 / fl(sqrt(fl(mean + eps)))) and
xn = fl(fl(x * r) * gamma)."""
import numpy as np

PARTIALS = 512
GROUP = 8
EPS = 1e-6

# the K of the tests: around the group of 8, the 256-k block, the 8 waves' K split (2048) and the 4096-element
# round of the 512 partials
KS = (1, 7, 8, 9, 64, 255, 256, 300, 2048, 4095, 4096, 4104)


def np_sumsq(x):
    """ss of every row of x (R x K float32) in the pinned order."""
    x = np.ascontiguousarray(x, np.float32)
    R, K = x.shape
    sq = (x * x).astype(np.float32)
    pad = -K % (PARTIALS * GROUP)  # +0 for the elements that are not there: p + 0 == p for p >= +0
    sq = np.concatenate([sq, np.zeros((R, pad), np.float32)], axis=1).reshape(R, -1, PARTIALS, GROUP)
    p = np.zeros((R, PARTIALS), np.float32)
    for rnd in range(sq.shape[1]):  # ascending k inside every partial
        for e in range(GROUP):
            p = p + sq[:, rnd, :, e]
    s = PARTIALS // 2
    while s >= 1:
        p = p[:, :s] + p[:, s:2 * s]
        s //= 2
    assert p.dtype == np.float32 and p.shape == (R, 1)
    return p[:, 0]


def np_sumsq_sequential(x):
    """The same squares added one after the other in ascending k (np.cumsum adds sequentially)."""
    x = np.ascontiguousarray(x, np.float32)
    return np.cumsum((x * x).astype(np.float32), axis=1, dtype=np.float32)[:, -1]


def np_sumsq_pairwise(x):
    """The same squares under np.sum's pairwise summation."""
    x = np.ascontiguousarray(x, np.float32)
    return np.array([np.sum(row, dtype=np.float32) for row in (x * x).astype(np.float32)], np.float32)


def np_rinv(ss, K, eps=EPS):
    mean = (np.asarray(ss, np.float32) / np.float32(K)).astype(np.float32)
    t = (mean + np.float32(eps)).astype(np.float32)
    r = np.float32(1.0) / np.sqrt(t)
    assert r.dtype == np.float32
    return r


def np_rmsnorm(x, gamma=None, eps=EPS, sumsq=np_sumsq):
    """(xn, r) of the rows of x; gamma None = all ones (the second multiply skipped: the same bits)."""
    x = np.ascontiguousarray(x, np.float32)
    r = np_rinv(sumsq(x), x.shape[1], eps)
    xn = (x * r[:, None]).astype(np.float32)
    if gamma is not None:
        xn = (xn * np.asarray(gamma, np.float32)[None, :]).astype(np.float32)
    return xn, r


def rows_of(K, seed):
    """16 finite fp32 rows whose squares do not overflow: row 0 has its maximum as the last element, row 1 a
    negative maximum, row 2 is all zeros, row 3 has equal magnitudes, row 4 is tiny, the rest are a seeded normal
    sample of mixed scales (the rows of tests/test_gpu_q8.py, without the 1e30 of its K = 1 case)."""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((16, K)) * rng.choice([1e-3, 1.0, 37.0], (16, 1))).astype(np.float32)
    X[0] = np.clip(X[0], -1.0, 1.0)
    X[0, K - 1] = 2.5
    X[1] = np.clip(X[1], -1.0, 1.0)
    X[1, K // 2] = -3.0
    X[2] = 0.0
    X[3] = np.where(rng.random(K) < 0.5, -0.75, 0.75).astype(np.float32)
    X[4] = X[4] * np.float32(1e-20)  # squares of 1e-40: subnormal, and kept
    if K == 1:
        X[:, 0] = [1.5, -2.25, 0.0, 3e-3, -1e-20, 127.0, -127.0, 1.0, -1.0, 0.1, 1e15, -1e-9, 5.0, -6.0, 7.0, 0.5]
    return X


def gamma_of(K, seed):
    """K norm weights of mixed signs and magnitudes, none of them zero."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(K) * rng.choice([0.05, 1.0, 8.0], K)
    g = np.where(np.abs(g) < 1e-3, 0.5, g)
    return g.astype(np.float32)


def seed_of(K, N):
    return 30000 + 3 * K + 5 * N
