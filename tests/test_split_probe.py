"""Input generators for tests/test_gpu_split_exact.py, and the conditions that
keep those GPU tests honest (no GPU needed here).

The MFMA path splits every fp32 x into three bf16 parts h + m + l (8 + 8 + 8
significand bits, csrc/tcsc_mfma.hip split3).  Inputs of at most 10 significant
bits never reach l, so the generators here make inputs that use all 24 bits and
whose sums are still exact in fp32 in any order:

* probe_x / probe_b: small integers plus, in every row, a few wide odd integers
  of ~2^p placed so that every k in [0, K) meets one, everything times a power
  of two.  Every partial sum is an integer below 2^24 times that power.
* onehot_values: one nonzero per row over the whole exponent range, so
  Y[r, j] == W[r, j] * x_r with no sum at all.

split3() is the numpy model of the device's split: mask to the top 16 bits,
subtract, mask again.  The tests below check on the committed shapes what the
GPU tests rely on.
"""
import numpy as np
import pytest

B_MAX = 512          # |bias| <= B_MAX (times the scale)
SMALL = 8            # |small entry| <= SMALL
FLAG_BELOW = np.float32(2.0 ** -100)   # k_split3 flags a row holding a nonzero |x| below this


def split3(x):
    """(h, m, l) as fp32 arrays whose low 16 bits are clear: the three bf16 parts of finite x."""
    x = np.ascontiguousarray(x, np.float32)
    mask = np.uint32(0xFFFF0000)
    h = (x.view(np.uint32) & mask).view(np.float32)
    r = x - h
    m = (r.view(np.uint32) & mask).view(np.float32)
    s = r - m
    l = (s.view(np.uint32) & mask).view(np.float32)
    return h, m, l


def probe_per(M, K):
    """Wide entries per row: rows r = 0 .. M-1 cover k = r * per .. r * per + per - 1 (mod K)."""
    return max(4, -(-K // M))


def probe_p(M, K):
    """Wide entries lie in [2^p, 2^(p+1)): the largest p with per * 2^(p+1) + SMALL * K + B_MAX < 2^24."""
    per = probe_per(M, K)
    p = 0
    while per * 2 ** (p + 2) + SMALL * K + B_MAX < 2 ** 24:
        p += 1
    assert per * 2 ** (p + 1) + SMALL * K + B_MAX < 2 ** 24
    return p


def probe_wide_mask(M, K):
    per = probe_per(M, K)
    rows = np.repeat(np.arange(M), per)
    cols = (rows * per + np.tile(np.arange(per), M)) % K
    mask = np.zeros((M, K), bool)
    mask[rows, cols] = True
    return mask


def probe_x(M, K, seed, scale_exp=0):
    """fp32 (M, K): integers in [-8, 8], a +-1 and `per` wide entries +-v in every row
    (v odd, 2^p <= v < 2^(p+1), all of h, m, l nonzero), times 2^scale_exp."""
    rng = np.random.default_rng(seed)
    per, p = probe_per(M, K), probe_p(M, K)
    assert p >= 16 and K > per, (M, K, per, p)
    X = rng.integers(-SMALL, SMALL + 1, (M, K)).astype(np.float32)
    rows = np.repeat(np.arange(M), per)
    cols = (rows * per + np.tile(np.arange(per), M)) % K
    v = (rng.integers(0, 2 ** p, rows.size) | 2 ** p | 1).astype(np.int64)
    # The middle byte of the 24-bit significand is bits p-8 .. p-15 of v.  Where it is
    # zero, or its leading bit so low that m's 8 bits reach down to v's last bit, l
    # would be 0: set the byte's top bit there (m is then that byte, l the odd rest).
    l = split3(v.astype(np.float32))[2]
    v = np.where(l == 0, v | (1 << (p - 8)), v)
    sign = rng.integers(0, 2, rows.size) * 2 - 1
    X[rows, cols] = (sign * v).astype(np.float32)
    # one entry of magnitude 1 per row, next to the row's wide ones: the smallest nonzero |x|
    X[np.arange(M), (np.arange(M) * per + per) % K] = (rng.integers(0, 2, M) * 2 - 1).astype(np.float32)
    return np.ldexp(X, scale_exp).astype(np.float32)


def probe_b(N, seed, scale_exp=0):
    rng = np.random.default_rng(seed)
    return np.ldexp(rng.integers(-B_MAX, B_MAX + 1, N).astype(np.float32), scale_exp).astype(np.float32)


def expect_f64(X, Wd, B, a=None):
    """float64 X @ Wd + B (exact: every sum is below 2^53 times the scale), cast to fp32
    (exact again: below 2^24 times the scale), then the PReLU in fp32."""
    v64 = X.astype(np.float64) @ Wd.astype(np.float64) + B.astype(np.float64)
    v = v64.astype(np.float32)
    assert np.array_equal(v.astype(np.float64), v64), "the expectation is not exact in fp32"
    return v if a is None else np.where(v < 0, np.float32(a) * v, v)


# ---- one-hot rows over the exponent range -----------------------------------

FLT_MAX = np.finfo(np.float32).max
ONEHOT_UNFLAGGED = [FLT_MAX, FLAG_BELOW, np.float32(2.0 ** -100 * (1 + 2.0 ** -16 + 2.0 ** -23))]
ONEHOT_FLAGGED = [np.nextafter(FLAG_BELOW, np.float32(0)), np.float32(2.0 ** -126), np.float32(2.0 ** -127),
                  np.float32(2.0 ** -149)]


def onehot_values(K, seed):
    """x_r for r < K: random sign, random 24-bit significand with all three bytes nonzero,
    exponents spread over [-100, 127]; then the planted values (at seeded rows, never the
    last ragged 64-block's last row, which keeps a random value)."""
    rng = np.random.default_rng(seed)
    byte = lambda: rng.integers(1, 256, K).astype(np.uint32)  # noqa: E731
    sig = (byte() | 0x80) << 16 | byte() << 8 | byte()  # 2^23 <= sig < 2^24
    e = np.arange(K) % 228 - 100
    e = e[rng.permutation(K)]
    x = np.ldexp(sig.astype(np.float32), (e - 23).astype(np.int32)).astype(np.float32)
    x *= (rng.integers(0, 2, K) * 2 - 1).astype(np.float32)
    planted = ONEHOT_UNFLAGGED + ONEHOT_FLAGGED
    at = rng.permutation(K - 1)[:2 * len(planted)]
    for i, v in enumerate(planted):
        x[at[2 * i]] = v
        x[at[2 * i + 1]] = -v
    assert np.isfinite(x).all() and (x != 0).all()
    return x


def onehot_flagged(x):
    return (x != 0) & (np.abs(x) < FLAG_BELOW)


def onehot_x(x):
    X = np.zeros((x.size, x.size), np.float32)
    X[np.arange(x.size), np.arange(x.size)] = x
    return X


# ---- the conditions, on the shapes the GPU tests use -------------------------

# (M, K, N, density, seed): every probe case of tests/test_gpu_split_exact.py
PROBE_SHAPES = {
    "unsplit_ragged": (200, 701, 300, 0.5, 1100),
    "unsplit_k64": (200, 704, 300, 0.5, 1110),
    "split_256": (256, 4096, 300, 0.5, 1120),
    "split_100": (100, 2050, 1000, 0.5, 1130),
    "split_130": (130, 1024, 257, 0.5, 1140),
    "narrow_64": (64, 4096, 300, 0.5, 1150),
    "narrow_33": (33, 2050, 700, 0.5, 1160),
    "narrow_17": (17, 1000, 520, 0.5, 1170),
    "big_ragged": (2050, 333, 4000, 0.5, 1180),
    "big_split2": (1024, 1100, 8192, 0.5, 1190),
    "transposed": (256, 1024, 512, 0.5, 1200),   # dX = G . W^T: G is 256 x 1024, W 512 x 1024
    "gather": (300, 777, 333, 0.05, 1210),
    "gather_split": (1024, 4096, 96, 0.05, 1220),  # the forward product's K is X's width: 86 chunks to split
    # M * per >= K with per <= 64 allows K <= 64 * M: K = 256 at the small-M path's M = 4
    "small_m": (4, 256, 2048, 0.05, 1230),
}
SCALES = (-101, -100, 0, 100)
SCALED_SHAPES = ("unsplit_ragged", "split_100")


def probe_case(oracle, name, scale_exp=0):
    """(Wd, X, B) of a named case.  W does not depend on the scale."""
    M, K, N, density, seed = PROBE_SHAPES[name]
    return oracle.ternary((K, N), density, seed), probe_x(M, K, seed + 1, scale_exp), probe_b(N, seed + 2, scale_exp)


@pytest.mark.parametrize("name", sorted(PROBE_SHAPES))
def test_probe_conditions(oracle, name):
    M, K, N, density, seed = PROBE_SHAPES[name]
    per, p = probe_per(M, K), probe_p(M, K)
    assert M * per >= K and per <= 64 and p >= 16, (per, p)
    Wd, X, B = probe_case(oracle, name)
    assert X.dtype == np.float32 and X.shape == (M, K) and B.shape == (N,)
    assert np.array_equal(X, np.rint(X)) and np.array_equal(B, np.rint(B))
    wide = probe_wide_mask(M, K)
    assert (np.abs(X[~wide]) <= SMALL).all() and np.abs(B).max() <= B_MAX
    aw = np.abs(X[wide]).astype(np.int64)
    assert ((aw >= 2 ** p) & (aw < 2 ** (p + 1)) & (aw % 2 == 1)).all()
    h, m, l = split3(X)
    assert np.array_equal((h.astype(np.float64) + m) + l, X.astype(np.float64))
    full = (h != 0) & (m != 0) & (l != 0)
    assert np.array_equal(full, wide), "exactly the wide entries use all three parts"
    assert full.any(axis=0).all(), "a k without a full 24-bit entry in any row"
    assert full.any(axis=1).all(), "a row without a wide entry"
    terms = np.abs(X).astype(np.float64) @ np.abs(Wd).astype(np.float64) + np.abs(B)
    print(f"{name}: per {per}, p {p}, max |b| + sum|x w| = {terms.max():.4g} (2^24 = {2 ** 24})")
    assert terms.max() < 2 ** 24
    assert np.abs(X).sum(axis=1).max() + B_MAX < 2 ** 24  # for any W, the transposed one included


@pytest.mark.parametrize("name", SCALED_SHAPES)
def test_probe_scales(oracle, name):
    M, K, N, _, seed = PROBE_SHAPES[name]
    Wd, X0, B0 = probe_case(oracle, name)
    terms = np.abs(X0).astype(np.float64) @ np.abs(Wd).astype(np.float64) + np.abs(B0)
    for s in SCALES:
        _, X, B = probe_case(oracle, name, s)
        assert np.array_equal(X.astype(np.float64), X0.astype(np.float64) * 2.0 ** s)
        assert np.array_equal(B.astype(np.float64), B0.astype(np.float64) * 2.0 ** s)
        h, m, l = split3(X)
        assert np.array_equal((h.astype(np.float64) + m) + l, X.astype(np.float64))
        assert np.array_equal((h != 0) & (m != 0) & (l != 0), probe_wide_mask(M, K))
        tiny = (X != 0) & (np.abs(X) < FLAG_BELOW)
        if s == -101:
            assert tiny.any(axis=1).all(), "a row the split would not flag"
        else:
            assert not tiny.any()
        # every part is a normal bf16 (>= 2^-126), so no MFMA input can be flushed
        parts = np.abs(np.stack([h, m, l]))
        assert parts[parts != 0].min() >= 2.0 ** -126
        assert terms.max() * 2.0 ** s < 2.0 ** (24 + s) and np.isfinite(np.float32(terms.max() * 2.0 ** s))
        y = expect_f64(X, Wd, B, 0.5)
        assert np.isfinite(y).all() and y.dtype == np.float32
    assert terms.max() * 2.0 ** 100 < 2.0 ** 124


@pytest.mark.parametrize("K,seed", [(701, 1300), (1100, 1310), (333, 1320)])
def test_onehot_conditions(K, seed):
    x = onehot_values(K, seed)
    assert x.dtype == np.float32 and x.shape == (K,)
    flagged = onehot_flagged(x)
    for v in ONEHOT_UNFLAGGED:
        assert ((x == v) & ~flagged).any() and ((x == -v) & ~flagged).any(), v
    for v in ONEHOT_FLAGGED:
        assert ((x == v) & flagged).any() and ((x == -v) & flagged).any(), v
    assert flagged.sum() == 2 * len(ONEHOT_FLAGGED)
    h, m, l = split3(x[~flagged])
    assert np.array_equal((h.astype(np.float64) + m) + l, x[~flagged].astype(np.float64))
    parts = np.abs(np.stack([h, m, l]))
    assert parts[parts != 0].min() >= 2.0 ** -123
    full = np.zeros(K, bool)
    full[~flagged] = (h != 0) & (m != 0) & (l != 0)
    assert full.sum() >= K / 2
    assert len(np.unique(np.flatnonzero(full) % 64)) == 64, "a k % 64 residue without a full 24-bit value"
    last = np.arange(K // 64 * 64, K)
    assert K % 64 and full[last].any() and full[K - 1], "the ragged last block"
    e = np.frexp(x[~flagged])[1] - 1
    assert e.min() == -100 and e.max() == 127
    # 0.5 * x is exact from 2^-125 up
    big = np.abs(x) >= 2.0 ** -125
    assert np.array_equal((np.float32(0.5) * x[big]).astype(np.float64) * 2, x[big].astype(np.float64))
