"""The int8 calls at the edges of fp32: the arithmetic of csrc/tcsc_quant.h, csrc/tcsc_i8_out.h (and, through
tests/norm_cases.py, csrc/tcsc_norm.h) restated in numpy float32 so that it is valid on ALL of fp32 -- non-finite
values, signed zeros, subnormals, sums of 2^24 and more -- and the inputs that take the kernels there.  Not a test
module: tests/test_i8_edges_cases.py (CPU) asserts that these inputs contain what they claim, and
tests/test_gpu_i8_edges.py compares every int8 route with the restatement.

The yardstick is IEEE arithmetic in numpy, one rounded float32 operation per step:
  quantizer   amax = max |x|;  d = fl(127 / amax);  zero = !(amax > 0) || d == inf;
              scale = zero ? 0 : fl(amax / 127);  inv = zero ? 0 : d;  q = clamp(rint(fl(x inv)), -127, 127)
  value       v = fl(fl(fl(float(S) s) c) + b), float(S) rounded to nearest even (it rounds from |S| = 2^24 + 1 on);
              PReLU v < 0 ? fl(a v) : v (a NaN and -0 are not < 0);  residual y = fl(v + r)
  gates       relu2: r = g < 0 ? 0 : g, h = fl(fl(r r) u);   silu: h = fl(fl(g / fl(1 + exp(-g))) u)
  bf16        a NaN keeps its upper 16 bits with the quiet bit set; everything else rounds to nearest even on the
              fp32 bits (so the finite values from 0x7F7F8000 on round to inf)
Comparison: integer bits; where the expected element is a NaN any NaN of that width is accepted (payload and sign
differ between hosts and the device), everything else -- -0, infinities, subnormals -- bit for bit."""
import numpy as np

import norm_cases as nc

F = np.float32
QUIET = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")


def f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def bits32(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32)


# ---- the yardstick ------------------------------------------------------------------------------------------------------

def np_quantize(x, rule="zero"):
    """(q int8, scale) of the rows of x.  rule 'zero': the rule above; 'unfixed': the quantizer before tiny rows were
    defined -- inv = fl(127 / amax) even where that is inf, and fmaxf(rintf(NaN), -127) = -127 as the device computes
    it -- kept to show that these inputs tell the two apart."""
    x = np.ascontiguousarray(x, np.float32)
    amax = np.max(np.abs(x), axis=1).astype(np.float32)
    with np.errstate(**QUIET):
        d = (F(127.0) / amax).astype(np.float32)
        zero = ~(amax > 0)
        if rule == "zero":
            zero = zero | np.isinf(d)
        scale = np.where(zero, F(0), amax / F(127.0)).astype(np.float32)
        inv = np.where(zero, F(0), d).astype(np.float32)
        t = (x * inv[:, None]).astype(np.float32)
    r = np.rint(t)
    r = np.where(np.isnan(r), F(-127.0), r)  # fmaxf(NaN, -127) = -127: reached by the unfixed rule (0 * inf) alone
    return np.clip(r, -127, 127).astype(np.int8), scale


def quant_threshold():
    """The largest float32 amax for which fl(127 / amax) is +inf (found by nextafter), and the float above it."""
    with np.errstate(**QUIET):
        a = F(127.0) / np.finfo(np.float32).max
        while np.isinf(F(127.0) / a):
            a = np.nextafter(a, F(1))
        while not np.isinf(F(127.0) / a):
            a = np.nextafter(a, F(0))
    return a, np.nextafter(a, F(1))


def int_sums(q, Wd):
    """The exact sums, through a float64 product (every partial sum is an integer below 2^53)."""
    S = q.astype(np.float64) @ np.asarray(Wd).astype(np.float64)
    assert np.abs(S).max(initial=0) < 2 ** 31 and np.array_equal(S, np.rint(S))
    return S.astype(np.int64)


def float_of(S):
    """float(S), rounded to nearest even: int64 -> float64 is exact here, float64 -> float32 rounds to nearest even."""
    return np.asarray(S, np.int64).astype(np.float64).astype(np.float32)


def float_of_int_rule(S, rule="even"):
    """float(S) in integer arithmetic, for the CPU test: 'even' (the contract), 'trunc' (toward zero) and 'away'
    (ties away from zero) -- the last two are the wrong conversions a kernel could have."""
    S = np.asarray(S, np.int64)
    mag = np.abs(S)
    out = np.empty(S.shape, np.float64)
    for idx in np.ndindex(S.shape):
        m = int(mag[idx])
        sh = max(m.bit_length() - 24, 0)
        keep, rest, half = m >> sh, m & ((1 << sh) - 1), (1 << sh) >> 1
        if rule == "even":
            keep += int(rest > half or (rest == half and sh > 0 and keep & 1))
        elif rule == "away":
            keep += int(sh > 0 and rest >= half)
        out[idx] = float(keep << sh) * (1 if S[idx] >= 0 else -1)
    res = out.astype(np.float32)
    assert np.array_equal(res.astype(np.float64), out)  # 24 significant bits: exact
    return res


def i8_value(S, s, c, b, fS=None):
    """v = fl(fl(fl(float(S) s) c) + b) as float32; s or c None: the multiply skipped (x * 1.0f == x for every x that
    is not a NaN, and a NaN stays one).  fS: float(S) by another rule."""
    v = float_of(S) if fS is None else np.asarray(fS, np.float32)
    with np.errstate(**QUIET):
        if s is not None:
            v = v * np.asarray(s, np.float32)[:, None]
        if c is not None:
            v = v * np.asarray(c, np.float32)[None, :]
        v = v + np.asarray(b, np.float32)[None, :]
    assert v.dtype == np.float32
    return v


def prelu(v, a):
    with np.errstate(**QUIET):
        out = np.where(v < 0, F(a) * v, v)
    assert out.dtype == np.float32
    return out


def residual(v, r):
    with np.errstate(**QUIET):
        y = v + np.asarray(r, np.float32)
    assert y.dtype == np.float32
    return y


def relu2(g, u):
    with np.errstate(**QUIET):
        r = np.where(g < 0, F(0), g)
        h = (r * r) * u
    assert h.dtype == np.float32
    return h


def silu_exact(g, u):
    """SiLU at the g of SILU_G alone, where exp(-g) is exactly 0, 1, inf or NaN in any correct library."""
    g = np.asarray(g, np.float32)
    with np.errstate(**QUIET):
        e = np.full(g.shape, np.nan, np.float32)
        e[g == 0] = 1.0
        e[g >= 200] = 0.0
        e[g <= -200] = np.inf
        assert not np.any(np.isnan(e) & ~np.isnan(g)), "silu_exact is defined on SILU_G alone"
        h = (g / (F(1.0) + e)) * u
    assert h.dtype == np.float32
    return h


SILU_G = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 200.0, -200.0, 1e30, -1e30], np.float32)


def np_bf16_bits(v, nan_branch=True):
    """fp32 -> bf16 bits.  nan_branch False: the rounding alone on 32 bits, which turns 0x7F800001 into +inf,
    0x7FFFFFFF into -0 and 0xFFFFFFFF into +0 -- kept to show that these inputs reach the branch."""
    u = bits32(v).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    if nan_branch:
        r = np.where((u & 0x7FFFFFFF) > 0x7F800000, (u >> 16) | 0x40, r)
    return r.astype(np.uint16)


def ybits(v, ytype):
    return np_bf16_bits(v) if ytype == "bf16" else bits32(v).copy()


def is_nan_bits(b):
    b = np.asarray(b)
    if b.dtype == np.uint16:
        return (b & 0x7FFF) > 0x7F80
    return (b & 0x7FFFFFFF) > 0x7F800000


def mismatches(got, want):
    """Indices where got differs from want: a NaN for a NaN, the same bits elsewhere."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    nan = is_nan_bits(want)
    return np.flatnonzero(np.where(nan, ~is_nan_bits(got), got != want).reshape(-1))


def assert_bits(got, want, what):
    bad = mismatches(got, want)
    if bad.size:
        g, w = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {w.size} elements differ, the first at flat index {i}: got "
                             f"{int(g[i]):#x}, expected {int(w[i]):#x}")


# ---- group A: sums of 2^24 and more, long K -------------------------------------------------------------------------------

A_KS = (133120, 133121)
A_N = 40
A_MS = (1, 16, 24, 40)
A_ROWS = 40
# rows made of the extreme values; 15, 23 and 39 are the last live rows of M = 16, 24, 40
A_SPECIAL = {0: "127", 1: "-128", 2: "-127", 3: "alt", 4: "127,126", 15: "-127,-126", 23: "127,126", 39: "-127"}

_a_cases = {}


def group_a(K, density=0.67):
    """W (K x 40 ternary, float32), X (40 x K int8), the exact S, and the three calls' operands."""
    key = (K, density)
    if key in _a_cases:
        return _a_cases[key]
    rng = np.random.default_rng(41000 + K)
    Wd = rng.choice(np.array([-1, 0, 1], np.float32), (K, A_N), p=[density / 2, 1 - density, density / 2])
    Wd[:, 0], Wd[:, 1] = 1.0, -1.0
    spots = (0, K // 2, K - 1)
    for n in (1, 2, 3):
        Wd[:, 1 + n] = 1.0  # columns 2, 3, 4: n zeros
        Wd[list(spots[:n]), 1 + n] = 0.0
        Wd[:, 4 + n] = 1.0  # columns 5, 6, 7: n times -1
        Wd[list(spots[:n]), 4 + n] = -1.0
    X = rng.integers(-128, 128, (A_ROWS, K)).astype(np.int8)
    for m, kind in A_SPECIAL.items():
        if kind == "alt":
            X[m, 0::2], X[m, 1::2] = 127, -128
        else:
            vals = [int(t) for t in kind.split(",")]
            X[m] = vals[0]
            if len(vals) > 1:
                X[m, (K // 3 + 7 * m) % K] = vals[1]
    S = int_sums(X, Wd)
    rng2 = np.random.default_rng(41001 + K)
    c = dict(K=K, Wd=Wd, X=X, S=S)
    c["b_int"] = np.where(np.arange(A_N) % 2 == 0, 0.0, rng2.integers(-3, 4, A_N)).astype(np.float32)
    c["s_pow2"] = (2.0 ** rng2.integers(-3, 4, A_ROWS)).astype(np.float32)
    c["s_float"] = rng2.uniform(0.01, 2.0, A_ROWS).astype(np.float32) * np.where(np.arange(A_ROWS) % 5 == 3, -1, 1).astype(np.float32)
    c["c_float"] = rng2.uniform(0.25, 1.5, A_N).astype(np.float32) * np.where(np.arange(A_N) % 3 == 1, -1, 1).astype(np.float32)
    c["b_float"] = rng2.uniform(-1, 1, A_N).astype(np.float32)
    _a_cases[key] = c
    return c


# scale None + integer bias, fp32 Y; power-of-two scales, fp32 Y; the float tail (float row and column scales and bias)
# into a bf16 Y, and into an fp32 Y, where one fp32 ulp of float(S) stays visible
A_CALLS = ("plain", "pow2", "float", "float32")


def a_operands(c, call):
    """(s, c, b, ytype) of one of the three calls."""
    if call == "plain":
        return None, None, c["b_int"], "f32"
    if call == "pow2":
        return c["s_pow2"], None, c["b_int"], "f32"
    return c["s_float"], c["c_float"], c["b_float"], "bf16" if call == "float" else "f32"


def a_expected(c, call, M, fS=None):
    s, cs, b, ytype = a_operands(c, call)
    fS = None if fS is None else fS[:M]
    return ybits(i8_value(c["S"][:M], None if s is None else s[:M], cs, b, fS), ytype)


def a_per_slab(c, call, M, slabs=2):
    """The wrong order 'a float per slab, the reduce in fp32': K cut into `slabs` runs of whole 128-k blocks, each
    slab's exact sum converted and taken through the row and column scale, the slabs added in float32, then the
    bias."""
    K = c["K"]
    blocks = (K + 127) // 128
    cuts = [min(K, 128 * ((blocks * i) // slabs)) for i in range(slabs + 1)]
    cuts[-1] = K
    s, cs, b, ytype = a_operands(c, call)
    acc = None
    with np.errstate(**QUIET):
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            part = float_of(int_sums(c["X"][:M, lo:hi], c["Wd"][lo:hi]))
            if s is not None:
                part = part * s[:M, None]
            if cs is not None:
                part = part * cs[None, :]
            acc = part if acc is None else (acc + part).astype(np.float32)
        v = acc + b[None, :]
    return ybits(v.astype(np.float32), ytype)


# ---- group B: special values through every tail ----------------------------------------------------------------------------

B_KS = (64, 272, 2049)
B_N = 136
B_ROWS = 65
B_MS = (1, 4, 5, 16, 24, 40, 65)

FLT_MAX, FLT_MIN = 0x7F7FFFFF, 0x00800000
TABLE_BITS = np.array([
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000,            # +-0, +-inf
    0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFFFFFFF, 0x7F800001,  # quiet NaNs of both signs, a signalling pattern
    FLT_MAX, 0x80000000 | FLT_MAX, FLT_MIN, 0x80000000 | FLT_MIN,
    0x007FFFFF, 0x807FFFFF, 0x00000001, 0x80000001,            # the largest and smallest subnormals
    0x3F808000, 0x3F807FFF, 0x3F808001,                        # half a bf16 ulp above an even bf16 value, +-1 ulp
    0x3F818000, 0x3F817FFF, 0x3F818001,                        # ... above an odd one
    0xBF808000, 0xBF818000,                                    # the two ties, negative
    0x7F7F8000, 0x7F7F7FFF, 0x7F7F8001, 0xFF7F8000, 0xFF7F7FFF,  # the finite values that round to bf16 inf, and below
    0x00008000, 0x00008001, 0x00007FFF, 0x80008001, 0x80008000,  # to the smallest bf16 subnormal, and to +-0
    0x00018000, 0x00010000, 0x80010000,                        # a tie above the odd subnormal 0x0001; it; its negative
    0x3F800000, 0xBF800000, 0x40490FDB, 0xC2F6E979, 0x3A83126F,  # ordinary values
], np.uint32)
TABLE = TABLE_BITS.view(np.float32)
PRELU_AS = (0.25, 0.0, -0.0, np.inf, np.nan)

# the classes the CPU test counts in the expected Y, from the fp32 value before the store and the stored bits
F32_CLASSES = ("+0", "-0", "+inf", "-inf", "nan", "+max", "-max", "+min", "-min", "+sub", "-sub", "+subtop", "-subtop",
               "+subbot", "-subbot", "+normal", "-normal")
BF16_CLASSES = ("+0", "-0", "+inf", "-inf", "nan", "+sub", "-sub", "+normal", "-normal", "tie->even down",
                "tie->even up", "below tie", "above tie", "finite->inf", "finite->-inf", "->smallest sub", "tiny->+0",
                "tiny->-0", "nan kept by the branch")


def classes_f32(v):
    u = bits32(v).reshape(-1)
    mag, neg = u & 0x7FFFFFFF, (u >> 31).astype(bool)
    out = set()

    def put(name, mask):
        for sign, m in (("+", mask & ~neg), ("-", mask & neg)):
            if m.any():
                out.add(sign + name)

    put("0", mag == 0)
    put("inf", mag == 0x7F800000)
    if (mag > 0x7F800000).any():
        out.add("nan")
    put("max", mag == FLT_MAX)
    put("min", mag == FLT_MIN)
    put("sub", (mag > 0) & (mag < FLT_MIN))
    put("subtop", mag == 0x007FFFFF)
    put("subbot", mag == 1)
    put("normal", (mag >= FLT_MIN) & (mag < 0x7F800000))
    return out


def classes_bf16(v):
    """Classes of a bf16 store: of the stored bits, and of the rounding that made them."""
    u = bits32(v).reshape(-1)
    h = np_bf16_bits(v).reshape(-1)
    mag, neg = (h & 0x7FFF).astype(np.uint32), (h >> 15).astype(bool)
    finite_in = (u & 0x7FFFFFFF) < 0x7F800000
    low, odd = u & 0xFFFF, ((u >> 16) & 1).astype(bool)
    out = set()
    for name, m in (("0", mag == 0), ("inf", mag == 0x7F80), ("sub", (mag > 0) & (mag < 0x80)),
                    ("normal", (mag >= 0x80) & (mag < 0x7F80))):
        for sign, mm in (("+", m & ~neg), ("-", m & neg)):
            if mm.any():
                out.add(sign + name)
    if (mag > 0x7F80).any():
        out.add("nan")
    nz = finite_in & ((u & 0x7FFFFFFF) != 0)
    for name, m in (("tie->even down", finite_in & (low == 0x8000) & ~odd), ("tie->even up", finite_in & (low == 0x8000) & odd),
                    ("below tie", finite_in & (low == 0x7FFF)), ("above tie", finite_in & (low == 0x8001)),
                    ("finite->inf", finite_in & (h == 0x7F80)), ("finite->-inf", finite_in & (h == 0xFF80)),
                    ("->smallest sub", nz & (mag == 1)), ("tiny->+0", nz & (h == 0)), ("tiny->-0", nz & (h == 0x8000)),
                    ("nan kept by the branch", ((u & 0x7FFFFFFF) > 0x7F800000)
                     & ~is_nan_bits(np_bf16_bits(v, nan_branch=False).reshape(-1)))):
        if m.any():
            out.add(name)
    return out


def table_at(n, shift):
    """n elements of the table from `shift` on, cyclically: each value lands in several columns (lanes), its size is
    odd, so on different positions of a 4-column store."""
    return TABLE[(np.arange(n) + shift) % TABLE.size].copy()


_b_cases = {}


def group_b(K):
    """W, the int8 rows and their float twins, and the ordinary operands of a shape of group B.
    Columns j % 5 == 0 of W are all zeros (S = 0) and columns j % 5 == 1 hold a single +1, at k1; rows m % 4 == 0 of X
    are all zeros (S = 0 in every column), rows m % 4 == 1 hold a single 1, at k1 (S = W[k1, j]: 1 in the single-one
    columns), rows m % 4 == 2 are random with a 1 at k1, rows m % 4 == 3 random.  The float rows are the int8 rows
    scaled so that a row's maximum is 127 s0[m] with s0 a power of two: the quantizer returns the int8 row and the
    scale s0[m], whichever X type carries it (every value is a bf16 value)."""
    if K in _b_cases:
        return _b_cases[K]
    rng = np.random.default_rng(42000 + K)
    N, k1 = B_N, (2 * K) // 3
    Wd = rng.choice(np.array([-1, 0, 1], np.float32), (K, N), p=[0.335, 0.33, 0.335])
    Wd[:, 0::5] = 0.0
    Wd[:, 1::5] = 0.0
    Wd[k1, 1::5] = 1.0
    Xi = rng.integers(-127, 128, (B_ROWS, K)).astype(np.int8)
    Xi[:, 0] = 127  # every random row's maximum
    Xi[0::4] = 0
    Xi[1::4] = 0
    Xi[1::4, k1] = 1
    Xi[2::4, k1] = 1
    s0 = (2.0 ** rng.integers(-2, 3, B_ROWS)).astype(np.float32)
    Xf = Xi.astype(np.float32) * s0[:, None]  # (the single-one rows quantize to a single 127 with scale s0 / 127)
    assert not np.any(bits32(Xf) & 0xFFFF)
    qf, sf = np_quantize(Xf)
    c = dict(K=K, N=N, k1=k1, Wd=Wd, Xi=Xi, Xf=Xf, qf=qf, sf=sf, Si=int_sums(Xi, Wd), Sf=int_sums(qf, Wd))
    c["s"] = (rng.choice(np.array([0.5, 1.0, 0.0123, 3.0], np.float32), B_ROWS)
              * np.where(np.arange(B_ROWS) % 3 == 1, -1, 1)).astype(np.float32)  # negative scales: -0 products
    c["c"] = (rng.choice(np.array([1.0, 0.5, 0.3, 2.0], np.float32), N) * np.where(np.arange(N) % 7 == 3, -1, 1)).astype(np.float32)
    c["b"] = rng.uniform(-2, 2, N).astype(np.float32)
    c["b"][0::9], c["b"][4::9] = 0.0, -0.0
    c["gamma"] = nc.gamma_of(K, 42001 + K)
    _b_cases[K] = c
    return c


def b_scenes(c, kind):
    """The calls of a shape: name -> dict(s, c, b, variant, a, R).  kind 'i8': int8 X with the caller's row scales
    (the table reaches s too); 'q8': float X, the scales are the quantizer's.  R: None, or a shift of the table."""
    N = c["N"]
    i8 = kind == "i8"
    s = c["s"] if i8 else None
    sc = {}

    def c_for(b, flip):
        """The ordinary column scales (flip: negated), negative where b is -0: S = 0 then gives -0 + -0 = -0 on a row
        whose scale is not negative."""
        cc = -c["c"] if flip else c["c"].copy()
        return np.where(bits32(b) == 0x80000000, -np.abs(cc), cc).astype(np.float32)

    sc["b"] = dict(s=s, c=c_for(table_at(N, 0), False), b=table_at(N, 0), variant="basic", a=0.0)
    for n, a in enumerate(PRELU_AS):
        b = table_at(N, 5 + 3 * n)
        sc[f"b prelu a={a}"] = dict(s=s, c=c_for(b, n % 2 == 0), b=b, variant="prelu_basic", a=a)
    sc["c"] = dict(s=s, c=table_at(N, 11), b=c["b"], variant="basic", a=0.0)
    sc["c prelu"] = dict(s=s, c=table_at(N, 30), b=c["b"], variant="prelu_basic", a=0.25)
    big = np.full(B_ROWS, 3e38, np.float32)
    cb = np.where(np.arange(N) % 2 == 0, 4.0, -4.0).astype(np.float32)
    bb = np.where(np.arange(N) % 3 == 0, -np.inf, np.where(np.arange(N) % 3 == 1, np.inf, 1.0)).astype(np.float32)
    # s c = inf (3e38 * 4; for a float X the quantizer's scale times 7.5e37), inf - inf against b, 0 * c on the zero rows
    sc["overflow"] = dict(s=big if i8 else None, c=cb if i8 else (cb * F(7.5e37)), b=bb, variant="basic", a=0.0)
    if i8:
        sc["s"] = dict(s=table_at(B_ROWS, 2), c=c["c"], b=c["b"], variant="basic", a=0.0)
        sc["s prelu"] = dict(s=table_at(B_ROWS, 19), c=None, b=c["b"], variant="prelu_basic", a=0.25)
    sc["R"] = dict(s=s, c=c["c"], b=c["b"], variant="basic", a=0.0, R=0)
    sc["R and b"] = dict(s=s, c=None, b=table_at(N, 17), variant="basic", a=0.0, R=23)
    for d in sc.values():
        d.setdefault("R", None)
    return sc


def every_bf16_class(n, shift):
    """n fp32 values that are bf16 values, walking every class of 16-bit pattern: the table rounded to bf16 (NaNs
    kept), and the bf16 specials themselves."""
    special = np.array([0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7F81, 0xFFFF, 0x7F7F, 0xFF7F, 0x0080, 0x8080,
                        0x007F, 0x807F, 0x0001, 0x8001, 0x3F80, 0xBF80, 0x4049], np.uint32)
    pool = np.concatenate([special, np_bf16_bits(TABLE).astype(np.uint32)])
    return (pool[(np.arange(n) + shift) % pool.size] << 16).view(np.float32)


def b_residual(c, M, ytype, shift):
    """R (M x N float32 values of Y's type): the table along the columns, moved on by one per row."""
    N = c["N"]
    idx = np.arange(N)[None, :] + np.arange(M)[:, None] + shift
    if ytype == "f32":
        return TABLE[idx % TABLE.size].copy()
    return every_bf16_class(N + M, shift)[(idx - shift) % (N + M)]


def b_quantized(c, xt="f32", norm=None):
    """(q, scale, S) of the float rows of a shape as the library quantizes them: norm None, or (gamma or None, eps);
    every value is a bf16 value, so xt changes nothing here."""
    x = c["Xf"]
    if norm is not None:
        x = nc.np_rmsnorm(x, norm[0], norm[1])[0]
    q, s = np_quantize(x)
    return q, s, int_sums(q, c["Wd"])


def b_expected(c, kind, scene, M, ytype, qs=None):
    """(v fp32 before the store, the bits of Y, R or None) of a scene's call on the first M rows; qs: the (S, scale)
    of another quantization of the float rows (the norm forms)."""
    S = (c["Si"] if kind == "i8" else c["Sf"] if qs is None else qs[0])[:M]
    s = scene["s"][:M] if scene["s"] is not None else (None if kind == "i8" else (c["sf"] if qs is None else qs[1])[:M])
    v = i8_value(S, s, scene["c"], scene["b"])
    if scene["variant"] != "basic":
        v = prelu(v, scene["a"])
    R = None
    if scene["R"] is not None:
        R = b_residual(c, M, ytype, scene["R"])
        v = residual(v, R)
    return v, ybits(v, ytype), R


def rbits(R, ytype):
    u = bits32(R)
    if ytype == "f32":
        return u.copy()
    assert not np.any(u & 0xFFFF)
    return (u >> 16).astype(np.uint16)


def b_glu_operands(c, act, M):
    """(Sg, Su, s, cg, bg, cu, bu) of a gated call on the int8 rows: relu2 with g and u from the table -- g = bg and
    u = bu on the zero rows of X -- and silu on an all-zero X (the caller passes zeros) with bg from SILU_G."""
    N = c["N"]
    if act == "relu2":
        return c["Si"][:M], c["Si"][:M, ::-1].copy(), c["s"][:M], c["c"], table_at(N, 3), None, table_at(N, 14)
    zero = np.zeros((M, N), np.int64)
    s = np.where(np.arange(M) % 2 == 0, 1.0, -1.0).astype(np.float32)  # fl(0 * -1) = -0: g = -0 where bg = -0
    return zero, zero, s, None, SILU_G[np.arange(N) % SILU_G.size].copy(), None, table_at(N, 0)


# ---- group C: the quantizer's range ------------------------------------------------------------------------------------------

C_KS = (1, 17, 256, 300)
C_N = 33
C_ROWS = 40
C_MS = (1, 4, 16, 40)
RATIOS = (1.0, 0.5, 1.0 / 254.0, 1.5 / 127.0)
C_ISOLATED = (5, 9, 22, 38)  # the rows that get inf / NaN in the isolation test (finite here)


def c_amaxes():
    """The row maxima of group C, by name."""
    a0, a1 = quant_threshold()
    return {"inf": a0, "above": a1, "1.2e-38": F(1.2e-38), "subnormal": f32(0x00345678)[()], "smallest": f32(0x00000001)[()],
            "FLT_MAX": f32(FLT_MAX)[()], "3e38": F(3e38), "ordinary": F(2.5), "1e-30": F(1e-30)}


C_TINY = ("inf", "above", "1.2e-38", "subnormal", "smallest")
C_ORDER = ("inf", "above", "subnormal", "1.2e-38", "smallest", "ordinary", "FLT_MAX", "3e38", "1e-30", "neglast")


def c_row(K, amax, m, rng, neg_last=False):
    """A row of maximum amax: zeros, -0, and elements at the RATIOS to amax, either sign; the maximum at a position
    that moves with m (neg_last: only as a negative last element)."""
    with np.errstate(**QUIET):
        pool = np.array([0.0, -0.0] + [F(amax) * F(r) for r in RATIOS] + [-(F(amax) * F(r)) for r in RATIOS], np.float32)
    row = pool[rng.integers(0, pool.size, K)]
    if neg_last:
        row = np.where(np.abs(row) >= F(amax), F(0.5) * row, row).astype(np.float32)
        row[K - 1] = -amax
    else:
        row[(3 * m) % K] = amax if m % 2 == 0 else -amax
    return row.astype(np.float32)


_c_cases = {}


def group_c(K, big=True):
    """40 fp32 rows (names in c['names']) and their bf16 forms (rounded by torch, widened), W and a bias.  big False:
    the rows of maximum FLT_MAX and 3e38 become ordinary ones (the norm's squares must not overflow)."""
    key = (K, big)
    if key in _c_cases:
        return _c_cases[key]
    import torch

    rng = np.random.default_rng(43000 + K)
    am = c_amaxes()
    names, rows = [], []
    for m in range(C_ROWS):
        name = C_ORDER[m % len(C_ORDER)]
        if not big and name in ("FLT_MAX", "3e38"):
            name = "ordinary"
        names.append(name)
        rows.append(c_row(K, am["1e-30"], m, rng, True) if name == "neglast" else c_row(K, am[name], m, rng))
    X = np.stack(rows)
    Xb = torch.from_numpy(X).to(torch.bfloat16).to(torch.float32).numpy()
    Xb = np.where(np.isinf(Xb), np.copysign(f32(0x7F7F0000)[()], Xb), Xb)  # FLT_MAX rounds to inf: the largest bf16 value
    # the threshold on the bf16 grid: rows 0 and 1 of the bf16 form get the bf16 values on either side of it
    top = int(bits32(am["inf"]).reshape(-1)[0]) & 0xFFFF0000
    lo, hi = f32(top)[()], f32(top + 0x10000)[()]
    for m, a in ((0, lo), (1, hi)):
        row = c_row(K, a, m, np.random.default_rng(43100 + K + m))
        Xb[m] = torch.from_numpy(row).to(torch.bfloat16).to(torch.float32).numpy()  # the maximum is a bf16 value: kept
        assert not np.any(bits32(Xb[m]) & 0xFFFF)
    Wd = rng.choice(np.array([-1, 0, 1], np.float32), (K, C_N), p=[0.335, 0.33, 0.335])
    c = dict(K=K, names=names, X={"f32": X, "bf16": Xb}, Wd=Wd, b=rng.uniform(-1e-36, 1e-36, C_N).astype(np.float32),
             gamma=nc.gamma_of(K, 43001 + K), bf16_threshold=(lo, hi))
    _c_cases[key] = c
    return c


def c_expected(c, xt, norm=None, rule="zero"):
    """(q, scale, S) of all rows; norm: None, or (gamma or None, eps)."""
    x = c["X"][xt]
    if norm is not None:
        with np.errstate(**QUIET):
            x = nc.np_rmsnorm(x, norm[0], norm[1])[0]
    q, s = np_quantize(x, rule)
    return q, s, int_sums(q, c["Wd"])


def with_nonfinite_rows(X):
    """X with inf / NaN put into the rows C_ISOLATED (those below X's row count)."""
    X = X.copy()
    K = X.shape[1]
    for n, m in enumerate(r for r in C_ISOLATED if r < X.shape[0]):
        X[m, (5 * n) % K] = (np.inf, np.nan, -np.inf, np.nan)[n]
        if n == 3:
            X[m] = np.nan
    return X
