"""tests/i8_edge_cases.py checked on the CPU: the inputs of tests/test_gpu_i8_edges.py contain what that file claims to
exercise, and the numpy yardstick can tell the faults it is there to catch -- a truncating or ties-away float(S), a
float taken per K slab, a bf16 rounding without its NaN branch, the quantizer before tiny rows were defined -- from
the contract on exactly these inputs.  A case generator that silently misses its edge fails here, without a GPU."""
import numpy as np
import pytest

import i8_edge_cases as ec
import norm_cases as nc

TWO24 = 2 ** 24


# ---- the yardstick itself ------------------------------------------------------------------------------------------------

def test_float_of_rounds_to_nearest_even():
    S = np.array([0, 1, -1, TWO24, TWO24 + 1, TWO24 + 2, TWO24 + 3, -(TWO24 + 1), -(TWO24 + 3), 2 ** 25 + 2, 2 ** 25 + 6,
                  2 ** 31 - 1, -(2 ** 31) + 1, 2 ** 25 + 3, 2 ** 25 + 5], np.int64)
    want = np.array([0, 1, -1, TWO24, TWO24, TWO24 + 2, TWO24 + 4, -TWO24, -(TWO24 + 4), 2 ** 25, 2 ** 25 + 8, 2 ** 31,
                     -(2 ** 31), 2 ** 25 + 4, 2 ** 25 + 4], np.float64)
    assert np.array_equal(ec.float_of(S).astype(np.float64), want)
    assert np.array_equal(ec.float_of_int_rule(S, "even").astype(np.float64), want)
    assert ec.float_of_int_rule(np.array([TWO24 + 3]), "trunc")[0] == TWO24 + 2
    assert ec.float_of_int_rule(np.array([TWO24 + 1]), "away")[0] == TWO24 + 2


def test_the_bf16_rounding_and_the_comparison_rule():
    v = ec.f32([0x7F800001, 0xFFFFFFFF, 0x7FC00000, 0x7F7F8000, 0x7F7F7FFF, 0x3F808000, 0x3F818000, 0x00008000, 0x00008001])
    assert list(ec.np_bf16_bits(v)) == [0x7FC0, 0xFFFF, 0x7FC0, 0x7F80, 0x7F7F, 0x3F80, 0x3F82, 0x0000, 0x0001]
    assert list(ec.np_bf16_bits(v, nan_branch=False)[:2]) == [0x7F80, 0x0000]  # inf and a carry out of the sign
    want = np.array([0x7FC0, 0x3F80, 0x8000], np.uint16)
    assert ec.mismatches(np.array([0xFFC1, 0x3F80, 0x8000], np.uint16), want).size == 0  # any NaN for a NaN
    assert list(ec.mismatches(np.array([0x7F80, 0x3F80, 0x0000], np.uint16), want)) == [0, 2]  # inf is none; -0 is not +0
    w32 = np.array([0x7FC00000, 0x80000000], np.uint32)
    assert ec.mismatches(np.array([0xFF800001, 0x80000000], np.uint32), w32).size == 0
    assert list(ec.mismatches(np.array([0x7F800000, 0], np.uint32), w32)) == [0, 1]
    with pytest.raises(AssertionError, match="differ"):
        ec.assert_bits(np.array([1], np.uint32), np.array([2], np.uint32), "x")


def test_the_numpy_order_is_the_torch_order_on_finite_values():
    """The restated bf16 rounding is torch's on the table's finite values and infinities, and NaN for NaN."""
    import torch

    got = torch.from_numpy(ec.TABLE.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert ec.mismatches(got, ec.np_bf16_bits(ec.TABLE)).size == 0


# ---- group A ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", ec.A_KS)
def test_group_a_reaches_the_rounding_of_float_S(K):
    c = ec.group_a(K)
    S, W, X = c["S"], c["Wd"], c["X"]
    assert W.shape == (K, ec.A_N) and np.all(W[:, 0] == 1) and np.all(W[:, 1] == -1)
    spots = [0, K // 2, K - 1]
    for n in (1, 2, 3):
        assert np.count_nonzero(W[:, 1 + n] == 0) == n and np.all(W[spots[:n], 1 + n] == 0) and W[:, 1 + n].sum() == K - n
        assert np.count_nonzero(W[:, 4 + n] == -1) == n and np.all(W[spots[:n], 4 + n] == -1) and W[:, 4 + n].sum() == K - 2 * n
    assert set(np.unique(W[:, 8:])) == {-1.0, 0.0, 1.0}
    assert np.all(X[0] == 127) and np.all(X[1] == -128) and np.all(X[2] == -127)
    assert np.all(X[3, 0::2] == 127) and np.all(X[3, 1::2] == -128)
    assert np.count_nonzero(X[4] == 126) == 1 and np.count_nonzero(X[4] == 127) == K - 1
    assert X[5:15].min() == -128 and X[5:15].max() == 127
    big = np.abs(S) >= TWO24
    assert np.count_nonzero(big) >= 16 and np.abs(S).max() < 2 ** 31
    # odd sums are ties between two floats there: |S| = 1 (mod 4) has its even neighbour below, 3 (mod 4) above
    for sign in (1, -1):
        for r in (1, 3):
            assert np.any(big & (np.sign(S) == sign) & (np.abs(S) % 4 == r)), (sign, r)
    for M in ec.A_MS:
        assert np.any(big[M - 1] & (np.abs(S[M - 1]) % 2 == 1)), f"the last live row of M = {M}"
    assert np.array_equal(ec.float_of(S), ec.float_of_int_rule(S, "even"))


@pytest.mark.parametrize("K", ec.A_KS)
def test_group_a_tells_the_wrong_conversions_apart(K):
    """A truncating float(S) and a ties-away float(S) change expected bits of every call with an fp32 Y at every M (and
    of the bf16 call somewhere: one fp32 ulp seldom survives that rounding); a float per K slab changes bits of the
    calls with float scales.  For the two exact calls the per-slab order CANNOT differ at this
    K, and the test says so: a slab of half of K holds |sum| <= 128 K / 2 < 2^24, so each slab converts exactly, the
    one fp32 add of the reduce is the one rounding of the contract, and a power-of-two scale commutes with it."""
    c = ec.group_a(K)
    for rule in ("trunc", "away"):
        fS = ec.float_of_int_rule(c["S"], rule)
        for call in ec.A_CALLS:
            for M in ec.A_MS:
                n = ec.mismatches(ec.a_expected(c, call, M, fS), ec.a_expected(c, call, M)).size
                assert n > 0 or call == "float", (rule, call, M)
    assert 128 * ((K + 1) // 2 + 128) < TWO24
    for M in (24, 40):
        for slabs in (2, 3, 8):
            assert ec.mismatches(ec.a_per_slab(c, "float32", M, slabs), ec.a_expected(c, "float32", M)).size > 0, (M, slabs)
            for call in ("plain", "pow2"):
                assert ec.mismatches(ec.a_per_slab(c, call, M, slabs), ec.a_expected(c, call, M)).size == 0
    # the scaled calls round where the plain one does: the scales are powers of two, or the sums are exact but large
    s, _, b, _ = ec.a_operands(c, "pow2")
    assert np.all(np.log2(s) == np.rint(np.log2(s))) and np.all(b == np.rint(b)) and np.any(b == 0) and np.any(b != 0)


# ---- group B ---------------------------------------------------------------------------------------------------------------

def test_the_table_holds_what_it_names():
    t = ec.TABLE_BITS
    for bits in (0, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00800000, 0x80800000, 0x007FFFFF, 1,
                 0x80000001, 0x7F800001, 0x7F7F8000):
        assert bits in t
    nan = ec.is_nan_bits(t)
    assert np.any(nan & (t >> 31 == 0)) and np.any(nan & (t >> 31 == 1)) and np.any(nan & (t & 0x00400000 == 0))
    assert ec.classes_f32(ec.TABLE) == set(ec.F32_CLASSES)
    assert ec.classes_bf16(ec.TABLE) >= set(ec.BF16_CLASSES) - {"+sub", "-sub"} and len(set(t)) == t.size
    # the finite values at and above 0x7F7F8000 round to inf, the one below does not
    assert list(ec.np_bf16_bits(ec.f32([0x7F7F8000, 0x7F7F8001, 0x7F7F7FFF, 0xFF7F8000]))) == [0x7F80, 0x7F80, 0x7F7F, 0xFF80]
    assert ec.TABLE.size % 2 == 1 and 3 * ec.TABLE.size <= ec.B_N  # a value's columns j, j + size, j + 2 size: three lanes,
    # three positions of a 4-column store
    assert set(ec.PRELU_AS[:2]) == {0.25, 0.0} and np.signbit(ec.PRELU_AS[2]) and np.isinf(ec.PRELU_AS[3]) and np.isnan(ec.PRELU_AS[4])


@pytest.mark.parametrize("K", ec.B_KS)
def test_group_b_places_the_table(K):
    c = ec.group_b(K)
    W, Xi, k1 = c["Wd"], c["Xi"], c["k1"]
    assert not W[:, 0::5].any() and np.all(np.abs(W[:, 1::5]).sum(0) == 1) and np.all(W[k1, 1::5] == 1)
    assert not Xi[0::4].any() and np.all(np.abs(Xi[1::4].astype(int)).sum(1) == 1) and np.all(Xi[1::4, k1] == 1)
    assert not c["Si"][:, 0::5].any() and not c["Si"][0::4].any() and np.all(c["Si"][1::4, 1::5] == 1)
    # the float rows quantize to the int8 rows (the single-one rows to a single 127), with power-of-two scales
    rnd = np.arange(ec.B_ROWS) % 4 >= 2
    assert np.array_equal(c["qf"][rnd], Xi[rnd]) and np.all(c["sf"][0::4] == 0) and np.all(c["qf"][1::4, k1] == 127)
    assert np.all(c["Sf"][1::4, 1::5] == 127)
    # S = 0 with a zero bias of either sign and scales of either sign: both zeros come out of the add
    assert np.any(c["s"] < 0) and np.any(c["c"] < 0) and np.any(ec.bits32(c["b"]) == 0x80000000) and np.any(ec.bits32(c["b"]) == 0)


@pytest.mark.parametrize("kind", ["i8", "q8"])
@pytest.mark.parametrize("K", ec.B_KS)
def test_group_b_every_class_reaches_y(K, kind):
    """Every class of the table is in the expected Y of both types at every M used, counted on the expected bits; and
    the out-of-place residual and every PReLU parameter are among the calls that put them there."""
    c = ec.group_b(K)
    scenes = ec.b_scenes(c, kind)
    assert {"b", "c", "overflow", "R", "R and b"} <= set(scenes) and (kind != "i8" or "s" in scenes)
    assert all(f"b prelu a={a}" in scenes for a in ec.PRELU_AS)
    for M in ec.B_MS:
        seen32, seen16 = set(), set()
        for name, sc in scenes.items():
            v, y, R = ec.b_expected(c, kind, sc, M, "f32")
            seen32 |= ec.classes_f32(v)
            assert np.array_equal(y, ec.bits32(v))
            v, y, R = ec.b_expected(c, kind, sc, M, "bf16")
            seen16 |= ec.classes_bf16(v)
            if R is not None:
                assert not np.any(ec.bits32(R) & 0xFFFF), "a bf16 R holds bf16 values"
        assert seen32 == set(ec.F32_CLASSES), (M, set(ec.F32_CLASSES) - seen32)
        assert seen16 == set(ec.BF16_CLASSES), (M, set(ec.BF16_CLASSES) - seen16)


@pytest.mark.parametrize("K", ec.B_KS)
def test_group_b_reaches_the_prelu_and_overflow_cases(K):
    c = ec.group_b(K)
    for kind in ("i8", "q8"):
        scenes = ec.b_scenes(c, kind)
        for M in ec.B_MS:
            # PReLU: negative v under every a, and -0 and NaN, which the predicate passes unchanged
            for a in ec.PRELU_AS:
                sc = scenes[f"b prelu a={a}"]
                v0 = ec.i8_value((c["Si"] if kind == "i8" else c["Sf"])[:M], sc["s"][:M] if kind == "i8" else c["sf"][:M],
                                 sc["c"], sc["b"])
                assert np.any(v0 < 0) and np.any(ec.bits32(v0) == 0x80000000) and np.any(np.isnan(v0)), (kind, M, a)
                out = ec.prelu(v0, a)
                neg = v0 < 0
                if np.isnan(a):
                    assert np.all(np.isnan(out[neg]))
                elif np.isinf(a):
                    assert np.all(out[neg] == -np.inf)
                elif a == 0:  # 0 * -inf is a NaN; a finite negative v gives the zero of the product's sign
                    fin = neg & np.isfinite(v0)
                    assert np.all(ec.bits32(out[fin]) == (0x80000000 if not np.signbit(a) else 0)) and fin.any()
                    assert np.any(v0 == -np.inf) and np.all(np.isnan(out[v0 == -np.inf]))
                assert np.array_equal(ec.bits32(out[~neg & ~np.isnan(v0)]), ec.bits32(v0[~neg & ~np.isnan(v0)]))
            # s c = inf, inf - inf and 0 * inf
            sc = scenes["overflow"]
            S = (c["Si"] if kind == "i8" else c["Sf"])[:M]
            s = sc["s"][:M] if kind == "i8" else c["sf"][:M]
            with np.errstate(**ec.QUIET):
                p0 = ec.float_of(S) * s[:, None]
                p = p0 * sc["c"][None, :]
                v = p + sc["b"][None, :]
            if M >= 4:
                assert np.any(np.isinf(p) & np.isfinite(p0)), "the column scale overflows it"
                assert np.any(np.isinf(p) & np.isinf(sc["b"])[None, :] & np.isnan(v)), "inf - inf"
            v, _, _ = ec.b_expected(c, kind, scenes["c"], M, "f32")
            zero_times_inf = (S == 0) & np.isinf(scenes["c"]["c"])[None, :]
            assert np.any(zero_times_inf) and np.all(np.isnan(v[zero_times_inf]))


def test_group_b_residual_holds_every_16_bit_class():
    c = ec.group_b(64)
    for M in ec.B_MS:
        R = ec.b_residual(c, M, "bf16", 0)
        h = ec.rbits(R, "bf16")
        mag = h & 0x7FFF
        for m in (mag == 0, mag == 0x7F80, mag > 0x7F80, (mag > 0) & (mag < 0x80), mag == 0x7F7F, mag == 1):
            assert np.any(m & (h >> 15 == 0)) and np.any(m & (h >> 15 == 1)), M
        assert np.any((mag > 0x7F80) & (h & 0x40 == 0)), "a signalling 16-bit pattern"
        assert ec.classes_f32(ec.b_residual(c, M, "f32", 0)) == set(ec.F32_CLASSES)


def test_the_gates():
    g = ec.SILU_G
    u = np.ones_like(g)
    h = ec.silu_exact(g, u)
    want = ec.f32([0, 0x80000000, 0x7F800000, 0x7FC00000, 0x7FC00000, 0x43480000, 0x80000000, 0x7149F2CA, 0x80000000])
    assert ec.mismatches(ec.bits32(h), ec.bits32(want)).size == 0
    assert np.isnan(h[3]), "silu(-inf) = -inf / inf = NaN, not the -0 of a very negative finite g"
    with pytest.raises(AssertionError):
        ec.silu_exact(np.array([1.0], np.float32), u[:1])
    c = ec.group_b(64)
    for M in (4, 40):
        Sg, Su, s, cg, bg, cu, bu = ec.b_glu_operands(c, "relu2", M)
        gg, uu = ec.i8_value(Sg, s, cg, bg), ec.i8_value(Su, s, cu, bu)
        assert ec.classes_f32(gg) == set(ec.F32_CLASSES) and ec.classes_f32(uu) == set(ec.F32_CLASSES)
        hh = ec.relu2(gg, uu)
        assert np.any(np.isnan(hh)) and np.any(np.isinf(hh)) and np.any(ec.bits32(hh) == 0x80000000)
        # relu2 of a NaN is a NaN, of -0 is -0 squared (+0), of -inf is 0 -- times u
        assert np.all(np.isnan(ec.relu2(ec.f32([0x7FC00000]), np.ones(1, np.float32))))
        Sg, Su, s, cg, bg, cu, bu = ec.b_glu_operands(c, "silu", M)
        gg = ec.i8_value(Sg, s, cg, bg)
        assert {int(x) for x in ec.bits32(gg[~np.isnan(gg)])} == {int(x) for x in ec.bits32(g[~np.isnan(g)])}
        assert np.any(np.isnan(gg)) and ec.classes_f32(ec.silu_exact(gg, ec.i8_value(Su, s, cu, bu))) >= {"nan", "+0", "-0", "+inf", "-inf"}


# ---- group C ---------------------------------------------------------------------------------------------------------------

def test_the_threshold():
    a0, a1 = ec.quant_threshold()
    with np.errstate(**ec.QUIET):
        assert np.isinf(np.float32(127) / a0) and np.isfinite(np.float32(127) / a1) and a1 == np.nextafter(a0, np.float32(1))
    assert ec.bits32(a0) == 0x02FE0000 and a0 == np.float32(127.0 * 2.0 ** -128)  # 127 / a0 = 2^128 exactly
    # the kernel's one compare is the rule: on the 4000 floats around the threshold, on every binade, and on 0, -0, NaN
    near = (np.arange(-2000, 2000) + 0x02FE0000).astype(np.uint32).view(np.float32)
    wide = (np.arange(0, 255, dtype=np.uint32) << 23 | 0x123456).view(np.float32)
    edge = ec.f32([0, 0x80000000, 1, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7FC00000])
    for amax in (near, wide, np.nextafter(wide, np.float32(0)), edge):
        with np.errstate(**ec.QUIET):
            rule = ~(amax > 0) | np.isinf(np.float32(127) / amax)
        assert np.array_equal(rule, ~(amax > a0))
    am = ec.c_amaxes()
    for name in ec.C_TINY:
        with np.errstate(**ec.QUIET):
            assert np.isinf(np.float32(127) / am[name]) == (name != "above"), name
    assert 0 < am["subnormal"] < np.finfo(np.float32).tiny and ec.bits32(am["smallest"]) == 1
    with np.errstate(**ec.QUIET):
        assert np.isfinite(np.float32(127) / am["FLT_MAX"]) and np.float32(127) / am["FLT_MAX"] >= np.finfo(np.float32).tiny


@pytest.mark.parametrize("K", ec.C_KS)
def test_group_c_rows_and_the_unfixed_quantizer(K):
    c = ec.group_c(K)
    am = ec.c_amaxes()
    assert c["names"][0] == "inf", "M = 1 is a row below the threshold"
    for xt in ("f32", "bf16"):
        X = c["X"][xt]
        assert np.isfinite(X).all()
        q, s, S = ec.c_expected(c, xt)
        q0, s0, _ = ec.c_expected(c, xt, rule="unfixed")
        amax = np.abs(X).max(1)
        with np.errstate(**ec.QUIET):
            tiny = np.isinf(np.float32(127) / amax) & (amax > 0)  # (bf16: the smallest fp32 subnormal rounds to a zero row)
        assert tiny[0] and not tiny[1]
        for M in ec.C_MS:
            assert np.any(tiny[:M]) and (M == 1 or np.any(~tiny[:M]))
        assert np.all(s[tiny] == 0) and not q[tiny].any() and np.all(s[~tiny & (amax > 0)] > 0)
        # the rule changes nothing elsewhere, and on the tiny rows the unfixed quantizer gives other bits
        assert np.array_equal(q[~tiny], q0[~tiny]) and np.array_equal(s[~tiny], s0[~tiny])
        assert np.any(s0[tiny] > 0) and np.all(np.abs(q0[tiny]) == 127)  # (the smallest subnormal / 127 is 0 either way)
        if K > 1:
            zeros = (X == 0) & tiny[:, None]
            assert zeros.any() and np.all(q0[zeros] == -127), "x = 0 became -127"
            assert np.any(np.signbit(X) & (X == 0)), "-0 is among the elements"
        # every q = 0 for x = 0, whatever the row
        assert not q[X == 0].any()
        if xt == "f32":
            for m, name in enumerate(c["names"]):
                if name == "neglast":
                    assert X[m, K - 1] == -amax[m] and (K == 1 or np.all(np.abs(X[m, :K - 1]) < amax[m])) and q[m, K - 1] == -127
                elif name in am:
                    assert amax[m] == am[name], (m, name)
        elif True:
            big = [m for m, n in enumerate(c["names"]) if n == "FLT_MAX"]
            assert np.all(ec.bits32(amax[big]) == 0x7F7F0000), "the largest bf16 value stands for FLT_MAX"
            if K >= 256:
                for name in ("above", "ordinary", "FLT_MAX", "3e38"):
                    rows = [m for m, n in enumerate(c["names"]) if n == name]
                    vals = set(np.abs(q[rows].astype(int)).reshape(-1))
                    # the ratios 1, 0.5, 1.5 / 127 (a tie unless inv was rounded down) and 1 / 254 (likewise)
                    assert {0, 127} <= vals and vals & {63, 64} and vals & {1, 2}, (name, sorted(vals))
        if xt == "bf16":
            lo, hi = c["bf16_threshold"]
            assert amax[0] == lo and amax[1] == hi and not np.any(ec.bits32(X) & 0xFFFF)
        assert np.all(np.isfinite(s)) and np.abs(S).max() < 2 ** 24


@pytest.mark.parametrize("K", ec.C_KS)
def test_group_c_under_the_norm(K):
    """eps = 1e-6 lifts a tiny row by r = 1000 (its squares underflow): rows at the threshold become ordinary rows,
    the subnormal ones stay below it, and nothing overflows in the rows kept for the norm."""
    c = ec.group_c(K, big=False)
    assert "FLT_MAX" not in c["names"] and "3e38" not in c["names"]
    for xt in ("f32", "bf16"):
        for gamma in (None, c["gamma"]):
            xn, r = nc.np_rmsnorm(c["X"][xt], gamma, nc.EPS)
            assert np.isfinite(xn).all() and np.isfinite(r).all()
            q, s, _ = ec.c_expected(c, xt, (gamma, nc.EPS))
            q0, s0, _ = ec.c_expected(c, xt, (gamma, nc.EPS), rule="unfixed")
            assert np.any(s == 0) and np.any(s > 0) and s[0] > 0
            if xt == "f32":  # (as bf16 that row is a row of zeros, and 1000 x the bf16 subnormal row is above the threshold)
                assert not (np.array_equal(q, q0) and np.array_equal(s, s0)), "the smallest subnormal row stays below it"


def test_the_nonfinite_rows_stand_between_finite_ones():
    c = ec.group_c(17)
    for M in (16, 40):
        X = ec.with_nonfinite_rows(c["X"]["f32"][:M])
        bad = ~np.isfinite(X).all(1)
        assert list(np.flatnonzero(bad)) == [m for m in ec.C_ISOLATED if m < M] and not bad[0] and not bad[M - 1]
        assert np.array_equal(ec.bits32(X[~bad]), ec.bits32(c["X"]["f32"][:M][~bad]))
    assert np.isinf(ec.with_nonfinite_rows(c["X"]["f32"])[5]).any() and np.isnan(ec.with_nonfinite_rows(c["X"]["f32"])[38]).all()
