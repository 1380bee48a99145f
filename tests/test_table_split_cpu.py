"""The f16-split dot products of the query x codebook table (csrc/fused5.h query_codebook5_body), modelled in numpy.

The table units form q_p . c as 2^-(eq + ecb) (lo.hi + hi.lo + hi.hi) with f16 operands and a binary32 accumulator.  The
model here takes the same exponents and the same split, forms every product exactly (22 bits: exact in float32) and sums in
float32 -- forwards, backwards and pairwise inside each of the three instructions -- and is compared with the float64 dot
product.  The bound is the per-position term of the derivation at the top of fused5.h, written ONCE below with the same
constants; the sum over twelve positions plus the twelve rint halves must fit what E = 512 u B + 28 scale leaves."""
import numpy as np
import pytest

U = 2.0 ** -24
S = 25
CBF_EXP = 10            # refine.h: the largest finite element lies in [2^9, 2^10)
# fused5.h, "per position", in units of u T with T = |q_p| max|c_p|
REPRESENTATION = 8.0 + 0.1    # sum |r_q c| + |q r_c| (the f16 subnormal part and the second-order term inside the 0.1)
LO_LO = 4.0                   # the dropped product
ACCUMULATION = 54.2 + 0.1     # hi.hi last: 27 roundings of <= 2 u (1 + 2^-9) T; lo.hi and hi.lo before it
DOT_TERM = REPRESENTATION + LO_LO + ACCUMULATION               # 66.4
QUOTIENT = 2.0                # -2 x * inv with inv = 1 / scale rounded
POSITION_TERM = DOT_TERM + QUOTIENT                            # 68.4 (<= the 69 the bracket books)
BOOKED = 69.0
# the rest of e (fused5.h): reference 39, row term 1, s' and s 7, residual 2 -- and what E / 4.2 asks for
OTHER_PARTS = 39.0 + 1.0 + 7.0 + 2.0
E_B, E_SCALE, E_DIV = 512.0, 28.0, 4.2
VMAX = 2730


def exponent(a):
    a = np.abs(np.asarray(a, np.float32))
    a = a[np.isfinite(a)]
    amax = float(a.max()) if a.size else 0.0
    if not amax > 0.0:
        return 0
    return CBF_EXP - int(np.frexp(np.float32(amax))[1])


def split(v, e):
    s = np.ldexp(np.asarray(v, np.float32), e).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        hi = s.astype(np.float16)
        lo = (s - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def f32_sum(terms, acc, order):
    """One instruction: the products `terms` and the incoming accumulator, summed in float32 in the given order."""
    t = [np.float32(x) for x in terms]
    if order == "forwards":
        for x in t:
            acc = np.float32(acc + x)
        return acc
    if order == "backwards":
        s = np.float32(0.0)
        for x in reversed(t):
            s = np.float32(s + x)
        return np.float32(s + acc)
    while len(t) > 1:   # pairwise
        t = [np.float32(t[i] + t[i + 1]) if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
    return np.float32(t[0] + acc)


def model_dot(q, c, eq, ecb, order):
    qh, ql = split(q, eq)
    ch, cl = split(c, ecb)
    f = lambda a, b: (a.astype(np.float32) * b.astype(np.float32)).astype(np.float32)   # exact: 11 x 11 bits
    for a, b in ((ql, ch), (qh, cl), (qh, ch)):   # the products really are exact in float32
        assert np.array_equal(f(a, b).astype(np.float64), a.astype(np.float64) * b.astype(np.float64))
    acc = np.float32(0.0)
    for a, b in ((ql, ch), (qh, cl), (qh, ch)):   # the kernel's order: small products first, hi.hi last
        acc = f32_sum(f(a, b), acc, order)
    return np.float32(np.ldexp(acc, -(eq + ecb)))


def norm_up(v):
    return float(np.sqrt(np.sum(np.asarray(v, np.float64) ** 2)))


def position_errors(q, cb):
    """q: a query's slice [S]; cb: the codewords of the position [n][S].  Largest error of the dot product and of the table
    value before rint, over codewords and summation orders, in units of u T and u 2 T / scale-free (both relative to T)."""
    q = np.asarray(q, np.float32)
    cb = np.asarray(cb, np.float32)
    eq, ecb = exponent(q), exponent(cb)
    T = norm_up(q) * max(norm_up(c) for c in cb)
    worst_dot = worst_val = 0.0
    for c in cb:
        exact = float(np.dot(q.astype(np.float64), c.astype(np.float64)))
        for order in ("forwards", "backwards", "pairwise"):
            x = model_dot(q, c, eq, ecb, order)
            assert np.isfinite(x)
            worst_dot = max(worst_dot, abs(float(x) - exact))
            if T > 0.0:
                # the quotient as the kernel forms it, for a scale at which this position alone fills the range
                sc = np.float32(2.0 * T / VMAX)
                inv = np.float32(1.0) / sc
                val = np.float32(np.float32(np.float32(-2.0) * x) * inv)
                worst_val = max(worst_val, abs(float(val) - (-2.0 * exact / float(sc))) * float(sc))
    return worst_dot, worst_val, T


def rng_cases():
    r = np.random.default_rng(20250)
    cases = {}
    cases["random"] = (r.standard_normal(S), r.standard_normal((24, S)))
    cases["random_small_codebook"] = (r.standard_normal(S) * 3e-3, r.standard_normal((24, S)) * 2.0 ** -20)
    cases["random_large_codebook"] = (r.standard_normal(S) * 50.0, r.standard_normal((24, S)) * 2.0 ** 12)
    big = r.standard_normal(S)
    big[7] *= 2.0 ** 10
    cbig = r.standard_normal((24, S))
    cbig[:, 3] *= 2.0 ** 10
    cases["one_element_2^10_times_the_rest"] = (big, cbig)
    cases["one_codeword_1000_times_its_neighbours"] = (r.standard_normal(S), np.vstack([r.standard_normal((23, S)), 1e3 * r.standard_normal((1, S))]))
    # after scaling the largest element sits in [2^9, 2^10): 2^-23 .. 2^-34 of it lands on f16's subnormals (2^-14 .. 2^-24)
    sub_q = np.concatenate([[1.0], 2.0 ** -np.arange(22, 34, 0.5)])[:S] * (1.0 + 0.3 * r.random(S))
    sub_c = np.tile(np.concatenate([[1.0], 2.0 ** -np.arange(23, 35, 0.5)])[:S], (8, 1)) * (1.0 + 0.3 * r.random((8, S)))
    cases["edge_of_f16_subnormals"] = (sub_q, sub_c)
    cases["subnormal_query_full_codebook"] = (sub_q, r.standard_normal((8, S)))
    cases["all_equal_signs"] = (np.abs(r.standard_normal(S)), np.abs(r.standard_normal((24, S))))
    a = r.standard_normal(S)
    cc = np.abs(r.standard_normal((24, S)))
    a[1::2] = -a[0:-1:2]          # q_j c_j + q_{j+1} c_{j+1} cancel
    cc[:, 1::2] = cc[:, 0:-1:2]
    cases["cancelling_pairs"] = (a, cc)
    cases["worst_rounding"] = (np.full(S, 1.0 + 2.0 ** -11 + 2.0 ** -23), np.full((4, S), 1.0 + 2.0 ** -11 + 2.0 ** -22))
    cases["zero_slice"] = (np.zeros(S), r.standard_normal((8, S)))
    cases["zero_codebook"] = (r.standard_normal(S), np.zeros((8, S)))
    return cases


CASES = rng_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_split_dot_product_stays_below_the_position_term(name):
    q, cb = CASES[name]
    dot_err, val_err, T = position_errors(q, cb)
    print(f"{name}: dot error {dot_err / (U * T) if T else 0.0:.3f} u T (term {DOT_TERM}), value error "
          f"{val_err / (U * 2 * T) if T else 0.0:.3f} u 2T (term {POSITION_TERM})")
    assert dot_err <= DOT_TERM * U * T
    assert val_err <= POSITION_TERM * U * 2.0 * T
    if T == 0.0:
        assert dot_err == 0.0


def test_zero_and_nonfinite_slices_give_no_nan_exponent():
    assert exponent(np.zeros(S)) == 0
    assert exponent([np.inf] + [0.0] * (S - 1)) == 0
    assert exponent([np.nan] * S) == 0
    v = np.zeros(S)
    v[0] = np.inf
    v[1] = 3.0
    e = exponent(v)
    assert e == CBF_EXP - 2      # the largest FINITE element decides
    hi, lo = split(v, e)
    assert np.isinf(hi[0]) and np.isnan(lo[0]) and np.isfinite(hi[1:]).all() and np.isfinite(lo[1:]).all()
    hi, lo = split(np.zeros(S), 0)
    assert not hi.any() and not lo.any()


def test_largest_element_lands_below_2_to_the_10():
    r = np.random.default_rng(5)
    for scale in (2.0 ** -120, 2.0 ** -20, 1.0, 2.0 ** 12, 2.0 ** 100):
        v = (r.standard_normal(S) * scale).astype(np.float32)
        hi, _ = split(v, exponent(v))
        assert 2.0 ** 9 <= np.abs(hi.astype(np.float64)).max() <= 2.0 ** 10


def test_twelve_positions_fit_what_E_leaves():
    m = 12
    assert POSITION_TERM <= BOOKED
    # the booked term itself fits: e = (OTHER_PARTS + BOOKED) u B + 6 scale <= E / 4.2
    assert OTHER_PARTS + BOOKED <= E_B / E_DIV and m * 0.5 <= E_SCALE / E_DIV
    names = sorted(n for n in CASES if not n.startswith("zero"))
    for shift in range(3):
        picks = [names[(i + shift) % len(names)] for i in range(m)]
        total, B, scale = 0.0, 0.0, 0.0
        for n in picks:
            q, cb = CASES[n]
            _, val_err, T = position_errors(q, cb)
            qn = norm_up(np.asarray(q, np.float32))
            cmax = max(norm_up(c) for c in np.asarray(cb, np.float32))
            total += val_err
            B += (qn + cmax) ** 2            # filter_width5 with pmax = max|c_p| (no coarse part: the smallest B)
            scale = max(scale, 2.0 * qn * cmax / VMAX)
        allowance = (E_B * U * B + E_SCALE * scale) / E_DIV - OTHER_PARTS * U * B
        print(f"shift {shift}: table error {total:.3e} + rint {m * 0.5 * scale:.3e} against {allowance:.3e}")
        assert total + m * 0.5 * scale <= allowance
