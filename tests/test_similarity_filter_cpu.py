"""No GPU: the bracket of option similarity_filter (csrc/similarity_filter.h) restated in numpy -- the f16 hi / lo split under the pass's
scales 2^ea and 2^eb = 2^(ea - 1), the three products accumulated in fp32, eps(j) = asf_eps_rel(d) bn_j max_i an_i + ENC_EPS_ABS --
on the GPU test's inputs: every fit pair's chain lies inside [a - eps, a + eps], the candidates that are no matches stay below 1 % of the
pairs (value 1 does not fall back there), and a per-pair eps an_i bn_j under ONE image scale is violated by one row 2^-28 times smaller."""
import numpy as np
import pytest

import similarity_inputs as si
import similarity_model as sm

ENC_EPS_ABS = np.float32(2e-34)


def eps_rel(d):                        # csrc/assign_filter.h asf_eps_rel
    return np.float32(2.5e-5 if d <= 64 else 9e-5 if d <= 320 else 1.4e-4)


def split(v, e):
    f = np.ldexp(v.astype(np.float32), e)
    hi = f.astype(np.float16)
    return hi.astype(np.float32), (f - hi.astype(np.float32)).astype(np.float16).astype(np.float32)


def filter_values(va, vb):
    """-> (a[na][nb], eps[nb], an[na], bn[nb]) for finite A rows va and B rows vb inside the pass's window"""
    d = va.shape[1]
    ea = 14 - int(np.frexp(np.abs(va).max())[1])
    eb = ea - 1
    ah, al = split(va, ea)
    bh, bl = split(vb, eb)
    acc = (ah @ bh.T + ah @ bl.T + al @ bh.T).astype(np.float32)
    a = np.ldexp(acc, -(ea + eb)).astype(np.float32)
    an = np.sqrt((va.astype(np.float64) ** 2).sum(axis=1))
    n2 = (vb * vb).sum(axis=1, dtype=np.float32)
    bn = np.sqrt(n2) * np.float32(1 + 2e-5) + np.float32(2.0 ** -69)
    eps = eps_rel(d) * (bn * np.float32(an.max() * (1 + 1e-6))) + ENC_EPS_ABS
    assert (np.abs(vb).max(axis=1) <= np.ldexp(1.0, 15 - eb)).all() and (np.sqrt(n2) >= np.ldexp(1.0, -(eb + 3))).all(), "a B row outside the window"
    return a, eps, an, bn


def near_duplicates():
    rng = np.random.default_rng(5)
    x = np.tile(si.table(300)[1][7], (400, 1)).view(np.uint32)
    x = (x + rng.integers(0, 4, size=x.shape).astype(np.uint32)).view(np.float32)
    x[300:] = si.table(300)[1][300:400]
    return x[:40], x[20:330]


def cases():
    for d in (16, 300, 512):
        ids, x = si.table(d)
        a, b = si.matrix_case(d, 33, 200)
        ra, rb = sm.rows_of(ids, a), sm.rows_of(ids, b)
        yield f"d={d}", x[ra[ra >= 0]], x[rb[rb >= 0]], 0.02
    yield ("near-duplicates",) + near_duplicates() + (None,)


@pytest.mark.parametrize("what,va,vb,frac", list(cases()), ids=lambda v: v if isinstance(v, str) else "")
def test_every_fit_pair_lies_inside_its_bracket_and_few_candidates_are_no_matches(what, va, vb, frac):
    a, eps, _, _ = filter_values(va, vb)
    chain = sm.chain(va[:, None, :], vb[None, :, :])
    assert (np.abs(a.astype(np.float64) - chain) <= eps[None, :]).all(), what
    if frac is not None:
        v = np.sort(chain.ravel())
        t = np.float32(v[int((1 - frac) * (v.size - 1))])
        cand = (a + eps[None, :] >= t)
        match = sm.float4gt(chain, t)
        assert (match <= cand).all() and (cand & ~match).sum() < 0.01 * chain.size, (what, int((cand & ~match).sum()))


def test_a_per_pair_eps_under_one_image_scale_is_violated_by_a_small_row():
    """31 rows of the table and one row 2^-28 times smaller: its halves go subnormal in f16 against the image's scale, and its error is
    relative to the LARGEST row -- beyond asf_eps_rel an_i bn_j for its own pairs, inside asf_eps_rel max_i an_i bn_j for all of them.
    The small row's largest error against the per-pair bound at d = 300, by its size: 2^-20: 0.9 %, 2^-24: 11 %, 2^-26: 34 %, 2^-28: 2.2
    times (58 of its 200 pairs): at 2^-20 the per-pair bound still holds, so the case is built at the first size that violates it."""
    ids, x = si.table(300)
    va, vb = x[:32].copy(), x[1000:1200]
    va[5] = np.ldexp(va[5], -28)
    a, eps, an, bn = filter_values(va, vb)
    chain = sm.chain(va[:, None, :], vb[None, :, :]).astype(np.float64)
    err = np.abs(a.astype(np.float64) - chain)
    assert (err <= eps[None, :]).all()
    per_pair = eps_rel(300) * an[:, None] * bn[None, :] + ENC_EPS_ABS
    assert (err[5] > per_pair[5]).any() and (err[np.arange(32) != 5] <= per_pair[np.arange(32) != 5]).all()
