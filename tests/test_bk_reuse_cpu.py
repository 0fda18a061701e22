"""The model of svd_bk's reused projection (tests/bk_reuse_ref.py) on the CPU: every case reaches the branch it is named for at a
threshold inside a gap of its coefficient maxima, the model itself keeps the bounds B1-B4 with room to spare, taking the guard away
breaks B1 where the cases are meant to bite, and the long-double residual is accurate enough to judge all of it."""
import numpy as np
import pytest

import bk_reuse_ref as R

CASE_NAMES = tuple(R.CASES)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_reaches_its_branch(name):
    p = R.prepared(name)
    c, r = p.case, p.model()
    assert (r.b, r.q) == (p.b, p.q) and r.branch == c.branch, (r.branch, r.flagged_older, r.limit)
    older = r.colmax[:r.q - r.b]
    room = R.MAX_PASS - r.b
    if c.target is not None:
        lo, hi = R.threshold_gap(p)
        assert 0.0 < lo and hi >= 4.0 * lo and hi < 1e7, (lo, hi)  # the gap: a factor 4, below 1e7
        assert abs(np.sqrt(lo * hi) - p.cmax) <= 1e-12 * p.cmax       # ... and the threshold is its geometric middle
    else:
        assert p.cmax == R.DEFAULT_CMAX
    assert r.limit <= 100.0 * p.cmax
    if r.reuse:
        assert r.cmax_dense < r.limit
    if c.branch == 0:
        assert r.flagged_older == 0 and r.limit == p.cmax
    elif c.branch == 1:
        assert 0 < r.flagged_older <= room and r.limit == p.cmax
    elif c.branch == 2:  # raised to the largest flagged: the pass carries the last block alone
        assert r.flagged_older > room and r.limit == np.nextafter(older.max(), np.inf) and len(r.direct) == r.b
    elif c.branch == 3:  # raised to `need`: the pass is exactly as wide as it may be
        assert r.flagged_older > room and p.cmax < r.limit < older.max() and len(r.direct) == R.MAX_PASS
    else:                # too many beyond two decades: a wide pass at the bound as given
        assert r.flagged_older > room and r.limit == p.cmax and len(r.direct) > R.MAX_PASS
    assert r.full_direct == (not r.reuse) and r.last_direct == r.reuse
    assert r.early_projections == (max(c.n_iter - 2, 0) if r.reuse else 0)


def test_named_shapes_of_the_cases():
    """What the cases are named for, beyond the branch."""
    m = {name: R.prepared(name).model() for name in CASE_NAMES}
    assert np.max(m["benign_none"].colmax[:96]) < 1e5
    assert 10 <= m["fits_wide_view"].flagged_older <= 20 and R.MAX_PASS - m["fits_wide_view"].b == 88
    assert R.prepared("fits_tall").dense_f.shape[0] > R.prepared("fits_tall").dense_f.shape[1]  # the rows_ge orientation
    assert m["deep_8_iterations"].flagged_older >= 60 and np.max(m["deep_8_iterations"].colmax) > 1e14
    assert m["deep_8_iterations"].early_projections == 6
    assert m["wide_pass"].flagged_older == 104 and R.MAX_PASS - m["wide_pass"].b == 52
    assert (m["b104_raised_top"].b, m["b100_raised_need"].b, m["b100_default"].b) == (104, 100, 100)
    assert 1 <= m["b100_default"].flagged_older <= 2
    assert (m["two_iterations"].early_projections, m["three_iterations"].early_projections) == (0, 1)
    assert m["odd_block"].b == 7 and m["odd_block"].full_direct
    for name, tr in R.VIEWS:  # a transposed view is the other orientation
        shp = R.prepared(name, tr).dense_f.shape
        assert shp == (R.CASES[name].shape[::-1] if tr else R.CASES[name].shape)


@pytest.mark.parametrize("name,transposed", R.VIEWS)
def test_model_keeps_the_bounds(name, transposed):
    p = R.prepared(name, transposed)
    for cm in R.settings(p):
        r, ra = R.model_ratios(p, cm)
        print(f"{name} t={int(transposed)} cmax {cm:.3g}: branch {r.branch} " + " ".join(f"{k} {v:.3g}" for k, v in ra.items()))
        assert ra["self"] < 2.0 ** -8, (cm, ra)  # the residual reference's own error against the bound it judges
        for key in ("b1", "b2", "b3", "b4_lower"):
            assert ra[key] <= 0.5, (cm, key, ra)
        assert ra["b4_upper"] <= 1.0, (cm, ra)


def test_kappa_u_is_four_times_the_models_worst():
    worst = 0.0
    for name, tr in R.VIEWS:
        p = R.prepared(name, tr)
        for cm in R.settings(p):
            worst = max(worst, R.model_ratios(p, cm)[1]["b3"] * R.KAPPA_U)
    assert R.KAPPA_U <= 8.0 and 4.0 * worst <= R.KAPPA_U < 4.0 * worst + 0.1, worst


@pytest.mark.parametrize("name", R.TEETH + ("b100_default",))
def test_without_the_guard_the_cases_bite(name):
    p = R.prepared(name)
    r = p.model(R.NO_GUARD)
    assert r.flagged_older == 0 and r.branch == 0 and len(r.direct) == r.b
    at_1e5, _ = R.b1_ratio(p.dense_f, r.q, 1e5, r.u, r.s, r.v)
    at_1, _ = R.b1_ratio(p.dense_f, r.q, 1.0, r.u, r.s, r.v)
    print(f"{name}: without the guard B1 ratio {at_1e5:.3g} at L = 1e5, {at_1:.3g} at L = 1")
    if name in R.TEETH:
        assert at_1e5 > 100.0
    else:  # largest coefficient 2.9e5: inside the bound for L = 1e5, far outside the direct product's (module docstring)
        assert at_1e5 < 1.0 and at_1 > 100.0


def test_residual_reference():
    """A residual the long-double product must resolve: exact triplets of an integer matrix perturbed by a known amount, and the
    self-error against every bound of the grid (held per view by test_model_keeps_the_bounds)."""
    assert np.finfo(np.longdouble).nmant >= 63
    rng = np.random.default_rng(5)
    a = rng.integers(0, 7, size=(60, 23)).astype(np.float64)
    v = np.zeros((23, 2))
    v[3, 0] = v[11, 1] = 1.0  # A v = two columns of A: exact in any precision
    s = np.array([4.0, 2.0])
    u = a[:, [3, 11]] / s
    res, err = R.residual(a, u, s, v)
    assert np.all(res == 0.0) and np.all(err < 1e-16)
    u[7, 1] += 2.0 ** -40
    res, _ = R.residual(a, u, s, v)
    assert res[0] == 0.0 and res[1] == 2.0 ** -39
    # wide orientation: op(A) = A^T, the Q side is U
    res_t, _ = R.residual(a.T.copy(), v, s, u)
    assert res_t[1] == 2.0 ** -39
    # a product f64 cannot hold: (2**53 + 1) needs 54 bits
    a2 = np.array([[2.0 ** 53, 1.0], [1.0, 0.0], [0.0, 1.0]])
    res, _ = R.residual(a2, np.array([[2.0 ** 53], [1.0], [1.0]]), np.array([1.0]), np.array([[1.0], [1.0]]))
    assert res[0] == 1.0
