"""The exact branch of the sSeq test on the host: `special::nb_term` / `special::nb_add_total` (scan-rs_amd/csrc/special.hpp, the source the device
kernels compile too) through scanrs_host_nb_exact_test, scanrs_host_nb_exact_test_ratio and scanrs_host_nb_log_prob_all, against the
high-precision reference tests/sseq_exact_ref.py.

The cases and their reference values are tests/golden/sseq_exact_table.json (written by tests/golden/make_sseq_exact_table.py; a sample of its
rows is recomputed here); the regimes and bounds are those of tests/sseq_exact_cases.py.

Measured, worst relative error of p per regime. `before`: the library as it was when this battery was written (nb_term added four rounded
ln Γ values to a constant holding -ln Γ(sf_a r) - ln Γ(sf_b r); Ratio left the mirror term to `<=`); `host` / `device`: now, the device on an
MI355X; f64_logspace / f64_ratio: the two double-precision yardsticks of the table, which do not touch the library.

  LogSpace (615 rows)  cases  before     host       device     f64_logspace  f64_ratio  bound
  <15/lo/body            45   3.1e-03 s  7.1e-12    7.1e-12    3.1e-03 s     1.5e-11    6.1e-11
  <15/lo/tail             2   9.3e-12    1.0e-11    1.0e-11    1.0e-11       2.1e-12    4.5e-11
  <1e4/lo/body           56   3.3e-12    3.7e-12    3.7e-12    3.8e-12       2.4e-13    3.8e-11
  <1e4/lo/body/wide       4   7.1e-11    7.6e-11    7.6e-11    7.6e-11       6.4e-14    1.2e-09
  <1e4/lo/tail           32   5.3e-12    3.8e-12    3.8e-12    5.3e-12       4.8e-13    2.7e-11
  <1e4/hi/body           44   5.1e-02 s  4.6e-12    4.6e-12    5.1e-02 s     3.4e-14    8.0e-11
  <1e4/hi/tail           25   3.8e-01 s  1.3e-11    1.3e-11    3.8e-01 s     2.7e-13    8.0e-11
  <1e6/lo/body           18   2.3e-10    1.0e-11    1.0e-11    2.1e-09       4.2e-15    7.2e-11
  <1e6/lo/tail            9   3.6e-10    1.3e-11    1.3e-11    3.6e-10       3.0e-14    7.2e-11
  <1e6/hi/body           85   1.2e-09    1.1e-11    1.1e-11    1.3e-09       2.8e-14    8.7e-11
  <1e6/hi/tail           54   2.6e-09    8.8e-12    9.5e-12    1.4e-09       2.3e-13    8.7e-11
  >=1e6/lo/body           5   3.0e-09    1.6e-11    1.6e-11    2.8e-09       9.7e-16    4.5e-11
  >=1e6/lo/tail           3   4.1e-09    5.8e-12    5.8e-12    2.9e-09       1.4e-14    4.5e-11
  >=1e6/hi/body         140   2.5e-06    2.1e-11    2.1e-11    2.5e-06       2.8e-15    1.0e-10
  >=1e6/hi/body/wide      1   2.1e-11    7.8e-12    7.8e-12    3.4e-10       7.2e-17    1.3e-09
  >=1e6/hi/tail          90   1.8e-06    1.8e-11    1.8e-11    1.8e-06       5.1e-14    1.1e-10
  >=1e6/hi/tail/wide      2   3.2e-10    2.0e-10    2.0e-10    4.7e-09       9.3e-16    1.6e-09

  Ratio (563 rows of its own partition)  before     host       device     f64_ratio  bound
  <15/lo/body            45              3.1e-03 s  1.5e-11    1.5e-11    1.5e-11    5.9e-11
  <15/lo/tail             2              2.1e-12    2.1e-12    2.1e-12    2.1e-12    8.4e-12
  <1e4/lo/body           56              2.4e-13    2.4e-13    2.4e-13    2.4e-13    9.4e-13
  <1e4/lo/body/wide       4              6.4e-14    6.4e-14    6.5e-14    6.4e-14    2.5e-13
  <1e4/lo/tail           27              4.8e-13    4.8e-13    4.8e-13    4.8e-13    1.9e-12
  <1e4/hi/body           44              5.1e-02 s  3.4e-14    3.5e-14    3.4e-14    1.4e-13
  <1e4/hi/tail           21              3.8e-01 s  2.7e-13    2.7e-13    2.7e-13    1.1e-12
  <1e6/lo/body           18              4.2e-15    4.2e-15    3.5e-15    4.2e-15    1.0e-13
  <1e6/lo/tail            6              2.3e-14    2.3e-14    2.2e-14    2.3e-14    1.0e-13
  <1e6/hi/body           85              2.8e-14    2.8e-14    2.8e-14    2.8e-14    1.1e-13
  <1e6/hi/tail           41              1.9e-13    1.9e-13    1.9e-13    1.9e-13    7.6e-13
  >=1e6/lo/body           5              9.7e-16    9.7e-16    5.5e-16    9.7e-16    1.0e-13
  >=1e6/lo/tail           2              1.1e-14    1.1e-14    1.1e-14    1.1e-14    1.0e-13
  >=1e6/hi/body         140              3.3e-02 s  2.8e-15    2.0e-15    2.8e-15    1.0e-13
  >=1e6/hi/body/wide      1              7.2e-17    7.2e-17    7.2e-17    7.2e-17    1.0e-13
  >=1e6/hi/tail          64              4.1e-14    4.1e-14    3.8e-14    4.1e-14    1.7e-13
  >=1e6/hi/tail/wide      2              9.3e-16    9.3e-16    8.7e-16    9.3e-16    1.0e-13
  the 52 rows outside the Ratio partition, against the LogSpace bound of their regime: host 4.1e-13 (its serial sweep goes on below 2^-970),
  device 1.8e-11 (the LogSpace kernels' bits)

  s: the figure is a symmetric row (sf_a == sf_b) whose mirror term was dropped. Apart from those rows `before` was 2.5e-6 at most for
  LogSpace (>=1e6/hi) and equal to `host` for Ratio. f64_ratio is the restatement WITH the library's mirror rule; the reference's own loop
  (and with it the library's host and device Ratio before) drops the mirror in (2000, 30, 50, 50, 20, 0.5): 4.86e-89 for 7.83e-89,
  (450, 440, 5e5, 5e5, 1e-3, 0.13): 0.7377 for 0.7629, (120, 80, 7, 7, 10, 0.3): 0.2175 for 0.2292 and (3, 6142, 0.4, 0.4, 0.8, 0.9): 0.9575 for
  0.9604, and keeps it in their swaps and in (1000, 1049, 2e6, 2e6, 0.8, 0.011). LogSpace before dropped it in the rows of sf = 50, 7 and 0.4.

ln T(k) - ln T(x_a) of scanrs_host_nb_log_prob_all against the reference, worst over k (bound MARGIN x 2^-53 x log_span of the row):
(5, 880, 1.2e3, 1e6, 0.9, 0.005) before 1.3e-06, now 4.9e-12 (bound 1.4e-11); over the fifteen rows of that test now 0.62 of the bound at most.

What was wrong before: at sf / phi = 2e8 the two ln Γ values of a difference of size 1.7e4 are each 3.6e9, and an ulp of that, 4.8e-7, went into
the logarithm of every term independently; and the terms k and n - k of a symmetric test, equal in exact arithmetic, were A + B - C - D and
B + A - D - C, which differ in the last bit often enough. Now each side is ln Γ(s r + k) - ln Γ(s r) - ln k! as one number (Stirling's series of
the difference from 15 on, the raised-argument product below) and a term is the sum of its two sides; the Ratio backend takes the mirror by
its index. The remaining error is the rounding of every term at the size of log_span: no digits are left to gain without dropping the
constant from the terms.

Beyond the table, the two n = 1e6 cases of tests/test_gpu_sseq.py's older battery whose p is above 1e-300, against the same reference
(term cap raised to 2e6): (443853, 556147, sf 2576.5 / 2106.2) gammaln of every argument 9.0e-10, difference form and library 5.5e-10;
(172724, 827276, sf 310.4 / 130.5) 7.7e-10 and 3.4e-10, on opposite sides of the reference (bound of such a row 1.2e-8). That battery's
rtol of 1e-9 is therefore met against the difference form of tests/sseq_ref.py and not against gammaln of every argument.

Near ties: 0 of 615 rows lie within 1e-12 of a tie with another term (mirror rows apart), so no row took the tie route, on the host or the
device. Left out of the table: 109 generated rows whose p is below 1e-300 (x_a = 0 or n, or the 1e-296 tail point, of the wide
distributions). A planted relative error of 1e-10 in one side of nb_term (CPU build, not committed) fails three tests here
(test_host_logspace_against_the_reference, test_symmetric_rows_include_the_mirror_term, test_host_log_terms_against_the_reference) and two
older ones (tests/test_sseq_cpu.py, tests/test_sseq_ratio_cpu.py).
"""
import os
import sys

import mpmath
import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import sseq_exact_cases as xc  # noqa: E402
import sseq_exact_ref as xref  # noqa: E402
import sseq_ratio_ref as rref  # noqa: E402
import sseq_ref  # noqa: E402

ARGS = ("x_a", "x_b", "sf_a", "sf_b", "mu", "phi")
GUARDS = [(0, 0, 1.5, 2.5, 1.0, 0.3), (4, 7, 1.5, 2.5, 1.0, 0.0), (4, 7, 0.0, 2.5, 1.0, 0.3), (4, 7, 1.5, 0.0, 1.0, 0.3)]
# sf / phi up to 2e8, the rest side of a one-vs-rest test, where the earlier form of nb_term lost seven digits: (x_a, x_b, sf_a, sf_b, mu, phi)
LARGE_PARAMETER_ROWS = [(5, 880, 1.2e3, 1e6, 0.9, 0.005), (300, 500, 2e5, 8e5, 1e-3, 0.005), (0, 850, 2e3, 1e6, 0.8, 0.02), (40, 700, 3e3, 9e5, 0.8, 0.011)]


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


@pytest.fixture(scope="module")
def table():
    return xc.load_table()


def _args(r):
    return tuple(r[k] for k in ARGS)


# ---- the reference and the table ----------------------------------------------------------------------------------------------------------
def test_table_rows_are_what_the_helper_computes(table):
    rows = [r for r in table["rows"] if r["x_a"] + r["x_b"] <= 6145][::23] + [r for r in table["rows"] if r["mirror"]][::3]
    assert len(rows) >= 25
    for r in rows:
        v = xref.nb_exact(*_args(r))
        with mpmath.workprec(xref.PREC):
            for k in ("p", "p_lower", "p_upper"):
                assert abs(v[k] - mpmath.mpf(r[k])) <= mpmath.mpf("1e-27") * v[k], (k, r)
        assert v["mirror"] == r["mirror"] and v["log_span"] == r["log_span"]
        assert abs(v["distance"] - r["distance"]) <= 1e-9 * r["distance"] + 1e-60
        assert (r["sar"], r["sbr"]) == (r["sf_a"] * (1.0 / r["phi"]), r["sf_b"] * (1.0 / r["phi"]))
        assert r["in_ratio"] == rref.in_ratio_partition(*_args(r))
        assert r["f64_logspace"] == sseq_ref.nb_exact_test(*_args(r), direct=True) and r["f64_ratio"] == rref.nb_exact_test_ratio(*_args(r))


def test_reference_agrees_with_closed_forms():
    with mpmath.workprec(xref.PREC):
        for sf_a, sf_b, phi in ((1.5, 2.5, 0.3), (7.0, 0.25, 2.0), (3e5, 2e3, 0.011)):
            _, a, b = xref.shape(sf_a, sf_b, phi)
            # n = 1: T(0) : T(1) = b : a
            lo, hi = min(a, b), max(a, b)
            for x_a, t in ((0, b), (1, a)):
                e = mpmath.mpf(1) if t == hi else lo / (a + b)
                assert abs(xref.nb_exact(x_a, 1 - x_a, sf_a, sf_b, 1.0, phi)["p"] - e) < mpmath.mpf("1e-90") * e
            # n = 2: T(0) : T(1) : T(2) = b (b + 1) / 2 : a b : a (a + 1) / 2
            t = [b * (b + 1) / 2, a * b, a * (a + 1) / 2]
            for x_a in range(3):
                e = sum(v for v in t if v <= t[x_a]) / sum(t)
                assert abs(xref.nb_exact(x_a, 2 - x_a, sf_a, sf_b, 1.0, phi)["p"] - e) < mpmath.mpf("1e-90") * e
        # r -> infinity: Binomial(n, sf_a / (sf_a + sf_b)); the first correction is of the order n^2 / (sf r)
        n, sf_a, sf_b, phi = 40, 3.0, 5.0, 2.0 ** -200
        for x_a in (0, 9, 15, 31):
            e = xref.binomial_p(x_a, n, mpmath.mpf(3) / 8)
            assert abs(xref.nb_exact(x_a, n - x_a, sf_a, sf_b, 1.0, phi)["p"] - e) < mpmath.mpf(2) ** -185 * e
        # sf_a == sf_b, n = 3: the terms are 1 : 3 a / (a + 2) : 3 a / (a + 2) : 1 with a = sf r: x_a = 1 takes the mirror term 2 with it
        _, a, _ = xref.shape(2.0, 2.0, 0.5)
        v = xref.nb_exact(0, 3, 2.0, 2.0, 1.0, 0.5)
        assert v["mirror"] and v["distance"] < 1e-90 and abs(v["p"] - 2 / (2 + 6 * a / (a + 2))) < mpmath.mpf("1e-90")
        assert abs(v["p_lower"] - v["p"] / 2) < mpmath.mpf("1e-90") and v["p_upper"] == v["p"]
        assert abs(xref.nb_exact(1, 2, 2.0, 2.0, 1.0, 0.5)["p"] - 1) < mpmath.mpf("1e-90")
    for c in GUARDS:
        v = xref.nb_exact(*c)
        assert v["p"] == 1 and v["p_lower"] == 1 and v["p_upper"] == 1 and not v["mirror"]


def test_reference_gives_no_value_at_its_term_cap():
    with pytest.raises(xref.TermCapExceeded):
        xref.nb_exact(5, 200_000, 3.0, 5.0, 1.0, 0.5)
    with pytest.raises(xref.TermCapExceeded):
        xref.nb_exact(5, 60, 3.0, 5.0, 1.0, 0.5, cap=50)


def test_the_grid_covers_what_it_should(table):
    rows = table["rows"]
    ks = set(xc.keys(rows))
    assert ks >= set(xc.REGIMES) and len(xc.REGIMES) == 14, set(xc.REGIMES) - ks
    ns = {r["x_a"] + r["x_b"] for r in rows}
    assert ns >= {1, 2, 10, 100, 2047, 2048, 2049, 4097, 6145} and max(ns) <= 100003
    wide = [r for r in rows if r["x_a"] + r["x_b"] >= xc.WIDE]
    assert 4 <= len(wide) <= 12 and all(r["x_a"] <= 900 for r in wide)
    assert {r["phi"] for r in rows} >= {0.005, 0.011, 0.13, 0.9, 2.3, 27.0}
    grid = [r for r in rows if not r["mirror"] and "pin" not in r["tag"]]
    ratio = [r["sf_b"] / r["sf_a"] for r in grid]
    sizes = [v for r in grid for v in (r["sf_a"], r["sf_b"])]
    assert min(ratio) <= 1e-3 and max(ratio) >= 1e3 and min(sizes) <= 0.3 and max(sizes) >= 2e6
    shapes = [v for r in rows for v in (r["sar"], r["sbr"])]
    assert min(shapes) < 1.0 and max(shapes) >= 4e8
    assert any(r["sar"] < 1 and r["sbr"] < 1 for r in rows)  # U-shaped
    # the mode at 0, at n and strictly inside, and x_a at the ends, at the mode and next to it, at the chunk ends
    big = [r for r in rows if r["x_a"] + r["x_b"] >= 2047]
    assert any(r["mode"] == 0 for r in big) and any(r["mode"] == r["x_a"] + r["x_b"] for r in big) and any(0 < r["mode"] < r["x_a"] + r["x_b"] for r in big)
    assert any(r["x_a"] == 0 for r in big) and any(r["x_b"] == 0 for r in big)
    for d in (-1, 0, 1):
        assert sum(r["x_a"] == r["mode"] + d for r in big) >= 10
    tags = " ".join(r["tag"] for r in rows)
    for t in ("chunk end 2047", "chunk end 2048", "anchor-2048", "anchor+2048"):
        assert t in tags, t
    # both tails, from about 0.5 down to 1e-8, 1e-40 and 1e-200
    p = np.array([float(r["p"]) for r in rows])
    lower = np.array([r["x_a"] < r["mode"] for r in rows])
    upper = np.array([r["x_a"] > r["mode"] for r in rows])
    for side in (lower, upper):
        for lo, hi in ((0.2, 1.0), (1e-12, 1e-7), (1e-50, 1e-38), (1e-215, 1e-190)):
            assert np.sum(side & (p >= lo) & (p <= hi)) >= 3, (lo, hi)
    assert p.min() >= 1e-300 and all(e["reason"] == "value below 1e-300" for e in table["left_out"])
    # the symmetric block: the three measured rows and their swaps
    sym = {_args(r) for r in rows if r["mirror"]}
    for c in ((30, 2000, 50.0, 50.0, 20.0, 0.5), (450, 440, 5e5, 5e5, 1e-3, 0.13), (120, 80, 7.0, 7.0, 10.0, 0.3)):
        assert c in sym and (c[1], c[0]) + c[2:] in sym
    assert all(r["sf_a"] == r["sf_b"] and r["x_a"] != r["x_b"] and r["distance"] < 1e-60 for r in rows if r["mirror"])
    assert sum("pin" in r["tag"] for r in rows) == 1 and 0 < sum(not r["in_ratio"] for r in rows) < len(rows) // 5
    assert 300 <= len(rows) <= 700 and table["summary"]["rows"] == len(rows)
    assert all(len({(rows[i]["sf_a"], rows[i]["sf_b"]) for i in idx}) == 1 for idx in xc.groups(rows))
    print("\nleft out of the table:", table["summary"]["left_out"], "; outside the Ratio partition:", table["summary"]["outside_ratio_partition"])


def test_tie_route_share_on_the_reference_alone(table):
    rows = table["rows"]
    ties = sum(xc.near_tie(r) for r in rows)
    print(f"\nrows within {xref.TIE_DISTANCE:g} of a tie (mirror rows apart): {ties} of {len(rows)}")
    assert ties <= xc.MAX_TIE_SHARE * len(rows) and ties == table["summary"]["near_ties"]


def test_difference_form_of_the_restatement_against_the_reference(table):
    """tests/sseq_ref.py's log_prob_all is the checker of the matrix-level device tests at rtol 1e-9: its ln Γ differences must carry that"""
    rows = [r for r in table["rows"] if not r["mirror"] and r["x_a"] + r["x_b"] <= 6145]
    err, _ = xc.errors(rows, [sseq_ref.nb_exact_test(*_args(r)) for r in rows])
    print(f"\nsseq_ref.nb_exact_test against the reference: {max(err):.2e} at most over {len(rows)} rows")
    assert max(err) <= 1e-10


# ---- the library ----------------------------------------------------------------------------------------------------------------------
def test_guards_return_exactly_one(sa):
    for c in GUARDS:
        assert sa.sseq.host_nb_exact_test(*c) == 1.0 and sa.host_nb_exact_test_ratio(*c) == 1.0


def test_host_logspace_against_the_reference(sa, table):
    rows = table["rows"]
    lib, tie_route = xc.errors(rows, [sa.sseq.host_nb_exact_test(*_args(r)) for r in rows])
    xc.report("host LogSpace", rows, lib, "logspace")
    print(f"  rows that matched the other side of a near tie: {tie_route} of {len(rows)}")
    bad = xc.failures(rows, lib, "logspace")
    assert not bad, (len(bad), sorted({b[0] for b in bad}), max(bad, key=lambda t: t[1] / t[2]))


def test_host_ratio_against_the_reference(sa, table):
    rows = table["rows"]
    lib, tie_route = xc.errors(rows, [sa.host_nb_exact_test_ratio(*_args(r)) for r in rows])
    xc.report("host Ratio", rows, lib, "ratio")
    print(f"  rows that matched the other side of a near tie: {tie_route} of {len(rows)}")
    bad = xc.failures(rows, lib, "ratio")
    assert not bad, (len(bad), sorted({b[0] for b in bad}), max(bad, key=lambda t: t[1] / t[2]))


def test_symmetric_rows_include_the_mirror_term(sa, table):
    """sf_a == sf_b: the term n - x_a equals the observed one in exact arithmetic and belongs to p; p(x_a, x_b) == p(x_b, x_a)"""
    rows = [r for r in table["rows"] if r["mirror"]]
    assert len(rows) >= 6
    for r in rows:  # the log-space terms k and n - k are the same two numbers added in either order: the same bits
        lp = np.asarray(sa.sseq.host_log_prob_all(r["x_a"] + r["x_b"], r["sf_a"], r["sf_b"], r["mu"], 1.0 / r["phi"]))
        assert lp.tobytes() == lp[::-1].tobytes(), _args(r)
    for name, f, backend in (("LogSpace", sa.sseq.host_nb_exact_test, "logspace"), ("Ratio", sa.host_nb_exact_test_ratio, "ratio")):
        bounds = xc.row_bounds(table["rows"], backend)
        for r, b in ((r, bounds[table["rows"].index(r)]) for r in rows):
            got = f(*_args(r))
            e, e_without = xc.rel_err(got, r["p"]), xc.rel_err(got, r["p_lower"])
            print(f"  {name:8s} {_args(r)}: p = {got!r}, {e:.2e} from the reference with the mirror, {e_without:.2e} from the one without")
            assert e <= b, (name, r, got)
            swapped = f(r["x_b"], r["x_a"], *_args(r)[2:])
            assert xc.rel_err(swapped, r["p"]) <= b, (name, r, swapped)


def test_host_log_terms_against_the_reference(sa, table):
    """ln T(k) - ln T(x_a) of scanrs_host_nb_log_prob_all against the reference's, every k: at most MARGIN x 2^-53 x log_span of the row. This
    names the faulty piece directly: an error of one ln Γ difference shows at its own k, whatever it does to p."""
    picked = list(LARGE_PARAMETER_ROWS)
    for key in xc.REGIMES[::2]:
        picked.append(next(_args(r) for r, k in zip(table["rows"], xc.keys(table["rows"])) if k == key and 100 <= r["x_a"] + r["x_b"] <= 2049))
    worst = 0.0
    for c in picked:
        x_a, x_b, sf_a, sf_b, mu, phi = c
        n = x_a + x_b
        lp = np.asarray(sa.sseq.host_log_prob_all(n, sf_a, sf_b, mu, 1.0 / phi))
        assert len(lp) == n + 1
        e = np.abs((lp - lp[x_a]) - xref.log_terms(x_a, n, sf_a, sf_b, phi))
        bound = xc.MARGIN * 2.0 ** -53 * xref.log_span(n, sf_a, sf_b, mu, phi)
        worst = max(worst, e.max() / bound)
        print(f"  {c}: {e.max():.2e} at k = {int(np.argmax(e))} (bound {bound:.2e})")
        assert e.max() <= bound, (c, int(np.argmax(e)), e.max(), bound)
    print(f"  worst: {worst:.2f} of its bound")
