"""The asymptotic (beta) branch of the sSeq test on the host: `special::betainc`, `special::betaincinv` and `special::nb_asymptotic`
(scan-rs_amd/csrc/special.hpp, the source the device kernel compiles too) against the high-precision reference tests/sseq_asym_ref.py.

The cases and their reference values are tests/golden/sseq_asym_table.json (written by tests/golden/make_sseq_asym_table.py; a sample
of its rows is recomputed here). scipy's double-precision values are stored beside them as the yardstick of what double precision
achieves; the bound of every regime is 4 x scipy's worst relative error against the reference in that regime, never below 1e-13
(tests/sseq_asym_cases.py). A regime is the branch of log_beta_pf that serves (a, b) (small: both < 15, stirling: both >= 15, mixed),
the size of a + b (S < 1e4 <= M < 1e6 <= L) and whether the value lies in the body (>= 1e-20) or the tail (down to 1e-300).

Measured, worst relative error per regime (library before this battery existed / library now / scipy 1.15.3):

  betainc (985 cases)            before     now        scipy     |  nb_asymptotic (295 cases)  before     now        scipy
  small/body                     1.9e-14    2.0e-14    2.9e-15   |                             8.2e-15    8.2e-15    5.0e-16
  small/tail                     5.5e-14    5.5e-14    2.4e-15   |
  mixed-S/body                   6.4e-13    2.5e-14    9.9e-15   |                             3.2e-14    2.3e-14    4.6e-15
  mixed-S/tail                   4.1e-13    1.3e-13    7.3e-14   |                             5.5e-14    5.5e-14    3.6e-14
  mixed-M/body                   4.8e-11    3.4e-14    9.3e-15   |                             3.6e-13    2.2e-14    3.1e-15
  mixed-M/tail                   1.0e-11    7.5e-14    1.8e-13   |                             2.7e-13    4.7e-14    5.3e-14
  mixed-L/body                   5.5e-10    5.4e-14    1.4e-14   |
  mixed-L/tail                   3.1e-10    8.9e-14    1.4e-13   |
  stirling-S/body                7.4e-13    9.1e-15    1.2e-13   |                             2.7e-13    5.5e-15    5.5e-14
  stirling-S/tail                1 (*)      1.5e-13    2.7e-13   |                             7.5e-13    1.9e-13    1.9e-13
  stirling-M/body                9.6e-11    9.7e-15    1.5e-11   |                             2.8e-11    8.0e-15    3.7e-12
  stirling-M/tail                1.6e-10    2.9e-13    1.5e-11   |                             2.1e-11    1.0e-13    1.6e-12
  stirling-L/body                1.1e-09    1.1e-14    9.3e-10   |                             1.9e-09    1.5e-14    9.3e-10
  stirling-L/tail                1 (*)      2.3e-13    1.6e-11   |                             2.8e-09    1.5e-13    9.1e-10

  betaincinv(a, b, 1/2), forward error |I - 1/2| / (1/2) at the returned x (91 cases)
                                 before     now        scipy       (the floor is the spacing of doubles at x times the density)
  small                          7.9e-15    3.5e-15    9.4e-16
  mixed-S / -M / -L              2.3e-12 / 1.3e-09 / 1.4e-08    6.8e-14 / 4.1e-11 / 7.4e-10    6.8e-14 / 4.1e-11 / 7.4e-10
  stirling-S / -M / -L           5.7e-13 / 5.3e-11 / 1.2e-09    1.6e-14 / 1.1e-12 / 4.1e-11    1.6e-14 / 1.2e-12 / 4.1e-11

  (*) the value came back 0: for a in [15, ~19] and I < ~1e-250, x/x0 - 1 rounded to -1 and its log1p to -inf.
  In the stirling-M and -L regimes scipy itself is off by up to 9.3e-10 (at a = b = 1e7; the reference there was confirmed by
  quadrature of the density), so the bound the yardstick gives is loose there; the table above is what the library reaches.

What was wrong before: ln of the prefactor took (a+b) ulp from the rounded 1 - x and a + b; the classical continued fraction lost what
its cancelling partial denominators cost times its value (up to ~a for b << a); betaincinv treated a Newton step that rounds to nothing
as a step out of the bracket and halved its way back, ending up to 13 ulp off; and the (*) above.

Largest betacf iteration count over the 1666 points at which the batteries run it: 1240 (cap 200000; at alpha = 8.0e6, beta = 9.7e6).
Cases within 1e-12 of the median (either side's value is accepted for them): 5 of 295 on the reference alone; the library took the
other side in none of them. Left out of the table: 6 betainc points whose series needs more than 1e8 terms (a or b = 1e7 or 5.5 against
the other at 0.5 or 5.5, next to the switch or at the q = 0.001 / 0.999 point on the slow side), 10 points whose x underflows or
rounds to 1 in double (all q = 1e-250), and 1 nb case below 1e-300. A planted error of 1e-11 in log_beta_pf fails three tests here.
"""
import os
import sys

import mpmath
import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import sseq_asym_ref as aref  # noqa: E402
from sseq_asym_cases import load_table, median_forward_error, nb_errors, nb_keys, regime_of, rel_err, report  # noqa: E402


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


@pytest.fixture(scope="module")
def table():
    return load_table()


# ---- the table itself ------------------------------------------------------------------------------------------------------------------
def test_table_rows_are_what_the_helper_computes(table):
    rows = [r for r in table["betainc"] if r["terms"] < 20000][::25]
    assert len(rows) >= 20
    for r in rows:
        with mpmath.workprec(aref.PREC):
            v = aref.betainc(r["a"], r["b"], r["x"])
            assert abs(v - mpmath.mpf(r["ref"])) <= mpmath.mpf("1e-27") * v, r
    nb = [r for r in table["nb"] if max(r["alpha"], r["beta"]) < 5e4][::12]
    assert len(nb) >= 8
    for r in nb:
        with mpmath.workprec(aref.PREC):
            v = aref.nb_asymptotic(r["x_a"], r["x_b"], r["sf_a"], r["sf_b"], r["mu"], r["phi"])
            assert (v["alpha"], v["beta"]) == (r["alpha"], r["beta"])
            for k in ("p", "p_lower", "p_upper"):
                assert abs(v[k] - mpmath.mpf(r[k])) <= mpmath.mpf("1e-27") * v[k], (k, r)
            assert abs(float(v["distance"]) - r["distance"]) <= 1e-9 * r["distance"] + 1e-18


def test_series_agrees_with_closed_forms():
    """I_x(a, b) where it is elementary: I_x(1, b) = 1 - (1-x)^b, I_x(a, 1) = x^a, I_{1/2}(a, a) = 1/2, on either side of the switch"""
    with mpmath.workprec(aref.PREC):
        for b, x in ((7.5, 0.01), (7.5, 0.9), (3000.25, 1e-4), (3000.25, 0.01)):
            e = 1 - (1 - mpmath.mpf(x)) ** mpmath.mpf(b)
            assert abs(aref.betainc(1.0, b, x) - e) < mpmath.mpf("1e-45") * e
            e = mpmath.mpf(1 - x) ** mpmath.mpf(b)  # I_{1-x}(b, 1), 1 - x a double of its own
            assert abs(aref.betainc(b, 1.0, 1 - x) - e) < mpmath.mpf("1e-45") * e
        for a in (0.5, 40.0, 1e5):
            assert abs(aref.betainc(a, a, 0.5) - mpmath.mpf(1) / 2) < mpmath.mpf("1e-45")
            assert abs(aref.beta_median(a, a) - mpmath.mpf(1) / 2) < mpmath.mpf("1e-30")


def test_series_gives_no_value_at_its_term_cap():
    with pytest.raises(aref.TermCapExceeded):
        aref.betainc(1e7, 0.5, 0.99999)
    with pytest.raises(aref.TermCapExceeded):
        aref.betainc(3000.0, 4000.0, 0.42, cap=50)


def test_the_grid_covers_what_it_should(table):
    bi, nb = table["betainc"], table["nb"]
    ab = {(r["a"], r["b"]) for r in bi}
    assert min(a for a, _ in ab) == 0.5 and max(a for a, _ in ab) == 1e7 and min(b for _, b in ab) == 0.5 and max(b for _, b in ab) == 1e7
    for edge in (14.999, 15.0, 15.001):
        assert {aref.regime(a, b)[:5] for a, b in ab if a == edge} >= {"small" if edge < 15 else "stirl", "mixed"}
        assert {aref.regime(a, b)[:5] for a, b in ab if b == edge} >= {"small" if edge < 15 else "stirl", "mixed"}
    tags = {r["tag"] for r in bi}
    assert tags >= {f"q={q:g}" for q in (1e-250, 1e-100, 1e-30, 1e-10, 1e-3, 0.3, 0.5, 0.7, 0.999)} | {"switch-", "switch+"}
    assert any(m["a"] < 1 for m in table["median"]) and any(m["b"] < 1 for m in table["median"])
    al = [r["alpha"] for r in nb]
    ratio = [r["beta"] / r["alpha"] for r in nb]
    assert min(al) < 1.0 and max(al) > 9e6 and min(ratio) < 1.01e-3 and max(ratio) > 0.99e3
    assert all(0.5 <= v <= 1e7 for r in nb for v in (r["alpha"], r["beta"]))
    assert all(0.5 <= v <= 1e7 for r in bi for v in (r["a"], r["b"]))
    assert min(float(r["p"]) for r in nb) < 1e-150 and sum(float(r["p_lower"]) < 1e-30 for r in nb) > 10 and sum(float(r["p_upper"]) < 1e-30 for r in nb) > 10
    assert sum(r["tag"].startswith("median") for r in nb) > 40
    assert max(r["x_a"] + r["x_b"] for r in nb) == 2 ** 40 - 5 and all(r["x_a"] >= 1 and r["x_b"] >= 1 for r in nb)
    assert 200 <= len(nb) <= 400
    print("\nleft out of the table:", table["summary"]["left_out"])


def test_tie_route_share_on_the_reference_alone(table):
    nb = table["nb"]
    ties = sum(r["distance"] < aref.TIE_DISTANCE for r in nb)
    print(f"\ncases within {aref.TIE_DISTANCE:g} of the median: {ties} of {len(nb)}")
    assert 0 < ties <= 0.02 * len(nb)


# ---- the library ----------------------------------------------------------------------------------------------------------------------
def test_host_betainc_against_the_series(sa, table):
    rows = table["betainc"]
    keys = [regime_of(r["a"], r["b"], r["ref"]) for r in rows]
    lib = [rel_err(sa.sseq.host_betainc(r["a"], r["b"], r["x"]), r["ref"]) for r in rows]
    yard = [rel_err(r["scipy"], r["ref"]) for r in rows]
    worst, bound = report("betainc", keys, lib, yard)
    assert len(worst) == 14
    bad = [(k, e, r) for k, e, r in zip(keys, lib, rows) if not e <= bound[k]]
    assert not bad, (len(bad), max(bad, key=lambda t: t[1]))


def test_host_betaincinv_forward_error(sa, table):
    rows = table["median"]
    keys = [aref.regime(m["a"], m["b"]) for m in rows]
    got = [sa.sseq.host_betaincinv(m["a"], m["b"], 0.5) for m in rows]
    lib = [median_forward_error(m, x) for m, x in zip(rows, got)]
    yard = [m["scipy_forward"] for m in rows]
    # the linearised forward error is the series' own wherever the series is cheap
    cheap = [i for i, m in enumerate(rows) if max(m["a"], m["b"]) <= 1e5][::6]
    assert len(cheap) >= 8
    for i in cheap:
        with mpmath.workprec(aref.PREC):
            direct = float(2 * abs(aref.betainc(rows[i]["a"], rows[i]["b"], got[i]) - mpmath.mpf(1) / 2))
        assert abs(direct - lib[i]) <= 1e-6 * lib[i] + 1e-25, (rows[i], direct, lib[i])
    worst, bound = report("betaincinv(a, b, 1/2), forward error", keys, lib, yard)
    assert len(worst) == 7
    bad = [(k, e, m) for k, e, m in zip(keys, lib, rows) if not e <= bound[k]]
    assert not bad, (len(bad), max(bad, key=lambda t: t[1]))


def test_host_nb_asymptotic_against_the_series(sa, table):
    rows = table["nb"]
    keys = nb_keys(rows)
    lib, tie_route = nb_errors(rows, [sa.sseq.host_nb_asymptotic_test(r["x_a"], r["x_b"], r["sf_a"], r["sf_b"], r["mu"], r["phi"]) for r in rows])
    yard, _ = nb_errors(rows, [r["scipy"] for r in rows])
    worst, bound = report("nb_asymptotic", keys, lib, yard)
    print(f"  cases that matched the other side of the median: {tie_route} of {len(rows)}")
    assert tie_route <= 0.02 * len(rows)
    bad = [(k, e, r) for k, e, r in zip(keys, lib, rows) if not e <= bound[k]]
    assert not bad, (len(bad), max(bad, key=lambda t: t[1]))


def battery_cf_points(table):
    """every (a, b, x) at which the batteries make special.hpp's betainc run its continued fraction"""
    pts = [(r["a"], r["b"], r["x"]) for r in table["betainc"]]
    pts += [(m["a"], m["b"], float(m["ref"])) for m in table["median"]]
    for r in table["nb"]:
        n = float(r["x_a"]) + float(r["x_b"])
        pts.append((r["alpha"], r["beta"], (r["x_a"] + 0.5) / n))
        pts.append((r["beta"], r["alpha"], (r["x_b"] + 0.5) / n))
    return np.array(pts).T


def test_betacf_stays_far_below_its_iteration_cap(table):
    a, b, x = battery_cf_points(table)
    it = aref.betainc_cf_iterations(a, b, x)
    i = int(np.argmax(it))
    print(f"\nlargest betacf iteration count over {len(it)} points: {it[i]} at a={a[i]!r} b={b[i]!r} x={x[i]!r}")
    assert 0 < it[i] < aref.BETACF_CAP // 10
    # the restatement is the library's fraction: I_x(a, b) = x^a y^b / B(a, b) / f
    pts = [(2.5, 4.0, 0.2), (700.25, 15.0, 0.9), (3.0e4, 5.0e4, 0.37), (1.0e5, 15.0, 0.9998)]
    f, n = aref.betacf_iterations(*zip(*pts))
    for (pa, pb, px), fi in zip(pts, f):
        with mpmath.workprec(aref.PREC):
            e = mpmath.exp(aref._log_prefactor(pa, pb, mpmath.mpf(px))) / aref.betainc(pa, pb, px)
            assert abs(fi - e) < 1e-14 * e, (pa, pb, px, fi, e)
