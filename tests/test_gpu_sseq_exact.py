"""The exact branch of the sSeq test on the device (sseq_exact_*_kernel of scan-rs_amd/csrc/sseq.hip, sseq_ratio_*_kernel of sseq_ratio.inc)
against the high-precision values of tests/golden/sseq_exact_table.json, for both backends. The cases, regimes and bounds are those of
tests/test_sseq_exact_cpu.py (tests/sseq_exact_cases.py); every table group is one sseq_de_from_sums call with big_count = 2^62.

Measured on an MI355X: the device's worst relative error per regime is the host's for LogSpace (2.1e-11 at most against a bound of 1.0e-10 in
>=1e6/hi, where the library's earlier form reached 2.5e-6; 583 of 615 rows bit-equal to the host, 32847 ulp at most, at p = 3.3e-201, where one
ulp of ln p is 512 ulp of p) and within a few per cent of the serial host loop's for Ratio (1.5e-11 at most, in <15/lo/body, the U-shaped
distributions over 6145 terms; 211 of 615 rows bit-equal; 112950 ulp at most, at p = 5.3e-297 on a row that the device hands to LogSpace and the
host's serial sweep does not). The per-regime table is in tests/test_sseq_exact_cpu.py. No row took the tie route. The seven tests take 1.2 s
together.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import sseq_exact_cases as xc  # noqa: E402

ARGS = ("x_a", "x_b", "sf_a", "sf_b", "mu", "phi")
EXACT = 2 ** 62  # big_count: no sum is above it, so every test takes the exact branch


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


def _params(sa, rows):
    mu, phi = np.array([r["mu"] for r in rows]), np.array([r["phi"] for r in rows])
    return sa.SSeqParams(0, len(rows), np.zeros(0), mu, np.ones(len(rows)), np.zeros(len(rows), dtype=bool), phi, 0.0, 0.0, phi)


def _call(sa, rows, backend, swap=False):
    """p-values of rows that share one (sf_a, sf_b), one gene per row, in ONE call; swap: the two sides exchanged"""
    assert len({(r["sf_a"], r["sf_b"]) for r in rows}) == 1
    a, b = [r["x_a"] for r in rows], [r["x_b"] for r in rows]
    fa, fb = rows[0]["sf_a"], rows[0]["sf_b"]
    if swap:
        a, b, fa, fb = b, a, fb, fa
    return sa.sseq_de_from_sums(a, b, fa, fb, _params(sa, rows), big_count=EXACT, backend=backend).p_values


def _battery(sa, rows, backend):
    p = np.zeros(len(rows))
    for idx in xc.groups(rows):
        p[idx] = _call(sa, [rows[i] for i in idx], backend)
    return p


def _ulps(a, b):
    """distance of positive doubles in units of the last place"""
    return np.abs(np.asarray(a, dtype=np.float64).view(np.int64) - np.asarray(b, dtype=np.float64).view(np.int64))


@pytest.fixture(scope="module")
def dev(sa):
    rows = xc.load_table()["rows"]
    return rows, {"logspace": _battery(sa, rows, sa.NB_EXACT_LOGSPACE), "ratio": _battery(sa, rows, sa.NB_EXACT_RATIO)}


@pytest.mark.parametrize("backend", ["logspace", "ratio"])
def test_exact_battery_matches_the_reference(dev, backend):
    rows, p = dev
    err, tie_route = xc.errors(rows, p[backend])
    xc.report(f"device {backend}", rows, err, backend)
    print(f"  rows that matched the other side of a near tie: {tie_route} of {len(rows)}")
    assert tie_route <= xc.MAX_TIE_SHARE * len(rows)
    bad = xc.failures(rows, err, backend)
    assert not bad, (len(bad), sorted({b[0] for b in bad}), max(bad, key=lambda t: t[1] / t[2]))


@pytest.mark.parametrize("backend", ["logspace", "ratio"])
def test_exact_battery_device_against_host(sa, dev, backend):
    """Host and device run one source with their own log, log1p and exp, and the Ratio host form is the serial sweep where the device multiplies
    in a tree: each is within its row's bound of the reference, so the two are within twice that of each other. The ulp figure is printed."""
    rows, p = dev
    f = sa.sseq.host_nb_exact_test if backend == "logspace" else sa.host_nb_exact_test_ratio
    host = np.array([f(*(r[k] for k in ARGS)) for r in rows])
    d = _ulps(p[backend], host)
    i = int(np.argmax(d))
    print(f"\n{backend}, host against device: {int(d[i])} ulp at most (p = {p[backend][i]!r}, {rows[i]['tag']}), {int(np.sum(d == 0))} of {len(rows)} rows bit-equal")
    rel = np.abs(p[backend] - host) / host
    bound = 2.0 * np.array(xc.row_bounds(rows, backend))
    near = np.array([xc.near_tie(r) for r in rows])
    bad = np.flatnonzero(~(rel <= bound) & ~near)
    assert bad.size == 0, (rows[bad[0]], p[backend][bad[0]], host[bad[0]])


def test_exact_result_does_not_depend_on_the_batch(sa, dev):
    rows, p = dev
    for backend, name in ((sa.NB_EXACT_LOGSPACE, "logspace"), (sa.NB_EXACT_RATIO, "ratio")):
        assert _battery(sa, rows, backend).tobytes() == p[name].tobytes()
        four_chunks = next(i for i, r in enumerate(rows) if r["x_a"] + r["x_b"] == 6145 and 2048 < r["x_a"] < 4096)
        inner = next(i for i, r in enumerate(rows) if r["x_a"] + r["x_b"] == 2049 and 0 < r["x_a"] < 2049)
        small = next(i for i, r in enumerate(rows) if r["x_a"] + r["x_b"] == 10)
        outside = next(i for i, r in enumerate(rows) if not r["in_ratio"])
        for i in (four_chunks, inner, small, outside):
            assert _call(sa, [rows[i]], backend)[0] == p[name][i], (name, rows[i])
        # a group in reverse order: other neighbours, other chunk offsets
        idx = xc.groups(rows)[0][::-1]
        assert _call(sa, [rows[i] for i in idx], backend).tobytes() == p[name][idx].tobytes()


def test_symmetric_rows_include_the_mirror_term(sa, dev):
    """sf_a == sf_b: the term n - x_a equals the observed one in exact arithmetic. Both backends count it (special::nb_term adds the two sides'
    numbers, which the mirror term adds in the other order; the Ratio kernels take it by its index), so p(x_a, x_b) and p(x_b, x_a) are both
    the reference's p with the mirror, within the regime's bound. The reference code's own `<=` on rounded terms drops it in these rows
    (tests/test_sseq_exact_cpu.py has the figures)."""
    rows, p = dev
    sym = [i for i, r in enumerate(rows) if r["mirror"]]
    assert len(sym) >= 6
    for backend, name in ((sa.NB_EXACT_LOGSPACE, "logspace"), (sa.NB_EXACT_RATIO, "ratio")):
        bounds = xc.row_bounds(rows, name)
        for i in sym:
            r = rows[i]
            swapped = _call(sa, [r], backend, swap=True)[0]
            for got in (p[name][i], swapped):
                e = xc.rel_err(got, r["p"])
                assert e <= bounds[i], (name, r, got, e, xc.rel_err(got, r["p_lower"]))


def test_rows_outside_the_ratio_partition_carry_the_logspace_bits(dev):
    """an observed term below 2^-970 of the anchor's: the Ratio backend hands the test to the LogSpace kernels (include/scanrs_amd.h)"""
    rows, p = dev
    out = np.array([not r["in_ratio"] for r in rows])
    assert out.sum() >= 20
    assert p["ratio"][out].tobytes() == p["logspace"][out].tobytes()
    assert (p["ratio"][~out] != p["logspace"][~out]).mean() > 0.5  # and the others are Ratio's own
