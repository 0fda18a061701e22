"""nearest_neighbors under pearson / cosine distance without a device: the host twin against the plain-Python
restatement of umap-rs/src/dist.rs:73-124 and knn.rs:112-166 (tests/metric_knn_ref.py) bit for bit, the reference's own pins
(dist.rs:185-195), the threshold of the filtered route in exact rational arithmetic, and the public surface."""
import ctypes
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import metric_knn_cases as cases  # noqa: E402
import metric_knn_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("pearson", "cosine")
NEW_SYMBOLS = {
    "scanrs_nearest_neighbors": r"knn\.rs:112-166",
    "scanrs_nearest_neighbors_device": r"knn\.rs:112-166",
    "scanrs_host_nearest_neighbors": r"knn\.rs:112-166",
    "scanrs_host_distance": r"dist\.rs:19-34, 73-124",
    "scanrs_host_metric_rows": r"dist\.rs:73-76, 106-115",
}


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_FULL = {}


def full_reference(kind, n, d):
    """every other row of every query in (key, index) order, once per (kind, n, d): the answer for k is its first min(k, n - 1) columns"""
    if (kind, n, d) not in _FULL:
        x = cases.special_points(n, d)
        idx, dist = ref.nearest_neighbors(x.tolist(), n - 1, kind)
        _FULL[kind, n, d] = (x, np.array(idx, dtype=np.uint32).reshape(n, n - 1), np.array(dist, dtype=np.float64).reshape(n, n - 1))
    return _FULL[kind, n, d]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [1, 2, 3, 50, 128])
@pytest.mark.parametrize("n", [2, 3, 65, 257])
def test_the_host_twin_equals_the_reference_bit_for_bit(sa, kind, n, d):
    x, ridx, rdist = full_reference(kind, n, d)
    for k in (1, 15, n - 1, n + 3):
        k_eff = min(k, n - 1)
        idx, dist = sa.host_nearest_neighbors(x, k, kind)
        assert idx.shape == (n, k_eff) and dist.shape == (n, k_eff) and idx.dtype == np.uint32
        assert np.array_equal(idx, ridx[:, :k_eff]), (kind, n, d, k)
        assert np.array_equal(bits(dist), bits(rdist[:, :k_eff])), (kind, n, d, k)


@pytest.mark.parametrize("kind", KINDS)
def test_the_special_inputs_take_the_branches_they_are_meant_to(sa, kind):
    """the planted rows of special_points under the reference restatement itself (what the grid above then holds the twin to)"""
    x = cases.special_points(65, 50)
    D = lambda a, b: ref.value(kind, x[a].tolist(), x[b].tolist())  # noqa: E731
    assert D(4, 6) == 0.0 and D(4, 30) == 1.0  # all-zero rows: 0 among them, 1 against others
    if kind == "pearson":
        assert D(3, 5) == 0.0 and D(3, 4) == 0.0 and D(3, 30) == 1.0  # constant rows are degenerate too
    assert D(7, 8) == 1.0 and ref.fold_xy(ref.prepare(kind, x[7])[0], ref.prepare(kind, x[8])[0]) == 0.0  # the s_xy == 0 branch
    assert abs(D(9, 10) - 2.0) < 1e-12 and D(0, 1) < 1e-15 and D(0, 2) < 1e-15
    assert math.isinf(ref._mul(ref.prepare(kind, x[15])[1], ref.prepare(kind, x[17])[1]))  # s_xx * s_yy overflows
    assert D(15, 17) in (0.0, 1.0)  # inf / inf = NaN loses against 0 in f64::max, or s_xy / inf = 0
    s16, s18, s25 = (ref.prepare(kind, x[r])[1] for r in (16, 18, 25))
    assert s16 == 0.0 and s18 > 0.0 and s25 > 0.0 and ref._mul(s18, s25) == 0.0  # ... and underflows: division by zero
    assert D(18, 25) in (0.0, float("inf")) and D(16, 18) in (0.0, 1.0, float("inf"))
    for a, b in ((15, 17), (16, 18), (18, 25), (15, 16), (15, 18), (3, 4), (7, 8), (9, 10), (0, 1), (11, 12)):
        key, dist = sa.host_distance(kind, x[a], x[b])
        rk, rd = ref.distance(kind, x[a].tolist(), x[b].tolist())
        assert bits(key) == bits(rk) and bits(dist) == bits(rd), (kind, a, b)
        key2, dist2 = sa.host_distance(kind, x[b], x[a])
        assert bits(key2) == bits(key) and bits(dist2) == bits(dist), "D is bitwise symmetric"


def test_d1_under_pearson_is_all_degenerate_and_d2_is_plus_minus_one(sa):
    idx, dist = sa.host_nearest_neighbors(cases.special_points(65, 1), 15, "pearson")
    assert np.all(dist == 0.0)
    assert np.array_equal(idx, np.array([[p for p in range(65) if p != q][:15] for q in range(65)], dtype=np.uint32))  # order by index
    x = np.random.default_rng(5).standard_normal((40, 2))
    _, dist = sa.host_nearest_neighbors(x, 39, "pearson")
    assert np.all((dist < 1e-15) | (np.abs(dist - 2.0) < 1e-15))


def test_the_pins_of_the_reference(sa):
    """dist.rs:190-195 (exact) and dist.rs:177-186 (within 1e-7)"""
    for y, want in (([3.0, 4.0], 0.0), ([-4.0, 3.0], 1.0), ([-3.0, -4.0], 2.0), ([4.0, -3.0], 1.0)):
        assert ref.value("cosine", [3.0, 4.0], y) == want
        key, dist = sa.host_distance("cosine", [3.0, 4.0], y)
        assert key == math.sqrt(want) and dist == key * key
    assert abs(ref.value("pearson", [1.0, 3.0, 5.0], [2.0, 4.0, 6.0])) <= 1e-7
    assert abs(sa.host_distance("pearson", [1.0, 3.0, 5.0], [2.0, 4.0, 6.0])[1]) <= 1e-7


@pytest.mark.parametrize("kind", KINDS)
def test_the_prepared_rows_are_the_reference_folds(sa, kind):
    x = cases.special_points(65, 50)
    c, s, z = sa.host_metric_rows(kind, x)
    for r in range(65):
        rc, rs = ref.prepare(kind, x[r].tolist())
        assert np.array_equal(bits(c[r]), bits(rc)) and bits(s[r]) == bits(rs)
        if rs == 0.0:
            assert np.all(z[r] == 0.0)
        else:
            root = math.sqrt(rs)
            assert np.array_equal(bits(z[r]), bits([t / root for t in rc]))


def test_euclidean_is_the_search_of_knn_with_a_square_root(sa):
    """ordered by (the fma-chain squared distance of scanrs_knn, index); the distance is its square root"""
    import knn_sharded_ref as ks

    x = cases.special_points(65, 50)[19:60]  # near-ties, no extreme magnitudes
    idx, dist = sa.host_nearest_neighbors(x, 15, "euclidean")
    n = x.shape[0]
    for q in range(n):
        sq = np.zeros(n)
        for j in range(x.shape[1]):
            t = x[:, j] - x[q, j]
            sq = ks.fma(t, t, sq)
        order = sorted((float(sq[p]), p) for p in range(n) if p != q)[:15]
        assert [p for _, p in order] == idx[q].tolist()
        assert np.array_equal(bits(dist[q]), bits(np.sqrt(np.array([v for v, _ in order]))))
        assert bits(sa.host_distance("euclidean", x[q], x[order[0][1]])[0]) == bits(dist[q, 0])


def test_refusals_of_the_host_twin(sa):
    x = np.ones((5, 3))
    x[3, 1] = np.nan
    with pytest.raises(sa.ScanrsError, match="row 3") as e:
        sa.host_nearest_neighbors(x, 2, "cosine")
    assert e.value.code == 6
    x[3, 1] = np.inf
    with pytest.raises(sa.ScanrsError, match="row 3"):
        sa.host_nearest_neighbors(x, 2, "pearson")
    with pytest.raises(sa.ScanrsError):
        sa.host_nearest_neighbors(np.ones((4, 129)), 2, "cosine")
    with pytest.raises(sa.ScanrsError):
        sa.host_nearest_neighbors(np.ones((4, 3)), 2, 7)
    with pytest.raises(sa.ScanrsError):
        sa.host_nearest_neighbors(np.ones((4, 3)), 2, "manhattan")
    idx, dist = sa.host_nearest_neighbors(np.ones((1, 3)), 4, "cosine")
    assert idx.shape == (1, 0) and dist.shape == (1, 0)
    idx, dist = sa.host_nearest_neighbors(np.ones((4, 3)), 0, "cosine")
    assert idx.shape == (4, 0)


# ---- the threshold of the filtered route -------------------------------------------------------------------------------------------
def adversarial_sets(d):
    """rows inside the magnitude window without a degenerate one: near-ties around every neighbour rank, near-duplicates at relative
    1e-12 .. 1e-3, mirrored rows, a common offset, magnitudes from 1e-30 to 1e30"""
    rng = np.random.default_rng(900 + d)
    base = rng.standard_normal((6, d))
    rows = [b for b in base]
    for e in range(-12, -2):
        rows.append(base[0] * (1.0 + 10.0**e * rng.standard_normal(d)))  # near-duplicates
    for i in range(4):
        rows.append(base[1] + 1e-7 * rng.standard_normal(d))  # near-ties around base[1]
    rows += [-base[2], -base[0] * (1.0 + 1e-9 * rng.standard_normal(d))]  # mirrored
    rows += [base[3] + 1e6, base[4] + 1e6, base[3] * 1e30, base[4] * 1e-30, base[5] * 1e30, base[5] * 1e-30 * (1.0 + 1e-8 * rng.standard_normal(d))]
    x = np.array(rows)
    if d == 2:
        x = x[np.abs(x[:, 0] - x[:, 1]) > 0]  # (pearson: x_0 == x_1 is a constant row)
    return x


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [2, 50, 58])
def test_the_threshold_of_the_filtered_route_covers_every_neighbour(sa, kind, d):
    """For every pair with key <= key_k the EXACT squared distance of the standardised rows the filter reads stays under the
    threshold the kernel forms from key_k, less the allowance for the filter's own chain. tau grows with key_k, so the pair's own key is the
    tightest key_k it has to pass: checked for every pair. Also held to the bound DERIVED in knn_metric.hip (2 kk (1 + 69 u) + 500 u
    without the chain's 251 u), which is far inside the constants the library uses."""
    prm = sa.debug_nearest_neighbors_params()
    delta, e, chain = prm["delta"], prm["e"], prm["chain"]
    x = adversarial_sets(d)
    c, s, z = sa.host_metric_rows(kind, x)
    assert np.all(s >= prm["sxx_min"]) and np.all(s <= prm["sxx_max"]), "the sets must lie inside the window"
    n = x.shape[0]
    zf = [[Fraction(float(t)) for t in row] for row in z]
    u = Fraction(1, 2**53)
    worst = Fraction(0)
    for q in range(n):
        for p in range(q + 1, n):
            key, _ = sa.host_distance(kind, x[q], x[p])
            kk = key * key
            tau = 2.0 * kk * (1.0 + delta) + e  # Metric::threshold of knn_metric.hip, the same IEEE operations
            exact = sum((a - b) ** 2 for a, b in zip(zf[q], zf[p]))
            assert exact <= Fraction(tau) - Fraction(chain), (kind, d, q, p, float(exact), tau)
            assert exact <= 2 * Fraction(kk) * (1 + 69 * u) + 500 * u, (kind, d, q, p, float(exact - 2 * Fraction(kk)))
            worst = max(worst, exact - 2 * Fraction(kk))
    print(f"{kind} d={d}: largest |z_q - z_p|^2 - 2 key^2 = {float(worst):.3e} (E = {e:.3e})")


def test_the_interface_is_declared_mirrored_and_exported(sa):
    hdr = open(os.path.join(ROOT, "include", "scanrs_amd.h")).read()
    hpp = open(os.path.join(ROOT, "include", "scanrs_amd.hpp")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(sa.LIB_PATH)
    for name, cite in NEW_SYMBOLS.items():
        assert re.search(r"\bint %s\s*\(" % name, code), f"{name} is not declared in scanrs_amd.h"
        assert name in hpp, f"{name} is not mirrored in scanrs_amd.hpp"
        assert name in sa.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"%s \(%s" % (name, cite), hdr), f"{name} does not cite the reference"
    assert re.search(r"SCANRS_DIST_EUCLIDEAN = 0, SCANRS_DIST_PEARSON = 1, SCANRS_DIST_COSINE = 2", code)
    assert "enum class DistanceType" in hpp and "simd_euclidean" in hdr  # the stated deviation of the euclidean kind
    for fn in ("nearest_neighbors", "nearest_neighbors_device", "host_nearest_neighbors", "host_distance", "host_metric_rows"):
        assert callable(getattr(sa, fn)), fn
