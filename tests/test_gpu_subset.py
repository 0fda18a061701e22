"""sum_rows / sum_cols / sum_rows_dual / mean_rows / mean_var_rows / var_axis on the device (scan-rs_amd/csrc/subset.hip,
subset_host.cpp) against the numpy restatement tests/subset_ref.py. Integer results are compared exactly; f64 results at the
tolerances written next to each assert. Each case runs on a CSR handle, a CSC handle and a transposed view."""
import json
import os
import sys

import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import select_ref as sref  # noqa: E402
import subset_ref as ref  # noqa: E402

import scanrs_oracle as so  # noqa: E402

KINDS = ["csr", "csc", "t"]
BIG = 0xFFFFFFFF


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


def _handle(sa, m, kind):
    """A handle that reads as the scipy matrix m: stored CSR, stored CSC, or the transposed view of m.T stored CSR (flag CSC)."""
    if kind == "t":
        base = sref.canonical(m.T, "csr")
        h = sa.AdaptiveMat.from_csmat(base.shape[0], base.shape[1], sa.CSR, base.indptr, base.indices, base.data).t()
        assert h.storage() == sa.CSC
        return h
    c = sref.canonical(m, kind)
    return sa.AdaptiveMat.from_csmat(c.shape[0], c.shape[1], sa.CSR if kind == "csr" else sa.CSC, c.indptr, c.indices, c.data)


def assert_close(a, b, rtol, atol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    err = np.abs(a - b) - (np.abs(b) * rtol + atol)
    print(f"   max |a - b| {float(np.max(np.abs(a - b), initial=0.0)):.3e}, beyond the bound by {float(np.max(err, initial=-np.inf)):.3e}")
    assert np.all(np.abs(a - b) <= np.abs(b) * rtol + atol), float(np.max(np.abs(a - b)))


def _passes(h):
    return h.counter("subset_masked_passes"), h.counter("subset_scatter_passes")


# ---- 1. the reference's own cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_golden_table(sa, kind):
    """sqz/src/mat.rs:1302-1370: integers exact, floats at the reference's own epsilon."""
    with open(os.path.join(TESTS, "golden", "subset_reference_tables.json")) as f:
        g = json.load(f)
    h = _handle(sa, sparse.csr_matrix(np.array(g["input_a"], dtype=np.uint32)), kind)
    c1, c2, tol = g["cols"], g["cols2"], g["abs_tol"]
    for dt in (np.uint64, np.uint32):
        assert h.sum_cols(c1, dt).tolist() == g["sum_cols"] and h.sum_cols(c1, dt).dtype == dt
        assert h.sum_rows(c1, dt).tolist() == g["sum_rows"]
        s1, s2 = h.sum_rows_dual(c1, c2, dt)
        assert [s1.tolist(), s2.tolist()] == g["sum_rows_dual"]
    assert np.allclose(h.sum_cols(c1), g["sum_cols"], rtol=0, atol=tol) and np.allclose(h.sum_rows(c1), g["sum_rows"], rtol=0, atol=tol)
    s1, s2 = h.sum_rows_dual(c1, c2)
    assert np.allclose(s1, g["sum_rows_dual"][0], rtol=0, atol=tol) and np.allclose(s2, g["sum_rows_dual"][1], rtol=0, atol=tol)
    assert np.allclose(h.mean_rows(c1), g["mean_rows"], rtol=0, atol=tol)
    mean, var = h.mean_var_rows(c1)
    assert np.allclose(mean, g["mean_var_rows"]["mean"], rtol=0, atol=tol) and np.allclose(var, g["mean_var_rows"]["var"], rtol=0, atol=tol)
    assert np.array_equal(h.var_axis(0), h.mean_var_axis(0)[1]) and np.array_equal(h.var_axis(1), h.mean_var_axis(1)[1])


# ---- 2. shapes at which the walk can go wrong ---------------------------------------------------------------------------------------
ROW_NNZ = [0, 1, 63, 64, 65, 255, 256, 257, 8192, 8193, 20000, 16384]
BIG_ROW, WIDE_COLS = 10, 40000


@pytest.fixture(scope="module")
def wide():
    """12 rows x 40 000 columns whose rows hold exactly 0, 1, 63, 64, 65, 255, 256, 257, 8192, 8193, 20 000 and (the twelfth row)
    16 384 nonzeros: no entry, a tail shorter than a stride of 64, exactly SCAN_U = 4 strides, and vectors of one, two and three work
    items of 8192 (one of them ending exactly on the cut). Counts 1..9; the row of 20 000 also holds three counts of 2^32 - 1 at odd
    columns, so that the list of every second (even) column does not see them. Returns the scipy matrix, its dense uint64 array,
    and the same pair for the transpose (40 000 x 12: many short vectors, and 12 columns of which three are cut)."""
    rng = np.random.default_rng(41)
    dense = np.zeros((len(ROW_NNZ), WIDE_COLS), dtype=np.uint64)
    for r, n in enumerate(ROW_NNZ):
        at = np.sort(rng.choice(WIDE_COLS, n, replace=False))
        dense[r, at] = rng.integers(1, 10, size=n)
    odd = np.flatnonzero((dense[BIG_ROW] != 0) & (np.arange(WIDE_COLS) % 2 == 1))
    dense[BIG_ROW, odd[[3, len(odd) // 2, len(odd) - 2]]] = BIG
    assert [int((dense[r] != 0).sum()) for r in range(len(ROW_NNZ))] == ROW_NNZ
    m = sparse.csr_matrix(dense.astype(np.uint32))
    return (m, dense), (sparse.csr_matrix(m.T), np.ascontiguousarray(dense.T))


def _lists(rng, n):
    """empty; one index; the first; the last; every column; every second column; random ascending columns (5 000, or half the
    columns of a narrower matrix)"""
    k = min(5000, n // 2)
    return [np.zeros(0, dtype=np.int64), np.array([n // 3]), np.array([0]), np.array([n - 1]), np.arange(n), np.arange(0, n, 2),
            np.sort(rng.choice(n, k, replace=False))]


def _pairs(rng, n):
    """identical, disjoint and half-overlapping pairs for the dual form"""
    k = min(5000, n // 2)
    a = np.sort(rng.choice(n, k, replace=False))
    rest = np.setdiff1d(np.arange(n), a)
    b_disjoint = np.sort(rng.choice(rest, min(k, rest.size), replace=False))
    b_half = np.sort(np.concatenate([a[: k // 2], b_disjoint[: k - k // 2]]))
    return [(a, a.copy()), (a, b_disjoint), (a, b_half), (np.arange(n), np.arange(1, n, 2))]


@pytest.fixture(scope="module")
def wide_expected(wide):
    """The restatement's results for every list of test 2, computed once: [which matrix] -> (lists, pairs, sum_rows, sum_cols, dual)."""
    out = []
    for m, dense in wide:
        rng = np.random.default_rng(5)
        lists, pairs = _lists(rng, m.shape[1]), _pairs(rng, m.shape[1])
        out.append((lists, pairs, [ref.sum_rows(dense, c) for c in lists], [ref.sum_cols(dense, c) for c in lists],
                    [ref.sum_rows_dual(dense, a, b) for a, b in pairs]))
    return out


@pytest.mark.parametrize("which", [0, 1], ids=["12x40000", "40000x12"])
@pytest.mark.parametrize("kind", KINDS)
def test_walk_shapes_u64_both_routes(sa, wide, wide_expected, kind, which):
    """u64 results equal the restatement exactly with "subset_scatter" 1 and 0, and the counters show the route: the row copy is the
    stored one for "csr" only, so there sum_rows is a masked walk and sum_cols the scatter; for "csc" and the transposed view it is
    the other way round; with the option off nothing is scattered (the missing copy is built). dtype uint32: OverflowError where a
    sum exceeds 2^32 - 1, else the u64 numbers."""
    m, _dense = wide[which]
    lists, pairs, e_rows, e_cols, e_dual = wide_expected[which]
    overflowed = narrowed = 0
    for scatter in (1, 0):
        h = _handle(sa, m, kind)  # fresh: only the stored copy exists
        if scatter == 0:
            h.set_option("subset_scatter", 0)
        assert _passes(h) == (0, 0)

        def ran(rows_result, before):
            scattered = scatter == 1 and ((kind == "csr") != rows_result)
            after = _passes(h)
            assert after == (before[0] + (0 if scattered else 1), before[1] + (1 if scattered else 0)), (after, before, scattered)

        for c, er, ec in zip(lists, e_rows, e_cols):
            before = _passes(h)
            got = h.sum_rows(c, np.uint64)
            assert got.dtype == np.uint64 and np.array_equal(got, er)
            ran(True, before)
            before = _passes(h)
            assert np.array_equal(h.sum_cols(c, np.uint64), ec)
            ran(False, before)
            for fn, e in ((h.sum_rows, er), (h.sum_cols, ec)):
                if e.size and int(e.max()) > BIG:
                    overflowed += 1
                    with pytest.raises(OverflowError):
                        fn(c, np.uint32)
                else:
                    narrowed += 1
                    got = fn(c, np.uint32)
                    assert got.dtype == np.uint32 and np.array_equal(got, e)
        for (a, b), (ea, eb) in zip(pairs, e_dual):
            before = _passes(h)
            ga, gb = h.sum_rows_dual(a, b, np.uint64)
            assert np.array_equal(ga, ea) and np.array_equal(gb, eb)
            ran(True, before)
        if scatter == 0:
            assert h.counter("subset_scatter_passes") == 0
    assert overflowed > 0 and narrowed > overflowed  # both sides of the uint32 rule were seen


@pytest.mark.parametrize("kind", KINDS)
def test_walk_shapes_f64(sa, wide, wide_expected, kind):
    """The f64 forms over the same vectors (the raw counts through the identity map): the cut vectors' partial sums meet in the slab.
    Sums of integers below 2^53 are exact in any order, so they equal the integer results; the variances (squares of 2^32 - 1 are
    not exact) at rtol 1e-10."""
    m, dense = wide[0]
    lists, pairs, e_rows, e_cols, e_dual = wide_expected[0]
    h = _handle(sa, m, kind)
    for c, er, ec in zip(lists, e_rows, e_cols):
        assert np.array_equal(h.sum_rows(c), er.astype(np.float64)) and np.array_equal(h.sum_cols(c), ec.astype(np.float64))
    for (a, b), (ea, eb) in zip(pairs, e_dual):
        ga, gb = h.sum_rows_dual(a, b)
        assert np.array_equal(ga, ea.astype(np.float64)) and np.array_equal(gb, eb.astype(np.float64))
    c = lists[6]
    mean, var = h.mean_var_rows(c)
    em, ev = ref.mean_var_rows(dense, c)
    assert_close(mean, em, rtol=1e-12, atol=1e-13)
    assert_close(var, ev, rtol=1e-10, atol=1e-12)
    assert _passes(h)[1] == 0  # f64 never scatters


# ---- 3. mapped values ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mapped_case():
    """3 000 x 700 at 5 %, counts 1..8 with a few large ones, and the two maps as dense arrays of the oracle's values."""
    rng = np.random.default_rng(17)
    m = sparse.random(3000, 700, density=0.05, format="csr", random_state=np.random.RandomState(17))
    m.data = rng.integers(1, 9, size=m.data.shape[0]).astype(np.uint32)
    m.data[rng.random(m.data.shape[0]) < 0.002] = 40000
    m = sref.canonical(m)
    f_rows, f_cols = rng.random(3000) * 2.0 + 0.25, rng.random(700) * 3.0 + 0.1
    o = so.AdaptiveMat.from_scipy(sparse.csr_matrix(m))
    dense_norm = so.normalize(o, "cellranger").inner_sparse().to_dense()
    dense_chain = (o.compose_map(so.MapOp(so.OP_SCALE_AXIS, axis=0, a=f_rows)).compose_map(so.MapOp(so.OP_SCALE_AXIS, axis=1, a=f_cols))
                   .apply(so.OP_LN_1P).to_dense())
    lists = [np.sort(rng.choice(700, 200, replace=False)), np.arange(700), np.arange(3, 700, 7), np.array([699])]
    pair = (lists[0], np.sort(np.concatenate([lists[0][:100], np.setdiff1d(np.arange(700), lists[0])[:150]])))
    expected = {}
    for name, d in (("normalize", dense_norm), ("chain", dense_chain)):
        expected[name] = {"sum_rows": [ref.sum_rows(d, c) for c in lists], "sum_cols": [ref.sum_cols(d, c) for c in lists],
                          "dual": ref.sum_rows_dual(d, *pair), "mean_rows": [ref.mean_rows(d, c) for c in lists],
                          "mean_var_rows": [ref.mean_var_rows(d, c) for c in lists]}
    return m, f_rows, f_cols, lists, pair, expected


def _mapped_handle(sa, m, kind, which, f_rows, f_cols):
    h = _handle(sa, m, kind)
    if which == "normalize":
        return sa.normalize(h, sa.Normalization.CellRanger)
    return h.compose_scale_axis(0, f_rows).compose_scale_axis(1, f_cols).apply(sa.FN_LN_1P)


def _all_f64(h, lists, pair):
    out = []
    for c in lists:
        out += [h.sum_rows(c), h.sum_cols(c), h.mean_rows(c), *h.mean_var_rows(c)]
    out += [*h.sum_rows_dual(*pair), h.var_axis(0), h.var_axis(1)]
    return out


@pytest.mark.parametrize("which", ["normalize", "chain"])
@pytest.mark.parametrize("kind", KINDS)
def test_mapped_values(sa, mapped_case, kind, which):
    """Means and sums at rtol 1e-12 / atol 1e-13, variances at rtol 1e-10 / atol 1e-12 (the tolerances of
    test_axis_moments_from_the_summed_over_copy for the same quantities and logarithm) against the correctly rounded restatement;
    mean_var_rows(all columns) meets mean_var_axis(1); var_axis is mean_var_axis's variance bit for bit; every f64 result is the same
    array when repeated, after a dot and an rdot on the handle, and on a fresh handle."""
    m, f_rows, f_cols, lists, pair, expected = mapped_case
    e = expected[which]
    h = _mapped_handle(sa, m, kind, which, f_rows, f_cols)
    for i, c in enumerate(lists):
        assert_close(h.sum_rows(c), e["sum_rows"][i], rtol=1e-12, atol=1e-13)
        assert_close(h.sum_cols(c), e["sum_cols"][i], rtol=1e-12, atol=1e-13)
        assert_close(h.mean_rows(c), e["mean_rows"][i], rtol=1e-12, atol=1e-13)
        mean, var = h.mean_var_rows(c)
        assert_close(mean, e["mean_var_rows"][i][0], rtol=1e-12, atol=1e-13)
        assert_close(var, e["mean_var_rows"][i][1], rtol=1e-10, atol=1e-12)
    s1, s2 = h.sum_rows_dual(*pair)
    assert_close(s1, e["dual"][0], rtol=1e-12, atol=1e-13)
    assert_close(s2, e["dual"][1], rtol=1e-12, atol=1e-13)
    mean, var = h.mean_var_rows(lists[1])
    am, av = h.mean_var_axis(1)
    assert_close(mean, am, rtol=1e-12, atol=1e-13)
    assert_close(var, av, rtol=1e-10, atol=1e-12)
    for axis in (0, 1):
        assert np.array_equal(h.var_axis(axis), h.mean_var_axis(axis)[1])
    with pytest.raises(sa.ScanrsError) as ei:  # integer results are defined on the raw counts
        h.sum_rows(lists[0], np.uint64)
    assert ei.value.code == 6 and "raw" in str(ei.value)
    first = _all_f64(h, lists, pair)
    for a, b in zip(first, _all_f64(h, lists, pair)):
        assert np.array_equal(a, b)
    rng = np.random.default_rng(2)
    h.dot(rng.random((700, 3)))
    h.rdot(rng.random((2, 3000)))
    for a, b in zip(first, _all_f64(h, lists, pair)):
        assert np.array_equal(a, b)
    for a, b in zip(first, _all_f64(_mapped_handle(sa, m, kind, which, f_rows, f_cols), lists, pair)):
        assert np.array_equal(a, b)


# ---- 4. a medium matrix -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def medium():
    """20 000 cells x 2 000 genes at 3 % (about 1.2 M nonzeros), genes x cells, with two overlapping and two disjoint cell lists."""
    m = sref.synth_genes_by_cells(20000, 2000, 0.03, 3)
    rng = np.random.default_rng(9)
    a = np.sort(rng.choice(20000, 6000, replace=False))
    b = np.sort(rng.choice(20000, 7000, replace=False))
    assert np.intersect1d(a, b).size > 0
    d = np.sort(rng.choice(np.setdiff1d(np.arange(20000), a), 5000, replace=False))
    dense = m.toarray().astype(np.uint64)
    return m, (a, b, d), {k: ref.sum_rows(dense, v) for k, v in (("a", a), ("b", b), ("d", d))}


@pytest.mark.parametrize("kind", KINDS)
def test_medium_dual_equals_two_single_calls_and_group_sums(sa, medium, kind):
    m, (a, b, d), e = medium
    h = _handle(sa, m, kind)
    s1, s2 = h.sum_rows_dual(a, b, np.uint64)
    assert np.array_equal(s1, e["a"]) and np.array_equal(s2, e["b"])
    assert np.array_equal(s1, h.sum_rows(a, np.uint64)) and np.array_equal(s2, h.sum_rows(b, np.uint64))
    s1, s2 = h.sum_rows_dual(a, d, np.uint64)  # disjoint: also what group_sums gives with the lists as labels
    assert np.array_equal(s1, e["a"]) and np.array_equal(s2, e["d"])
    labels = np.full(m.shape[1], -1, dtype=np.int16)
    labels[a], labels[d] = 0, 1
    sums = sa.group_sums(h, labels, 2)
    sums = sums[0] if isinstance(sums, tuple) else sums
    assert np.array_equal(np.asarray(sums)[:, 0], s1) and np.array_equal(np.asarray(sums)[:, 1], s2)


# ---- 5. interface behaviour ---------------------------------------------------------------------------------------------------------
def _small():
    rng = np.random.default_rng(0)
    m = sparse.random(300, 170, density=0.08, format="csr", random_state=np.random.RandomState(0))
    m.data = rng.integers(1, 9, size=m.data.shape[0]).astype(np.uint32)
    return sref.canonical(m)


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_leave_the_handle_usable(sa, kind):
    m = _small()
    dense = m.toarray().astype(np.uint64)
    h = _handle(sa, m, kind)
    good = np.arange(5, 160, 3)

    def refused(fn, word):
        with pytest.raises(sa.ScanrsError) as ei:
            fn()
        assert ei.value.code == 6 and word in str(ei.value), str(ei.value)
        assert not isinstance(ei.value, sa.CancellationError)
        assert np.array_equal(h.sum_rows(good, np.uint64), ref.sum_rows(dense, good))  # the handle still works

    for fn in (h.sum_rows, h.sum_cols, h.mean_rows, h.mean_var_rows):
        refused(lambda: fn([5, 4, 9]), "cols")     # descending
        refused(lambda: fn([4, 4, 9]), "cols")     # a duplicate
        refused(lambda: fn([4, 170]), "cols")      # out of range
    refused(lambda: h.sum_rows_dual(good, [9, 3], np.uint64), "cols2")
    refused(lambda: h.sum_rows_dual([3, 3], good), "cols1")
    refused(lambda: h.sum_rows([-1]), "out of range")
    n = sa.normalize(_handle(sa, m, kind), sa.Normalization.CellRanger)
    for fn in (lambda: n.sum_rows(good, np.uint64), lambda: n.sum_cols(good, np.uint32), lambda: n.sum_rows_dual(good, good, np.uint64)):
        refused(fn, "raw")
    assert n.sum_rows(good).shape == (300,)
    s = _handle(sa, m, "csr")
    s.set_shard(0, 2, 0, 2 * m.shape[0], allreduce=lambda ptr, count, dtype: 0)
    for fn in (lambda: s.sum_rows(good, np.uint64), lambda: s.sum_cols(good), lambda: s.sum_rows_dual(good, good), lambda: s.mean_rows(good),
               lambda: s.mean_var_rows(good)):
        refused(fn, "sharded")
    with pytest.raises(sa.ScanrsError):
        h.sum_rows(good, np.int32)


@pytest.mark.parametrize("kind", KINDS)
def test_empty_lists(sa, kind):
    h = _handle(sa, _small(), kind)
    for dt in (np.uint64, np.uint32, np.float64):
        assert h.sum_rows([], dt).tolist() == [0] * 300 and h.sum_rows([], dt).dtype == dt
        assert h.sum_cols([], dt).shape == (0,)
        s1, s2 = h.sum_rows_dual([], [], dt)
        assert not s1.any() and not s2.any() and s1.shape == (300,)
    s1, s2 = h.sum_rows_dual([], [1, 2], np.uint64)
    assert not s1.any() and np.array_equal(s2, ref.sum_rows(_small().toarray().astype(np.uint64), [1, 2]))
    assert np.isnan(h.mean_rows([])).all()
    mean, var = h.mean_var_rows([])
    assert np.isnan(mean).all() and np.isnan(var).all()


@pytest.mark.parametrize("kind", KINDS)
def test_snoop_of_the_dual_form(sa, kind):
    m = _small()
    dense = m.toarray().astype(np.uint64)
    a, b = np.arange(0, 170, 2), np.arange(50, 120)
    for dt in (np.uint64, np.float64):
        h = _handle(sa, m, kind)
        sn = sa.AtomicSnoop()
        sn.cancel()
        with pytest.raises(sa.CancellationError):
            h.sum_rows_dual(a, b, dt, snoop=sn)
        s1, s2 = h.sum_rows_dual(a, b, dt)  # the same call without cancellation then succeeds
        assert np.array_equal(s1, ref.sum_rows(dense, a).astype(dt)) and np.array_equal(s2, ref.sum_rows(dense, b).astype(dt))
        sn = sa.AtomicSnoop()
        g1, g2 = h.sum_rows_dual(a, b, dt, snoop=sn)
        assert np.array_equal(g1, s1) and np.array_equal(g2, s2)
        assert sn.history[0] == 0.0 and sn.history[-1] == 1.0 and all(x <= y for x, y in zip(sn.history, sn.history[1:]))
