"""select_rows / select_cols / partition_on_thresholds / to_csmat on the device (scan-rs_amd/csrc/select.hip, select_host.cpp)
against the numpy / scipy restatement tests/select_ref.py. Counts are integers: every comparison is exact equality. Each case runs
on a CSR handle, a CSC handle and a transposed view."""
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

KINDS = ["csr", "csc", "t"]


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


def _assert_same(sa, h, expected, kind, dense=False):
    """The handle's shape, storage flag and to_csmat arrays against the scipy matrix (exact)."""
    assert h.shape() == list(expected.shape)
    flag = sa.CSR if kind == "csr" else sa.CSC
    assert h.storage() == flag
    ip, ix, vv = h.to_csmat()
    eip, eix, evv = sref.triplet(expected, "csr" if flag == sa.CSR else "csc")
    assert ip.dtype == np.uint64 and ix.dtype == np.uint32 and vv.dtype == np.uint32
    assert np.array_equal(ip, eip) and np.array_equal(ix, eix) and np.array_equal(vv, evv)
    assert h.nnz() == expected.nnz
    if dense and expected.shape[0] * expected.shape[1]:
        assert np.array_equal(h.to_dense(), np.asarray(expected.todense(), dtype=np.float64))


def _small(seed=0, rows=300, cols=170):
    rng = np.random.default_rng(seed)
    m = sparse.random(rows, cols, density=0.08, format="csr", random_state=np.random.RandomState(seed))
    m.data = rng.integers(1, 9, size=m.data.shape[0]).astype(np.uint32)
    return sref.canonical(m)


@pytest.fixture(scope="module")
def big():
    """100 000 cells x 33 000 genes at 3 % (seed 3), genes x cells."""
    return sref.synth_genes_by_cells(100000, 33000, 0.03, 3)


# ---- select ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_select_small(sa, kind):
    m = _small()
    dense = m.toarray()
    h = _handle(sa, m, kind)
    rng = np.random.default_rng(1)
    for axis, n in ((0, m.shape[0]), (1, m.shape[1])):
        lists = [rng.integers(0, n, 100), np.sort(rng.choice(n, 60, replace=False)), rng.permutation(n), np.array([n - 1]), np.arange(n)]
        for idx in lists:
            got = h.select_rows(idx) if axis == 0 else h.select_cols(idx)
            want = sref.select_rows(dense, idx) if axis == 0 else sref.select_cols(dense, idx)
            assert np.array_equal(got.to_dense(), want.astype(np.float64))
            _assert_same(sa, got, sparse.csr_matrix(want), kind)


@pytest.mark.parametrize("kind", KINDS)
def test_select_empty_list_gives_an_empty_dimension(sa, kind):
    """scanrs_mat_create accepts an empty dimension (checked here too); an empty index list gives such a matrix."""
    e = sa.AdaptiveMat.from_csmat(0, 170, sa.CSR, np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32))
    assert e.shape() == [0, 170] and e.nnz() == 0
    m = _small()
    h = _handle(sa, m, kind)
    r = h.select_rows(np.zeros(0, dtype=np.int64))
    assert r.shape() == [0, m.shape[1]] and r.nnz() == 0
    c = h.select_cols([])
    assert c.shape() == [m.shape[0], 0] and c.nnz() == 0
    ip, ix, vv = c.to_csmat()
    assert not ip.any() and ix.size == 0 and vv.size == 0


@pytest.mark.parametrize("kind", KINDS)
def test_select_large_matches_scipy_slices(sa, big, kind):
    h = _handle(sa, big, kind)
    rng = np.random.default_rng(2)
    genes, cells = big.shape
    for idx in (rng.integers(0, genes, 2000), np.sort(rng.choice(genes, 2000, replace=False))):
        _assert_same(sa, h.select_rows(idx), sref.select_rows(big, idx), kind)
    for idx in (np.arange(0, cells, 2), rng.integers(0, cells, 5000)):
        _assert_same(sa, h.select_cols(idx), sref.select_cols(big, idx), kind)


# ---- partition ------------------------------------------------------------------------------------------------------------------
def _check_partition(sa, m, kind, row_t, col_t, expect_rounds=None, min_rounds=None, dense=False):
    h = _handle(sa, m, kind)
    f, r, sel_r, sel_c = h.partition_on_thresholds(row_t, col_t)
    ef, er, esr, esc, rounds = sref.partition_on_thresholds(m, row_t, col_t)
    print(f"partition {m.shape} {kind}: rounds {h.counter('partition_rounds')} (restatement {rounds}), "
          f"{m.shape[0] - len(sel_r)} rows / {m.shape[1] - len(sel_c)} columns excluded")
    assert np.array_equal(sel_r, esr) and np.array_equal(sel_c, esc)
    assert h.counter("partition_rounds") == rounds
    if expect_rounds is not None:
        assert rounds == expect_rounds
    if min_rounds is not None:
        assert h.counter("partition_rounds") >= min_rounds
    _assert_same(sa, f, ef, kind, dense)
    _assert_same(sa, r, er, kind, dense)
    return h, f, r, sel_r, sel_c


def _quantile_thresholds(m):
    return sref.quantile_threshold(m.sum(axis=1)), sref.quantile_threshold(m.sum(axis=0))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ["3000x800", "3000x800_heavy", "20000x5000", "20000x5000_heavy"])
def test_partition_quantile_thresholds(sa, kind, case):
    heavy = dict(gene_shape=0.1, shared_profile=0.5) if case.endswith("heavy") else {}
    if case.startswith("3000"):
        m = sref.synth_genes_by_cells(3000, 800, 0.05, 3, **heavy)
        expect = 3 if heavy else 5
    else:
        m = sref.synth_genes_by_cells(20000, 5000, 0.03, 3, **heavy)
        expect = 4 if heavy else 8
    rt, ct = _quantile_thresholds(m)
    _check_partition(sa, m, kind, rt, ct, expect_rounds=expect, min_rounds=3, dense=case.startswith("3000"))


@pytest.mark.parametrize("kind", KINDS)
def test_partition_large(sa, big, kind):
    rt, ct = _quantile_thresholds(big)
    _, _, _, sel_r, sel_c = _check_partition(sa, big, kind, rt, ct, expect_rounds=7, min_rounds=3)
    assert big.shape[0] - len(sel_r) == 5049 and big.shape[1] - len(sel_c) == 16251


@pytest.mark.parametrize("kind", KINDS)
def test_partition_one_sided_none_and_everything(sa, kind):
    m = sref.synth_genes_by_cells(3000, 800, 0.05, 3)
    rt, ct = _quantile_thresholds(m)
    _check_partition(sa, m, kind, rt, None, dense=True)
    _check_partition(sa, m, kind, None, ct, dense=True)
    _check_partition(sa, m, kind, float("nan"), float("nan"), expect_rounds=1, dense=True)
    h, f, r, sel_r, sel_c = _check_partition(sa, m, kind, None, None, expect_rounds=1, dense=True)
    assert f.shape() == list(m.shape) and r.shape() == [m.shape[0], 0] and r.nnz() == 0
    # a threshold above every sum: everything is excluded, the matrices have empty dimensions
    top = float(m.sum()) + 1.0
    h, f, r, sel_r, sel_c = _check_partition(sa, m, kind, top, top)
    assert len(sel_r) == 0 and len(sel_c) == 0 and f.shape() == [0, 0] and r.shape() == [0, m.shape[1]] and f.nnz() == 0 and r.nnz() == 0
    # only one of the matrices asked for
    f, r, sel_r2, sel_c2 = h.partition_on_thresholds(rt, ct, residual=False)
    assert r is None
    _assert_same(sa, f, sref.partition_on_thresholds(m, rt, ct)[0], kind)
    f, r, _, _ = h.partition_on_thresholds(rt, ct, filtered=False)
    assert f is None
    _assert_same(sa, r, sref.partition_on_thresholds(m, rt, ct)[1], kind)


@pytest.mark.parametrize("kind", KINDS)
def test_partition_on_threshold_three(sa, kind):
    m = sref.synth_genes_by_cells(3000, 800, 0.05, 3, gene_shape=0.1, shared_profile=0.5)
    h = _handle(sa, m, kind)
    f, r, sel_r, sel_c = h.partition_on_threshold(3.0)
    ef, er, esr, esc, rounds = sref.partition_on_threshold(m, 3.0)
    assert rounds == 2 and m.shape[0] - len(esr) == 1
    assert h.counter("partition_rounds") == 2
    assert np.array_equal(sel_r, esr) and np.array_equal(sel_c, esc)
    _assert_same(sa, f, ef, kind, dense=True)
    _assert_same(sa, r, er, kind, dense=True)


@pytest.mark.parametrize("kind", KINDS)
def test_partition_hand_made_cascade(sa, kind):
    a, gone_r, gone_c, rounds = sref.cascade_matrix()
    m = sparse.csr_matrix(a.astype(np.uint32))
    h, f, r, sel_r, sel_c = _check_partition(sa, m, kind, 10.0, 10.0, expect_rounds=rounds, min_rounds=5, dense=True)
    assert np.array_equal(np.setdiff1d(np.arange(a.shape[0]), sel_r), gone_r)
    assert np.array_equal(np.setdiff1d(np.arange(a.shape[1]), sel_c), gone_c)
    fd, rd, _, _, _ = sref.partition_dense(a, 10, 10)
    assert np.array_equal(f.to_dense(), fd) and np.array_equal(r.to_dense(), rd)


# ---- the reference's chain: partition_on_threshold(3.0) -> normalize -> run_pca ---------------------------------------------------
def _sign_fix(a, ref):
    return a * np.sign(np.sum(a * ref, axis=0))


def test_partition_normalize_pca_chain_matches_oracle(sa):
    """normalization.rs:376-379: the tolerances are those of tests/test_gpu_parity.py::test_bksvd_matches_oracle."""
    import scanrs_oracle as so

    m = sref.synth_genes_by_cells(3000, 800, 0.05, 3, gene_shape=0.1, shared_profile=0.5)  # genes x cells
    k = 10
    h = _handle(sa, m, "csc")
    f, _, sel_r, sel_c = h.partition_on_threshold(3.0)
    ef = sref.partition_on_threshold(m, 3.0)[0]
    assert ef.shape != m.shape
    c = sref.canonical(ef, "csc")
    o = so.AdaptiveMat(c.shape[0], c.shape[1], so.CSC, c.indptr.astype(np.uint64), c.indices.astype(np.uint32), c.data.astype(np.uint32))
    omega = so.omega_panel((2 * k, c.shape[0]), 0)
    u, s, v = sa.BkSvd().run_pca(sa.normalize(f, sa.Normalization.CellRanger), k, omega=omega)
    uo, s_o, vo = so.BkSvd().run_pca(so.normalize(o, "cellranger"), k, omega=omega)
    assert u.shape == uo.shape and v.shape == vo.shape
    assert np.max(np.abs(s - s_o) / s_o) < 1e-8
    assert np.max(np.abs(_sign_fix(u, uo) - uo)) < 1e-6
    assert np.max(np.abs(_sign_fix(v, vo) - vo)) < 1e-6


# ---- lifetime, repeatability, refusals, memory ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_results_outlive_the_source_and_repeat_bitwise(sa, kind):
    m = sref.synth_genes_by_cells(3000, 800, 0.05, 3)
    rt, ct = _quantile_thresholds(m)
    rng = np.random.default_rng(4)
    idx = rng.integers(0, m.shape[1], 700)
    h = _handle(sa, m, kind)
    first = (h.select_cols(idx), h.select_rows(idx[:100] % m.shape[0])) + h.partition_on_thresholds(rt, ct)[:2]
    second = (h.select_cols(idx), h.select_rows(idx[:100] % m.shape[0])) + h.partition_on_thresholds(rt, ct)[:2]
    del h  # the source is freed first
    want = (sref.select_cols(m, idx), sref.select_rows(m, idx[:100] % m.shape[0])) + sref.partition_on_thresholds(m, rt, ct)[:2]
    for a, b, w in zip(first, second, want):
        ta, tb = a.to_csmat(), b.to_csmat()
        assert all(np.array_equal(x, y) for x, y in zip(ta, tb))
        _assert_same(sa, a, w, kind)
        assert a.sum_axis(1, dtype=np.uint32).tolist() == np.asarray(w.sum(axis=1)).ravel().tolist()  # the result is a working handle


def test_refusals_name_their_cause(sa):
    m = _small()
    idx = np.arange(10)

    def refused(fn, code, *words):
        with pytest.raises(sa.ScanrsError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        assert all(w in str(e.value) for w in words), str(e.value)

    h = _handle(sa, m, "csr")
    h.compose_scale_axis(0, np.ones(m.shape[0]))
    for fn in (lambda: h.select_rows(idx), lambda: h.select_cols(idx), lambda: h.partition_on_threshold(3.0)):
        refused(fn, 6, "map", "identity")
    h.reset_map()
    assert h.select_rows(idx).shape() == [10, m.shape[1]]
    h.center(0)
    for fn in (lambda: h.select_rows(idx), lambda: h.select_cols(idx), lambda: h.partition_on_threshold(3.0)):
        refused(fn, 6, "offset")
    h.reset_map()
    assert h.select_cols(idx).shape() == [m.shape[0], 10]
    s = _handle(sa, m, "csr")
    s.set_shard(0, 2, 0, 2 * m.shape[0], allreduce=lambda ptr, count, dtype: 0)
    for fn in (lambda: s.select_rows(idx), lambda: s.select_cols(idx), lambda: s.partition_on_threshold(3.0)):
        refused(fn, 6, "sharded")
    g = _handle(sa, m, "csc")
    refused(lambda: g.select_rows([0, m.shape[0]]), 6, "out of range")
    refused(lambda: g.select_cols([m.shape[1] + 5]), 6, "out of range")
    refused(lambda: g.t().select_rows([m.shape[1]]), 6, "out of range")
    refused(lambda: g.select_rows([-1]), 6, "out of range")


def test_device_memory_returns_to_its_start(sa):
    import gc

    m = sref.synth_genes_by_cells(3000, 800, 0.05, 3)
    rt, ct = _quantile_thresholds(m)
    gc.collect()
    sa.release_cached_memory()
    start = sa.device_memory_in_use()
    for kind in KINDS:
        h = _handle(sa, m, kind)
        a = h.select_rows(np.arange(0, m.shape[0], 3))
        b = h.select_cols(np.random.default_rng(0).integers(0, m.shape[1], 500))
        f, r, _, _ = h.partition_on_thresholds(rt, ct)
        assert sa.device_memory_in_use() > start
        del h, a, b, f, r
    gc.collect()
    sa.release_cached_memory()
    assert sa.device_memory_in_use() == start
