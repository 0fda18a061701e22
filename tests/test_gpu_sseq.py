"""sSeq differential expression on the device (scan-rs_amd/csrc/sseq.hip) against the CPU restatement tests/sseq_ref.py, and its
asymptotic branch (sseq_asymptotic_kernel) against the high-precision values of tests/golden/sseq_asym_table.json (section 9; the
cases, regimes and bounds are those of tests/test_sseq_asym_cpu.py).

Measured on an MI355X: the device's worst relative error against the reference is of the host's size in every regime (the table in
tests/test_sseq_asym_cpu.py; 6.7e-14 against 4.7e-14 in mixed-M/tail is the largest difference), 1.9e-13 at most (stirling-S/tail);
host against device 768 ulp at most. The six tests of section 9 take 0.4 s together."""
import os
import sys

import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import sseq_asym_cases as acases  # noqa: E402
import sseq_ref as ref  # noqa: E402

FIELDS = ("sums_in", "sums_out", "p_values", "adjusted_p_values", "log2_fold_change", "normalized_mean_in", "normalized_mean_out")


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd
    import scanrs_amd.hdf5_io  # noqa: F401

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


def _golden(name):
    return os.path.join(TESTS, "golden", name)


def _random_counts(genes, cells, density, seed):
    rng = np.random.default_rng(seed)
    m = sparse.random(genes, cells, density=density, format="csr", random_state=seed, data_rvs=lambda n: rng.geometric(0.3, n))
    return m.astype(np.uint32)


def _handle(sa, m, storage):
    """genes x cells scipy matrix -> handle in the given storage (CSR: gene-major, CSC: cell-major)."""
    g, c = m.shape
    s = sparse.csr_matrix(m) if storage == sa.CSR else sparse.csc_matrix(m)
    s.sort_indices()
    return sa.AdaptiveMat.from_csmat(g, c, storage, s.indptr.astype(np.uint64), s.indices.astype(np.uint32), s.data.astype(np.uint32))


def _tiny(sa):
    h = sa.hdf5_io.read_csc_matrix(_golden("tiny_10x.h5"))
    m = sparse.csc_matrix((h.values, h.indices, h.indptr.astype(np.int64)), shape=(h.rows, h.cols))
    return m


def _ref_group_sums(m, labels, n_groups):
    out = np.zeros((m.shape[0], n_groups), dtype=np.uint64)
    for j in range(n_groups):
        sel = np.flatnonzero(labels == j)
        if sel.size:
            out[:, j] = np.asarray(sparse.csc_matrix(m)[:, sel].sum(axis=1), dtype=np.uint64).ravel()
    return out


def _assert_params(got, exp, cells):
    np.testing.assert_array_equal(got.use_genes, exp["use_genes"])
    for f in ("size_factors", "gene_means", "gene_variances", "gene_moment_phi", "gene_phi"):
        # phi_mm is a difference (m var - mean sum_sf): where it cancels to ~0 only an absolute bound at the field's scale means anything
        np.testing.assert_allclose(getattr(got, f), exp[f], rtol=1e-12, atol=1e-12 * np.max(np.abs(exp[f])), err_msg=f)
    np.testing.assert_allclose([got.zeta_hat, got.delta], [exp["zeta_hat"], exp["delta"]], rtol=1e-12)
    assert len(got.size_factors) == cells


def _assert_de(got, exp, prtol=1e-9):
    for f in FIELDS:
        g, e = getattr(got, f), exp[f]
        if f.startswith("sums"):
            np.testing.assert_array_equal(g, e, err_msg=f)
        else:
            np.testing.assert_allclose(g, e, rtol=prtol if "p_values" in f else 1e-12, atol=0, err_msg=f)


# ---- 1. group sums ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_groups", [1, 7, 1024])
def test_group_sums_are_exact_in_every_orientation(sa, n_groups):
    m = _random_counts(300, 2500, 0.05, 11)
    rng = np.random.default_rng(n_groups)
    labels = rng.integers(-1, n_groups, m.shape[1]).astype(np.int16)
    if n_groups > 2:
        labels[labels == 2] = 3  # group 2 stays empty
    exp = _ref_group_sums(m, labels, n_groups)
    cnt = np.bincount(labels[labels >= 0], minlength=n_groups)
    outs = []
    for storage in (sa.CSR, sa.CSC):
        h = _handle(sa, m, storage)
        s, c = sa.group_sums(h, labels, n_groups)
        np.testing.assert_array_equal(s, exp)
        np.testing.assert_array_equal(c, cnt)
        s2, _ = sa.group_sums(h, labels, n_groups)
        assert s2.tobytes() == s.tobytes()
        outs.append(s)
    # a cells x genes handle used through .t()
    ht = _handle(sa, m.T.tocsr(), sa.CSR).t()
    np.testing.assert_array_equal(sa.group_sums(ht, labels, n_groups)[0], exp)


def test_group_sums_refuse_labels_out_of_range(sa):
    m = _random_counts(20, 50, 0.2, 1)
    h = _handle(sa, m, sa.CSR)
    with pytest.raises(sa.ScanrsError):
        sa.group_sums(h, np.full(50, 3, dtype=np.int16), 3)


# ---- 2. parameters ------------------------------------------------------------------------------------------------------------
def test_params_on_tiny_10x(sa):
    m = _tiny(sa)
    for storage in (sa.CSR, sa.CSC):
        got = sa.compute_sseq_params(_handle(sa, m, storage))
        _assert_params(got, ref.compute_sseq_params(m), m.shape[1])


@pytest.mark.parametrize("with_cells,with_umi", [(False, False), (True, False), (False, True), (True, True)])
def test_params_synthetic(sa, with_cells, with_umi):
    m = _random_counts(500, 2000, 0.04, 5)
    rng = np.random.default_rng(9)
    cells = np.sort(rng.choice(2000, 1300, replace=False)) if with_cells else None
    n_sel = 2000 if cells is None else len(cells)
    umi = rng.uniform(50, 400, n_sel) if with_umi else None
    exp = ref.compute_sseq_params(m, 0.995, cells, umi)
    res = []
    for storage in (sa.CSR, sa.CSC):
        got = sa.compute_sseq_params(_handle(sa, m, storage), 0.995, cells, umi)
        _assert_params(got, exp, 2000)
        res.append(got)
    # both copies give the same bits (exact integer / fixed-point sums)
    assert res[0].gene_means.tobytes() == res[1].gene_means.tobytes()
    assert res[0].gene_variances.tobytes() == res[1].gene_variances.tobytes()


# ---- 3. one-vs-rest on the analysis file's clusterings --------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["_graphclust", "_kmeans_2_clusters"])
def test_one_vs_rest_on_tiny_analysis(sa, key):
    m = _tiny(sa)
    nc, clusters = sa.hdf5_io.get_clustering(_golden("tiny_analysis.h5"), key)
    labels = sa.labels_from_clustering(clusters)
    params = sa.compute_sseq_params(_handle(sa, m, sa.CSC))
    pref = ref.compute_sseq_params(m)
    got = sa.sseq_de_one_vs_rest(_handle(sa, m, sa.CSR), labels, params, n_groups=nc)
    exp = ref.one_vs_rest(m, labels, pref, n_groups=nc)
    assert len(got) == nc
    for g, e in zip(got, exp):
        _assert_de(g, e)
    table = sa.diff_exp_table(got)
    stored = sa.hdf5_io.get_differential_expression(_golden("tiny_analysis.h5"), key)
    assert table.shape == stored.shape


# ---- 4. pairwise, both branches, matrix path == sums path ------------------------------------------------------------------------
def test_pairwise_both_branches_and_from_sums(sa):
    m = _random_counts(400, 3000, 0.08, 21)
    m = m.multiply(40).astype(np.uint32).tocsr()  # large enough sums for the asymptotic branch
    a = np.arange(0, 1400)
    b = np.arange(1400, 3000)
    params = sa.compute_sseq_params(_handle(sa, m, sa.CSR))
    pref = ref.compute_sseq_params(m)
    sa_, sb_ = (np.asarray(m[:, s].sum(axis=1)).ravel() for s in (a, b))
    tested = np.flatnonzero(pref["use_genes"])
    big = int(np.median(np.minimum(sa_[tested], sb_[tested])))
    got = sa.sseq_differential_expression(_handle(sa, m, sa.CSC), a, b, params, big_count=big)
    exp = ref.differential_expression(m, a, b, pref, big_count=big)
    asym = pref["use_genes"] & (sa_ > big) & (sb_ > big)
    assert asym.sum() > 20 and (~asym).sum() > 20
    _assert_de(got, exp)
    fa, fb = sum(params.size_factors[i] for i in a), sum(params.size_factors[i] for i in b)
    fs = sa.sseq_de_from_sums(got.sums_in, got.sums_out, fa, fb, params, big_count=big)
    for f in FIELDS:
        assert getattr(fs, f).tobytes() == getattr(got, f).tobytes(), f


def test_pairwise_refuses_bad_index_lists(sa):
    m = _random_counts(30, 60, 0.2, 2)
    h = _handle(sa, m, sa.CSR)
    params = sa.compute_sseq_params(h)
    for a, b in (([3, 1], [5]), ([1, 1], [5]), ([1, 2], [2, 5])):
        with pytest.raises(sa.ScanrsError):
            sa.sseq_differential_expression(h, a, b, params)


# ---- 5. exact test battery ----------------------------------------------------------------------------------------------------------
def test_exact_battery_matches_direct_gammaln(sa):
    cases = [(6, 3, 885.7432862994995, 2023.055530268548, 0.0029272959469517066, 27.024221110009037)]
    rng = np.random.default_rng(17)
    for n in (1, 2, 10, 100, 2047, 2048, 2049, 10000, 100000, 1000000):
        for _ in range(3):
            xa = int(rng.integers(0, n + 1))
            fa, fb = rng.uniform(0.2, 3000, 2)
            cases.append((xa, n - xa, fa, fb, rng.uniform(0.01, 4), rng.uniform(0.005, 2)))
    for xa, xb, fa, fb, mu, phi in cases:
        params = sa.SSeqParams(0, 1, np.zeros(0), np.array([mu]), np.array([1.0]), np.array([False]), np.array([phi]), 0.0, 0.0, np.array([phi]))
        g = sa.sseq_de_from_sums([xa], [xb], fa, fb, params, big_count=2**62).p_values[0]
        e = ref.nb_exact_test(xa, xb, fa, fb, mu, phi)
        if abs(g - e) > 1e-9 * e:
            lo, hi = ref.nb_exact_test_tie_bounds(xa, xb, fa, fb, mu, phi)
            assert lo * (1 - 1e-9) <= g <= hi * (1 + 1e-9), (xa, xb, fa, fb, mu, phi, g, e)
    pin = cases[0]
    params = sa.SSeqParams(0, 1, np.zeros(0), np.array([pin[4]]), np.array([1.0]), np.array([False]), np.array([pin[5]]), 0.0, 0.0, np.array([pin[5]]))
    assert abs(sa.sseq_de_from_sums([6], [3], pin[2], pin[3], params).p_values[0] - 0.03254) <= 1e-5


def test_exact_result_does_not_depend_on_the_other_tests(sa):
    rng = np.random.default_rng(4)
    genes = 64
    xa, xb = rng.integers(0, 5000, genes), rng.integers(0, 50000, genes)
    mu, phi = rng.uniform(0.1, 3, genes), rng.uniform(0.05, 1, genes)
    params = sa.SSeqParams(0, genes, np.zeros(0), mu, np.ones(genes), np.zeros(genes, dtype=bool), phi, 0.0, 0.0, phi)
    allp = sa.sseq_de_from_sums(xa, xb, 300.0, 2000.0, params, big_count=2**62).p_values
    for g in (0, 17, 63):
        one = sa.SSeqParams(0, 1, np.zeros(0), mu[g:g + 1], np.ones(1), np.zeros(1, dtype=bool), phi[g:g + 1], 0.0, 0.0, phi[g:g + 1])
        assert sa.sseq_de_from_sums(xa[g:g + 1], xb[g:g + 1], 300.0, 2000.0, one, big_count=2**62).p_values[0] == allp[g]


# ---- 6. degenerate cases ------------------------------------------------------------------------------------------------------------
def test_degenerate_cases(sa):
    m = _random_counts(50, 200, 0.1, 8).tolil()
    m[7, :] = 0  # an all-zero gene
    m = m.tocsr().astype(np.uint32)
    m.eliminate_zeros()
    h = _handle(sa, m, sa.CSR)
    params = sa.compute_sseq_params(h)
    pref = ref.compute_sseq_params(m)
    assert not params.use_genes[7] and params.gene_phi[7] == 0.0
    labels = np.zeros(200, dtype=np.int16)
    labels[100:] = 1
    labels[:5] = 3  # group 2 is empty
    got = sa.sseq_de_one_vs_rest(h, labels, params, n_groups=4)
    exp = ref.one_vs_rest(m, labels, pref, n_groups=4)
    for g, e in zip(got, exp):
        _assert_de(g, e)
    assert (got[2].p_values == 1.0).all() and (got[2].normalized_mean_in == 0).all()
    assert got[0].p_values[7] == 1.0
    # a zero size factor on one side
    one = sa.SSeqParams(0, 1, np.zeros(0), np.array([1.0]), np.array([1.0]), np.array([True]), np.array([0.5]), 0.0, 0.0, np.array([0.5]))
    assert sa.sseq_de_from_sums([3], [4], 0.0, 10.0, one).p_values[0] == 1.0
    zero_phi = sa.SSeqParams(0, 1, np.zeros(0), np.array([1.0]), np.array([1.0]), np.array([True]), np.array([0.0]), 0.0, 0.0, np.array([0.0]))
    assert sa.sseq_de_from_sums([3], [4], 5.0, 10.0, zero_phi).p_values[0] == 1.0


# ---- 7. progress and cancellation ------------------------------------------------------------------------------------------------
def test_progress_and_cancel(sa):
    m = _random_counts(80, 300, 0.1, 3)
    h = _handle(sa, m, sa.CSR)
    params = sa.compute_sseq_params(h)
    labels = (np.arange(300) % 3).astype(np.int16)
    sn = sa.AtomicSnoop()
    sa.sseq_de_one_vs_rest(h, labels, params, snoop=sn)
    assert sn.history == [0.0, 0.1, 0.6, 0.75, 0.9, 0.95, 1.0]
    sn = sa.AtomicSnoop()
    sn.cancel()
    with pytest.raises(sa.CancellationError) as e:
        sa.sseq_de_one_vs_rest(h, labels, params, snoop=sn)
    assert e.value.code == 3


# ---- 8. at scale ---------------------------------------------------------------------------------------------------------------------
def test_one_vs_rest_at_100k_cells(sa):
    from scanrs_amd.synth import synth_counts_fast

    fx = np.load(os.path.join(TESTS, "golden", "config2_100k.npz"))
    cells, genes = int(fx["cells"]), int(fx["genes"])
    m = synth_counts_fast(cells, genes, float(fx["density"]), int(fx["seed"]))
    assert m.nnz == int(fx["nnz"])
    assert int(m.indices.astype(np.int64).sum()) == int(fx["sum_indices"]) and int(m.data.astype(np.int64).sum()) == int(fx["sum_values"])
    g = sparse.csc_matrix((m.data, m.indices, m.indptr), shape=(genes, cells))  # genes x cells, cell-major
    h = sa.AdaptiveMat.from_csmat(genes, cells, sa.CSC, m.indptr, m.indices, m.data)
    rng = np.random.default_rng(20)
    labels = rng.integers(-1, 20, cells).astype(np.int16)
    params = sa.compute_sseq_params(h)
    pref = ref.compute_sseq_params(g)
    np.testing.assert_array_equal(params.use_genes, pref["use_genes"])
    np.testing.assert_allclose(params.gene_phi, pref["gene_phi"], rtol=1e-10)
    got = sa.sseq_de_one_vs_rest(h, labels, params, n_groups=20)
    sums = np.zeros((genes, 20), dtype=np.uint64)
    gl = g.tocsc()
    for j in range(20):
        sums[:, j] = np.asarray(gl[:, np.flatnonzero(labels == j)].sum(axis=1), dtype=np.uint64).ravel()
    allsum = sums.sum(axis=1)
    totals = np.asarray(gl.sum(axis=1)).ravel()
    sample = np.unique(np.concatenate([rng.choice(genes, 290, replace=False), np.argsort(totals)[-10:]]))
    for j in range(20):
        np.testing.assert_array_equal(got[j].sums_in, sums[:, j])
        np.testing.assert_array_equal(got[j].sums_out, allsum - sums[:, j])
        fa = 0.0
        for i in np.flatnonzero(labels == j):
            fa += params.size_factors[i]
        fb = 0.0
        for i in np.flatnonzero((labels >= 0) & (labels != j)):
            fb += params.size_factors[i]
        sub = {k: (v[sample] if isinstance(v, np.ndarray) and v.shape == (genes,) else v) for k, v in params.__dict__.items()}
        e = ref.de_from_sums(sums[sample, j], allsum[sample] - sums[sample, j], fa, fb, sub)
        np.testing.assert_allclose(got[j].p_values[sample], e["p_values"], rtol=1e-9)
        # BH over every tested gene, from the device's p-values
        idx = np.flatnonzero(params.use_genes)
        np.testing.assert_allclose(got[j].adjusted_p_values[idx], ref.adjusted_pvalue_bh(got[j].p_values[idx]), rtol=1e-15)


# ---- 9. asymptotic test battery ---------------------------------------------------------------------------------------------------------
ASYM_BLOCK = 64  # threads per block of sseq_asymptotic_kernel
# Host and device run one source with their own log, log1p, exp and fma contraction. First measured: 768 ulp at most, at p = 9.8e-201,
# where one ulp of ln p (|ln p| = 460) is 512 ulp of p; about half of the 295 cases were bit-equal. Held to 4 x that (never below 4 ulp).
ASYM_HOST_DEVICE_ULP = 4 * 768


def _asym_params(sa, rows, use=True):
    mu, phi = np.array([r["mu"] for r in rows]), np.array([r["phi"] for r in rows])
    return sa.SSeqParams(0, len(rows), np.zeros(0), mu, np.ones(len(rows)), np.full(len(rows), use), phi, 0.0, 0.0, phi)


def _asym_call(sa, rows, **kw):
    """p-values of rows that share one (sf_a, sf_b), one gene per row, in ONE call"""
    assert len({(r["sf_a"], r["sf_b"]) for r in rows}) == 1
    kw.setdefault("big_count", 0)
    res = sa.sseq_de_from_sums([r["x_a"] for r in rows], [r["x_b"] for r in rows], rows[0]["sf_a"], rows[0]["sf_b"], _asym_params(sa, rows), **kw)
    return res.p_values


def _asym_groups(rows):
    return [[i for i, r in enumerate(rows) if r["group"] == g] for g in sorted({r["group"] for r in rows})]


def _asym_battery(sa, rows, **kw):
    """one call per (sf_a, sf_b) group: sseq_de_from_sums takes one size factor per test and side"""
    p = np.zeros(len(rows))
    for idx in _asym_groups(rows):
        p[idx] = _asym_call(sa, [rows[i] for i in idx], **kw)
    return p


def _ulps(a, b):
    """distance of positive doubles in units of the last place"""
    return np.abs(np.asarray(a, dtype=np.float64).view(np.int64) - np.asarray(b, dtype=np.float64).view(np.int64))


@pytest.fixture(scope="module")
def asym(sa):
    rows = acases.load_table()["nb"]
    assert len(_asym_groups(rows)) == 5 and min(len(g) for g in _asym_groups(rows)) > ASYM_BLOCK // 2
    return rows, _asym_battery(sa, rows)


def test_asym_battery_matches_the_series(sa, asym):
    rows, p = asym
    keys = acases.nb_keys(rows)
    err, tie_route = acases.nb_errors(rows, p)
    yard, _ = acases.nb_errors(rows, [r["scipy"] for r in rows])
    _, bound = acases.report("nb_asymptotic on the device", keys, err, yard)
    assert tie_route <= 0.02 * len(rows)
    bad = [(k, e, r) for k, e, r in zip(keys, err, rows) if not e <= bound[k]]
    assert not bad, (len(bad), max(bad, key=lambda t: t[1]))


def test_asym_battery_device_against_host(sa, asym):
    rows, p = asym
    host = np.array([sa.sseq.host_nb_asymptotic_test(r["x_a"], r["x_b"], r["sf_a"], r["sf_b"], r["mu"], r["phi"]) for r in rows])
    # a case at the median may take the other side on the other machine: both sides are in the table
    near = np.array([r["distance"] < acases.TIE_DISTANCE for r in rows])
    d = _ulps(p, host)
    for i in np.flatnonzero(near & (d > ASYM_HOST_DEVICE_ULP)):
        sides = [float(rows[i]["p_lower"]), float(rows[i]["p_upper"])]
        assert min(abs(p[i] - v) / v for v in sides) < 1e-12 and min(abs(host[i] - v) / v for v in sides) < 1e-12
        d[i] = 0
    i = int(np.argmax(d))
    print(f"\nhost against device: {int(d[i])} ulp at most (p = {p[i]!r}, {rows[i]['tag']}), {int(np.sum(d == 0))} of {len(rows)} cases bit-equal")
    assert d[i] <= ASYM_HOST_DEVICE_ULP


def test_asym_result_does_not_depend_on_the_batch(sa, asym):
    rows, p = asym
    again = _asym_battery(sa, rows)
    assert again.tobytes() == p.tobytes()
    for idx in _asym_groups(rows):
        # every case alone
        for i in idx:
            assert _asym_call(sa, [rows[i]])[0] == p[i], rows[i]
    # one test more than a block, against the same tests inside two full blocks
    sub = [r for r in rows if r["group"] == 2]
    assert len(sub) >= ASYM_BLOCK + 1
    wide = sub + sub
    wide = wide[:2 * ASYM_BLOCK]
    full = _asym_call(sa, wide)
    odd = _asym_call(sa, wide[:ASYM_BLOCK + 1])
    assert odd.tobytes() == full[:ASYM_BLOCK + 1].tobytes()
    assert full.tobytes() == np.array([p[rows.index(r)] for r in wide]).tobytes()


def test_asym_branch_is_taken_only_above_big_count_on_tested_genes(sa, asym):
    rows, p = asym
    sub = [r for r in rows if r["x_a"] + r["x_b"] == 3001 and min(r["x_a"], r["x_b"]) > 1 and r["group"] == 2][:6]
    assert len(sub) >= 3
    xa, xb = [r["x_a"] for r in sub], [r["x_b"] for r in sub]
    fa, fb = sub[0]["sf_a"], sub[0]["sf_b"]
    exact = sa.sseq_de_from_sums(xa, xb, fa, fb, _asym_params(sa, sub), big_count=2 ** 62).p_values
    asymp = np.array([p[rows.index(r)] for r in sub])
    # big_count = 2^62 is the exact test by definition; the restatement agrees with it as far as gammaln at sf / phi ~ 1e8 carries
    # (1e-8 absolute in every term's logarithm), and that is far closer than the beta approximation is to either
    e = np.array([ref.nb_exact_test(r["x_a"], r["x_b"], fa, fb, r["mu"], r["phi"]) for r in sub])
    np.testing.assert_allclose(exact, e, rtol=1e-6)
    assert (exact != asymp).all() and (np.abs(asymp - e) > 1e-3 * e).any()
    # use_genes false: the exact test, whatever the sums (diff_exp.rs:262)
    unused = sa.sseq_de_from_sums(xa, xb, fa, fb, _asym_params(sa, sub, use=False), big_count=0).p_values
    assert unused.tobytes() == exact.tobytes()
    # `>` big_count on both sides: a sum equal to big_count keeps the exact test, one above it on both sides leaves it
    for k, r in enumerate(sub):
        one = _asym_params(sa, [r])
        for big, want in ((r["x_a"], exact[k]), (r["x_b"], exact[k]), (min(r["x_a"], r["x_b"]) - 1, asymp[k])):
            got = sa.sseq_de_from_sums([r["x_a"]], [r["x_b"]], fa, fb, one, big_count=big).p_values[0]
            assert got == want, (r, big)


def test_asym_bits_do_not_depend_on_the_backend(sa, asym):
    rows, p = asym
    assert _asym_battery(sa, rows, backend=sa.NB_EXACT_RATIO).tobytes() == p.tobytes()
    assert _asym_battery(sa, rows, backend=sa.NB_EXACT_LOGSPACE).tobytes() == p.tobytes()


def test_asym_rows_through_the_matrix_routes(sa, asym):
    """A dozen battery rows as a 4-cell matrix (two cells per side, the counts split between them, u32): the matrix route on one
    handle and on a MultiMat with the cells sharded gives the bits of the sums route. sseq_de_pairs computes mu and phi of every
    pair from the matrix itself and so cannot be handed the battery's rows."""
    rows, p = asym
    sub = [r for r in rows if r["group"] == 2 and max(r["x_a"], r["x_b"]) < 2 ** 32 and min(r["x_a"], r["x_b"]) > 1][:12]
    assert len(sub) == 12
    m = np.array([[r["x_a"] // 2, r["x_a"] - r["x_a"] // 2, r["x_b"] // 2, r["x_b"] - r["x_b"] // 2] for r in sub], dtype=np.uint32)
    params = _asym_params(sa, sub)
    fa, fb = sub[0]["sf_a"], sub[0]["sf_b"]
    params.size_factors = np.array([fa / 2, fa / 2, fb / 2, fb / 2])
    assert fa / 2 + fa / 2 == fa and fb / 2 + fb / 2 == fb
    want = np.array([p[rows.index(r)] for r in sub])
    s = sparse.csc_matrix(m)
    s.sort_indices()
    ip, ix, vv = s.indptr.astype(np.uint64), s.indices.astype(np.uint32), s.data.astype(np.uint32)
    one = sa.sseq_differential_expression(sa.AdaptiveMat.from_csmat(12, 4, sa.CSC, ip, ix, vv), [0, 1], [2, 3], params, big_count=0)
    np.testing.assert_array_equal(one.sums_in, [r["x_a"] for r in sub])
    np.testing.assert_array_equal(one.sums_out, [r["x_b"] for r in sub])
    assert one.p_values.tobytes() == want.tobytes()
    multi = sa.sseq_differential_expression(sa.MultiMat(12, 4, sa.CSC, ip, ix, vv, 2, devices=[0, 0]), [0, 1], [2, 3], params, big_count=0)
    for f in FIELDS:
        assert getattr(multi, f).tobytes() == getattr(one, f).tobytes(), f
