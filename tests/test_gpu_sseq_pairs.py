"""Batched pairwise DE with per-pair sSeq parameters on the device (scan-rs_amd/csrc/sseq_pairs.hip) against the two CPU
restatements of tests/sseq_pairs_ref.py (the reference's two calls per pair, and the library's route in exact integers), against
the library's own literal route, and against itself (independence of the pairs, of the orientation and of the order of a pair).

Bounds against the restatements (the ones tests/test_sseq_pairs_cpu.py holds the two restatements to): use_genes and the sums
identical; means rtol 1e-12; variance, zeta_hat, delta rtol 1e-10; |Δphi| <= 1e-10 zeta_hat; p and adjusted p rtol 1e-9. A p
outside 1e-9 passes only inside the tie bounds of its own inputs (a term tying with the observed one to 1e-12: rounding decides
its side of `<=`, in the reference too), for at most 0.1 % of a case's tests. log2 fold changes: rtol 1e-12 against the fused
restatement (the same size factors), |Δ| <= 1e-12 against the literal one (size factors equal to 1e-15 relative move the logarithm by
that much absolutely, whatever its size)."""
import os
import sys

import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import sseq_pairs_ref as pref  # noqa: E402
import sseq_ratio_ref as rref  # noqa: E402
import sseq_ref as ref  # noqa: E402

ORIENTATIONS = ("csr", "csc", "t")
RESULT_FIELDS = ("sums_in", "sums_out", "p_values", "adjusted_p_values", "log2_fold_change", "normalized_mean_in", "normalized_mean_out")
PARAM_FIELDS = ("gene_means", "gene_variances", "gene_moment_phi", "gene_phi", "use_genes")
PARAM_SCALARS = ("zeta_hat", "delta", "median_total", "sum_size_factors", "num_cells")


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


def _handle(sa, m, orientation):
    """genes x cells scipy matrix -> a genes x cells handle: gene-major (csr), cell-major (csc), or the transposed view of a
    cells x genes handle (t)."""
    g, c = m.shape
    if orientation == "t":
        s = sparse.csr_matrix(m.T)
        s.sort_indices()
        return sa.AdaptiveMat.from_csmat(c, g, sa.CSR, s.indptr.astype(np.uint64), s.indices.astype(np.uint32), s.data.astype(np.uint32)).t()
    storage = sa.CSR if orientation == "csr" else sa.CSC
    s = sparse.csr_matrix(m) if orientation == "csr" else sparse.csc_matrix(m)
    s.sort_indices()
    return sa.AdaptiveMat.from_csmat(g, c, storage, s.indptr.astype(np.uint64), s.indices.astype(np.uint32), s.data.astype(np.uint32))


def _bits(results, params):
    out = []
    for r, q in zip(results, params):
        out.append(tuple(np.ascontiguousarray(getattr(r, f)).tobytes() for f in RESULT_FIELDS) +
                   tuple(np.ascontiguousarray(getattr(q, f)).tobytes() for f in PARAM_FIELDS) +
                   tuple(np.float64(getattr(q, f)).tobytes() for f in PARAM_SCALARS + ("size_factor_a", "size_factor_b")))
    return out


def _param_bits(q):
    return tuple(np.ascontiguousarray(getattr(q, f)).tobytes() for f in PARAM_FIELDS) + tuple(np.float64(getattr(q, f)).tobytes() for f in PARAM_SCALARS)


def _close(got, exp, rtol, what):
    np.testing.assert_allclose(got, exp, rtol=rtol, atol=0, err_msg=what)


def _assert_params(q, e, what, phi_scale=None):
    """phi_scale: the scale of the dispersion bound, zeta_hat unless the caller has a reason for another."""
    np.testing.assert_array_equal(q.use_genes, e["use_genes"], err_msg=what)
    _close(q.gene_means, e["gene_means"], 1e-12, what + " means")
    _close(q.gene_variances, e["gene_variances"], 1e-10, what + " variances")
    _close([q.zeta_hat, q.delta], [e["zeta_hat"], e["delta"]], 1e-10, what + " zeta_hat, delta")
    d = np.abs(q.gene_phi - e["gene_phi"])
    np.testing.assert_array_equal(np.isnan(q.gene_phi), np.isnan(e["gene_phi"]), err_msg=what)
    scale = e["zeta_hat"] if phi_scale is None else phi_scale
    assert np.all(np.where(np.isnan(d), 0.0, d) <= 1e-10 * scale), (what, float(np.nanmax(d)), scale)
    assert len(q.size_factors) == 0


def _assert_result(r, q, e, backend, what, same_size_factors):
    """-> the number of p-values that needed the tie bounds."""
    np.testing.assert_array_equal(r.sums_in, e["sums_in"], err_msg=what)
    np.testing.assert_array_equal(r.sums_out, e["sums_out"], err_msg=what)
    _close([q.size_factor_a, q.size_factor_b], [e["size_factor_a"], e["size_factor_b"]], 1e-12, what + " size factors")
    _close(r.normalized_mean_in, e["normalized_mean_in"], 1e-12, what + " mean_in")
    _close(r.normalized_mean_out, e["normalized_mean_out"], 1e-12, what + " mean_out")
    if same_size_factors:
        _close(r.log2_fold_change, e["log2_fold_change"], 1e-12, what + " log2fc")
    else:
        np.testing.assert_allclose(r.log2_fold_change, e["log2_fold_change"], rtol=0, atol=1e-12, err_msg=what + " log2fc")
    p, ep = r.p_values, e["p_values"]
    np.testing.assert_array_equal(np.isnan(p), np.isnan(ep), err_msg=what)
    with np.errstate(invalid="ignore", divide="ignore"):
        off = np.flatnonzero(~np.isnan(p) & (p != ep) & ~(np.abs(p - ep) <= 1e-9 * np.abs(ep)))
    for g in off:
        assert e["exact"][g], (what, g, p[g], ep[g])
        args = (int(r.sums_in[g]), int(r.sums_out[g]), q.size_factor_a, q.size_factor_b, float(q.gene_means[g]), float(q.gene_phi[g]))
        ratio = backend == pref.RATIO and rref.in_ratio_partition(*args)
        lo, hi = (rref.nb_exact_test_ratio_tie_bounds if ratio else ref.nb_exact_test_tie_bounds)(*args)
        assert lo * (1 - 1e-9) <= p[g] <= hi * (1 + 1e-9), (what, g, p[g], ep[g], lo, hi)
    use = np.flatnonzero(r.genes_tested)
    # BH over the tested genes, from the device's own p-values; against the restatement's where no p needed the tie bounds
    np.testing.assert_allclose(r.adjusted_p_values[use], ref.adjusted_pvalue_bh(p[use]), rtol=1e-12, atol=0, err_msg=what)
    np.testing.assert_array_equal(np.delete(r.adjusted_p_values, use), np.delete(p, use), err_msg=what)
    if not len(off):
        _close(r.adjusted_p_values, e["adjusted_p_values"], 1e-9, what + " adjusted p")
    return len(off)


_RUNS = {}


def _run_case(sa, idx, backend, orientation):
    key = (idx, backend, orientation)
    if key not in _RUNS:
        case = pref.case_results(idx, backend)[0]
        h = _handle(sa, case["mat"], orientation)
        _RUNS[key] = sa.sseq_de_pairs(h, case["labels"], case["pairs"], backend=backend, n_groups=case["n_groups"])
    return _RUNS[key]


# ---- 1. against both restatements ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orientation", ORIENTATIONS)
@pytest.mark.parametrize("backend", [pref.LOGSPACE, pref.RATIO])
@pytest.mark.parametrize("idx", range(len(pref.CASES)))
def test_against_both_restatements(sa, idx, backend, orientation):
    case, lit, fus = pref.case_results(idx, backend)
    results, params = _run_case(sa, idx, backend, orientation)
    assert len(results) == len(params) == len(case["pairs"])
    n_tie = {"literal": 0, "fused": 0}
    for j, (a, b) in enumerate(case["pairs"]):
        r, q = results[j], params[j]
        assert not q.literal and q.num_cells == q.num_cells_a + q.num_cells_b
        assert (q.num_cells_a, q.num_cells_b) == (int(np.sum(case["labels"] == a)), int(np.sum(case["labels"] == b)))
        for name, (ep, er), same in (("literal", lit[j], False), ("fused", fus[j], True)):
            what = f"case {pref.CASES[idx]} pair {(a, b)} {orientation} against the {name} restatement"
            _assert_params(q, ep, what)
            n_tie[name] += _assert_result(r, q, er, backend, what, same)
        _close([q.median_total, q.sum_size_factors], [fus[j][0]["median_total"], fus[j][0]["sum_size_factors"]], 1e-15, "pair header")
        np.testing.assert_array_equal(r.common_mean, q.gene_means)
        np.testing.assert_array_equal(r.common_dispersion, q.gene_phi)
    assert max(n_tie.values()) <= 1e-3 * case["genes"] * len(case["pairs"]), n_tie


# ---- 2. independence ------------------------------------------------------------------------------------------------------------------
def test_a_pair_does_not_depend_on_the_other_pairs_of_the_call(sa):
    case = pref.case_results(3)[0]
    for backend in (pref.LOGSPACE, pref.RATIO):
        many = _bits(*_run_case(sa, 3, backend, "csr"))
        h = _handle(sa, case["mat"], "csr")
        for j, pair in enumerate(case["pairs"]):
            one = _bits(*sa.sseq_de_pairs(h, case["labels"], [pair], backend=backend, n_groups=case["n_groups"]))
            assert one[0] == many[j], (backend, pair)
        # and not on their order or on a repeated pair
        rev = _bits(*sa.sseq_de_pairs(h, case["labels"], case["pairs"][::-1] + case["pairs"][:2], backend=backend, n_groups=case["n_groups"]))
        assert rev[:len(many)] == many[::-1] and rev[len(many):] == many[:2]


@pytest.mark.parametrize("idx", [0, 2, 4])
def test_every_orientation_gives_the_same_bits(sa, idx):
    for backend in (pref.LOGSPACE, pref.RATIO):
        base = _bits(*_run_case(sa, idx, backend, "csr"))
        for o in ("csc", "t"):
            assert _bits(*_run_case(sa, idx, backend, o)) == base, (backend, o)


def test_swapping_a_pair_leaves_its_parameters_bit_identical(sa):
    case = pref.case_results(4)[0]
    h = _handle(sa, case["mat"], "csc")
    fw_r, fw = sa.sseq_de_pairs(h, case["labels"], case["pairs"], n_groups=case["n_groups"])
    bw_r, bw = sa.sseq_de_pairs(h, case["labels"], [(b, a) for a, b in case["pairs"]], n_groups=case["n_groups"])
    for j in range(len(fw)):
        assert _param_bits(fw[j]) == _param_bits(bw[j]), case["pairs"][j]
        assert (fw[j].size_factor_a, fw[j].size_factor_b) == (bw[j].size_factor_b, bw[j].size_factor_a)
        np.testing.assert_array_equal(fw_r[j].sums_in, bw_r[j].sums_out)
        np.testing.assert_array_equal(fw_r[j].log2_fold_change, -bw_r[j].log2_fold_change)


# ---- 3. against the library's literal route ------------------------------------------------------------------------------------------
def test_against_the_literal_calls_at_20k_cells(sa):
    rng = np.random.default_rng(31)
    genes, cells, n_groups = 2000, 20000, 13  # a control and 12 conditions
    rate = rng.gamma(0.5, 0.4, genes)
    rate[:5] = 3.0
    m = sparse.csr_matrix(rng.poisson(rate[:, None] * rng.uniform(0.5, 2.0, cells)[None, :]).astype(np.uint32))
    labels = np.where(rng.random(cells) < 0.5, 0, rng.integers(-1, n_groups, cells)).astype(np.int16)
    h = _handle(sa, m, "csc")
    results, params = sa.sseq_de_each_vs_control(h, labels, control=0, n_groups=n_groups)
    assert len(results) == 12 and h.counter("de_pairs_passes") == 2 and h.counter("de_pairs_literal") == 0
    for j, g in enumerate(range(1, n_groups)):
        a, b = np.flatnonzero(labels == g), np.flatnonzero(labels == 0)
        lp = sa.compute_sseq_params(h, cell_indices=np.sort(np.concatenate([a, b])))
        lr = sa.sseq_differential_expression(h, a, b, lp)
        np.testing.assert_array_equal(params[j].use_genes, lp.use_genes)
        np.testing.assert_array_equal(results[j].sums_in, lr.sums_in)
        np.testing.assert_array_equal(results[j].sums_out, lr.sums_out)
        np.testing.assert_allclose(params[j].gene_means, lp.gene_means, rtol=1e-12)
        np.testing.assert_allclose([params[j].zeta_hat, params[j].delta], [lp.zeta_hat, lp.delta], rtol=1e-10)
        np.testing.assert_allclose(results[j].adjusted_p_values, lr.adjusted_p_values, rtol=1e-6, atol=0)


# ---- 4. edge cases --------------------------------------------------------------------------------------------------------------------
def test_a_union_with_median_total_zero_takes_the_literal_route(sa):
    rng = np.random.default_rng(7)
    genes = 40
    labels = np.repeat(np.arange(3), [30, 30, 40]).astype(np.int16)
    counts = rng.poisson(2.0, (genes, 100)).astype(np.uint32)
    counts[:, :25] = 0
    counts[:, 30:55] = 0  # groups 0 and 1 are mostly empty cells
    m = sparse.csr_matrix(counts)
    for o in ORIENTATIONS:
        h = _handle(sa, m, o)
        for backend in (pref.LOGSPACE, pref.RATIO):
            results, params = sa.sseq_de_pairs(h, labels, [(2, 0), (0, 1), (1, 2)], backend=backend)
            assert [q.literal for q in params] == [False, True, False]
            assert h.counter("de_pairs_literal") == 1 and h.counter("de_pairs_passes") == 2 + 4
            a, b = np.flatnonzero(labels == 0), np.flatnonzero(labels == 1)
            lp = sa.compute_sseq_params(h, cell_indices=np.concatenate([a, b]))
            lr = sa.sseq_differential_expression(h, a, b, lp, backend=backend)
            for f in RESULT_FIELDS:
                assert np.ascontiguousarray(getattr(results[1], f)).tobytes() == np.ascontiguousarray(getattr(lr, f)).tobytes(), f
            for f in PARAM_FIELDS + ("zeta_hat", "delta"):
                assert np.ascontiguousarray(getattr(params[1], f)).tobytes() == np.ascontiguousarray(getattr(lp, f)).tobytes(), f
            assert params[1].median_total == 0.0
            # the other pairs of the call are the ones a call without the literal pair gives
            alone = sa.sseq_de_pairs(h, labels, [(2, 0), (1, 2)], backend=backend)
            assert _bits(*alone) == [_bits(results, params)[0], _bits(results, params)[2]]
            assert h.counter("de_pairs_literal") == 0 and h.counter("de_pairs_passes") == 2


def test_one_empty_side_gives_p_one_everywhere(sa):
    case = pref.case_results(2)[0]
    h = _handle(sa, case["mat"], "csr")
    empty = case["n_groups"]  # a group no cell carries
    results, params = sa.sseq_de_pairs(h, case["labels"], [(empty, 0), (1, empty)], n_groups=case["n_groups"] + 1)
    gs = pref.GroupSums(case["mat"], case["labels"], case["n_groups"] + 1)
    for (r, q), (a, b) in zip(zip(results, params), [(empty, 0), (1, empty)]):
        assert (q.num_cells_a == 0) != (q.num_cells_b == 0) and (q.size_factor_a == 0.0) != (q.size_factor_b == 0.0)
        assert np.all(r.p_values == 1.0) and np.all(r.adjusted_p_values == 1.0)
        ep, er = pref.fused_pair(gs, a, b)
        _assert_params(q, ep, "one empty side")
        _assert_result(r, q, er, pref.LOGSPACE, "one empty side", True)
        lp, lr = pref.literal_pair(case["mat"], case["labels"], a, b)
        _assert_params(q, lp, "one empty side, literal")


def test_no_gene_with_variance(sa):
    # every cell holds (1, 1, 2, 0): x / u is exact in binary, so every variance is exactly 0 and no gene is used
    m = sparse.csr_matrix(np.tile(np.array([[1], [1], [2], [0]], dtype=np.uint32), (1, 50)))
    labels = (np.arange(50) % 3).astype(np.int16)
    for o in ORIENTATIONS:
        results, params = sa.sseq_de_pairs(_handle(sa, m, o), labels, [(0, 1), (2, 0)])
        for r, q in zip(results, params):
            assert not q.use_genes.any() and q.zeta_hat == 0.0 and q.delta == 0.0 and not q.gene_phi.any() and not q.literal
            np.testing.assert_array_equal(q.gene_means, [1.0, 1.0, 2.0, 0.0])
            assert np.all(r.p_values == 1.0) and np.all(r.adjusted_p_values == 1.0)


@pytest.mark.parametrize("zeta", [0.0, 1.0, 0.5])
def test_zeta_quintile_ends(sa, zeta):
    case = pref.case_results(2)[0]
    gs = pref.GroupSums(case["mat"], case["labels"], case["n_groups"])
    results, params = sa.sseq_de_pairs(_handle(sa, case["mat"], "t"), case["labels"], case["pairs"], zeta_quintile=zeta, n_groups=case["n_groups"])
    for j, (a, b) in enumerate(case["pairs"]):
        ep, er = pref.fused_pair(gs, a, b, zeta=zeta)
        used = ep["gene_moment_phi"][ep["use_genes"]]
        if zeta in (0.0, 1.0):
            assert params[j].zeta_hat == (used.min() if zeta == 0.0 else used.max())  # an element of the list, bit for bit
        # phi is a mix of phi_mm and zeta_hat whose weight delta is held to rtol 1e-10: its error is bounded by 1e-10 of the larger of
        # the two, and below the top quantile zeta_hat is the smaller one (0 at zeta = 0), so the largest used dispersion is the scale
        _assert_params(params[j], ep, f"zeta {zeta} pair {(a, b)}", phi_scale=used.max())
        _assert_result(results[j], params[j], er, pref.LOGSPACE, f"zeta {zeta} pair {(a, b)}", True)


def test_a_single_used_gene(sa):
    # the one-gene case: x / u is 1 in the cells that hold a count and 0 elsewhere, so its gene has a variance and is the only used one
    case = pref.case_results(0)[0]
    gs = pref.GroupSums(case["mat"], case["labels"], case["n_groups"])
    for zeta in (0.0, 0.3, 1.0):
        results, params = sa.sseq_de_pairs(_handle(sa, case["mat"], "csc"), case["labels"], case["pairs"], zeta_quintile=zeta, n_groups=case["n_groups"])
        for j, (a, b) in enumerate(case["pairs"]):
            ep, er = pref.fused_pair(gs, a, b, zeta=zeta)
            if params[j].use_genes[0]:
                assert params[j].zeta_hat == params[j].gene_moment_phi[0]
            _assert_params(params[j], ep, f"one gene, zeta {zeta}, pair {(a, b)}")
            _assert_result(results[j], params[j], er, pref.LOGSPACE, f"one gene, zeta {zeta}, pair {(a, b)}", True)
        assert sum(int(q.use_genes[0]) for q in params) >= len(params) - 1


def test_unions_of_one_and_two_cells(sa):
    """A union of one cell: m_S is its total and every size-normalized count is the count itself; the variance is 0 up to the
    rounding of x / u * u, so the tests all return 1 whether or not that rounding leaves a gene marked as used (the literal calls
    divide by a size factor of exactly 1 and mark none). Checked against the fused restatement, which rounds as the library does,
    and in its p-values against the literal one. A union of two cells is an ordinary case for both."""
    case = pref.case_results(3)[0]
    labels = case["labels"].copy()
    n = case["n_groups"]
    free = np.flatnonzero(labels == -1)[:2]
    labels[free[0]], labels[free[1]] = n, n + 1  # two more singletons; group n + 2 is empty
    single = n - 2
    pairs = [(single, n + 2), (n + 2, n), (single, n), (n + 1, n)]
    gs = pref.GroupSums(case["mat"], labels, n + 3)
    for o in ORIENTATIONS:
        results, params = sa.sseq_de_pairs(_handle(sa, case["mat"], o), labels, pairs, n_groups=n + 3)
        for j, (a, b) in enumerate(pairs):
            ep, er = pref.fused_pair(gs, a, b)
            lp, lr = pref.literal_pair(case["mat"], labels, a, b)
            what = f"pair {(a, b)} {o}"
            assert params[j].num_cells == (1 if j < 2 else 2) and params[j].median_total == ep["median_total"]
            _assert_params(params[j], ep, what)
            _assert_result(results[j], params[j], er, pref.LOGSPACE, what, True)
            if j < 2:
                assert np.all(results[j].p_values == 1.0) and np.all(lr["p_values"] == 1.0) and np.all(results[j].adjusted_p_values == 1.0)
            else:
                _assert_params(params[j], lp, what + " literal")
                _assert_result(results[j], params[j], lr, pref.LOGSPACE, what + " literal", False)


# ---- 5. pass counts -------------------------------------------------------------------------------------------------------------------
def test_more_groups_than_one_tile_of_the_grouped_pass(sa):
    rng = np.random.default_rng(17)
    genes, cells, n_groups = 64, 4000, 1601
    m = sparse.csr_matrix((rng.geometric(0.4, (genes, cells)) - 1).astype(np.uint32))
    labels = rng.integers(1, n_groups, cells).astype(np.int16)
    labels[rng.permutation(cells)[:800]] = 0
    labels[:5] = n_groups - 1  # the last group of the second tile is not empty
    pairs = [(g, 0) for g in range(1, n_groups)]
    hg, hc = _handle(sa, m, "csr"), _handle(sa, m, "csc")
    got_g = sa.sseq_de_pairs(hg, labels, pairs, n_groups=n_groups)
    got_c = sa.sseq_de_pairs(hc, labels, pairs, n_groups=n_groups)
    assert hg.counter("de_pairs_passes") == 3 and hc.counter("de_pairs_passes") == 2
    assert _bits(*got_g) == _bits(*got_c)
    # spot checks against the restatement, in both tiles
    gs = pref.GroupSums(m, labels, n_groups)
    for j in (0, 700, 1535, 1536, 1599):
        ep, er = pref.fused_pair(gs, *pairs[j])
        _assert_params(got_g[1][j], ep, f"pair {pairs[j]}")
        _assert_result(got_g[0][j], got_g[1][j], er, pref.LOGSPACE, f"pair {pairs[j]}", True)


def test_two_passes_whatever_the_number_of_pairs(sa):
    case = pref.case_results(3)[0]
    for o in ORIENTATIONS:
        h = _handle(sa, case["mat"], o)
        for pairs in (case["pairs"][:1], case["pairs"], case["pairs"] * 40):
            sa.sseq_de_pairs(h, case["labels"], pairs, n_groups=case["n_groups"])
            assert h.counter("de_pairs_passes") == 2 and h.counter("de_pairs_literal") == 0
    labels = (np.arange(case["cells"]) % 1536).astype(np.int16)
    h = _handle(sa, case["mat"], "csr")
    sa.sseq_de_pairs(h, labels, [(5, 0), (1535, 7)], n_groups=1536)
    assert h.counter("de_pairs_passes") == 2


# ---- 6. refusals, progress and cancel ------------------------------------------------------------------------------------------------
def test_refusals(sa):
    case = pref.case_results(2)[0]
    h = _handle(sa, case["mat"], "csr")
    lab, n = case["labels"], case["n_groups"]
    bad = [
        (dict(pairs=[(1, n)]), "outside"),  # a group index >= n_groups
        (dict(pairs=[(n, 1)]), "outside"),
        (dict(pairs=[(1, 0), (2, 2)]), "against itself"),
        (dict(pairs=[(n, n + 1)], n_groups=n + 2), "no cell"),  # both sides empty
        (dict(pairs=[]), "n_pairs"),
        (dict(pairs=[(1, 0)], n_groups=8193), "n_groups"),
    ]
    for kw, word in bad:
        with pytest.raises(sa.ScanrsError) as e:
            sa.sseq_de_pairs(h, lab, **{"n_groups": n, **kw})
        assert e.value.code == 6 and word in str(e.value), (kw, str(e.value))
    for backend in (2, -1, True, None):
        with pytest.raises(sa.ScanrsError) as e:
            sa.sseq_de_pairs(h, lab, [(1, 0)], backend=backend)
        assert e.value.code == 6 and "backend" in str(e.value)
    # the C entry point refuses a bad backend itself
    import ctypes

    z = np.zeros(case["genes"])
    zi = np.zeros(case["genes"], dtype=np.uint64)
    pa, pb = np.array([1], dtype=np.uint32), np.array([0], dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    code = sa._lib.scanrs_sseq_de_pairs(h._h, p(lab), ctypes.c_uint32(n), p(pa), p(pb), ctypes.c_uint32(1), ctypes.c_double(0.995),
                                        ctypes.c_uint64(900), ctypes.c_int(7), None, p(zi), p(zi.copy()), p(z), p(z.copy()), p(z.copy()),
                                        p(z.copy()), p(z.copy()), None)
    assert code == 6
    with pytest.raises(sa.ScanrsError):
        sa.sseq_de_pairs(h, lab, [(1, 0)], zeta_quintile=1.5)
    with pytest.raises(sa.ScanrsError):
        sa.sseq_de_each_vs_control(h, lab, control=n, n_groups=n)


def test_a_sharded_handle_is_refused(sa):
    case = pref.case_results(2)[0]
    h = _handle(sa, case["mat"], "csr")
    h.set_shard(0, 1, 0, case["cells"], lambda *a: 0)
    with pytest.raises(sa.ScanrsError) as e:
        sa.sseq_de_pairs(h, case["labels"], [(1, 0)])
    assert e.value.code == 6 and "sharded" in str(e.value)


def test_null_params_and_each_vs_control(sa):
    import ctypes

    case = pref.case_results(2)[0]
    h = _handle(sa, case["mat"], "csc")
    n, genes = case["n_groups"], case["genes"]
    results, params = sa.sseq_de_each_vs_control(h, case["labels"], control=0, n_groups=n)
    assert _bits(results, params) == _bits(*_run_case(sa, 2, pref.LOGSPACE, "csc"))[:n - 1]
    ctl = sa.sseq_de_each_vs_control(h, case["labels"], control=2, n_groups=n)
    assert _bits(*ctl) == _bits(*sa.sseq_de_pairs(h, case["labels"], [(g, 2) for g in range(n) if g != 2], n_groups=n))
    # params = NULL: the results alone, the same bits
    t = n - 1
    pa, pb = np.arange(1, n, dtype=np.uint32), np.zeros(t, dtype=np.uint32)
    si, so = np.zeros((genes, t), dtype=np.uint64), np.zeros((genes, t), dtype=np.uint64)
    pv, pq, l2, mi, mo = (np.zeros((genes, t)) for _ in range(5))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lab = np.ascontiguousarray(case["labels"], dtype=np.int16)
    code = sa._lib.scanrs_sseq_de_pairs(h._h, p(lab), ctypes.c_uint32(n), p(pa), p(pb), ctypes.c_uint32(t), ctypes.c_double(0.995),
                                        ctypes.c_uint64(900), ctypes.c_int(0), None, p(si), p(so), p(pv), p(pq), p(l2), p(mi), p(mo), None)
    assert code == 0
    for j in range(t):
        np.testing.assert_array_equal(pv[:, j], results[j].p_values)
        np.testing.assert_array_equal(pq[:, j], results[j].adjusted_p_values)
        np.testing.assert_array_equal(si[:, j], results[j].sums_in)


def test_progress_and_cancel(sa):
    case = pref.case_results(2)[0]
    h = _handle(sa, case["mat"], "csr")
    sn = sa.AtomicSnoop()
    sa.sseq_de_pairs(h, case["labels"], case["pairs"], snoop=sn)
    assert sn.history == [0.0, 0.1, 0.6, 0.75, 0.9, 0.95, 1.0]
    sn = sa.AtomicSnoop()
    sn.cancel()
    with pytest.raises(sa.CancellationError) as e:
        sa.sseq_de_pairs(h, case["labels"], case["pairs"], snoop=sn)
    assert e.value.code == 3
