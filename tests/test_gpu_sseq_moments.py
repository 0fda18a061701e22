"""The moments of compute_sseq_params on the device (sseq_gene_major_kernel, sseq_cell_major_kernel, sseq_term_class_kernel) and the
per-pair parameters of sseq_de_pairs against exact sums: the cases of tests/sseq_moments_cases.py, the reference and the contract of
tests/sseq_moments_ref.py (per gene |mean - exact| <= 1e-12 mean, |var - exact| <= 1e-10 S2 / m, use_genes equal wherever it is
posed, the dispersions within those bounds carried through their formulas). tests/test_sseq_moments_cpu.py asks the same of the
accumulation restated in Python integers and names the cases on which one quantum for all genes fails.

Every case runs from the gene-major and from the cell-major copy and over two shards of a MultiMat on device 0, which must give
identical bits. Five cases also run one one-vs-rest call with the device's parameters, umi_spread_1e12 with those of the per-gene
route. Four run once more with two workgroups per launch (option "sseq_grid_cap"), so that a wave takes several genes or cells in
turn, and one merge_clusters call pins the fused pass's literal route for a union that holds a cell total of 2^40.

Measured on an MI355X: the device's error / bound equals the Python-integer restatement's figure for figure (the sums are exact
integers), so the table of tests/test_sseq_moments_cpu.py is the device's as well. With the library as it was before the per-gene
quanta, 7 tests fail: one_huge_count (both variants: var 1.0e10 times its bound, one gene out of use_genes, zeta_hat 7.7,
delta 7.3, gene_phi 44), umi_spread_1e12 (its three umi variants: var 6.6 in median_small), huge_count_and_spread-huge_in_large
and pairs_total_2^40 (var 2.2 in the pairs that hold the cell). With it all pass, the worst at mean 2.7e-4 and var 4.9e-4 of the
bound (pairs_total_2^34, which stays on the batched route). The file takes 4 s."""
import os
import sys

import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import sseq_moments_cases as mc  # noqa: E402
import sseq_moments_ref as mr  # noqa: E402
import sseq_ref as ref  # noqa: E402

VARIANTS = mc.variant_ids()
IDS = [f"{a}-{b}" for a, b in VARIANTS]
PARAM_FIELDS = ("size_factors", "gene_means", "gene_variances", "use_genes", "gene_moment_phi", "gene_phi")
DE_FIELDS = ("sums_in", "sums_out", "p_values", "adjusted_p_values", "log2_fold_change", "normalized_mean_in", "normalized_mean_out")
# the variant whose parameters a case's one-vs-rest call runs with
# (umi_spread_1e12: the route with a quantum per gene)
DE_VARIANT = {"benign": "umi", "umi_spread_1e3": "median_large", "umi_spread_1e6": "median_large", "umi_spread_1e12": "median_large",
              "constant_gene": "umi"}
# the cases that also run with two workgroups per launch
CAPPED = [("wave_edges", "natural"), ("wave_edges", "cells+umi"), ("one_huge_count", "natural"), ("umi_spread_1e12", "median_large")]


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


def _arrays(m, storage_is_csr):
    s = sparse.csr_matrix(m) if storage_is_csr else sparse.csc_matrix(m)
    s.sort_indices()
    return s.indptr.astype(np.uint64), s.indices.astype(np.uint32), s.data.astype(np.uint32)


def _handle(sa, m, storage):
    """genes x cells scipy matrix -> handle in the given storage (CSR: gene-major, CSC: cell-major)"""
    return sa.AdaptiveMat.from_csmat(m.shape[0], m.shape[1], storage, *_arrays(m, storage == sa.CSR))


def _two_shards(sa, m):
    """the cells cut over two shards on device 0"""
    return sa.MultiMat(m.shape[0], m.shape[1], sa.CSC, *_arrays(m, False), 2, devices=[0, 0])


def _same_bits(a, b, what):
    for f in PARAM_FIELDS:
        assert np.asarray(getattr(a, f)).tobytes() == np.asarray(getattr(b, f)).tobytes(), (what, f)
    assert np.array([a.zeta_hat, a.delta]).tobytes() == np.array([b.zeta_hat, b.delta]).tobytes(), what


@pytest.mark.parametrize("name,vname", VARIANTS, ids=IDS)
def test_params_meet_the_contract_in_every_orientation_and_sharding(sa, name, vname):
    m, v = mc.case(name)["mat"], mc.variant(name, vname)
    mom, par, bounds = mr.exact_variant(name, vname)
    args = (0.995, v["cell_indices"], v["umi_counts"])
    res = {}
    for what, mat in (("gene-major", _handle(sa, m, sa.CSR)), ("cell-major", _handle(sa, m, sa.CSC)), ("two shards", _two_shards(sa, m))):
        got = res[what] = sa.compute_sseq_params(mat, *args)
        worst, mism = mr.worst_ratios(mom, par, bounds, got)
        print(name, vname, what, worst, mism)
        assert max(worst.values()) <= 1.0, (what, worst)
        assert mism == [], what
        np.testing.assert_array_equal(got.size_factors, mom["sf"])
    _same_bits(res["gene-major"], res["cell-major"], "cell-major")
    _same_bits(res["gene-major"], res["two shards"], "two shards")
    if name == "zero_factor":  # the non-finite path: (inf, NaN), out of use_genes, dispersion 0
        bad = np.array(mom["bad"])
        got = res["gene-major"]
        assert np.isposinf(got.gene_means[bad]).all() and np.isnan(got.gene_variances[bad]).all()
        assert not got.use_genes[bad].any() and (got.gene_phi[bad] == 0.0).all()


@pytest.mark.parametrize("name,vname", CAPPED, ids=[f"{a}-{b}" for a, b in CAPPED])
def test_a_wave_that_takes_several_genes_or_cells_gives_the_same_bits(sa, name, vname):
    """"sseq_grid_cap" = 2: two workgroups, eight outer vectors per sweep, so every wave of the moment pass, of the class walk and of
    the group pass walks 16 genes (32 or more cells) in turn, re-deriving a gene's scales at each"""
    m, v = mc.case(name)["mat"], mc.variant(name, vname)
    mom, par, bounds = mr.exact_variant(name, vname)
    labels = mc.de_labels(name)
    for what, storage in (("gene-major", sa.CSR), ("cell-major", sa.CSC)):
        h = _handle(sa, m, storage)
        whole = sa.compute_sseq_params(h, 0.995, v["cell_indices"], v["umi_counts"])
        sums = sa.group_sums(h, labels, 3)[0]
        h.set_option("sseq_grid_cap", 2)
        got = sa.compute_sseq_params(h, 0.995, v["cell_indices"], v["umi_counts"])
        _same_bits(whole, got, what)
        assert sa.group_sums(h, labels, 3)[0].tobytes() == sums.tobytes(), what
        worst, mism = mr.worst_ratios(mom, par, bounds, got)
        assert max(worst.values()) <= 1.0 and mism == [], (what, worst)
    mm = _two_shards(sa, m)
    mm.set_option("sseq_grid_cap", 2)
    _same_bits(whole, sa.compute_sseq_params(mm, 0.995, v["cell_indices"], v["umi_counts"]), "two shards")


def test_a_merge_candidate_with_a_huge_cell_total_takes_the_literal_route(sa):
    """the fused pass of merge_clusters: a union that holds a cell total of 2^40 is beyond the pass's one quantum and runs
    compute_sseq_params over the union (a quantum per gene: 5 passes) as the unfused route does, with the same bits"""
    c = mc.merge_total_case()
    h = _handle(sa, c["mat"], sa.CSC)
    lf, tf = sa.merge_clusters(h, c["scores"], c["labels"], trace=True)
    h.set_option("merge_fused", 0)
    ll, tl = sa.merge_clusters(h, c["scores"], c["labels"], trace=True)
    np.testing.assert_array_equal(lf, ll)
    assert (tf.leaf0[0], tf.leaf1[0]) == (0, 1)
    assert [e[:3] for e in tf.entries] == [e[:3] for e in tl.entries]
    huge = tf.leaf0 == 0  # cell 0's cluster keeps the label 0 through every merge
    assert huge.sum() >= 1
    assert tf.min_p_adj[huge].tobytes() == tl.min_p_adj[huge].tobytes()
    np.testing.assert_allclose(tf.min_p_adj, tl.min_p_adj, rtol=1e-6, atol=0)
    assert tf.n_passes == 2 + 5 * int(huge.sum())
    assert tl.n_passes == 5 * int(huge.sum()) + 4 * int((~huge).sum())


@pytest.mark.parametrize("name", list(mc.PAIRS_CASES))
def test_pair_params_meet_the_contract(sa, name):
    c = mc.case(name)
    m = c["mat"]
    res = {}
    for what, mat in (("gene-major", _handle(sa, m, sa.CSR)), ("cell-major", _handle(sa, m, sa.CSC)), ("two shards", _two_shards(sa, m))):
        _, params = sa.sseq_de_pairs(mat, c["labels"], c["pairs"], big_count=0, n_groups=c["n_groups"])
        res[what] = params
        for pair, got in zip(c["pairs"], params):
            mom = mr.pairs_exact(m, c["labels"], pair)
            par = mr.exact_params(mom)
            bounds = mr.downstream_bounds(mom, par)
            worst, mism = mr.worst_ratios(mom, par, bounds, got)
            print(name, pair, what, "literal" if got.literal else "batched", worst, mism)
            assert max(worst.values()) <= 1.0, (what, pair, worst)
            assert mism == [], (what, pair)
            assert got.literal == (mr.pairs_route(m, c["labels"], pair) == "literal")
            assert got.median_total == mom["m_s"] and got.num_cells == mom["m"]
    for what in ("cell-major", "two shards"):
        for a, b in zip(res["gene-major"], res[what]):
            for f in PARAM_FIELDS[1:]:
                assert np.asarray(getattr(a, f)).tobytes() == np.asarray(getattr(b, f)).tobytes(), (what, f)
            assert (a.zeta_hat, a.delta) == (b.zeta_hat, b.delta), what


@pytest.mark.parametrize("name", list(DE_VARIANT))
def test_one_vs_rest_with_the_adversarial_parameters(sa, name):
    """the device's parameters feed the tests: every DE field agrees with the restatement fed with the exact parameters"""
    m = mc.case(name)["mat"]
    assert mc.case(name)["de"]
    v = mc.variant(name, DE_VARIANT[name])
    mom, par, _ = mr.exact_variant(name, DE_VARIANT[name])
    labels = mc.de_labels(name)
    params = sa.compute_sseq_params(_handle(sa, m, sa.CSC), 0.995, v["cell_indices"], v["umi_counts"])
    got = sa.sseq_de_one_vs_rest(_handle(sa, m, sa.CSR), labels, params, n_groups=3)
    pref = dict(size_factors=mom["sf"], gene_means=np.array([float(x) for x in mom["mean"]]), use_genes=np.array(par["use"]),
                gene_phi=np.array([float(x) for x in par["gene_phi"]]))
    exp = ref.one_vs_rest(m, labels, pref, n_groups=3)
    for g, e in zip(got, exp):
        for f in DE_FIELDS:  # tests/test_gpu_sseq.py::_assert_de
            if f.startswith("sums"):
                np.testing.assert_array_equal(getattr(g, f), e[f], err_msg=f)
            else:
                np.testing.assert_allclose(getattr(g, f), e[f], rtol=1e-9 if "p_values" in f else 1e-12, atol=0, err_msg=f)
