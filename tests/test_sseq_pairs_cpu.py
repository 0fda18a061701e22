"""Batched pairwise DE with per-pair parameters, without a device: the new symbols, the host's union median against the sorted
concatenation, and the fused restatement (the library's route, exact integer fixed point) against the literal one (the reference's
two calls per pair) on the cases the GPU tests run. Bounds: use_genes identical; means rtol 1e-12; variance, zeta_hat, delta rtol
1e-10; |Δphi| <= 1e-10 zeta_hat; p and adjusted p rtol 1e-9 (the `_assert_de` bound of tests/test_gpu_sseq.py), with no allowance
for ties: the generator's seeds are fixed to cases that need none."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import sseq_pairs_ref as pref  # noqa: E402
import sseq_ref as ref  # noqa: E402

NEW_SYMBOLS = ("scanrs_sseq_de_pairs", "scanrs_host_union_median")


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


def test_the_pairs_interface_is_declared_mirrored_exported_and_cites_the_reference(sa):
    hdr = open(os.path.join(ROOT, "include", "scanrs_amd.h")).read()
    hpp = open(os.path.join(ROOT, "include", "scanrs_amd.hpp")).read()
    lib = ctypes.CDLL(sa.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name + "(" in hpp, name
        assert name in sa.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert "} scanrs_sseq_pair_params;" in hdr
    doc = hdr[hdr.index("Batched pairwise DE"):hdr.index("int scanrs_sseq_de_pairs(")]
    for cite in ("diff_exp.rs:125-161", "diff_exp.rs:361-376", "diff_exp.rs:458-490", "merge_clusters.rs", "de_pairs_passes", "de_pairs_literal"):
        assert cite in doc, cite
    counters = hdr[hdr.index("Event counters of the handle"):hdr.index("int scanrs_mat_get_counter(")]
    assert "de_pairs_passes" in counters and "de_pairs_literal" in counters
    for fn in ("sseq_de_pairs", "sseq_de_each_vs_control", "host_union_median"):
        assert callable(getattr(sa, fn)) and getattr(sa, fn) is getattr(sa.sseq, fn)
    assert os.path.exists(os.path.join(ROOT, "scan-rs_amd", "csrc", "sseq_pairs.hip"))
    mk = open(os.path.join(ROOT, "scan-rs_amd", "csrc", "Makefile")).read()
    assert "sseq_pairs.hip" in mk and "sseq_pairs_host.cpp" in mk


@pytest.mark.parametrize("na,nb", [(0, 1), (1, 0), (1, 1), (2, 3), (64, 65)])
def test_host_union_median_equals_the_median_of_the_concatenation(sa, na, nb):
    rng = np.random.default_rng(100 * na + nb)
    for trial in range(8):
        hi = 4 if trial % 2 else 1000  # a small range: many ties inside and across the lists
        a = np.sort(rng.integers(0, hi, na).astype(np.float64))
        b = np.sort(rng.integers(0, hi, nb).astype(np.float64))
        got = sa.host_union_median(a, b)
        exp = ref.median(np.concatenate([a, b]))
        assert got == exp and np.signbit(got) == np.signbit(exp), (a, b, got, exp)
        assert sa.host_union_median(b, a) == exp


def test_host_union_median_refuses_two_empty_lists(sa):
    with pytest.raises(sa.ScanrsError) as e:
        sa.host_union_median([], [])
    assert e.value.code == 6


def _rel(got, exp):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    both_nan = np.isnan(got) & np.isnan(exp)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(got - exp) / np.abs(exp)
    r = np.where((got == exp) | both_nan, 0.0, r)
    return float(np.max(r)) if r.size else 0.0


@pytest.mark.parametrize("backend", [pref.LOGSPACE, pref.RATIO])
@pytest.mark.parametrize("idx", range(len(pref.CASES)))
def test_fused_restatement_against_the_literal_one(idx, backend):
    case, lit, fus = pref.case_results(idx, backend)
    worst = dict(mean=0.0, var=0.0, phi=0.0, zeta=0.0, delta=0.0, p=0.0, padj=0.0)
    n_asym = 0
    for (lp, lr), (fp, fr) in zip(lit, fus):
        np.testing.assert_array_equal(fp["use_genes"], lp["use_genes"])
        np.testing.assert_array_equal(fr["sums_in"], lr["sums_in"])
        np.testing.assert_array_equal(fr["sums_out"], lr["sums_out"])
        worst["mean"] = max(worst["mean"], _rel(fp["gene_means"], lp["gene_means"]))
        worst["var"] = max(worst["var"], _rel(fp["gene_variances"], lp["gene_variances"]))
        worst["zeta"] = max(worst["zeta"], _rel(fp["zeta_hat"], lp["zeta_hat"]))
        worst["delta"] = max(worst["delta"], _rel(fp["delta"], lp["delta"]))
        if lp["zeta_hat"] > 0:
            d = np.abs(fp["gene_phi"] - lp["gene_phi"])
            worst["phi"] = max(worst["phi"], float(np.max(np.where(np.isnan(d), 0.0, d))) / lp["zeta_hat"])
        np.testing.assert_array_equal(np.isnan(fp["gene_phi"]), np.isnan(lp["gene_phi"]))
        worst["p"] = max(worst["p"], _rel(fr["p_values"], lr["p_values"]))
        worst["padj"] = max(worst["padj"], _rel(fr["adjusted_p_values"], lr["adjusted_p_values"]))
        np.testing.assert_allclose([fr["size_factor_a"], fr["size_factor_b"]], [lr["size_factor_a"], lr["size_factor_b"]], rtol=1e-12)
        n_asym += int(np.sum(~lr["exact"]))
    print(f"case {pref.CASES[idx]} backend {backend}: {worst}, asymptotic tests {n_asym}")
    assert worst["mean"] <= 1e-12 and worst["var"] <= 1e-10 and worst["zeta"] <= 1e-10 and worst["delta"] <= 1e-10, worst
    assert worst["phi"] <= 1e-10 and worst["p"] <= 1e-9 and worst["padj"] <= 1e-9, worst
    if case["genes"] >= 16:
        assert n_asym >= 5  # the hot genes of the large pairs reach the asymptotic branch


def test_the_generator_carries_what_the_cases_need():
    for idx, (seed, genes, cells, n_cond) in enumerate(pref.CASES):
        case = pref.make_case(seed, genes, cells, n_cond)
        lab = case["labels"]
        cnt = np.bincount(lab[lab >= 0], minlength=case["n_groups"])
        assert np.sum(lab == -1) >= cells // 20 and cnt[0] == cells // 2 and cnt[-2] == 1 and cnt[-1] == 3
        assert case["mat"].shape == (genes, cells) and len(case["pairs"]) == n_cond + 2
        if genes >= 16:
            assert case["mat"][5].nnz == 0 and case["mat"][:5].mean() > 30
