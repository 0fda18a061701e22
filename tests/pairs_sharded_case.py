"""The seeded fixture of the sharded sseq_de_pairs tests (tests/test_gpu_sseq_pairs_sharded.py, tests/test_pairs_sharded_cpu.py), a
restatement of the limb scheme that carries the 128-bit accumulators through a u64 sum (scan-rs_amd/csrc/sseq_pairs.hip), and the
comparison helpers of tests/test_gpu_sseq_pairs.py at its bounds.

The fixture is `sseq_pairs_ref.make_case(14, 65, 1200, 7)` (65 genes x 1 200 cells, a control of half the cells, seven conditions)
with these additions, each of which a cut of the cells over shards has to get right:
  * a block of cells around the second fifth of the matrix is in no group: at five shards one shard holds no labelled cell (the two
    tiny groups of make_case keep their sizes: a member inside the block trades places with a control cell outside it);
  * 32 cells are appended: 24 empty cells and 4 ordinary ones form group EMPTYISH, the last 4 cells form group SMALL. The union of the
    two has a median total of 0 (the literal route), and SMALL lies inside the last shard of any cut;
  * group NOBODY has no cell; the pair (NOBODY, 1) has one empty side."""
import os
import sys

import numpy as np
from scipy import sparse

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import sseq_pairs_ref as pref  # noqa: E402
import sseq_ratio_ref as rref  # noqa: E402
import sseq_ref as ref  # noqa: E402

BASE = (14, 65, 1200, 7)
N_EMPTY, N_EMPTYISH_FULL, N_SMALL = 24, 4, 4
UNLABELLED_BLOCK = (0.17, 0.43)  # as fractions of the base cells: covers the second of five nonzero-balanced shards with room to spare
SHARDS = (1, 2, 3, 5)
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1


def make_case():
    base = pref.make_case(*BASE)
    rng = np.random.default_rng(BASE[0] + 1000)
    genes, c0 = base["genes"], base["cells"]
    n0 = base["n_groups"]
    emptyish, small, nobody = n0, n0 + 1, n0 + 2
    labels = base["labels"].copy()
    lo, hi = int(UNLABELLED_BLOCK[0] * c0), int(UNLABELLED_BLOCK[1] * c0)
    outside_control = [c for c in np.flatnonzero(labels == 0) if not lo <= c < hi]
    for c in range(lo, hi):
        if labels[c] in (n0 - 2, n0 - 1):  # the singleton and the 3-cell condition stay whole
            labels[outside_control.pop()] = labels[c]
        labels[c] = -1
    dense = base["mat"].toarray()
    extra = np.zeros((genes, N_EMPTY + N_EMPTYISH_FULL + N_SMALL), dtype=np.uint32)
    extra[:, N_EMPTY:] = rng.poisson(3.0, (genes, N_EMPTYISH_FULL + N_SMALL))
    mat = sparse.csr_matrix(np.hstack([dense, extra]).astype(np.uint32))
    labels = np.concatenate([labels, np.full(N_EMPTY + N_EMPTYISH_FULL, emptyish), np.full(N_SMALL, small)]).astype(np.int16)
    pairs = base["pairs"] + [(emptyish, small), (nobody, 1), (small, 0)]
    return dict(mat=mat, labels=labels, n_groups=n0 + 3, pairs=pairs, genes=genes, cells=mat.shape[1], literal_pair=(emptyish, small),
                empty_group=nobody, one_shard_group=small, unlabelled_block=(lo, hi))


def cell_ranges(cells, world):
    """`world` equal ranges of the cells."""
    return [(cells * r // world, cells * (r + 1) // world) for r in range(world)]


def partial_sums(case, ranges):
    """One GroupSums per range: what a rank holding those cells accumulates. The quantum comes from the GLOBAL cell count, as the
    library takes it (GroupSums derives it from the matrix's shape, which stays whole here: the other cells are unlabelled)."""
    out = []
    for lo, hi in ranges:
        lab = np.full(case["cells"], -1, dtype=np.int16)
        lab[lo:hi] = case["labels"][lo:hi]
        out.append(pref.GroupSums(case["mat"], lab, case["n_groups"]))
    return out


# ---- the limb scheme of pairs_acc_split_kernel / pairs_acc_join_kernel ---------------------------------------------------------------
def limb_split(v):
    """A 128-bit sum as the three u64 words a rank contributes: the two 32-bit halves of its low word, and its high word."""
    lo, hi = v & M64, v >> 64
    return [lo & M32, lo >> 32, hi]


def limb_join(words):
    """The all-reduced words (plain u64 sums over the ranks, which must not have wrapped) back to (lo, hi)."""
    assert all(0 <= w <= M64 for w in words)
    c = (words[0] >> 32) + words[1]
    assert c <= M64
    lo = (words[0] & M32) | ((c & M32) << 32)
    hi = (words[2] + (c >> 32)) & M64
    return lo, hi


# ---- the comparisons of tests/test_gpu_sseq_pairs.py, at its bounds -------------------------------------------------------------------
RESULT_FIELDS = ("sums_in", "sums_out", "p_values", "adjusted_p_values", "log2_fold_change", "normalized_mean_in", "normalized_mean_out",
                 "genes_tested", "common_mean", "common_dispersion")
PARAM_FIELDS = ("gene_means", "gene_variances", "gene_moment_phi", "gene_phi", "use_genes")
PARAM_SCALARS = ("zeta_hat", "delta", "median_total", "sum_size_factors", "num_cells", "num_cells_a", "num_cells_b", "size_factor_a",
                 "size_factor_b", "literal", "num_genes")


def as_arrays(results, params):
    """Every field of the results and of the per-pair parameters as one dict of arrays."""
    out = {}
    for j, (r, q) in enumerate(zip(results, params)):
        for f in RESULT_FIELDS:
            out[f"pair{j}.result.{f}"] = np.asarray(getattr(r, f))
        for f in PARAM_FIELDS:
            out[f"pair{j}.params.{f}"] = np.asarray(getattr(q, f))
        out[f"pair{j}.params.scalars"] = np.array([float(getattr(q, f)) for f in PARAM_SCALARS], dtype=np.float64)
        out[f"pair{j}.params.size_factors"] = np.asarray(q.size_factors)
    return out


def assert_same_bits(got, exp):
    assert got.keys() == exp.keys()
    for k in exp:
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, k
        assert np.array_equal(got[k], exp[k], equal_nan=got[k].dtype.kind == "f"), k


def _close(got, exp, rtol, what):
    np.testing.assert_allclose(got, exp, rtol=rtol, atol=0, err_msg=what)


def assert_params(q, e, what, phi_scale=None):
    np.testing.assert_array_equal(q.use_genes, e["use_genes"], err_msg=what)
    _close(q.gene_means, e["gene_means"], 1e-12, what + " means")
    _close(q.gene_variances, e["gene_variances"], 1e-10, what + " variances")
    _close([q.zeta_hat, q.delta], [e["zeta_hat"], e["delta"]], 1e-10, what + " zeta_hat, delta")
    d = np.abs(q.gene_phi - e["gene_phi"])
    np.testing.assert_array_equal(np.isnan(q.gene_phi), np.isnan(e["gene_phi"]), err_msg=what)
    scale = e["zeta_hat"] if phi_scale is None else phi_scale
    assert np.all(np.where(np.isnan(d), 0.0, d) <= 1e-10 * scale), (what, float(np.nanmax(d)), scale)
    assert len(q.size_factors) == 0


def assert_result(r, q, e, backend, what, same_size_factors):
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
    np.testing.assert_allclose(r.adjusted_p_values[use], ref.adjusted_pvalue_bh(p[use]), rtol=1e-12, atol=0, err_msg=what)
    np.testing.assert_array_equal(np.delete(r.adjusted_p_values, use), np.delete(p, use), err_msg=what)
    if not len(off):
        _close(r.adjusted_p_values, e["adjusted_p_values"], 1e-9, what + " adjusted p")
    return len(off)
