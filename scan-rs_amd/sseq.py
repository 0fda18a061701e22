"""sSeq differential expression (diff-exp/src/diff_exp.rs, dist.rs; both NbExactBackends) over the count-matrix handle.

Rows of the handle are genes, columns are cells (the reference's feature x barcode matrix); a cell-major handle is used
through ``.t()``. DE reads the stored u32 counts and ignores the handle's map and offset. The passes over the nonzeros and
the tests run on the device through ``include/scanrs_amd.h``; the O(genes) finishing steps run in the library's host code.

``compute_sseq_params``, ``group_sums``, ``sseq_differential_expression``, ``sseq_de_one_vs_rest`` and ``sseq_de_vs_control`` also
take a ``MultiMat`` (or a sharded ``AdaptiveMat``) whose cells are the sharded dimension: a genes x cells CSC ``MultiMat``, or a
cells x genes CSR one with ``transposed=True``. All per-cell arguments then span the whole matrix and every result equals the
unsharded call bit for bit. ``sseq_de_pairs`` and ``sseq_de_each_vs_control`` take a ``MultiMat`` in the same way
(DESIGN.md §7i); on a sharded ``AdaptiveMat`` they stay refused, and ``sseq_de_pairs_sharded`` is the collective form every rank calls.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import AdaptiveMat, MultiMat, ScanrsError, _check, _lib, _p

BIG_COUNT_DEFAULT = 900  # diff_exp.rs:15
ZETA_QUINTILE_DEFAULT = 0.995  # diff_exp.rs:17
NB_EXACT_LOGSPACE = 0  # NbExactBackend::LogSpace (dist.rs:52-68), the default
NB_EXACT_RATIO = 1  # NbExactBackend::Ratio: nb_exact_test_ratio (dist.rs:116-215)

_u64, _f64c, _u32 = ctypes.c_uint64, ctypes.c_double, ctypes.c_uint32


@dataclass
class SSeqParams:
    """`SSeqParams` (diff_exp.rs:19-40)."""

    num_cells: int
    num_genes: int
    size_factors: np.ndarray
    gene_means: np.ndarray
    gene_variances: np.ndarray
    use_genes: np.ndarray
    gene_moment_phi: np.ndarray
    zeta_hat: float
    delta: float
    gene_phi: np.ndarray


@dataclass
class DiffExpResult:
    """`DiffExpResult` (diff_exp.rs:42-65)."""

    genes_tested: np.ndarray
    sums_in: np.ndarray
    sums_out: np.ndarray
    common_mean: np.ndarray
    common_dispersion: np.ndarray
    normalized_mean_in: np.ndarray
    normalized_mean_out: np.ndarray
    p_values: np.ndarray
    adjusted_p_values: np.ndarray
    log2_fold_change: np.ndarray


def _shape(mat, transposed: bool):
    """(genes, cells) of the WHOLE matrix: of a MultiMat (transposed: created cells x genes), of a handle, or of a sharded handle,
    whose own column count is its slice of the cells."""
    if isinstance(mat, MultiMat):
        return (mat.cols, mat.rows) if transposed else (mat.rows, mat.cols)
    if transposed:
        raise ScanrsError(6, "transposed is for a MultiMat; use .t() on an AdaptiveMat")
    genes, cells = mat.shape()
    # a sharded handle (set_shard*) whose outer vectors are the view's columns holds a slice of the cells; one sharded over the genes is
    # refused by the library
    if getattr(mat, "_outer_global", None) is not None and mat.storage() == 1:
        cells = mat._outer_global
    return genes, cells


def compute_sseq_params(mat, zeta_quintile: float = ZETA_QUINTILE_DEFAULT, cell_indices=None, umi_counts=None, transposed: bool = False) -> SSeqParams:
    """`compute_sseq_params` (diff_exp.rs:458-500). mat: an AdaptiveMat or a MultiMat (see the module's docstring)."""
    genes, cells = _shape(mat, transposed)
    ci = None if cell_indices is None else np.ascontiguousarray(cell_indices, dtype=np.uint64)
    n_sel = cells if ci is None else len(ci)
    um = None
    if umi_counts is not None:
        um = np.ascontiguousarray(umi_counts, dtype=np.float64)
        if len(um) != n_sel:
            raise ScanrsError(6, "umi_counts needs one value per selected cell")
    sf, mean, var, phi_mm, phi = (np.zeros(cells), np.zeros(genes), np.zeros(genes), np.zeros(genes), np.zeros(genes))
    use = np.zeros(genes, dtype=np.uint8)
    zh, dl = _f64c(), _f64c()
    args = (_f64c(zeta_quintile), _p(ci), _u64(0 if ci is None else len(ci)), _p(um), _p(sf), _p(mean), _p(var), _p(use), _p(phi_mm),
            ctypes.byref(zh), ctypes.byref(dl), _p(phi))
    if isinstance(mat, MultiMat):
        _check(_lib.scanrs_multi_sseq_params(mat._h, ctypes.c_int(int(transposed)), *args))
    else:
        _check(_lib.scanrs_sseq_params(mat._h, *args))
    return SSeqParams(n_sel, genes, sf, mean, var, use.astype(bool), phi_mm, zh.value, dl.value, phi)


def sseq_params_from_moments(mean_g, var_g, sum_size_factors: float, n_cells: float, n_genes: float, zeta_quintile: float) -> SSeqParams:
    """`sseq_params_from_moments` (diff_exp.rs:377-456); size_factors is left empty, as in the reference."""
    mean_g = np.ascontiguousarray(mean_g, dtype=np.float64)
    var_g = np.ascontiguousarray(var_g, dtype=np.float64)
    n = len(var_g)
    use, phi_mm, phi = np.zeros(n, dtype=np.uint8), np.zeros(n), np.zeros(n)
    zh, dl = _f64c(), _f64c()
    _check(_lib.scanrs_sseq_params_from_moments(_p(mean_g), _p(var_g), _u64(n), _f64c(sum_size_factors), _f64c(n_cells), _f64c(n_genes),
                                                _f64c(zeta_quintile), _p(use), _p(phi_mm), ctypes.byref(zh), ctypes.byref(dl), _p(phi)))
    return SSeqParams(int(n_cells), int(n_genes), np.zeros(0), mean_g.copy(), var_g.copy(), use.astype(bool), phi_mm, zh.value, dl.value, phi)


def _labels(labels, cells: int) -> np.ndarray:
    lab = np.asarray(labels)
    if lab.shape != (cells,):
        raise ScanrsError(6, f"labels need one entry per cell ({cells})")
    if lab.size and (lab.min() < -1 or lab.max() > np.iinfo(np.int16).max):
        raise ScanrsError(6, "labels must be -1 or a group number below 32768")
    return np.ascontiguousarray(lab, dtype=np.int16)


def group_sums(mat, labels, n_groups: int, transposed: bool = False):
    """Per (gene, group) u64 count sums in one pass over the nonzeros (sum_rows / sum_rows_dual, sqz/src/mat.rs:449-610,
    generalised to many groups) and the number of cells per group. labels: per cell, -1 = in no group."""
    genes, cells = _shape(mat, transposed)
    lab = _labels(labels, cells)
    sums = np.zeros((genes, n_groups), dtype=np.uint64)
    cnt = np.zeros(n_groups, dtype=np.uint64)
    if isinstance(mat, MultiMat):
        _check(_lib.scanrs_multi_group_sums(mat._h, ctypes.c_int(int(transposed)), _p(lab), _u32(n_groups), _p(sums), _p(cnt)))
    else:
        _check(_lib.scanrs_mat_group_sums(mat._h, _p(lab), _u32(n_groups), _p(sums), _p(cnt)))
    return sums, cnt


def _snoop_arg(snoop):
    if snoop is None:
        return None, None
    st = snoop._struct()
    return ctypes.byref(st), st


def _params_arrays(params: SSeqParams, genes: int):
    mean = np.ascontiguousarray(params.gene_means, dtype=np.float64)
    phi = np.ascontiguousarray(params.gene_phi, dtype=np.float64)
    use = np.ascontiguousarray(params.use_genes, dtype=np.uint8)
    if len(mean) != genes or len(phi) != genes or len(use) != genes:
        raise ScanrsError(6, "params do not match the number of genes")
    return mean, phi, use


def _results(params, sums_in, sums_out, p, padj, l2, mi, mo) -> List[DiffExpResult]:
    use = np.asarray(params.use_genes, dtype=bool)
    return [DiffExpResult(use.copy(), sums_in[:, j].copy(), sums_out[:, j].copy(), np.asarray(params.gene_means, dtype=np.float64).copy(),
                          np.asarray(params.gene_phi, dtype=np.float64).copy(), mi[:, j].copy(), mo[:, j].copy(), p[:, j].copy(), padj[:, j].copy(),
                          l2[:, j].copy()) for j in range(p.shape[1])]


def _backend(backend) -> int:
    if isinstance(backend, (bool, np.bool_)) or not isinstance(backend, (int, np.integer)) or int(backend) not in (NB_EXACT_LOGSPACE, NB_EXACT_RATIO):
        raise ScanrsError(6, "backend must be NB_EXACT_LOGSPACE (0) or NB_EXACT_RATIO (1)")
    return int(backend)


def _de_matrix(mat, labels, n_groups, mode, params, big_count, snoop, backend=NB_EXACT_LOGSPACE, transposed=False):
    genes, cells = _shape(mat, transposed)
    lab = _labels(labels, cells)
    mean, phi, use = _params_arrays(params, genes)
    sf = np.ascontiguousarray(params.size_factors, dtype=np.float64)
    if len(sf) != cells:
        raise ScanrsError(6, "params.size_factors needs one value per cell of the matrix")
    t = n_groups if mode == 0 else 1 if mode == 1 else max(n_groups - 1, 0)
    si, so = np.zeros((genes, t), dtype=np.uint64), np.zeros((genes, t), dtype=np.uint64)
    p, padj, l2, mi, mo = (np.zeros((genes, t)) for _ in range(5))
    sn, _keep = _snoop_arg(snoop)
    bc = BIG_COUNT_DEFAULT if big_count is None else int(big_count)
    args = (_p(lab), _u32(n_groups), ctypes.c_int(mode), _p(sf), _p(mean), _p(phi), _p(use), _u64(bc), ctypes.c_int(_backend(backend)), sn, _p(si),
            _p(so), _p(p), _p(padj), _p(l2), _p(mi), _p(mo))
    if isinstance(mat, MultiMat):
        _check(_lib.scanrs_multi_sseq_de(mat._h, ctypes.c_int(int(transposed)), *args))
    else:
        _check(_lib.scanrs_sseq_de_backend(mat._h, *args))
    return _results(params, si, so, p, padj, l2, mi, mo)


def _index_list(v, cells: int, name: str) -> np.ndarray:
    a = np.asarray(v, dtype=np.int64)
    if a.ndim != 1:
        raise ScanrsError(6, f"{name} must be a 1-d list of cell indices")
    if a.size and (a.min() < 0 or a.max() >= cells):
        raise ScanrsError(6, f"{name} holds a cell index outside 0 .. {cells - 1}")
    if a.size > 1 and not np.all(np.diff(a) > 0):
        raise ScanrsError(6, f"{name} must be sorted ascending without duplicates")
    return a


def sseq_differential_expression(mat, cond_a: Sequence[int], cond_b: Sequence[int], params: SSeqParams, big_count: Optional[int] = None,
                                 snoop=None, backend: int = NB_EXACT_LOGSPACE, transposed: bool = False) -> DiffExpResult:
    """`sseq_differential_expression` (diff_exp.rs:68-175): cells of cond_a against cells of cond_b. The lists must be sorted,
    free of duplicates and disjoint (the reference assumes sorted lists without checking). backend: the exact test's kernel
    (`sseq_differential_expression_backend`, diff_exp.rs:125-161)."""
    genes, cells = _shape(mat, transposed)
    a, b = _index_list(cond_a, cells, "cond_a"), _index_list(cond_b, cells, "cond_b")
    if np.intersect1d(a, b).size:
        raise ScanrsError(6, "cond_a and cond_b overlap")
    lab = np.full(cells, -1, dtype=np.int16)
    lab[a], lab[b] = 0, 1
    return _de_matrix(mat, lab, 2, 1, params, big_count, snoop, backend, transposed)[0]


def sseq_de_one_vs_rest(mat, labels, params: SSeqParams, big_count: Optional[int] = None, n_groups: Optional[int] = None,
                        snoop=None, backend: int = NB_EXACT_LOGSPACE, transposed: bool = False) -> List[DiffExpResult]:
    """Every group against all other labelled cells (Cell Ranger's per-cluster DE over `initial_cluster_assignments`,
    diff-exp/src/utils.rs:77-117). labels: per cell, the group 0 .. n_groups - 1 or -1 (in no group)."""
    lab = np.asarray(labels)
    if n_groups is None:
        n_groups = int(lab.max()) + 1 if lab.size else 0
    return _de_matrix(mat, lab, n_groups, 0, params, big_count, snoop, backend, transposed)


def sseq_de_vs_control(mat, labels, params: SSeqParams, control: int = 0, big_count: Optional[int] = None,
                       n_groups: Optional[int] = None, snoop=None, backend: int = NB_EXACT_LOGSPACE, transposed: bool = False) -> List[DiffExpResult]:
    """Every other group against the group `control` (the shared-control shape of Cell Ranger's batched DE): one pass over the
    nonzeros, the control's sums and size factor computed once. Returns one DiffExpResult per group other than the control, in
    group order; each equals `sseq_differential_expression(mat, cells of the group, cells of the control, ...)` bit for bit.
    labels: per cell, the group 0 .. n_groups - 1 or -1 (in no group)."""
    lab = np.asarray(labels)
    if n_groups is None:
        n_groups = int(lab.max()) + 1 if lab.size else 0
    if not 0 <= int(control) < n_groups:
        raise ScanrsError(6, f"control must be a group 0 .. {n_groups - 1}")
    if control != 0:
        # the library tests against group 0: the control becomes group 0 and the groups below it move up by one
        lab = np.where(lab == control, 0, np.where((lab >= 0) & (lab < control), lab + 1, lab))
    return _de_matrix(mat, lab, n_groups, 2, params, big_count, snoop, backend, transposed)


class _PairParams(ctypes.Structure):
    """`scanrs_sseq_pair_params` (include/scanrs_amd.h)."""

    _fields_ = [(n, ctypes.c_void_p) for n in ("gene_means", "gene_variances", "gene_moment_phi", "gene_phi", "use_genes", "zeta_hat", "delta", "sf_a",
                                               "sf_b", "median_total", "sum_size_factors", "n_cells_a", "n_cells_b", "literal")]


def sseq_de_pairs(mat, labels, pairs, zeta_quintile: float = ZETA_QUINTILE_DEFAULT, big_count: Optional[int] = None,
                  n_groups: Optional[int] = None, backend: int = NB_EXACT_LOGSPACE, snoop=None, transposed: bool = False):
    """Batched pairwise DE with per-pair parameters: for every (a, b) of `pairs`, `compute_sseq_params(mat, zeta_quintile, cells of
    a ∪ b)` (diff_exp.rs:458-490) and then the cells of group a against those of group b (diff_exp.rs:125-161), as merge_clusters.rs
    runs its candidates and as diff_exp.rs:361-376 describes the shared-control batched path. All pairs share two passes over the
    nonzeros; each pair's parameters are combined on the device from its two groups' integer sums. Returns
    `(List[DiffExpResult], List[SSeqParams])`, one of each per pair; `size_factors` is left empty, as in
    `sseq_params_from_moments`, and the pair's scalars are attached to its params: `size_factor_a`, `size_factor_b`,
    `median_total`, `sum_size_factors`, `num_cells_a`, `num_cells_b`, `literal` (the union's median total was 0, or it holds a cell total too
    large for the call's shared fixed-point quantum, and the pair ran the two reference calls themselves). labels: per cell, the group 0 .. n_groups - 1 or -1 (in no group).
    mat: an AdaptiveMat, or a MultiMat whose cells are the sharded dimension (`transposed=True` for one created cells x genes): labels
    then span the whole matrix and every output equals the unsharded call's bit for bit. A sharded AdaptiveMat is
    refused; `sseq_de_pairs_sharded` is the collective form for one."""
    return _de_pairs(mat, labels, pairs, zeta_quintile, big_count, n_groups, backend, snoop, transposed, False)


def sseq_de_pairs_sharded(mat: AdaptiveMat, labels, pairs, zeta_quintile: float = ZETA_QUINTILE_DEFAULT, big_count: Optional[int] = None,
                          n_groups: Optional[int] = None, backend: int = NB_EXACT_LOGSPACE, snoop=None):
    """`sseq_de_pairs` on one sharded handle (set_shard with a host hook, or set_shard_comm): COLLECTIVE, every rank calls it with the same
    arguments; labels span the whole matrix and every rank gets the complete results. On an unsharded handle it is `sseq_de_pairs`."""
    return _de_pairs(mat, labels, pairs, zeta_quintile, big_count, n_groups, backend, snoop, False, True)


def _de_pairs(mat, labels, pairs, zeta_quintile, big_count, n_groups, backend, snoop, transposed, collective):
    if isinstance(mat, MultiMat) or collective:
        genes, cells = _shape(mat, transposed)
    else:
        if transposed:
            raise ScanrsError(6, "transposed is for a MultiMat; use .t() on an AdaptiveMat")
        genes, cells = mat.shape()
    lab = _labels(labels, cells)
    if n_groups is None:
        n_groups = int(lab.max()) + 1 if lab.size else 0
    pr = np.asarray(pairs, dtype=np.int64)
    if pr.size == 0:
        pr = pr.reshape(0, 2)
    if pr.ndim != 2 or pr.shape[1] != 2:
        raise ScanrsError(6, "pairs must be a list of (group a, group b)")
    if pr.size and (pr.min() < 0 or pr.max() > 0xFFFFFFFF):
        raise ScanrsError(6, "pairs hold a group number outside 0 .. n_groups - 1")
    pa, pb = np.ascontiguousarray(pr[:, 0], dtype=np.uint32), np.ascontiguousarray(pr[:, 1], dtype=np.uint32)
    t = len(pa)
    si, so = np.zeros((genes, t), dtype=np.uint64), np.zeros((genes, t), dtype=np.uint64)
    p, padj, l2, mi, mo, mean, var, phi_mm, phi = (np.zeros((genes, t)) for _ in range(9))
    use, lit = np.zeros((genes, t), dtype=np.uint8), np.zeros(t, dtype=np.uint8)
    zh, dl, fa, fb, med, ssf = (np.zeros(t) for _ in range(6))
    na, nb = np.zeros(t, dtype=np.uint64), np.zeros(t, dtype=np.uint64)
    pp = _PairParams(*(a.ctypes.data for a in (mean, var, phi_mm, phi, use, zh, dl, fa, fb, med, ssf, na, nb, lit)))
    sn, _keep = _snoop_arg(snoop)
    bc = BIG_COUNT_DEFAULT if big_count is None else int(big_count)
    args = (_p(lab), _u32(n_groups), _p(pa), _p(pb), _u32(t), _f64c(zeta_quintile), _u64(bc), ctypes.c_int(_backend(backend)), sn, _p(si), _p(so),
            _p(p), _p(padj), _p(l2), _p(mi), _p(mo), ctypes.byref(pp))
    if isinstance(mat, MultiMat):
        _check(_lib.scanrs_multi_sseq_de_pairs(mat._h, ctypes.c_int(int(transposed)), *args))
    elif collective:
        _check(_lib.scanrs_sseq_de_pairs_sharded(mat._h, *args))
    else:
        _check(_lib.scanrs_sseq_de_pairs(mat._h, *args))
    results, params = [], []
    for j in range(t):
        prm = SSeqParams(int(na[j] + nb[j]), genes, np.zeros(0), mean[:, j].copy(), var[:, j].copy(), use[:, j].astype(bool), phi_mm[:, j].copy(),
                         float(zh[j]), float(dl[j]), phi[:, j].copy())
        prm.size_factor_a, prm.size_factor_b = float(fa[j]), float(fb[j])
        prm.median_total, prm.sum_size_factors = float(med[j]), float(ssf[j])
        prm.num_cells_a, prm.num_cells_b, prm.literal = int(na[j]), int(nb[j]), bool(lit[j])
        params.append(prm)
        results.append(DiffExpResult(prm.use_genes.copy(), si[:, j].copy(), so[:, j].copy(), prm.gene_means.copy(), prm.gene_phi.copy(), mi[:, j].copy(),
                                     mo[:, j].copy(), p[:, j].copy(), padj[:, j].copy(), l2[:, j].copy()))
    return results, params


def sseq_de_each_vs_control(mat, labels, control: int = 0, zeta_quintile: float = ZETA_QUINTILE_DEFAULT, big_count: Optional[int] = None,
                            n_groups: Optional[int] = None, backend: int = NB_EXACT_LOGSPACE, snoop=None, transposed: bool = False):
    """Every other group against the group `control`, each test with the parameters of its own union (`sseq_de_pairs` over the
    pairs (g, control), g ascending). Returns `(List[DiffExpResult], List[SSeqParams])`, one per group other than the control.
    mat: an AdaptiveMat or a MultiMat, as for `sseq_de_pairs`."""
    lab = np.asarray(labels)
    if n_groups is None:
        n_groups = int(lab.max()) + 1 if lab.size else 0
    if not 0 <= int(control) < n_groups:
        raise ScanrsError(6, f"control must be a group 0 .. {n_groups - 1}")
    pairs = [(g, int(control)) for g in range(n_groups) if g != int(control)]
    return sseq_de_pairs(mat, lab, pairs, zeta_quintile, big_count, n_groups, backend, snoop, transposed)


def host_union_median(a, b) -> float:
    """`percentile_of_sorted(.., 50)` (stat.rs:140-162) of the union of two ascending lists, from the two ranks it reads."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    out = _f64c()
    _check(_lib.scanrs_host_union_median(_p(a) if len(a) else None, _u64(len(a)), _p(b) if len(b) else None, _u64(len(b)), ctypes.byref(out)))
    return out.value


def sseq_de_from_sums(feature_sums_a, feature_sums_b, size_factor_a, size_factor_b, params: SSeqParams, big_count: Optional[int] = None,
                      snoop=None, backend: int = NB_EXACT_LOGSPACE):
    """`sseq_de_from_sums` (diff_exp.rs:177-300) on the device. 1-d sums with scalar size factors give one DiffExpResult;
    2-d (genes x tests) sums with one size factor per test give a list. backend: the exact test's kernel; Cell Ranger's
    batched path passes NB_EXACT_RATIO (diff_exp.rs:172-175)."""
    sa, sb = np.asarray(feature_sums_a, dtype=np.uint64), np.asarray(feature_sums_b, dtype=np.uint64)
    single = sa.ndim == 1
    sa, sb = np.ascontiguousarray(sa.reshape(len(sa), -1)), np.ascontiguousarray(sb.reshape(len(sb), -1))
    if sa.shape != sb.shape:
        raise ScanrsError(6, "feature_sums_a and feature_sums_b differ in shape")
    genes, t = sa.shape
    fa = np.ascontiguousarray(np.atleast_1d(size_factor_a), dtype=np.float64)
    fb = np.ascontiguousarray(np.atleast_1d(size_factor_b), dtype=np.float64)
    if len(fa) != t or len(fb) != t:
        raise ScanrsError(6, "one size factor per test and side")
    mean, phi, use = _params_arrays(params, genes)
    p, padj, l2, mi, mo = (np.zeros((genes, t)) for _ in range(5))
    sn, _keep = _snoop_arg(snoop)
    bc = BIG_COUNT_DEFAULT if big_count is None else int(big_count)
    _check(_lib.scanrs_sseq_de_from_sums_backend(_u64(genes), _u32(t), _p(sa), _p(sb), _p(fa), _p(fb), _p(mean), _p(phi), _p(use), _u64(bc),
                                                 ctypes.c_int(_backend(backend)), sn, _p(p), _p(padj), _p(l2), _p(mi), _p(mo)))
    res = _results(params, sa, sb, p, padj, l2, mi, mo)
    return res[0] if single else res


def diff_exp_table(results: Sequence[DiffExpResult]) -> np.ndarray:
    """genes x 3 C table [mean_in, log2fc, p_adj] per cluster (utils.rs:158-205), the layout
    `hdf5_io.get_differential_expression` reads."""
    if not results:
        return np.zeros((0, 0))
    return np.stack([np.column_stack([r.normalized_mean_in, r.log2_fold_change, r.adjusted_p_values]) for r in results], axis=1).reshape(
        len(results[0].p_values), 3 * len(results))


def labels_from_clustering(clusters) -> np.ndarray:
    """`hdf5_io.get_clustering`'s 1-based cluster numbers as labels (v - 1, utils.rs:88-90): 0 becomes -1 (in no group)."""
    return (np.asarray(clusters, dtype=np.int32) - 1).astype(np.int16)


# ---- the shared math on the host (the kernels run the same special functions) ----------------------------------------------
def host_nb_exact_test(x_a, x_b, size_factor_a, size_factor_b, mu, phi) -> float:
    out = _f64c()
    _check(_lib.scanrs_host_nb_exact_test(_u64(x_a), _u64(x_b), _f64c(size_factor_a), _f64c(size_factor_b), _f64c(mu), _f64c(phi), ctypes.byref(out)))
    return out.value


def host_nb_exact_test_ratio(x_a, x_b, size_factor_a, size_factor_b, mu, phi) -> float:
    """`nb_exact_test_ratio` (dist.rs:155-215) on the host, line for line."""
    out = _f64c()
    _check(_lib.scanrs_host_nb_exact_test_ratio(_u64(x_a), _u64(x_b), _f64c(size_factor_a), _f64c(size_factor_b), _f64c(mu), _f64c(phi),
                                                ctypes.byref(out)))
    return out.value


def host_nb_exact_ratio_step(k, n, sa_r, sb_r) -> float:
    """`nb_exact_ratio_step` (dist.rs:124-126)."""
    out = _f64c()
    _check(_lib.scanrs_host_nb_exact_ratio_step(_f64c(k), _f64c(n), _f64c(sa_r), _f64c(sb_r), ctypes.byref(out)))
    return out.value


def host_nb_asymptotic_test(x_a, x_b, size_factor_a, size_factor_b, mu, phi) -> float:
    out = _f64c()
    _check(_lib.scanrs_host_nb_asymptotic_test(_u64(x_a), _u64(x_b), _f64c(size_factor_a), _f64c(size_factor_b), _f64c(mu), _f64c(phi),
                                               ctypes.byref(out)))
    return out.value


def host_log_prob_all(count, sa, sb, mu, r) -> np.ndarray:
    out = np.zeros(int(count) + 1)
    _check(_lib.scanrs_host_nb_log_prob_all(_u64(count), _f64c(sa), _f64c(sb), _f64c(mu), _f64c(r), _p(out)))
    return out


def host_adjusted_pvalue_bh(p) -> np.ndarray:
    p = np.ascontiguousarray(p, dtype=np.float64)
    out = np.zeros_like(p)
    _check(_lib.scanrs_host_adjusted_pvalue_bh(_p(p), _u64(len(p)), _p(out)))
    return out


def host_betainc(a, b, x) -> float:
    out = _f64c()
    _check(_lib.scanrs_host_betainc(_f64c(a), _f64c(b), _f64c(x), ctypes.byref(out)))
    return out.value


def host_betaincinv(a, b, p) -> float:
    out = _f64c()
    _check(_lib.scanrs_host_betaincinv(_f64c(a), _f64c(b), _f64c(p), ctypes.byref(out)))
    return out.value
