"""merge_clusters (scan-rs/src/merge_clusters.rs) and what it is made of: pdist and complete linkage (linkage.rs), the cluster
medoids (`medioids`, with `median_mut` of stats.rs) and relabel_by_size.

Labels are int16 values 0 .. K-1 with every value present, K <= 8192. The scores are cells x d f64: a numpy array or the
`PcaResultDevice` of a handle's last PCA (its `v` stays in device memory). pdist, linkage and relabel_by_size run on the host;
the medoids and the merge's passes and tests run on the device through ``include/scanrs_amd.h``.

``merge_clusters`` and ``cluster_medoids`` also take a ``MultiMat`` whose cells are the sharded dimension (``transposed=True`` for one
created cells x genes): labels and scores then span the whole matrix and the results equal the unsharded call's bit for bit (DESIGN.md
§7i). ``merge_clusters_sharded`` and ``cluster_medoids_sharded`` are the collective forms on one sharded handle.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import AdaptiveMat, MultiMat, PcaResultDevice, ScanrsError, _check, _lib, _p

_u64, _u32 = ctypes.c_uint64, ctypes.c_uint32


class _MergeTrace(ctypes.Structure):
    _fields_ = [
        ("capacity", ctypes.c_uint64),
        ("leaf0", ctypes.c_void_p),
        ("leaf1", ctypes.c_void_p),
        ("n_de", ctypes.c_void_p),
        ("min_p_adj", ctypes.c_void_p),
        ("n_candidates", ctypes.c_uint64),
        ("n_rounds", ctypes.c_uint64),
        ("n_merges", ctypes.c_uint64),
        ("n_passes", ctypes.c_uint64),
    ]


@dataclass
class MergeTrace:
    """What merge_clusters evaluated, in the reference's order: per candidate the two leaves (labels of that round), the number
    of genes with adjusted p < 0.05 and the smallest adjusted p; totals of candidates, rounds and merges; passes over the
    nonzeros."""

    leaf0: np.ndarray
    leaf1: np.ndarray
    n_de: np.ndarray
    min_p_adj: np.ndarray
    n_candidates: int = 0
    n_rounds: int = 0
    n_merges: int = 0
    n_passes: int = 0
    entries: List[tuple] = field(default_factory=list)


def _points(x) -> np.ndarray:
    x = np.ascontiguousarray(np.atleast_2d(np.asarray(x, dtype=np.float64)))
    if x.ndim != 2:
        raise ScanrsError(6, "points must be a 2-d array")
    return x


def pdist(x) -> np.ndarray:
    """`pdist` (linkage.rs:14-26): the m (m - 1) / 2 Euclidean distances of the rows, pairs (i, j > i) in row order."""
    x = _points(x)
    m, d = x.shape
    out = np.zeros(m * (m - 1) // 2)
    _check(_lib.scanrs_host_pdist(_p(x), _u64(m), _u32(d), _p(out)))
    return out


def linkage(x) -> np.ndarray:
    """`linkage(x, &Complete)` (linkage.rs:43-158): (m - 1) x 4 [a, b, distance, size], rows by (distance, row)."""
    x = _points(x)
    m, d = x.shape
    if m == 0:
        raise ScanrsError(6, "linkage of no points")
    z = np.zeros((m - 1, 4))
    _check(_lib.scanrs_host_linkage_complete(_p(x), _u64(m), _u32(d), _p(z)))
    return z


def relabel_by_size(labels) -> np.ndarray:
    """`relabel_by_size` (merge_clusters.rs:43-56): labels ordered by count, largest first; equal counts in label order."""
    lab = np.asarray(labels)
    if lab.size and (lab.min() < np.iinfo(np.int16).min or lab.max() > np.iinfo(np.int16).max):
        raise ScanrsError(6, "labels must be int16 values")
    lab = np.ascontiguousarray(lab, dtype=np.int16).ravel()
    out = np.zeros_like(lab)
    _check(_lib.scanrs_host_relabel_by_size(_p(lab), _u64(len(lab)), _p(out)))
    return out


def _labels(labels, n: int) -> np.ndarray:
    lab = np.asarray(labels)
    if lab.ndim != 1 or len(lab) != n:
        raise ScanrsError(6, f"labels need one entry per cell ({n}), got {lab.shape}")
    if lab.size and (lab.min() < np.iinfo(np.int16).min or lab.max() > np.iinfo(np.int16).max):
        raise ScanrsError(6, "labels must be int16 values")
    return np.ascontiguousarray(lab, dtype=np.int16)


def _scores(pca):
    """(pointer, on device, n, ld, d, keep-alive) of a numpy array or a PcaResultDevice (its v: cells x k)."""
    if isinstance(pca, PcaResultDevice):
        return ctypes.c_void_p(pca.d_v), 1, pca.cols, pca.ld_v, pca.k, pca
    a = np.asarray(pca, dtype=np.float64)
    if a.ndim != 2:
        raise ScanrsError(6, "the scores must be a cells x d array")
    a = np.ascontiguousarray(a)
    return ctypes.c_void_p(a.ctypes.data), 0, a.shape[0], a.shape[1], a.shape[1], a


def medioids(pca, labels, n_clusters: Optional[int] = None) -> np.ndarray:
    """`medioids` (merge_clusters.rs:20-40): K x d, row i the per-column median of the scores of the cells labelled i."""
    ptr, on_dev, n, ld, d, keep = _scores(pca)
    lab = _labels(labels, n)
    k = int(lab.max()) + 1 if n_clusters is None and lab.size else int(n_clusters or 0)
    out = np.zeros((k, d))
    fn = _lib.scanrs_cluster_medoids_device if on_dev else _lib.scanrs_cluster_medoids
    _check(fn(ptr, _u64(n), _u32(ld), _u32(d), _p(lab), _u32(k), _p(out)))
    del keep
    return out


def _cells(mat, transposed: bool, collective: bool):
    """(cells of the WHOLE matrix, cells this handle holds)."""
    if isinstance(mat, MultiMat):
        n = mat.rows if transposed else mat.cols
        return n, n
    if transposed:
        raise ScanrsError(6, "transposed is for a MultiMat; use .t() on an AdaptiveMat")
    local = mat.shape()[1]
    if collective and getattr(mat, "_outer_global", None) is not None and mat.storage() == 1:
        return mat._outer_global, local
    return local, local


def cluster_medoids(mat, pca, labels, n_clusters: Optional[int] = None, transposed: bool = False) -> np.ndarray:
    """`medioids` over the cells of a matrix: mat is an AdaptiveMat (then this is `medioids(pca, labels)`) or a MultiMat, whose shards
    each key their own cells' scores and select the medians by exchanging integer histograms. pca: a cells x d host array
    over all cells."""
    if not isinstance(mat, MultiMat):
        if transposed:
            raise ScanrsError(6, "transposed is for a MultiMat; use .t() on an AdaptiveMat")
        return medioids(pca, labels, n_clusters)
    return _medoids_on(mat, pca, labels, n_clusters, transposed, False)


def cluster_medoids_sharded(mat: AdaptiveMat, pca, labels, n_clusters: Optional[int] = None) -> np.ndarray:
    """`cluster_medoids` on one sharded handle: COLLECTIVE, every rank calls it with the same labels (over the whole matrix). pca: a host
    array over all cells, or a PcaResultDevice holding the rank's own cells."""
    return _medoids_on(mat, pca, labels, n_clusters, False, True)


def _medoids_on(mat, pca, labels, n_clusters, transposed, collective):
    cells, local = _cells(mat, transposed, collective)
    ptr, on_dev, n, ld, d, keep = _scores(pca)
    if n != (local if on_dev else cells):
        raise ScanrsError(6, f"the scores have {n} rows for {local if on_dev else cells} cells")
    lab = _labels(labels, cells)
    k = int(lab.max()) + 1 if n_clusters is None and lab.size else int(n_clusters or 0)
    out = np.zeros((k, d))
    if isinstance(mat, MultiMat):
        if on_dev:
            raise ScanrsError(6, "a MultiMat takes the scores as a host array over all cells")
        _check(_lib.scanrs_multi_cluster_medoids(mat._h, ctypes.c_int(int(transposed)), ptr, _u32(ld), _u32(d), _p(lab), _u32(k), _p(out)))
    else:
        _check(_lib.scanrs_cluster_medoids_sharded(mat._h, ptr, ctypes.c_int(on_dev), _u32(ld), _u32(d), _p(lab), _u32(k), _p(out)))
    del keep
    return out


def merge_clusters(mat, pca, labels, trace: bool = False, snoop=None, capacity: int = 4096, transposed: bool = False):
    """`merge_clusters(fbm, pca, labels)` (merge_clusters.rs:59-138). Rows of `mat` are genes, columns are cells; pca is a
    cells x d array or a PcaResultDevice. Returns the merged labels (relabel_by_size), and with trace=True also a MergeTrace
    (at most `capacity` entries are kept; the totals count all). mat: an AdaptiveMat, or a MultiMat whose cells are the sharded
    dimension (`transposed=True` for one created cells x genes; pca then is a host array over all cells); a sharded AdaptiveMat is
    refused, `merge_clusters_sharded` is the collective form for one."""
    return _merge(mat, pca, labels, trace, snoop, capacity, transposed, False)


def merge_clusters_sharded(mat: AdaptiveMat, pca, labels, trace: bool = False, snoop=None, capacity: int = 4096):
    """`merge_clusters` on one sharded handle: COLLECTIVE, every rank calls it with the same labels (over the whole matrix). pca: a host
    array over all cells, or a PcaResultDevice holding the rank's own cells. Every rank gets the complete labels and trace."""
    return _merge(mat, pca, labels, trace, snoop, capacity, False, True)


def _merge(mat, pca, labels, trace, snoop, capacity, transposed, collective):
    cells, local = _cells(mat, transposed, collective)
    ptr, on_dev, n, ld, d, keep = _scores(pca)
    if n != (local if on_dev else cells):
        raise ScanrsError(6, f"the scores have {n} rows for {local if on_dev else cells} cells")
    if isinstance(mat, MultiMat) and on_dev:
        raise ScanrsError(6, "a MultiMat takes the scores as a host array over all cells")
    lab = _labels(labels, cells)
    out = np.zeros(cells, dtype=np.int16)
    tr, st = None, None
    if trace:
        cap = int(capacity)
        tr = MergeTrace(np.zeros(cap, dtype=np.int16), np.zeros(cap, dtype=np.int16), np.zeros(cap, dtype=np.uint64), np.zeros(cap))
        st = _MergeTrace(cap, tr.leaf0.ctypes.data, tr.leaf1.ctypes.data, tr.n_de.ctypes.data, tr.min_p_adj.ctypes.data, 0, 0, 0, 0)
    sn_keep = None if snoop is None else snoop._struct()
    sn = None if sn_keep is None else ctypes.byref(sn_keep)
    tail = (_u32(ld), _u32(d), _p(lab), _p(out), sn, None if st is None else ctypes.byref(st))
    if isinstance(mat, MultiMat):
        _check(_lib.scanrs_multi_merge_clusters(mat._h, ctypes.c_int(int(transposed)), ptr, *tail))
    elif collective:
        _check(_lib.scanrs_merge_clusters_sharded(mat._h, ptr, ctypes.c_int(on_dev), *tail))
    else:
        _check(_lib.scanrs_merge_clusters(mat._h, ptr, ctypes.c_int(on_dev), *tail))
    del keep
    if not trace:
        return out
    m = min(int(st.n_candidates), len(tr.leaf0))
    tr.leaf0, tr.leaf1, tr.n_de, tr.min_p_adj = tr.leaf0[:m], tr.leaf1[:m], tr.n_de[:m], tr.min_p_adj[:m]
    tr.n_candidates, tr.n_rounds, tr.n_merges, tr.n_passes = int(st.n_candidates), int(st.n_rounds), int(st.n_merges), int(st.n_passes)
    tr.entries = [(int(a), int(b), int(c), float(p)) for a, b, c, p in zip(tr.leaf0, tr.leaf1, tr.n_de, tr.min_p_adj)]
    return out, tr
