"""hclust (hclust/src/lib.rs): hierarchical clustering with leaf ordering.

``HierarchicalCluster(array, method, direction)`` is `HierarchicalCluster::new` (:132-148) with the Euclidean metric: the distance
pass and the nearest-neighbour chain run on the device, the dendrogram is kodama::linkage's (steps sorted by
dissimilarity, the cluster of sorted step i named n + i, cluster1 < cluster2). ``leaves`` (:150-206),
``merge_clusters_below_distance_threshold`` (:210-227) and ``fcluster`` (:231-239) are the reference's. Centroid and Median linkage
are not provided (they are not reducible) and raise ``ScanrsError``.

``array`` is a numpy array (f32 is widened to f64) or a ``DeviceArray2`` naming a row-major f64 array in device memory, e.g.
``DeviceArray2.u_of(pca_result_device(mat))``. ``host_linkage`` is the chain's host twin: the same steps in plain C++, equal bit for bit.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import PcaResultDevice, ScanrsError, _check, _lib, _p

_u64, _u32 = ctypes.c_uint64, ctypes.c_uint32

_lib.scanrs_hclust_free.restype = None
_lib.scanrs_hclust_free.argtypes = [ctypes.c_void_p]
_lib.scanrs_hclust_merge_below.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p]
_lib.scanrs_hclust_merge_below.restype = ctypes.c_int


class LinkageMethod:
    """kodama::Method, in its order."""

    Single, Complete, Average, Weighted, Ward, Centroid, Median = range(7)
    _NAMES = {"single": 0, "complete": 1, "average": 2, "weighted": 3, "ward": 4, "centroid": 5, "median": 6}

    @staticmethod
    def from_str(s: str) -> int:
        if s.lower() not in LinkageMethod._NAMES:
            raise ValueError(f"LinkageMethod not recognized: {s}")
        return LinkageMethod._NAMES[s.lower()]


class ClusterDirection:
    """ClusterDirection (:30-35): which axis of the array holds the observations."""

    Rows, Columns = 0, 1


class LeafOrdering:
    """LeafOrdering (:53-59)."""

    Naive, ModularSmallest = 0, 1


@dataclass
class DeviceArray2:
    """A rows x cols f64 array in device memory, row-major with leading dimension ld (elements). `keep` is held so that its owner
    outlives the call."""

    ptr: int
    rows: int
    cols: int
    ld: int
    keep: object = None

    @staticmethod
    def u_of(res: PcaResultDevice) -> "DeviceArray2":
        return DeviceArray2(res.d_u, res.rows, res.k, res.ld_u, res)

    @staticmethod
    def v_of(res: PcaResultDevice) -> "DeviceArray2":
        return DeviceArray2(res.d_v, res.cols, res.k, res.ld_v, res)


@dataclass
class Steps:
    """kodama::Dendrogram's steps: n - 1 entries each."""

    cluster1: np.ndarray
    cluster2: np.ndarray
    dissimilarity: np.ndarray
    size: np.ndarray

    def __len__(self):
        return len(self.cluster1)


def _method(method) -> int:
    return LinkageMethod.from_str(method) if isinstance(method, str) else int(method)


class HierarchicalCluster:
    """`HierarchicalCluster` (hclust/src/lib.rs:127-240)."""

    def __init__(self, array, method=LinkageMethod.Ward, direction=ClusterDirection.Rows, snoop=None, _handle: Optional[int] = None):
        self._h = None
        if _handle is not None:
            self._h = ctypes.c_void_p(_handle)
            return
        sn_keep = None if snoop is None else snoop._struct()
        sn = None if sn_keep is None else ctypes.byref(sn_keep)
        h = ctypes.c_void_p()
        if isinstance(array, PcaResultDevice):
            raise ScanrsError(6, "name the factor: DeviceArray2.u_of(result) or DeviceArray2.v_of(result)")
        if isinstance(array, DeviceArray2):
            _check(_lib.scanrs_hclust_create_device(ctypes.c_void_p(array.ptr), _u64(array.rows), _u64(array.cols), _u64(array.ld), ctypes.c_int(int(direction)),
                                                    ctypes.c_int(_method(method)), sn, ctypes.byref(h)))
        else:
            a = np.asarray(array)
            if a.ndim != 2:
                raise ScanrsError(6, "the observations must be a 2-d array")
            a = np.ascontiguousarray(a, dtype=np.float64)  # (f32 widens exactly)
            _check(_lib.scanrs_hclust_create(_p(a), _u64(a.shape[0]), _u64(a.shape[1]), _u64(a.shape[1]), ctypes.c_int(int(direction)),
                                             ctypes.c_int(_method(method)), sn, ctypes.byref(h)))
        self._h = h

    @staticmethod
    def from_steps(cluster1, cluster2, dissimilarity, size) -> "HierarchicalCluster":
        """A handle around a given, already sorted dendrogram (host only; validated)."""
        c1 = np.ascontiguousarray(cluster1, dtype=np.uint32).ravel()
        c2 = np.ascontiguousarray(cluster2, dtype=np.uint32).ravel()
        ds = np.ascontiguousarray(dissimilarity, dtype=np.float64).ravel()
        sz = np.ascontiguousarray(size, dtype=np.uint32).ravel()
        if not (len(c1) == len(c2) == len(ds) == len(sz)):
            raise ScanrsError(6, "the four step arrays must have the same length")
        h = ctypes.c_void_p()
        _check(_lib.scanrs_hclust_from_steps(_u64(len(c1) + 1), _p(c1), _p(c2), _p(ds), _p(sz), ctypes.byref(h)))
        return HierarchicalCluster(None, _handle=h.value)

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.scanrs_hclust_free(self._h)
            self._h = None

    @property
    def observations(self) -> int:
        n = _u64()
        _check(_lib.scanrs_hclust_n(self._h, ctypes.byref(n)))
        return int(n.value)

    @property
    def steps(self) -> Steps:
        m = self.observations - 1
        s = Steps(np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint32), np.zeros(m), np.zeros(m, dtype=np.uint32))
        _check(_lib.scanrs_hclust_steps(self._h, _p(s.cluster1), _p(s.cluster2), _p(s.dissimilarity), _p(s.size)))
        return s

    def leaves(self, ordering=LeafOrdering.Naive) -> np.ndarray:
        """`leaves` (:201-206): x[i] = j, observation j stands at position i from the left."""
        out = np.zeros(self.observations, dtype=np.uint32)
        _check(_lib.scanrs_hclust_leaves(self._h, ctypes.c_int(int(ordering)), _p(out)))
        return out

    def merge_clusters_below_distance_threshold(self, distance_threshold: float) -> np.ndarray:
        """(:210-227): every link with dissimilarity < threshold merged; labels 1, 2, .. in order of first appearance."""
        out = np.zeros(self.observations, dtype=np.uint32)
        _check(_lib.scanrs_hclust_merge_below(self._h, ctypes.c_double(float(distance_threshold)), _p(out)))
        return out

    def fcluster(self, num_clusters: int) -> np.ndarray:
        """`fcluster` (:231-239)."""
        if int(num_clusters) < 0:
            raise ScanrsError(6, "num_clusters is a count")
        out = np.zeros(self.observations, dtype=np.uint32)
        _check(_lib.scanrs_hclust_fcluster(self._h, _u64(int(num_clusters)), _p(out)))
        return out

    def info(self) -> dict:
        """What the device run did: chain steps, kernel launches, batches the host waited for, bytes of the distance matrix,
        milliseconds of the distance pass and of the chain (HIP events), merges."""
        v = np.zeros(7, dtype=np.uint64)
        _check(_lib.scanrs_hclust_info(self._h, _p(v), _u32(7)))
        return {"chain_steps": int(v[0]), "launches": int(v[1]), "batches": int(v[2]), "matrix_bytes": int(v[3]), "pdist_ms": int(v[4]) / 1e3,
                "chain_ms": int(v[5]) / 1e3, "merges": int(v[6])}


def host_linkage(x, method) -> Steps:
    """`scanrs_host_hclust_linkage`: the device chain's host twin on the rows of x (tests and small inputs)."""
    x = np.asarray(x)
    if x.ndim != 2:
        raise ScanrsError(6, "the observations must be a 2-d array")
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, d = x.shape
    m = max(n - 1, 0)
    s = Steps(np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint32), np.zeros(m), np.zeros(m, dtype=np.uint32))
    _check(_lib.scanrs_host_hclust_linkage(_p(x), _u64(n), _u32(d), ctypes.c_int(_method(method)), _p(s.cluster1), _p(s.cluster2), _p(s.dissimilarity),
                                           _p(s.size)))
    return s


def debug_pdist(x, squared: bool, d: Optional[int] = None) -> np.ndarray:
    """`scanrs_debug_hclust_pdist`: the device distance pass alone, condensed in `pdist`'s order. x is n x ld; its first d columns
    (default: all) are the coordinates, the rest is padding that is never read."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    n, ld = x.shape
    d = ld if d is None else int(d)
    out = np.zeros(n * (n - 1) // 2)
    _check(_lib.scanrs_debug_hclust_pdist(_p(x), _u64(n), _u32(d), _u64(ld), ctypes.c_int(1 if squared else 0), _p(out)))
    return out
