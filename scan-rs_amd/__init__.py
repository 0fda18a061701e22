"""scan-rs_amd: MI355X (gfx950) implementation of scan-rs's sparse-count-matrix
normalize -> PCA hot path, behind the C ABI of ``include/scanrs_amd.h``.

This module is the Python host-side mirror used by the tests and ``bench.py``:
same names, argument meaning and error behaviour as the reference's operator
surface (``sqz::AdaptiveMat`` / ``LowRankOffset`` / ``scan_rs::normalization`` /
``scan_rs::dim_red::{BkSvd, RandSvd, Irlba}``), every call going straight
through ctypes into ``lib/libscanrs_amd.so``.  There is no CPU fallback: if the
shared library is missing the import fails, and without a gfx950 device every
compute call raises ``ScanrsError``.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SCANRS_AMD_LIB: another build of the same library (A/B timing of two builds on one GPU box; tools/pass_bench.py)
LIB_PATH = os.environ.get("SCANRS_AMD_LIB") or os.path.join(_HERE, "lib", "libscanrs_amd.so")

CSR, CSC = 0, 1
FN_LN_1P, FN_LOG2_1P, FN_LOG10_1P, FN_SQUARE = 2, 3, 4, 5


class Normalization:
    """`enum Normalization` (scan-rs/src/normalization.rs:11-28) and its `FromStr` (:30-43)."""

    CellRanger, CellRanger8, SeuratLog, BinomialDeviance, BinomialPearson, WithSizeFactors, LogTransform = range(7)
    _NAMES = {
        "cellranger": 0,
        "cellranger8": 1,
        "seuratlog": 2,
        "binomialdeviance": 3,
        "binomialpearson": 4,
    }

    @staticmethod
    def from_str(s: str) -> int:
        if s not in Normalization._NAMES:
            raise ValueError(f"Normalization not recognized: {s}")
        return Normalization._NAMES[s]


class ScanrsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[scanrs {code}] {msg}")
        self.code = code


class CancellationError(ScanrsError):
    """snoop::CancellationError (snoop/src/lib.rs:5-18)."""


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(hipcc --offload-arch=gfx950). scan-rs_amd has no CPU fallback."
    )


def _preload_rocm_runtime():
    """PyTorch-ROCm wheels bundle their own HIP / HSA runtime under torch/lib with the same sonames as
    /opt/rocm's. Whichever copy is loaded first serves the whole process, and torch does not find the GPU
    when the system copy came first. So if torch is installed (not imported: find_spec only) its copy is
    loaded up front; without torch the system runtime is used."""
    import importlib.util

    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
            except OSError:
                return


_preload_rocm_runtime()
_lib = ctypes.CDLL(LIB_PATH)
_lib.scanrs_last_error.restype = ctypes.c_char_p
_lib.scanrs_version.restype = ctypes.c_char_p

_PROGRESS_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_double)
_ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int)


class _Snoop(ctypes.Structure):
    _fields_ = [("cancel", ctypes.c_void_p), ("progress", _PROGRESS_FN), ("ctx", ctypes.c_void_p)]


class _KernelStat(ctypes.Structure):
    _fields_ = [
        ("name", ctypes.c_char * 48),
        ("launches", ctypes.c_uint64),
        ("total_ms", ctypes.c_double),
        ("algorithmic_bytes", ctypes.c_double),
        ("onchip_gather_bytes", ctypes.c_double),
    ]


def _check(code: int):
    if code != 0:
        msg = _lib.scanrs_last_error().decode("utf-8", "replace")
        if code == 3:
            raise CancellationError(code, msg)
        raise ScanrsError(code, msg)


def device_available() -> bool:
    return bool(_lib.scanrs_device_available())


def version() -> str:
    return _lib.scanrs_version().decode()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _index_list(idx, prefix: str = ""):
    """An index list for the C ABI: flattened to int64, negatives refused (`prefix` names the argument in the message), as uint64."""
    idx = np.ascontiguousarray(np.asarray(idx).reshape(-1), dtype=np.int64)
    if idx.size and int(idx.min()) < 0:
        raise ScanrsError(6, prefix + "index out of range: negative index")
    return idx.astype(np.uint64)


def _partition_on_thresholds(fn, handle, shape, wrap, row_threshold, col_threshold, filtered, residual):
    """The three `partition_on_thresholds` methods: `fn` is the C entry point, `shape` the [rows, cols] the kept lists are sized
    from, `wrap` makes the object of a returned handle."""
    rows, cols = shape
    sel_r, sel_c = np.zeros(max(rows, 1), dtype=np.uint64), np.zeros(max(cols, 1), dtype=np.uint64)
    n_r, n_c = ctypes.c_uint64(), ctypes.c_uint64()
    rt = None if row_threshold is None else ctypes.byref(ctypes.c_double(row_threshold))
    ct = None if col_threshold is None else ctypes.byref(ctypes.c_double(col_threshold))
    hf, hr = ctypes.c_void_p(), ctypes.c_void_p()
    _check(fn(handle, rt, ct, ctypes.byref(hf) if filtered else None, ctypes.byref(hr) if residual else None, _p(sel_r), ctypes.byref(n_r),
              _p(sel_c), ctypes.byref(n_c)))
    f = wrap(hf.value) if filtered else None
    r = wrap(hr.value) if residual else None
    return f, r, sel_r[: n_r.value].astype(np.int64), sel_c[: n_c.value].astype(np.int64)


class AtomicSnoop:
    """`snoop::AtomicSnoop` (snoop/src/lib.rs:117-226): cancel flag + progress fraction."""

    def __init__(self):
        self._flag = (ctypes.c_uint8 * 1)(0)
        self.progress = 0.0
        self.history = []
        self._cb = _PROGRESS_FN(self._on_progress)

    def _on_progress(self, _ctx, frac):
        self.progress = frac
        self.history.append(frac)

    def cancel(self):
        self._flag[0] = 1

    def is_cancelled(self):
        return bool(self._flag[0])

    def _struct(self):
        return _Snoop(ctypes.cast(self._flag, ctypes.c_void_p), self._cb, None)


def knn(v, k: int):
    """`nn::knn(v, k)` (scan-rs/src/nn.rs:38-57): (cells x k) u32 indices of the k nearest other rows of `v`, nearest first."""
    v = _f64(np.atleast_2d(v))
    n, d = v.shape
    out = np.zeros((n, k), dtype=np.uint32)
    _check(_lib.scanrs_knn(_p(v), ctypes.c_uint64(n), ctypes.c_uint32(d), ctypes.c_uint32(k), _p(out)))
    return out


def find_nn(v, k: int, tree_points, include_self: bool):
    """`nn::find_nn(v, k, ball_tree, include_self)` (nn.rs:63-83); the "tree" is the point set itself."""
    v, t = _f64(np.atleast_2d(v)), _f64(np.atleast_2d(tree_points))
    if v.shape[1] != t.shape[1]:
        raise ScanrsError(1, "Dimension mismatch")
    out = np.zeros((v.shape[0], k), dtype=np.uint32)
    _check(_lib.scanrs_find_nn(_p(v), ctypes.c_uint64(v.shape[0]), _p(t), ctypes.c_uint64(t.shape[0]), ctypes.c_uint32(v.shape[1]),
                               ctypes.c_uint32(k), ctypes.c_int(1 if include_self else 0), _p(out)))
    return out


ADAPTIVE_KINDS = ("D3", "D4", "D8", "D16", "V", "S3", "S4", "S8")  # `enum AdaptiveVec` (vec.rs:1029-1053): the `kind` codes


def choose_storage(length: int, values):
    """`AdaptiveVec::choose_storage(len, values)` (vec.rs:1086-1131) on the host: (kind code, min_size)."""
    v = np.ascontiguousarray(values, dtype=np.uint32)
    kind, min_size = ctypes.c_int(), ctypes.c_uint64()
    _check(_lib.scanrs_host_choose_storage(ctypes.c_uint64(int(length)), _p(v), ctypes.c_uint64(v.shape[0]), ctypes.byref(kind),
                                           ctypes.byref(min_size)))
    return int(kind.value), int(min_size.value)


class AdaptiveVecDesc(ctypes.Structure):
    """`scanrs_adaptive_vec` (include/scanrs_amd.h): one sqz::AdaptiveVec by its encoded buffers."""
    _fields_ = [("kind", ctypes.c_uint32), ("len", ctypes.c_uint64), ("n_units", ctypes.c_uint64), ("data", ctypes.c_void_p),
                ("data_bytes", ctypes.c_uint64), ("fallback_indexes", ctypes.c_void_p), ("fallback_values", ctypes.c_void_p),
                ("n_fallback", ctypes.c_uint64), ("index_bytes", ctypes.c_void_p), ("block_starts", ctypes.c_void_p),
                ("n_block_starts", ctypes.c_uint64)]


def _export_kind(kind) -> int:
    """force_kind of the to_adaptive calls: None = choose_storage (-1), a code 0..7, or a name of ADAPTIVE_KINDS."""
    if isinstance(kind, str):
        if kind not in ADAPTIVE_KINDS:
            raise ScanrsError(6, f"unknown AdaptiveVec encoding {kind!r}")
        return ADAPTIVE_KINDS.index(kind)
    return -1 if kind is None else int(kind)


EXPORT_STORED, EXPORT_INNER = 0, 1  # SCANRS_EXPORT_*


def _export_major(major) -> int:
    """`major` of the to_adaptive calls: "stored" / "inner" or a SCANRS_EXPORT_* code (the library refuses what it does not know)."""
    if isinstance(major, str):
        if major not in ("stored", "inner"):
            raise ScanrsError(6, f"major must be 'stored' or 'inner', not {major!r}")
        return EXPORT_INNER if major == "inner" else EXPORT_STORED
    return int(major)


def _export_totals(e):
    """(total_bytes, kind_counts) of a `scanrs_adaptive_export`."""
    total, counts = ctypes.c_uint64(), (ctypes.c_uint64 * 8)()
    _check(_lib.scanrs_adaptive_export_info(e, None, ctypes.byref(total), counts))
    return int(total.value), [int(c) for c in counts]


def _export_vecs(e):
    """The table of a `scanrs_adaptive_export` as the mappings `from_adaptive_vecs` takes (numpy copies)."""
    n, table = ctypes.c_uint64(), ctypes.POINTER(AdaptiveVecDesc)()
    _check(_lib.scanrs_adaptive_export_info(e, ctypes.byref(n), None, None))
    _check(_lib.scanrs_adaptive_export_vecs(e, ctypes.byref(table)))

    def arr(ptr, count, dt):
        if not count:
            return np.zeros(0, dtype=dt)
        return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(count,)).copy()

    out = []
    for i in range(int(n.value)):
        d = table[i]
        k = int(d.kind)
        v = dict(kind=k, len=int(d.len), n_units=int(d.n_units), data=None, index_bytes=None, block_starts=None)
        v["fallback_indexes"] = arr(d.fallback_indexes, d.n_fallback, np.uint32)
        v["fallback_values"] = arr(d.fallback_values, d.n_fallback, np.uint32)
        if k != 4:
            dt = np.uint64 if k in (0, 5) else np.uint16 if k == 3 else np.uint8
            v["data"] = arr(d.data, d.data_bytes // np.dtype(dt).itemsize, dt)
        if k >= 5:
            v["index_bytes"] = arr(d.index_bytes, d.n_units, np.uint8)
            v["block_starts"] = arr(d.block_starts, d.n_block_starts, np.uint32)
        out.append(v)
    return out


def _adaptive_table(vecs):
    """The `scanrs_adaptive_vec` table of one mapping per outer vector (see `AdaptiveMat.from_adaptive_vecs`): (n, table, arrays
    that must outlive the call)."""
    n = len(vecs)
    table = (AdaptiveVecDesc * max(n, 1))()
    keep = []  # arrays must outlive the call

    def arr(a, dt):
        if a is None:
            return None, 0
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data_as(ctypes.c_void_p), a.shape[0]

    for i, v in enumerate(vecs):
        d = table[i]
        d.kind, d.len, d.n_units = int(v["kind"]), int(v["len"]), int(v["n_units"])
        data = v.get("data")
        if data is not None:
            data = np.ascontiguousarray(data)
            keep.append(data)
            d.data, d.data_bytes = data.ctypes.data_as(ctypes.c_void_p), data.nbytes
        fi, nfi = arr(v.get("fallback_indexes"), np.uint32)
        fv, nfv = arr(v.get("fallback_values"), np.uint32)
        if nfi != nfv:
            raise ScanrsError(6, "fallback indexes / values differ in length")
        d.fallback_indexes, d.fallback_values, d.n_fallback = fi, fv, nfi
        ib, _ = arr(v.get("index_bytes"), np.uint8)
        bs, nbs = arr(v.get("block_starts"), np.uint32)
        d.index_bytes, d.block_starts, d.n_block_starts = ib, bs, nbs
    return n, table, keep


def _sharded_points(points, device: bool = False, cells=None):
    """The `points` of the searches over a sharded point set -> (points, ld, d): a device address to pass as it is (device=True),
    or a host array for `_p` that the caller keeps alive over the call. device=True: the rank's own rows in device memory, a PcaResultDevice (its d_v / ld_v / k) or a tuple (address, ld, d); None: the scores a PCA left
    on the device (a MultiMat); otherwise a host array over all cells, `cells` rows if given."""
    if device:
        ptr, ld, d = (points.d_v, points.ld_v, points.k) if isinstance(points, PcaResultDevice) else points
        return ctypes.c_void_p(int(ptr) if ptr else None), int(ld), int(d)
    if points is None:
        return None, 0, 0
    pts = _f64(np.atleast_2d(points))
    if cells is not None and pts.shape[0] != cells:
        raise ScanrsError(6, f"the points have {pts.shape[0]} rows for {cells} cells")
    return pts, int(pts.shape[1]), int(pts.shape[1])


class AdaptiveMat:
    """Device-resident `sqz::AdaptiveMat<N, D, M>` (sqz/src/mat.rs:34-42). Once a low-rank
    offset is installed (`center`, `scale_and_center`, `normalize`) the same object plays
    `sqz::LowRankOffset` (sqz/src/low_rank_offset.rs:12-16)."""

    def __init__(self, handle):
        self._h = ctypes.c_void_p(handle)
        self._keep = []  # callbacks that must outlive the handle

    # -- constructors ----------------------------------------------------------------
    @staticmethod
    def from_csmat(rows: int, cols: int, storage: int, indptr, indices, data, unsorted: bool = False) -> "AdaptiveMat":
        """`AdaptiveMat::from_csmat` (mat.rs:92-124): host indptr(u64) / indices(u32) / data(u32).
        unsorted=True: indices may be in any order inside an outer vector (hdf5-io/src/matrix.rs:66-75 fallback)."""
        indptr = np.ascontiguousarray(indptr, dtype=np.uint64)
        indices = np.ascontiguousarray(indices, dtype=np.uint32)
        data = np.ascontiguousarray(data, dtype=np.uint32)
        n_outer = rows if storage == CSR else cols
        if indptr.shape[0] != n_outer + 1:
            raise ScanrsError(6, "indptr length does not match the outer dimension")
        if indices.shape[0] != data.shape[0] or (indptr.shape[0] and int(indptr[-1]) != indices.shape[0]):
            raise ScanrsError(6, "indices/data length does not match indptr")
        h = ctypes.c_void_p()
        fn = _lib.scanrs_mat_create_unsorted if unsorted else _lib.scanrs_mat_create
        _check(fn(ctypes.c_uint64(rows), ctypes.c_uint64(cols), ctypes.c_int(storage), _p(indptr), _p(indices), _p(data), ctypes.byref(h)))
        return AdaptiveMat(h.value)

    @staticmethod
    def from_adaptive_vecs(rows: int, cols: int, storage: int, vecs) -> "AdaptiveMat":
        """`AdaptiveMat::new(rows, cols, storage, Vec<AdaptiveVec>)` (mat.rs:68-90): `vecs` is one mapping per outer
        vector with the fields of `scanrs_adaptive_vec` (kind, len, n_units, data, fallback_indexes, fallback_values,
        index_bytes, block_starts) holding numpy arrays in the reference's in-memory layout; decoded on the device."""
        n, table, _keep = _adaptive_table(vecs)
        h = ctypes.c_void_p()
        _check(_lib.scanrs_mat_create_adaptive(ctypes.c_uint64(rows), ctypes.c_uint64(cols), ctypes.c_int(storage), table,
                                              ctypes.c_uint64(n), ctypes.byref(h)))
        return AdaptiveMat(h.value)

    @staticmethod
    def from_device(rows: int, cols: int, storage: int, indptr_ptr: int, indices_ptr: int, data_ptr: int) -> "AdaptiveMat":
        """Same triplet already in device memory (e.g. `tensor.data_ptr()`); copied, not adopted."""
        h = ctypes.c_void_p()
        _check(
            _lib.scanrs_mat_create_device(
                ctypes.c_uint64(rows), ctypes.c_uint64(cols), ctypes.c_int(storage), ctypes.c_void_p(indptr_ptr),
                ctypes.c_void_p(indices_ptr), ctypes.c_void_p(data_ptr), ctypes.byref(h)))
        return AdaptiveMat(h.value)

    @staticmethod
    def from_scipy(m) -> "AdaptiveMat":
        import scipy.sparse as sp

        if sp.isspmatrix_csc(m):
            st = CSC
        else:
            m = m.tocsr()
            st = CSR
        m.sort_indices()
        return AdaptiveMat.from_csmat(m.shape[0], m.shape[1], st, m.indptr, m.indices, m.data)

    @staticmethod
    def from_dense(dense, storage: int = CSR) -> "AdaptiveMat":
        """`AdaptiveMat::from_dense` (mat.rs:122-150)."""
        import scipy.sparse as sp

        dense = np.asarray(dense)
        m = sp.csr_matrix(dense) if storage == CSR else sp.csc_matrix(dense)
        return AdaptiveMat.from_scipy(m)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None:  # (at interpreter shutdown the module globals may be gone already)
            _lib.scanrs_mat_free(h)
            self._h = ctypes.c_void_p()

    # -- shape / views -----------------------------------------------------------------
    def shape(self):
        r, c = ctypes.c_uint64(), ctypes.c_uint64()
        _check(_lib.scanrs_mat_shape(self._h, ctypes.byref(r), ctypes.byref(c)))
        return [int(r.value), int(c.value)]

    def rows(self):
        return self.shape()[0]

    def cols(self):
        return self.shape()[1]

    def nnz(self):
        n = ctypes.c_uint64()
        _check(_lib.scanrs_mat_nnz(self._h, ctypes.byref(n)))
        return int(n.value)

    def storage(self):
        s = ctypes.c_int()
        _check(_lib.scanrs_mat_storage(self._h, ctypes.byref(s)))
        return int(s.value)

    def view(self) -> "AdaptiveMat":
        h = ctypes.c_void_p()
        _check(_lib.scanrs_mat_view(self._h, ctypes.byref(h)))
        v = AdaptiveMat(h.value)
        v._keep = self._keep
        v._outer_global = getattr(self, "_outer_global", None)
        return v

    def t(self) -> "AdaptiveMat":
        h = ctypes.c_void_p()
        _check(_lib.scanrs_mat_t(self._h, ctypes.byref(h)))
        v = AdaptiveMat(h.value)
        v._keep = self._keep
        v._outer_global = getattr(self, "_outer_global", None)
        return v

    # -- lazy maps --------------------------------------------------------------------------
    def reset_map(self):
        _check(_lib.scanrs_mat_reset_map(self._h))
        return self

    def compose_scale_axis(self, axis: int, factors):
        """`compose_map(ScaleAxis::new(Axis(axis), factors))`."""
        f = _f64(factors)
        want = self.rows() if axis == 0 else self.cols()
        if axis in (0, 1) and f.shape[0] != want:
            raise ScanrsError(1, "Dimension mismatch")
        _check(_lib.scanrs_mat_compose_scale_axis(self._h, ctypes.c_int(axis), _p(f)))
        return self

    def apply(self, scalar_fn: int):
        _check(_lib.scanrs_mat_apply(self._h, ctypes.c_int(scalar_fn)))
        return self

    def set_offset(self, u, v):
        """`LowRankOffset::new(mat, u, v)`: u rows x rank, v rank x cols."""
        u, v = _f64(u), _f64(v)
        r, c = self.shape()
        if u.ndim != 2 or v.ndim != 2 or u.shape[0] != r or v.shape[1] != c or u.shape[1] != v.shape[0]:
            raise ScanrsError(1, "Dimension mismatch")
        _check(_lib.scanrs_mat_set_offset(self._h, ctypes.c_uint32(u.shape[1]), _p(u), _p(v)))
        return self

    def center(self, axis: int, m=None):
        mm = None if m is None else _f64(m)
        _check(_lib.scanrs_mat_center(self._h, ctypes.c_int(axis), _p(mm)))
        return self

    def scale(self, axis: int, s=None):
        ss = None if s is None else _f64(s)
        _check(_lib.scanrs_mat_scale(self._h, ctypes.c_int(axis), _p(ss)))
        return self

    def scale_and_center(self, axis: int, scaling_factors=None):
        ss = None if scaling_factors is None else _f64(scaling_factors)
        _check(_lib.scanrs_mat_scale_and_center(self._h, ctypes.c_int(axis), _p(ss)))
        return self

    # -- reductions ----------------------------------------------------------------------------
    def sum_axis(self, axis: int, dtype=np.float64):
        if axis not in (0, 1):
            raise ScanrsError(6, "axis must be 0 or 1")
        n = self.cols() if axis == 0 else self.rows()
        if dtype == np.uint32:
            out = np.zeros(n, dtype=np.uint32)
            _check(_lib.scanrs_mat_sum_axis_u32(self._h, ctypes.c_int(axis), _p(out)))
        else:
            out = np.zeros(n, dtype=np.float64)
            _check(_lib.scanrs_mat_sum_axis_f64(self._h, ctypes.c_int(axis), _p(out)))
        return out

    def mean_axis(self, axis: int):
        n = self.cols() if axis == 0 else self.rows()
        out = np.zeros(n)
        _check(_lib.scanrs_mat_mean_axis(self._h, ctypes.c_int(axis), _p(out)))
        return out

    def mean_var_axis(self, axis: int):
        n = self.cols() if axis == 0 else self.rows()
        mean, var = np.zeros(n), np.zeros(n)
        _check(_lib.scanrs_mat_mean_var_axis(self._h, ctypes.c_int(axis), _p(mean), _p(var)))
        return mean, var

    def var_axis(self, axis: int):
        """`var_axis` (mat.rs:409-411): `mean_var_axis(axis)[1]`, the same bits."""
        if axis not in (0, 1):
            raise ScanrsError(6, "axis must be 0 or 1")
        out = np.zeros(self.cols() if axis == 0 else self.rows())
        _check(_lib.scanrs_mat_var_axis(self._h, ctypes.c_int(axis), _p(out)))
        return out

    # -- statistics over a list of columns (mat.rs:279-282, 333-374, 414-583) ---------------
    # One implementation per statistic serves the plain, the *_sharded and the MultiMat methods. `head`: the leading arguments of the
    # C call (the handle; MultiMat adds `transposed`); n_rows / n_out: where the length of a result comes from, read after the lists
    # have been checked.
    @staticmethod
    def _sum_dtype(dtype):
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.uint64), np.dtype(np.uint32), np.dtype(np.float64)):
            raise ScanrsError(6, "dtype must be np.uint64, np.uint32 or np.float64")
        return dt

    @staticmethod
    def _narrow(out, dt):
        # u32 results are computed in 64 bits and narrowed; the reference's u32 accumulator panics on overflow in a debug build
        if dt != np.dtype(np.uint32):
            return out
        if out.size and int(out.max()) > 0xFFFFFFFF:
            raise OverflowError(f"a sum of {int(out.max())} does not fit in uint32")
        return out.astype(np.uint32)

    @staticmethod
    def _sums_over(head, fn_u64, fn_f64, cols, dtype, n_out):
        dt, cols = AdaptiveMat._sum_dtype(dtype), _index_list(cols)
        is_f = dt == np.dtype(np.float64)
        out = np.zeros(n_out(cols), dtype=np.float64 if is_f else np.uint64)
        _check((fn_f64 if is_f else fn_u64)(*head, _p(cols), ctypes.c_uint64(cols.shape[0]), _p(out)))
        return AdaptiveMat._narrow(out, dt)

    @staticmethod
    def _sum_rows_dual(head, fn_u64, fn_f64, n_rows, cols1, cols2, dtype, snoop):
        dt, c1, c2 = AdaptiveMat._sum_dtype(dtype), _index_list(cols1), _index_list(cols2)
        is_f = dt == np.dtype(np.float64)
        o1, o2 = (np.zeros(n_rows(), dtype=np.float64 if is_f else np.uint64) for _ in range(2))
        sn, _keep = _snoop_arg(snoop)
        _check((fn_f64 if is_f else fn_u64)(*head, _p(c1), ctypes.c_uint64(c1.shape[0]), _p(c2), ctypes.c_uint64(c2.shape[0]), sn, _p(o1), _p(o2)))
        return AdaptiveMat._narrow(o1, dt), AdaptiveMat._narrow(o2, dt)

    @staticmethod
    def _mean_rows(head, fn, n_rows, cols):
        cols = _index_list(cols)
        out = np.zeros(n_rows())
        _check(fn(*head, _p(cols), ctypes.c_uint64(cols.shape[0]), _p(out)))
        return out

    @staticmethod
    def _mean_var_rows(head, fn, n_rows, cols):
        cols = _index_list(cols)
        mean, var = np.zeros(n_rows()), np.zeros(n_rows())
        _check(fn(*head, _p(cols), ctypes.c_uint64(cols.shape[0]), _p(mean), _p(var)))
        return mean, var

    def sum_rows(self, cols, dtype=np.float64):
        """`sum_rows::<O>(cols)` (mat.rs:449-481): per row, the sum over the listed columns (strictly ascending). Integer dtypes read
        the raw counts (exact), float64 the mapped values."""
        return self._sums_over((self._h,), _lib.scanrs_mat_sum_rows_u64, _lib.scanrs_mat_sum_rows_f64, cols, dtype, lambda c: self.rows())

    def sum_cols(self, cols, dtype=np.float64):
        """`sum_cols::<O>(cols)` (mat.rs:414-446): per listed column, in list order, the sum over all rows."""
        return self._sums_over((self._h,), _lib.scanrs_mat_sum_cols_u64, _lib.scanrs_mat_sum_cols_f64, cols, dtype, lambda c: c.shape[0])

    def sum_rows_dual(self, cols1, cols2, dtype=np.float64, snoop=None):
        """`sum_rows_dual` / `sum_rows_dual_with_cancellation` (mat.rs:484-583): `sum_rows` over two lists from one walk; the lists
        may overlap."""
        return self._sum_rows_dual((self._h,), _lib.scanrs_mat_sum_rows_dual_u64, _lib.scanrs_mat_sum_rows_dual_f64, self.rows, cols1, cols2, dtype, snoop)

    def mean_rows(self, cols):
        """`mean_rows(cols)` (mat.rs:279-282); an empty list gives NaN."""
        return self._mean_rows((self._h,), _lib.scanrs_mat_mean_rows, self.rows, cols)

    def mean_var_rows(self, cols):
        """`mean_var_rows(cols)` (mat.rs:333-374): per row, mean and E[x^2] - E[x]^2 of the mapped values over the listed columns."""
        return self._mean_var_rows((self._h,), _lib.scanrs_mat_mean_var_rows, self.rows, cols)

    # -- the same over a sharded handle: collective, global lists, complete outputs on every rank ----
    def _rows_all(self) -> int:
        """The view's rows over all shards (an unsharded handle: its own)."""
        return self._global_shape()[0]

    def sum_rows_sharded(self, cols, dtype=np.float64):
        """`scanrs_mat_sum_rows_*_sharded`: `sum_rows` over a sharded handle; every rank calls it with the same (global) list."""
        return self._sums_over((self._h,), _lib.scanrs_mat_sum_rows_u64_sharded, _lib.scanrs_mat_sum_rows_f64_sharded, cols, dtype,
                               lambda c: self._rows_all())

    def sum_cols_sharded(self, cols, dtype=np.float64):
        """`scanrs_mat_sum_cols_*_sharded` (see `sum_rows_sharded`)."""
        return self._sums_over((self._h,), _lib.scanrs_mat_sum_cols_u64_sharded, _lib.scanrs_mat_sum_cols_f64_sharded, cols, dtype,
                               lambda c: c.shape[0])

    def sum_rows_dual_sharded(self, cols1, cols2, dtype=np.float64, snoop=None):
        """`scanrs_mat_sum_rows_dual_*_sharded` (see `sum_rows_sharded`)."""
        return self._sum_rows_dual((self._h,), _lib.scanrs_mat_sum_rows_dual_u64_sharded, _lib.scanrs_mat_sum_rows_dual_f64_sharded, self._rows_all,
                                   cols1, cols2, dtype, snoop)

    def mean_rows_sharded(self, cols):
        """`scanrs_mat_mean_rows_sharded` (see `sum_rows_sharded`)."""
        return self._mean_rows((self._h,), _lib.scanrs_mat_mean_rows_sharded, self._rows_all, cols)

    def mean_var_rows_sharded(self, cols):
        """`scanrs_mat_mean_var_rows_sharded` (see `sum_rows_sharded`)."""
        return self._mean_var_rows((self._h,), _lib.scanrs_mat_mean_var_rows_sharded, self._rows_all, cols)

    def to_dense(self):
        r, c = self.shape()
        out = np.zeros((r, c))
        _check(_lib.scanrs_mat_to_dense(self._h, _p(out)))
        return out

    # -- select / partition / download (mat.rs:207-241, 766-888, 1004-1071) --------------
    def _select(self, fn, idx) -> "AdaptiveMat":
        idx = _index_list(idx)
        h = ctypes.c_void_p()
        _check(fn(self._h, _p(idx), ctypes.c_uint64(idx.shape[0]), ctypes.byref(h)))
        return AdaptiveMat(h.value)

    def select_rows(self, idx) -> "AdaptiveMat":
        """`select_rows` (mat.rs:1041-1071): row i of the result is row idx[i]; any order, repeats allowed. A fresh handle."""
        return self._select(_lib.scanrs_mat_select_rows, idx)

    def select_cols(self, idx) -> "AdaptiveMat":
        """`select_cols` (mat.rs:1004-1038)."""
        return self._select(_lib.scanrs_mat_select_cols, idx)

    def partition_on_thresholds(self, row_threshold: Optional[float], col_threshold: Optional[float], filtered: bool = True,
                                residual: bool = True):
        """`partition_on_thresholds` (mat.rs:774-888): (filtered, residual, selected_rows, selected_cols); a threshold may be None.
        filtered=False / residual=False: that matrix is not built (None in its place)."""
        return _partition_on_thresholds(_lib.scanrs_mat_partition_on_thresholds, self._h, self.shape(), AdaptiveMat, row_threshold, col_threshold,
                                        filtered, residual)

    def partition_on_threshold(self, threshold: float):
        """`partition_on_threshold` (mat.rs:768-770)."""
        return self.partition_on_thresholds(threshold, threshold)

    # -- the collective forms for a sharded handle -------------------------
    def shard_info(self) -> dict:
        """`scanrs_mat_shard_info`: rank, world, outer_begin, outer_global (an unsharded handle: 0, 1, 0 and its own outer extent)."""
        r, w, b, g = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(_lib.scanrs_mat_shard_info(self._h, ctypes.byref(r), ctypes.byref(w), ctypes.byref(b), ctypes.byref(g)))
        return {"rank": int(r.value), "world": int(w.value), "outer_begin": int(b.value), "outer_global": int(g.value)}

    def _global_shape(self):
        """[rows, cols] of the whole matrix: the local shape with the sharded (stored outer) dimension replaced by outer_global."""
        shape = self.shape()
        shape[0 if self.storage() == CSR else 1] = self.shard_info()["outer_global"]
        return shape

    def _bound_like_self(self, result):
        if result is not None:
            result._keep.extend(self._keep)  # the transport (host hook or Comm) the result is bound to
            result._outer_global = result.shard_info()["outer_global"]
        return result

    def select_rows_sharded(self, idx) -> "AdaptiveMat":
        """`scanrs_mat_select_rows_sharded`: collective `select_rows` of a sharded handle. A list along the sharded dimension holds
        global positions and must not descend. On an unsharded handle: `select_rows`."""
        return self._bound_like_self(self._select(_lib.scanrs_mat_select_rows_sharded, idx))

    def select_cols_sharded(self, idx) -> "AdaptiveMat":
        """`scanrs_mat_select_cols_sharded` (see `select_rows_sharded`)."""
        return self._bound_like_self(self._select(_lib.scanrs_mat_select_cols_sharded, idx))

    def partition_on_thresholds_sharded(self, row_threshold: Optional[float], col_threshold: Optional[float], filtered: bool = True,
                                        residual: bool = True):
        """`scanrs_mat_partition_on_thresholds_sharded`: collective `partition_on_thresholds` of a sharded handle. The kept lists are
        those of the whole matrix, the same on every rank; the two matrices are this rank's shards of the results."""
        return _partition_on_thresholds(_lib.scanrs_mat_partition_on_thresholds_sharded, self._h, self._global_shape(),
                                        lambda h: self._bound_like_self(AdaptiveMat(h)), row_threshold, col_threshold, filtered, residual)

    def to_csmat(self):
        """`to_csmat` of the stored counts (mat.rs:207-241): (indptr u64, indices u32, data u32) in the handle's storage flag."""
        rows, cols = self.shape()
        n_outer = rows if self.storage() == CSR else cols
        nnz = self.nnz()
        indptr = np.zeros(n_outer + 1, dtype=np.uint64)
        indices, data = np.zeros(nnz, dtype=np.uint32), np.zeros(nnz, dtype=np.uint32)
        _check(_lib.scanrs_mat_to_csmat(self._h, _p(indptr), _p(indices), _p(data)))
        return indptr, indices, data

    def to_scipy(self):
        """The stored counts as scipy.sparse csr_matrix / csc_matrix (by the storage flag)."""
        import scipy.sparse as sp

        indptr, indices, data = self.to_csmat()
        cls = sp.csr_matrix if self.storage() == CSR else sp.csc_matrix
        return cls((data, indices.astype(np.int64), indptr.astype(np.int64)), shape=tuple(self.shape()))

    # -- back into sqz's own type: the AdaptiveVec encodings (mat.rs:92-124, vec.rs:1086-1160) ----
    def _export(self, kind, major="stored"):
        e = ctypes.c_void_p()
        _check(_lib.scanrs_mat_to_adaptive_major(self._h, ctypes.c_int(_export_major(major)), ctypes.c_int(_export_kind(kind)), ctypes.byref(e)))
        return e

    def adaptive_info(self, kind=None, major="stored"):
        """(total_bytes, kind_counts) of `to_adaptive_vecs(kind, major)`: the sum of `AdaptiveVec::mem_size` and how many vectors
        took each of the eight encodings (order of ADAPTIVE_KINDS)."""
        e = self._export(kind, major)
        try:
            return _export_totals(e)
        finally:
            _lib.scanrs_adaptive_export_free(e)

    def to_adaptive_vecs(self, kind=None, major="stored"):
        """`AdaptiveMat::from_csmat` backwards (mat.rs:92-124): the stored counts as one encoded `AdaptiveVec` per outer vector
        (`AdaptiveVec::new`, vec.rs:1086-1160), encoded on the device. kind=None: `choose_storage`; a code 0..7 or a name of
        ADAPTIVE_KINDS: that encoding for every vector. major="stored": one vector per stored outer vector; major="inner"
        (`scanrs_mat_to_adaptive_major`): one per INNER position, from the handle's transposed copy - what `from_adaptive_vecs` takes
        with the OTHER storage flag; refused on a sharded handle (`MultiMat.to_adaptive_vecs`). Returns the mappings
        `from_adaptive_vecs` takes (kind, len, n_units, data, fallback_indexes, fallback_values, index_bytes, block_starts), numpy
        copies in the reference's in-memory layout; pieces an encoding does not have are None."""
        e = self._export(kind, major)
        try:
            return _export_vecs(e)
        finally:
            _lib.scanrs_adaptive_export_free(e)

    def export_info(self, kind=None, major="stored") -> dict:
        """`scanrs_adaptive_export_multi_info` of this handle's export: always ScanrsError 6, since only `MultiMat.to_adaptive_vecs`
        makes an export over shards (the mirror of the C refusal)."""
        e = self._export(kind, major)
        try:
            return _export_multi_info(e)
        finally:
            _lib.scanrs_adaptive_export_free(e)

    # -- products ----------------------------------------------------------------------------------
    def dot(self, rhs):
        """`self.dot(&rhs)` (mat.rs:1074-1112, low_rank_offset.rs:68-81)."""
        rhs = np.asarray(rhs)
        one_d = rhs.ndim == 1
        if one_d:
            rhs = rhs.reshape(-1, 1)
        r, c = self.shape()
        if rhs.shape[0] != c:
            raise ScanrsError(1, "Dimension mismatch")
        l = rhs.shape[1]
        if rhs.dtype == np.uint32:
            rhs_c = np.ascontiguousarray(rhs)
            out = np.zeros((r, l), dtype=np.uint32)
            _check(_lib.scanrs_mat_dot_u32(self._h, _p(rhs_c), ctypes.c_uint32(l), _p(out)))
        else:
            rhs_c = _f64(rhs)
            out = np.zeros((r, l))
            _check(_lib.scanrs_mat_dot(self._h, _p(rhs_c), ctypes.c_uint32(l), _p(out)))
        return out[:, 0] if one_d else out

    def rdot(self, lhs):
        """`lhs.dot(&self)` (mat.rs:1114-1170, low_rank_offset.rs:83-96)."""
        lhs = np.asarray(lhs)
        one_d = lhs.ndim == 1
        if one_d:
            lhs = lhs.reshape(1, -1)
        r, c = self.shape()
        if lhs.shape[1] != r:
            raise ScanrsError(1, "Dimension mismatch")
        l = lhs.shape[0]
        if lhs.dtype == np.uint32:
            lhs_c = np.ascontiguousarray(lhs)
            out = np.zeros((l, c), dtype=np.uint32)
            _check(_lib.scanrs_mat_rdot_u32(self._h, _p(lhs_c), ctypes.c_uint32(l), _p(out)))
        else:
            lhs_c = _f64(lhs)
            out = np.zeros((l, c))
            _check(_lib.scanrs_mat_rdot(self._h, _p(lhs_c), ctypes.c_uint32(l), _p(out)))
        return out[0, :] if one_d else out

    def dot_device(self, transpose: bool, rhs_ptr: int, ld_rhs: int, l: int, out_ptr: int, ld_out: int):
        _check(
            _lib.scanrs_mat_dot_device(
                self._h, ctypes.c_int(int(transpose)), ctypes.c_void_p(rhs_ptr), ctypes.c_uint32(ld_rhs), ctypes.c_uint32(l),
                ctypes.c_void_p(out_ptr), ctypes.c_uint32(ld_out)))

    # -- sharding / measurement ------------------------------------------------------------------------
    def set_shard(self, rank: int, world: int, outer_begin: int, outer_global: int, allreduce=None):
        """`allreduce(dev_ptr:int, count:int, dtype:int) -> int` sums in place across ranks (0 f64, 1 u64)."""
        cb = None
        if allreduce is not None:
            def _tramp(_ctx, ptr, count, dtype, _f=allreduce):
                try:
                    return int(_f(int(ptr), int(count), int(dtype)) or 0)
                except Exception:  # never unwind into C
                    import traceback

                    traceback.print_exc()
                    return 1

            cb = _ALLREDUCE_FN(_tramp)
            self._keep.append(cb)
        _check(
            _lib.scanrs_mat_set_shard(
                self._h, ctypes.c_uint32(rank), ctypes.c_uint32(world), ctypes.c_uint64(outer_begin),
                ctypes.c_uint64(outer_global), cb if cb is not None else ctypes.cast(None, _ALLREDUCE_FN), None))
        self._outer_global = int(outer_global)
        return self

    def set_shard_comm(self, comm: "Comm", outer_begin: int, outer_global: int):
        """Sharded handle over the library's own transport (`scanrs_mat_set_shard_comm`): RCCL collectives on the handle's
        stream. `comm` must outlive the handle's sharded calls."""
        _check(_lib.scanrs_mat_set_shard_comm(self._h, comm._c, ctypes.c_uint32(comm.rank), ctypes.c_uint32(comm.world),
                                              ctypes.c_uint64(outer_begin), ctypes.c_uint64(outer_global)))
        self._keep.append(comm)
        self._outer_global = int(outer_global)
        return self

    def knn_sharded(self, points, k: int, device: bool = False, return_sq_dist: bool = False):
        """`nn::knn` over a sharded point set (`scanrs_knn_sharded`, nn.rs:38-83): COLLECTIVE, every rank calls it with
        the same k. The handle gives the transport and the rank's range of cells (its columns). points: a host array over ALL cells, or
        with device=True the rank's own rows in device memory: a PcaResultDevice (its d_v / ld_v / k) or a tuple (address, ld, d).
        Returns the (n_local x k) u32 GLOBAL indices of the rank's cells, nearest first, UINT32_MAX padded - what `knn` of the whole
        point set returns for those rows, bit for bit - and with return_sq_dist also the squared distances (+inf in padded slots).
        On an unsharded handle it is `knn` / `knn_device` of the given points."""
        n_local = int(self.shape()[1])
        pts, ld, d = _sharded_points(points, device)
        out = np.zeros((n_local, k), dtype=np.uint32)
        sq = np.zeros((n_local, k)) if return_sq_dist else None
        _check(_lib.scanrs_knn_sharded(self._h, pts if device else _p(pts), ctypes.c_int(1 if device else 0), ctypes.c_uint32(ld), ctypes.c_uint32(d),
                                       ctypes.c_uint32(k), _p(out), _p(sq)))
        del pts
        return (out, sq) if return_sq_dist else out

    def nearest_neighbors_sharded(self, points, k: int, distance="euclidean", device: bool = False):
        """`nearest_neighbors` over a sharded point set (`scanrs_nearest_neighbors_sharded`, knn.rs:112-166):
        COLLECTIVE, every rank calls it with the same k and distance. points as for `knn_sharded`. Returns (indices, distances) of the
        rank's cells, n_local x min(k, n - 1) with n the global number of cells: GLOBAL indices, nearest first - what
        `nearest_neighbors` of the whole point set returns for those rows, in every bit. On an unsharded handle it is
        `nearest_neighbors` / `nearest_neighbors_device` of the given points."""
        n_local = int(self.shape()[1])
        pts, ld, d = _sharded_points(points, device)
        k = int(k)
        idx = np.full((n_local, k), 0xFFFFFFFF, dtype=np.uint32)
        dist = np.full((n_local, k), np.inf, dtype=np.float64)
        _check(_lib.scanrs_nearest_neighbors_sharded(self._h, pts if device else _p(pts), ctypes.c_int(1 if device else 0), ctypes.c_uint32(ld), ctypes.c_uint32(d),
                                                     ctypes.c_uint32(k), ctypes.c_int(_distance_type(distance)), _p(idx), _p(dist)))
        del pts
        n = int(getattr(self, "_outer_global", 0) or n_local)
        k_eff = min(k, max(n - 1, 0))
        return np.ascontiguousarray(idx[:, :k_eff]), np.ascontiguousarray(dist[:, :k_eff])

    def profile_enable(self, on: bool = True):
        _check(_lib.scanrs_profile_enable(self._h, ctypes.c_int(int(on))))

    def profile_reset(self):
        _check(_lib.scanrs_profile_reset(self._h))

    def profile_get(self):
        arr = (_KernelStat * 64)()
        n = ctypes.c_uint32()
        _check(_lib.scanrs_profile_get(self._h, arr, ctypes.c_uint32(64), ctypes.byref(n)))
        return {
            arr[i].name.decode(): {
                "launches": int(arr[i].launches),
                "total_ms": float(arr[i].total_ms),
                "algorithmic_bytes": float(arr[i].algorithmic_bytes),
                "onchip_gather_bytes": float(arr[i].onchip_gather_bytes),
            }
            for i in range(min(int(n.value), 64))
        }

    def sync(self):
        _check(_lib.scanrs_mat_sync(self._h))

    def set_panel_precision(self, precision: int):
        """0 = f64 panels (default, the reference's arithmetic); 1 = f32 gather panels with f64 sums (opt-in fast mode)."""
        _check(_lib.scanrs_mat_set_panel_precision(self._h, ctypes.c_int(precision)))
        return self

    def set_spmm_path(self, path: int):
        """0 auto, 1 plain gather kernel, 2 L2-blocked gather kernel, 3 hybrid LDS tiles + gather (see scanrs_mat_set_spmm_path)."""
        _check(_lib.scanrs_mat_set_spmm_path(self._h, ctypes.c_int(path)))
        return self

    def set_option(self, key: str, value: float):
        """Tuning options of the handle (include/scanrs_amd.h, scanrs_mat_set_option)."""
        _check(_lib.scanrs_mat_set_option(self._h, key.encode(), ctypes.c_double(value)))
        return self

    def counter(self, key: str) -> int:
        v = ctypes.c_uint64()
        _check(_lib.scanrs_mat_get_counter(self._h, key.encode(), ctypes.byref(v)))
        return int(v.value)

    def chol_rinv(self, g, rows: int, pass_no: int = 0):
        """One factor step of the device-side CholeskyQR (scanrs_mat_chol_rinv): (rinv, done, status, err, shift)."""
        g = _f64(g)
        n = g.shape[0]
        rinv = np.zeros((n, n))
        done, status = ctypes.c_int(), ctypes.c_int()
        err, shift = ctypes.c_double(), ctypes.c_double()
        _check(_lib.scanrs_mat_chol_rinv(self._h, _p(g), ctypes.c_uint32(n), ctypes.c_uint64(rows), ctypes.c_int(pass_no), _p(rinv),
                                         ctypes.byref(done), ctypes.byref(status), ctypes.byref(err), ctypes.byref(shift)))
        return rinv, int(done.value), int(status.value), float(err.value), float(shift.value)

    def debug_dense_gram(self, x, n: int, y, mcols: int, rows: int, c, route: int = 0, skip: bool = False):
        """C = X^T Y through one Gram kernel (scanrs_debug_dense_gram). x, y: (rows_alloc, ld) arrays whose first `rows` rows and
        n / mcols columns are the operands (y None: Y is X itself); c: the (n, mcols) buffer the kernels write into. Returns the
        buffer as it comes back."""
        x = _f64(x)
        y = None if y is None else _f64(y)
        c = np.array(c, dtype=np.float64, order="C")
        if c.shape != (n, mcols) or (y is not None and y.shape[0] != x.shape[0]):
            raise ValueError("c must be n x mcols, x and y must hold the same number of rows")
        _check(_lib.scanrs_debug_dense_gram(self._h, ctypes.c_int(route), _p(x), ctypes.c_uint32(x.shape[1]), ctypes.c_uint32(n), _p(y),
                                            ctypes.c_uint32(x.shape[1] if y is None else y.shape[1]), ctypes.c_uint32(mcols),
                                            ctypes.c_uint64(rows), ctypes.c_uint64(x.shape[0]), ctypes.c_int(int(skip)), _p(c)))
        return c

    def debug_dense_gemm(self, x, n: int, w, mcols: int, rows: int, out, alpha: float = 1.0, beta: float = 0.0, cin=None,
                         in_place: bool = False, route: int = 0, x_skew: int = 0, skip: bool = False):
        """Out = beta Cin + alpha X W through one GEMM kernel (scanrs_debug_dense_gemm). x: (rows_alloc, ldx), w: (n, ldw),
        out: (rows_alloc, ldo), cin: (rows_alloc, ldc) or None; in_place: Cin is Out's device buffer. Returns the whole out buffer."""
        x, w = _f64(x), _f64(w)
        cin = None if cin is None else _f64(cin)
        out = np.array(out, dtype=np.float64, order="C")
        if out.shape[0] != x.shape[0] or w.shape[0] != n or (cin is not None and cin.shape[0] != x.shape[0]):
            raise ValueError("x, out and cin must hold the same number of rows, w must hold n")
        ldc = out.shape[1] if in_place else (cin.shape[1] if cin is not None else 0)
        _check(_lib.scanrs_debug_dense_gemm(self._h, ctypes.c_int(route), _p(x), ctypes.c_int(x_skew), ctypes.c_uint32(x.shape[1]),
                                            ctypes.c_uint32(n), _p(w), ctypes.c_uint32(w.shape[1]), ctypes.c_uint32(mcols), ctypes.c_uint64(rows),
                                            ctypes.c_uint64(x.shape[0]), ctypes.c_double(alpha), ctypes.c_double(beta), _p(cin),
                                            ctypes.c_uint32(ldc), _p(out), ctypes.c_uint32(out.shape[1]), ctypes.c_int(int(in_place)),
                                            ctypes.c_int(int(skip))))
        return out

    def debug_weighted_colsum(self, b, x, l: int, w, xc=None):
        """w = B^T X[:, :l] (scanrs_debug_weighted_colsum). b: (n, rank), x: (n, ldx), w: (rank, ldw), xc: (n, ldc) or None.
        Returns (w, xc) as the buffers come back."""
        b, x = _f64(b), _f64(x)
        w = np.array(w, dtype=np.float64, order="C")
        xc = None if xc is None else np.array(xc, dtype=np.float64, order="C")
        if b.shape[0] != x.shape[0] or w.shape[0] != b.shape[1] or (xc is not None and xc.shape[0] != x.shape[0]):
            raise ValueError("b, x and xc must hold the same number of rows, w one row per column of b")
        _check(_lib.scanrs_debug_weighted_colsum(self._h, _p(b), ctypes.c_uint32(b.shape[1]), _p(x), ctypes.c_uint32(x.shape[1]),
                                                 ctypes.c_uint64(x.shape[0]), ctypes.c_uint32(l), _p(w), ctypes.c_uint32(w.shape[1]), _p(xc),
                                                 ctypes.c_uint32(0 if xc is None else xc.shape[1])))
        return w, xc

    def target_umi(self) -> float:
        t = ctypes.c_double()
        _check(_lib.scanrs_mat_target_umi(self._h, ctypes.byref(t)))
        return float(t.value)


# explicit prototypes of the entry points that take doubles or 64-bit integers by value (ctypes' default conversion is for ints)
_lib.scanrs_mat_set_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_double]
_lib.scanrs_mat_set_option.restype = ctypes.c_int
_lib.scanrs_set_global_option.argtypes = [ctypes.c_char_p, ctypes.c_double]
_lib.scanrs_set_global_option.restype = ctypes.c_int
_lib.scanrs_mat_get_counter.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)]
_lib.scanrs_mat_get_counter.restype = ctypes.c_int
_lib.scanrs_debug_wait_never.argtypes = [ctypes.c_double]
_lib.scanrs_debug_wait_never.restype = ctypes.c_int
_lib.scanrs_reserve_device_memory.argtypes = [ctypes.c_uint64]
_lib.scanrs_reserve_device_memory.restype = ctypes.c_int
_lib.scanrs_adaptive_export_free.argtypes = [ctypes.c_void_p]
_lib.scanrs_adaptive_export_free.restype = None


GRAM_WAVE, GRAM_VEC, GRAM_TILED = 1, 2, 3  # SCANRS_DENSE_GRAM_*
GEMM_WAVE, GEMM_TILED, GEMM_SKINNY_LDS, GEMM_DIRECT = 1, 2, 3, 4  # SCANRS_DENSE_GEMM_*


def debug_dense_route(kind: str, n: int, m: int, rows: int, ldx: int, ldy: int = 0, x_aligned16: bool = True, side: bool = False,
                      flag: bool = False):
    """What the dense dispatcher would choose (scanrs_debug_dense_route, host only): (route, nt, groups). kind "gram": flag = a skip
    flag is set; kind "gemm": flag = the "gemm_direct" option."""
    route, nt, groups = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_uint32()
    _check(_lib.scanrs_debug_dense_route(ctypes.c_int({"gram": 0, "gemm": 1}[kind]), ctypes.c_uint32(n), ctypes.c_uint32(m), ctypes.c_uint64(rows),
                                         ctypes.c_uint32(ldx), ctypes.c_uint32(ldy), ctypes.c_int(int(x_aligned16)), ctypes.c_int(int(side)),
                                         ctypes.c_int(int(flag)), ctypes.byref(route), ctypes.byref(nt), ctypes.byref(groups)))
    return int(route.value), int(nt.value), int(groups.value)


def debug_knn_filter_params() -> dict:
    """The constants of the kNN filter (scanrs_debug_knn_filter_params, host only): gamma, cap, dmax, k_max, nq_min and the magnitude
    window coord_min <= max |coordinate| <= coord_max."""
    gamma, cmin, cmax = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    cap, dmax, k_max, nq_min = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    _check(_lib.scanrs_debug_knn_filter_params(ctypes.byref(gamma), ctypes.byref(cap), ctypes.byref(dmax), ctypes.byref(k_max),
                                               ctypes.byref(nq_min), ctypes.byref(cmin), ctypes.byref(cmax)))
    return {"gamma": gamma.value, "cap": int(cap.value), "dmax": int(dmax.value), "k_max": int(k_max.value), "nq_min": int(nq_min.value),
            "coord_min": cmin.value, "coord_max": cmax.value}


def debug_knn_filter(queries, points, tau, stride: int = 1):
    """One pass of the kNN filter (scanrs_debug_knn_filter) over rows 0, stride, ... of `points` with the thresholds `tau` (squared
    distances): (cnt[n_q], cand[n_q, cap]); a list is valid up to min(cnt, cap), unwritten slots hold UINT32_MAX."""
    q, p = _f64(np.atleast_2d(queries)), _f64(np.atleast_2d(points))
    t = _f64(tau).reshape(-1)
    if q.shape[1] != p.shape[1] or t.shape[0] != q.shape[0]:
        raise ScanrsError(1, "Dimension mismatch")
    cap = debug_knn_filter_params()["cap"]
    cnt, cand = np.zeros(q.shape[0], dtype=np.uint32), np.zeros((q.shape[0], cap), dtype=np.uint32)
    _check(_lib.scanrs_debug_knn_filter(_p(q), ctypes.c_uint64(q.shape[0]), _p(p), ctypes.c_uint64(p.shape[0]), ctypes.c_uint32(q.shape[1]),
                                        _p(t), ctypes.c_uint64(int(stride)), _p(cnt), _p(cand)))
    return cnt, cand


def debug_knn_last_stats() -> dict:
    """What the last knn / knn_device / find_nn of the process did (scanrs_debug_knn_last_stats): {"filtered", "first_stride",
    "rounds": [{"stride", "points", "cand_sum", "cand_max", "overflowed"}, ...]}."""
    cap = 64
    filtered, first, n = ctypes.c_int(), ctypes.c_uint64(), ctypes.c_uint32()
    st, pts, cs = (np.zeros(cap, dtype=np.uint64) for _ in range(3))
    cm, ov = (np.zeros(cap, dtype=np.uint32) for _ in range(2))
    _check(_lib.scanrs_debug_knn_last_stats(ctypes.byref(filtered), ctypes.byref(first), ctypes.byref(n), ctypes.c_uint32(cap), _p(st), _p(pts),
                                            _p(cs), _p(cm), _p(ov)))
    rounds = [{"stride": int(st[i]), "points": int(pts[i]), "cand_sum": int(cs[i]), "cand_max": int(cm[i]), "overflowed": int(ov[i])}
              for i in range(min(int(n.value), cap))]
    return {"filtered": bool(filtered.value), "first_stride": int(first.value), "rounds": rounds}


def set_global_option(key: str, value: float):
    """Process-wide options of the entry points that take no handle (include/scanrs_amd.h, scanrs_set_global_option)."""
    _check(_lib.scanrs_set_global_option(key.encode(), ctypes.c_double(value)))


def init():
    """`scanrs_init`: load the device code and start the one-off table computation now instead of inside the first call."""
    _check(_lib.scanrs_init())


def reserve_device_memory(n_bytes: int):
    """`scanrs_reserve_device_memory`: one allocation now that the library's later large buffers are carved from."""
    _check(_lib.scanrs_reserve_device_memory(ctypes.c_uint64(int(n_bytes))))


def release_cached_memory():
    """Give the device blocks the library keeps for reuse back to the driver (include/scanrs_amd.h, "device_cache_fraction")."""
    _check(_lib.scanrs_release_cached_memory())


def cached_memory_bytes() -> int:
    n = ctypes.c_uint64()
    _check(_lib.scanrs_cached_memory_bytes(ctypes.byref(n)))
    return int(n.value)


def device_memory_in_use() -> int:
    n = ctypes.c_uint64()
    _check(_lib.scanrs_device_memory_in_use(ctypes.byref(n)))
    return int(n.value)


def debug_arena_selftest(rounds: int = 20000, seed: int = 1):
    """The bookkeeping of a device-memory reserve driven on a made-up address range (no device needed): raises when blocks overlap,
    holes fail to merge or the arena is not whole at the end."""
    _lib.scanrs_debug_arena_selftest.argtypes = [ctypes.c_uint32, ctypes.c_uint64]
    _lib.scanrs_debug_arena_selftest.restype = ctypes.c_int
    _check(_lib.scanrs_debug_arena_selftest(ctypes.c_uint32(rounds), ctypes.c_uint64(seed)))


def debug_wait_never(timeout_s: float):
    """The library's bounded wait on an event that is never signalled (no device needed): raises ScanrsError(DEVICE) after
    `timeout_s` seconds, with the report of a real stuck wait."""
    _check(_lib.scanrs_debug_wait_never(ctypes.c_double(timeout_s)))


# ---- scan-rs/src/normalization.rs ---------------------------------------------------------------
def normalize(mat: AdaptiveMat, norm: int) -> AdaptiveMat:
    """`normalize(mat, norm)` (normalization.rs:46-69); consumes `mat` like the reference, returns it."""
    _check(_lib.scanrs_normalize(mat._h, ctypes.c_int(norm), None))
    return mat


def normalize_with_size_factor(mat: AdaptiveMat, norm: int, size_factors=None) -> AdaptiveMat:
    """normalization.rs:72-102."""
    sf = None
    if size_factors is not None:
        sf = np.ascontiguousarray(size_factors, dtype=np.uint32)
        if sf.shape[0] != mat.cols():
            raise ScanrsError(1, "Size of the size factor and matrix columns dont match.")
    _check(_lib.scanrs_normalize(mat._h, ctypes.c_int(norm), _p(sf)))
    return mat


def log_normalize_with_size_factor(mat: AdaptiveMat, umi_count_sum: Optional[float], log_fn: int, size_factors=None):
    """normalization.rs:138-178 (no centre/scale)."""
    sf = None
    if size_factors is not None:
        sf = np.ascontiguousarray(size_factors, dtype=np.uint32)
        if sf.shape[0] != mat.cols():
            raise ScanrsError(1, "Size of the size factor and matrix columns dont match.")
    _check(
        _lib.scanrs_log_normalize(
            mat._h, ctypes.c_double(-1.0 if umi_count_sum is None else float(umi_count_sum)), ctypes.c_int(log_fn), _p(sf)))
    return mat


def log1p_normalize_fixed_point(mat: AdaptiveMat, log_fn: int, base: int, exponent: int) -> AdaptiveMat:
    """normalization.rs:191-213."""
    _check(_lib.scanrs_log1p_normalize_fixed_point(mat._h, ctypes.c_int(log_fn), ctypes.c_uint32(base), ctypes.c_uint32(exponent)))
    return mat


def binom_deviance_resid(mat: AdaptiveMat) -> AdaptiveMat:
    return normalize(mat, Normalization.BinomialDeviance)


def binom_pearson_resid(mat: AdaptiveMat) -> AdaptiveMat:
    return normalize(mat, Normalization.BinomialPearson)


# ---- scan-rs/src/dim_red ---------------------------------------------------------------------------
def omega_fill(seed: int, count: int) -> np.ndarray:
    out = np.zeros(count)
    _check(_lib.scanrs_omega_fill(ctypes.c_uint64(seed), ctypes.c_uint64(count), _p(out)))
    return out


def _snoop_arg(snoop):
    if snoop is None:
        return None, None
    s = snoop._struct()
    return ctypes.byref(s), s


class BkSvd:
    """`BkSvd` (dim_red/bk_svd.rs:16-53)."""

    def __init__(self, k_multiplier: float = 2.0, n_iter: int = 5):
        self.k_multiplier, self.n_iter = k_multiplier, n_iter

    def run_pca(self, matrix: AdaptiveMat, k: int, omega=None, snoop: Optional[AtomicSnoop] = None, seed: int = 0, out=None):
        """Returns (u rows x k, s k, v cols x k) — `PcaResult` (dim_red/mod.rs:47). `out=(u, v)`: the factors are written into
        these C-contiguous float64 arrays of shape (rows, k) / (cols, k) — the C ABI's own form (caller-allocated buffers,
        include/scanrs_amd.h) — instead of fresh ones."""
        r, c = matrix.shape()
        if out is not None:
            u, v = out
            for a_, shp in ((u, (r, k)), (v, (c, k))):
                if not (isinstance(a_, np.ndarray) and a_.dtype == np.float64 and a_.flags.c_contiguous and a_.shape == shp):
                    raise ScanrsError(6, f"out arrays must be C-contiguous float64 of shape {shp}")
            s = np.zeros(max(k, 0))
        else:
            u, s, v = np.zeros((r, max(k, 0))), np.zeros(max(k, 0)), np.zeros((c, max(k, 0)))
        om = None if omega is None else _f64(omega)
        sref, _keep = _snoop_arg(snoop)
        _check(
            _lib.scanrs_pca_bk(
                matrix._h, ctypes.c_uint32(k), ctypes.c_double(self.k_multiplier), ctypes.c_uint32(self.n_iter),
                ctypes.c_uint64(seed), _p(om), sref, _p(u), _p(s), _p(v)))
        return u, s, v

    run_pca_cancellable = run_pca

    def run_pca_device(self, matrix: AdaptiveMat, k: int, omega=None, snoop: Optional[AtomicSnoop] = None, seed: int = 0):
        """The same call with U and V left in device memory: returns (s, PcaResultDevice). The factors are reached through
        `scanrs_pca_result_device` (pointers + leading dimensions) — for a device consumer such as `knn_device`."""
        s = np.zeros(max(k, 0))
        om = None if omega is None else _f64(omega)
        sref, _keep = _snoop_arg(snoop)
        _check(
            _lib.scanrs_pca_bk(
                matrix._h, ctypes.c_uint32(k), ctypes.c_double(self.k_multiplier), ctypes.c_uint32(self.n_iter),
                ctypes.c_uint64(seed), _p(om), sref, None, _p(s), None))
        return s, pca_result_device(matrix)


class Comm:
    """`scanrs_comm`: the library's RCCL communicator of the one-process-per-GPU form. Rank 0 draws the id with
    `Comm.unique_id()` and the host program hands the 128 bytes to the other ranks (bench.py: a torch.distributed
    broadcast on the gloo control plane); every rank then builds `Comm(id, rank, world)` with its device current."""

    ID_BYTES = 128

    @staticmethod
    def unique_id() -> bytes:
        buf = (ctypes.c_uint8 * Comm.ID_BYTES)()
        _check(_lib.scanrs_comm_get_unique_id(buf))
        return bytes(buf)

    def __init__(self, uid: bytes, rank: int, world: int):
        if len(uid) != Comm.ID_BYTES:
            raise ScanrsError(6, "unique id must be 128 bytes")
        self.rank, self.world = int(rank), int(world)
        self._c = ctypes.c_void_p()
        buf = (ctypes.c_uint8 * Comm.ID_BYTES).from_buffer_copy(uid)
        _check(_lib.scanrs_comm_create(buf, ctypes.c_uint32(rank), ctypes.c_uint32(world), ctypes.byref(self._c)))

    def info(self) -> dict:
        """`scanrs_comm_info`: ranks / this rank as RCCL itself counts them (ncclCommCount, ncclCommUserRank) and the sum all-reduces
        that went through this communicator so far."""
        n, r = ctypes.c_uint32(), ctypes.c_uint32()
        calls, nbytes = ctypes.c_uint64(), ctypes.c_uint64()
        _check(_lib.scanrs_comm_info(self._c, ctypes.byref(n), ctypes.byref(r), ctypes.byref(calls), ctypes.byref(nbytes)))
        return {"rccl_nranks": int(n.value), "rccl_rank": int(r.value), "allreduce_calls": int(calls.value), "allreduce_bytes": int(nbytes.value)}

    def close(self):
        if getattr(self, "_c", None) is not None and self._c:
            _lib.scanrs_comm_free(self._c)
            self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiMat:
    """`scanrs_multi`: the single-process multi-GPU form (one handle for the whole matrix, the library shards it by
    nonzeros over `devices` and drives every shard from its own host thread). `devices` may repeat an id."""

    def __init__(self, rows, cols, storage, indptr, indices, values, n_shards: int, devices=None):
        ip = np.ascontiguousarray(indptr, dtype=np.uint64)
        ix = np.ascontiguousarray(indices, dtype=np.uint32)
        vv = np.ascontiguousarray(values, dtype=np.uint32)
        self.rows, self.cols, self.storage, self.n_shards = int(rows), int(cols), int(storage), int(n_shards)
        dv = None if devices is None else (ctypes.c_int * n_shards)(*[int(d) for d in devices])
        self._h = ctypes.c_void_p()
        _check(_lib.scanrs_multi_create(ctypes.c_uint64(rows), ctypes.c_uint64(cols), ctypes.c_int(storage), _p(ip), _p(ix), _p(vv),
                                        ctypes.c_uint32(n_shards), dv, ctypes.byref(self._h)))

    @classmethod
    def _from_handle(cls, handle) -> "MultiMat":
        """Takes over a `scanrs_multi` handle (the results of select_rows / select_cols / partition_on_thresholds)."""
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p(handle)
        n, st = ctypes.c_uint32(), ctypes.c_int()
        r, c = ctypes.c_uint64(), ctypes.c_uint64()
        _check(_lib.scanrs_multi_n_shards(self._h, ctypes.byref(n)))
        _check(_lib.scanrs_multi_shape(self._h, ctypes.byref(r), ctypes.byref(c), None, ctypes.byref(st)))
        self.rows, self.cols, self.storage, self.n_shards = int(r.value), int(c.value), int(st.value), int(n.value)
        return self

    @staticmethod
    def _devices_arg(n_shards: int, devices):
        if devices is None:
            return None
        devices = [int(d) for d in devices]
        if len(devices) != int(n_shards):
            raise ScanrsError(6, "one device id per shard is required")
        return (ctypes.c_int * max(len(devices), 1))(*devices)

    @classmethod
    def from_csmat_inner(cls, rows, cols, storage, indptr, indices, data, n_shards: int, devices=None) -> "MultiMat":
        """`scanrs_multi_create_inner`: the matrix in the reference's own orientation (genes x cells CSR, mat.rs:68-124),
        its INNER dimension sharded over the devices. The result has the same rows x cols and the OTHER storage flag (cells sharded),
        and equals `MultiMat` of the host-transposed triplet bit for bit; nothing is transposed on the host and every nonzero is
        uploaded once. `devices` may repeat an id."""
        ip = np.ascontiguousarray(indptr, dtype=np.uint64)
        ix = np.ascontiguousarray(indices, dtype=np.uint32)
        vv = np.ascontiguousarray(data, dtype=np.uint32)
        n_outer = rows if storage == CSR else cols
        if ip.shape[0] != n_outer + 1:
            raise ScanrsError(6, "indptr length does not match the outer dimension")
        if ix.shape[0] != vv.shape[0] or int(ip[-1]) != ix.shape[0]:
            raise ScanrsError(6, "indices/data length does not match indptr")
        h = ctypes.c_void_p()
        _check(_lib.scanrs_multi_create_inner(ctypes.c_uint64(rows), ctypes.c_uint64(cols), ctypes.c_int(storage), _p(ip), _p(ix), _p(vv),
                                              ctypes.c_uint32(n_shards), cls._devices_arg(n_shards, devices), ctypes.byref(h)))
        return cls._from_handle(h.value)

    @classmethod
    def from_adaptive_vecs_inner(cls, rows, cols, storage, vecs, n_shards: int, devices=None) -> "MultiMat":
        """`scanrs_multi_create_adaptive_inner`: the same from the mappings `AdaptiveMat.from_adaptive_vecs` takes, one per outer
        vector (mat.rs:68-90; what read_adaptive_csr_matrix holds, hdf5-io/src/matrix.rs:119-192). The compressed buffers of a slab are
        uploaded and expanded on its device."""
        n, table, _keep = _adaptive_table(vecs)
        h = ctypes.c_void_p()
        _check(_lib.scanrs_multi_create_adaptive_inner(ctypes.c_uint64(rows), ctypes.c_uint64(cols), ctypes.c_int(storage), table, ctypes.c_uint64(n),
                                                       ctypes.c_uint32(n_shards), cls._devices_arg(n_shards, devices), ctypes.byref(h)))
        return cls._from_handle(h.value)

    @classmethod
    def from_file(cls, path, n_shards: int, devices=None, retain_feature_like=None, shrink_row=None) -> "MultiMat":
        """`scanrs_multi_create_from_file` (cmd.rs:61-70): a 10x `.h5` through `read_adaptive_csr_matrix`, anything else through
        `load_mtx`, then `from_csmat_inner` on the CSR arrays: genes x cells, CSC, the cells sharded."""
        h = ctypes.c_void_p()
        rfl = None if retain_feature_like is None else str(retain_feature_like).encode()
        _check(_lib.scanrs_multi_create_from_file(str(path).encode(), rfl, ctypes.c_int64(-1 if shrink_row is None else int(shrink_row)),
                                                  ctypes.c_uint32(n_shards), cls._devices_arg(n_shards, devices), ctypes.byref(h), None))
        return cls._from_handle(h.value)

    def create_info(self) -> dict:
        """`scanrs_multi_create_info`: what the inner-sharding constructor did. slab_bounds (n_shards + 1: the outer vectors every
        shard uploaded), moved (n_shards x n_shards: stored entries of slab s that lie in shard d's range, stored zeros included) and
        uploaded_bytes per shard. ScanrsError on a MultiMat that no such constructor made."""
        n = self.n_shards
        sb, mv, up = np.zeros(n + 1, dtype=np.uint64), np.zeros((n, n), dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        _check(_lib.scanrs_multi_create_info(self._h, _p(sb), _p(mv), _p(up)))
        return {"slab_bounds": sb, "moved": mv, "uploaded_bytes": up}

    def _shard_handle(self, i: int) -> ctypes.c_void_p:
        """The `scanrs_mat` handle of shard i (`scanrs_multi_shard`); it stays the MultiMat's own."""
        h = ctypes.c_void_p()
        _check(_lib.scanrs_multi_shard(self._h, ctypes.c_uint32(i), ctypes.byref(h), None, None, None))
        return h

    def shard_csmat(self, i: int):
        """`scanrs_mat_to_csmat` of shard i: (indptr u64, indices u32, data u32) of its own outer vectors."""
        h = self._shard_handle(i)
        r, c, nnz = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(_lib.scanrs_mat_shape(h, ctypes.byref(r), ctypes.byref(c)))
        _check(_lib.scanrs_mat_nnz(h, ctypes.byref(nnz)))
        indptr = np.zeros((r.value if self.storage == CSR else c.value) + 1, dtype=np.uint64)
        indices, data = np.zeros(nnz.value, dtype=np.uint32), np.zeros(nnz.value, dtype=np.uint32)
        _check(_lib.scanrs_mat_to_csmat(h, _p(indptr), _p(indices), _p(data)))
        return indptr, indices, data

    def shape(self):
        """[rows, cols] of the whole matrix (`scanrs_multi_shape`)."""
        r, c = ctypes.c_uint64(), ctypes.c_uint64()
        _check(_lib.scanrs_multi_shape(self._h, ctypes.byref(r), ctypes.byref(c), None, None))
        return [int(r.value), int(c.value)]

    def nnz(self) -> int:
        n = ctypes.c_uint64()
        _check(_lib.scanrs_multi_shape(self._h, None, None, ctypes.byref(n), None))
        return int(n.value)

    def to_csmat(self):
        """`scanrs_multi_to_csmat`: (indptr u64, indices u32, data u32) of the whole matrix, the shards concatenated."""
        rows, cols = self.shape()
        nnz = self.nnz()
        indptr = np.zeros((rows if self.storage == CSR else cols) + 1, dtype=np.uint64)
        indices, data = np.zeros(nnz, dtype=np.uint32), np.zeros(nnz, dtype=np.uint32)
        _check(_lib.scanrs_multi_to_csmat(self._h, _p(indptr), _p(indices), _p(data)))
        return indptr, indices, data

    def to_scipy(self):
        """The stored counts of the whole matrix as scipy.sparse csr_matrix / csc_matrix (by the storage flag)."""
        import scipy.sparse as sp

        indptr, indices, data = self.to_csmat()
        cls = sp.csr_matrix if self.storage == CSR else sp.csc_matrix
        return cls((data, indices.astype(np.int64), indptr.astype(np.int64)), shape=tuple(self.shape()))

    # -- back into sqz's own type: the whole matrix as AdaptiveVec encodings, in either orientation ----
    def _export(self, kind, major="stored"):
        e = ctypes.c_void_p()
        _check(_lib.scanrs_multi_to_adaptive(self._h, ctypes.c_int(_export_major(major)), ctypes.c_int(_export_kind(kind)), ctypes.byref(e)))
        return e

    def to_adaptive_vecs(self, kind=None, major="stored"):
        """`scanrs_multi_to_adaptive`: the stored counts of the WHOLE matrix as one list of encoded `AdaptiveVec` mappings (see
        `AdaptiveMat.to_adaptive_vecs`), made on the devices. major="stored": one per outer vector in global order, what
        `AdaptiveMat.from_csmat(*mm.to_csmat()).to_adaptive_vecs(kind)` returns. major="inner", the inverse of
        `from_adaptive_vecs_inner`: one per INNER position (per gene, for a cell-sharded genes x cells matrix), each spanning all
        shards, with len = the sharded extent - what `from_adaptive_vecs` takes with the OTHER storage flag, byte for byte the export
        of the host-transposed whole matrix whatever the shards."""
        e = self._export(kind, major)
        try:
            return _export_vecs(e)
        finally:
            _lib.scanrs_adaptive_export_free(e)

    def adaptive_info(self, kind=None, major="stored"):
        """(total_bytes, kind_counts) of `to_adaptive_vecs(kind, major)`, over the whole table."""
        e = self._export(kind, major)
        try:
            return _export_totals(e)
        finally:
            _lib.scanrs_adaptive_export_free(e)

    def export_info(self, kind=None, major="inner") -> dict:
        """`scanrs_adaptive_export_multi_info` of `to_adaptive_vecs(kind, major)`: slab_bounds (n_shards + 1: the table entries shard d
        encoded), moved (n_shards x n_shards: nonzeros of source shard s in slab d) and arena_bytes per shard (the encoded bytes that
        crossed the host link)."""
        e = self._export(kind, major)
        try:
            return _export_multi_info(e)
        finally:
            _lib.scanrs_adaptive_export_free(e)

    def _select(self, fn, idx) -> "MultiMat":
        idx = _index_list(idx)
        h = ctypes.c_void_p()
        _check(fn(self._h, _p(idx), ctypes.c_uint64(idx.shape[0]), ctypes.byref(h)))
        return MultiMat._from_handle(h.value)

    def select_rows(self, idx) -> "MultiMat":
        """`scanrs_multi_select_rows`: a new MultiMat on the same devices (shards not rebalanced: `.rebalance(consume=True)` on the
        result does that). A list along the sharded dimension (the rows of a CSR matrix, the columns of a CSC one) must not descend
        (any order: `gather_outer`); along the other any order, repeats allowed."""
        return self._select(_lib.scanrs_multi_select_rows, idx)

    def select_cols(self, idx) -> "MultiMat":
        """`scanrs_multi_select_cols` (see `select_rows`)."""
        return self._select(_lib.scanrs_multi_select_cols, idx)

    def gather_outer(self, idx, n_shards: Optional[int] = None, devices=None) -> "MultiMat":
        """`scanrs_multi_gather_outer`: the outer vectors `idx` of the WHOLE matrix (positions along the sharded
        dimension: the rows of a CSR matrix, the columns of a CSC one; any order, repeats allowed), in list order, as a freshly
        balanced MultiMat over `n_shards` shards (None: as many as this one) on `devices` (None: this one's when the shard count
        stays, else 0 .. n_shards-1). It equals `MultiMat(...)` of the selected triplet bit for bit; no nonzero crosses the host link."""
        idx = _index_list(idx, "idx: ")
        if n_shards is None:
            n_shards = self.n_shards
            if devices is None:
                devices = [dev for dev, _lo, _hi in self.shard_ranges()]
        h = ctypes.c_void_p()
        _check(_lib.scanrs_multi_gather_outer(self._h, _p(idx), ctypes.c_uint64(idx.shape[0]), ctypes.c_uint32(int(n_shards)),
                                              self._devices_arg(n_shards, devices), ctypes.byref(h)))
        return MultiMat._from_handle(h.value)

    def rebalance(self, n_shards: Optional[int] = None, devices=None, consume: bool = False) -> "MultiMat":
        """`scanrs_multi_rebalance`: the same matrix cut anew by nonzeros (the identity list of `gather_outer`), e.g. after a filter
        left the shards unequal. n_shards=None: as many shards as this one, on its devices. consume=True: this MultiMat - the
        unbalanced intermediate of `mm.partition_on_thresholds(rt, ct)[0].rebalance(consume=True)` - is closed once the call
        returns or fails."""
        n = 0 if n_shards is None else int(n_shards)
        if n_shards is not None and n == 0:
            raise ScanrsError(6, "n_shards: 1 <= n_shards <= 16 is required (0 given)")
        h = ctypes.c_void_p()
        try:
            _check(_lib.scanrs_multi_rebalance(self._h, ctypes.c_uint32(n), None if n == 0 else self._devices_arg(n, devices), ctypes.byref(h)))
        finally:
            if consume:
                self.close()
        return MultiMat._from_handle(h.value)

    def balance(self) -> dict:
        """`scanrs_multi_balance`: {"shard_nnz": nonzeros per shard, "imbalance": max / mean of them (1.0 without nonzeros)}."""
        nnz, imb = np.zeros(max(self.n_shards, 1), dtype=np.uint64), ctypes.c_double()
        _check(_lib.scanrs_multi_balance(self._h, _p(nnz), ctypes.byref(imb)))
        return {"shard_nnz": nnz[: self.n_shards], "imbalance": float(imb.value)}

    def gather_info(self) -> dict:
        """`scanrs_multi_gather_info`: what the `gather_outer` / `rebalance` that made this MultiMat did. bounds (n_shards + 1), moved
        (n_src x n_shards nonzeros, from source shard s to shard d) and host_bytes per shard (metadata only: the sources' indptr down,
        the list up). ScanrsError on a MultiMat these calls did not make."""
        n, n_src = self.n_shards, ctypes.c_uint32()
        _check(_lib.scanrs_multi_gather_info(self._h, ctypes.byref(n_src), None, None, None))
        bd, mv, hb = np.zeros(n + 1, dtype=np.uint64), np.zeros((max(n_src.value, 1), max(n, 1)), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
        _check(_lib.scanrs_multi_gather_info(self._h, None, _p(bd), _p(mv), _p(hb)))
        return {"n_src": int(n_src.value), "bounds": bd, "moved": mv[: n_src.value, :n], "host_bytes": hb[:n]}

    def partition_on_thresholds(self, row_threshold: Optional[float], col_threshold: Optional[float], filtered: bool = True,
                                residual: bool = True):
        """`scanrs_multi_partition_on_thresholds`: (filtered, residual, selected_rows, selected_cols) as `AdaptiveMat.partition_on_thresholds`
        gives them, the two matrices as MultiMat objects; every output equals the unsharded call's. The shards keep what the filter
        left them: `.rebalance(consume=True)` on a result cuts it anew and frees the unbalanced intermediate."""
        return _partition_on_thresholds(_lib.scanrs_multi_partition_on_thresholds, self._h, self.shape(), MultiMat._from_handle, row_threshold,
                                        col_threshold, filtered, residual)

    def partition_on_threshold(self, threshold: float):
        return self.partition_on_thresholds(threshold, threshold)

    # -- statistics over a list of columns (`scanrs_multi_sum_rows_u64` ... `scanrs_multi_mean_var_rows`): the dtypes and
    # results of the AdaptiveMat methods; `transposed`: of the transposed matrix
    def _view_rows(self, transposed: bool) -> int:
        return self.shape()[1 if transposed else 0]

    def _head(self, transposed: bool):
        return (self._h, ctypes.c_int(int(transposed)))

    def sum_rows(self, cols, dtype=np.float64, transposed: bool = False):
        return AdaptiveMat._sums_over(self._head(transposed), _lib.scanrs_multi_sum_rows_u64, _lib.scanrs_multi_sum_rows_f64, cols, dtype,
                                      lambda c: self._view_rows(transposed))

    def sum_cols(self, cols, dtype=np.float64, transposed: bool = False):
        return AdaptiveMat._sums_over(self._head(transposed), _lib.scanrs_multi_sum_cols_u64, _lib.scanrs_multi_sum_cols_f64, cols, dtype,
                                      lambda c: c.shape[0])

    def sum_rows_dual(self, cols1, cols2, dtype=np.float64, snoop=None, transposed: bool = False):
        return AdaptiveMat._sum_rows_dual(self._head(transposed), _lib.scanrs_multi_sum_rows_dual_u64, _lib.scanrs_multi_sum_rows_dual_f64,
                                          lambda: self._view_rows(transposed), cols1, cols2, dtype, snoop)

    def mean_rows(self, cols, transposed: bool = False):
        return AdaptiveMat._mean_rows(self._head(transposed), _lib.scanrs_multi_mean_rows, lambda: self._view_rows(transposed), cols)

    def mean_var_rows(self, cols, transposed: bool = False):
        return AdaptiveMat._mean_var_rows(self._head(transposed), _lib.scanrs_multi_mean_var_rows, lambda: self._view_rows(transposed), cols)

    def compose_scale_axis(self, axis: int, factors):
        """`compose_map(ScaleAxis::new(Axis(axis), factors))` on every shard (`scanrs_mat_compose_scale_axis`); `factors` spans the whole
        matrix, every shard takes its slice along the sharded dimension."""
        f = _f64(factors)
        if axis not in (0, 1) or f.shape[0] != self.shape()[axis]:
            raise ScanrsError(1, "Dimension mismatch")
        sharded_axis = 0 if self.storage == CSR else 1
        for i, (_dev, lo, hi) in enumerate(self.shard_ranges()):
            h = self._shard_handle(i)
            part = np.ascontiguousarray(f[lo:hi]) if axis == sharded_axis else f
            if part.shape[0] == 0:
                part = np.zeros(1)  # (a shard without vectors: nothing is read)
            _check(_lib.scanrs_mat_compose_scale_axis(h, ctypes.c_int(axis), _p(part)))
        return self

    def _with_shard(self, i: int, fn):
        """fn(shard i as an AdaptiveMat); the handle stays the MultiMat's own."""
        b = AdaptiveMat(self._shard_handle(i).value)
        try:
            return fn(b)
        finally:
            b._h = ctypes.c_void_p()  # borrowed: nothing is freed

    def profile_enable(self, on: bool = True):
        """`scanrs_profile_enable` / `scanrs_profile_reset` on every shard; `profile_get(shard)` reads one shard's kernel classes."""
        for i in range(self.n_shards):
            self._with_shard(i, lambda b: (b.profile_enable(on), b.profile_reset()))
        return self

    def profile_get(self, shard: int = 0) -> dict:
        return self._with_shard(shard, lambda b: b.profile_get())

    def reset_map(self):
        """`scanrs_mat_reset_map` on every shard."""
        for i in range(self.n_shards):
            _check(_lib.scanrs_mat_reset_map(self._shard_handle(i)))
        return self

    def shard_ranges(self):
        out = []
        for i in range(self.n_shards):
            lo, hi, dev = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
            _check(_lib.scanrs_multi_shard(self._h, ctypes.c_uint32(i), None, ctypes.byref(dev), ctypes.byref(lo), ctypes.byref(hi)))
            out.append((dev.value, lo.value, hi.value))
        return out

    def normalize(self, normalization: int, size_factors=None):
        sf = None if size_factors is None else np.ascontiguousarray(size_factors, dtype=np.uint32)
        _check(_lib.scanrs_multi_normalize(self._h, ctypes.c_int(int(normalization)), _p(sf)))
        return self

    def run_pca_bk(self, k: int, k_multiplier: float = 2.0, n_iter: int = 5, omega=None, seed: int = 0, snoop=None):
        u, s, v = np.zeros((self.rows, k)), np.zeros(k), np.zeros((self.cols, k))
        om = None if omega is None else _f64(omega)
        sref, _keep = _snoop_arg(snoop)
        _check(_lib.scanrs_multi_pca_bk(self._h, ctypes.c_uint32(k), ctypes.c_double(k_multiplier), ctypes.c_uint32(n_iter),
                                        ctypes.c_uint64(seed), _p(om), sref, _p(u), _p(s), _p(v)))
        return u, s, v

    def run_pca_rand(self, k: int, l_multiplier: float = 10.0, n_iter: int = 2, omega=None, seed: int = 0):
        u, s, v = np.zeros((self.rows, k)), np.zeros(k), np.zeros((self.cols, k))
        om = None if omega is None else _f64(omega)
        _check(_lib.scanrs_multi_pca_rand(self._h, ctypes.c_uint32(k), ctypes.c_double(l_multiplier), ctypes.c_uint32(n_iter),
                                          ctypes.c_uint64(seed), _p(om), _p(u), _p(s), _p(v)))
        return u, s, v

    def log_normalize(self, umi_count_sum=None, log_fn: int = 3, size_factors=None):
        sf = None if size_factors is None else np.ascontiguousarray(size_factors, dtype=np.uint32)
        _check(_lib.scanrs_multi_log_normalize(self._h, ctypes.c_double(-1.0 if umi_count_sum is None else umi_count_sum),
                                               ctypes.c_int(log_fn), _p(sf)))
        return self

    def knn(self, k: int, points=None, return_sq_dist: bool = False):
        """`nn::knn` over the shards (`scanrs_multi_knn`, nn.rs:38-83): (cells x k) u32 global indices, nearest first,
        equal to `knn` of the whole point set bit for bit; the cells are the sharded dimension. points: a host array over all cells,
        or None: every shard searches the scores its last run_pca_bk / run_pca_rand left on its device (V of a genes x cells CSC
        matrix). With return_sq_dist also the squared distances."""
        cells = self.cols if self.storage == CSC else self.rows
        pts, d, _ = _sharded_points(points, cells=cells)
        out = np.zeros((cells, k), dtype=np.uint32)
        sq = np.zeros((cells, k)) if return_sq_dist else None
        _check(_lib.scanrs_multi_knn(self._h, _p(pts), ctypes.c_uint32(d), ctypes.c_uint32(d), ctypes.c_uint32(k), _p(out), _p(sq)))
        return (out, sq) if return_sq_dist else out

    def nearest_neighbors(self, k: int, points=None, distance="euclidean"):
        """`nearest_neighbors` over the shards (`scanrs_multi_nearest_neighbors`, knn.rs:112-166): (indices u32,
        distances f64), each cells x min(k, cells - 1), global indices, nearest first, equal to `nearest_neighbors` of the whole point
        set in every bit. points: a host array over all cells, or None: every shard searches the scores its last run_pca_bk /
        run_pca_rand left on its device."""
        cells = self.cols if self.storage == CSC else self.rows
        pts, d, _ = _sharded_points(points, cells=cells)
        return _nearest_neighbors_call(_lib.scanrs_multi_nearest_neighbors, int(cells), int(k), self._h, _p(pts), ctypes.c_uint32(d),
                                       ctypes.c_uint32(d), ctypes.c_uint32(k), ctypes.c_int(_distance_type(distance)))

    def comm_info(self, shard: int = 0) -> dict:
        """`scanrs_comm_info` of shard `shard`'s communicator: the sum all-reduces that went through it so far."""
        n, r = ctypes.c_uint32(), ctypes.c_uint32()
        calls, nbytes = ctypes.c_uint64(), ctypes.c_uint64()
        _check(_lib.scanrs_multi_comm_info(self._h, ctypes.c_uint32(shard), ctypes.byref(n), ctypes.byref(r), ctypes.byref(calls), ctypes.byref(nbytes)))
        return {"nranks": int(n.value), "rank": int(r.value), "allreduce_calls": int(calls.value), "allreduce_bytes": int(nbytes.value)}

    def counter(self, key: str, shard: int = 0) -> int:
        """`scanrs_mat_get_counter` of shard `shard` (e.g. "de_shard_tests", "de_shard_allreduces")."""
        v = ctypes.c_uint64()
        _check(_lib.scanrs_mat_get_counter(self._shard_handle(shard), key.encode(), ctypes.byref(v)))
        return int(v.value)

    def set_option(self, key: str, value: float):
        """`scanrs_mat_set_option` on every shard (e.g. "merge_fused")."""
        for i in range(self.n_shards):
            _check(_lib.scanrs_mat_set_option(self._shard_handle(i), key.encode(), ctypes.c_double(value)))
        return self

    def run_pca_irlba(self, k: int, tol: float = 1e-4, max_iter: int = 50, v0=None):
        u, s, v = np.zeros((self.rows, k)), np.zeros(k), np.zeros((self.cols, k))
        v0c = None if v0 is None else _f64(v0)
        mp = ctypes.c_uint32()
        _check(_lib.scanrs_multi_pca_irlba(self._h, ctypes.c_uint32(k), ctypes.c_double(tol), ctypes.c_uint32(max_iter), _p(v0c), None,
                                           _p(u), _p(s), _p(v), ctypes.byref(mp)))
        self.mprod = int(mp.value)
        return u, s, v

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _lib.scanrs_multi_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DevArray:
    """A run of `n` f64 values of device memory at raw address `ptr` as a __cuda_array_interface__ object
    (torch.as_tensor(DevArray(...), device=...) views it without a copy)."""

    def __init__(self, ptr: int, n: int, typestr: str = "<f8"):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr), False), "version": 2}


class PcaResultDevice:
    """Where the last PCA of a handle left its factors in HBM (`scanrs_pca_result_device`): raw device addresses,
    leading dimensions in elements; `u` is rows x k, `v` cols x k. Valid until the handle's next PCA call."""

    def __init__(self, d_u, ld_u, d_v, ld_v, k, rows, cols):
        self.d_u, self.ld_u, self.d_v, self.ld_v, self.k, self.rows, self.cols = d_u, ld_u, d_v, ld_v, k, rows, cols


def pca_result_device(matrix: "AdaptiveMat") -> PcaResultDevice:
    d_u, d_v = ctypes.c_void_p(), ctypes.c_void_p()
    ld_u, ld_v, k = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    _check(_lib.scanrs_pca_result_device(matrix._h, ctypes.byref(d_u), ctypes.byref(ld_u), ctypes.byref(d_v), ctypes.byref(ld_v),
                                         ctypes.byref(k)))
    r, c = matrix.shape()
    return PcaResultDevice(d_u.value, ld_u.value, d_v.value, ld_v.value, k.value, r, c)


def host_knn_merge(da, ia, db, ib):
    """The merge rule of the sharded kNN on the host (`scanrs_host_knn_merge`; scan-rs_amd/csrc/knn_merge.hpp): two lists of k
    (squared distance, index) entries, each ascending by (distance, index) and padded with (+inf, UINT32_MAX), sharing no index ->
    the first k of their union in the same form, as (distances f64, indices u32)."""
    da, db = _f64(np.asarray(da).reshape(-1)), _f64(np.asarray(db).reshape(-1))
    ia = np.ascontiguousarray(np.asarray(ia).reshape(-1), dtype=np.uint32)
    ib = np.ascontiguousarray(np.asarray(ib).reshape(-1), dtype=np.uint32)
    k = int(da.shape[0])
    if not (ia.shape[0] == k and db.shape[0] == k and ib.shape[0] == k):
        raise ScanrsError(6, "the four lists must have the same length k")
    dout, iout = np.zeros(k), np.zeros(k, dtype=np.uint32)
    _check(_lib.scanrs_host_knn_merge(ctypes.c_uint32(k), _p(da), _p(ia), _p(db), _p(ib), _p(dout), _p(iout)))
    return dout, iout


def host_col_moments_plan(max_count: int, links, n_outer: int, n_inner: int, n_wg: int, mode: int):
    """The plan of the fixed-point column moments on the host (`scanrs_host_col_moments_plan`; scan-rs_amd/csrc/col_moments_plan.hpp,
    the source normalize_ops.hip decides by). `links`: the map's links in order, each `(FN_LN_1P | FN_LOG2_1P | FN_LOG10_1P,)` or
    `("scale", fmin_pos, fmax)` / `("scale", fmin_pos, fmax, on_summed_axis)` with the link's smallest positive and its largest
    factor. Returns (accept, e1, e2): the terms are added as rint(f * 2**e1) and rint(f * f * 2**e2)."""
    kinds, on, lo, hi = [], [], [], []
    for l in links:
        if l[0] == "scale":
            kinds.append(1)
            lo.append(float(l[1]))
            hi.append(float(l[2]))
            on.append(int(bool(l[3])) if len(l) > 3 else 1)
        else:
            kinds.append(int(l[0]))
            lo.append(0.0)
            hi.append(0.0)
            on.append(1)
    n = len(kinds)
    ka, oa = (ctypes.c_int * max(n, 1))(*kinds), (ctypes.c_int * max(n, 1))(*on)
    la, ha = (ctypes.c_double * max(n, 1))(*lo), (ctypes.c_double * max(n, 1))(*hi)
    acc, e1, e2 = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _check(_lib.scanrs_host_col_moments_plan(ctypes.c_uint32(int(max_count)), ctypes.c_uint32(n), ka, oa, la, ha, ctypes.c_uint64(int(n_outer)),
                                             ctypes.c_uint64(int(n_inner)), ctypes.c_uint32(int(n_wg)), ctypes.c_int(int(mode)),
                                             ctypes.byref(acc), ctypes.byref(e1), ctypes.byref(e2)))
    return bool(acc.value), int(e1.value), int(e2.value)


# kernel families of a sparse product (counter "spmm_route", host_spmm_route; SCANRS_SPMM_* of scanrs_amd.h)
SPMM_TILES, SPMM_GATHER2D, SPMM_GATHER2D_F32, SPMM_SLICE_WALK, SPMM_SPMV2D, SPMM_SPMV_LDS, SPMM_SPMV, SPMM_GATHER = range(1, 9)
SPMM_SLIVER = 1 << 16


def option_info(scope: int = 0):
    """The library's table of options (`scanrs_host_option_info`): of a handle (scope 0) or of the process (scope 1). One dict per
    key: name, default, lo, hi, open_lo, settable, route_position (position + 1 in the options array of host_spmm_route, 0: not in it)."""
    rows, i = [], 0
    name, d, lo, hi, flags = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_uint32()
    if scope not in (0, 1):
        raise ScanrsError(6, "scope must be 0 (per handle) or 1 (global)")
    while _lib.scanrs_host_option_info(ctypes.c_int(scope), ctypes.c_uint32(i), ctypes.byref(name), ctypes.byref(d), ctypes.byref(lo), ctypes.byref(hi),
                                       ctypes.byref(flags)) == 0:
        rows.append(dict(name=name.value.decode(), default=d.value, lo=lo.value, hi=hi.value, open_lo=bool(flags.value & 1),
                         settable=bool(flags.value & 2), route_position=flags.value >> 8))
        i += 1
    return rows


def host_option_parse(name: str, value: float, scope: int = 0) -> float:
    """What `set_option` (scope 0) or `set_global_option` (scope 1) would store for `value` under the key `name`, or its refusal
    (`scanrs_host_option_parse`): the parser alone, nothing is stored."""
    out = ctypes.c_double()
    _check(_lib.scanrs_host_option_parse(ctypes.c_int(scope), name.encode(), ctypes.c_double(value), ctypes.byref(out)))
    return float(out.value)


def counter_names():
    """The keys of `counter` (`scanrs_host_counter_name`)."""
    names, name = [], ctypes.c_char_p()
    while _lib.scanrs_host_counter_name(ctypes.c_uint32(len(names)), ctypes.byref(name)) == 0:
        names.append(name.value.decode())
    return names


# the options host_spmm_route takes, in the order of the library's array, and their defaults
_SPMM_ROUTE_ROWS = sorted((o for o in option_info() if o["route_position"]), key=lambda o: o["route_position"])
SPMM_ROUTE_OPTIONS = tuple(o["name"] for o in _SPMM_ROUTE_ROWS)


def host_spmm_route(n_outer: int, n_inner: int, nnz: int, l: int, ldx: int, links=(), tiles_available: bool = False, values_room: bool = True,
                    **options):
    """The route of a sparse product on the host (`scanrs_host_spmm_route`; scan-rs_amd/csrc/spmm_route.hpp, the source kernels.hip
    decides by). `links`: the map as the walked copy sees it, `(kind, a_outer)` per link; `options`: any of SPMM_ROUTE_OPTIONS, the
    library's defaults otherwise. Returns (family, form, chunks, chunk_width, even_ld, tile_candidate) as scanrs_amd.h documents."""
    unknown = set(options) - set(SPMM_ROUTE_OPTIONS)
    if unknown:
        raise ScanrsError(6, f"unknown options {sorted(unknown)}")
    vals = [float(options.get(o["name"], o["default"])) for o in _SPMM_ROUTE_ROWS]
    n = len(links)
    opts = (ctypes.c_double * len(vals))(*vals)
    ka, oa = (ctypes.c_int * max(n, 1))(*[int(k) for k, _ in links]), (ctypes.c_int * max(n, 1))(*[int(bool(a)) for _, a in links])
    out = (ctypes.c_uint64 * 6)()
    _check(_lib.scanrs_host_spmm_route(opts, ctypes.c_uint64(int(n_outer)), ctypes.c_uint64(int(n_inner)), ctypes.c_uint64(int(nnz)), ctypes.c_uint32(int(l)),
                                       ctypes.c_uint32(int(ldx)), ctypes.c_uint32(n), ka, oa, ctypes.c_uint32((1 if tiles_available else 0) | (0 if values_room else 2)), out))
    return tuple(int(v) for v in out)


def host_bk_plan(colmax, b: int, n_iter: int, reuse_cmax: float = 1e5, coef_valid: bool = True):
    """The projection plan of svd_bk on the host (`scanrs_host_bk_plan`; scan-rs_amd/csrc/bk_plan.hpp, the source solver.cpp decides
    by). `colmax`: max |C| per column of Q, b * n_iter entries. Returns a dict with reuse, flagged_older (before any raise),
    limit_branch, limit, direct (tuple, in the order the repair pass carries the columns), last_direct, full_direct, n_early and
    cmax_dense, as scanrs_amd.h documents."""
    cm = _f64(colmax).reshape(-1)
    out, limit, dense = (ctypes.c_uint64 * 7)(), ctypes.c_double(), ctypes.c_double()
    direct = np.zeros(cm.size + 1, dtype=np.uint32)
    _check(_lib.scanrs_host_bk_plan(_p(cm), ctypes.c_uint64(cm.size), ctypes.c_uint32(int(b)), ctypes.c_uint32(int(n_iter)), ctypes.c_double(float(reuse_cmax)),
                                    ctypes.c_int(1 if coef_valid else 0), out, ctypes.byref(limit), ctypes.byref(dense), _p(direct)))
    return dict(reuse=bool(out[0]), flagged_older=int(out[1]), limit_branch=int(out[2]), limit=float(limit.value),
                direct=tuple(int(j) for j in direct[:int(out[3])]), last_direct=bool(out[4]), full_direct=bool(out[5]), n_early=int(out[6]),
                cmax_dense=float(dense.value))


TRANSPOSE_NONE, TRANSPOSE_PACKED_KEY, TRANSPOSE_PAIR_SORT = 0, 1, 2  # counter "transpose_route", host_transpose_plan


def host_transpose_plan(n_outer: int, n_inner: int, max_value: int):
    """Which sort the transposed copy of an n_outer x n_inner copy is built through (`scanrs_host_transpose_plan`;
    scan-rs_amd/csrc/transpose_plan.hpp, the source copy_build.hip decides by). `max_value`: the largest stored count, 0 = not known.
    Returns (route, ib, ob, cb): TRANSPOSE_PACKED_KEY when the bits of inner index, outer id and count sum to at most 64, else
    TRANSPOSE_PAIR_SORT; `AdaptiveMat.counter("transpose_route")` is the route a build took."""
    route, ib, ob, cb = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    _check(_lib.scanrs_host_transpose_plan(ctypes.c_uint64(int(n_outer)), ctypes.c_uint64(int(n_inner)), ctypes.c_uint32(int(max_value)),
                                           ctypes.byref(route), ctypes.byref(ib), ctypes.byref(ob), ctypes.byref(cb)))
    return int(route.value), int(ib.value), int(ob.value), int(cb.value)


def knn_device(d_points: int, n: int, ld: int, d: int, k: int):
    """`nn::knn` on scores that already live in device memory (e.g. PcaResultDevice.d_v / ld_v): (n x k) u32 host array."""
    out = np.zeros((n, k), dtype=np.uint32)
    _check(_lib.scanrs_knn_device(ctypes.c_void_p(d_points), ctypes.c_uint64(n), ctypes.c_uint32(ld), ctypes.c_uint32(d),
                                  ctypes.c_uint32(k), _p(out)))
    return out


DISTANCE_TYPES = {"euclidean": 0, "pearson": 1, "cosine": 2}  # `DistanceType` (umap-rs/src/dist.rs:12-35): SCANRS_DIST_*


def _distance_type(distance) -> int:
    if isinstance(distance, str):
        if distance not in DISTANCE_TYPES:
            raise ScanrsError(6, f"unknown distance {distance!r}: one of {sorted(DISTANCE_TYPES)}")
        return DISTANCE_TYPES[distance]
    return int(distance)


def _nearest_neighbors_call(fn, n: int, k: int, *head):
    """The C entry points write n x k, padded from column min(k, n - 1) on; the reference returns that width (knn.rs:124-127)."""
    idx = np.full((n, k), 0xFFFFFFFF, dtype=np.uint32)
    dist = np.full((n, k), np.inf, dtype=np.float64)
    _check(fn(*head, _p(idx), _p(dist)))
    k_eff = min(k, max(n - 1, 0))
    return np.ascontiguousarray(idx[:, :k_eff]), np.ascontiguousarray(dist[:, :k_eff])


def nearest_neighbors(data, k: int, distance="euclidean"):
    """`umap_rs::knn::nearest_neighbors(data, k, distance_type, ..)` (umap-rs/src/knn.rs:112-166) on the device: (indices u32,
    distances f64), each n x min(k, n - 1), nearest first, under "euclidean", "pearson" or "cosine" distance (dist.rs:12-35, 69-124).
    pearson / cosine: the reference's formula bit for bit, ordered by (sqrt(D), index), distance = sqrt(D)^2; euclidean: the search of
    `knn` with the square root of its squared distance. Equal to `host_nearest_neighbors` in every bit."""
    data = _f64(np.atleast_2d(data))
    n, d = data.shape
    return _nearest_neighbors_call(_lib.scanrs_nearest_neighbors, n, int(k), _p(data), ctypes.c_uint64(n), ctypes.c_uint32(d), ctypes.c_uint32(k),
                                   ctypes.c_int(_distance_type(distance)))


def nearest_neighbors_device(d_data: int, n: int, ld: int, d: int, k: int, distance="euclidean"):
    """`nearest_neighbors` on points that already live in device memory (n x d, leading dimension ld >= d), e.g.
    PcaResultDevice.d_v / ld_v (`scanrs_nearest_neighbors_device`, knn.rs:112-166): host arrays (indices, distances)."""
    return _nearest_neighbors_call(_lib.scanrs_nearest_neighbors_device, int(n), int(k), ctypes.c_void_p(d_data), ctypes.c_uint64(n), ctypes.c_uint32(ld),
                                   ctypes.c_uint32(d), ctypes.c_uint32(k), ctypes.c_int(_distance_type(distance)))


def host_nearest_neighbors(data, k: int, distance="euclidean"):
    """The host twin of `nearest_neighbors` (`scanrs_host_nearest_neighbors`, knn.rs:112-166; no device): exhaustive search."""
    data = _f64(np.atleast_2d(data))
    n, d = data.shape
    return _nearest_neighbors_call(_lib.scanrs_host_nearest_neighbors, n, int(k), _p(data), ctypes.c_uint64(n), ctypes.c_uint32(d), ctypes.c_uint32(k),
                                   ctypes.c_int(_distance_type(distance)))


def _nearest_neighbors_query_call(fn, n_q: int, n_p: int, k: int, *args):
    """The C entry points write n_q x k; the width returned is min(k, n_p), padded with UINT32_MAX / +inf where a row has fewer."""
    idx = np.full((n_q, k), 0xFFFFFFFF, dtype=np.uint32)
    dist = np.full((n_q, k), np.inf, dtype=np.float64)
    _check(fn(*args, _p(idx), _p(dist)))
    k_eff = min(k, n_p)
    return np.ascontiguousarray(idx[:, :k_eff]), np.ascontiguousarray(dist[:, :k_eff])


def _query_sets(queries, points):
    queries, points = _f64(np.atleast_2d(queries)), _f64(np.atleast_2d(points))
    if queries.shape[1] != points.shape[1]:
        raise ScanrsError(1, "Dimension mismatch")
    return queries, points


def nearest_neighbors_query(queries, points, k: int, distance="euclidean", include_self: bool = True):
    """`nearest_neighbors` with a query set of its own (`scanrs_nearest_neighbors_query`, knn.rs:112-166): (indices
    u32 into `points`, distances f64), each n_q x min(k, n_p), nearest first. include_self=False drops the point whose index equals
    the query's row number (the rule of `find_nn`); a row with fewer admissible points is padded with UINT32_MAX / +inf. With
    queries is points and include_self=False it is `nearest_neighbors` in every bit. Equal to `host_nearest_neighbors_query`."""
    queries, points = _query_sets(queries, points)
    (n_q, d), n_p = queries.shape, points.shape[0]
    return _nearest_neighbors_query_call(_lib.scanrs_nearest_neighbors_query, n_q, n_p, int(k), _p(queries), ctypes.c_uint64(n_q), _p(points),
                                         ctypes.c_uint64(n_p), ctypes.c_uint32(d), ctypes.c_uint32(k), ctypes.c_int(_distance_type(distance)),
                                         ctypes.c_int(1 if include_self else 0))


def nearest_neighbors_query_device(d_queries: int, n_q: int, ld_q: int, d_points: int, n_p: int, ld_p: int, d: int, k: int, distance="euclidean",
                                   include_self: bool = True):
    """`nearest_neighbors_query` on sets that already live in device memory, leading dimensions ld_q, ld_p >= d
    (`scanrs_nearest_neighbors_query_device`, knn.rs:112-166): host arrays (indices, distances)."""
    return _nearest_neighbors_query_call(_lib.scanrs_nearest_neighbors_query_device, int(n_q), int(n_p), int(k), ctypes.c_void_p(d_queries),
                                         ctypes.c_uint64(n_q), ctypes.c_uint32(ld_q), ctypes.c_void_p(d_points), ctypes.c_uint64(n_p),
                                         ctypes.c_uint32(ld_p), ctypes.c_uint32(d), ctypes.c_uint32(k), ctypes.c_int(_distance_type(distance)),
                                         ctypes.c_int(1 if include_self else 0))


def host_nearest_neighbors_query(queries, points, k: int, distance="euclidean", include_self: bool = True):
    """The host twin of `nearest_neighbors_query` (`scanrs_host_nearest_neighbors_query`, knn.rs:112-166; no device, any k)."""
    queries, points = _query_sets(queries, points)
    (n_q, d), n_p = queries.shape, points.shape[0]
    return _nearest_neighbors_query_call(_lib.scanrs_host_nearest_neighbors_query, n_q, n_p, int(k), _p(queries), ctypes.c_uint64(n_q), _p(points),
                                         ctypes.c_uint64(n_p), ctypes.c_uint32(d), ctypes.c_uint32(k), ctypes.c_int(_distance_type(distance)),
                                         ctypes.c_int(1 if include_self else 0))


def host_distance(distance, x, y):
    """One pair (`scanrs_host_distance`, dist.rs:19-34, 73-124; no device): (key, dist) = (the rank key sqrt(D), key * key); euclidean:
    both are the distance."""
    x, y = _f64(np.ravel(x)), _f64(np.ravel(y))
    if x.shape != y.shape:
        raise ScanrsError(1, "Dimension mismatch")
    key, dist = ctypes.c_double(), ctypes.c_double()
    _check(_lib.scanrs_host_distance(ctypes.c_int(_distance_type(distance)), _p(x), _p(y), ctypes.c_uint32(x.shape[0]), ctypes.byref(key),
                                     ctypes.byref(dist)))
    return key.value, dist.value


def host_metric_rows(distance, data):
    """What the search forms once per row, exactly as the device forms it (`scanrs_host_metric_rows`, dist.rs:73-76, 106-115; no device):
    (c, s, z) = the centred rows (pearson) or the rows (cosine), their s_xx, and the standardised rows c / sqrt(s_xx) the filter reads."""
    data = _f64(np.atleast_2d(data))
    n, d = data.shape
    c, s, z = np.zeros((n, d)), np.zeros(n), np.zeros((n, d))
    _check(_lib.scanrs_host_metric_rows(ctypes.c_int(_distance_type(distance)), _p(data), ctypes.c_uint64(n), ctypes.c_uint32(d), _p(c), _p(s), _p(z)))
    return c, s, z


def debug_nearest_neighbors_params() -> dict:
    """The constants of the filtered route of `nearest_neighbors` (`scanrs_debug_nearest_neighbors_params`, host only): the filter's
    threshold on the standardised rows is 2 key_k^2 (1 + delta) + e, of which `chain` allows for the filter's own fma chain; the filter
    declines outside sxx_min <= s_xx <= sxx_max."""
    v = [ctypes.c_double() for _ in range(5)]
    _check(_lib.scanrs_debug_nearest_neighbors_params(*[ctypes.byref(x) for x in v]))
    return dict(zip(("delta", "e", "chain", "sxx_min", "sxx_max"), (x.value for x in v)))


class _FuzzyParams(ctypes.Structure):
    _fields_ = [("local_connectivity", ctypes.c_double), ("set_op_mix_ratio", ctypes.c_double), ("apply_fuzzy_combine", ctypes.c_int32),
                ("n_iter", ctypes.c_uint32), ("bandwidth", ctypes.c_double)]


def _fuzzy_params(local_connectivity, set_op_mix_ratio, apply_fuzzy_combine, n_iter, bandwidth):
    return _FuzzyParams(float(local_connectivity), float(set_op_mix_ratio), 1 if apply_fuzzy_combine else 0, int(n_iter or 0), float(bandwidth or 0.0))


_lib.scanrs_graph_free.argtypes = [ctypes.c_void_p]
_lib.scanrs_graph_free.restype = None


class FuzzyGraph:
    """The UMAP graph of `fuzzy_simplicial_set` (`scanrs_graph`, umap-rs/src/fuzzy.rs:30-62): n x n CSR, resident on the
    device (or in host memory for `host_fuzzy_simplicial_set`)."""

    def __init__(self, handle):
        self._h = handle
        info = (ctypes.c_uint64 * 4)()
        _check(_lib.scanrs_graph_info(self._hp(), info, ctypes.c_uint32(4)))
        self._n, self._nnz, self.k, self.on_device = int(info[0]), int(info[1]), int(info[2]), bool(info[3])

    def _hp(self):
        if not self._h:
            raise ScanrsError(6, "the graph has been closed")
        return ctypes.c_void_p(self._h)

    @property
    def shape(self):
        return (self._n, self._n)

    @property
    def nnz(self) -> int:
        return self._nnz

    def to_csr(self):
        """(indptr u64, indices u32, values f64); indices ascend within a row, zeros are stored."""
        indptr, indices, values = np.zeros(self._n + 1, np.uint64), np.zeros(self._nnz, np.uint32), np.zeros(self._nnz, np.float64)
        _check(_lib.scanrs_graph_to_host(self._hp(), _p(indptr), _p(indices), _p(values)))
        return indptr, indices, values

    def _sigmas_rhos(self):
        sigmas, rhos = np.zeros(self._n), np.zeros(self._n)
        _check(_lib.scanrs_graph_sigmas_rhos(self._hp(), _p(sigmas), _p(rhos)))
        return sigmas, rhos

    @property
    def sigmas(self):
        return self._sigmas_rhos()[0]

    @property
    def rhos(self):
        return self._sigmas_rhos()[1]

    def device_pointers(self):
        """(d_indptr, d_indices, d_values): device addresses, valid until close() (`scanrs_graph_device`)."""
        a, b, c = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        _check(_lib.scanrs_graph_device(self._hp(), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def edge_count(self, n_epochs: float) -> int:
        count = ctypes.c_uint64()
        _check(_lib.scanrs_graph_edge_count(self._hp(), ctypes.c_double(n_epochs), ctypes.byref(count)))
        return int(count.value)

    def edges(self, n_epochs: float):
        """The pruned edge list of `initialize_simplicial_set_embedding` before its shuffle (embedding.rs:38-53, 75-85):
        (head u32, tail u32, weights f64, epochs_per_sample f64) in CSR order; tail = row, head = column."""
        m = self.edge_count(n_epochs)
        head, tail, w, eps = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m), np.zeros(m)
        _check(_lib.scanrs_graph_edges(self._hp(), ctypes.c_double(n_epochs), _p(head), _p(tail), _p(w), _p(eps)))
        return head, tail, w, eps

    def close(self):
        if self._h:
            _lib.scanrs_graph_free(ctypes.c_void_p(self._h))
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _knn_lists(indices, distances):
    indices = np.ascontiguousarray(np.atleast_2d(indices), dtype=np.uint32)
    distances = _f64(np.atleast_2d(distances))
    if indices.shape != distances.shape:
        raise ScanrsError(1, "Dimension mismatch")
    return indices, distances


def _graph_call(fn, *head):
    h = ctypes.c_void_p()
    _check(fn(*head, ctypes.byref(h)))
    return FuzzyGraph(h.value)


def fuzzy_simplicial_set(indices, distances, local_connectivity: float = 1.0, set_op_mix_ratio: float = 1.0, apply_fuzzy_combine: bool = True,
                         n_iter: int = 0, bandwidth: float = 0.0) -> FuzzyGraph:
    """`umap_rs::fuzzy::fuzzy_simplicial_set` (umap-rs/src/fuzzy.rs:30-62) of the lists `nearest_neighbors` returns (n x k, u32 / f64,
    UINT32_MAX / +inf padding accepted), on the device (`scanrs_fuzzy_simplicial_set`). n_iter 0 = 64, bandwidth 0 = 1.0.
    Equal to `host_fuzzy_simplicial_set` in every bit."""
    indices, distances = _knn_lists(indices, distances)
    n, k = indices.shape
    prm = _fuzzy_params(local_connectivity, set_op_mix_ratio, apply_fuzzy_combine, n_iter, bandwidth)
    return _graph_call(_lib.scanrs_fuzzy_simplicial_set, _p(indices), _p(distances), ctypes.c_uint64(n), ctypes.c_uint32(k), ctypes.byref(prm))


def fuzzy_simplicial_set_device(d_indices: int, d_distances: int, n: int, ld: int, k: int, local_connectivity: float = 1.0,
                                set_op_mix_ratio: float = 1.0, apply_fuzzy_combine: bool = True, n_iter: int = 0, bandwidth: float = 0.0) -> FuzzyGraph:
    """`fuzzy_simplicial_set` on lists that already live in device memory, leading dimension ld >= k (`scanrs_fuzzy_simplicial_set_device`)."""
    prm = _fuzzy_params(local_connectivity, set_op_mix_ratio, apply_fuzzy_combine, n_iter, bandwidth)
    return _graph_call(_lib.scanrs_fuzzy_simplicial_set_device, ctypes.c_void_p(d_indices), ctypes.c_void_p(d_distances), ctypes.c_uint64(n),
                       ctypes.c_uint32(ld), ctypes.c_uint32(k), ctypes.byref(prm))


def host_fuzzy_simplicial_set(indices, distances, local_connectivity: float = 1.0, set_op_mix_ratio: float = 1.0, apply_fuzzy_combine: bool = True,
                              n_iter: int = 0, bandwidth: float = 0.0) -> FuzzyGraph:
    """The host twin of `fuzzy_simplicial_set` (`scanrs_host_fuzzy_simplicial_set`, fuzzy.rs:30-62; no device)."""
    indices, distances = _knn_lists(indices, distances)
    n, k = indices.shape
    prm = _fuzzy_params(local_connectivity, set_op_mix_ratio, apply_fuzzy_combine, n_iter, bandwidth)
    return _graph_call(_lib.scanrs_host_fuzzy_simplicial_set, _p(indices), _p(distances), ctypes.c_uint64(n), ctypes.c_uint32(k), ctypes.byref(prm))


def umap_graph(points, k: int, distance="euclidean", local_connectivity: float = 1.0, set_op_mix_ratio: float = 1.0, apply_fuzzy_combine: bool = True,
               n_iter: int = 0, bandwidth: float = 0.0) -> FuzzyGraph:
    """`nearest_neighbors` then `fuzzy_simplicial_set` with the lists staying on the device (`scanrs_umap_graph`, umap.rs:89-100):
    equal to `fuzzy_simplicial_set(*nearest_neighbors(points, k, distance), ...)` in every bit."""
    points = _f64(np.atleast_2d(points))
    n, d = points.shape
    prm = _fuzzy_params(local_connectivity, set_op_mix_ratio, apply_fuzzy_combine, n_iter, bandwidth)
    return _graph_call(_lib.scanrs_umap_graph, _p(points), ctypes.c_uint64(n), ctypes.c_uint32(d), ctypes.c_uint32(k),
                       ctypes.c_int(_distance_type(distance)), ctypes.byref(prm))


def umap_graph_device(d_points: int, n: int, ld: int, d: int, k: int, distance="euclidean", local_connectivity: float = 1.0,
                      set_op_mix_ratio: float = 1.0, apply_fuzzy_combine: bool = True, n_iter: int = 0, bandwidth: float = 0.0) -> FuzzyGraph:
    """`umap_graph` on points that already live in device memory, leading dimension ld >= d (`scanrs_umap_graph_device`)."""
    prm = _fuzzy_params(local_connectivity, set_op_mix_ratio, apply_fuzzy_combine, n_iter, bandwidth)
    return _graph_call(_lib.scanrs_umap_graph_device, ctypes.c_void_p(d_points), ctypes.c_uint64(n), ctypes.c_uint32(ld), ctypes.c_uint32(d),
                       ctypes.c_uint32(k), ctypes.c_int(_distance_type(distance)), ctypes.byref(prm))


def host_fuzzy_exp(x):
    """The library's f64 exponential, element by element (`scanrs_host_fuzzy_exp`; no device): the one both the kernels and the twin use."""
    x = _f64(x)
    out = np.zeros_like(x)
    _check(_lib.scanrs_host_fuzzy_exp(_p(x), ctypes.c_uint64(x.size), _p(out)))
    return out


def host_smooth_knn_dist(distances, rho: float, bandwidth: float = 0.0, n_iter: int = 0):
    """`smooth_knn_dist` of one row (`scanrs_host_smooth_knn_dist`, fuzzy.rs:117-145; no device): (sigma, iterations)."""
    distances = _f64(np.ravel(distances))
    sigma, it = ctypes.c_double(), ctypes.c_uint32()
    _check(_lib.scanrs_host_smooth_knn_dist(_p(distances), ctypes.c_uint32(distances.shape[0]), ctypes.c_double(rho), ctypes.c_double(bandwidth),
                                            ctypes.c_uint32(n_iter), ctypes.byref(sigma), ctypes.byref(it)))
    return sigma.value, int(it.value)


def host_membership_strengths(indices, distances, sigmas, rhos):
    """`compute_membership_strengths` (`scanrs_host_membership_strengths`, fuzzy.rs:148-181; no device): (rows, cols, values)."""
    indices, distances = _knn_lists(indices, distances)
    n, k = indices.shape
    sigmas, rhos = _f64(np.ravel(sigmas)), _f64(np.ravel(rhos))
    if sigmas.shape[0] < n or rhos.shape[0] < n:
        raise ScanrsError(1, "Dimension mismatch")
    rows, cols, values = np.zeros(n * k, np.uint32), np.zeros(n * k, np.uint32), np.zeros(n * k)
    count = ctypes.c_uint64()
    _check(_lib.scanrs_host_membership_strengths(_p(indices), _p(distances), ctypes.c_uint64(n), ctypes.c_uint32(k), _p(sigmas), _p(rhos), _p(rows),
                                                 _p(cols), _p(values), ctypes.byref(count)))
    m = int(count.value)
    return rows[:m].copy(), cols[:m].copy(), values[:m].copy()


class RandSvd:
    """`RandSvd` (dim_red/rand_svd.rs:13-50)."""

    def __init__(self, l_multiplier: float = 10.0, n_iter: int = 2):
        self.l_multiplier, self.n_iter = l_multiplier, n_iter

    def run_pca(self, matrix: AdaptiveMat, k: int, omega=None, seed: int = 0):
        r, c = matrix.shape()
        u, s, v = np.zeros((r, k)), np.zeros(k), np.zeros((c, k))
        om = None if omega is None else _f64(omega)
        _check(
            _lib.scanrs_pca_rand(
                matrix._h, ctypes.c_uint32(k), ctypes.c_double(self.l_multiplier), ctypes.c_uint32(self.n_iter),
                ctypes.c_uint64(seed), _p(om), _p(u), _p(s), _p(v)))
        return u, s, v


class Irlba:
    """`Irlba` (dim_red/irlba.rs:36-67)."""

    def __init__(self, tol: float = 0.0001, max_iter: int = 50):
        self.tol, self.max_iter = tol, max_iter
        self.mprod = 0

    def run_pca(self, matrix: AdaptiveMat, k: int, v0=None, snoop: Optional[AtomicSnoop] = None):
        r, c = matrix.shape()
        u, s, v = np.zeros((r, k)), np.zeros(k), np.zeros((c, k))
        vv = None if v0 is None else _f64(v0)
        sref, _keep = _snoop_arg(snoop)
        mp = ctypes.c_uint32()
        _check(
            _lib.scanrs_pca_irlba(
                matrix._h, ctypes.c_uint32(k), ctypes.c_double(self.tol), ctypes.c_uint32(self.max_iter), _p(vv), sref,
                _p(u), _p(s), _p(v), ctypes.byref(mp)))
        self.mprod = int(mp.value)
        return u, s, v


def plan_shards(indptr, world: int) -> np.ndarray:
    """nnz-balanced contiguous partition of the outer dimension."""
    indptr = np.ascontiguousarray(indptr, dtype=np.uint64)
    bounds = np.zeros(world + 1, dtype=np.uint64)
    _check(_lib.scanrs_plan_shards(_p(indptr), ctypes.c_uint64(indptr.shape[0] - 1), ctypes.c_uint32(world), _p(bounds)))
    return bounds


# host-side dense helpers (checked by the CPU test-suite)
def host_plan_inner(indptr, indices, n_inner: int, world: int):
    """`scanrs_host_plan_inner` (host only, no device): the plan of the inner-sharding constructors for a feature-major triplet.
    Returns (slab_bounds, bounds, moved): the slabs of the outer vectors, the shard ranges of the inner dimension (world + 1
    entries each) and the world x world table of stored entries of slab s that lie in shard d's range."""
    ip = np.ascontiguousarray(indptr, dtype=np.uint64)
    ix = np.ascontiguousarray(indices, dtype=np.uint32)
    if ip.shape[0] < 1 or int(ip[-1]) != ix.shape[0]:
        raise ScanrsError(6, "indices length does not match indptr")
    world = int(world)
    sb, bd = np.zeros(max(world, 0) + 1, dtype=np.uint64), np.zeros(max(world, 0) + 1, dtype=np.uint64)
    mv = np.zeros((max(world, 1), max(world, 1)), dtype=np.uint64)
    _check(_lib.scanrs_host_plan_inner(_p(ip), _p(ix), ctypes.c_uint64(ip.shape[0] - 1), ctypes.c_uint64(n_inner), ctypes.c_uint32(world),
                                       _p(sb), _p(bd), _p(mv)))
    return sb, bd, mv


def _export_multi_info(e) -> dict:
    """What `scanrs_multi_to_adaptive` did for the export `e` (ScanrsError 6 on an export of a single handle)."""
    n = ctypes.c_uint32()
    _check(_lib.scanrs_adaptive_export_multi_info(e, ctypes.byref(n), None, None, None))
    n = int(n.value)
    sb, mv, ab = np.zeros(n + 1, dtype=np.uint64), np.zeros((max(n, 1), max(n, 1)), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
    _check(_lib.scanrs_adaptive_export_multi_info(e, None, _p(sb), _p(mv), _p(ab)))
    return {"n_shards": n, "slab_bounds": sb, "moved": mv[:n, :n], "arena_bytes": ab[:n]}


def host_plan_export(counts, n_dst: int):
    """`scanrs_host_plan_export` (host only, no device): the plan of `MultiMat.to_adaptive_vecs(major="inner")` from counts
    (n_src x n_inner: the stored entries source shard s holds of every inner position). Returns (indptr, slab_bounds, moved): the
    whole matrix's inner-major indptr (n_inner + 1), the slabs of inner positions scanrs_plan_shards gives for it (n_dst + 1) and the
    n_src x n_dst table of entries of source s in slab d."""
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    if c.ndim != 2:
        raise ScanrsError(6, "counts: an n_src x n_inner table is required")
    n_src, n_inner, n_dst = c.shape[0], c.shape[1], int(n_dst)
    tip, sb = np.zeros(n_inner + 1, dtype=np.uint64), np.zeros(max(n_dst, 0) + 1, dtype=np.uint64)
    mv = np.zeros((max(n_src, 1), max(n_dst, 1)), dtype=np.uint64)
    _check(_lib.scanrs_host_plan_export(_p(c) if c.size else None, ctypes.c_uint32(n_src), ctypes.c_uint64(n_inner), ctypes.c_uint32(n_dst), _p(tip),
                                        _p(sb), _p(mv)))
    return tip, sb, mv[:n_src, :n_dst]


def host_plan_gather(indptr, src_bounds, idx, n_dst: int):
    """`scanrs_host_plan_gather` (host only, no device): the plan of `MultiMat.gather_outer` / `rebalance` from the source's global
    indptr, its shard bounds (n_src + 1 entries) and the list. Returns (indptr, bounds, moved): the selected matrix's indptr
    (len(idx) + 1), the shard ranges scanrs_plan_shards gives for it (n_dst + 1) and the n_src x n_dst table of nonzeros that go
    from source shard s to shard d."""
    ip = np.ascontiguousarray(indptr, dtype=np.uint64)
    sb = np.ascontiguousarray(src_bounds, dtype=np.uint64)
    idx = np.ascontiguousarray(np.asarray(idx).reshape(-1), dtype=np.int64)
    if ip.shape[0] < 1 or sb.shape[0] < 1:
        raise ScanrsError(6, "indptr and src_bounds need at least one entry")
    if idx.size and int(idx.min()) < 0:
        raise ScanrsError(6, "idx: index out of range: negative index")
    idx = idx.astype(np.uint64)
    n_src, n_dst = sb.shape[0] - 1, int(n_dst)
    tip, bd = np.zeros(idx.shape[0] + 1, dtype=np.uint64), np.zeros(max(n_dst, 0) + 1, dtype=np.uint64)
    mv = np.zeros((max(n_src, 1), max(n_dst, 1)), dtype=np.uint64)
    _check(_lib.scanrs_host_plan_gather(_p(ip), ctypes.c_uint64(ip.shape[0] - 1), _p(sb), ctypes.c_uint32(n_src), _p(idx),
                                        ctypes.c_uint64(idx.shape[0]), ctypes.c_uint32(n_dst), _p(tip), _p(bd), _p(mv)))
    return tip, bd, mv


def host_chol_upper(g):
    g = _f64(g).copy()
    _check(_lib.scanrs_host_chol_upper(_p(g), ctypes.c_int(g.shape[0])))
    return g


def host_inv_upper(r):
    r = _f64(r).copy()
    _check(_lib.scanrs_host_inv_upper(_p(r), ctypes.c_int(r.shape[0])))
    return r


def host_sym_eig(a):
    a = _f64(a)
    n = a.shape[0]
    w, z = np.zeros(n), np.zeros((n, n))
    _check(_lib.scanrs_host_sym_eig(_p(a), ctypes.c_int(n), _p(w), _p(z)))
    return w, z


def host_sym_eig_topk(a, k):
    a = _f64(a)
    n = a.shape[0]
    w, z = np.zeros(k), np.zeros((n, k))
    _check(_lib.scanrs_host_sym_eig_topk(_p(a), ctypes.c_int(n), ctypes.c_int(k), _p(w), _p(z)))
    return w, z


EXPORTED_SYMBOLS = [
    "scanrs_comm_info", "scanrs_last_error", "scanrs_device_available", "scanrs_version", "scanrs_mat_create", "scanrs_mat_create_unsorted", "scanrs_mat_create_device", "scanrs_mat_create_adaptive", "scanrs_knn", "scanrs_find_nn",
    "scanrs_mat_free", "scanrs_mat_view", "scanrs_mat_t", "scanrs_mat_shape", "scanrs_mat_nnz", "scanrs_mat_storage",
    "scanrs_mat_reset_map", "scanrs_mat_compose_scale_axis", "scanrs_mat_apply", "scanrs_mat_set_offset",
    "scanrs_mat_center", "scanrs_mat_scale", "scanrs_mat_scale_and_center", "scanrs_mat_sum_axis_u32",
    "scanrs_mat_sum_axis_f64", "scanrs_mat_mean_axis", "scanrs_mat_mean_var_axis", "scanrs_mat_to_dense",
    "scanrs_mat_dot", "scanrs_mat_rdot", "scanrs_mat_dot_u32", "scanrs_mat_rdot_u32", "scanrs_mat_dot_device",
    "scanrs_normalize", "scanrs_log_normalize", "scanrs_log1p_normalize_fixed_point", "scanrs_mat_target_umi",
    "scanrs_pca_bk", "scanrs_pca_rand", "scanrs_pca_irlba", "scanrs_pca_result_device", "scanrs_knn_device", "scanrs_knn_sharded", "scanrs_multi_knn", "scanrs_host_knn_merge", "scanrs_omega_fill", "scanrs_mat_set_shard", "scanrs_mat_set_shard_comm", "scanrs_comm_get_unique_id", "scanrs_comm_create", "scanrs_comm_free",
    "scanrs_multi_create", "scanrs_multi_free", "scanrs_multi_n_shards", "scanrs_multi_shard", "scanrs_multi_normalize", "scanrs_multi_pca_bk", "scanrs_multi_pca_rand", "scanrs_multi_pca_irlba", "scanrs_multi_log_normalize", "scanrs_multi_sseq_params", "scanrs_multi_group_sums", "scanrs_multi_sseq_de", "scanrs_multi_comm_info",
    "scanrs_sseq_de_pairs_sharded", "scanrs_merge_clusters_sharded", "scanrs_cluster_medoids_sharded", "scanrs_multi_sseq_de_pairs", "scanrs_multi_merge_clusters", "scanrs_multi_cluster_medoids",
    "scanrs_plan_shards", "scanrs_multi_create_inner", "scanrs_multi_create_adaptive_inner", "scanrs_multi_create_from_file", "scanrs_multi_create_info", "scanrs_host_plan_inner", "scanrs_multi_gather_outer", "scanrs_multi_rebalance", "scanrs_multi_balance", "scanrs_multi_gather_info", "scanrs_host_plan_gather", "scanrs_profile_enable", "scanrs_profile_reset", "scanrs_profile_get", "scanrs_mat_sync", "scanrs_mat_set_spmm_path", "scanrs_mat_set_option", "scanrs_set_global_option", "scanrs_mat_set_panel_precision",
    "scanrs_mat_chol_rinv", "scanrs_mat_get_counter", "scanrs_host_chol_upper", "scanrs_host_inv_upper", "scanrs_host_sym_eig", "scanrs_host_sym_eig_topk", "scanrs_debug_wait_never", "scanrs_debug_barrier_alone", "scanrs_debug_arena_selftest", "scanrs_debug_dense_route", "scanrs_debug_dense_gram", "scanrs_debug_dense_gemm", "scanrs_debug_weighted_colsum", "scanrs_debug_knn_filter", "scanrs_debug_knn_last_stats", "scanrs_debug_knn_filter_params", "scanrs_init", "scanrs_release_cached_memory", "scanrs_cached_memory_bytes", "scanrs_reserve_device_memory", "scanrs_device_memory_in_use",
    "scanrs_h5_read_csc_matrix", "scanrs_h5_read_adaptive_csr_matrix", "scanrs_h5_read_matrix_metadata", "scanrs_h5_matrix_free",
    "scanrs_h5_matrix_shape", "scanrs_h5_matrix_arrays", "scanrs_h5_matrix_n_strings", "scanrs_h5_matrix_string", "scanrs_h5_matrix_removed",
    "scanrs_h5_read_umi_counts", "scanrs_h5_get_clustering_keys", "scanrs_h5_get_clustering", "scanrs_h5_get_differential_expression",
    "scanrs_h5_read_f64", "scanrs_h5_read_strings", "scanrs_h5_member_names", "scanrs_mtx_read", "scanrs_mat_create_from_file",
    "scanrs_sseq_params", "scanrs_sseq_params_from_moments", "scanrs_mat_group_sums", "scanrs_sseq_de", "scanrs_sseq_de_from_sums",
    "scanrs_sseq_de_backend", "scanrs_sseq_de_from_sums_backend", "scanrs_host_nb_exact_test_ratio", "scanrs_host_nb_exact_ratio_step",
    "scanrs_host_nb_exact_test", "scanrs_host_nb_asymptotic_test", "scanrs_host_nb_log_prob_all", "scanrs_host_adjusted_pvalue_bh",
    "scanrs_host_betainc", "scanrs_host_betaincinv", "scanrs_sseq_de_pairs", "scanrs_host_union_median",
    "scanrs_host_pdist", "scanrs_host_linkage_complete", "scanrs_host_relabel_by_size", "scanrs_cluster_medoids", "scanrs_cluster_medoids_device",
    "scanrs_merge_clusters",
    "scanrs_hclust_create", "scanrs_hclust_create_device", "scanrs_hclust_from_steps", "scanrs_hclust_free", "scanrs_hclust_n", "scanrs_hclust_steps",
    "scanrs_hclust_leaves", "scanrs_hclust_merge_below", "scanrs_hclust_fcluster", "scanrs_hclust_info", "scanrs_host_hclust_linkage",
    "scanrs_debug_hclust_pdist",
    "scanrs_nearest_neighbors", "scanrs_nearest_neighbors_device", "scanrs_host_nearest_neighbors",
    "scanrs_nearest_neighbors_query", "scanrs_nearest_neighbors_query_device", "scanrs_host_nearest_neighbors_query",
    "scanrs_nearest_neighbors_sharded", "scanrs_multi_nearest_neighbors", "scanrs_host_distance", "scanrs_host_metric_rows",
    "scanrs_debug_nearest_neighbors_params",
    "scanrs_fuzzy_simplicial_set", "scanrs_fuzzy_simplicial_set_device", "scanrs_umap_graph", "scanrs_umap_graph_device",
    "scanrs_host_fuzzy_simplicial_set", "scanrs_graph_info", "scanrs_graph_to_host", "scanrs_graph_sigmas_rhos", "scanrs_graph_device",
    "scanrs_graph_free", "scanrs_graph_edge_count", "scanrs_graph_edges", "scanrs_host_fuzzy_exp", "scanrs_host_smooth_knn_dist",
    "scanrs_host_membership_strengths",
    "scanrs_mat_select_rows", "scanrs_mat_select_cols", "scanrs_mat_partition_on_thresholds", "scanrs_mat_to_csmat",
    "scanrs_mat_select_rows_sharded", "scanrs_mat_select_cols_sharded", "scanrs_mat_partition_on_thresholds_sharded", "scanrs_mat_shard_info",
    "scanrs_multi_shape", "scanrs_multi_to_csmat", "scanrs_multi_select_rows", "scanrs_multi_select_cols", "scanrs_multi_partition_on_thresholds",
    "scanrs_mat_to_adaptive", "scanrs_mat_to_adaptive_major", "scanrs_multi_to_adaptive", "scanrs_adaptive_export_multi_info", "scanrs_host_plan_export",
    "scanrs_adaptive_export_info", "scanrs_adaptive_export_vecs", "scanrs_adaptive_export_free",
    "scanrs_host_choose_storage", "scanrs_host_col_moments_plan", "scanrs_host_spmm_route", "scanrs_host_bk_plan", "scanrs_host_transpose_plan",
    "scanrs_host_option_info", "scanrs_host_option_parse", "scanrs_host_counter_name",
    "scanrs_mat_sum_rows_u64", "scanrs_mat_sum_rows_f64", "scanrs_mat_sum_cols_u64", "scanrs_mat_sum_cols_f64", "scanrs_mat_sum_rows_dual_u64",
    "scanrs_mat_sum_rows_dual_f64", "scanrs_mat_mean_rows", "scanrs_mat_mean_var_rows", "scanrs_mat_var_axis",
    "scanrs_mat_sum_rows_u64_sharded", "scanrs_mat_sum_rows_f64_sharded", "scanrs_mat_sum_cols_u64_sharded", "scanrs_mat_sum_cols_f64_sharded",
    "scanrs_mat_sum_rows_dual_u64_sharded", "scanrs_mat_sum_rows_dual_f64_sharded", "scanrs_mat_mean_rows_sharded", "scanrs_mat_mean_var_rows_sharded",
    "scanrs_multi_sum_rows_u64", "scanrs_multi_sum_rows_f64", "scanrs_multi_sum_cols_u64", "scanrs_multi_sum_cols_f64",
    "scanrs_multi_sum_rows_dual_u64", "scanrs_multi_sum_rows_dual_f64", "scanrs_multi_mean_rows", "scanrs_multi_mean_var_rows",
]

# sSeq differential expression (sseq.py)
from .sseq import (  # noqa: E402
    NB_EXACT_LOGSPACE, NB_EXACT_RATIO, DiffExpResult, SSeqParams, compute_sseq_params, diff_exp_table, group_sums, host_nb_exact_ratio_step,
    host_nb_exact_test_ratio, host_union_median, labels_from_clustering, sseq_de_each_vs_control, sseq_de_from_sums, sseq_de_one_vs_rest, sseq_de_pairs,
    sseq_de_pairs_sharded, sseq_de_vs_control, sseq_differential_expression, sseq_params_from_moments,
)

# merge_clusters, linkage and medoids (cluster.py)
from .cluster import (  # noqa: E402
    MergeTrace, cluster_medoids, cluster_medoids_sharded, linkage, medioids, merge_clusters, merge_clusters_sharded, pdist, relabel_by_size,
)

# hierarchical clustering with leaf ordering (hclust.py)
from .hclust import (  # noqa: E402
    ClusterDirection, DeviceArray2, HierarchicalCluster, LeafOrdering, LinkageMethod,
)
