"""scanrs_mat_to_adaptive (scan-rs_amd/csrc/encode.hip, encode_host.cpp): the AdaptiveVec encoders on the device against the oracle's
restatement of the reference's constructors (oracle/adaptive_vec.py). Integer work: every comparison is equality of bytes."""
import collections
import gc
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import adaptive_grid as ag  # noqa: E402
import adaptive_vec as av  # noqa: E402

FIELDS = ("data", "fallback_indexes", "fallback_values", "index_bytes", "block_starts")
DTYPES = {"fallback_indexes": np.uint32, "fallback_values": np.uint32, "index_bytes": np.uint8, "block_starts": np.uint32}


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


@pytest.fixture(scope="module")
def grid():
    return ag.grid()


@pytest.fixture(scope="module")
def oracle_pieces(grid):
    """{(length, kind or None): [pieces() of every vector]}: computed once, shared, never changed"""
    out = {}
    for length, vecs in grid.items():
        for kind in (None,) + av.KINDS:
            out[(length, kind)] = [(av.AdaptiveVec.new(length, v, i) if kind is None else av.AdaptiveVec.with_kind(kind, length, v, i))
                                   for i, v in vecs]
    return out


@pytest.fixture(scope="module")
def synth(sa):
    from scanrs_amd.synth import synth_counts

    return synth_counts(3000, 700, 0.05, 5)  # cells x genes CSR: taken cell by cell


def _handle(sa, length, vecs, storage):
    indptr, indices, data = ag.as_csmat(vecs)
    n = len(vecs)
    rows, cols = (n, length) if storage == sa.CSR else (length, n)
    return sa.AdaptiveMat.from_csmat(rows, cols, storage, indptr, indices, data)


def _assert_same_vec(got, want, where):
    for key in ("kind", "len", "n_units"):
        assert int(got[key]) == int(want[key]), (where, key, got[key], want[key])
    for key in FIELDS:
        g, w = got[key], want[key]
        if w is None:
            assert g is None, (where, key)
            continue
        assert g is not None, (where, key)
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == (DTYPES[key] if key in DTYPES else w.dtype), (where, key, g.dtype)
        assert g.shape == w.shape, (where, key, g.shape, w.shape)  # the exact length of data and block_starts included
        assert g.tobytes() == w.tobytes(), (where, key)


@pytest.mark.parametrize("length", ag.LENGTHS)
def test_every_encoder_is_bit_exact_against_the_oracle(sa, grid, oracle_pieces, length):
    for storage in (sa.CSR, sa.CSC):
        h = _handle(sa, length, grid[length], storage)
        for kind in (None,) + av.KINDS:
            got = h.to_adaptive_vecs(kind)
            want = oracle_pieces[(length, kind)]
            assert len(got) == len(want) == 25
            for o, (g, w) in enumerate(zip(got, want)):
                _assert_same_vec(g, w.pieces(), (length, storage, kind, o))


def test_accounting_equals_the_oracle(sa, grid, oracle_pieces):
    for length in (22, 5000):
        h = _handle(sa, length, grid[length], sa.CSR)
        for kind in (None, "D3", "S8", "V"):
            want = oracle_pieces[(length, kind)]
            total, counts = h.adaptive_info(kind)
            assert total == sum(v.mem_size() for v in want), (length, kind)
            hist = collections.Counter(v.kind for v in want)
            assert counts == [hist.get(k, 0) for k in av.KINDS], (length, kind)


def _same_csmat(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a.to_csmat(), b.to_csmat())) and a.shape() == b.shape() and a.storage() == b.storage()


def _round_trip(sa, h):
    r, c = h.shape()
    back = sa.AdaptiveMat.from_adaptive_vecs(r, c, h.storage(), h.to_adaptive_vecs())
    assert _same_csmat(back, h)


def test_round_trip_through_create_adaptive(sa, grid, synth):
    for storage in (sa.CSR, sa.CSC):
        _round_trip(sa, _handle(sa, 300, grid[300], storage))
        _round_trip(sa, _handle(sa, 5000, grid[5000], storage))
    m = synth
    for h in (sa.AdaptiveMat.from_csmat(m.shape[0], m.shape[1], sa.CSR, m.indptr, m.indices, m.data),
              sa.AdaptiveMat.from_csmat(m.shape[1], m.shape[0], sa.CSC, m.indptr, m.indices, m.data)):
        rows = np.random.default_rng(1).integers(0, h.rows(), size=h.rows() // 2)  # permuted, with repeats
        _round_trip(sa, h.select_rows(rows))
        f, r, _, _ = h.partition_on_threshold(60.0)  # cells below 60 counts go, then the genes the rest leaves below 60
        assert 0 < f.nnz() < h.nnz()
        if h.storage() == sa.CSR:
            assert r.nnz() > 0
        _round_trip(sa, f)
        _round_trip(sa, r)


def test_compression_of_the_synthetic_matrix(sa, synth):
    m = synth
    h = sa.AdaptiveMat.from_csmat(m.shape[1], m.shape[0], sa.CSC, m.indptr, m.indices, m.data)  # genes x cells, one vector per cell
    total, counts = h.adaptive_info()
    assert sum(counts) == m.shape[0]
    assert total < 0.75 * 8 * m.nnz
    vecs = av.from_csmat(m.shape[0], m.shape[1], m.indptr, m.indices.astype(np.uint32), m.data.astype(np.uint32))
    assert total == sum(v.mem_size() for v in vecs)


def test_counts_are_exported_not_mapped_values_and_views_share_the_vectors(sa, grid, synth):
    m = synth
    raw = sa.AdaptiveMat.from_csmat(m.shape[1], m.shape[0], sa.CSC, m.indptr, m.indices, m.data).to_adaptive_vecs()
    normed = sa.normalize(sa.AdaptiveMat.from_csmat(m.shape[1], m.shape[0], sa.CSC, m.indptr, m.indices, m.data), sa.Normalization.CellRanger)
    for o, (g, w) in enumerate(zip(normed.to_adaptive_vecs(), raw)):
        _assert_same_vec(g, w, ("normalized", o))
    vecs = grid[300]
    raw = _handle(sa, 300, vecs, sa.CSC).to_adaptive_vecs()
    h = _handle(sa, 300, vecs, sa.CSR)
    t = h.t()
    assert t.storage() == sa.CSC and tuple(t.shape()) == (300, 25)
    for o, (g, w) in enumerate(zip(t.to_adaptive_vecs(), raw)):
        _assert_same_vec(g, w, ("transposed", o))
    back = sa.AdaptiveMat.from_adaptive_vecs(300, 25, t.storage(), t.to_adaptive_vecs())
    assert _same_csmat(back, t)


def test_two_calls_return_identical_arenas(sa, grid):
    h = _handle(sa, 70001, grid[70001], sa.CSR)
    for kind in (None, "S3", "D4"):
        a, b = h.to_adaptive_vecs(kind), h.to_adaptive_vecs(kind)
        for o, (x, y) in enumerate(zip(a, b)):
            _assert_same_vec(x, y, (kind, o))


def test_errors_and_empty_matrices(sa):
    h = sa.AdaptiveMat.from_dense(np.arange(12, dtype=np.uint32).reshape(3, 4))
    for bad in (8, -2):
        with pytest.raises(sa.ScanrsError) as e:
            h.to_adaptive_vecs(bad)
        assert e.value.code == 6
    with pytest.raises(sa.ScanrsError):
        h.to_adaptive_vecs("D5")
    n = 5
    empty = np.zeros(0, dtype=np.uint32)
    none = sa.AdaptiveMat.from_csmat(0, n, sa.CSR, np.zeros(1, dtype=np.uint64), empty, empty)
    assert none.to_adaptive_vecs() == [] and none.adaptive_info() == (0, [0] * 8)
    hollow = sa.AdaptiveMat.from_csmat(n, 0, sa.CSR, np.zeros(n + 1, dtype=np.uint64), empty, empty)
    got = hollow.to_adaptive_vecs()
    assert len(got) == n
    for o, g in enumerate(got):
        _assert_same_vec(g, av.AdaptiveVec.new(0, empty, empty).pieces(), ("hollow", o))


def test_no_device_memory_is_left_behind(sa, grid):
    h = _handle(sa, 5000, grid[5000], sa.CSR)
    h.to_adaptive_vecs()
    gc.collect()
    sa.release_cached_memory()
    start = sa.device_memory_in_use()
    for kind in (None, "D16", "S4"):
        h.to_adaptive_vecs(kind)
        h.adaptive_info(kind)
    gc.collect()
    sa.release_cached_memory()
    assert sa.device_memory_in_use() == start
