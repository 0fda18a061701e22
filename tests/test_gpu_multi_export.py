"""scanrs_multi_to_adaptive and scanrs_mat_to_adaptive_major (scan-rs_amd/csrc/export_multi.hip, multi.cpp,
encode_host.cpp): the whole multi-GPU matrix as AdaptiveVec encodings in either orientation, against the oracle's restatement of the
reference's constructors (oracle/adaptive_vec.py) and against the export of the unsharded matrix. Integer work: every comparison is
equality of bytes. All shards share device 0."""
import ctypes
import functools
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
import reshard_ref  # noqa: E402

FIELDS = ("data", "fallback_indexes", "fallback_values", "index_bytes", "block_starts")
DTYPES = {"fallback_indexes": np.uint32, "fallback_values": np.uint32, "index_bytes": np.uint8, "block_starts": np.uint32}
ALL_KINDS = (None,) + av.KINDS
SHARDS = (1, 2, 3, 5)
ARGUMENT = 6  # SCANRS_ERR_ARGUMENT


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
def synth(sa):
    from scanrs_amd.synth import synth_counts

    return synth_counts(3000, 700, 0.05, 5)  # cells x genes CSR: taken cell by cell


@functools.lru_cache(maxsize=None)
def case(name):
    """(n_outer, n_inner, triplet) of reshard_ref.CASES, feature-major, computed once and read-only"""
    n_outer, n_inner, ip, ix, vv = reshard_ref.CASES[name]()
    for a in (ip, ix, vv):
        a.setflags(write=False)
    return n_outer, n_inner, (ip, ix, vv)


def _oracle(grid, length, kind):
    return [(av.AdaptiveVec.new(length, v, i) if kind is None else av.AdaptiveVec.with_kind(kind, length, v, i)).pieces() for i, v in grid[length]]


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


def _assert_same_table(got, want, where):
    assert len(got) == len(want), (where, len(got), len(want))
    for o, (g, w) in enumerate(zip(got, want)):
        _assert_same_vec(g, w, (where, o))


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def _grid_multi(sa, grid, length, n):
    """The 25 grid vectors as a 25 x length CSR triplet, its `length` inner positions sharded: 25 x length, CSC"""
    return sa.MultiMat.from_csmat_inner(25, length, sa.CSR, *ag.as_csmat(grid[length]), n, devices=[0] * n)


# ---- INNER on the grid -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [x for x in ag.LENGTHS if x != 70001])
def test_inner_on_the_grid_is_bit_exact_against_the_oracle_and_the_unsharded_export(sa, grid, length):
    """The small lengths are the point: 1 with 5 shards leaves four shards empty, 21 / 22 cut one Dense3 word across shards, 300 cuts
    across a 256-index block, 5000 gives a vector more elements than a pull tile at density 1 (it spans tiles and sources)."""
    single = sa.AdaptiveMat.from_csmat(25, length, sa.CSR, *ag.as_csmat(grid[length]))
    want = {kind: (_oracle(grid, length, kind), single.to_adaptive_vecs(kind)) for kind in ALL_KINDS}
    for n in SHARDS:
        mm = _grid_multi(sa, grid, length, n)
        assert mm.storage == sa.CSC and mm.shape() == [25, length]
        if length == 1 and n == 5:
            assert sum(hi > lo for _, lo, hi in mm.shard_ranges()) == 1
        for kind in ALL_KINDS:
            got = mm.to_adaptive_vecs(kind, major="inner")
            assert len(got) == 25 and all(v["len"] == length for v in got)
            _assert_same_table(got, want[kind][0], (length, n, kind, "oracle"))
            _assert_same_table(got, want[kind][1], (length, n, kind, "unsharded"))
        total, counts = mm.adaptive_info(None, major="inner")
        assert (total, counts) == single.adaptive_info(None)
        mm.close()


def test_inner_at_the_long_length_and_two_calls_return_identical_arenas(sa, grid):
    length = 70001
    mm = _grid_multi(sa, grid, length, 3)
    for kind in (None, "S3", "D4"):
        a, b = mm.to_adaptive_vecs(kind, major="inner"), mm.to_adaptive_vecs(kind, major="inner")
        _assert_same_table(a, _oracle(grid, length, kind), (length, kind))
        _assert_same_table(a, b, (length, kind, "second call"))
    info = mm.export_info()
    assert int(info["moved"].sum()) == mm.nnz()
    # a slab with more elements than one pull tile, fed by more than one source
    assert int(info["moved"].sum(axis=0).max()) > 2048 and int((info["moved"] > 0).sum(axis=0).max()) > 1
    mm.close()


# ---- INNER on every case of reshard_ref.CASES ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(reshard_ref.CASES))
def test_inner_on_the_reshard_cases(sa, name):
    n_outer, n_inner, (ip, ix, vv) = case(name)
    kept = reshard_ref.drop_zeros(ip, ix, vv)
    single = sa.AdaptiveMat.from_csmat(n_outer, n_inner, sa.CSR, *kept)
    want = {kind: single.to_adaptive_vecs(kind) for kind in (None, "D3", "S8")}
    for n in reshard_ref.SHARDS:
        where = f"{name} over {n}"
        mm = sa.MultiMat.from_csmat_inner(n_outer, n_inner, sa.CSR, ip, ix, vv, n, devices=[0] * n)
        for kind, table in want.items():
            got = mm.to_adaptive_vecs(kind, major="inner")
            assert len(got) == n_outer and all(v["len"] == n_inner for v in got), where
            _assert_same_table(got, table, (where, kind))
        # back through the decoder: the original feature-major triplet, stored zeros dropped
        back = sa.AdaptiveMat.from_adaptive_vecs(n_outer, n_inner, sa.CSR, mm.to_adaptive_vecs(major="inner"))
        assert _same(back.to_csmat(), kept), where
        # what the call did, against the plan on the host from the shards' own per-position counts
        counts = np.stack([np.bincount(mm.shard_csmat(s)[1].astype(np.int64), minlength=n_outer).astype(np.uint64) for s in range(n)])
        tip, sb, mv = sa.host_plan_export(counts, n)
        info = mm.export_info()
        assert info["n_shards"] == n and np.array_equal(info["slab_bounds"], sb) and np.array_equal(info["moved"], mv), where
        assert int(info["moved"].sum()) == mm.nnz() == int(kept[0][-1]), where
        assert np.array_equal(tip, kept[0]), where  # the whole matrix's inner-major indptr is the feature-major one
        total, _ = mm.adaptive_info(None, major="inner")
        assert info["arena_bytes"].shape == (n,) and int(info["arena_bytes"].sum()) >= total, where
        empty = np.diff(sb.astype(np.int64)) == 0
        assert np.all(info["arena_bytes"][empty] == 0), where
        assert all(mm.counter(f"export_{p}_us", i) >= 0 for p in ("plan", "pull", "encode") for i in range(n))
        mm.close()


# ---- STORED --------------------------------------------------------------------------------------------------------------------------
def _assert_stored_equals_unsharded(sa, mm, where, kinds=(None, "D4", "S3")):
    rows, cols = mm.shape()
    single = sa.AdaptiveMat.from_csmat(rows, cols, mm.storage, *mm.to_csmat())
    n_outer = rows if mm.storage == sa.CSR else cols
    for kind in kinds:
        got = mm.to_adaptive_vecs(kind)
        assert len(got) == n_outer, where
        _assert_same_table(got, single.to_adaptive_vecs(kind), (where, kind))
        _assert_same_table(mm.to_adaptive_vecs(kind, major="stored"), got, (where, kind, "major spelled out"))
    assert mm.adaptive_info() == single.adaptive_info(), where
    info = mm.export_info(major="stored")
    bounds = np.array([0] + [hi for _, _, hi in mm.shard_ranges()], dtype=np.uint64)
    assert np.array_equal(info["slab_bounds"], bounds) and np.array_equal(info["moved"], np.diag(mm.balance()["shard_nnz"])), where
    # and the other orientation of the same matrix, against the handle's own transposed copy
    _assert_same_table(mm.to_adaptive_vecs(None, major="inner"), single.to_adaptive_vecs(None, major="inner"), (where, "inner"))


def test_stored_equals_the_unsharded_export(sa, synth):
    m = synth
    mm = sa.MultiMat(m.shape[1], m.shape[0], sa.CSC, m.indptr, m.indices, m.data, 3, devices=[0] * 3)  # genes x cells, the cells sharded
    _assert_stored_equals_unsharded(sa, mm, "synth over 3")
    _assert_same_table(mm.to_adaptive_vecs(), mm.to_adaptive_vecs(), "stored, second call")
    f, r, _, _ = mm.partition_on_threshold(60.0)  # unbalanced shards, nothing rebalanced
    assert 0 < f.nnz() < mm.nnz()
    _assert_stored_equals_unsharded(sa, f, "filtered", kinds=(None,))
    _assert_stored_equals_unsharded(sa, r, "residual", kinds=(None,))
    b = f.rebalance()
    assert b.shard_ranges() != f.shard_ranges() or f.balance()["imbalance"] == 1.0
    _assert_stored_equals_unsharded(sa, b, "rebalanced", kinds=(None,))
    for x in (b, f, r, mm):
        x.close()


def test_stored_over_empty_shards_and_a_csr_matrix(sa):
    n_outer, n_inner, (ip, ix, vv) = case("one_position")  # every nonzero in one inner position: the cut leaves empty shards
    mm = sa.MultiMat.from_csmat_inner(n_outer, n_inner, sa.CSR, ip, ix, vv, 5, devices=[0] * 5)
    assert any(hi == lo for _, lo, hi in mm.shard_ranges())
    _assert_stored_equals_unsharded(sa, mm, "one_position over 5")
    mm.close()
    n_outer, n_inner, (ip, ix, vv) = case("seeded")
    kept = reshard_ref.drop_zeros(ip, ix, vv)
    mm = sa.MultiMat(n_outer, n_inner, sa.CSR, *kept, 3, devices=[0] * 3)  # the rows sharded
    _assert_stored_equals_unsharded(sa, mm, "seeded CSR over 3")
    mm.close()


# ---- independence of the cut -------------------------------------------------------------------------------------------------------
def test_inner_does_not_depend_on_the_cut(sa):
    n_outer, n_inner, (ip, ix, vv) = case("seeded")
    first = {}
    for n in SHARDS:
        mm = sa.MultiMat.from_csmat_inner(n_outer, n_inner, sa.CSR, ip, ix, vv, n, devices=[0] * n)
        for kind in (None, "D8", "S4"):
            got = mm.to_adaptive_vecs(kind, major="inner")
            _assert_same_table(got, first.setdefault(kind, got), ("seeded", n, kind))
        if n == 3:  # the same matrix over another shard count, cut by gather_outer's own plan
            other = mm.gather_outer(np.arange(n_inner), 4, devices=[0] * 4)
            assert other.shard_ranges() != mm.shard_ranges()
            for kind in (None, "D8", "S4"):
                _assert_same_table(other.to_adaptive_vecs(kind, major="inner"), first[kind], ("seeded", "gather_outer", kind))
            other.close()
        mm.close()


# ---- round trip --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["seeded", "long_vector", "one_position"])
def test_round_trip_through_the_inner_sharding_constructor(sa, name):
    n_outer, n_inner, (ip, ix, vv) = case(name)
    for n in (2, 5):
        mm = sa.MultiMat.from_csmat_inner(n_outer, n_inner, sa.CSR, ip, ix, vv, n, devices=[0] * n)
        back = sa.MultiMat.from_adaptive_vecs_inner(n_outer, n_inner, sa.CSR, mm.to_adaptive_vecs(major="inner"), n, devices=[0] * n)
        assert back.storage == mm.storage and back.shape() == mm.shape() and back.shard_ranges() == mm.shard_ranges(), (name, n)
        assert _same(back.to_csmat(), mm.to_csmat()), (name, n)
        back.close()
        mm.close()


# ---- one handle ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [22, 300, 5000])
def test_one_handle_exports_its_other_orientation(sa, grid, length):
    ip, ix, vv = ag.as_csmat(grid[length])
    tp = reshard_ref.transposed_triplet(ip, ix, vv, 25, length)
    kinds = ALL_KINDS if length < 5000 else (None, "D3", "S4")
    for storage, other in ((sa.CSR, sa.CSC), (sa.CSC, sa.CSR)):
        rows, cols = (25, length) if storage == sa.CSR else (length, 25)
        h = sa.AdaptiveMat.from_csmat(rows, cols, storage, ip, ix, vv)
        host_t = sa.AdaptiveMat.from_csmat(rows, cols, other, *tp)  # the same matrix, transposed on the host
        for kind in kinds:
            got = h.to_adaptive_vecs(kind, major="inner")
            assert len(got) == length and all(v["len"] == 25 for v in got)
            _assert_same_table(got, host_t.to_adaptive_vecs(kind), (length, storage, kind))
        # what create_adaptive takes under the OTHER flag
        back = sa.AdaptiveMat.from_adaptive_vecs(rows, cols, other, h.to_adaptive_vecs(major="inner"))
        assert _same(back.to_csmat(), tp) and back.storage() == other
        # "stored" is today's call
        e = ctypes.c_void_p()
        sa._check(sa._lib.scanrs_mat_to_adaptive(h._h, ctypes.c_int(-1), ctypes.byref(e)))
        try:
            today = sa._export_vecs(e)
        finally:
            sa._lib.scanrs_adaptive_export_free(e)
        _assert_same_table(h.to_adaptive_vecs(None, major="stored"), today, (length, storage, "stored"))
        _assert_same_table(h.to_adaptive_vecs(), today, (length, storage, "default"))
        _assert_same_table(today, _oracle(grid, length, None), (length, storage, "oracle"))
        # through a transposed view the vectors are those of the stored arrays
        _assert_same_table(h.t().to_adaptive_vecs(None, major="inner"), h.to_adaptive_vecs(None, major="inner"), (length, storage, "view"))


def test_a_sharded_handle_refuses_inner_and_keeps_exporting_its_shard(sa, grid):
    ip, ix, vv = ag.as_csmat(grid[300])
    h = sa.AdaptiveMat.from_csmat(25, 300, sa.CSR, ip, ix, vv)
    today = h.to_adaptive_vecs()
    h.set_shard(0, 2, 0, 50, allreduce=lambda ptr, count, dtype: 0)  # rank 0 of 2: the rows 0 .. 24 of 50 (the export exchanges nothing)
    with pytest.raises(sa.ScanrsError) as e:
        h.to_adaptive_vecs(major="inner")
    assert e.value.code == ARGUMENT and "scanrs_multi_to_adaptive" in str(e.value)
    _assert_same_table(h.to_adaptive_vecs(major="stored"), today, "sharded, stored")


def test_counts_are_exported_not_mapped_values(sa, synth):
    m = synth
    args = (m.shape[1], m.shape[0], sa.CSC, m.indptr, m.indices, m.data)
    raw = sa.AdaptiveMat.from_csmat(*args).to_adaptive_vecs(major="inner")
    normed = sa.normalize(sa.AdaptiveMat.from_csmat(*args), sa.Normalization.CellRanger)
    _assert_same_table(normed.to_adaptive_vecs(major="inner"), raw, "normalized handle")
    mm = sa.MultiMat(*args, 3, devices=[0] * 3)
    mm.normalize(sa.Normalization.CellRanger)
    _assert_same_table(mm.to_adaptive_vecs(major="inner"), raw, "normalized multi")
    mm.close()


# ---- empty inputs, errors and memory ---------------------------------------------------------------------------------------------------
def test_matrices_without_vectors(sa):
    empty = np.zeros(0, dtype=np.uint32)
    hollow_vec = av.AdaptiveVec.new(0, empty, empty).pieces()
    none = sa.MultiMat(5, 0, sa.CSC, np.zeros(1, dtype=np.uint64), empty, empty, 2, devices=[0, 0])  # 5 x 0: no outer vector
    assert none.to_adaptive_vecs() == [] and none.adaptive_info() == (0, [0] * 8)
    got = none.to_adaptive_vecs(major="inner")
    assert len(got) == 5
    for o, g in enumerate(got):
        _assert_same_vec(g, hollow_vec, ("no outer vector", o))
    none.close()
    hollow = sa.MultiMat(0, 5, sa.CSC, np.zeros(6, dtype=np.uint64), empty, empty, 2, devices=[0, 0])  # 0 x 5: no inner position
    assert hollow.to_adaptive_vecs(major="inner") == [] and hollow.adaptive_info(major="inner") == (0, [0] * 8)
    got = hollow.to_adaptive_vecs()
    assert len(got) == 5
    for o, g in enumerate(got):
        _assert_same_vec(g, hollow_vec, ("no inner position", o))
    hollow.close()
    single = sa.AdaptiveMat.from_csmat(0, 5, sa.CSR, np.zeros(1, dtype=np.uint64), empty, empty)
    got = single.to_adaptive_vecs(major="inner")
    assert len(got) == 5 and single.to_adaptive_vecs() == []
    for o, g in enumerate(got):
        _assert_same_vec(g, hollow_vec, ("single", o))


def test_errors(sa, grid):
    h = sa.AdaptiveMat.from_dense(np.arange(12, dtype=np.uint32).reshape(3, 4))
    mm = _grid_multi(sa, grid, 22, 2)
    for x in (h, mm):
        for major in ("stored", "inner"):
            for bad in (8, -2):
                with pytest.raises(sa.ScanrsError) as e:
                    x.to_adaptive_vecs(bad, major=major)
                assert e.value.code == ARGUMENT and "force_kind" in str(e.value)
        for bad in (2, -1, "outer"):
            with pytest.raises(sa.ScanrsError) as e:
                x.to_adaptive_vecs(None, major=bad)
            assert e.value.code == ARGUMENT and "major" in str(e.value)
        with pytest.raises(sa.ScanrsError):
            x.to_adaptive_vecs("D5")
    with pytest.raises(sa.ScanrsError) as e:
        h.export_info()  # an export the multi call did not make
    assert e.value.code == ARGUMENT and "scanrs_multi_to_adaptive" in str(e.value)
    out = ctypes.c_void_p(7)
    assert sa._lib.scanrs_multi_to_adaptive(mm._h, ctypes.c_int(3), ctypes.c_int(-1), ctypes.byref(out)) == ARGUMENT and out.value is None
    assert mm.export_info()["n_shards"] == 2  # the handle is as usable as before
    mm.close()


def test_no_device_memory_is_left_behind(sa, grid):
    mm = _grid_multi(sa, grid, 5000, 3)
    mm.to_adaptive_vecs(major="inner")  # (settles the shards' transposed copies, which they keep)
    mm.to_adaptive_vecs(major="stored")
    gc.collect()
    sa.release_cached_memory()
    start = sa.device_memory_in_use()
    for kind in (None, "D16", "S4"):
        mm.to_adaptive_vecs(kind, major="inner")
        mm.to_adaptive_vecs(kind, major="stored")
        mm.adaptive_info(kind, major="inner")
    mm.export_info()
    gc.collect()
    sa.release_cached_memory()
    assert sa.device_memory_in_use() == start
    h = sa.AdaptiveMat.from_csmat(25, 5000, sa.CSR, *ag.as_csmat(grid[5000]))
    h.to_adaptive_vecs(major="inner")
    gc.collect()
    sa.release_cached_memory()
    start = sa.device_memory_in_use()
    for kind in (None, "D16", "S4"):
        h.to_adaptive_vecs(kind, major="inner")
        h.to_adaptive_vecs(kind, major="stored")
    gc.collect()
    sa.release_cached_memory()
    assert sa.device_memory_in_use() == start
    mm.close()
