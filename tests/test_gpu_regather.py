"""MultiMat.gather_outer / rebalance against the route a caller had before: the selected triplet, made on the host by
tests/regather_ref.py, handed to MultiMat(...). Everything up to the solvers is integer work and compared with np.array_equal: the
shard ranges, every shard's arrays, the whole matrix, gather_info against host_plan_gather, and the bytes that crossed the host link
against their bound. All shards share device 0."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import regather_ref as ref  # noqa: E402
import reshard_ref  # noqa: E402
import select_ref as sref  # noqa: E402
import select_sharded_case as sc  # noqa: E402

ARGUMENT = 6  # SCANRS_ERR_ARGUMENT, and SCANRS_ERR_INVALID under its other name
# host_bytes per shard: at most 8 (outer extent + n_idx + n_shards + 1) and this constant: every source shard's indptr has one entry more
# than it has vectors, 8 bytes each for at most 16 sources, and all of them may be charged to one destination
HOST_BYTES_SLACK = 8 * 16
# (source shards, destination shards) per matrix: every count of {1, 2, 3, 5} on either side, equal and unequal, over the twelve
# (matrix, orientation) cases; every pair runs every list: 12 x 2 x 7 gathers, each against its own host-route MultiMat
PAIRS = {"seeded": ((2, 3), (5, 5)), "long_vector": ((3, 5), (1, 2)), "one_position": ((5, 2), (3, 3)), "zeros_and_max": ((1, 1), (2, 5)),
         "empty": ((3, 2), (2, 2)), "heavy_vector": ((2, 3), (5, 1))}


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


@functools.lru_cache(maxsize=None)
def case(name):
    """(n_outer, n_inner, triplet) with the sharded dimension outermost, computed once and read-only"""
    n_outer, n_inner, ip, ix, vv = ref.CASES[name]()
    for a in (ip, ix, vv):
        a.setflags(write=False)
    return n_outer, n_inner, (ip, ix, vv)


def shape_of(sa, storage, n_outer, n_inner):
    """genes x cells CSC: the cells (outer) are the columns; cells x genes CSR: the rows"""
    return (n_outer, n_inner) if storage == sa.CSR else (n_inner, n_outer)


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def in_use(sa):
    sa.release_cached_memory()
    return sa.device_memory_in_use()


def assert_equals_host_route(sa, got, storage, n_inner, triplet, n_dst, where):
    """`got` against MultiMat(...) of the triplet over n_dst shards: shape, ranges, every shard's arrays, the whole matrix"""
    n_sel = triplet[0].shape[0] - 1
    rows, cols = shape_of(sa, storage, n_sel, n_inner)
    host = sa.MultiMat(rows, cols, storage, *triplet, n_dst, devices=[0] * n_dst)
    assert got.storage == storage and got.shape() == [rows, cols] and got.n_shards == n_dst, where
    bounds = sa.plan_shards(triplet[0], n_dst)
    assert got.shard_ranges() == host.shard_ranges() == [(0, int(bounds[i]), int(bounds[i + 1])) for i in range(n_dst)], where
    for i in range(n_dst):
        assert same(got.shard_csmat(i), host.shard_csmat(i)), f"{where}: shard {i}"
    assert same(got.to_csmat(), triplet) and got.nnz() == triplet[1].shape[0], where
    host.close()


@pytest.mark.parametrize("storage_name", ["csc", "csr"])
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_gather_equals_host_route(sa, name, storage_name):
    storage = sa.CSC if storage_name == "csc" else sa.CSR
    n_outer, n_inner, (ip, ix, vv) = case(name)
    rows, cols = shape_of(sa, storage, n_outer, n_inner)
    for n_src, n_dst in PAIRS[name]:
        src = sa.MultiMat(rows, cols, storage, ip, ix, vv, n_src, devices=[0] * n_src)
        src_bounds = np.array([0] + [hi for _, _, hi in src.shard_ranges()], dtype=np.uint64)
        before = src.to_csmat()
        assert same(before, (ip, ix, vv))
        lists = ref.lists(n_outer, src_bounds)
        for list_name, idx in sorted(lists.items()):
            where = f"{name} {storage_name} {list_name} {n_src} -> {n_dst}"
            if list_name == "identity":  # the identity list through its own entry point, shard count and devices spelled out
                got = src.rebalance(n_dst, devices=[0] * n_dst)
            else:
                got = src.gather_outer(idx, n_dst, devices=[0] * n_dst)
            want = ref.select_outer(ip, ix, vv, idx)
            assert_equals_host_route(sa, got, storage, n_inner, want, n_dst, where)
            # what the call did, against the plan on the host
            info = got.gather_info()
            tip, bd, mv = sa.host_plan_gather(ip, src_bounds, idx, n_dst)
            assert info["n_src"] == n_src and np.array_equal(info["bounds"], bd) and np.array_equal(info["moved"], mv), where
            assert np.array_equal(got.balance()["shard_nnz"], tip[bd[1:].astype(np.int64)] - tip[bd[:-1].astype(np.int64)]), where
            # metadata only on the host link
            limit = 8 * (n_outer + idx.shape[0] + n_dst + 1) + HOST_BYTES_SLACK
            print(f"{where}: host_bytes {info['host_bytes'].tolist()} (limit {limit} each), moved {int(mv.sum())} nonzeros")
            assert info["host_bytes"].shape == (n_dst,) and int(info["host_bytes"].max()) <= limit, where
            assert int(info["host_bytes"].sum()) == 8 * (n_outer + n_src) + 4 * idx.shape[0] + 8 * n_dst, where
            assert all(got.counter(f"regather_{p}_us", i) >= 0 for p in ("plan", "pull", "finish") for i in range(n_dst))
            if list_name == "skip_shard" and n_src > 1:  # the list really takes nothing from one source shard
                assert np.any(info["moved"].sum(axis=1) == 0) or int(mv.sum()) == 0, where
            got.close()
            assert same(src.to_csmat(), before), f"{where}: the source changed"
        src.close()


def test_the_heavy_vector_spans_several_tiles():
    """The matrix built for the pull's tiles: one vector longer than two tiles, every other vector empty."""
    n_outer, _, (ip, _, _) = case("heavy_vector")
    lens = np.diff(ip.astype(np.int64))
    assert lens.max() > 2 * ref.TILE and lens.max() % ref.TILE != 0 and np.count_nonzero(lens) == 1 and n_outer > 16


# ---- chains -------------------------------------------------------------------------------------------------------------------------------
def _multi(sa, mat, n_shards):
    return sa.MultiMat(mat.shape[0], mat.shape[1], sa.CSC, *sref.triplet(mat, "csc"), n_shards, devices=[0] * n_shards)


def _plan_of_identity(sa, mm):
    """host_plan_gather for rebalance() of mm: (the balanced shard_nnz, bounds)"""
    ip = mm.to_csmat()[0]
    sb = np.array([0] + [hi for _, _, hi in mm.shard_ranges()], dtype=np.uint64)
    tip, bd, _ = sa.host_plan_gather(ip, sb, np.arange(ip.shape[0] - 1), mm.n_shards)
    return tip[bd[1:].astype(np.int64)] - tip[bd[:-1].astype(np.int64)], bd


@pytest.mark.parametrize("emptied", [False, True])
def test_rebalance_after_a_filter(sa, emptied):
    """partition_on_thresholds of the 61 x 157 matrix over 3 shards, then rebalance(). None of the thresholds of the sharded select
    tests empties exactly one of three shards of this matrix, so the second run first takes the middle shard's cells out with
    select_cols (its result keeps an EMPTY middle shard through the filter) and the first runs the (34, 13) filter as it is."""
    mat = sref.canonical(sc.seeded_matrix(), "csc")
    one = sa.AdaptiveMat.from_csmat(mat.shape[0], mat.shape[1], sa.CSC, *sref.triplet(mat, "csc"))
    mm = _multi(sa, mat, 3)
    thresholds = (34, 13)
    if emptied:
        ranges = mm.shard_ranges()
        keep = np.concatenate([np.arange(ranges[0][1], ranges[0][2]), np.arange(ranges[2][1], ranges[2][2])])
        mm, one, thresholds = mm.select_cols(keep), one.select_cols(keep), (3, 3)
    f, _, sel_r, sel_c = mm.partition_on_thresholds(*thresholds, residual=False)
    g, _, want_r, want_c = one.partition_on_thresholds(*thresholds)
    assert np.array_equal(sel_r, want_r) and np.array_equal(sel_c, want_c)
    unbalanced = f.balance()
    if emptied:
        assert unbalanced["shard_nnz"][1] == 0 and f.shard_ranges()[1][1] == f.shard_ranges()[1][2]
    want_nnz, want_bounds = _plan_of_identity(sa, f)
    b = f.rebalance()
    balanced = b.balance()
    print(f"filter {thresholds}, emptied {emptied}: shard_nnz {unbalanced['shard_nnz'].tolist()} (imbalance {unbalanced['imbalance']:.3f}) -> "
          f"{balanced['shard_nnz'].tolist()} ({balanced['imbalance']:.3f})")
    assert np.array_equal(balanced["shard_nnz"], want_nnz) and np.array_equal(b.gather_info()["bounds"], want_bounds)
    assert balanced["imbalance"] == 3.0 * int(want_nnz.max()) / int(want_nnz.sum()) <= unbalanced["imbalance"]
    # the bits of MultiMat(...) of the single handle's filtered triplet
    filtered = g.to_csmat()
    assert_equals_host_route(sa, b, sa.CSC, g.shape()[0], filtered, 3, "rebalance after a filter")
    # straight through rebalance(), the unbalanced intermediate freed: the same arrays
    f2, _, sel_r2, sel_c2 = mm.partition_on_thresholds(*thresholds, residual=False)
    b2 = f2.rebalance(consume=True)
    assert f2._h is None and np.array_equal(sel_r2, want_r) and np.array_equal(sel_c2, want_c) and b2.shard_ranges() == b.shard_ranges()
    assert all(same(b2.shard_csmat(i), b.shard_csmat(i)) for i in range(3)) and np.array_equal(b2.gather_info()["moved"], b.gather_info()["moved"])
    # ... and behind the select calls (the ascending list they allow along the sharded dimension)
    cols = np.arange(0, f.shape()[1], 2)
    s2 = f.select_cols(cols).rebalance(consume=True)
    assert_equals_host_route(sa, s2, sa.CSC, g.shape()[0], g.select_cols(cols).to_csmat(), 3, "select_cols, rebalanced")
    rows = np.arange(g.shape()[0])[::-1]
    s3 = f.select_rows(rows).rebalance(consume=True)
    assert_equals_host_route(sa, s3, sa.CSC, len(rows), g.select_rows(rows).to_csmat(), 3, "select_rows, rebalanced")


def test_a_source_made_by_from_csmat_inner(sa):
    n_outer, n_inner, ip, ix, vv = reshard_ref.CASES["seeded"]()  # feature-major: genes x cells CSR
    src = sa.MultiMat.from_csmat_inner(n_outer, n_inner, sa.CSR, ip, ix, vv, 3, devices=[0] * 3)
    cells, genes, (cip, cix, cvv) = case("seeded")
    assert src.storage == sa.CSC and same(src.to_csmat(), (cip, cix, cvv))
    idx = ref.lists(cells, [0, cells])["shuffle"]
    got = src.gather_outer(idx, 2, devices=[0, 0])
    src.close()
    assert_equals_host_route(sa, got, sa.CSC, genes, ref.select_outer(cip, cix, cvv, idx), 2, "from_csmat_inner source")
    with pytest.raises(sa.ScanrsError):
        got.create_info()  # the record of the inner-sharding constructor is the source's, not the result's


# ---- downstream -------------------------------------------------------------------------------------------------------------------------
def test_downstream(sa):
    """CellRanger normalisation + BkSvd(k = 7, explicit start panel), group_sums and kNN after a shuffled gather_outer over 3 shards. The
    shards are those of the host route, so the same code runs on the same arrays: U, sigma and V must be EQUAL. Against one handle
    sigma agrees to the suite's bound for shards against one handle (1e-8 relative); the integer results are equal."""
    from scanrs_amd import sseq

    cells, genes, (ip, ix, vv) = case("seeded")
    k = 7
    idx = ref.lists(cells, [0, cells])["shuffle"]
    src = sa.MultiMat(genes, cells, sa.CSC, ip, ix, vv, 2, devices=[0, 0])
    mm = src.gather_outer(idx, 3, devices=[0, 0, 0])
    src.close()
    tip, tix, tvv = ref.select_outer(ip, ix, vv, idx)
    host = sa.MultiMat(genes, cells, sa.CSC, tip, tix, tvv, 3, devices=[0, 0, 0])
    one = sa.AdaptiveMat.from_csmat(genes, cells, sa.CSC, tip, tix, tvv)
    labels = sc.seeded_labels()[idx.astype(np.int64)]
    sums1, cnt1 = sseq.group_sums(one, labels, sc.N_GROUPS)
    sums, cnt = sseq.group_sums(mm, labels, sc.N_GROUPS)
    assert np.array_equal(sums, sums1) and np.array_equal(cnt, cnt1)
    omega = np.random.default_rng(7).uniform(-1.0, 1.0, size=(2 * k, genes))  # rows < cols: (b x rows)
    u, s, v = mm.normalize(sa.Normalization.CellRanger).run_pca_bk(k, omega=omega)
    uh, sh, vh = host.normalize(sa.Normalization.CellRanger).run_pca_bk(k, omega=omega)
    print("sigma (gathered)  ", s, "\nsigma (host route)", sh)
    assert np.array_equal(s, sh) and np.array_equal(u, uh) and np.array_equal(v, vh)
    u1, s1, v1 = sa.BkSvd().run_pca(sa.normalize(one, sa.Normalization.CellRanger), k, omega=omega)
    rel = float(np.max(np.abs(s - s1) / s1))
    print("sigma against one handle: max relative difference", rel)
    assert rel < 1e-8
    assert np.array_equal(mm.knn(5, points=v1), sa.knn(v1, 5))


# ---- lifetime and refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source_first", [True, False])
def test_either_may_be_freed_first(sa, source_first):
    cells, genes, (ip, ix, vv) = case("seeded")
    before = in_use(sa)
    src = sa.MultiMat(genes, cells, sa.CSC, ip, ix, vv, 3, devices=[0] * 3)
    idx = ref.lists(cells, [0, cells])["repeats"]
    got = src.gather_outer(idx, 2, devices=[0, 0])
    want = ref.select_outer(ip, ix, vv, idx)
    first, second = (src, got) if source_first else (got, src)
    first.close()
    assert same(second.to_csmat(), want if source_first else (ip, ix, vv))
    if source_first:  # the result lives on with its own group: an exchange step still works
        sums = second.sum_rows(np.arange(idx.shape[0]), dtype=np.uint64)
        assert np.array_equal(sums, np.bincount(want[1], weights=want[2], minlength=genes).astype(np.uint64))
    second.close()
    assert in_use(sa) == before


def test_refusals(sa):
    cells, genes, (ip, ix, vv) = case("seeded")
    lib = sa._lib
    src = sa.MultiMat(genes, cells, sa.CSC, ip, ix, vv, 3, devices=[0] * 3)
    held = {"bytes": in_use(sa)}  # what the source holds on the device: a refused call leaves exactly this behind
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def refused(idx, n_idx, n_shards, devices, *words):
        out = ctypes.c_void_p(0x1234)
        dv = None if devices is None else (ctypes.c_int * len(devices))(*devices)
        rc = lib.scanrs_multi_gather_outer(src._h, p(idx), ctypes.c_uint64(n_idx), ctypes.c_uint32(n_shards), dv, ctypes.byref(out))
        msg = lib.scanrs_last_error().decode()
        assert rc == ARGUMENT and out.value is None and all(w in msg for w in words), (rc, msg)
        assert in_use(sa) == held["bytes"]

    ok = np.array([5, 0, 156], dtype=np.uint64)
    refused(np.array([5, 157, 0], dtype=np.uint64), 3, 2, [0, 0], "idx", "entry 1 of the list is 157", "157 outer vectors")
    refused(None, 3, 2, [0, 0], "idx", "null index list")
    refused(ok, 3, 17, None, "n_shards", "16")
    refused(ok, 3, 0, None, "n_shards")
    refused(ok, 3, 2, [0, 99], "device 99 of shard 1")
    refused(ok, 3, 2, [-1, 0], "device -1 of shard 0")
    with pytest.raises(sa.ScanrsError) as e:
        src.gather_info()
    assert e.value.code == ARGUMENT and "gather_info" in str(e.value)
    # the preconditions of select_rows: the identity map, no offset
    src.normalize(sa.Normalization.CellRanger)
    held["bytes"] = in_use(sa)  # (the map's arrays)
    refused(ok, 3, 2, [0, 0], "gather_outer", "scanrs_mat_reset_map")
    out = ctypes.c_void_p(0x1234)
    assert lib.scanrs_multi_rebalance(src._h, ctypes.c_uint32(0), None, ctypes.byref(out)) == ARGUMENT and out.value is None
    assert "scanrs_mat_reset_map" in lib.scanrs_last_error().decode()
    src.reset_map()
    got = src.gather_outer(ok, 2, devices=[0, 0])
    assert same(got.to_csmat(), ref.select_outer(ip, ix, vv, ok))
    got.close()
    # the empty list: what MultiMat(...) makes of a matrix without outer vectors, a valid matrix of empty shards
    none = src.gather_outer(np.zeros(0, dtype=np.uint64), 2, devices=[0, 0])
    assert none.shape() == [genes, 0] and none.nnz() == 0 and none.shard_ranges() == [(0, 0, 0), (0, 0, 0)]
    assert none.balance()["imbalance"] == 1.0 and none.balance()["shard_nnz"].tolist() == [0, 0]
    none.close()
    src.close()
