"""nearest_neighbors with a query set of its own and over a sharded point set, without a device: the host twin
against the numpy restatement (tests/metric_knn_sharded_ref.py) bit for bit, that restatement against the plain-Python one
(tests/metric_knn_ref.py), the block model (cuts, blocks, strict seed, merge by (key, global index)) against one pass, and the
interface."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import metric_knn_cases as cases  # noqa: E402
import metric_knn_ref as plain  # noqa: E402
import metric_knn_sharded_ref as ref  # noqa: E402

ROOT = os.path.dirname(TESTS)
KINDS = ("pearson", "cosine")
NEW_SYMBOLS = ("scanrs_nearest_neighbors_query", "scanrs_nearest_neighbors_query_device", "scanrs_host_nearest_neighbors_query",
               "scanrs_nearest_neighbors_sharded", "scanrs_multi_nearest_neighbors")


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want, label):
    assert got[0].shape == want[0].shape, (label, got[0].shape, want[0].shape)
    assert np.array_equal(got[0], want[0]), (label, "indices")
    assert np.array_equal(bits(got[1]), bits(want[1])), (label, "distance bits")


# ---- the restatement itself -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_the_numpy_restatement_is_the_plain_python_one(kind):
    x = cases.special_points(65, 3)
    idx, dist = ref.nearest_neighbors_query(kind, x, x, 64, include_self=False)
    want_i, want_d = plain.nearest_neighbors(x.tolist(), 64, kind)
    assert np.array_equal(idx, np.asarray(want_i, dtype=np.uint32))
    assert np.array_equal(bits(dist), bits(np.asarray(want_d)))


# ---- the host twin of the query form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3, 50, 128])
@pytest.mark.parametrize("n_p", [1, 2, 65, 257])
@pytest.mark.parametrize("kind", KINDS)
def test_the_host_twin_equals_the_restatement_bit_for_bit(sa, kind, n_p, d):
    p = cases.special_points(n_p, d)
    for n_q in (1, 3, 65):
        q = cases.special_points(n_q, d, seed=5)
        m = min(n_q, n_p)
        q[:m:2] = p[:m:2]  # rows the sets share at the same row number
        for include_self in (True, False):
            want = ref.nearest_neighbors_query(kind, q, p, n_p + 3, include_self)
            for k in (1, 15, n_p, n_p + 3):
                got = sa.host_nearest_neighbors_query(q, p, k, kind, include_self)
                ke = min(k, n_p)
                same(got, (want[0][:, :ke], want[1][:, :ke]), (kind, n_q, n_p, d, k, include_self))
            # the C entry point pads behind the admissible points
            idx, dist = np.zeros((n_q, n_p + 3), dtype=np.uint32), np.zeros((n_q, n_p + 3))
            rc = sa._lib.scanrs_host_nearest_neighbors_query(q.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(n_q), p.ctypes.data_as(ctypes.c_void_p),
                                                             ctypes.c_uint64(n_p), ctypes.c_uint32(d), ctypes.c_uint32(n_p + 3),
                                                             ctypes.c_int(sa.DISTANCE_TYPES[kind]), ctypes.c_int(int(include_self)),
                                                             idx.ctypes.data_as(ctypes.c_void_p), dist.ctypes.data_as(ctypes.c_void_p))
            assert rc == 0
            same((idx, dist), want, (kind, n_q, n_p, d, "padded", include_self))
            assert np.all(idx[:, n_p:] == ref.U32MAX) and np.all(np.isposinf(dist[:, n_p:]))


@pytest.mark.parametrize("kind", ("euclidean",) + KINDS)
def test_the_point_set_as_its_own_queries_is_host_nearest_neighbors(sa, kind):
    for n, d in ((65, 3), (257, 50)):
        x = cases.special_points(n, d)
        for k in (1, 15, n + 3):
            got = sa.host_nearest_neighbors_query(x, x, k, kind, include_self=False)
            want = sa.host_nearest_neighbors(x, k, kind)
            ke = want[0].shape[1]  # min(k, n - 1); the query form is min(k, n) wide and padded in the last column
            same((got[0][:, :ke], got[1][:, :ke]), want, (kind, n, d, k))
            assert np.all(got[0][:, ke:] == ref.U32MAX)


def test_refusals_of_the_host_twin_name_the_set(sa):
    p, q = cases.special_points(65, 3), cases.special_points(3, 3)
    for value in (np.nan, np.inf, -np.inf):
        bad = q.copy()
        bad[2, 1] = value
        with pytest.raises(sa.ScanrsError, match="row 2 of the queries") as e:
            sa.host_nearest_neighbors_query(bad, p, 4, "cosine")
        assert e.value.code == 6
        bad = p.copy()
        bad[40, 0] = value
        with pytest.raises(sa.ScanrsError, match="row 40 of the points"):
            sa.host_nearest_neighbors_query(q, bad, 4, "pearson")
    with pytest.raises(sa.ScanrsError, match="dimensions"):
        sa.host_nearest_neighbors_query(np.ones((2, 129)), np.ones((5, 129)), 2, "cosine")
    with pytest.raises(sa.ScanrsError, match="distance"):
        sa.host_nearest_neighbors_query(q, p, 2, 7)
    idx, dist = sa.host_nearest_neighbors_query(q, p, 0, "cosine")
    assert idx.shape == (3, 0) and dist.shape == (3, 0)


# ---- the block model ----------------------------------------------------------------------------------------------------------------------
BLOCK_N = 96
BLOCK_CUTS = ([0, 0, 48, 96], [0, 47, 48, 96], [0, 7, 8, 50, 96])  # an empty shard, one-row shards, a cut off the block boundaries


def tie_pair(kind, q, base, rng):
    """two rows near `base` whose D against q differs while sqrt(D) ties (the square root halves the spacing of the doubles in
    [1/4, 1)): (row with the smaller D, row with the larger D)"""
    cand = base * (1.0 + 4e-16 * rng.standard_normal((400, len(base))))
    c, s = ref.prepare_rows(kind, np.vstack([q, cand]))
    key, val = ref.keys_of(c[0], s[0], c[1:], s[1:])
    for a in range(len(cand)):
        for b in range(a + 1, len(cand)):
            if key[a] == key[b] and val[a] != val[b]:
                return (cand[a], cand[b]) if val[a] < val[b] else (cand[b], cand[a])
    raise AssertionError("no pair with distinct D and equal sqrt(D) among the candidates")


def boundary_points(kind, smaller_first):
    """96 x 3 with, on both sides of the boundary at 48 (a block boundary of block_rows 1 and 48 and a shard boundary of the cuts): a
    pair of rows whose D against row 0 differs and whose keys tie (rows 47 | 48), and exact duplicates of row 1 (rows 1, 40 | 53, 90)."""
    rng = np.random.default_rng(96 + (kind == "pearson"))
    x = rng.standard_normal((BLOCK_N, 3))
    x[0] = [1.0, 0.25, -0.5]
    lo, hi = tie_pair(kind, x[0], np.array([0.9, -0.4, 0.3]), rng)
    x[47], x[48] = (lo, hi) if smaller_first else (hi, lo)
    for r in (40, 53, 90):
        x[r] = x[1]
    return x


@pytest.mark.parametrize("smaller_first", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_the_block_model_equals_one_pass(kind, smaller_first):
    x = boundary_points(kind, smaller_first)
    c, s = ref.prepare_rows(kind, x)
    key, val = ref.keys_of(c[0], s[0], c, s)
    assert key[47] == key[48] and val[47] != val[48] and (val[47] < val[48]) == smaller_first  # the planted tie is one
    # rows 47 and 48 tie for row 0: the smaller INDEX wins, whichever D is smaller
    first = ref.nearest_neighbors_query(kind, x, x, BLOCK_N, include_self=False)[0][0]
    pos = {int(p): i for i, p in enumerate(first)}
    assert pos[47] + 1 == pos[48] and len(np.flatnonzero(key == key[47])) == 2
    # k = pos + 1 puts row 0's k-th key on row 47 when the block of row 48 arrives: the strict seed must drop row 48, and only it
    for k in sorted({1, 3, pos[47] + 1, pos[47] + 2, BLOCK_N + 3}):
        one = ref.nearest_neighbors_query(kind, x, x, k, include_self=False)
        for r in (1, 40, 53, 90):  # the duplicates come in ascending index, whatever the query
            others = [t for t in (1, 40, 53, 90) if t != r]
            assert list(one[0][r, : min(k, 3)]) == others[: min(k, 3)]
        for cuts in BLOCK_CUTS:
            for block_rows in (1, 7, 48, BLOCK_N):
                got = ref.sharded_model(kind, x, cuts, block_rows, k)
                same(got, one, (kind, k, cuts, block_rows))


def test_the_block_model_on_the_special_inputs(sa):
    x = cases.special_points(65, 3)  # degenerate rows, 1e+-200, keys of +inf: the seed of +inf must let a key of +inf in
    for kind in KINDS:
        for k in (1, 15, 64, 70):
            one = ref.nearest_neighbors_query(kind, x, x, k, include_self=False)
            ke = min(k, 64)
            host = sa.host_nearest_neighbors(x, k, kind)
            same((one[0][:, :ke], one[1][:, :ke]), host, (kind, k, "host twin"))
            for cuts in ([0, 65], [0, 0, 20, 65], [0, 1, 64, 65]):
                for block_rows in (1, 7, 64, 65):
                    same(ref.sharded_model(kind, x, cuts, block_rows, k), one, (kind, k, cuts, block_rows))


# ---- the interface ------------------------------------------------------------------------------------------------------------------------
def test_the_interface_is_declared_mirrored_and_exported(sa):
    hdr = open(os.path.join(ROOT, "include", "scanrs_amd.h")).read()
    hpp = open(os.path.join(ROOT, "include", "scanrs_amd.hpp")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(sa.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, code), f"{name} is not declared in scanrs_amd.h"
        assert name in hpp, f"{name} is not mirrored in scanrs_amd.hpp"
        assert name in sa.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"%s \(knn\.rs:112-166" % name, hdr), f"{name} does not cite the reference"
    assert '"knn_blocks_filtered"' in hdr  # the new counter is documented
    block = hdr[hdr.index("nearest_neighbors under Euclidean, Pearson and cosine distance"):]
    block = block[: block.index("*/", block.index("NOT provided"))]
    not_provided = block[block.index("NOT provided"):].split(".")[0]
    assert "sharded" not in not_provided and "query set" not in not_provided, not_provided
    for fn in ("nearest_neighbors_query", "nearest_neighbors_query_device", "host_nearest_neighbors_query"):
        assert callable(getattr(sa, fn)), fn
    assert callable(sa.AdaptiveMat.nearest_neighbors_sharded) and callable(sa.MultiMat.nearest_neighbors)
