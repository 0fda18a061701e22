"""nearest_neighbors with a query set of its own and over sharded / multi-GPU point sets (umap-rs knn.rs:112-166).
"Equal" is np.array_equal on the indices and on the distance bit patterns, against the host twin (host_nearest_neighbors[_query]).
All shards share device 0: a MultiMat (the library cuts the cells), or handles bound with set_shard to explicit cuts with a host hook
that records the dtypes it carried (tests/shard_ring.py)."""
import contextlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import metric_knn_cases as cases  # noqa: E402
from shard_ring import Ring, run_ranks  # noqa: E402

KINDS = ("euclidean", "pearson", "cosine")
DEFAULT_BLOCK_ROWS = 262144
UMAX = 0xFFFFFFFF


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@contextlib.contextmanager
def options(sa, exhaustive=0, min_points=32768, block_rows=DEFAULT_BLOCK_ROWS):
    sa.set_global_option("knn_exhaustive", exhaustive)
    sa.set_global_option("knn_filter_min_points", min_points)
    sa.set_global_option("knn_block_rows", block_rows)
    try:
        yield
    finally:
        sa.set_global_option("knn_exhaustive", 0)
        sa.set_global_option("knn_filter_min_points", 32768)
        sa.set_global_option("knn_block_rows", DEFAULT_BLOCK_ROWS)


def same(got, want, label):
    assert got[0].shape == want[0].shape and got[0].dtype == np.uint32, (label, got[0].shape, want[0].shape)
    assert np.array_equal(got[0], want[0]), (label, "indices", int(np.sum(np.any(got[0] != want[0], axis=1))))
    assert np.array_equal(bits(got[1]), bits(want[1])), (label, "distance bits")


def ordered(idx, dist):
    """no list descends (key * key is monotone in the key; which of two equal distances comes first is checked on the planted rows)"""
    assert np.all((np.diff(dist, axis=1) >= 0) | (idx[:, 1:] == UMAX))


_TWIN = {}


def twin(sa, kind, x, k):
    """the host twin once per point set: the answer for a smaller k is a prefix of the answer for a larger one"""
    key = (kind, x.shape, hash(x.tobytes()))
    if key not in _TWIN or _TWIN[key][0].shape[1] < k:
        _TWIN[key] = sa.host_nearest_neighbors(x, max(k, 64), kind)
    idx, dist = _TWIN[key]
    return idx[:, :k], dist[:, :k]


def cell_matrix(n_cells):
    """a genes x cells CSC matrix with one count per cell: the handle only gives the transport and the range of cells"""
    return np.arange(n_cells + 1, dtype=np.uint64), np.zeros(n_cells, dtype=np.uint32), np.ones(n_cells, dtype=np.uint32)


class Hooked:
    """Handles bound with set_shard to explicit cuts, one thread per rank."""

    def __init__(self, sa, cuts):
        self.sa, self.cuts, self.world = sa, list(cuts), len(cuts) - 1
        self.ring = Ring(self.world)
        self.hs = []
        for r, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
            h = sa.AdaptiveMat.from_csmat(1, hi - lo, sa.CSC, *cell_matrix(hi - lo))
            h.set_shard(r, self.world, lo, cuts[-1], self.ring.hook(r))
            self.hs.append(h)

    def on_all(self, fn):
        """[result or exception] per rank"""
        out, err = run_ranks(self.world, lambda r: fn(r, self.hs[r]))
        return [o if e is None else e for o, e in zip(out, err)]

    def nn(self, pts, k, kind):
        out = self.on_all(lambda r, h: h.nearest_neighbors_sharded(pts, k, kind))
        for o in out:
            if isinstance(o, BaseException):
                raise o
        return np.concatenate([o[0] for o in out], axis=0), np.concatenate([o[1] for o in out], axis=0)

    def counters(self, key):
        return [h.counter(key) for h in self.hs]

    def close(self):
        pass


class Multi:
    """A MultiMat with all shards on device 0 (the library cuts the cells)."""

    def __init__(self, sa, n, world):
        self.world = world
        self.mm = sa.MultiMat(1, n, sa.CSC, *cell_matrix(n), world, devices=[0] * world)

    def nn(self, pts, k, kind):
        return self.mm.nearest_neighbors(k, pts, kind)

    def counters(self, key):
        return [self.mm.counter(key, shard=i) for i in range(self.world)]

    def close(self):
        self.mm.close()


# ---- 1. the query form, exhaustive route: every DMAX instance ------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 9, 17, 33, 53, 65, 128])
@pytest.mark.parametrize("n_q,n_p", [(1, 2), (257, 3), (300, 257), (257, 1500)])
def test_query_form_exhaustive_route_equals_the_host_twin(sa, n_q, n_p, d):
    p = cases.special_points(n_p, d)
    q = cases.special_points(n_q, d, seed=5)
    m = min(n_q, n_p, 40)
    q[:m:3] = p[:m:3]  # rows the two sets share, at the same row number: what include_self=False drops
    with options(sa, exhaustive=1):
        for kind in KINDS:
            for include_self in (True, False):
                want = sa.host_nearest_neighbors_query(q, p, 128, kind, include_self)
                for k in (1, 15, 128):
                    got = sa.nearest_neighbors_query(q, p, k, kind, include_self)
                    ke = min(k, n_p)
                    same(got, (want[0][:, :ke], want[1][:, :ke]), (kind, n_q, n_p, d, k, include_self))
                    assert not sa.debug_knn_last_stats()["filtered"]
        with pytest.raises(sa.ScanrsError, match="k must not exceed 128"):
            sa.nearest_neighbors_query(q, p, 129, "cosine")


def test_query_form_of_the_point_set_itself_is_nearest_neighbors(sa):
    x = cases.special_points(257, 50)
    for kind in KINDS:
        got = sa.nearest_neighbors_query(x, x, 15, kind, include_self=False)
        same(got, sa.nearest_neighbors(x, 15, kind), kind)
        same(got, sa.host_nearest_neighbors(x, 15, kind), kind)


def test_query_form_on_device_sets_with_leading_dimensions_and_nan_behind_the_columns(sa):
    import torch

    p, q = cases.special_points(257, 50), cases.special_points(300, 50, seed=3)
    tp = torch.full((257, 64), float("nan"), dtype=torch.float64, device="cuda")
    tq = torch.full((300, 57), float("nan"), dtype=torch.float64, device="cuda")
    tp[:, :50] = torch.from_numpy(p).cuda()
    tq[:, :50] = torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    for kind in KINDS:
        for include_self in (True, False):
            got = sa.nearest_neighbors_query_device(tq.data_ptr(), 300, 57, tp.data_ptr(), 257, 64, 50, 15, kind, include_self)
            same(got, sa.host_nearest_neighbors_query(q, p, 15, kind, include_self), (kind, include_self))
    for ld_q, ld_p in ((49, 64), (57, 49)):
        with pytest.raises(sa.ScanrsError, match="leading dimension"):
            sa.nearest_neighbors_query_device(tq.data_ptr(), 300, ld_q, tp.data_ptr(), 257, ld_p, 50, 15, "cosine")


# ---- 2. the query form, filtered route ----------------------------------------------------------------------------------------------------
N_FILTER = 4096


@pytest.mark.parametrize("kind", ["pearson", "cosine"])
@pytest.mark.parametrize("d", [2, 50, 58])
def test_query_form_filtered_route_equals_the_exhaustive_route_and_the_host_twin(sa, kind, d):
    p = cases.clustered_points(N_FILTER, d)
    qs = cases.clustered_points(300, d, seed=9)
    qs[::7] = p[:300:7]
    want = {s: sa.host_nearest_neighbors_query(qs, p, 64, kind, s) for s in (True, False)}
    for n_q in (256, 300):
        q = qs[:n_q]
        for k in (15, 64):
            for include_self in (True, False):
                with options(sa, min_points=1024):
                    got = sa.nearest_neighbors_query(q, p, k, kind, include_self)
                    st = sa.debug_knn_last_stats()
                assert st["filtered"] and st["rounds"][-1]["stride"] == 1 and st["rounds"][-1]["points"] == N_FILTER, st
                if kind == "pearson" and d == 2:  # every row standardises to +-(1, -1) / sqrt 2: the overflow redo answers
                    assert st["rounds"][-1]["overflowed"] > 0, st
                with options(sa, exhaustive=1):
                    plain = sa.nearest_neighbors_query(q, p, k, kind, include_self)
                    assert not sa.debug_knn_last_stats()["filtered"]
                same(got, plain, (kind, d, n_q, k, include_self, "filtered against exhaustive"))
                w = want[include_self]
                same(got, (w[0][:n_q, :k], w[1][:n_q, :k]), (kind, d, n_q, k, include_self, "against the host twin"))


def _declines(sa, q, p, k, kind, label):
    with options(sa, min_points=1024):
        got = sa.nearest_neighbors_query(q, p, k, kind)
        assert not sa.debug_knn_last_stats()["filtered"], (label, "the filter should have declined")
    same(got, sa.host_nearest_neighbors_query(q, p, k, kind), label)


def test_query_form_filter_declines_where_it_must(sa):
    p, q = cases.clustered_points(N_FILTER, 50), cases.clustered_points(300, 50, seed=9)
    for kind, flat in (("pearson", 0.75), ("cosine", 0.0)):
        _declines(sa, q[:255], p, 15, kind, "255 queries")
        _declines(sa, cases.clustered_points(300, 59, seed=9), cases.clustered_points(N_FILTER, 59), 15, kind, "d = 59")
        _declines(sa, q, p, 65, kind, "k = 65")
        for side in ("queries", "points"):
            for what, value in (("degenerate row", None), ("s_xx below the window", 1e-130), ("s_xx above the window", 1e130)):
                q2, p2 = q.copy(), p.copy()
                target = q2 if side == "queries" else p2
                if value is None:
                    target[77] = flat
                else:
                    target[77] *= value
                _declines(sa, q2, p2, 15, kind, (kind, side, what))
    with options(sa, min_points=1024):  # and just inside, it takes the shape
        sa.nearest_neighbors_query(q[:256], p[:1025], 15, "cosine")
        assert sa.debug_knn_last_stats()["filtered"]


# ---- 3. sharded, exhaustive -----------------------------------------------------------------------------------------------------------
N_SHARD = 1500


@pytest.fixture(scope="module")
def shard_points(sa):
    x = cases.special_points(N_SHARD, 50)
    return x, {kind: sa.host_nearest_neighbors(x, 128, kind) for kind in KINDS}


def _sharded_case(sa, shard_points, run, shards):
    x, want = shard_points
    for block_rows in (64, 1000, DEFAULT_BLOCK_ROWS):
        n_blocks = -(-N_SHARD // block_rows)
        with options(sa, block_rows=block_rows):
            for kind in KINDS:
                for k in (15, 128):
                    got = run.nn(x, k, kind)
                    same(got, (want[kind][0][:, :k], want[kind][1][:, :k]), (kind, k, block_rows))
                    assert run.counters("knn_blocks") == [n_blocks] * shards
                    assert run.counters("knn_allreduces") == [n_blocks + 1] * shards
                    assert run.counters("knn_blocks_filtered") == [0] * shards


@pytest.mark.parametrize("world", [1, 2, 3])
def test_multimat_exhaustive_equals_the_whole_set(sa, shard_points, world):
    run = Multi(sa, N_SHARD, world)
    try:
        _sharded_case(sa, shard_points, run, world)
    finally:
        run.close()


@pytest.mark.parametrize("cuts", [[0, 0, 700, 1500], [0, 1, 1499, 1500]])
def test_hooked_cuts_exhaustive_equal_the_whole_set(sa, shard_points, cuts):
    run = Hooked(sa, cuts)
    _sharded_case(sa, shard_points, run, len(cuts) - 1)
    assert run.ring.dtypes == {1}  # only integers cross the shards


# ---- 4. sharded, filtered inside blocks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pearson", "cosine"])
def test_sharded_blocks_through_the_filter(sa, kind):
    x = cases.clustered_points(N_FILTER, 50)
    with options(sa, min_points=1024):
        whole_filtered = sa.nearest_neighbors(x, 15, kind)
        assert sa.debug_knn_last_stats()["filtered"]
    with options(sa, exhaustive=1):
        whole_plain = sa.nearest_neighbors(x, 15, kind)
    run = Multi(sa, N_FILTER, 2)
    try:
        with options(sa, min_points=1024, block_rows=2048):
            got = run.nn(x, 15, kind)
            assert run.counters("knn_blocks_filtered") == [2, 2] and run.counters("knn_blocks") == [2, 2]
            same(got, whole_filtered, (kind, "unsharded filtered"))
            same(got, whole_plain, (kind, "unsharded exhaustive"))
            same(got, twin(sa, kind, x, 15), (kind, "host twin"))
            y = x.copy()
            y[3000] = 0.75 if kind == "pearson" else 0.0  # one degenerate row, in the second block only
            got = run.nn(y, 15, kind)
            # Shard 0 filters the first block and declines the second. The row is also a QUERY of shard 1 (the shard cut and the
            # block cut coincide at 2048), and a block takes the filter only when no local query row is degenerate: shard 1 filters none.
            assert run.counters("knn_blocks_filtered") == [1, 0]
            same(got, twin(sa, kind, y, 15), (kind, "degenerate row in block 2"))
    finally:
        run.close()


# ---- 5. ties across block and shard boundaries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("route", ["filtered", "exhaustive"])
def test_ties_across_boundaries_go_by_global_index(sa, kind, route):
    x = cases.clustered_points(N_FILTER, 50)
    for r in (10, 2058, 4000):
        x[r] = x[3]  # exact duplicates on both sides of the block and shard boundary at 2048
    x[2049] = 2.5 * x[5]  # positive multiples of one another: cosine D = 0
    want = twin(sa, kind, x, 15)
    run = Multi(sa, N_FILTER, 2)
    try:
        with options(sa, min_points=1024, block_rows=2048, exhaustive=1 if route == "exhaustive" else 0):
            got = run.nn(x, 15, kind)
            if kind != "euclidean":
                assert run.counters("knn_blocks_filtered") == ([2, 2] if route == "filtered" else [0, 0])
    finally:
        run.close()
    same(got, want, (kind, route))
    ordered(*got)
    for r in (3, 10, 2058, 4000):  # the other three copies lead the list with one and the same key, in ascending global index
        others = [t for t in (3, 10, 2058, 4000) if t != r]
        assert list(got[0][r, :3]) == others and len(set(bits(got[1][r, :3]).tolist())) == 1, (r, got[0][r, :4], got[1][r, :4])
    if kind == "cosine":
        assert got[0][5, 0] == 2049 and got[0][2049, 0] == 5


# ---- 6. the scores a PCA left on the devices ----------------------------------------------------------------------------------------------
def test_scores_of_a_pca_on_two_shards(sa):
    from scanrs_amd.synth import synth_counts

    m = synth_counts(n_cells=1500, n_genes=600, density=0.05, seed=11)
    mm = sa.MultiMat(m.shape[1], m.shape[0], sa.CSC, m.indptr, m.indices, m.data, 2, devices=[0, 0])
    try:
        with pytest.raises(sa.ScanrsError) as e:
            mm.nearest_neighbors(15, distance="cosine")
        assert e.value.code == 6 and "no PCA result" in str(e.value)
        mm.normalize(sa.Normalization.CellRanger)
        u, s, v = mm.run_pca_bk(10)
        for kind in KINDS:
            same(mm.nearest_neighbors(15, distance=kind), sa.host_nearest_neighbors(v, 15, kind), kind)
    finally:
        mm.close()


# ---- 7. refusals: every rank returns the error, nobody hangs ---------------------------------------------------------------------------
def test_refusals_on_every_rank(sa):
    x = cases.clustered_points(97, 5)
    cuts = [0, 40, 42, 97]
    run = Hooked(sa, cuts)
    for value in (np.nan, np.inf, -np.inf):
        bad = x.copy()
        bad[41, 1] = value  # in the middle shard (rows 40, 41)
        bad[90, 0] = value  # a later row of another shard: the FIRST offending global row is named
        for o in run.on_all(lambda r, h: h.nearest_neighbors_sharded(bad, 5, "pearson")):
            assert isinstance(o, sa.ScanrsError) and o.code == 6 and "row 41 " in str(o), o
    for o in run.on_all(lambda r, h: h.nearest_neighbors_sharded(x, 129, "cosine")):
        assert isinstance(o, sa.ScanrsError) and o.code == 6 and "k must not exceed 128" in str(o), o
    for o in run.on_all(lambda r, h: h.nearest_neighbors_sharded(x, 5, "cosine" if r == 1 else "pearson")):
        assert isinstance(o, sa.ScanrsError) and o.code == 6 and "disagree" in str(o), o
    for o in run.on_all(lambda r, h: h.nearest_neighbors_sharded(x, 4 if r == 1 else 5, "euclidean")):
        assert isinstance(o, sa.ScanrsError) and o.code == 6 and "disagree" in str(o), o
    import torch

    t = torch.zeros((97, 8), dtype=torch.float64, device="cuda")
    for o in run.on_all(lambda r, h: h.nearest_neighbors_sharded((t.data_ptr() + 64 * cuts[r], 4, 5), 5, "cosine", device=True)):
        assert isinstance(o, sa.ScanrsError) and o.code == 6 and "leading dimension" in str(o), o
    for kind in KINDS:  # the handles stay usable; k = 0 gives nothing
        same(run.nn(x, 5, kind), sa.host_nearest_neighbors(x, 5, kind), kind)
        idx, dist = run.nn(x, 0, kind)
        assert idx.shape == (97, 0) and dist.shape == (97, 0)


@pytest.mark.parametrize("kind", KINDS)
def test_fewer_than_two_points_give_padding_only(sa, kind):
    import ctypes

    x = cases.clustered_points(4, 5)
    one = Hooked(sa, [0, 0, 1])  # n = 1: an empty rank and a rank with the only row
    out = one.on_all(lambda r, h: h.nearest_neighbors_sharded(x[:1], 3, kind))
    assert [o[0].shape for o in out] == [(0, 0), (1, 0)]
    # the C entry point writes n_local x k of padding
    idx, dist = np.zeros((1, 3), dtype=np.uint32), np.zeros((1, 3))
    pts = np.ascontiguousarray(x[:1])

    def raw(r, h):
        if r == 0:
            return sa._lib.scanrs_nearest_neighbors_sharded(h._h, pts.ctypes.data_as(ctypes.c_void_p), 0, 5, 5, 3, sa.DISTANCE_TYPES[kind], None, None)
        return sa._lib.scanrs_nearest_neighbors_sharded(h._h, pts.ctypes.data_as(ctypes.c_void_p), 0, 5, 5, 3, sa.DISTANCE_TYPES[kind],
                                                        idx.ctypes.data_as(ctypes.c_void_p), dist.ctypes.data_as(ctypes.c_void_p))

    assert one.on_all(raw) == [0, 0]
    assert np.all(idx == UMAX) and np.all(np.isposinf(dist))
    three = Hooked(sa, [0, 1, 3])  # n = 3, k = 5: columns 2 .. 4 are padding
    got = three.nn(x[:3], 5, kind)
    same(got, sa.host_nearest_neighbors(x[:3], 5, kind), kind)


def test_unsharded_handle_is_the_plain_call(sa):
    x = cases.special_points(257, 9)
    h = sa.AdaptiveMat.from_csmat(1, 257, sa.CSC, *cell_matrix(257))
    for kind in KINDS:
        same(h.nearest_neighbors_sharded(x, 15, kind), sa.nearest_neighbors(x, 15, kind), kind)
    assert h.counter("knn_blocks") == 0 and h.counter("knn_allreduces") == 0 and h.counter("knn_blocks_filtered") == 0
