"""The bf16-MFMA filter of the kNN search (knn.hip) on the device, pinned down on SMALL point sets ("knn_filter_min_points" = 0)
built to make bf16 rounding add up (tests/knn_filter_ref.py): one filter pass alone through scanrs_debug_knn_filter (complete:
no true neighbour missing; selective: nothing far beyond the margin, overflow as the CPU model predicts), the whole search against
the float64 reference bit for bit, the tile edges of the filter kernel, the routing rules and the magnitude window.

What these inputs did to the search before the margin was re-derived (gamma = 0.0021, clamp = sentinel = 1e30, no magnitude window),
measured once on an MI355X: rows of knn(v, 15) that differ from the float64 reference, with the kernels of the commit before
(whose parking buffer sent many queries of such small sets to the exhaustive kernel, which hides errors) / with the present kernels
and only the margin set back:
    u12_2d 17 / 21 of 2048, circle 0 / 0 of 4096, worst_2d 213 / 213 of 4096, worst_3d 0 / 0, worst_5d 0 / 0,
    worst_2d_towards_zero 0 / 0, worst_2d_signed 7 / 7 of 2048, worst_2d_up40 and _down40 472 / 472 of 2048,
    box_one_bf16_cell 2048 / 2048 of 2048 (every row all padding), u12_1d 281 / 647 of 4096, gauss_50d, gauss_2d, pca_like 0 / 0.
The CPU model of tests/knn_filter_ref.py says 21, 0, 215, 0, 0, 0, 7, 473, 473, 2048, 647, 0, 0, 0 for the second column. With the
old margin a single pass with tau = 0 (k = 1) does not even find the query itself on the worst_* sets: q~.q~ falls short of |q|^2 by
more than 2 gamma |q|^2."""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import knn_filter_ref as kr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


@pytest.fixture(scope="module")
def params(sa):
    return sa.debug_knn_filter_params()


@pytest.fixture(scope="module", params=kr.CASES)
def name(request):
    """module scope: pytest then runs all tests of one builder case together, and its float64 reference is computed once"""
    return request.param


@contextlib.contextmanager
def small_sets_filtered(sa, ratio=4):
    sa.set_global_option("knn_filter_min_points", 0)
    sa.set_global_option("knn_ratio", ratio)
    sa.set_global_option("knn_exhaustive", 0)
    try:
        yield
    finally:
        sa.set_global_option("knn_filter_min_points", 32768)
        sa.set_global_option("knn_ratio", 4)
        sa.set_global_option("knn_exhaustive", 0)


def exhaustive(sa, fn):
    sa.set_global_option("knn_exhaustive", 1)
    try:
        return fn()
    finally:
        sa.set_global_option("knn_exhaustive", 0)


def check_pass(params, q, p, d2, tau, stride, cnt, cand, label):
    """one filter pass: well-formed lists, complete, selective. Returns the overflow mask."""
    cap, gamma = params["cap"], params["gamma"]
    n_q, n_p = d2.shape
    over = cnt > cap
    slots = (np.arange(cap)[None, :] < cnt[:, None]) & ~over[:, None]  # what an overflowed list holds is nobody's business
    assert np.all(cand[~over][~slots[~over]] == kr.UMAX), label  # nothing written behind a list's end
    rows, vals = np.nonzero(slots)[0], cand[slots].astype(np.int64)
    assert vals.size == 0 or vals.max() < n_p, (label, "index past the points (a sentinel row?)")
    assert np.all(vals % stride == 0), (label, "point off the stride")
    member = np.zeros((n_q, n_p), dtype=bool)
    member[rows, vals] = True
    assert np.array_equal(member.sum(axis=1)[~over], cnt[~over]), (label, "duplicate in a list")
    on_stride = np.zeros(n_p, dtype=bool)
    on_stride[::stride] = True
    need = (d2 <= tau[:, None]) & on_stride[None, :]
    assert np.all(cnt >= need.sum(axis=1)), (label, "fewer candidates than true neighbours: an overflowed query must count past the cap")
    missing = (need & ~member)[~over]
    assert not missing.any(), (label, f"{int(missing.any(axis=1).sum())} queries miss a true neighbour")
    qn, pn = np.sum(q * q, axis=1), np.sum(p * p, axis=1)
    with np.errstate(invalid="ignore"):
        far = member & (d2 > tau[:, None] + 4.0 * gamma * (1.0 + 1e-3) * (qn[:, None] + pn[None, :]))
    assert not far.any(), (label, f"{int(far.sum())} candidates beyond the margin")
    return over


def overflow_tolerance(model_cnt, cap):
    """queries whose model count sits within 2 % of the cap may overflow on one side only (f32 summation order at the margin's edge)"""
    return int(((model_cnt > 0.98 * cap) & (model_cnt < 1.02 * cap)).sum())


def test_filter_pass_is_complete_and_selective(sa, params, name):
    v, d2 = kr.case(name)
    for stride in (1, 4):
        sub = d2[:, ::stride]
        for k in (1, 15, 64):
            tau = kr.kth_d2(sub, k)  # the exact k-th distance (the query itself included: this pass drops nothing)
            cnt, cand = sa.debug_knn_filter(v, v, tau, stride)
            over = check_pass(params, v, v, d2, tau, stride, cnt, cand, (name, stride, k))
            model = kr.filter_pass(v, v[::stride], tau, params["gamma"]).sum(axis=1)
            print(f"{name} stride {stride} k {k}: mean candidates {cnt.mean():.1f} max {cnt.max()} overflowed {int(over.sum())} (model {int((model > params['cap']).sum())})")
            assert abs(int(over.sum()) - int((model > params["cap"]).sum())) <= overflow_tolerance(model, params["cap"]), (name, stride, k)
            if name in kr.SELECTIVE:
                assert not over.any(), (name, stride, k)


def test_search_equals_the_float64_reference(sa, params, name):
    v, d2 = kr.case(name)
    n, k, cap = v.shape[0], 15, params["cap"]
    with small_sets_filtered(sa):
        got = sa.knn(v, k)
        st = sa.debug_knn_last_stats()
        got_find = {inc: sa.find_nn(v[:300], k, v, inc) for inc in (True, False)}
        st_find = sa.debug_knn_last_stats()
    want = kr.rank(d2, k, drop_self=True)
    print(f"{name}: {int(np.any(got.astype(np.int64) != want, axis=1).sum())} of {n} rows differ from the reference; {st}")
    assert np.array_equal(got.astype(np.int64), want)
    assert np.array_equal(got_find[True].astype(np.int64), kr.rank(d2[:300], k))
    assert np.array_equal(got_find[False].astype(np.int64), kr.rank(d2[:300], k, drop_self=True))
    # ... and it was the filter that answered, with as many fallbacks as the model says
    st0, strides = kr.search_strides(n, 4, cap)
    assert st["filtered"] and st_find["filtered"] and st["first_stride"] == st0 and [r["stride"] for r in st["rounds"]] == strides
    for rd, (stride, model_cnt, _) in zip(st["rounds"], kr.model_search(v, d2, k, params["gamma"], cap=cap)):
        assert rd["points"] == (n + stride - 1) // stride and rd["cand_max"] >= rd["cand_sum"] / n
        assert abs(rd["overflowed"] - int((model_cnt > cap).sum())) <= overflow_tolerance(model_cnt, cap), (name, rd)
        if name in kr.SELECTIVE:
            assert rd["overflowed"] == 0 and rd["cand_max"] <= cap, (name, rd)
        if name == "box_one_bf16_cell":  # all points share one bf16 cell: every query falls back, and the answer is still exact
            assert rd["overflowed"] == n


EDGES = [  # n_q, n_p, d, k, knn_ratio: the 128-row query tile, the 32-point block and its sentinel row, block counts off the
    # 12-block ring, first stride 2 -> 4 at 2048 -> 2049, the widest operand rows, one and three filter rounds
    (256, 1025, 1, 1, 4), (257, 1056, 57, 64, 2), (383, 1057, 58, 1, 16), (384, 2047, 3, 64, 4),
    (257, 4097, 58, 64, 4), (384, 2049, 2, 1, 2), (256, 2048, 57, 1, 16), (383, 4097, 1, 64, 2),
]


@pytest.mark.parametrize("n_q,n_p,d,k,ratio", EDGES)
def test_tile_edges(sa, params, n_q, n_p, d, k, ratio):
    rng = np.random.default_rng(n_q * 10007 + n_p)
    if d <= 3:  # off-centre, every coordinate at its worst rounding; spread wide enough for the lists not to overflow
        pts = kr.worst_rounding(rng.uniform(8.0, 64.0, size=(n_p, d)) if d > 1 else rng.uniform(-64.0, 64.0, size=(n_p, d)), 0.47)
        qs = kr.worst_rounding(rng.uniform(8.0, 64.0, size=(n_q, d)) if d > 1 else rng.uniform(-64.0, 64.0, size=(n_q, d)), 0.47)
    else:
        pts, qs = rng.standard_normal((n_p, d)) + 0.5, rng.standard_normal((n_q, d)) + 0.5
    d2 = kr.exact_d2(qs, pts)
    with small_sets_filtered(sa, ratio):
        for inc in (True, False):  # a query count that differs from the point count
            got = sa.find_nn(qs, k, pts, inc)
            st = sa.debug_knn_last_stats()
            assert np.array_equal(got.astype(np.int64), kr.rank(d2, k, drop_self=not inc)), (inc, st)
            assert st["filtered"] and [r["stride"] for r in st["rounds"]] == kr.search_strides(n_p, ratio, params["cap"])[1]
    # one pass over every 4th point; three queries have no threshold yet (fewer than k neighbours so far: tau = +inf)
    tau = kr.kth_d2(d2[:, ::4], k)
    open_q = [0, 5, n_q - 1]
    tau[open_q] = np.inf
    cnt, cand = sa.debug_knn_filter(qs, pts, tau, 4)
    check_pass(params, qs, pts, d2, tau, 4, cnt, cand, (n_q, n_p, d, k))
    n_sub = (n_p + 3) // 4
    assert np.all(cnt[open_q] == n_sub)  # every point of the subset and no sentinel row
    if n_sub <= params["cap"]:
        for q in open_q:
            assert sorted(cand[q, :n_sub].tolist()) == list(range(0, n_p, 4))


def test_fewer_points_than_k_pads(sa, params):
    """a pass over a subset smaller than k: tau = +inf for everybody, the lists are the subset; and find_nn pads"""
    v = kr.points("worst_2d")[:1100]
    cnt, cand = sa.debug_knn_filter(v[:256], v, np.full(256, np.inf), 64)  # 18 points
    assert np.all(cnt == 18) and np.all(np.sort(cand[:, :18], axis=1) == np.arange(0, 1100, 64)[None, :]) and np.all(cand[:, 18:] == kr.UMAX)
    with small_sets_filtered(sa):
        got = sa.find_nn(v[:256], 20, v[:12], True)  # 12 points are no case for the filter: the padding is the exhaustive kernel's
        assert not sa.debug_knn_last_stats()["filtered"]
    assert np.array_equal(got.astype(np.int64), kr.rank(kr.exact_d2(v[:256], v[:12]), 20))
    assert np.all(got[:, 12:] == kr.UMAX)


def test_routing(sa, params):
    rng = np.random.default_rng(42)
    v = rng.standard_normal((1100, 59)) + 1.0
    v3 = np.ascontiguousarray(v[:, :3])

    def run(fn):
        with small_sets_filtered(sa):
            got = fn()
            filtered = sa.debug_knn_last_stats()["filtered"]
        return got, filtered, exhaustive(sa, fn)

    got, filtered, want = run(lambda: sa.knn(v3, 5))
    assert filtered and np.array_equal(got, want)  # the control: this shape goes through the filter
    assert np.array_equal(got.astype(np.int64), kr.rank(kr.exact_d2(v3, v3), 5, drop_self=True))
    for label, fn in (("d = 59", lambda: sa.knn(v, 5)),
                      ("k = 65", lambda: sa.knn(v3, 65)),
                      ("n_q = 255", lambda: sa.find_nn(v3[:255], 5, v3, True)),
                      ("above the window", lambda: sa.knn(v3 * (2.0 * params["coord_max"]), 5)),
                      ("below the window", lambda: sa.knn(v3 * (params["coord_min"] / 16.0), 5)),
                      ("all zero", lambda: sa.knn(np.zeros((1100, 3)), 5))):
        got, filtered, want = run(fn)
        assert not filtered, label
        assert np.array_equal(got, want), label
    want3 = kr.rank(kr.exact_d2(v3, v3), 65, drop_self=True)
    assert np.array_equal(sa.knn(v3, 65).astype(np.int64), want3)
    for label, bad in (("NaN", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
        w = v3.copy()
        w[700, 1] = bad
        got, filtered, want = run(lambda: sa.knn(w, 5))  # the assertion is only: it returns, and as the exhaustive kernel does
        assert not filtered, label
        assert np.array_equal(got, want), label
        with pytest.raises(sa.ScanrsError):
            sa.debug_knn_filter(w[:256], w, np.ones(256), 1)
    with pytest.raises(sa.ScanrsError):
        sa.debug_knn_filter(v[:256], v, np.ones(256), 1)  # d = 59
    with pytest.raises(sa.ScanrsError):
        sa.debug_knn_filter(v3[:256] * 2.0 * params["coord_max"], v3, np.ones(256), 1)


def test_scaling_by_powers_of_two_changes_nothing(sa, params):
    """x -> 2^s x is exact in f64, so the neighbours are the same at every scale: inside the window through the filter, one step
    outside each end through the exhaustive kernel"""
    base = np.minimum(kr.points("worst_2d_up40") * 2.0 ** -40, 4.0)
    base[0, 0] = 4.0  # max |coordinate| = 2^2 exactly, so that the ends of the window can be hit exactly
    want = kr.rank(kr.exact_d2(base, base), 15, drop_self=True)
    hi, lo = int(np.log2(params["coord_max"])) - 2, int(np.log2(params["coord_min"])) - 2
    assert 4.0 * 2.0 ** hi == params["coord_max"] and 4.0 * 2.0 ** lo == params["coord_min"]
    with small_sets_filtered(sa):
        for s, inside in ((0, True), (-40, True), (40, True), (hi, True), (lo, True), (hi + 1, False), (lo - 1, False)):
            got = sa.knn(base * 2.0 ** s, 15)
            st = sa.debug_knn_last_stats()
            assert st["filtered"] == inside, (s, st)
            assert np.array_equal(got.astype(np.int64), want), (s, int(np.any(got != want, axis=1).sum()), st)
            if inside:  # the filter stays a filter at every scale inside the window
                assert all(r["overflowed"] == 0 for r in st["rounds"]), (s, st)


# ---- lists that overflow in every round, not only the last --------------------------------------------------------------------------
# 8192 points, d = 5, k = 10, "knn_filter_min_points" 1024, "knn_ratio" 2: round 0 ranks 1024 rows at stride 8, the filter rounds run at
# strides 4, 2, 1. Every row r with r % 4 != 3 is one and the same point (6144 rows), so the subset of stride 4 (rows r % 4 == 0) is
# 2048 coincident rows: every query of the cluster holds more than `cap` candidates at distance 0 and overflows at strides 4, 2 AND 1
# (and so do the 2048 other queries, whose k-th neighbour so far is the cluster itself). The sharded form below has both kinds of query.
OVER_N, OVER_D, OVER_K = 8192, 5, 10


@contextlib.contextmanager
def overflow_options(sa):
    sa.set_global_option("knn_filter_min_points", 1024)
    sa.set_global_option("knn_ratio", 2)
    try:
        yield
    finally:
        sa.set_global_option("knn_filter_min_points", 32768)
        sa.set_global_option("knn_ratio", 4)


@pytest.fixture(scope="module")
def overflow_case():
    """the points and their float64 reference with one more column: rank(d2, k + 1), the query's own row still in it"""
    rng = np.random.default_rng(8192)
    v = rng.standard_normal((OVER_N, OVER_D))
    v[np.arange(OVER_N) % 4 != 3] = rng.standard_normal(OVER_D)
    ranked = np.concatenate([kr.rank(kr.exact_d2(v[a:a + 1024], v), OVER_K + 1) for a in range(0, OVER_N, 1024)], axis=0)
    ranked.setflags(write=False)
    return v, ranked


def reference(ranked, drop_self):
    """the first k of a row of rank(d2, k + 1), its own index taken out first: what rank(d2, k, drop_self) returns"""
    if not drop_self:
        return ranked[:, :OVER_K]
    keep = ranked != np.arange(ranked.shape[0])[:, None]
    keep[keep.all(axis=1), OVER_K] = False  # the row itself is not among the k + 1 nearest: the last column goes
    return ranked[keep].reshape(ranked.shape[0], OVER_K)


def overflows_in_every_round(st):
    return st["filtered"] and [r["stride"] for r in st["rounds"]] == [4, 2, 1] and all(r["overflowed"] > 0 for r in st["rounds"])


def test_overflow_in_every_round_knn(sa, overflow_case):
    v, ranked = overflow_case
    with overflow_options(sa):
        got = sa.knn(v, OVER_K)
        st = sa.debug_knn_last_stats()
        want = exhaustive(sa, lambda: sa.knn(v, OVER_K))
    print(st)
    assert np.array_equal(got, want)
    assert np.array_equal(got.astype(np.int64), reference(ranked, True))
    assert overflows_in_every_round(st), st


@pytest.mark.parametrize("include_self", (True, False))
def test_overflow_in_every_round_find_nn(sa, overflow_case, include_self):
    v, ranked = overflow_case
    with overflow_options(sa):
        got = sa.find_nn(v, OVER_K, v, include_self)
        st = sa.debug_knn_last_stats()
        want = exhaustive(sa, lambda: sa.find_nn(v, OVER_K, v, include_self))
    assert np.array_equal(got, want)
    assert np.array_equal(got.astype(np.int64), reference(ranked, not include_self))
    assert overflows_in_every_round(st), st


def test_overflow_in_every_round_sharded_and_seeded(sa, overflow_case):
    """two ranks, blocks of 4096 rows: the second block is searched with the seed of the first, and its lists overflow as well"""
    import test_gpu_knn_sharded as ks

    v, ranked = overflow_case
    run = ks.make(sa, "hook", OVER_N, [0, OVER_N // 2, OVER_N])
    plain = sa.AdaptiveMat.from_csmat(1, OVER_N, sa.CSC, *ks.cell_matrix(OVER_N))
    try:
        with overflow_options(sa), ks.options(sa, block_rows=4096, min_points=1024):
            got, dist = run.knn(v, OVER_K)
            st = sa.debug_knn_last_stats()
            blocks = run.counters("knn_blocks")
            want, want_dist = plain.knn_sharded(v, OVER_K, return_sq_dist=True)
            assert overflows_in_every_round(sa.debug_knn_last_stats())
    finally:
        run.close()
    print(st)
    assert np.array_equal(got, want) and np.array_equal(got.astype(np.int64), reference(ranked, True))
    ks.same_bits(dist, want_dist)
    # a block is 4096 rows and a seeded search ranks 256 of them exactly: strides 8, 4, 2, 1, and from 2048 rows on a list overflows
    assert blocks == [2, 2] and st["filtered"] and [r["stride"] for r in st["rounds"]] == [8, 4, 2, 1]
    assert [r["overflowed"] > 0 for r in st["rounds"]] == [False, False, True, True], st
    # some of the rank's 4096 queries overflow and some take the plain filter path in the same rounds: the list of queries handed to
    # the exhaustive kernel is a proper subset, not 0 .. n_q - 1 (a query far from the cluster holds k nearer rows after the first block)
    assert all(0 < r["overflowed"] < OVER_N // 2 for r in st["rounds"][2:]), st


def test_overflow_in_every_round_cosine(sa, overflow_case):
    """the twin under cosine distance: coincident rows standardise to one z, so the same lists overflow in the same rounds"""
    v, _ = overflow_case
    with overflow_options(sa):
        idx, dist = sa.nearest_neighbors(v, OVER_K, "cosine")
        st = sa.debug_knn_last_stats()
    want_idx, want_dist = sa.host_nearest_neighbors(v, OVER_K, "cosine")
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(np.ascontiguousarray(dist).view(np.uint64), np.ascontiguousarray(want_dist).view(np.uint64))
    assert overflows_in_every_round(st), st
