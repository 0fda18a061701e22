"""select_rows / select_cols / partition_on_thresholds over sharded and multi-GPU matrices against the restatement
tests/select_ref.py and against the same calls on one unsharded handle. Every sum that crosses the shards is a u64 integer, so
every comparison is exact equality, for any number of shards. Fixtures: tests/select_sharded_case.py (checked on the CPU by
tests/test_select_sharded_cpu.py). All shards share device 0."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import select_ref as sref  # noqa: E402
import select_sharded_case as sc  # noqa: E402

SHARDS = (1, 2, 3, 5)
FORMS = ("csc", "csr_t")  # genes x cells stored CSC / its transpose, cells x genes, stored CSR: the cells are the sharded dimension in both
CASES = ["cascade"] + list(sc.SEEDED_CASES)


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


def _oriented(m, form):
    """(the scipy matrix the handles of this form hold, its storage name)."""
    return (sref.canonical(m, "csc"), "csc") if form == "csc" else (sref.canonical(m.T, "csr"), "csr")


def _flag(sa, storage):
    return sa.CSR if storage == "csr" else sa.CSC


def _multi(sa, mat, storage, n_shards):
    ip, ix, vv = sref.triplet(mat, storage)
    return sa.MultiMat(mat.shape[0], mat.shape[1], _flag(sa, storage), ip, ix, vv, n_shards, devices=[0] * n_shards)


def _single(sa, mat, storage):
    ip, ix, vv = sref.triplet(mat, storage)
    return sa.AdaptiveMat.from_csmat(mat.shape[0], mat.shape[1], _flag(sa, storage), ip, ix, vv)


def _same_triplet(got, expected, storage):
    want = sref.triplet(expected, storage)
    assert all(g.dtype == w.dtype for g, w in zip(got, want))
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def _assert_multi_is(sa, mm, expected, storage, n_shards):
    """A MultiMat result against the scipy matrix it must hold: shape, nonzeros, the concatenated triplet, and shard ranges that tile
    the outer dimension without gaps."""
    assert mm.shape() == list(expected.shape) and (mm.rows, mm.cols) == expected.shape
    assert mm.storage == _flag(sa, storage) and mm.n_shards == n_shards
    assert mm.nnz() == expected.nnz
    _same_triplet(mm.to_csmat(), expected, storage)
    assert mm.to_scipy().shape == expected.shape and mm.to_scipy().format == storage
    ranges = mm.shard_ranges()
    n_outer = expected.shape[0] if storage == "csr" else expected.shape[1]
    assert len(ranges) == n_shards and ranges[0][1] == 0 and ranges[-1][2] == n_outer
    assert all(lo <= hi for _, lo, hi in ranges) and all(ranges[i][2] == ranges[i + 1][1] for i in range(n_shards - 1))


def _case_input(case):
    """(genes x cells matrix, row threshold, column threshold) of a case name."""
    if case == "cascade":
        m, thr, _, _ = sc.cascade()
        return m, thr, thr
    return sc.seeded_matrix(), case[0], case[1]


@pytest.fixture(scope="module")
def expected(sa):
    """(case, form) -> what the restatement and ONE unsharded handle give, computed once: the matrix of the form, its storage, the two
    thresholds in its orientation, the restatement's 5-tuple, and the single handle's to_csmat of both results."""
    made = {}

    def get(case, form):
        if (case, form) not in made:
            m, rt, ct = _case_input(case)
            mat, storage = _oriented(m, form)
            if form == "csr_t":
                rt, ct = ct, rt
            want = sref.partition_on_thresholds(mat, rt, ct)
            h = _single(sa, mat, storage)
            f, r, sel_r, sel_c = h.partition_on_thresholds(rt, ct)
            assert np.array_equal(sel_r, want[2]) and np.array_equal(sel_c, want[3]) and h.counter("partition_rounds") == want[4]
            assert h.counter("partition_allreduces") == 0
            made[(case, form)] = (mat, storage, rt, ct, want, f.to_csmat(), r.to_csmat())
        return made[(case, form)]

    return get


# ---- partition ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=str)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_shards", SHARDS)
def test_partition_equals_the_restatement_and_the_single_handle(sa, expected, n_shards, form, case):
    mat, storage, rt, ct, (ef, er, esr, esc, rounds), single_f, single_r = expected(case, form)
    if form == "csc" and case != "cascade":
        assert (rounds, mat.shape[0] - len(esr), mat.shape[1] - len(esc)) == sc.SEEDED_CASES[case]
    mm = _multi(sa, mat, storage, n_shards)
    f, r, sel_r, sel_c = mm.partition_on_thresholds(rt, ct)
    counted = [(mm.counter("partition_rounds", i), mm.counter("partition_allreduces", i)) for i in range(n_shards)]
    mm.close()  # the source goes first: the results have their own group and communicators
    print(f"partition {case} {form} x{n_shards}: rounds {counted[0][0]} (restatement {rounds}), exchange steps {counted[0][1]}")
    assert np.array_equal(sel_r, esr) and np.array_equal(sel_c, esc)
    # the inner dimension is the one that is not sharded: the rows of a CSC matrix
    inner_thr, outer_thr = (rt, ct) if storage == "csc" else (ct, rt)
    bound = sc.allreduce_bound(rounds, inner_thr is not None, outer_thr is not None)
    assert all(c == (rounds, counted[0][1]) for c in counted) and 1 <= counted[0][1] <= bound
    _assert_multi_is(sa, f, ef, storage, n_shards)
    _assert_multi_is(sa, r, er, storage, n_shards)
    assert all(np.array_equal(g, w) for g, w in zip(f.to_csmat(), single_f))
    assert all(np.array_equal(g, w) for g, w in zip(r.to_csmat(), single_r))
    f.close()
    r.close()


@pytest.mark.parametrize("form", FORMS)
def test_partition_builds_only_what_is_asked_for(sa, expected, form):
    mat, storage, rt, ct, (ef, er, esr, esc, rounds), _, _ = expected((34, 13), form)
    mm = _multi(sa, mat, storage, 3)
    f, r, sel_r, sel_c = mm.partition_on_thresholds(rt, ct, residual=False)
    assert r is None and np.array_equal(sel_r, esr) and np.array_equal(sel_c, esc)
    _assert_multi_is(sa, f, ef, storage, 3)
    f2, r2, sel_r, sel_c = mm.partition_on_thresholds(rt, ct, filtered=False)
    assert f2 is None and np.array_equal(sel_r, esr) and np.array_equal(sel_c, esc)
    _assert_multi_is(sa, r2, er, storage, 3)
    f3, r3, sel_r, sel_c = mm.partition_on_thresholds(rt, ct, filtered=False, residual=False)
    assert f3 is None and r3 is None and np.array_equal(sel_r, esr) and np.array_equal(sel_c, esc)
    assert mm.counter("partition_rounds", 2) == rounds
    f4, _, _, _ = mm.partition_on_threshold(3.0)
    _assert_multi_is(sa, f4, sref.partition_on_threshold(mat, 3.0)[0], storage, 3)
    mm.close()


# ---- select -------------------------------------------------------------------------------------------------------------------------
def _sharded_axis_lists(ranges):
    """Ascending lists with repeats over the sharded axis: one whose run skips a whole shard (from 3 shards on), one that takes
    nothing from the last shard (from 2 shards on), one that is empty."""
    n = len(ranges)

    def some_of(shards):
        pos = np.concatenate([np.arange(ranges[i][1], ranges[i][2]) for i in shards] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        pos = pos[::3]
        return np.sort(np.concatenate([pos, pos[::4], pos[-1:]]))  # repeats, next to each other once sorted

    skipping = some_of([i for i in range(n) if not (n >= 3 and i == 1)])
    short = some_of(range(n - 1) if n >= 2 else range(n))
    if n >= 3:
        assert not np.any((skipping >= ranges[1][1]) & (skipping < ranges[1][2])) and np.any(skipping >= ranges[2][1])
    if n >= 2:
        assert short.max() < ranges[-1][1]
    assert np.any(np.diff(skipping) == 0) and np.all(np.diff(skipping) >= 0)
    return [skipping, short, np.zeros(0, dtype=np.int64)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_shards", SHARDS)
def test_select_along_both_axes(sa, n_shards, form):
    mat, storage = _oriented(sc.seeded_matrix(), form)
    mm = _multi(sa, mat, storage, n_shards)
    ranges = mm.shard_ranges()
    rows_sharded = storage == "csr"
    along = (mm.select_rows, sref.select_rows) if rows_sharded else (mm.select_cols, sref.select_cols)
    across = (mm.select_cols, sref.select_cols) if rows_sharded else (mm.select_rows, sref.select_rows)
    for idx in _sharded_axis_lists(ranges):
        got = along[0](idx)
        _assert_multi_is(sa, got, sref.canonical(along[1](mat, idx), storage), storage, n_shards)
        # where the result's shards lie: the entries below each source range
        assert [lo for _, lo, _ in got.shard_ranges()] == [int(np.searchsorted(idx, lo)) for _, lo, _ in ranges]
        got.close()
    n_inner = mat.shape[1] if rows_sharded else mat.shape[0]
    rng = np.random.default_rng(5)
    shuffled = rng.integers(0, n_inner, 2 * n_inner)  # any order, repeats: the vectors are sorted again after the expansion
    assert np.any(np.diff(shuffled) < 0) and len(set(shuffled.tolist())) < len(shuffled)
    for idx in (shuffled, np.zeros(0, dtype=np.int64)):
        got = across[0](idx)
        _assert_multi_is(sa, got, sref.canonical(across[1](mat, idx), storage), storage, n_shards)
        assert got.shard_ranges() == ranges  # a list along the replicated dimension leaves the ranges alone
        got.close()
    mm.close()


@pytest.mark.parametrize("form", FORMS)
def test_select_refusals(sa, form):
    mat, storage = _oriented(sc.seeded_matrix(), form)
    mm = _multi(sa, mat, storage, 3)
    single = _single(sa, mat, storage)
    rows_sharded = storage == "csr"
    along, plain = (mm.select_rows, single.select_rows) if rows_sharded else (mm.select_cols, single.select_cols)
    n_outer = mat.shape[0] if rows_sharded else mat.shape[1]
    with pytest.raises(sa.ScanrsError) as e:
        along([0, 5, 5, 40, 39, 41, 2])
    assert e.value.code == 6 and "entry 4" in str(e.value) and "between ranks" in str(e.value), str(e.value)
    # an index outside the matrix: SCANRS_ERR_INVALID, the code and the words the plain function reports it with
    with pytest.raises(sa.ScanrsError) as e_plain:
        plain([0, n_outer])
    with pytest.raises(sa.ScanrsError) as e:
        along([0, n_outer])
    assert e.value.code == e_plain.value.code and "out of range" in str(e.value) and "out of range" in str(e_plain.value)
    hdr = open(os.path.join(os.path.dirname(TESTS), "include", "scanrs_amd.h")).read()
    assert f"SCANRS_ERR_INVALID = {e.value.code}," in hdr
    # the handle is usable after a refusal, and nothing was left behind by it
    got = along([1, 1, n_outer - 1])
    assert got.shape()[0 if rows_sharded else 1] == 3
    got.close()
    mm.close()


# ---- chains and what runs downstream ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_shards", (2, 5))
def test_results_chain_like_one_handle(sa, n_shards, form):
    mat, storage = _oriented(sc.seeded_matrix(), form)
    t1, t2 = ((3, 3), (34, 13)) if form == "csc" else ((3, 3), (13, 34))
    mm, h = _multi(sa, mat, storage, n_shards), _single(sa, mat, storage)
    f1, _, _, _ = mm.partition_on_thresholds(*t1)
    g1, _, _, _ = h.partition_on_thresholds(*t1)
    mm.close()
    f2, r2, sel_r, sel_c = f1.partition_on_thresholds(*t2)  # partition of a partition result
    g2, s2, want_r, want_c = g1.partition_on_thresholds(*t2)
    assert np.array_equal(sel_r, want_r) and np.array_equal(sel_c, want_c)
    assert f1.counter("partition_rounds", n_shards - 1) == g1.counter("partition_rounds")
    _assert_multi_is(sa, f2, g2.to_scipy(), storage, n_shards)
    _assert_multi_is(sa, r2, s2.to_scipy(), storage, n_shards)
    cols = np.arange(0, f1.shape()[1], 2)  # ascending: valid whichever axis is the sharded one
    _assert_multi_is(sa, f1.select_cols(cols), g1.select_cols(cols).to_scipy(), storage, n_shards)  # select_cols of a partition result
    want = sref.partition_on_thresholds(sref.partition_on_thresholds(mat, *t1)[0], *t2)
    _same_triplet(f2.to_csmat(), want[0], storage)
    _same_triplet(r2.to_csmat(), want[1], storage)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_shards", SHARDS)
def test_group_sums_over_the_filtered_matrix(sa, expected, n_shards, form):
    mat, storage, rt, ct, (ef, _, esr, esc, _), _, _ = expected((34, 13), form)
    mm = _multi(sa, mat, storage, n_shards)
    f, _, sel_r, sel_c = mm.partition_on_thresholds(rt, ct, residual=False)
    mm.close()
    kept_cells = sel_c if form == "csc" else sel_r
    labels = sc.seeded_labels()[kept_cells]
    genes_by_cells = np.asarray((ef if form == "csc" else ef.T).todense()).astype(np.uint64)  # the host-filtered matrix
    want = np.stack([genes_by_cells[:, labels == g].sum(axis=1, dtype=np.uint64) for g in range(sc.N_GROUPS)], axis=1)
    sums, cnt = sa.group_sums(f, labels, sc.N_GROUPS, transposed=form == "csr_t")
    assert sums.dtype == np.uint64 and np.array_equal(sums, want)
    assert np.array_equal(cnt, np.bincount(labels[labels >= 0], minlength=sc.N_GROUPS).astype(np.uint64))
    f.close()


@pytest.mark.parametrize("n_shards", SHARDS)
def test_normalize_and_pca_on_the_filtered_matrix(sa, expected, n_shards):
    """normalize + BkSvd on the filtered MultiMat against the same two calls on one handle made from the restatement's filtered
    matrix. Bound: relative 1e-8 on the singular values, what tests/test_gpu_parity.py holds a 2-shard MultiMat to against one
    handle; only the order of the f64 all-reduces differs."""
    mat, storage, rt, ct, (ef, _, _, _, _), _, _ = expected((3, 3), "csc")
    k = 6
    one = _single(sa, ef, storage)
    _, s1, _ = sa.BkSvd().run_pca(sa.normalize(one, sa.Normalization.CellRanger), k)
    mm = _multi(sa, mat, storage, n_shards)
    f, _, _, _ = mm.partition_on_thresholds(rt, ct, residual=False)
    mm.close()
    f.normalize(sa.Normalization.CellRanger)
    u, s, v = f.run_pca_bk(k)
    assert u.shape == (ef.shape[0], k) and v.shape == (ef.shape[1], k)
    rel = np.max(np.abs(s - s1) / s1)
    print(f"pca of the filtered matrix x{n_shards}: sigma rel diff {rel:.2e}")
    assert rel < 1e-8
    f.close()


# ---- the handle's own collective entry points: host hook, views, refusals -------------------------------------------------------------
@pytest.mark.parametrize("kind", ("csc", "csr", "t"))
def test_host_hook_world_of_one_equals_the_plain_calls(sa, kind):
    m = sc.seeded_matrix()
    dtypes = []

    def hook(ptr, count, dtype):
        dtypes.append(dtype)
        return 0  # a world of one rank: the sum is what is there

    def handle(sharded):
        if kind == "t":  # the transposed view of the cells x genes CSR matrix reads as genes x cells, flag CSC; its columns are sharded
            base = sref.canonical(m.T, "csr")
            b = _single(sa, base, "csr")
            if sharded:
                b.set_shard(0, 1, 0, base.shape[0], hook)
            return b.t()
        h = _single(sa, sref.canonical(m, kind), kind)
        if sharded:
            h.set_shard(0, 1, 0, m.shape[0] if kind == "csr" else m.shape[1], hook)
        return h

    s, p = handle(True), handle(False)
    want_info = {"rank": 0, "world": 1, "outer_begin": 0}
    assert {k: s.shard_info()[k] for k in want_info} == want_info
    for rt, ct in ((34, 13), (None, 8), (20, None)):
        f, r, sel_r, sel_c = s.partition_on_thresholds_sharded(rt, ct)
        pf, pr, psel_r, psel_c = p.partition_on_thresholds(rt, ct)
        assert np.array_equal(sel_r, psel_r) and np.array_equal(sel_c, psel_c)
        assert s.counter("partition_rounds") == p.counter("partition_rounds")
        outer_thr, inner_thr = (rt, ct) if kind == "csr" else (ct, rt)
        assert 1 <= s.counter("partition_allreduces") <= sc.allreduce_bound(p.counter("partition_rounds"), inner_thr is not None, outer_thr is not None)
        for got, want in ((f, pf), (r, pr)):
            assert got.shape() == want.shape() and got.storage() == want.storage()
            assert all(np.array_equal(a, b) for a, b in zip(got.to_csmat(), want.to_csmat()))
            info = got.shard_info()  # the result reports the same world, over its own range
            n_outer = got.shape()[0] if got.storage() == sa.CSR else got.shape()[1]
            assert info == {"rank": 0, "world": 1, "outer_begin": 0, "outer_global": n_outer}
        # the result is bound to the hook: a collective call on it goes through the hook again
        before = len(dtypes)
        f.partition_on_thresholds_sharded(rt, ct, filtered=False, residual=False)
        assert len(dtypes) > before
    rows = np.array([0, 0, 7, 30, 60])
    cols = np.array([2, 2, 50, 150, 155])
    for got, want in ((s.select_rows_sharded(rows), p.select_rows(rows)), (s.select_cols_sharded(cols), p.select_cols(cols)),
                      (s.select_rows_sharded([]), p.select_rows([]))):
        assert got.shape() == want.shape() and all(np.array_equal(a, b) for a, b in zip(got.to_csmat(), want.to_csmat()))
        assert got.shard_info()["world"] == 1
    assert dtypes and set(dtypes) == {1}  # u64 sums only
    # an unsharded handle: the collective forms are the plain calls
    f, r, sel_r, sel_c = p.partition_on_thresholds_sharded(34, 13)
    pf, pr, psel_r, psel_c = p.partition_on_thresholds(34, 13)
    assert np.array_equal(sel_r, psel_r) and np.array_equal(sel_c, psel_c) and p.counter("partition_allreduces") == 0
    assert all(np.array_equal(a, b) for a, b in zip(f.to_csmat(), pf.to_csmat())) and all(np.array_equal(a, b) for a, b in zip(r.to_csmat(), pr.to_csmat()))
    assert all(np.array_equal(a, b) for a, b in zip(p.select_cols_sharded(cols[::-1]).to_csmat(), p.select_cols(cols[::-1]).to_csmat()))


def test_what_stays_refused(sa):
    m = sc.seeded_matrix()
    idx = np.arange(10)

    def refused(fn, code, *words):
        with pytest.raises(sa.ScanrsError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        assert all(w in str(e.value) for w in words), str(e.value)

    # the plain entry points still refuse a sharded handle (the assertion of tests/test_gpu_select.py, kept here beside the feature)
    s = _single(sa, m, "csr")
    s.set_shard(0, 2, 0, 2 * m.shape[0], allreduce=lambda ptr, count, dtype: 0)
    for fn in (lambda: s.select_rows(idx), lambda: s.select_cols(idx), lambda: s.partition_on_threshold(3.0)):
        refused(fn, 6, "sharded")
    # a composed map or an offset on the shards: today's messages, on the handle's and on the multi entry points
    h = _single(sa, m, "csc")
    h.set_shard(0, 1, 0, m.shape[1], allreduce=lambda ptr, count, dtype: 0)
    h.compose_scale_axis(0, np.ones(m.shape[0]))
    for fn in (lambda: h.select_rows_sharded(idx), lambda: h.select_cols_sharded(idx), lambda: h.partition_on_thresholds_sharded(3.0, 3.0)):
        refused(fn, 6, "not the identity", "scanrs_mat_reset_map")
    h.reset_map()
    assert h.select_rows_sharded(idx).shape() == [10, m.shape[1]]
    mat, storage = _oriented(m, "csc")
    mm = _multi(sa, mat, storage, 2)
    mm.normalize(sa.Normalization.CellRanger)
    for fn in (lambda: mm.select_rows(idx), lambda: mm.select_cols(idx), lambda: mm.partition_on_threshold(3.0)):
        refused(fn, 6, "scanrs_mat_reset_map")
    mm.close()
    o = _single(sa, m, "csc")
    o.set_shard(0, 1, 0, m.shape[1], allreduce=lambda ptr, count, dtype: 0)
    o.center(0)
    refused(lambda: o.partition_on_thresholds_sharded(3.0, 3.0), 6, "offset", "scanrs_mat_reset_map")
