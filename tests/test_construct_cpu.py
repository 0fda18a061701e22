"""The construction reference and its cases, on the CPU (tests/construct_ref.py; the GPU side is tests/test_gpu_construct.py and
tests/test_gpu_adaptive_decode.py): the reference against itself and against dense numpy, the properties of the cases the GPU tests
rely on, and the sort-route decision of the transposed copy (scanrs_host_transpose_plan, scan-rs_amd/csrc/transpose_plan.hpp)."""
import os
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import construct_ref as cr  # noqa: E402


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def dense_of(n_outer, n_inner, indptr, indices, values):
    d = np.zeros((n_outer, n_inner), dtype=np.uint64)
    d[cr.outer_ids(n_outer, indptr), indices.astype(np.int64)] = values
    return d


def small(seed, n_outer=37, n_inner=23):
    rng = np.random.default_rng(seed)
    return cr.Case(n_outer, n_inner, *cr.build(n_inner, rng.integers(0, n_inner + 1, size=n_outer), rng, 1, 2**32))


def bits_for(x):
    return max(1, int(x).bit_length())


def plan_of(sa, case, max_value=None):
    return sa.host_transpose_plan(case.n_outer, case.n_inner, case.max_value if max_value is None else max_value)


# ---- the reference against itself -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_transpose_twice_is_the_identity_and_agrees_with_dense(seed):
    c = small(seed)
    t = cr.transpose(*c.args())
    assert same(cr.transpose(c.n_inner, c.n_outer, *t), c.triplet)
    assert np.array_equal(dense_of(c.n_inner, c.n_outer, *t), dense_of(*c.args()).T)
    tip = t[0].astype(np.int64)
    for i in range(c.n_inner):  # outer ids ascend strictly inside every inner vector
        assert np.all(np.diff(t[1][tip[i]:tip[i + 1]].astype(np.int64)) > 0)


def test_transpose_of_the_shared_cases_is_an_involution():
    for name in cr.TRANSPOSE_CASES:
        c = cr.transpose_case(name)
        t = cr.transpose(*c.args())
        assert int(t[0][-1]) == c.nnz and same(cr.transpose(c.n_inner, c.n_outer, *t), c.triplet), name


@pytest.mark.parametrize("seed", [1, 2])
def test_products_sums_and_selections_agree_with_dense(seed):
    c = small(seed)
    d = dense_of(*c.args())
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 2**32, size=(c.n_inner, 3), dtype=np.uint64).astype(np.uint32)
    y = rng.integers(0, 2**32, size=(c.n_outer, 2), dtype=np.uint64).astype(np.uint32)
    wrap = lambda m: (m & np.uint64(cr.U32_MAX)).astype(np.uint32)  # noqa: E731
    assert np.array_equal(cr.product(c.n_outer, *c.triplet, x), wrap(d @ x.astype(np.uint64)))
    assert np.array_equal(cr.product_t(*c.args(), y), wrap(d.T @ y.astype(np.uint64)))
    so, si = cr.sums(*c.args())
    assert np.array_equal(so, wrap(d.sum(axis=1))) and np.array_equal(si, wrap(d.sum(axis=0)))
    idx_o, idx_i = rng.integers(0, c.n_outer, size=50), rng.integers(0, c.n_inner, size=40)
    assert np.array_equal(dense_of(50, c.n_inner, *cr.select_outer(c.n_outer, *c.triplet, idx_o)), d[idx_o])
    picked = cr.select_inner(*c.args(), idx_i)
    assert np.array_equal(dense_of(c.n_outer, 40, *picked), d[:, idx_i]) and cr.validate(c.n_outer, 40, *picked)[0] == 0


def test_compact_and_sort_within_restate_the_repairs():
    c = cr.zeros_case("vector")
    ip, ix, vv = cr.compact(c.n_outer, *c.triplet)
    assert np.all(vv != 0) and int(ip[-1]) == vv.shape[0] == int(np.count_nonzero(c.values)) and int(ip[101]) == int(ip[100])
    assert np.array_equal(dense_of(c.n_outer, c.n_inner, ip, ix, vv), dense_of(*c.args()))
    assert same(cr.compact(c.n_outer, ip, ix, vv), (ip, ix, vv))
    u = cr.unsorted_case()
    assert cr.validate(*u.args())[0] > 0
    s = cr.sort_within(u.n_outer, *u.triplet)
    assert cr.validate(u.n_outer, u.n_inner, *s) == (0, 0, u.max_value)
    assert np.array_equal(dense_of(u.n_outer, u.n_inner, *s), dense_of(*u.args()))
    uz = cr.unsorted_case(zeros=True)
    a = cr.compact(uz.n_outer, *cr.sort_within(uz.n_outer, *uz.triplet))
    b = cr.sort_within(uz.n_outer, *cr.compact(uz.n_outer, *uz.triplet))
    assert same(a, b) and a[2].shape[0] == uz.nnz - 500


def test_items_at_the_edges():
    ip = np.concatenate([[0], np.cumsum([0, 1, 8191, 8192, 8193, 16384, 16385, 24577])])
    assert list(cr.items(ip)) == [1, 1, 1, 1, 2, 2, 3, 4]


# ---- validate: every valid case 0, every invalid case >= 1 --------------------------------------------------------------------------
def valid_cases():
    for name in cr.TRANSPOSE_CASES:
        yield name, cr.transpose_case(name)
    for name in cr.MAX_CASES:
        yield name, cr.max_case(name)
    for name in cr.ZEROS_CASES:
        yield name, cr.zeros_case(name)
    yield "valid_base", cr.valid_base()
    yield "all_starts_descend", cr.all_starts_descend()
    yield "items", cr.items_case()
    yield "big", cr.big_case(cr.MI355X_CUS)


def test_every_valid_case_validates_to_zero():
    for name, c in valid_cases():
        bad, zeros, largest = cr.validate(*c.args())
        assert bad == 0 and largest == c.max_value, name
        assert (zeros > 0) == (name in cr.ZEROS_CASES), name


def test_every_invalid_case_is_counted():
    base = cr.valid_base()
    assert 2000 < base.nnz < 5000 and base.nnz % 4 == 2
    for violation in cr.VIOLATIONS:
        seen = set()
        for where in cr.PLACES:
            p = cr.place(base, violation, where)
            seen.add(p)
            if where.startswith("mod_"):
                assert p % 4 == int(where[-1])
            bad = cr.validate(*cr.violate(base, violation, p).args())[0]
            assert bad == (2 if violation == "indptr_beyond" else 1), (violation, where, p)
        assert len(seen) == len(cr.PLACES), violation
        if violation in ("descent", "duplicate", "beyond"):
            assert cr.place(base, violation, "last") == base.nnz - 1
    big = cr.big_case(cr.MI355X_CUS)
    for violation in cr.VIOLATIONS:
        p = cr.place(big, violation, "second_trip")
        assert cr.stream_span(cr.MI355X_CUS) <= p < big.nnz
        assert cr.validate(*cr.violate(big, violation, p).args())[0] >= 1
    d = cr.all_starts_descend()
    assert cr.validate(*cr.violate(d, "duplicate", cr.place(d, "duplicate", "mod_2")).args())[0] == 1
    u = cr.unsorted_case()
    ix = u.indices.copy()
    a = int(u.indptr[6])
    ix[a + 7] = ix[a + 12000]
    assert cr.validate(u.n_outer, u.n_inner, *cr.sort_within(u.n_outer, u.indptr, ix, u.values))[0] == 1


def test_descents_at_vector_starts_are_where_the_gpu_tests_expect_them():
    base = cr.valid_base()
    places = cr.start_descent_places(base)
    ip = base.indptr.astype(np.int64)
    for where, p in places.items():
        assert p in ip and p > 0 and base.indices[p] <= base.indices[p - 1], where
        if where.startswith("mod_"):
            assert p % 4 == int(where[-1])
    assert len(set(places.values())) == 6
    eq, at = cr.equal_across_a_start(base)
    assert len(at) == 4 and sorted(p % 4 for p in at) == [0, 1, 2, 3]
    assert all(eq.indices[p] == eq.indices[p - 1] and p in ip for p in at) and cr.validate(*eq.args())[0] == 0
    # the streaming formula counts every one of these as a descent and takes it off again: there are hundreds
    down = np.count_nonzero(base.indices[1:] <= base.indices[:-1])
    assert down > 200 and cr.validate(*base.args())[0] == 0
    d = cr.all_starts_descend()
    assert np.count_nonzero(d.indices[1:] <= d.indices[:-1]) == d.n_outer - 1


# ---- the cases have the properties the GPU tests rely on --------------------------------------------------------------------------
def test_transposed_copy_cases_take_the_intended_route(sa):
    routes = set()
    for name, want in cr.TRANSPOSE_CASES.items():
        c = cr.transpose_case(name)
        if want is None:
            assert c.nnz == 0
            continue
        route, ib, ob, cb = plan_of(sa, c)
        assert (ib + ob + cb, route) == want, name
        assert (ib, ob, cb) == (bits_for(c.n_inner - 1), bits_for(c.n_outer - 1), bits_for(c.max_value)), name
        assert 1024 < c.nnz < 20000 or name in ("edge_64_small", "edge_64_large", "one_outer")
        routes.add(route)
    assert routes == {cr.PACKED, cr.PAIR}
    assert cr.transpose_case("edge_64").max_value == cr.transpose_case("pair_65").max_value == cr.U32_MAX
    assert cr.transpose_case("edge_64_small").nnz <= 1024 and cr.transpose_case("edge_64_large").nnz > 2**20  # the sort's other algorithms
    assert cr.transpose_case("edge_64_small").max_value == cr.transpose_case("edge_64_large").max_value == cr.U32_MAX
    assert cr.transpose_case("pair_66").max_value == 2**31 and cr.transpose_case("packed_65_small_counts").max_value < 2**31
    assert cr.transpose_case("all_ones").max_value == 1
    for name in ("edge_64", "edge_64_small", "edge_64_large", "pair_65", "pair_66"):  # the corners of the index range are stored
        c = cr.transpose_case(name)
        assert c.indices[0] == 0 and c.indices[-1] == c.n_inner - 1 and c.indptr[1] > 0 and c.indptr[-2] < c.nnz
    for a, b in (("long_pair", "long_packed"), ("pair_65", "packed_65_small_counts")):  # the same matrix but for one count
        x, y = cr.transpose_case(a), cr.transpose_case(b)
        assert np.array_equal(x.indptr, y.indptr) and np.array_equal(x.indices, y.indices) and np.count_nonzero(x.values != y.values) == 1
        assert list(np.unique(cr.items(x.indptr))) == ([1, 2] if a == "long_pair" else [1])
    m = cr.transpose_case("mostly_empty_inner")
    assert np.unique(m.indices).shape[0] == 12


def test_long_vector_cases_have_the_stated_lengths():
    assert 8192 in cr.UNSORTED_LENGTHS and 8193 in cr.UNSORTED_LENGTHS and 20000 in cr.UNSORTED_LENGTHS and {0, 1} <= set(cr.UNSORTED_LENGTHS)
    assert tuple(np.diff(cr.unsorted_case().indptr.astype(np.int64))) == cr.UNSORTED_LENGTHS and cr.unsorted_case().n_inner == 70001
    c = cr.items_case()
    lens = np.diff(c.indptr.astype(np.int64))
    assert tuple(lens) == cr.ITEM_LENGTHS and {0, 1, 8191, 8192, 8193, 16384, 16385, 24577} == set(cr.ITEM_LENGTHS)
    assert list(cr.items(c.indptr)) == [1, 1, 1, 1, 2, 2, 3, 4, 1]
    so, si = cr.sums(*c.args())
    exact = np.add.reduceat(c.values.astype(np.uint64), c.indptr[:-1][lens > 0].astype(np.int64))
    assert np.all(exact[lens[lens > 0] > 1] > cr.U32_MAX)  # the u32 sums of all but the one-nonzero vector wrap


def test_the_largest_count_sits_where_stated():
    for name in cr.MAX_CASES:
        c = cr.max_case(name)
        at = c.notes["big_at"]
        assert c.values[at] == cr.U32_MAX and np.count_nonzero(c.values > 3) == 1
        if name == "first":
            assert at == 0
        else:
            assert at == c.nnz - 1 and c.nnz % 4 == int(name[-1])
    n_cu = cr.MI355X_CUS
    big = cr.big_case(n_cu)
    assert big.nnz == n_cu * 16 * 256 * 4 + 1029 == 4195333
    at = big.notes["big_at"]
    assert big.nnz - 1029 <= at < big.nnz and big.values[at] == cr.U32_MAX and np.count_nonzero(big.values > 3) == 1
    lens = np.diff(big.indptr.astype(np.int64))
    assert np.all(lens[10:20] == 0) and lens.max() <= big.n_inner


def test_zeros_cases():
    for name in ("residues", "vector", "with_max"):
        c = cr.zeros_case(name)
        z = np.nonzero(c.values == 0)[0]
        assert {int(r) for r in z % 4} == {0, 1, 2, 3} and z[0] == 0 and z[-1] == c.nnz - 1
    assert np.all(cr.zeros_case("all").values == 0) and cr.zeros_case("with_max").max_value == cr.U32_MAX
    c = cr.zeros_case("vector")
    assert np.all(c.values[int(c.indptr[100]):int(c.indptr[101])] == 0) and c.indptr[101] - c.indptr[100] == 12


# ---- the decoder's tables ---------------------------------------------------------------------------------------------------------
def test_decode_tables():
    import adaptive_vec as av

    grid = cr.decode_grid()
    assert set(grid) == set(cr.DECODE_LENGTHS) and {1, 21, 22, 42, 2048, 2049, 4097, 70001} <= set(grid)
    assert all(len(v) == 25 for v in grid.values())
    vecs, notes = cr.mixed_table()
    assert {v.kind for v in vecs if v.iter()[0].shape[0]} == set(av.KINDS) and all(v.length == cr.MIXED_LENGTH for v in vecs)
    lens = [v.iter()[0].shape[0] for v in vecs]
    assert lens[0] == lens[1] == lens[-1] == lens[-2] == 0 and lens[3] == lens[4] == lens[5] == 0
    for v, note in zip(vecs, notes):
        if not note.startswith("empty"):
            assert v.pieces()["n_units"] > 4 * cr.DECODE_CHUNK, note  # five chunks or more each
    tail = vecs[notes.index("last chunk only")]
    assert tail.kind == "D16" and tail.iter()[0].min() >= (cr.MIXED_LENGTH - 1) // cr.DECODE_CHUNK * cr.DECODE_CHUNK
    for name, v in cr.foreign_vectors():
        pos, val = v.iter()
        assert np.all(val != 0) and np.all(np.diff(pos.astype(np.int64)) > 0), name
        p = v.pieces()
        if name.startswith("only"):
            assert pos.shape[0] == 0 and p["n_units"] > 0, name
        elif name.startswith("stored zeros"):
            assert 0 < pos.shape[0] < 700 and p["n_units"] == 700, name
        else:  # orphans: three entries fewer than the stored values would give
            assert pos.shape[0] == 700 - 3, name


# ---- host_transpose_plan at its edges -----------------------------------------------------------------------------------------------
def test_host_transpose_plan_edges(sa):
    plan = sa.host_transpose_plan
    for n in (0, 1):  # a dimension of 0 or 1: one bit
        assert plan(n, n, 1) == (cr.PACKED, 1, 1, 1)
        assert plan(n, 1000, 5) == (cr.PACKED, 10, 1, 3) and plan(1000, n, 5) == (cr.PACKED, 1, 10, 3)
    assert plan(2, 2, 1) == (cr.PACKED, 1, 1, 1) and plan(3, 2, 1) == (cr.PACKED, 1, 2, 1)
    for max_value, cb in ((0, 32), (1, 1), (2, 2), (3, 2), (2**31 - 1, 31), (2**31, 32), (2**32 - 1, 32)):
        assert plan(65536, 65536, max_value) == (cr.PACKED, 16, 16, cb)
        assert plan(65536, 65537, max_value) == (cr.PACKED if cb < 32 else cr.PAIR, 17, 16, cb)
        assert plan(65537, 65536, max_value) == (cr.PACKED if cb < 32 else cr.PAIR, 16, 17, cb)
        assert plan(65537, 65537, max_value) == (cr.PACKED if cb < 31 else cr.PAIR, 17, 17, cb)
    top = 2**32 - 1
    assert plan(1, top, 1) == (cr.PACKED, 32, 1, 1) and plan(top, 1, 1) == (cr.PACKED, 1, 32, 1)
    assert plan(2**31, top, 1) == (cr.PACKED, 32, 31, 1) and plan(2**31 + 1, top, 1) == (cr.PAIR, 32, 32, 1)
    assert plan(top, top, top) == (cr.PAIR, 32, 32, 32) and plan(1, top, top) == (cr.PAIR, 32, 1, 32) and plan(1, 2**31, top) == (cr.PACKED, 31, 1, 32)
    for rows, cols in ((2**32, 1), (1, 2**32)):
        with pytest.raises(sa.ScanrsError) as e:
            plan(rows, cols, 1)
        assert e.value.code == 1
    for n_outer, n_inner, max_value in ((5, 7, 9), (70000, 65536, 2**32 - 1), (4096, 4096, 2**32 - 1), (123456, 999, 1000)):
        route, ib, ob, cb = plan(n_outer, n_inner, max_value)
        assert (ib, ob, cb) == (bits_for(n_inner - 1), bits_for(n_outer - 1), bits_for(max_value))
        assert route == (cr.PACKED if ib + ob + cb <= 64 else cr.PAIR)
    assert (sa.TRANSPOSE_NONE, sa.TRANSPOSE_PACKED_KEY, sa.TRANSPOSE_PAIR_SORT) == (0, cr.PACKED, cr.PAIR)
