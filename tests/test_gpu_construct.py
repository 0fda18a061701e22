"""Matrix construction on the device (scan-rs_amd/csrc/copy_build.hip: validate_copy, compact_nonzeros, sort_outer_vectors,
build_items, build_transposed_copy) against the plain numpy reference tests/construct_ref.py. The transposed copy is read directly,
through to_adaptive_vecs("V", major="inner"), whose fallback_indexes / fallback_values per vector are the copy's (indices, values),
and every case asserts the sort route it was planned to take (host_transpose_plan) and the one it took (counter "transpose_route").
Integer work: every comparison is equality. The cases' own properties are checked in tests/test_construct_cpu.py."""
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import construct_ref as cr  # noqa: E402

ORDER = "indices must be in range and strictly ascending within each outer vector"


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def handle(sa, case, storage=None, unsorted=False):
    """The case as the rows of a CSR matrix (default) or as the columns of a CSC matrix: the same copy either way."""
    storage = sa.CSR if storage is None else storage
    rows, cols = (case.n_outer, case.n_inner) if storage == sa.CSR else (case.n_inner, case.n_outer)
    return sa.AdaptiveMat.from_csmat(rows, cols, storage, *case.triplet, unsorted=unsorted)


def inner_export(h, n_outer, n_inner):
    """The handle's transposed copy as a triplet: one V vector per inner position, its entries the copy's (indices, values)."""
    vecs = h.to_adaptive_vecs("V", major="inner")
    assert len(vecs) == n_inner
    assert all(v["kind"] == 4 and v["len"] == n_outer and v["n_units"] == v["fallback_indexes"].shape[0] == v["fallback_values"].shape[0] for v in vecs)
    ip = np.concatenate([[0], np.cumsum([v["n_units"] for v in vecs])]).astype(np.uint64)
    cat = lambda k: np.concatenate([v[k] for v in vecs]).astype(np.uint32) if vecs else np.zeros(0, dtype=np.uint32)  # noqa: E731
    return ip, cat("fallback_indexes"), cat("fallback_values")


def check_copies(sa, h, n_outer, n_inner, want, route, where, storage=None, fresh=True):
    """nnz(), to_csmat(), the inner export, the route and the u32 products of a handle against the reference triplet `want`."""
    storage = sa.CSR if storage is None else storage
    assert h.storage() == storage and h.shape() == ([n_outer, n_inner] if storage == sa.CSR else [n_inner, n_outer]), where
    assert h.nnz() == want[1].shape[0], where
    assert same(h.to_csmat(), want), where
    if fresh:
        assert h.counter("transpose_route") == sa.TRANSPOSE_NONE, where  # no transposed copy yet
    assert same(inner_export(h, n_outer, n_inner), cr.transpose(n_outer, n_inner, *want)), where
    assert h.counter("transpose_route") == route, (where, route)
    rng = np.random.default_rng(n_outer + n_inner)
    x = rng.integers(0, 2**32, size=(n_inner, 2), dtype=np.uint64).astype(np.uint32)
    y = rng.integers(0, 2**32, size=(n_outer, 3), dtype=np.uint64).astype(np.uint32)
    ax, aty = cr.product(n_outer, *want, x), cr.product_t(n_outer, n_inner, *want, y)
    if storage == sa.CSR:  # rows are the outer vectors
        assert np.array_equal(h.dot(x), ax), where
        assert np.array_equal(h.rdot(np.ascontiguousarray(y.T)), aty.T), where
    else:
        assert np.array_equal(h.dot(y), aty), where
        assert np.array_equal(h.rdot(np.ascontiguousarray(x.T)), ax.T), where
    assert same(h.to_csmat(), want) and h.counter("transpose_route") == route, where


def planned(sa, case, max_value=None):
    if case.nnz == 0:
        return sa.TRANSPOSE_NONE
    return sa.host_transpose_plan(case.n_outer, case.n_inner, case.max_value if max_value is None else max_value)[0]


# ---- the transposed copy, both sort routes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cr.TRANSPOSE_CASES))
def test_transposed_copy_equals_the_stable_sort(sa, name):
    c = cr.transpose_case(name)
    route = planned(sa, c)
    assert route == (cr.TRANSPOSE_CASES[name][1] if cr.TRANSPOSE_CASES[name] else sa.TRANSPOSE_NONE)
    check_copies(sa, handle(sa, c), c.n_outer, c.n_inner, c.triplet, route, name)
    if name in ("pair_66", "long_pair", "long_packed", "all_ones", "empty", "one_inner"):
        check_copies(sa, handle(sa, c, sa.CSC), c.n_outer, c.n_inner, c.triplet, route, name + " csc", storage=sa.CSC)


def test_both_routes_occur(sa):
    routes = {planned(sa, cr.transpose_case(name)) for name in cr.TRANSPOSE_CASES}
    assert routes == {sa.TRANSPOSE_NONE, sa.TRANSPOSE_PACKED_KEY, sa.TRANSPOSE_PAIR_SORT}


def test_transposed_copy_of_a_triplet_in_device_memory(sa):
    import torch

    c = cr.transpose_case("pair_65")
    dev = [torch.from_numpy(a.view(dt).copy()).cuda() for a, dt in zip(c.triplet, (np.int64, np.int32, np.int32))]
    torch.cuda.synchronize()
    h = sa.AdaptiveMat.from_device(c.n_outer, c.n_inner, sa.CSR, *(t.data_ptr() for t in dev))
    del dev
    check_copies(sa, h, c.n_outer, c.n_inner, c.triplet, sa.TRANSPOSE_PAIR_SORT, "from_device")


@pytest.fixture(scope="module")
def wide(sa):
    """pair_65 (65536 x 65537 with one count 2^32 - 1) as a handle, and where that count sits"""
    c = cr.transpose_case("pair_65")
    at = c.notes["big_at"]
    return c, handle(sa, c), cr.vector_of(c.indptr, at), int(c.indices[at])


@pytest.mark.parametrize("axis,keeps,n_idx", [("rows", True, 65537), ("rows", False, 3000), ("cols", True, 4000), ("cols", False, 65537)])
def test_selected_copies_inherit_a_bound_for_their_route(sa, wide, axis, keeps, n_idx):
    c, h, big_outer, big_inner = wide
    rng = np.random.default_rng(n_idx)
    extent, big = (c.n_outer, big_outer) if axis == "rows" else (c.n_inner, big_inner)
    idx = rng.integers(0, extent, size=n_idx)  # permuted, with repeats
    idx[idx == big] = (big + 1) % extent
    if keeps:
        idx[[7, n_idx // 2]] = big
    if axis == "rows":
        got, want = h.select_rows(idx), cr.select_outer(c.n_outer, *c.triplet, idx)
        n_outer, n_inner = n_idx, c.n_inner
    else:
        got, want = h.select_cols(idx), cr.select_inner(*c.args(), idx)
        n_outer, n_inner = c.n_outer, n_idx
    own = int(want[2].max())
    assert (own == cr.U32_MAX) == keeps and want[1].shape[0] > 0
    route = sa.host_transpose_plan(n_outer, n_inner, cr.U32_MAX)[0]  # the source's largest count, not the result's own
    assert route == (sa.TRANSPOSE_PAIR_SORT if n_idx == 65537 else sa.TRANSPOSE_PACKED_KEY)
    if n_idx == 65537 and not keeps:
        assert sa.host_transpose_plan(n_outer, n_inner, own)[0] == sa.TRANSPOSE_PACKED_KEY  # (its own maximum would have fitted)
    check_copies(sa, got, n_outer, n_inner, want, route, (axis, keeps, n_idx))


# ---- where the largest count is read ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cr.MAX_CASES)
def test_largest_count_in_the_last_chunk_or_first(sa, name):
    c = cr.max_case(name)
    check_copies(sa, handle(sa, c), c.n_outer, c.n_inner, c.triplet, sa.TRANSPOSE_PACKED_KEY, name)


@pytest.fixture(scope="module")
def big(sa):
    """The ~4.2 M-nonzero case sized by this device's CU count, and its handle: made once for the tests that use it."""
    import torch

    c = cr.big_case(int(torch.cuda.get_device_properties(0).multi_processor_count))
    return c, handle(sa, c)


def test_largest_count_in_the_second_grid_stride_trip(sa, big):
    c, h = big
    at = c.notes["big_at"]
    assert c.nnz - 1029 <= at < c.nnz and c.values[at] == cr.U32_MAX and planned(sa, c) == sa.TRANSPOSE_PACKED_KEY
    assert h.nnz() == c.nnz and same(h.to_csmat(), c.triplet)
    assert same(inner_export(h, c.n_outer, c.n_inner), cr.transpose(*c.args()))
    assert h.counter("transpose_route") == sa.TRANSPOSE_PACKED_KEY


# ---- validation -------------------------------------------------------------------------------------------------------------------
def refused(sa, case, exactly=None, unsorted=False):
    with pytest.raises(sa.ScanrsError) as e:
        handle(sa, case, unsorted=unsorted)
    assert e.value.code == 6 and ORDER in str(e.value), str(e.value)
    count = int(re.search(r"\((\d+) violations\)", str(e.value)).group(1))
    print("violations reported:", count, "expected:", exactly)
    assert count >= 1 if exactly is None else count == exactly, (count, exactly)


def test_valid_matrix_is_accepted_unchanged(sa):
    base = cr.valid_base()
    assert cr.validate(*base.args())[0] == 0
    for storage in (sa.CSR, sa.CSC):
        check_copies(sa, handle(sa, base, storage), base.n_outer, base.n_inner, base.triplet, sa.TRANSPOSE_PACKED_KEY, "valid_base", storage=storage)


@pytest.mark.parametrize("violation", cr.VIOLATIONS)
def test_one_violation_is_refused_wherever_it_sits(sa, violation):
    base = cr.valid_base()
    for where in cr.PLACES:
        bad = cr.violate(base, violation, cr.place(base, violation, where))
        want = cr.validate(*bad.args())[0]
        assert want >= 1
        refused(sa, bad, want if violation in ("descent", "duplicate", "beyond") else None)


@pytest.mark.parametrize("violation", cr.VIOLATIONS)
def test_one_violation_in_the_second_grid_stride_trip_is_refused(sa, big, violation):
    c, _ = big
    p = cr.place(c, violation, "second_trip")
    assert c.notes["second_trip"] <= p < c.nnz
    refused(sa, cr.violate(c, violation, p), 1 if violation in ("descent", "duplicate", "beyond") else None)


def test_descents_at_vector_starts_are_accepted(sa):
    base = cr.valid_base()
    places = cr.start_descent_places(base)  # a start at every residue of the chunk of four, the last start, the start behind a run of empty vectors
    ip = base.indptr.astype(np.int64)
    assert len(places) == 6 and all(p in ip and base.indices[p] <= base.indices[p - 1] for p in places.values())
    assert same(handle(sa, base).to_csmat(), base.triplet)
    eq, at = cr.equal_across_a_start(base)  # equality across a start, at every residue
    assert sorted(p % 4 for p in at) == [0, 1, 2, 3] and cr.validate(*eq.args())[0] == 0
    assert same(handle(sa, eq).to_csmat(), eq.triplet)
    # one vector start alone, at each residue: two vectors, the second starting below the end of the first
    for n_first in (4, 5, 6, 7):
        two = cr.Case(2, 50, [0, n_first, n_first + 3], list(range(20, 20 + n_first)) + [3, 40, 41], np.arange(1, n_first + 4))
        assert same(handle(sa, two).to_csmat(), two.triplet)
        ix = two.indices.copy()
        ix[n_first] = ix[n_first - 1]  # equal to the index before the start
        two = two.with_arrays(indices=ix)
        assert cr.validate(*two.args())[0] == 0 and same(handle(sa, two).to_csmat(), two.triplet)


def test_every_start_a_descent_and_one_real_violation(sa):
    d = cr.all_starts_descend()
    check_copies(sa, handle(sa, d), d.n_outer, d.n_inner, d.triplet, sa.TRANSPOSE_PACKED_KEY, "all starts descend")
    for violation in ("descent", "duplicate", "beyond"):
        for where in ("mod_0", "mod_1", "mod_2", "mod_3", "last"):
            bad = cr.violate(d, violation, cr.place(d, violation, where))
            assert cr.validate(*bad.args())[0] == 1
            refused(sa, bad, 1)


# ---- stored zeros -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cr.ZEROS_CASES)
def test_stored_zeros_are_dropped(sa, name):
    c = cr.zeros_case(name)
    want = cr.compact(c.n_outer, *c.triplet)
    assert cr.validate(*c.args())[:2] == (0, int(np.count_nonzero(c.values == 0))) and want[1].shape[0] < c.nnz
    route = sa.TRANSPOSE_NONE if name == "all" else sa.TRANSPOSE_PACKED_KEY
    assert (want[1].shape[0] == 0) == (name == "all")
    for storage in (sa.CSR, sa.CSC):
        check_copies(sa, handle(sa, c, storage), c.n_outer, c.n_inner, want, route, name, storage=storage)


# ---- unsorted input ---------------------------------------------------------------------------------------------------------------
def test_unsorted_vectors_are_sorted(sa):
    u = cr.unsorted_case()
    want = cr.sort_within(u.n_outer, *u.triplet)
    refused(sa, u)  # without the flag the same arrays are refused
    check_copies(sa, handle(sa, u, unsorted=True), u.n_outer, u.n_inner, want, sa.TRANSPOSE_PACKED_KEY, "unsorted")
    assert same(handle(sa, u, sa.CSC, unsorted=True).to_csmat(), want)


def test_unsorted_with_a_repeated_index_is_refused(sa):
    u = cr.unsorted_case()
    for o, i, j in ((6, 7, 12000), (2, 0, 8191), (5, 8192, 100)):  # inside the 20000-, the 8192- and the 8193-vector
        ix = u.indices.copy()
        a = int(u.indptr[o])
        ix[a + i] = ix[a + j]
        refused(sa, u.with_arrays(indices=ix), 1, unsorted=True)


def test_unsorted_with_stored_zeros_is_sorted_then_compacted(sa):
    u = cr.unsorted_case(zeros=True)
    want = cr.compact(u.n_outer, *cr.sort_within(u.n_outer, *u.triplet))
    assert want[1].shape[0] == u.nnz - 500
    check_copies(sa, handle(sa, u, unsorted=True), u.n_outer, u.n_inner, want, sa.TRANSPOSE_PACKED_KEY, "unsorted with zeros")


# ---- work items -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage_name", ["csr", "csc"])
def test_vectors_at_the_work_item_edges(sa, storage_name):
    c = cr.items_case()
    storage = sa.CSR if storage_name == "csr" else sa.CSC
    h = handle(sa, c, storage)
    check_copies(sa, h, c.n_outer, c.n_inner, c.triplet, sa.TRANSPOSE_PACKED_KEY, "items", storage=storage)
    per_outer, per_inner = cr.sums(*c.args())
    for fresh in (h, handle(sa, c, storage)):  # with both copies built, and from the stored one alone
        over_rows, over_cols = fresh.sum_axis(0, dtype=np.uint32), fresh.sum_axis(1, dtype=np.uint32)
        assert np.array_equal(over_cols if storage == sa.CSR else over_rows, per_outer)
        assert np.array_equal(over_rows if storage == sa.CSR else over_cols, per_inner)
