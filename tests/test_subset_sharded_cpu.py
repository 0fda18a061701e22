"""CPU checks of the fixture and the restatement behind tests/test_gpu_subset_sharded.py: the fixture has the
properties the GPU tests rely on, a global list is split over ranges as the library splits it, and the Python-integer restatement
of the fixed-point sums (tests/subset_sharded_ref.py) agrees with the correctly rounded sums of tests/subset_ref.py at the
tolerances the GPU tests use - which shows that those tolerances are reachable by the documented rule alone."""
import math
import os
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import subset_ref as ref  # noqa: E402
import subset_sharded_case as sc  # noqa: E402
import subset_sharded_ref as fx  # noqa: E402

MAPS = ("raw", "scale", "log")
SUM_TOL = dict(rtol=1e-12, atol=1e-13)
VAR_TOL = dict(rtol=1e-10, atol=1e-12)


def close(a, b, rtol, atol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(both_nan | (np.abs(a - b) <= np.abs(b) * rtol + atol)))


@pytest.fixture(scope="module")
def m():
    return sc.matrix()


def test_symbols_are_declared_and_exported():
    import scanrs_amd as sa

    lib = sa._lib
    with open(os.path.join(os.path.dirname(TESTS), "include", "scanrs_amd.h")) as f:
        header = f.read()
    names = [f"scanrs_mat_{n}_sharded" for n in ("sum_rows_u64", "sum_rows_f64", "sum_cols_u64", "sum_cols_f64", "sum_rows_dual_u64",
                                                  "sum_rows_dual_f64", "mean_rows", "mean_var_rows")]
    names += [f"scanrs_multi_{n}" for n in ("sum_rows_u64", "sum_rows_f64", "sum_cols_u64", "sum_cols_f64", "sum_rows_dual_u64",
                                            "sum_rows_dual_f64", "mean_rows", "mean_var_rows")]
    for name in names:
        assert name in sa.EXPORTED_SYMBOLS and hasattr(lib, name) and f"int {name}(" in header, name
    for method in ("sum_rows_sharded", "sum_cols_sharded", "sum_rows_dual_sharded", "mean_rows_sharded", "mean_var_rows_sharded"):
        assert callable(getattr(sa.AdaptiveMat, method))
    for method in ("sum_rows", "sum_cols", "sum_rows_dual", "mean_rows", "mean_var_rows"):
        assert callable(getattr(sa.MultiMat, method))


def test_the_fixture_has_the_properties_the_gpu_tests_rely_on(m):
    assert m.shape == (sc.GENES, sc.CELLS) and m.has_sorted_indices
    assert 0.05 < m.nnz / (sc.GENES * sc.CELLS) < 0.09
    assert m.data.min() == 1 and m.data.max() == sc.MAX_COUNT
    per_gene, per_cell = np.diff(m.indptr), np.diff(m.tocsc().indptr)
    e0, e1 = sc.EMPTY_CELLS
    assert per_gene[sc.EMPTY_GENE] == 0 and not per_cell[e0:e1].any()
    assert per_gene[sc.FULL_GENE] == sc.CELLS - (e1 - e0) and per_cell[:e0].all() and per_cell[e1:].all()
    # the full gene's vector in the transposed copy of a shard: cut into slab pieces at 1 and 2 shards, whole at 3 and 5
    full = (m[sc.FULL_GENE].toarray().reshape(-1) != 0)
    for world, bounds in sc.RANGES.items():
        assert bounds[0] == 0 and bounds[-1] == sc.CELLS and len(bounds) == world + 1 and all(a < b for a, b in zip(bounds, bounds[1:]))
        lens = [int(full[a:b].sum()) for a, b in zip(bounds, bounds[1:])]
        assert all(n > sc.ITEM_NNZ for n in lens) if world <= 2 else all(n <= sc.ITEM_NNZ for n in lens), (world, lens)
    widths = [b - a for a, b in zip(sc.RANGES[5], sc.RANGES[5][1:])]
    assert len(set(widths)) == 5  # uneven
    assert tuple(sc.RANGES[5][2:4]) == sc.EMPTY_CELLS  # a shard without nonzeros
    for world, bounds in sc.GENE_RANGES.items():
        assert bounds[0] == 0 and bounds[-1] == sc.GENES and len(bounds) == world + 1 and all(a < b for a, b in zip(bounds, bounds[1:]))
    assert tuple(sc.GENE_RANGES[5][2:4]) == (sc.EMPTY_GENE, sc.EMPTY_GENE + 1)


@pytest.mark.parametrize("lists, ranges, extent", [(sc.cell_lists(), sc.RANGES, sc.CELLS), (sc.gene_lists(), sc.GENE_RANGES, sc.GENES)],
                         ids=["cells", "genes"])
def test_the_lists_and_their_split_over_the_ranges(lists, ranges, extent):
    for name, idx in lists.items():
        assert np.all(np.diff(idx) > 0) and (idx.size == 0 or (idx[0] >= 0 and idx[-1] < extent)), name
    assert lists["empty"].size == 0 and np.array_equal(lists["all"], np.arange(extent))
    shared = np.intersect1d(lists["third"], lists["half"]).size
    assert shared == (lists["third"].size + 1) // 2 and lists["half"].size > shared
    for world, bounds in ranges.items():
        for name, idx in lists.items():
            parts = sc.split_list(idx, bounds)
            assert len(parts) == world
            back = np.concatenate([loc + lo for (_, loc), lo in zip(parts, bounds[:-1])]) if world else idx
            assert np.array_equal(back, idx), (name, world)
            at = 0
            for (below, loc), lo, hi in zip(parts, bounds[:-1], bounds[1:]):
                assert below == at and (loc.size == 0 or (loc.min() >= 0 and loc.max() < hi - lo))
                at += loc.size
        if world > 1:
            held = [loc.size > 0 for _, loc in sc.split_list(lists["inside"], bounds)]
            assert sum(held) == 1, ("inside", world)  # inside one shard
    for world in (3, 5):
        held = [loc.size > 0 for _, loc in sc.split_list(lists["skips"], ranges[world])]
        assert not all(held) and sum(held) >= 2, ("skips", world)  # skips a whole shard


def test_the_restated_conversions():
    """to_fixed_signed / from_fixed_signed on values whose words are known."""
    assert fx.fx_scale(0.0) == 1.0 and math.isnan(fx.fx_scale(math.inf)) and fx.fx_scale(1e-300) == 2.0 ** 1000
    assert fx.fx_scale(1.0) == 2.0 ** 123 and fx.fx_scale(3.0) == 2.0 ** 122 and fx.fx_scale(0.75) == 2.0 ** 124
    s = 2.0 ** 10
    assert fx.to_fixed_signed(1.0, s) == 1024 and fx.to_fixed_signed(-1.0, s) == -1024
    assert fx.to_fixed_signed(0.5 / 1024, s) == 0 and fx.to_fixed_signed(1.5 / 1024, s) == 2 and fx.to_fixed_signed(-2.5 / 1024, s) == -2  # half to even
    assert fx.from_fixed_signed(-1024, s) == -1.0 and fx.from_fixed_signed((1 << 64) + 3, 1.0) == 18446744073709551616.0 + 3.0
    big = (1 << 120) + (1 << 66) + 1  # the low word is rounded on its own before the sum
    assert fx.from_fixed_signed(big, 1.0) == float(1 << 120) + (float(1 << 66) + 1.0)


@pytest.mark.parametrize("which", MAPS)
def test_the_restatement_meets_the_tolerances_of_the_gpu_tests(m, which):
    """On every list, in both orientations: the fixed-point restatement against the correctly rounded sums."""
    d = sc.mapped_dense(m, which)
    for name, c in sc.cell_lists().items():  # genes x cells, lists of cells
        assert close(fx.sum_rows(d, c), ref.sum_rows(d, c), **SUM_TOL), name
        assert close(fx.mean_rows(d, c), ref.mean_rows(d, c), **SUM_TOL), name
        (gm, gv), (em, ev) = fx.mean_var_rows(d, c), ref.mean_var_rows(d, c)
        assert close(gm, em, **SUM_TOL) and close(gv, ev, **VAR_TOL), name
    lists = sc.cell_lists()
    for a, b in sc.dual_pairs(lists):
        for g, e in zip(fx.sum_rows_dual(d, lists[a], lists[b]), ref.sum_rows_dual(d, lists[a], lists[b])):
            assert close(g, e, **SUM_TOL), (a, b)
    dt = np.ascontiguousarray(d.T)  # cells x genes, lists of genes: sum_cols crosses the shards
    for name, c in sc.gene_lists().items():
        assert close(fx.sum_cols(dt, c), ref.sum_cols(dt, c), **SUM_TOL), name
    if which == "raw":  # integers well below 2^53: the fixed-point sum IS the sum
        c = sc.cell_lists()["third"]
        assert np.array_equal(fx.sum_rows(d, c), ref.sum_rows(d.astype(np.uint64), c).astype(np.float64))


def test_a_term_that_is_not_finite_gives_nan_in_its_result_alone(m):
    d = sc.mapped_dense(m, "raw")
    c = sc.cell_lists()["third"]
    g = int(np.flatnonzero(d[:, c[4]] != 0)[0])
    d[g, c[4]] = math.inf
    got = fx.sum_rows(d, c)
    assert math.isnan(got[g]) and np.isfinite(np.delete(got, g)).all()
    assert np.array_equal(np.delete(got, g), np.delete(ref.sum_rows(d.astype(np.float64), c), g))
