"""sSeq differential expression over sharded and multi-GPU matrices: every output of `compute_sseq_params`,
`group_sums` and DE on a `MultiMat` or a sharded handle must equal the call on one unsharded `AdaptiveMat` of the same matrix bit for
bit, for any number of shards: all sums that cross the shards are integers. The fixture is tests/sseq_sharded_case.py; the reference
of every comparison is computed once per module on an unsharded handle."""
import os
import sys

import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import sseq_ref as ref  # noqa: E402
import sseq_sharded_case as sc  # noqa: E402

PARAM_FIELDS = ("size_factors", "gene_means", "gene_variances", "use_genes", "gene_moment_phi", "gene_phi")
DE_FIELDS = ("genes_tested", "sums_in", "sums_out", "common_mean", "common_dispersion", "normalized_mean_in", "normalized_mean_out", "p_values",
             "adjusted_p_values", "log2_fold_change")
VARIANTS = ("all", "cells", "umi")  # compute_sseq_params over every cell / over cell_indices / with umi_counts
SHARDS = (1, 2, 3, 5)
FORMS = ("csc", "csr_t")  # MultiMat(genes, cells, CSC) / MultiMat(cells, genes, CSR) with transposed=True


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


@pytest.fixture(scope="module")
def case():
    return sc.make_case()


def _csc_handle(sa, m):
    s = sparse.csc_matrix(m)
    s.sort_indices()
    return sa.AdaptiveMat.from_csmat(s.shape[0], s.shape[1], sa.CSC, s.indptr.astype(np.uint64), s.indices.astype(np.uint32), s.data.astype(np.uint32))


def _multi(sa, m, form, n_shards):
    """genes x cells scipy matrix -> (MultiMat with the cells sharded, transposed flag)."""
    s = sparse.csc_matrix(m)
    s.sort_indices()
    g, c = s.shape
    ip, ix, vv = s.indptr.astype(np.uint64), s.indices.astype(np.uint32), s.data.astype(np.uint32)
    if form == "csc":
        return sa.MultiMat(g, c, sa.CSC, ip, ix, vv, n_shards, devices=[0] * n_shards), False
    return sa.MultiMat(c, g, sa.CSR, ip, ix, vv, n_shards, devices=[0] * n_shards), True  # the CSC arrays of m are the CSR arrays of its transpose


def _variant_args(case, variant):
    if variant == "cells":
        return dict(cell_indices=case["subset"])
    if variant == "umi":
        return dict(umi_counts=case["umi_all"])
    return {}


def _run_all(sa, mat, case, variant, **kw):
    """Everything the feature serves, in one dict of arrays: the parameters, the group sums and DE in modes 0, 1 and 2 with both
    backends at both values of big_count."""
    labels = case["labels"]
    out = {}
    params = sa.compute_sseq_params(mat, 0.995, **_variant_args(case, variant), **kw)
    for f in PARAM_FIELDS:
        out["params." + f] = np.asarray(getattr(params, f))
    out["params.scalars"] = np.array([params.zeta_hat, params.delta, params.num_cells, params.num_genes], dtype=np.float64)
    sums, cnt = sa.group_sums(mat, labels, sc.N_GROUPS, **kw)
    out["group_sums"], out["cells_per_group"] = sums, cnt
    for backend in (sa.NB_EXACT_LOGSPACE, sa.NB_EXACT_RATIO):
        for big in sc.BIG_COUNTS:
            res = {
                0: sa.sseq_de_one_vs_rest(mat, labels, params, big_count=big, n_groups=sc.N_GROUPS, backend=backend, **kw),
                1: [sa.sseq_differential_expression(mat, np.flatnonzero(labels == 0), np.flatnonzero(labels == 1), params, big_count=big,
                                                    backend=backend, **kw)],
                2: sa.sseq_de_vs_control(mat, labels, params, control=0, big_count=big, n_groups=sc.N_GROUPS, backend=backend, **kw),
            }
            for mode, rs in res.items():
                assert len(rs) == sc.n_tests(mode)
                for j, r in enumerate(rs):
                    for f in DE_FIELDS:
                        out[f"de.b{backend}.big{big}.m{mode}.t{j}.{f}"] = np.asarray(getattr(r, f))
    return out, params


@pytest.fixture(scope="module")
def unsharded(sa, case):
    """variant -> (outputs, params) of the unsharded handle: the reference of every bit comparison, computed once."""
    h = _csc_handle(sa, case["mat"])
    return {v: _run_all(sa, h, case, v) for v in VARIANTS}


@pytest.fixture(scope="module")
def multis(sa, case):
    made = {}

    def get(form, n_shards):
        if (form, n_shards) not in made:
            made[(form, n_shards)] = _multi(sa, case["mat"], form, n_shards)
        return made[(form, n_shards)]

    yield get
    for mm, _ in made.values():
        mm.close()


def _assert_same_bits(got, exp):
    assert got.keys() == exp.keys()
    for k in exp:
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, k
        assert np.array_equal(got[k], exp[k], equal_nan=got[k].dtype.kind == "f"), k


# ---- 1. and 2. bit identity: every cell, then cell_indices (unsorted, across every shard boundary) and umi_counts -----------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_shards", SHARDS)
def test_every_output_equals_the_unsharded_call_bit_for_bit(sa, case, unsharded, multis, n_shards, form, variant):
    mm, transposed = multis(form, n_shards)
    ranges = mm.shard_ranges()
    assert len(ranges) == n_shards and ranges[0][1] == 0 and ranges[-1][2] == sc.CELLS
    if variant == "cells":
        sub = np.sort(case["subset"].astype(np.int64))
        assert np.any(np.diff(case["subset"].astype(np.int64)) < 0)  # unsorted
        for _, lo, hi in ranges:  # the subset has members and gaps in every shard
            inside = np.count_nonzero((sub >= lo) & (sub < hi))
            assert 0 < inside < hi - lo
    if n_shards >= 3:  # group 3 lies in the first 40 cells: the last shard holds none of it
        assert not np.any(case["labels"][ranges[-1][1]:] == 3)
    got, _ = _run_all(sa, mm, case, variant, transposed=transposed)
    _assert_same_bits(got, unsharded[variant][0])


def test_the_fixture_reaches_both_branches(case):
    params = ref.compute_sseq_params(case["mat"])
    for mode in (0, 1, 2):
        asym, exact, settled = sc.branch_counts(case["mat"], case["labels"], params, mode, sc.BIG_COUNTS[1])
        assert asym > 0 and exact > 0 and settled > 0, (mode, asym, exact, settled)


# ---- 3. against the restatement, at the bounds tests/test_gpu_sseq.py uses for the unsharded call ------------------------------------------
def _assert_params(got, exp, cells):  # tests/test_gpu_sseq.py::_assert_params
    np.testing.assert_array_equal(got.use_genes, exp["use_genes"])
    for f in ("size_factors", "gene_means", "gene_variances", "gene_moment_phi", "gene_phi"):
        np.testing.assert_allclose(getattr(got, f), exp[f], rtol=1e-12, atol=1e-12 * np.max(np.abs(exp[f])), err_msg=f)
    np.testing.assert_allclose([got.zeta_hat, got.delta], [exp["zeta_hat"], exp["delta"]], rtol=1e-12)
    assert len(got.size_factors) == cells


def _assert_de(got, exp, prtol=1e-9):  # tests/test_gpu_sseq.py::_assert_de
    for f in ("sums_in", "sums_out", "p_values", "adjusted_p_values", "log2_fold_change", "normalized_mean_in", "normalized_mean_out"):
        g, e = getattr(got, f), exp[f]
        if f.startswith("sums"):
            np.testing.assert_array_equal(g, e, err_msg=f)
        else:
            np.testing.assert_allclose(g, e, rtol=prtol if "p_values" in f else 1e-12, atol=0, err_msg=f)


@pytest.mark.parametrize("form", FORMS)
def test_three_shards_against_the_restatement(sa, case, multis, form):
    mm, transposed = multis(form, 3)
    m, labels = case["mat"], case["labels"]
    for variant in VARIANTS:
        args = _variant_args(case, variant)
        _assert_params(sa.compute_sseq_params(mm, 0.995, transposed=transposed, **args), ref.compute_sseq_params(m, 0.995, **args), sc.CELLS)
    params, pref = sa.compute_sseq_params(mm, transposed=transposed), ref.compute_sseq_params(m)
    for big in sc.BIG_COUNTS:
        kw = {} if big is None else dict(big_count=big)
        got = sa.sseq_de_one_vs_rest(mm, labels, params, n_groups=sc.N_GROUPS, transposed=transposed, **kw)
        for g, e in zip(got, ref.one_vs_rest(m, labels, pref, n_groups=sc.N_GROUPS, **kw)):
            _assert_de(g, e)
        got = sa.sseq_de_vs_control(mm, labels, params, control=0, n_groups=sc.N_GROUPS, transposed=transposed, **kw)
        for g, (a, b) in zip(got, sc.sides_of_tests(labels, 2)):
            _assert_de(g, ref.differential_expression(m, a, b, pref, **kw))


# ---- 4. the tests are split over the shards ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", [0, 1])
def test_the_test_stage_is_split_by_gene(sa, case, unsharded, multis, backend):
    labels, params = case["labels"], unsharded["all"][1]
    h = _csc_handle(sa, case["mat"])
    mm, transposed = multis("csc", 3)
    for mode, big in ((0, None), (0, sc.BIG_COUNTS[1]), (2, None)):
        f = sa.sseq_de_one_vs_rest if mode == 0 else sa.sseq_de_vs_control
        f(h, labels, params, big_count=big, n_groups=sc.N_GROUPS, backend=backend)
        f(mm, labels, params, big_count=big, n_groups=sc.N_GROUPS, backend=backend, transposed=transposed)
        whole = h.counter("de_shard_tests")
        asym, exact, _ = sc.branch_counts(case["mat"], labels, ref.compute_sseq_params(case["mat"]), mode, big)
        assert whole == asym + exact and h.counter("de_shard_allreduces") == 0
        per_shard = [mm.counter("de_shard_tests", i) for i in range(3)]
        assert sum(per_shard) == whole, per_shard
        assert max(per_shard) <= -(-sc.GENES // 3) * sc.n_tests(mode) and min(per_shard) > 0, per_shard
        steps = [mm.counter("de_shard_allreduces", i) for i in range(3)]
        assert steps[0] == steps[1] == steps[2] == 2, steps  # the group sums and the p-values


# ---- 5. the host-hook transport ---------------------------------------------------------------------------------------------------------------
def test_a_host_hook_carries_every_exchange_as_u64(sa, case, unsharded):
    calls = []

    def hook(ptr, count, dtype):
        calls.append((count, dtype))
        return 0

    h = _csc_handle(sa, case["mat"])
    h.set_shard(0, 1, 0, sc.CELLS, hook)
    for variant in ("all", "cells"):
        got, _ = _run_all(sa, h, case, variant)
        _assert_same_bits(got, unsharded[variant][0])
    assert calls and {d for _, d in calls} == {1}
    assert (sc.CELLS, 1) in calls and (sc.GENES * sc.N_GROUPS, 1) in calls and (sc.GENES * 9, 1) in calls and (1, 1) in calls
    # through the transposed view of a cells x genes CSR handle as well
    calls.clear()
    s = sparse.csr_matrix(case["mat"].T)
    s.sort_indices()
    ht = sa.AdaptiveMat.from_csmat(sc.CELLS, sc.GENES, sa.CSR, s.indptr.astype(np.uint64), s.indices.astype(np.uint32), s.data.astype(np.uint32))
    ht.set_shard(0, 1, 0, sc.CELLS, hook)
    got, _ = _run_all(sa, ht.t(), case, "umi")
    _assert_same_bits(got, unsharded["umi"][0])
    assert calls and {d for _, d in calls} == {1}


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_cancellation(sa, case, unsharded, multis):
    m, labels, params = case["mat"], case["labels"], unsharded["all"][1]
    # the genes sharded: a gene-major handle sharded over its rows, and a MultiMat created gene-major
    s = sparse.csr_matrix(m)
    s.sort_indices()
    ip, ix, vv = s.indptr.astype(np.uint64), s.indices.astype(np.uint32), s.data.astype(np.uint32)
    hg = sa.AdaptiveMat.from_csmat(sc.GENES, sc.CELLS, sa.CSR, ip, ix, vv)
    hg.set_shard(0, 1, 0, sc.GENES, lambda *a: 0)
    mg = sa.MultiMat(sc.GENES, sc.CELLS, sa.CSR, ip, ix, vv, 2, devices=[0, 0])
    for mat in (hg, mg):
        for call in (lambda: sa.compute_sseq_params(mat), lambda: sa.group_sums(mat, labels, sc.N_GROUPS),
                     lambda: sa.sseq_de_one_vs_rest(mat, labels, params, n_groups=sc.N_GROUPS)):
            with pytest.raises(sa.ScanrsError) as e:
                call()
            assert e.value.code == 6 and "cells" in str(e.value) and "sharded" in str(e.value)
    mg.close()
    mm, transposed = multis("csc", 3)
    lo, hi = mm.shard_ranges()[1][1:]
    for short in (labels[:-1], labels[lo:hi]):  # one short of the global count; the slice of one shard
        with pytest.raises(sa.ScanrsError):
            sa.group_sums(mm, short, sc.N_GROUPS)
        with pytest.raises(sa.ScanrsError):
            sa.sseq_de_one_vs_rest(mm, short, params, n_groups=sc.N_GROUPS)
    # a cancelled snoop: SCANRS_ERR_CANCELLED from the MultiMat call, and the handle serves the next call
    sn = sa.AtomicSnoop()
    sn.cancel()
    with pytest.raises(sa.CancellationError) as e:
        sa.sseq_de_one_vs_rest(mm, labels, params, n_groups=sc.N_GROUPS, snoop=sn, transposed=transposed)
    assert e.value.code == 3
    seen = sa.AtomicSnoop()
    got = sa.sseq_de_one_vs_rest(mm, labels, params, n_groups=sc.N_GROUPS, snoop=seen, transposed=transposed)
    for j, r in enumerate(got):
        for f in DE_FIELDS:
            exp = unsharded["all"][0][f"de.b0.bigNone.m0.t{j}.{f}"]
            assert np.array_equal(np.asarray(getattr(r, f)), exp, equal_nan=exp.dtype.kind == "f"), (j, f)
    assert not seen.is_cancelled()


# ---- 7. a shard without nonzeros --------------------------------------------------------------------------------------------------------------
def test_a_shard_without_nonzeros(sa, case):
    """scanrs_plan_shards cuts by nonzeros: the last shard gets none when the last non-empty cell holds more than a fifth of them. Ten
    cells of the fixture, one cell with every gene, then a tail of 30 empty cells, over 5 shards."""
    head = sparse.csc_matrix(case["mat"])[:, 20:30].toarray()
    full = np.arange(1, sc.GENES + 1, dtype=np.uint32).reshape(-1, 1) * 3
    dense = np.hstack([head, full, np.zeros((sc.GENES, 30), dtype=np.uint32)]).astype(np.uint32)
    m = sparse.csc_matrix(dense)
    m.sort_indices()
    cells = m.shape[1]
    bounds = sa.plan_shards(m.indptr.astype(np.uint64), 5)
    assert bounds[4] < cells and m.indptr[bounds[4]] == m.nnz  # the last shard: cells, no nonzeros
    rng = np.random.default_rng(5)
    sub = dict(case, mat=m, labels=rng.integers(-1, 5, cells).astype(np.int16), subset=rng.permutation(cells)[:30].astype(np.uint64),
               umi_all=rng.uniform(50.0, 4000.0, cells))
    exp = {v: _run_all(sa, _csc_handle(sa, m), sub, v)[0] for v in VARIANTS}
    for form in FORMS:
        mm, transposed = _multi(sa, m, form, 5)
        assert mm.shard_ranges()[-1][1] == bounds[4]
        for v in VARIANTS:
            _assert_same_bits(_run_all(sa, mm, sub, v, transposed=transposed)[0], exp[v])
        mm.close()
