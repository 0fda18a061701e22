"""sseq_de_pairs over sharded and multi-GPU matrices: every field of the results and of the per-pair parameters from
a `MultiMat` or a sharded handle must equal the call on one unsharded `AdaptiveMat` of the same matrix bit for bit, for any number of
shards: all sums that cross the shards are integers. The fixture is tests/pairs_sharded_case.py; the reference of every comparison is
computed once per module on an unsharded handle."""
import os
import sys

import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import pairs_sharded_case as pc  # noqa: E402
import sseq_pairs_ref as pref  # noqa: E402

FORMS = ("csc", "csr_t")  # MultiMat(genes, cells, CSC) / MultiMat(cells, genes, CSR) with transposed=True
BACKENDS = (pref.LOGSPACE, pref.RATIO)


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


@pytest.fixture(scope="module")
def case():
    return pc.make_case()


def _handle(sa, m, storage="csc"):
    s = sparse.csc_matrix(m) if storage == "csc" else sparse.csr_matrix(m)
    s.sort_indices()
    return sa.AdaptiveMat.from_csmat(s.shape[0], s.shape[1], sa.CSC if storage == "csc" else sa.CSR, s.indptr.astype(np.uint64),
                                     s.indices.astype(np.uint32), s.data.astype(np.uint32))


def _multi(sa, m, form, n_shards):
    """genes x cells scipy matrix -> (MultiMat with the cells sharded, transposed flag)."""
    s = sparse.csc_matrix(m)
    s.sort_indices()
    g, c = s.shape
    ip, ix, vv = s.indptr.astype(np.uint64), s.indices.astype(np.uint32), s.data.astype(np.uint32)
    if form == "csc":
        return sa.MultiMat(g, c, sa.CSC, ip, ix, vv, n_shards, devices=[0] * n_shards), False
    return sa.MultiMat(c, g, sa.CSR, ip, ix, vv, n_shards, devices=[0] * n_shards), True  # the CSC arrays of m are the CSR arrays of its transpose


def _run(sa, mat, case, backend, **kw):
    """(arrays of the pairs call, arrays of each-against-the-control, the pairs call's own return)."""
    got = sa.sseq_de_pairs(mat, case["labels"], case["pairs"], backend=backend, n_groups=case["n_groups"], **kw)
    ctl = sa.sseq_de_each_vs_control(mat, case["labels"], control=0, backend=backend, n_groups=case["n_groups"], **kw)
    return pc.as_arrays(*got), pc.as_arrays(*ctl), got


@pytest.fixture(scope="module")
def unsharded(sa, case):
    h = _handle(sa, case["mat"])
    return {b: _run(sa, h, case, b) for b in BACKENDS}


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


# ---- 1. bit equality -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_shards", pc.SHARDS)
def test_every_field_equals_the_unsharded_call_bit_for_bit(sa, case, unsharded, multis, n_shards, form, backend):
    mm, transposed = multis(form, n_shards)
    ranges = mm.shard_ranges()
    assert len(ranges) == n_shards and ranges[0][1] == 0 and ranges[-1][2] == case["cells"]
    labels = case["labels"]
    if n_shards > 1:  # a group inside one shard; at five shards a shard without a labelled cell
        assert np.flatnonzero(labels == case["one_shard_group"]).min() >= ranges[-1][1]
    if n_shards == 5:
        assert np.all(labels[ranges[1][1]:ranges[1][2]] == -1)
    pairs, ctl, raw = _run(sa, mm, case, backend, transposed=transposed)
    pc.assert_same_bits(pairs, unsharded[backend][0])
    pc.assert_same_bits(ctl, unsharded[backend][1])
    lit = [bool(q.literal) for q in raw[1]]
    assert lit == [pr == case["literal_pair"] for pr in case["pairs"]] and raw[1][lit.index(True)].median_total == 0.0


# ---- 2. against the restatements, at the bounds of tests/test_gpu_sseq_pairs.py -------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_three_shards_against_the_restatements(sa, case, multis, backend):
    mm, transposed = multis("csr_t", 3)
    results, params = sa.sseq_de_pairs(mm, case["labels"], case["pairs"], backend=backend, n_groups=case["n_groups"], transposed=transposed)
    gs = pref.GroupSums(case["mat"], case["labels"], case["n_groups"])
    n_tie = {"literal": 0, "fused": 0}
    for j, (a, b) in enumerate(case["pairs"]):
        r, q = results[j], params[j]
        what = f"pair {(a, b)} backend {backend}"
        assert (q.num_cells_a, q.num_cells_b) == (int(np.sum(case["labels"] == a)), int(np.sum(case["labels"] == b)))
        if (a, b) == case["literal_pair"]:
            # the library's own sharded literal calls, bit for bit (the union's size factors are not finite: no restatement bounds apply)
            ca, cb = np.flatnonzero(case["labels"] == a), np.flatnonzero(case["labels"] == b)
            lp = sa.compute_sseq_params(mm, cell_indices=np.concatenate([ca, cb]), transposed=transposed)
            lr = sa.sseq_differential_expression(mm, ca, cb, lp, backend=backend, transposed=transposed)
            for f in ("sums_in", "sums_out", "p_values", "adjusted_p_values", "log2_fold_change", "normalized_mean_in", "normalized_mean_out"):
                assert np.ascontiguousarray(getattr(r, f)).tobytes() == np.ascontiguousarray(getattr(lr, f)).tobytes(), f
            for f in pc.PARAM_FIELDS + ("zeta_hat", "delta"):
                assert np.ascontiguousarray(getattr(q, f)).tobytes() == np.ascontiguousarray(getattr(lp, f)).tobytes(), f
            continue
        ep, er = pref.fused_pair(gs, a, b, backend=backend)
        pc.assert_params(q, ep, what + " fused")
        n_tie["fused"] += pc.assert_result(r, q, er, backend, what + " fused", True)
        np.testing.assert_allclose([q.median_total, q.sum_size_factors], [ep["median_total"], ep["sum_size_factors"]], rtol=1e-15, atol=0)
        lp, lr = pref.literal_pair(case["mat"], case["labels"], a, b, backend=backend)
        pc.assert_params(q, lp, what + " literal")
        if case["empty_group"] not in (a, b):
            n_tie["literal"] += pc.assert_result(r, q, lr, backend, what + " literal", False)
        else:
            assert np.all(r.p_values == 1.0) and np.all(r.adjusted_p_values == 1.0)
    assert max(n_tie.values()) <= 1e-3 * case["genes"] * len(case["pairs"]), n_tie


# ---- 3. tiles ---------------------------------------------------------------------------------------------------------------------------
def _many_groups(genes, seed):
    """1 600 groups of 3 cells (more than one 1 536-group tile of the gene-major grouped pass)."""
    rng = np.random.default_rng(seed)
    n_groups, cells = 1600, 4800
    m = sparse.random(genes, cells, density=0.3, format="csc", random_state=seed, data_rvs=lambda s: rng.geometric(0.3, s)).astype(np.uint32)
    labels = rng.permutation(np.repeat(np.arange(n_groups), 3)).astype(np.int16)
    return m, labels, n_groups, [(1599, 0), (7, 1536)]


@pytest.mark.parametrize("genes,acc_tiles", [(64, 1), (660, 2)])  # 1 600 x 660 (group, gene) entries pass the 2^20 of one accumulator tile
def test_many_groups_over_two_shards(sa, genes, acc_tiles):
    m, labels, n_groups, pairs = _many_groups(genes, 17)
    assert -(-n_groups * genes // (1 << 20)) == acc_tiles
    hg, hc = _handle(sa, m, "csr"), _handle(sa, m, "csc")
    exp = pc.as_arrays(*sa.sseq_de_pairs(hg, labels, pairs, n_groups=n_groups))
    assert hg.counter("de_pairs_passes") == 3  # totals + two tiles of groups
    pc.assert_same_bits(pc.as_arrays(*sa.sseq_de_pairs(hc, labels, pairs, n_groups=n_groups)), exp)
    mm, transposed = _multi(sa, m, "csc", 2)
    got = pc.as_arrays(*sa.sseq_de_pairs(mm, labels, pairs, n_groups=n_groups, transposed=transposed))
    pc.assert_same_bits(got, exp)
    assert [mm.counter("de_shard_allreduces", i) for i in range(2)] == [2 + acc_tiles] * 2  # totals, accumulator tiles, p-values
    mm.close()


# ---- 4. counters -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_the_exchange_steps_and_the_split_of_the_tests(sa, case, multis, backend):
    h = _handle(sa, case["mat"])
    mm, transposed = multis("csc", 3)
    for pairs in (case["pairs"], [pr for pr in case["pairs"] if pr != case["literal_pair"]], [case["literal_pair"]] * 2 + case["pairs"][:1]):
        n_lit = sum(pr == case["literal_pair"] for pr in pairs)
        sa.sseq_de_pairs_sharded(h, case["labels"], pairs, backend=backend, n_groups=case["n_groups"])  # unsharded: every test is its own
        whole = h.counter("de_shard_tests")
        assert whole > 0 and h.counter("de_shard_allreduces") == 0
        sa.sseq_de_pairs(mm, case["labels"], pairs, backend=backend, n_groups=case["n_groups"], transposed=transposed)
        per_shard = [mm.counter("de_shard_tests", i) for i in range(3)]
        assert sum(per_shard) == whole and min(per_shard) > 0, (per_shard, whole)
        steps = [mm.counter("de_shard_allreduces", i) for i in range(3)]
        # totals, accumulators (one tile), p-values; a literal pair adds §7g's 3 (totals, largest count, moment limbs) + 2 (group sums, p-values)
        assert steps == [3 + 5 * n_lit] * 3, (steps, n_lit)
        assert [mm.counter("de_pairs_literal", i) for i in range(3)] == [n_lit] * 3


# ---- 5. the host-hook transport ----------------------------------------------------------------------------------------------------------
def test_a_host_hook_with_a_world_of_one(sa, case, unsharded):
    calls = []

    def hook(ptr, count, dtype):
        calls.append((count, dtype))
        return 0

    h = _handle(sa, case["mat"])
    h.set_shard(0, 1, 0, case["cells"], hook)
    got = sa.sseq_de_pairs_sharded(h, case["labels"], case["pairs"], n_groups=case["n_groups"])
    pc.assert_same_bits(pc.as_arrays(*got), unsharded[pref.LOGSPACE][0])
    assert calls and {d for _, d in calls} == {1}
    entries = case["n_groups"] * case["genes"]
    assert (case["cells"], 1) in calls and (7 * (entries + entries % 2), 1) in calls and (case["genes"] * len(case["pairs"]), 1) in calls
    assert len(calls) == h.counter("de_shard_allreduces") == 3 + 5
    with pytest.raises(sa.ScanrsError) as e:  # the plain call keeps refusing it
        sa.sseq_de_pairs(h, case["labels"], case["pairs"], n_groups=case["n_groups"])
    assert e.value.code == 6 and "sharded" in str(e.value)
    # through the transposed view of a cells x genes CSR handle as well
    calls.clear()
    s = sparse.csr_matrix(case["mat"].T)
    s.sort_indices()
    ht = sa.AdaptiveMat.from_csmat(case["cells"], case["genes"], sa.CSR, s.indptr.astype(np.uint64), s.indices.astype(np.uint32), s.data.astype(np.uint32))
    ht.set_shard(0, 1, 0, case["cells"], hook)
    got = sa.sseq_de_pairs_sharded(ht.t(), case["labels"], case["pairs"], backend=pref.RATIO, n_groups=case["n_groups"])
    pc.assert_same_bits(pc.as_arrays(*got), unsharded[pref.RATIO][0])
    assert calls and {d for _, d in calls} == {1}
    # an unsharded handle: the collective call is the plain one
    plain = sa.sseq_de_pairs_sharded(_handle(sa, case["mat"], "csr"), case["labels"], case["pairs"], n_groups=case["n_groups"])
    pc.assert_same_bits(pc.as_arrays(*plain), unsharded[pref.LOGSPACE][0])


# ---- 6. degenerate cases and refusals -----------------------------------------------------------------------------------------------------
def test_a_shard_without_nonzeros(sa, case):
    """scanrs_plan_shards cuts by nonzeros: the last shard gets none when the last non-empty cell holds more than a fifth of them. Four
    cells of the fixture, one cell with every gene, then a tail of 30 empty cells, over 5 shards (most groups are made of empty cells
    here: several unions have a median total of 0 and take the literal route)."""
    genes = case["genes"]
    head = sparse.csc_matrix(case["mat"])[:, 20:24].toarray()
    full = np.arange(1, genes + 1, dtype=np.uint32).reshape(-1, 1) * 3
    dense = np.hstack([head, full, np.zeros((genes, 30), dtype=np.uint32)]).astype(np.uint32)
    m = sparse.csc_matrix(dense)
    m.sort_indices()
    cells = m.shape[1]
    bounds = sa.plan_shards(m.indptr.astype(np.uint64), 5)
    assert bounds[3] < bounds[4] < cells and m.indptr[bounds[4]] == m.nnz  # the last shard: cells, no nonzeros
    labels = np.random.default_rng(5).integers(-1, 4, cells).astype(np.int16)
    labels[-3:] = [0, 1, 3]
    pairs = [(0, 1), (2, 3), (3, 0), (1, 2)]
    h = _handle(sa, m)
    for backend in BACKENDS:
        exp = pc.as_arrays(*sa.sseq_de_pairs(h, labels, pairs, backend=backend, n_groups=4))
        for form in FORMS:
            mm, transposed = _multi(sa, m, form, 5)
            assert mm.shard_ranges()[-1][1] == bounds[4]
            pc.assert_same_bits(pc.as_arrays(*sa.sseq_de_pairs(mm, labels, pairs, backend=backend, n_groups=4, transposed=transposed)), exp)
            mm.close()


def test_refusals_and_cancellation(sa, case, unsharded, multis):
    m, labels, pairs, n = case["mat"], case["labels"], case["pairs"], case["n_groups"]
    # the genes sharded: a gene-major handle sharded over its rows, and a MultiMat created gene-major
    s = sparse.csr_matrix(m)
    s.sort_indices()
    ip, ix, vv = s.indptr.astype(np.uint64), s.indices.astype(np.uint32), s.data.astype(np.uint32)
    hg = sa.AdaptiveMat.from_csmat(case["genes"], case["cells"], sa.CSR, ip, ix, vv)
    hg.set_shard(0, 1, 0, case["genes"], lambda *a: 0)
    mg = sa.MultiMat(case["genes"], case["cells"], sa.CSR, ip, ix, vv, 2, devices=[0, 0])
    for call in (lambda: sa.sseq_de_pairs_sharded(hg, labels, pairs, n_groups=n), lambda: sa.sseq_de_pairs(mg, labels, pairs, n_groups=n),
                 lambda: sa.sseq_de_each_vs_control(mg, labels, n_groups=n)):
        with pytest.raises(sa.ScanrsError) as e:
            call()
        assert e.value.code == 6 and "cells" in str(e.value) and "sharded" in str(e.value)
    mg.close()
    mm, transposed = multis("csc", 3)
    lo, hi = mm.shard_ranges()[1][1:]
    for short in (labels[:-1], labels[lo:hi]):  # one short of the global count; the slice of one shard
        with pytest.raises(sa.ScanrsError):
            sa.sseq_de_pairs(mm, short, pairs, n_groups=n)
    # the argument checks run before the first exchange, on every shard alike: no shard is left waiting
    for bad, groups, word in (([(1, n)], n, "outside"), ([(2, 2)], n, "against itself"), ([(case["empty_group"], n)], n + 1, "no cell")):
        with pytest.raises(sa.ScanrsError) as e:
            sa.sseq_de_pairs(mm, labels, bad, n_groups=groups)
        assert e.value.code == 6 and word in str(e.value)
    # a cancelled snoop: SCANRS_ERR_CANCELLED from the MultiMat call, and the handle serves the next call
    sn = sa.AtomicSnoop()
    sn.cancel()
    with pytest.raises(sa.CancellationError) as e:
        sa.sseq_de_pairs(mm, labels, pairs, n_groups=n, snoop=sn, transposed=transposed)
    assert e.value.code == 3
    seen = sa.AtomicSnoop()
    got = sa.sseq_de_pairs(mm, labels, pairs, n_groups=n, snoop=seen, transposed=transposed)
    pc.assert_same_bits(pc.as_arrays(*got), unsharded[pref.LOGSPACE][0])
    assert not seen.is_cancelled() and seen.history == [0.0, 0.1, 0.6, 0.75, 0.9, 0.95, 1.0]
