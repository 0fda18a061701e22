"""sum_axis / mean_var_axis of a log-normalized map on the device, every route, against the exact moments of tests/moments_ref.py.

The contract, for every slice and without an absolute term: |sum - S1| <= 1e-12 S1, the same for the mean,
|var - var_ref| <= 1e-10 S2/m, and a slice without nonzeros gives exactly 0 and 0. It binds the fixed-point route
(col_moments_kernel, option "col_moments" = 2) wherever scanrs_host_col_moments_plan accepts, and the ordinary pass (option 0,
and every map the plan refuses). The adversarial cases are those on which one quantum for the whole matrix, chosen from the
largest possible value alone, loses the slices that hold small values only (tests/test_moments_cpu.py shows it by emulation)."""
import os
import sys
import threading

import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import moments_ref as mr  # noqa: E402

CASES = sorted(mr.grid_cases())


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


def _triplet(case, cell_major):
    """The case's arrays as they are (one vector per cell) or regrouped by gene."""
    if cell_major:
        return case.indptr, case.indices, case.values
    m = sparse.csr_matrix((case.values, case.indices.astype(np.int64), case.indptr.astype(np.int64)), shape=(case.n_outer, case.n_inner)).tocsc()
    m.sort_indices()
    return m.indptr.astype(np.uint64), m.indices.astype(np.uint32), m.data.astype(np.uint32)


def _handle(sa, case, storage, axis, mode):
    """A handle whose `axis` runs over the case's cells (mean_var_axis(axis) sums over them), both copies built, the map composed."""
    cells_are_rows = axis == 0
    rows, cols = (case.n_outer, case.n_inner) if cells_are_rows else (case.n_inner, case.n_outer)
    cell_major = (storage == sa.CSR) == cells_are_rows
    g = sa.AdaptiveMat.from_csmat(rows, cols, storage, *_triplet(case, cell_major))
    g.set_option("col_moments", mode)
    g.dot(np.ones((cols, 1)))
    g.rdot(np.ones((1, rows)))  # both copies exist
    for l in case.links:
        if isinstance(l, np.ndarray):
            g.compose_scale_axis(axis, l)
        else:
            g.apply(int(l))
    return g


def _routes(prof):
    return {k for k in ("col_moments", "col_sums") if k in prof}


def _measure(sa, case, storage, axis, mode):
    g = _handle(sa, case, storage, axis, mode)
    g.profile_enable(True)
    g.profile_reset()
    mean, var = g.mean_var_axis(axis)
    total = g.sum_axis(axis)
    mean_t, var_t = g.t().mean_var_axis(1 - axis)
    routes = _routes(g.profile_get())
    g.profile_enable(False)
    if routes:  # integer accumulation: the same bits on every call
        again, again_sum = g.mean_var_axis(axis), g.sum_axis(axis)
        assert np.array_equal(again[0], mean) and np.array_equal(again[1], var) and np.array_equal(again_sum, total)
    return (total, mean, var), (mean_t, var_t), routes


@pytest.mark.parametrize("name", CASES)
def test_every_route_meets_the_contract(sa, name):
    """Both storages, both axes, the transposed view, sum_axis (sums only) beside mean_var_axis, "col_moments" 2 and 0.
    On the parent of scanrs_host_col_moments_plan the option-2 half of the adversarial cases failed; error / bound on the device:
    see the table in DESIGN.md (col_moments_kernel)."""
    case = mr.grid_cases()[name]
    worst = {}
    for storage in (sa.CSR, sa.CSC):
        for axis in (0, 1):
            for mode in (2, 0):
                (total, mean, var), (mean_t, var_t), routes = _measure(sa, case, storage, axis, mode)
                if mode == 0:
                    assert not routes
                elif not case.adversarial:
                    assert routes == {"col_moments", "col_sums"}, "a benign case must stay on the fixed-point route"
                else:
                    assert routes in (set(), {"col_moments", "col_sums"}, {"col_sums"})  # (the sums alone tolerate a wider spread)
                r = np.maximum(mr.contract_ratios(total, mean, var, case.ref), mr.contract_ratios(None, mean_t, var_t, case.ref)).tolist()
                key = (mode, "fixed" if "col_moments" in routes else "ordinary")
                worst[key] = np.maximum(worst.get(key, 0.0), r)
                print(name, "storage", storage, "axis", axis, "col_moments", mode, sorted(routes), "error / bound (sum, mean, var):", r)
    print(name, {k: v.tolist() for k, v in worst.items()})
    for key, r in worst.items():
        assert np.all(r <= 1.0), (name, key, r.tolist())


def _normalized_products(sa, case, storage, mode, panel, left):
    genes, cells = case.n_inner, case.n_outer
    g = sa.AdaptiveMat.from_csmat(genes, cells, storage, *_triplet(case, storage == sa.CSC))
    g.set_option("col_moments", mode)
    g.dot(np.ones((cells, 1)))
    g.rdot(np.ones((1, genes)))
    g.profile_enable(True)
    g.profile_reset()
    n = sa.normalize(g, sa.Normalization.CellRanger)
    routes = _routes(g.profile_get())
    g.profile_enable(False)
    return n.dot(panel), n.rdot(left), routes


def test_normalize_carries_the_moments_into_the_products(sa):
    """normalize(CellRanger) of the raw profile (log2(1 + count / total), then every gene centred and scaled by its standard
    deviation): A P and L A against the same products from the exact moments, |difference| <= 1e-9 (|A| |P|) elementwise, for
    "col_moments" 2 and 0 in both storages. A variance that is off by 1e-7 of S2/m moves a gene's row of A P by as much."""
    case = mr.grid_cases()["raw_profile"]
    genes, cells, ref = case.n_inner, case.n_outer, case.ref
    rng = np.random.default_rng(5)
    panel, left = rng.standard_normal((cells, 3)), rng.standard_normal((2, genes))
    f = np.array([float(t) for t in mr.exact_terms(*case.args())])
    dense = np.zeros((genes, cells))
    dense[case.indices.astype(np.int64), mr._cell_of(case.indptr)] = f
    mean = np.array([float(x) for x in ref["mean"]])
    sd = np.array([float(mr.MP.sqrt(v)) for v in ref["var"]])
    assert np.all(sd > 0)
    a = (dense - mean[:, None]) / sd[:, None]
    want_dot, bound_dot = a @ panel, 1e-9 * (np.abs(a) @ np.abs(panel))
    want_rdot, bound_rdot = left @ a, 1e-9 * (np.abs(left) @ np.abs(a))
    bad = []
    for storage in (sa.CSC, sa.CSR):
        for mode in (2, 0):
            got_dot, got_rdot, routes = _normalized_products(sa, case, storage, mode, panel, left)
            assert mode == 2 or not routes
            r = (float(np.max(np.abs(got_dot - want_dot) / bound_dot)), float(np.max(np.abs(got_rdot - want_rdot) / bound_rdot)))
            print("raw_profile normalize: storage", storage, "col_moments", mode, sorted(routes), "error / bound (A P, L A):", r)
            if max(r) > 1.0:
                bad.append((storage, mode, r))
    assert not bad, bad


@pytest.mark.parametrize("name", ["two_links_two_maxima", "benign_wide"])
def test_sharded_contraction(sa, name):
    """The cells cut over two shards on one device: every rank plans from its own cells and adds its own sums, the all-reduced
    result is held to the same contract; the benign case stays on the fixed-point route on every shard."""
    case = mr.grid_cases()[name]
    for mode in (2, 0):
        mm = sa.MultiMat(case.n_inner, case.n_outer, sa.CSC, case.indptr, case.indices, case.values, 2, devices=[0, 0])
        try:
            mm.set_option("col_moments", mode)
            for l in case.links:
                if isinstance(l, np.ndarray):
                    mm.compose_scale_axis(1, l)
                else:
                    for i in range(mm.n_shards):
                        mm._with_shard(i, lambda b: b.apply(int(l)))
            mm.profile_enable(True)
            out, err = [None] * mm.n_shards, [None] * mm.n_shards

            def work(i):
                try:
                    out[i] = mm._with_shard(i, lambda b: (b.mean_var_axis(1), b.sum_axis(1)))
                except BaseException as e:  # noqa: BLE001
                    err[i] = e

            threads = [threading.Thread(target=work, args=(i,)) for i in range(mm.n_shards)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            assert err == [None] * mm.n_shards, err
            for i in range(mm.n_shards):
                routes = _routes(mm.profile_get(i))
                if mode == 0:
                    assert not routes
                elif not case.adversarial:
                    assert routes == {"col_moments", "col_sums"}
                (mean, var), total = out[i]
                r = mr.contract_ratios(total, mean, var, case.ref)
                print(name, "shard", i, "col_moments", mode, sorted(routes), "error / bound (sum, mean, var):", r)
                assert max(r) <= 1.0, (name, i, mode, r)
            assert np.array_equal(out[0][0][0], out[1][0][0]) and np.array_equal(out[0][0][1], out[1][0][1])
        finally:
            mm.close()


def test_routing(sa):
    """What must stay on the fixed-point route under "col_moments" = 2 and what must never take it."""
    from scanrs_amd.synth import synth_counts, synth_counts_fast

    for m in (synth_counts(3000, 700, 0.05, 5), synth_counts_fast(3000, 700, 0.05, 5, gene_shape=0.1, shared_profile=1.0)):
        cells, genes = m.shape
        t = sparse.csr_matrix(m.T)  # genes x cells, gene-major
        t.sort_indices()
        for storage, trip in ((sa.CSC, m), (sa.CSR, t)):
            g = sa.AdaptiveMat.from_csmat(genes, cells, storage, trip.indptr.astype(np.uint64), trip.indices.astype(np.uint32), trip.data.astype(np.uint32))
            g.set_option("col_moments", 2)
            g.dot(np.ones((cells, 1)))
            g.rdot(np.ones((1, genes)))
            g.profile_enable(True)
            g.profile_reset()
            sa.normalize(g, sa.Normalization.CellRanger)
            assert "col_moments" in g.profile_get(), ("normalize(CellRanger) left the fixed-point route", storage)
            g.profile_enable(False)
    # refused before and now: a factor on the other axis, a negative factor, a map without a logarithm; plus a non-finite factor
    rng = np.random.default_rng(29)
    dense = np.zeros((300, 9000), dtype=np.uint32)
    mask = rng.random(dense.shape) < 0.02
    dense[mask] = rng.integers(1, 6, size=int(mask.sum()))
    inf = np.ones(9000)
    inf[77] = np.inf
    for make in (lambda g: g.compose_scale_axis(0, np.arange(300) % 7 + 0.5).apply(sa.FN_LOG2_1P),
                 lambda g: g.compose_scale_axis(1, -(np.arange(9000) % 2) * 0.5 + 0.4).apply(sa.FN_LOG2_1P),
                 lambda g: g.compose_scale_axis(1, np.arange(9000) + 1.0),
                 lambda g: g.compose_scale_axis(1, inf).apply(sa.FN_LN_1P)):
        out = []
        for mode in (2, 0):
            g = sa.AdaptiveMat.from_dense(dense, sa.CSR)
            g.set_option("col_moments", mode)
            g.dot(np.ones((9000, 1)))
            g.rdot(np.ones((1, 300)))
            make(g)
            g.profile_enable(True)
            g.profile_reset()
            out.append(g.mean_var_axis(1) + (g.sum_axis(1),))
            assert not _routes(g.profile_get())
            g.profile_enable(False)
        for a, b in zip(*out):
            assert np.array_equal(a, b, equal_nan=True)
    # a zero factor beside positive ones does not refuse: its terms are exactly 0
    f = 0.5 + rng.random(9000)
    f[::3] = 0.0
    g = sa.AdaptiveMat.from_dense(dense, sa.CSR)
    g.set_option("col_moments", 2)
    g.dot(np.ones((9000, 1)))
    g.rdot(np.ones((1, 300)))
    g.compose_scale_axis(1, f).apply(sa.FN_LOG10_1P)
    g.profile_enable(True)
    g.profile_reset()
    mean, var = g.mean_var_axis(1)
    assert "col_moments" in g.profile_get()
    g.profile_enable(False)
    ip = np.concatenate(([0], np.cumsum((dense.T != 0).sum(axis=1)))).astype(np.uint64)
    gi = np.nonzero(dense.T)[1]
    ref = mr.exact_moments(ip, gi, dense.T[dense.T != 0], [f, mr.LOG10_1P], 9000, 300)
    r = mr.contract_ratios(None, mean, var, ref)
    assert max(r) <= 1.0, r
