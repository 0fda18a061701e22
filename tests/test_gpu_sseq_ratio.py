"""The Ratio backend of the exact NB test on the device (scan-rs_amd/csrc/sseq_ratio.inc) against the serial restatement of
nb_exact_test_ratio (tests/sseq_ratio_ref.py), and the shared-control mode of the matrix path."""
import ctypes
import os
import sys

import numpy as np
import pytest
from scipy import sparse

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import sseq_ratio_ref as rref  # noqa: E402
import sseq_ref as ref  # noqa: E402

FIELDS = ("sums_in", "sums_out", "p_values", "adjusted_p_values", "log2_fold_change", "normalized_mean_in", "normalized_mean_out")
PIN = (6, 3, 885.7432862994995, 2023.055530268548, 0.0029272959469517066, 27.024221110009037)  # dist.rs:420-429
NO_ASYM = 2 ** 62  # big_count: every test takes the exact branch


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


def _random_counts(genes, cells, density, seed):
    rng = np.random.default_rng(seed)
    m = sparse.random(genes, cells, density=density, format="csr", random_state=seed, data_rvs=lambda n: rng.geometric(0.3, n))
    return m.astype(np.uint32)


def _handle(sa, m, storage):
    g, c = m.shape
    s = sparse.csr_matrix(m) if storage == sa.CSR else sparse.csc_matrix(m)
    s.sort_indices()
    return sa.AdaptiveMat.from_csmat(g, c, storage, s.indptr.astype(np.uint64), s.indices.astype(np.uint32), s.data.astype(np.uint32))


def _one_gene(sa, mu, phi):
    return sa.SSeqParams(0, 1, np.zeros(0), np.array([mu]), np.array([1.0]), np.array([False]), np.array([phi]), 0.0, 0.0, np.array([phi]))


def _device_p(sa, case, backend):
    xa, xb, fa, fb, mu, phi = case
    return sa.sseq_de_from_sums([xa], [xb], fa, fb, _one_gene(sa, mu, phi), big_count=NO_ASYM, backend=backend).p_values[0]


def _bits(x):
    return np.float64(x).tobytes()


def _check_case(sa, case, got, expected=None):
    """The bound of the exact-test battery: 1e-9 relative to the serial restatement, else inside its tie bounds widened by
    1e-9. A case outside the Ratio partition (observed term 0, not finite or below 2^-970) must carry the device's LogSpace
    bits. Returns whether the case went through the ratio partition."""
    if rref.degenerate(case[0], case[1], case[2], case[3], case[5]):
        assert got == 1.0, case
        return False
    if not rref.in_ratio_partition(*case):
        assert _bits(got) == _bits(_device_p(sa, case, sa.NB_EXACT_LOGSPACE)), (case, got)
        return False
    e = rref.nb_exact_test_ratio(*case) if expected is None else expected
    assert np.isfinite(got), (case, got)
    if abs(got - e) > 1e-9 * e:
        lo, hi = rref.nb_exact_test_ratio_tie_bounds(*case)
        assert lo * (1 - 1e-9) <= got <= hi * (1 + 1e-9), (case, got, e, lo, hi)
    return True


# ---- 1. the battery ---------------------------------------------------------------------------------------------------------------
def _battery():
    cases = []
    rng = np.random.default_rng(17)  # the generator of test_exact_battery_matches_direct_gammaln
    for n in (1, 2, 10, 100, 2047, 2048, 2049, 4097, 10000, 100000, 1000000):
        for _ in range(3):
            xa = int(rng.integers(0, n + 1))
            fa, fb = rng.uniform(0.2, 3000, 2)
            cases.append((xa, n - xa, fa, fb, rng.uniform(0.01, 4), rng.uniform(0.005, 2)))
    cases.append(PIN)
    for fa, fb, phi in ((0.6, 0.9, 2.0), (0.9, 0.3, 1.5)):  # U-shaped: sf / phi below 1 on both sides
        for n in (5, 300, 5000):
            cases.append((n // 3, n - n // 3, fa, fb, 1.3, phi))
    cases += [(3, 400000, 40.0, 90000.0, 0.5, 0.3), (40, 800000, 40.0, 90000.0, 2.0, 0.1)]  # one condition against a shared control
    cases.append((250, 750, 40.0, 40.0, 1.0, 0.4))  # sf_a == sf_b: U[k] == U[n - k]
    return cases


def test_ratio_battery_matches_the_serial_restatement(sa):
    cases = _battery()
    assert len(cases) == 43
    through = 0
    for case in cases:
        got = _device_p(sa, case, sa.NB_EXACT_RATIO)
        through += _check_case(sa, case, got)
    assert through >= 30, through
    assert abs(_device_p(sa, PIN, sa.NB_EXACT_RATIO) - 0.03254) <= 1e-5
    assert rref.in_ratio_partition(*PIN)


# ---- 2. edges: chunk boundaries, the three places of the anchor, x_a around the anchor and at chunk ends ------------------------------
REGIMES = {"anchor_0": (0.5, 3.0, 1.0), "anchor_n": (3.0, 0.5, 1.0), "interior": (30.0, 50.0, 0.5)}  # (sf_a, sf_b, phi)


@pytest.mark.parametrize("regime", sorted(REGIMES))
@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
def test_ratio_edges(sa, n, regime):
    fa, fb, phi = REGIMES[regime]
    mu = 0.8
    anchor, u = rref.ratio_terms(n, fa, fb, phi)
    assert {"anchor_0": anchor == 0, "anchor_n": anchor == n, "interior": 0 < anchor < n}[regime]
    chunk = 2048  # SSEQ_CHUNK: the terms next to the anchor open a side's first chunk, the ones 2048 away close it
    xs = sorted({x for x in (0, n, anchor - 1, anchor, anchor + 1, anchor - chunk, anchor - chunk - 1, anchor + chunk, anchor + chunk + 1,
                             anchor - 2 * chunk, anchor + 2 * chunk) if 0 <= x <= n})
    xa = np.array(xs, dtype=np.uint64)
    params = sa.SSeqParams(0, len(xs), np.zeros(0), np.full(len(xs), mu), np.ones(len(xs)), np.zeros(len(xs), dtype=bool), np.full(len(xs), phi), 0.0,
                           0.0, np.full(len(xs), phi))
    got = sa.sseq_de_from_sums(xa, n - xa, fa, fb, params, big_count=NO_ASYM, backend=sa.NB_EXACT_RATIO).p_values
    log = sa.sseq_de_from_sums(xa, n - xa, fa, fb, params, big_count=NO_ASYM).p_values
    sum_all = np.add.accumulate(u)[-1]
    through = 0
    for i, x in enumerate(xs):
        case = (x, n - x, fa, fb, mu, phi)
        e = float(np.add.accumulate(np.where(u <= u[x], u, 0.0))[-1] / sum_all)  # dist.rs:205-214
        if _check_case(sa, case, got[i], e):
            through += 1
            # the two backends at n <= 10000: the step's tolerance (dist.rs:481)
            if abs(got[i] - log[i]) > 1e-9 * log[i]:
                lo, hi = rref.nb_exact_test_ratio_tie_bounds(*case)
                assert lo * (1 - 1e-9) <= log[i] <= hi * (1 + 1e-9), (case, got[i], log[i])
    assert through >= len(xs) - 2


# ---- 3. a test's result depends on its own inputs only --------------------------------------------------------------------------------
def test_ratio_result_does_not_depend_on_the_other_tests(sa):
    rng = np.random.default_rng(4)
    genes = 64
    xa, xb = rng.integers(0, 5000, genes), rng.integers(0, 50000, genes)
    mu, phi = rng.uniform(0.1, 3, genes), rng.uniform(0.05, 1, genes)
    params = sa.SSeqParams(0, genes, np.zeros(0), mu, np.ones(genes), np.zeros(genes, dtype=bool), phi, 0.0, 0.0, phi)
    allp = sa.sseq_de_from_sums(xa, xb, 300.0, 2000.0, params, big_count=NO_ASYM, backend=sa.NB_EXACT_RATIO).p_values
    logp = sa.sseq_de_from_sums(xa, xb, 300.0, 2000.0, params, big_count=NO_ASYM, backend=sa.NB_EXACT_LOGSPACE).p_values
    part = np.array([rref.in_ratio_partition(int(xa[g]), int(xb[g]), 300.0, 2000.0, mu[g], phi[g]) for g in range(genes)])
    assert part.sum() >= 8 and (~part).sum() >= 8  # both kinds share the launch
    for g in range(genes):
        case = (int(xa[g]), int(xb[g]), 300.0, 2000.0, mu[g], phi[g])
        assert _bits(_device_p(sa, case, sa.NB_EXACT_RATIO)) == _bits(allp[g]), g
        if not part[g]:
            assert _bits(allp[g]) == _bits(logp[g]), g
        _check_case(sa, case, allp[g])


# ---- 4. the matrix path ------------------------------------------------------------------------------------------------------------------
def _ref_de_from_sums_ratio(sums_a, sums_b, sf_a, sf_b, params, big_count):
    """diff_exp.rs:208-300 with NbExactBackend::Ratio; outside the ratio partition the log-space test, as the library falls back."""
    out = ref.de_from_sums(sums_a, sums_b, sf_a, sf_b, params, big_count)
    mu, phi, use = params["gene_means"], params["gene_phi"], params["use_genes"]
    p = out["p_values"].copy()
    for g in range(len(p)):
        a, b = int(sums_a[g]), int(sums_b[g])
        if use[g] and a > big_count and b > big_count:
            continue
        case = (a, b, sf_a, sf_b, mu[g], phi[g])
        if not rref.degenerate(a, b, sf_a, sf_b, phi[g]) and rref.in_ratio_partition(*case):
            p[g] = rref.nb_exact_test_ratio(*case)
    padj = p.copy()
    idx = np.flatnonzero(use)
    padj[idx] = ref.adjusted_pvalue_bh(p[idx])
    out["p_values"], out["adjusted_p_values"] = p, padj
    return out


def _assert_de(got, exp):
    for f in FIELDS:
        g, e = getattr(got, f), exp[f]
        if f.startswith("sums"):
            np.testing.assert_array_equal(g, e, err_msg=f)
        else:
            np.testing.assert_allclose(g, e, rtol=1e-9 if "p_values" in f else 1e-12, atol=0, err_msg=f)


@pytest.fixture(scope="module")
def pairwise(sa):
    m = _random_counts(400, 3000, 0.08, 21)
    m = m.multiply(40).astype(np.uint32).tocsr()  # large enough sums for the asymptotic branch
    a, b = np.arange(0, 1400), np.arange(1400, 3000)
    params = sa.compute_sseq_params(_handle(sa, m, sa.CSR))
    pref = ref.compute_sseq_params(m)
    sa_, sb_ = (np.asarray(m[:, s].sum(axis=1)).ravel() for s in (a, b))
    tested = np.flatnonzero(pref["use_genes"])
    big = int(np.median(np.minimum(sa_[tested], sb_[tested])))
    return m, a, b, params, pref, big


def test_ratio_pairwise_matches_the_restatement_and_from_sums(sa, pairwise):
    m, a, b, params, pref, big = pairwise
    h = _handle(sa, m, sa.CSC)
    got = sa.sseq_differential_expression(h, a, b, params, big_count=big, backend=sa.NB_EXACT_RATIO)
    log = sa.sseq_differential_expression(h, a, b, params, big_count=big)
    fa, fb = 0.0, 0.0
    for i in a:
        fa += pref["size_factors"][i]
    for i in b:
        fb += pref["size_factors"][i]
    sums_a, sums_b = (np.asarray(m[:, s].sum(axis=1), dtype=np.uint64).ravel() for s in (a, b))
    exp = _ref_de_from_sums_ratio(sums_a, sums_b, fa, fb, pref, big)
    asym = pref["use_genes"] & (sums_a > big) & (sums_b > big)
    assert asym.sum() > 20 and (~asym).sum() > 20
    _assert_de(got, exp)
    assert got.sums_in.tobytes() == log.sums_in.tobytes() and got.sums_out.tobytes() == log.sums_out.tobytes()
    assert got.p_values[asym].tobytes() == log.p_values[asym].tobytes()  # the asymptotic branch does not know the backend
    # the matrix path is the sums path (the reference's rtol = 0 test, diff_exp.rs:503-617)
    dfa, dfb = sum(params.size_factors[i] for i in a), sum(params.size_factors[i] for i in b)
    fs = sa.sseq_de_from_sums(got.sums_in, got.sums_out, dfa, dfb, params, big_count=big, backend=sa.NB_EXACT_RATIO)
    for f in FIELDS:
        assert getattr(fs, f).tobytes() == getattr(got, f).tobytes(), f


def test_ratio_one_vs_rest_matches_the_restatement(sa, pairwise):
    m, _, _, params, pref, big = pairwise
    labels = (np.arange(m.shape[1]) % 4).astype(np.int16) - 1  # -1 (in no group), 0, 1, 2
    got = sa.sseq_de_one_vs_rest(_handle(sa, m, sa.CSR), labels, params, big_count=big, n_groups=3, backend=sa.NB_EXACT_RATIO)
    log = sa.sseq_de_one_vs_rest(_handle(sa, m, sa.CSR), labels, params, big_count=big, n_groups=3)
    mc = sparse.csc_matrix(m)
    for j in range(3):
        ca, cb = np.flatnonzero(labels == j), np.flatnonzero((labels >= 0) & (labels != j))
        fa, fb = 0.0, 0.0
        for i in ca:
            fa += pref["size_factors"][i]
        for i in cb:
            fb += pref["size_factors"][i]
        sums_a, sums_b = (np.asarray(mc[:, s].sum(axis=1), dtype=np.uint64).ravel() for s in (ca, cb))
        _assert_de(got[j], _ref_de_from_sums_ratio(sums_a, sums_b, fa, fb, pref, big))
        assert got[j].sums_in.tobytes() == log[j].sums_in.tobytes() and got[j].sums_out.tobytes() == log[j].sums_out.tobytes()


# ---- 5. the shared control (mode 2) ----------------------------------------------------------------------------------------------------------
def test_shared_control_equals_the_pairwise_calls(sa):
    m = _random_counts(300, 2000, 0.06, 31)
    h = _handle(sa, m, sa.CSR)
    params = sa.compute_sseq_params(h)
    rng = np.random.default_rng(6)
    labels = rng.integers(-1, 6, 2000).astype(np.int16)
    labels[:700] = 0  # the control is the largest group
    for backend in (sa.NB_EXACT_LOGSPACE, sa.NB_EXACT_RATIO):
        got = sa.sseq_de_vs_control(h, labels, params, backend=backend)
        assert len(got) == 5
        for j in range(5):
            one = sa.sseq_differential_expression(h, np.flatnonzero(labels == j + 1), np.flatnonzero(labels == 0), params, backend=backend)
            for f in FIELDS:
                assert getattr(got[j], f).tobytes() == getattr(one, f).tobytes(), (backend, j, f)
    # another control: the other groups keep their order
    got = sa.sseq_de_vs_control(h, labels, params, control=3, backend=sa.NB_EXACT_RATIO)
    for j, grp in enumerate((0, 1, 2, 4, 5)):
        one = sa.sseq_differential_expression(h, np.flatnonzero(labels == grp), np.flatnonzero(labels == 3), params, backend=sa.NB_EXACT_RATIO)
        for f in FIELDS:
            assert getattr(got[j], f).tobytes() == getattr(one, f).tobytes(), (grp, f)
    with pytest.raises(sa.ScanrsError):
        sa.sseq_de_vs_control(h, np.zeros(2000, dtype=np.int16), params)  # mode 2 needs a second group
    with pytest.raises(sa.ScanrsError):
        sa.sseq_de_vs_control(h, labels, params, control=6)


def _raw_de(sa, h, labels, n_groups, mode, params, backend):
    """scanrs_sseq_de (backend None) or scanrs_sseq_de_backend through ctypes: the return code."""
    p_ = sa.sseq._p
    genes, cells = h.shape()
    lab = np.ascontiguousarray(labels, dtype=np.int16)
    mean, phi, use = sa.sseq._params_arrays(params, genes)
    sf = np.ascontiguousarray(params.size_factors, dtype=np.float64)
    t = max(n_groups, 1)
    si, so = np.zeros((genes, t), dtype=np.uint64), np.zeros((genes, t), dtype=np.uint64)
    out = [np.zeros((genes, t)) for _ in range(5)]
    head = (h._h, p_(lab), ctypes.c_uint32(n_groups), ctypes.c_int(mode), p_(sf), p_(mean), p_(phi), p_(use), ctypes.c_uint64(900))
    tail = (None, p_(si), p_(so)) + tuple(p_(o) for o in out)
    if backend is None:
        return sa._lib.scanrs_sseq_de(*head, *tail)
    return sa._lib.scanrs_sseq_de_backend(*head, ctypes.c_int(backend), *tail)


def test_old_entry_refuses_mode_2_and_bad_backends_raise(sa):
    m = _random_counts(40, 120, 0.2, 2)
    h = _handle(sa, m, sa.CSR)
    params = sa.compute_sseq_params(h)
    labels = (np.arange(120) % 3).astype(np.int16)
    assert _raw_de(sa, h, labels, 3, 2, params, None) == 6  # SCANRS_ERR_ARGUMENT
    assert _raw_de(sa, h, labels, 3, 1, params, None) == 0
    assert _raw_de(sa, h, labels, 3, 2, params, sa.NB_EXACT_RATIO) == 0
    assert _raw_de(sa, h, labels, 3, 0, params, 2) == 6
    assert _raw_de(sa, h, labels, 3, 3, params, sa.NB_EXACT_RATIO) == 6
    for call in (lambda: sa.sseq_de_one_vs_rest(h, labels, params, backend=2),
                 lambda: sa.sseq_de_vs_control(h, labels, params, backend=2),
                 lambda: sa.sseq_differential_expression(h, [0, 1], [2, 3], params, backend=2),
                 lambda: sa.sseq_de_from_sums([3], [4], 5.0, 10.0, _one_gene(sa, 1.0, 0.5), backend=2)):
        with pytest.raises(sa.ScanrsError):
            call()


# ---- 6. the default is LogSpace ----------------------------------------------------------------------------------------------------------------
def test_default_backend_is_logspace_bit_for_bit(sa, pairwise):
    m, a, b, params, _, big = pairwise
    h = _handle(sa, m, sa.CSR)
    labels = (np.arange(m.shape[1]) % 3).astype(np.int16)
    pairs = [
        ([sa.sseq_differential_expression(h, a, b, params, big_count=big)],
         [sa.sseq_differential_expression(h, a, b, params, big_count=big, backend=sa.NB_EXACT_LOGSPACE)]),
        (sa.sseq_de_one_vs_rest(h, labels, params), sa.sseq_de_one_vs_rest(h, labels, params, backend=sa.NB_EXACT_LOGSPACE)),
    ]
    d = pairs[0][0][0]
    pairs.append(([sa.sseq_de_from_sums(d.sums_in, d.sums_out, 700.0, 900.0, params)],
                  [sa.sseq_de_from_sums(d.sums_in, d.sums_out, 700.0, 900.0, params, backend=sa.NB_EXACT_LOGSPACE)]))
    for x, y in pairs:
        assert len(x) == len(y)
        for r, s in zip(x, y):
            for f in FIELDS:
                assert getattr(r, f).tobytes() == getattr(s, f).tobytes(), f


# ---- 7. progress and cancellation -----------------------------------------------------------------------------------------------------------------
def test_progress_and_cancel_with_ratio(sa):
    m = _random_counts(80, 300, 0.1, 3)
    h = _handle(sa, m, sa.CSR)
    params = sa.compute_sseq_params(h)
    labels = (np.arange(300) % 3).astype(np.int16)
    for f in (sa.sseq_de_one_vs_rest, sa.sseq_de_vs_control):
        sn = sa.AtomicSnoop()
        f(h, labels, params, snoop=sn, backend=sa.NB_EXACT_RATIO)
        assert sn.history == [0.0, 0.1, 0.6, 0.75, 0.9, 0.95, 1.0]
        sn = sa.AtomicSnoop()
        sn.cancel()
        with pytest.raises(sa.CancellationError) as e:
            f(h, labels, params, snoop=sn, backend=sa.NB_EXACT_RATIO)
        assert e.value.code == 3
