"""sSeq differential expression without a device: the CPU restatement (tests/sseq_ref.py) and the library's host entry
points (the special functions the kernels run) against the reference's own pinned values and against scipy."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(TESTS, "golden", "sseq_reference_tables.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ref():
    import sys

    if TESTS not in sys.path:
        sys.path.insert(0, TESTS)
    import sseq_ref

    return sseq_ref


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


def test_bh_pins(pins, ref, sa):
    t = pins["bh"]
    assert list(ref.adjusted_pvalue_bh(t["p"])) == t["expected"]
    assert list(sa.sseq.host_adjusted_pvalue_bh(t["p"])) == t["expected"]


def test_bh_nans_go_first_and_read_as_one(ref, sa):
    p = [0.5, float("nan"), 0.01, 0.2, float("nan")]
    np.testing.assert_array_equal(sa.sseq.host_adjusted_pvalue_bh(p), ref.adjusted_pvalue_bh(p))
    assert sa.sseq.host_adjusted_pvalue_bh(p)[1] == 1.0


def test_log_prob_all_pins(pins, ref, sa):
    t = pins["log_prob_all"]
    n = t["x_a"] + t["x_b"]
    for got in (ref.log_prob_all(n, t["sa"], t["sb"], t["mu"], 1 / t["phi"]), sa.sseq.host_log_prob_all(n, t["sa"], t["sb"], t["mu"], 1 / t["phi"])):
        np.testing.assert_allclose(got, t["expected"], rtol=0, atol=t["tol"])


def test_nb_exact_test_pin(pins, ref, sa):
    t = pins["nb_exact_test"]
    args = (t["x_a"], t["x_b"], t["size_factor_a"], t["size_factor_b"], t["mu"], t["phi"])
    assert abs(ref.nb_exact_test(*args) - t["expected"]) <= t["tol"]
    assert abs(sa.sseq.host_nb_exact_test(*args) - t["expected"]) <= t["tol"]


def test_nb_asymptotic_test_pin(pins, ref, sa):
    t = pins["nb_asymptotic_test"]
    args = (t["x_a"], t["x_b"], t["size_factor_a"], t["size_factor_b"], t["mu"], t["phi"])
    assert abs(ref.nb_asymptotic_test(*args) - t["expected"]) <= t["tol"]
    assert abs(sa.sseq.host_nb_asymptotic_test(*args) - t["expected"]) <= t["tol"]


def test_stat_pins(pins, ref):
    s = pins["stats"]["small"]
    v = s["v"]
    assert abs(ref.mean(v) - s["mean"]) <= s["tol"]
    assert abs(ref.var(v, 0.0) - s["var0"]) <= s["tol"]
    assert abs(ref.median(v) - s["median"]) <= s["tol"]
    assert abs(ref.percentile(v, 0.95) - s["percentile_0_95"]) <= s["tol"]
    big = pins["stats"]["large"]
    v = [big["v_head"]] + [big["v_tail_value"]] * big["v_tail_len"]
    assert abs(ref.mean(v) - big["mean"]) <= big["tol"]
    assert abs(ref.var(v, 0.0) - big["var0"]) <= big["tol"]
    assert abs(ref.median(v) - big["median"]) <= big["tol"]
    assert abs(ref.percentile(v, 95.0) - big["percentile_95"]) <= big["tol"]


def test_host_betainc_and_inverse_match_scipy(sa):
    from scipy.special import betainc, betaincinv

    grid = np.geomspace(1e-2, 1e6, 17)
    worst, worst_inv = 0.0, 0.0
    for a in grid:
        for b in grid:
            m = betaincinv(a, b, 0.5)
            worst_inv = max(worst_inv, abs(sa.sseq.host_betaincinv(a, b, 0.5) - m) / m)
            for q in (1e-6, 0.05, 0.5, 0.95):
                x = betaincinv(a, b, q)
                if not 0.0 < x < 1.0:
                    continue
                e = betainc(a, b, x)
                if e > 1e-280:
                    worst = max(worst, abs(sa.sseq.host_betainc(a, b, x) - e) / e)
    assert worst < 1e-8 and worst_inv < 1e-8, (worst, worst_inv)


def test_host_exact_test_matches_the_restatement(ref, sa):
    rng = np.random.default_rng(3)
    for _ in range(40):
        xa, xb = (int(v) for v in rng.integers(0, 400, 2))
        fa, fb = rng.uniform(0.5, 300, 2)
        mu, phi = rng.uniform(0.01, 5), rng.uniform(0.01, 3)
        e = ref.nb_exact_test(xa, xb, fa, fb, mu, phi)
        lo, hi = ref.nb_exact_test_tie_bounds(xa, xb, fa, fb, mu, phi) if xa + xb else (e, e)
        g = sa.sseq.host_nb_exact_test(xa, xb, fa, fb, mu, phi)
        assert abs(g - e) <= 1e-9 * e or lo * (1 - 1e-9) <= g <= hi * (1 + 1e-9), (xa, xb, g, e)


def test_exact_test_early_returns(sa):
    t = sa.sseq.host_nb_exact_test
    assert t(0, 0, 1.0, 1.0, 1.0, 1.0) == 1.0
    assert t(3, 4, 1.0, 1.0, 1.0, 0.0) == 1.0
    assert t(3, 4, 0.0, 1.0, 1.0, 1.0) == 1.0 and t(3, 4, 1.0, 0.0, 1.0, 1.0) == 1.0


def test_params_from_moments_matches_the_restatement(ref, sa):
    rng = np.random.default_rng(5)
    mean = rng.uniform(0.01, 3, 300)
    var = np.where(rng.uniform(size=300) < 0.1, 0.0, mean * rng.uniform(0.5, 4, 300))
    got = sa.sseq_params_from_moments(mean, var, 812.5, 500.0, 310.0, 0.995)
    exp = ref.params_from_moments(mean, var, 812.5, 500.0, 310.0, 0.995)
    np.testing.assert_array_equal(got.use_genes, exp["use_genes"])
    np.testing.assert_array_equal(got.gene_moment_phi, exp["gene_moment_phi"])
    assert got.zeta_hat == exp["zeta_hat"] and got.delta == exp["delta"]
    np.testing.assert_array_equal(got.gene_phi, exp["gene_phi"])
    z = sa.sseq_params_from_moments(mean, np.zeros(300), 812.5, 500.0, 310.0, 0.995)
    assert z.zeta_hat == 0.0 and z.delta == 0.0 and not z.use_genes.any() and (z.gene_phi == 0).all()


def test_de_table_layout_and_clustering_labels(sa):
    n = 4
    res = [sa.DiffExpResult(*([np.arange(n) + 10 * j] * 5), np.arange(n) + 10 * j + 1, np.arange(n) + 10 * j + 2, np.arange(n) + 10 * j + 3,
                            np.arange(n) + 10 * j + 4, np.arange(n) + 10 * j + 5) for j in range(3)]
    t = sa.diff_exp_table(res)
    assert t.shape == (n, 9)
    for j, r in enumerate(res):
        np.testing.assert_array_equal(t[:, 3 * j], r.normalized_mean_in)
        np.testing.assert_array_equal(t[:, 3 * j + 1], r.log2_fold_change)
        np.testing.assert_array_equal(t[:, 3 * j + 2], r.adjusted_p_values)
    np.testing.assert_array_equal(sa.labels_from_clustering(np.array([1, 3, 0, 2], dtype=np.int16)), [0, 2, -1, 1])
