"""svd_bk's reused projection T' = H C on the device against the model and the bounds of tests/bk_reuse_ref.py.

Every view of R.VIEWS runs with the factorizations on the device and on the host ("device_factor" 1 / 0) at its own "reuse_cmax",
at 1e-300 (every column recomputed directly: the control) and at the default 1e5; two cases also as CSR and through g.t(), one as a
two-shard MultiMat whose T side is sharded. A run first proves its branch from the "bk_*" counters — branch, flagged columns,
direct columns, last_direct and early projections equal to the model's, the bound used above every coefficient that took the dense
route and at most 100 x reuse_cmax — and then holds B1 (projection residual in long double), B2 / B3 (orthonormality of the two
factors) and B4 (singular values between the oracle's and the exact ones). At the default bound a branch-1 run may flag the columns
whose coefficient maximum lies within a factor 2 of 1e5 differently from the model (fits_tall, deep_8_iterations, b100_default and
the transposed views); everywhere else the counts are equal. With the guard taken away (reuse_cmax 1e300) the two TEETH cases must
leave B1's bound for L = 1e5 by more than a factor 100.

Measured on the MI355X, one run (ratio to the bound; dev = device path, host = "device_factor" 0; branch and counts at the view's own
reuse_cmax, "direct" = bk_direct_columns):
  view                   own setting                  dev: B1    B2    B3    B4-    host: B1    B2    B3    B4-
  benign_none            branch 0,   0 flagged,  24 direct   0.059 0.001 0.072 1e-08 (retries 0)   0.057 0.001 0.072 1e-07
  fits_wide_view         branch 1,  16 flagged,  32 direct   0.146 0.015 0.044 1e-07 (retries 0)   0.112 0.016 0.040 2e-07
  fits_tall              branch 1,  24 flagged,  40 direct   0.101 0.001 0.059 7e-04 (retries 0)   0.095 0.001 0.088 1e-03
  deep_8_iterations      branch 1,  68 flagged,  84 direct   0.109 0.001 0.058 5e-03 (retries 0)   0.109 0.001 0.052 5e-02
  wide_pass              branch 4, 104 flagged, 156 direct   0.084 0.001 0.049 6e-02 (retries 0)   0.083 0.001 0.065 4e-02
  b104_raised_top        branch 2,   1 flagged, 104 direct   0.035 0.001 0.026 1e-10 (retries 0)   0.045 0.001 0.026 1e-10
  b100_raised_need       branch 3, 101 flagged, 104 direct   0.037 0.001 0.013 9e-11 (retries 0)   0.049 0.002 0.026 8e-11
  b100_default           branch 1,   1 flagged, 101 direct   0.041 0.001 0.012 6e-08 (retries 0)   0.044 0.002 0.071 1e-07
  two_iterations         branch 0,   0 flagged,  16 direct   0.178 0.000 0.046 0e+00 (retries 0)   0.168 0.001 0.023 0e+00
  three_iterations       branch 0,   0 flagged,  16 direct   0.163 0.001 0.076 3e-10 (retries 0)   0.165 0.001 0.114 6e-09
  odd_block              branch 0,   0 flagged,   0 direct   0.148 0.001 0.044 4e-04 (retries 0)   0.148 0.001 0.044 2e-04
  cellranger             branch 0,   0 flagged,  16 direct   0.083 0.001 0.118 9e-08 (retries 0)   0.103 0.001 0.088 9e-08
  fits_wide_view.t()     branch 1,  16 flagged,  32 direct   0.116 0.004 0.118 2e-07 (retries 0)   0.117 0.004 0.059 1e-07
  fits_tall.t()          branch 1,  25 flagged,  41 direct   0.125 0.001 0.042 1e-05 (retries 0)   0.126 0.002 0.042 2e-04
  fits_wide_view as two column shards: B1 0.098, B2 0.009, B3 0.047, B4- 1e-07, the same counters on both shards, retries 0.
  Without the guard: deep_8_iterations leaves B1 at L = 1e5 by a factor 9.3e8, wide_pass by 1.2e5.
B1-B3 are the worst ratios over the settings of the view (the all-direct control, L = 1, gives the largest B1; at L = 1e5 the
worst is 0.05), B4- the worst of the lower bracket; the upper one (s_i <= sigma_i (1 + 1e-12)) held everywhere. Every branch 1-4,
the early projections at 3, 5 and 8 iterations, the sharded T side and both orientations ran on the device path (retries 0); no
branch-1 run used the factor-2 allowance. The file's 72 tests take 9 s.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bk_reuse_ref as R  # noqa: E402
import scanrs_oracle as so  # noqa: E402

COUNTERS = ("bk_q", "bk_b", "bk_coef_valid", "bk_flagged_older", "bk_limit_branch", "bk_limit_bits", "bk_direct_columns", "bk_last_direct",
            "bk_full_direct", "bk_early_projections", "bk_cmax_dense_bits", "bk_host_retries")
# the views whose device-side factorizations converge within the queued passes on the MI355X: their "device_factor" 1 runs are served
# by the device bookkeeping (bk_host_retries == 0). Between them: every branch 1-4, early projections at 3, 5 and 8 iterations, both
# orientations.
DEVICE_PATH = {name for name in R.CASES}


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gfx950 device required for -m gpu tests (no CPU fallback exists)")
    return scanrs_amd


def _f64(bits):
    return float(np.array([bits], dtype=np.uint64).view(np.float64)[0])


def _handle(sa, p, storage):
    g = sa.AdaptiveMat.from_dense(p.counts, storage)
    if p.case.normalized:
        g = sa.normalize(g, sa.Normalization.CellRanger)
    return (g.t(), g) if p.transposed else (g, g)  # (the view, the handle it was taken from: kept alive beside it)


def _run(sa, p, storage, cmax, dev):
    g, _base = _handle(sa, p, storage)
    g.set_option("device_factor", dev)
    if cmax is not None:
        g.set_option("reuse_cmax", cmax)
    u, s, v = sa.BkSvd(p.case.mult, p.case.n_iter).run_pca(g, p.case.k, omega=p.omega)
    return u, s, v, {key: g.counter(key) for key in COUNTERS}


def _check_counters(p, cmax, c, tag):
    """The branch the run took, from its counters, against the model's."""
    r = p.model(cmax)
    even = r.b % 2 == 0
    assert (c["bk_q"], c["bk_b"]) == (r.q, r.b) and c["bk_coef_valid"] == 1, (tag, c)
    assert c["bk_limit_branch"] == r.branch, (tag, c, r.branch)
    if r.branch == 1 and cmax == R.DEFAULT_CMAX and c["bk_flagged_older"] != r.flagged_older:
        lo, hi = R.flagged_range(p, cmax)  # no gap was asked for at the default: the columns within a factor 2 of it may go either way
        assert lo <= c["bk_flagged_older"] <= hi, (tag, c, lo, hi)
        print(f"{tag}: flagged {c['bk_flagged_older']} (model {r.flagged_older}, allowed {lo}..{hi})")
    else:
        assert c["bk_flagged_older"] == r.flagged_older, (tag, c, r.flagged_older)
        assert c["bk_direct_columns"] == len(r.direct), (tag, c, len(r.direct))
    assert c["bk_last_direct"] == int(r.last_direct) and c["bk_full_direct"] == int(r.full_direct) == int(not even), (tag, c)
    assert c["bk_early_projections"] == (max(p.case.n_iter - 2, 0) if even else 0), (tag, c)
    limit, dense = _f64(c["bk_limit_bits"]), _f64(c["bk_cmax_dense_bits"])
    assert limit <= 100.0 * cmax and limit >= cmax, (tag, limit)
    if even:
        assert dense < limit, (tag, dense, limit)
    if r.branch in (0, 1, 4):
        assert limit == cmax, (tag, limit)
    else:
        assert abs(limit - r.limit) <= 1e-6 * r.limit, (tag, limit, r.limit)  # a coefficient below 1e7: reproducible far beyond this
    return R.used_limit(limit, cmax == R.ALL_DIRECT or r.full_direct), r


def _check_bounds(p, q, L, u, s, v, tag):
    ra = R.ratios(p.dense_f, q, L, u, s, v, p.sigma, p.s_oracle)
    print(f"{tag}: L {L:.3g} " + " ".join(f"{k} {x:.3g}" for k, x in ra.items()))
    assert ra["self"] < 2.0 ** -8, (tag, ra)
    assert ra["b1"] <= 1.0, (tag, "B1 projection", ra)
    assert ra["b2"] < 1.0, (tag, "B2 Q-side factor", ra)
    assert ra["b3"] <= 1.0, (tag, "B3 T-side factor", ra)
    assert ra["b4_upper"] <= 1.0 and ra["b4_lower"] <= 1.0, (tag, "B4 subspace", ra)
    return ra


def _grid():
    out = []
    for name, tr in R.VIEWS:
        for storage in ((so.CSC, so.CSR) if name in R.BOTH_STORAGES and not tr else (so.CSC,)):
            for which in ("own", "direct", "default"):
                if which == "default" and R.CASES[name].target is None:
                    continue  # its own bound is the default
                for dev in (1, 0):
                    out.append(pytest.param(name, tr, storage, which, dev, id=f"{name}{'-t' if tr else ''}-{'csr' if storage == so.CSR else 'csc'}-{which}-{'dev' if dev else 'host'}"))
    return out


def _cmax(p, which):
    return {"own": p.cmax, "direct": R.ALL_DIRECT, "default": R.DEFAULT_CMAX}[which]


@pytest.mark.parametrize("name,transposed,storage,which,dev", _grid())
def test_reused_projection(sa, name, transposed, storage, which, dev):
    p = R.prepared(name, transposed)
    cmax = _cmax(p, which)
    # "own" at the default leaves the option alone: the library's default is part of what is tested
    u, s, v, c = _run(sa, p, storage, None if (which == "own" and cmax == R.DEFAULT_CMAX) else cmax, dev)
    tag = f"{name} t={int(transposed)} storage={storage} {which} dev={dev} retries={c['bk_host_retries']}"
    if dev == 0:
        assert c["bk_host_retries"] == 0, tag
    elif name in DEVICE_PATH:
        assert c["bk_host_retries"] == 0, (tag, "the device bookkeeping did not serve this run")
    L, r = _check_counters(p, cmax, c, tag)
    print(f"{tag}: branch {c['bk_limit_branch']} flagged {c['bk_flagged_older']} direct {c['bk_direct_columns']} limit {_f64(c['bk_limit_bits']):.4g}")
    _check_bounds(p, r.q, L, u, s, v, tag)


@pytest.mark.parametrize("which", ["own", "direct"])
def test_sharded_t_side(sa, which):
    """fits_wide_view (300 x 700: the T side is the columns) as two column shards on device 0: every shard takes the same decisions
    (the flagged set is a function of the coefficients alone), the assembled factors keep the bounds."""
    import scipy.sparse as sp

    p = R.prepared("fits_wide_view")
    cmax = _cmax(p, which)
    m = sp.csc_matrix(p.counts)
    mm = sa.MultiMat(p.counts.shape[0], p.counts.shape[1], sa.CSC, m.indptr, m.indices, m.data, 2, devices=[0, 0])
    if which != "own":
        mm.set_option("reuse_cmax", cmax)
    u, s, v = mm.run_pca_bk(p.case.k, p.case.mult, p.case.n_iter, omega=p.omega)
    cs = [{key: mm.counter(key, shard) for key in COUNTERS} for shard in range(2)]
    assert cs[0] == cs[1], cs
    tag = f"fits_wide_view two shards {which} retries={cs[0]['bk_host_retries']}"
    assert cs[0]["bk_host_retries"] == 0, tag
    L, r = _check_counters(p, cmax, cs[0], tag)
    _check_bounds(p, r.q, L, u, s, v, tag)


@pytest.mark.parametrize("name", R.TEETH)
def test_without_the_guard_the_projection_is_wrong(sa, name):
    """B5: reuse_cmax 1e300 flags nothing, every older column goes through H C with coefficients to 1e15 (1e12): the residual leaves
    B1's bound for L = 1e5 by more than a factor 100 — the cases above would notice a guard that lets such a column through."""
    p = R.prepared(name)
    u, s, v, c = _run(sa, p, so.CSC, R.NO_GUARD, 1)
    assert c["bk_flagged_older"] == 0 and c["bk_limit_branch"] == 0 and c["bk_direct_columns"] == c["bk_b"] and c["bk_last_direct"] == 1, c
    assert _f64(c["bk_cmax_dense_bits"]) > 1e9, c
    ratio, _ = R.b1_ratio(p.dense_f, c["bk_q"], 1e5, u, s, v)
    print(f"{name} without the guard (retries {c['bk_host_retries']}): B1 ratio at L = 1e5 {ratio:.3g}")
    assert ratio > 100.0
