"""The Ratio backend of the exact NB test without a device: the library's host restatement of nb_exact_test_ratio
(diff-exp/src/dist.rs:116-215) against the pure-Python loop of tests/sseq_ratio_ref.py, bit for bit; the ratio step against
the log-space terms; the reference's pin; the new symbols."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import sseq_ratio_ref as rref  # noqa: E402

PIN = (6, 3, 885.7432862994995, 2023.055530268548, 0.0029272959469517066, 27.024221110009037)  # dist.rs:420-429
NEW_SYMBOLS = ("scanrs_sseq_de_backend", "scanrs_sseq_de_from_sums_backend", "scanrs_host_nb_exact_test_ratio", "scanrs_host_nb_exact_ratio_step")
GUARDS = [(0, 0, 1.5, 2.5, 1.0, 0.3), (4, 7, 1.5, 2.5, 1.0, 0.0), (4, 7, 0.0, 2.5, 1.0, 0.3), (4, 7, 1.5, 0.0, 1.0, 0.3)]
# the observed term of these underflows to 0.0: the fallback to the log-space test (dist.rs:199-203)
UNDERFLOW = [(0, 5000, 3000.0, 0.2, 1.0, 0.005), (5000, 0, 0.2, 3000.0, 0.7, 0.005), (10, 4000, 2500.0, 1.0, 2.0, 0.01)]


def _battery():
    cases = [PIN]
    for fa, fb, phi in ((0.6, 0.9, 2.0), (0.9, 0.3, 1.5)):  # U-shaped: sf_a / phi and sf_b / phi below 1
        for n in (5, 300, 5000):
            for xa in sorted({0, 1, n // 3, n - 1, n}):
                cases.append((xa, n - xa, fa, fb, 1.3, phi))
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 10, 100, 999, 2049, 5000):
        for _ in range(4):
            xa = int(rng.integers(0, n + 1))
            fa, fb = rng.uniform(0.2, 3000, 2)
            cases.append((xa, n - xa, float(fa), float(fb), float(rng.uniform(0.01, 4)), float(rng.uniform(0.005, 2))))
    for n in (7, 500):  # sf_a == sf_b: the terms are symmetric about n / 2
        cases.append((n // 4, n - n // 4, 40.0, 40.0, 1.0, 0.4))
    return cases


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


def test_guards_return_exactly_one(sa):
    for c in GUARDS:
        assert sa.host_nb_exact_test_ratio(*c) == 1.0
        assert rref.nb_exact_test_ratio_loop(*c) == 1.0 and rref.nb_exact_test_ratio(*c) == 1.0


def test_host_ratio_equals_the_python_loop_bit_for_bit(sa):
    n_real = 0
    for c in _battery():
        got = sa.host_nb_exact_test_ratio(*c)
        o = rref.u_obs(*c)
        assert np.isfinite(o), c
        if o == 0.0:  # a random case whose observed term underflowed: the host's own log-space test (the loop's is scipy's)
            assert got == sa.sseq.host_nb_exact_test(*c), c
            continue
        loop = rref.nb_exact_test_ratio_loop(*c)
        assert got == loop, (c, got, loop)
        assert rref.nb_exact_test_ratio(*c) == loop, c  # the accumulate form used by the GPU battery is the same loop
        assert 0.0 <= got <= 1.0 + 1e-15
        n_real += 1
    assert n_real >= 60


def test_underflowed_observed_term_falls_back_to_the_host_logspace_test(sa):
    for c in UNDERFLOW:
        assert rref.u_obs(*c) == 0.0, c
        assert sa.host_nb_exact_test_ratio(*c) == sa.sseq.host_nb_exact_test(*c), c


def test_ratio_step_matches_consecutive_logspace_terms(sa):
    """dist.rs:459-493, the reference's grid and tolerance."""
    mu = 5.0
    for s_a in (0.6, 1.2, 2.0, 3.0):
        for s_b in (0.6, 1.2, 2.0, 3.0):
            for phi in (0.05, 0.3, 1.0, 2.0):
                for n in (10, 50, 200):
                    r = 1.0 / phi
                    lp = sa.sseq.host_log_prob_all(n, s_a, s_b, mu, r)
                    assert len(lp) == n + 1
                    for k in range(n):
                        step = sa.host_nb_exact_ratio_step(float(k), float(n), s_a * r, s_b * r)
                        expected = np.exp(lp[k + 1] - lp[k])
                        assert abs(step - expected) <= 1e-10 + 1e-9 * abs(expected), (s_a, s_b, phi, n, k, step, expected)
                        assert step == rref.ratio_step(float(k), float(n), s_a * r, s_b * r)


def test_reference_pin_through_ratio(sa):
    assert abs(sa.host_nb_exact_test_ratio(*PIN) - 0.03254) <= 1e-5
    assert abs(rref.nb_exact_test_ratio_loop(*PIN) - 0.03254) <= 1e-5


def test_ratio_agrees_with_logspace_on_the_host(sa):
    """Both backends evaluate the same conditional distribution; up to n = 5000 they agree to the step's tolerance of 1e-9."""
    for c in _battery():
        a, b = sa.host_nb_exact_test_ratio(*c), sa.sseq.host_nb_exact_test(*c)
        if abs(a - b) > 1e-9 * b:
            lo, hi = rref.nb_exact_test_ratio_tie_bounds(*c)
            assert lo * (1 - 1e-9) <= b <= hi * (1 + 1e-9), (c, a, b)


def test_new_symbols_in_headers_package_and_library(sa):
    hdr = open(os.path.join(ROOT, "include", "scanrs_amd.h")).read()
    hpp = open(os.path.join(ROOT, "include", "scanrs_amd.hpp")).read()
    lib = ctypes.CDLL(sa.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in scanrs_amd.h"
        assert name in hpp, f"{name} is not mirrored in scanrs_amd.hpp"
        assert name in sa.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert re.search(r"SCANRS_NB_EXACT_LOGSPACE\s*=\s*0\b", hdr) and re.search(r"SCANRS_NB_EXACT_RATIO\s*=\s*1\b", hdr)
    assert (sa.NB_EXACT_LOGSPACE, sa.NB_EXACT_RATIO) == (0, 1)
    for f in ("sseq_de_vs_control", "host_nb_exact_test_ratio", "host_nb_exact_ratio_step"):
        assert callable(getattr(sa, f))
    sseq = hdr[hdr.index("sSeq differential expression"):hdr.index("merge_clusters (scan-rs")]
    for cite in ("dist.rs:155-215", "dist.rs:124-126", "diff_exp.rs:125", "diff_exp.rs:208"):  # the entry points cite the reference
        assert cite in sseq, cite


def test_bad_backend_is_an_argument_error_without_a_device(sa):
    one = sa.SSeqParams(0, 1, np.zeros(0), np.array([1.0]), np.array([1.0]), np.array([True]), np.array([0.5]), 0.0, 0.0, np.array([0.5]))
    for bad in (2, -1, True, "ratio"):
        with pytest.raises(sa.ScanrsError) as e:
            sa.sseq_de_from_sums([3], [4], 5.0, 10.0, one, backend=bad)
        assert e.value.code == 6
    p = np.zeros(1)
    arr = lambda v, t: np.array([v], dtype=t)  # noqa: E731
    u64, f64 = ctypes.c_uint64, ctypes.c_double
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    a, b, fa, fb, mu, phi, use = arr(3, np.uint64), arr(4, np.uint64), arr(5.0, float), arr(10.0, float), arr(1.0, float), arr(0.5, float), arr(1, np.uint8)
    rc = sa._lib.scanrs_sseq_de_from_sums_backend(u64(1), ctypes.c_uint32(1), ptr(a), ptr(b), ptr(fa), ptr(fb), ptr(mu), ptr(phi), ptr(use), u64(900),
                                                  ctypes.c_int(2), None, ptr(p), ptr(p), ptr(p), ptr(p), ptr(p))
    assert rc == 6
