"""The plan of the fixed-point column moments (scanrs_host_col_moments_plan; scan-rs_amd/csrc/col_moments_plan.hpp, the source
normalize_ops.hip decides by) against an exact emulation of the accumulation (tests/moments_ref.py). No device.

The contract, for every slice and without an absolute term: |sum - S1| <= 1e-12 S1, the same for the mean, and
|var - var_ref| <= 1e-10 S2/m; a slice without nonzeros gives exactly 0 and 0."""
import math
import os
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import moments_ref as mr  # noqa: E402


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


def _emulate(case, e1, e2):
    fp = mr.fixed_point_moments(*case.args(), case.n_outer, case.n_inner, e1, e2)
    return mr.contract_ratios(fp["sum"], fp["mean"], fp["var"], case.ref)


def _plan(sa, case, mode=2, n_cu=256):
    return sa.host_col_moments_plan(case.max_count, mr.plan_links(case.links), case.n_outer, case.n_inner, mr.n_workgroups(case.n_outer, n_cu), mode)


def test_symbol_is_declared_exported_and_mirrored(sa):
    name = "scanrs_host_col_moments_plan"
    assert name in sa.EXPORTED_SYMBOLS and hasattr(sa._lib, name)
    for f in ("scanrs_amd.h", "scanrs_amd.hpp"):
        assert name in open(os.path.join(ROOT, "include", f)).read(), f"{name} is missing from {f}"


CASES = sorted(mr.grid_cases())
ADVERSARIAL = [n for n in CASES if mr.grid_cases()[n].adversarial]


@pytest.mark.parametrize("name", CASES)
def test_cases_are_well_posed(name):
    """Plain f64 summation of the f64 terms (the ordinary pass's arithmetic) meets the contract with a margin of two: what the
    cases ask of a route is within reach of f64, the map's rounding of 1 + x included."""
    c = mr.grid_cases()[name]
    pl = mr.plain_f64_moments(*c.args(), c.n_outer, c.n_inner)
    r = mr.contract_ratios(pl["sum"], pl["mean"], pl["var"], c.ref)
    print(name, "plain f64, error / bound (sum, mean, var):", r)
    assert max(r) <= 0.5, r


@pytest.mark.parametrize("name", ADVERSARIAL)
def test_old_rule_accepts_and_violates_the_contract(name):
    c = mr.grid_cases()[name]
    ok, e1, e2 = mr.legacy_plan(mr.legacy_x(c.max_count, c.links), c.n_outer, mr.n_workgroups(c.n_outer), 2)
    assert ok, "the parent's plan took the fixed-point route for this case"
    r = _emulate(c, e1, e2)
    print(name, "old rule, error / bound (sum, mean, var):", r)
    assert max(r) > 1.0, r


@pytest.mark.parametrize("name", CASES)
def test_new_rule_holds_where_it_accepts(sa, name):
    c = mr.grid_cases()[name]
    for mode in (1, 2):
        ok, e1, e2 = _plan(sa, c, mode)
        if not c.adversarial:
            assert ok, "a benign case must stay on the fixed-point route"
        if ok:
            r = _emulate(c, e1, e2)
            print(name, mode, "new rule, error / bound (sum, mean, var):", r)
            assert max(r[:2] if mode == 1 else r) <= 1.0, r


def test_new_rule_at_its_boundary(sa):
    """Slices made of the smallest term only, next to one cell that holds a count of 4000 under factor 1, the small factor swept
    downwards (powers of two: 1 + x stays exact): the plan flips from accept to refuse along the sweep, and every accepted step
    meets the contract."""
    n, accepted, refused = 700, 0, 0
    for k, fn in enumerate((mr.LOG2_1P, mr.LN_1P, mr.LOG10_1P) * 6):
        cells = [{1 + (c % 5): 1} for c in range(n)]
        cells[3] = {0: 4000}
        f = np.full(n, 2.0 ** -(k + 1))
        f[3] = 1.0
        c = mr._from_cells(f"sweep{k}", 7, cells, [f, int(fn)], True)
        ok, e1, e2 = _plan(sa, c)
        if ok:
            accepted += 1
            r = _emulate(c, e1, e2)
            assert max(r) <= 1.0, (k, r)
        else:
            refused += 1
            lok, l1, l2 = mr.legacy_plan(mr.legacy_x(c.max_count, c.links), c.n_outer, mr.n_workgroups(c.n_outer), 2)
            assert lok  # (the old rule took all of them)
    assert accepted >= 3 and refused >= 3, (accepted, refused)


def _bench_like_links(n_cells=1_000_000, seed=0):
    """CellRanger's map on the benchmark's synthetic profile: depth exp(N(0, 0.3)), ~990 genes per cell at depth 1, counts
    1 + Geometric(0.6); factor = median total / total."""
    rng = np.random.default_rng(seed)
    depth = np.exp(rng.normal(0.0, 0.3, size=n_cells))
    total = np.maximum(1.0, np.rint(rng.poisson(990.0 * depth) / 0.6))
    return [np.median(total) / total, mr.LOG2_1P]


def test_benchmark_like_input_stays_on_the_route_with_the_parents_exponents(sa):
    links = _bench_like_links()
    for max_count in (12, 40, 5000):
        for mode in (1, 2):
            ok, e1, e2 = sa.host_col_moments_plan(max_count, mr.plan_links(links), 1_000_000, 33_000, 256, mode)
            assert ok, (max_count, mode)
            lok, l1, l2 = mr.legacy_plan(mr.legacy_x(max_count, links), 1_000_000, 256, mode)
            assert lok and (e1, e2) == (l1, l2)  # the same quanta as before: the accepted results do not change


def test_must_stay_matrices_are_accepted(sa):
    from scanrs_amd.synth import synth_counts, synth_counts_fast

    for m in (synth_counts(3000, 700, 0.05, 5), synth_counts_fast(3000, 700, 0.05, 5, gene_shape=0.1, shared_profile=1.0)):
        tot = np.asarray(m.sum(axis=1)).ravel().astype(np.float64)
        assert tot.min() >= 1
        links = [max(np.median(tot.astype(np.uint32)), 1.0) / tot, mr.LOG2_1P]
        ok, _, _ = sa.host_col_moments_plan(int(m.data.max()), mr.plan_links(links), m.shape[0], m.shape[1], mr.n_workgroups(m.shape[0]), 2)
        assert ok


def _int_bounds_hold(x, n_outer, n_wg, e1, e2):
    """With integers: ceil(n_outer / n_wg) ceil(x 2^e1) < 2^62 and ceil(x 2^e1) < 2^52, likewise for x^2 and e2; x an mpf."""
    cells = -(-n_outer // n_wg)
    for v, e in ((x, e1), (x * x, e2)):
        t = int(mr.MP.ceil(mr.MP.ldexp(v, e)))
        if not (t < 2**52 and cells * t < 2**62):
            return False
    return True


def _exact_x(max_count, links):
    """The largest term there can be, exactly: the chain at the largest count under the largest factors, in mpmath; and the
    device's own evaluation of it (f64, 1 + x rounded), whichever is larger."""
    x = mr.MP.mpf(max_count)
    for l in links:
        x = mr._mp_log(int(l), x) if mr._is_log(l) else x * mr.MP.mpf(float(np.max(l)))
    xd = mr.f64_terms([0, 1], [0], [max_count], [l if mr._is_log(l) else np.array([float(np.max(l))]) for l in links])[0]
    return max(x, mr.MP.mpf(float(xd)))


def test_accumulators_cannot_overflow(sa):
    seen = 0
    # x 1.0001 just below and just above a power of two: the factor is tuned so that log2(1 + c f) 1.0001 straddles 2^k
    for k in (-3, 0, 2, 4):
        for eps in (-3e-16, -1e-9, 0.0, 1e-9, 3e-16):
            target = 2.0**k / 1.0001 * (1.0 + eps)
            f = (2.0**target - 1.0) / 100.0
            links = [np.array([f, f * 0.9]), mr.LOG2_1P]
            for n_outer, n_wg in ((2, 1), (1_000_000, 256), (9000, 141), (2**26, 256), (2**32 - 1, 1)):
                ok, e1, e2 = sa.host_col_moments_plan(100, mr.plan_links(links), n_outer, 10, n_wg, 2)
                assert ok or n_outer >= 2**26, (k, eps, n_outer)  # (with 2^18 and more cells per workgroup the sums leave no room for 40 bits)
                if not ok:
                    continue
                assert _int_bounds_hold(_exact_x(100, links), n_outer, n_wg, e1, e2), (k, eps, n_outer, e1, e2)
                seen += 1
    # all factors near 1e-13: the f64 bound log2(1.0 + x) itself is off in the third digit
    for fn in (mr.LN_1P, mr.LOG2_1P, mr.LOG10_1P):
        for f in (1e-13, 1.37e-13, 0.9e-13, 2.0**-43 * 1.0000001):
            links = [np.array([f, f * 0.99]), int(fn)]
            for n_outer, n_wg in ((300, 5), (1_000_000, 256)):
                ok, e1, e2 = sa.host_col_moments_plan(3, mr.plan_links(links), n_outer, 10, n_wg, 2)
                assert ok, (fn, f)
                assert _int_bounds_hold(_exact_x(3, links), n_outer, n_wg, e1, e2), (fn, f, e1, e2)
                seen += 1
    # a count of 2^32 - 1 in every cell of one slice
    for f, must in ((1e-9, False), (1.0, True), (3e4, True)):
        c = mr._from_cells("huge", 2, [{0: 2**32 - 1}] * 130, [np.full(130, f), mr.LN_1P], False)
        ok, e1, e2 = _plan(sa, c)
        assert ok or not must, f
        if ok:
            assert _int_bounds_hold(_exact_x(2**32 - 1, c.links), 130, mr.n_workgroups(130), e1, e2)
            assert max(_emulate(c, e1, e2)) <= 1.0
            seen += 1
    assert seen >= 80


def test_refusals(sa):
    P = sa.host_col_moments_plan
    good = [("scale", 0.5, 2.0), (mr.LOG2_1P,)]
    assert P(9, good, 1000, 50, 16, 2)[0] and P(9, good, 1000, 50, 16, 1)[0]
    assert not P(9, good, 0, 50, 1, 2)[0] and not P(9, good, 1000, 0, 16, 2)[0]  # nothing to sum over / no slice
    assert not P(9, good, 1000, 50, 16, 0)[0] and not P(9, good, 1000, 50, 16, 3)[0]
    for bad in (float("nan"), float("inf"), -1.0, -0.0 - 1e-300):
        assert not P(9, [("scale", 0.5, bad), (mr.LOG2_1P,)], 1000, 50, 16, 2)[0], bad
    assert not P(9, [("scale", -0.5, 2.0), (mr.LOG2_1P,)], 1000, 50, 16, 2)[0]
    assert not P(9, [("scale", float("nan"), 2.0), (mr.LOG2_1P,)], 1000, 50, 16, 2)[0]
    assert not P(9, [("scale", 0.5, 2.0, False), (mr.LOG2_1P,)], 1000, 50, 16, 2)[0]  # a factor per slice, not per summed-over position
    assert not P(9, [("scale", 0.5, 2.0)], 1000, 50, 16, 2)[0]                         # no logarithm
    assert not P(9, [("scale", 0.5, 2.0), (5,)], 1000, 50, 16, 2)[0]                   # another scalar function (square)
    assert not P(9, [("scale", 0.0, 0.0), (mr.LOG2_1P,)], 1000, 50, 16, 2)[0]          # every factor zero
    # moments_ref.plan_links reduces the factor vectors as the device does: zeros are left out of the minimum and do not refuse
    z = np.array([0.0, 0.7, 1.9, 0.0])
    assert mr.plan_links([z, mr.LN_1P])[0] == ("scale", 0.7, 1.9)
    assert P(9, mr.plan_links([z, mr.LN_1P]), 4, 50, 1, 2)[0]
    assert math.isnan(mr.plan_links([np.array([1.0, -2.0])])[0][2]) and math.isnan(mr.plan_links([np.array([1.0, np.inf])])[0][2])
    # the two accuracy conditions are separate: a spread the sums tolerate and the squares do not
    wide = [("scale", 0.01, 8.9), (mr.LN_1P,)]  # largest / smallest term = 430
    assert P(8, wide, 1000, 50, 16, 1)[0] and not P(8, wide, 1000, 50, 16, 2)[0]
