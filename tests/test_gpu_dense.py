"""Every dense f64-MFMA kernel on its own (scan-rs_amd/csrc/panel_ops.hip, dense.hip, dense_skinny.inc) through the test entry points
scanrs_debug_dense_gram / _gemm / _weighted_colsum, over the grid of tests/dense_ref.py.

Exact class: integer inputs, every partial sum an integer below 2**53, so the result is bit-identical to the int64 reference whatever
the order of the sums: np.array_equal, no tolerance. The same calls again with NaN in every padding column and surplus row must give
the same bits and leave everything outside the result untouched. Rounding class: dyadic inputs against the int64 reference under
gamma_K (|X|^T |Y|), the bound of any summation order with or without FMA (K = rows + 2 for a Gram, n + 4 for a GEMM)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import dense_ref as dr  # noqa: E402

ERR_ARGUMENT = 6


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


@pytest.fixture(scope="module")
def h(sa):
    """one handle from a tiny matrix: the dense kernels only use its stream and scratch"""
    rng = np.random.default_rng(5)
    return sa.AdaptiveMat.from_dense((rng.random((20, 30)) < 0.3).astype(np.uint32), sa.CSR)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- one call -----------------------------------------------------------------------------------------------------------------
def gram_call(h, c, kind="int", poison=False, route=0, skip=False, x_vals=None):
    d = dr.gram_data(c, kind)
    ra = c.rows + dr.SURPLUS_ROWS
    xv = dr.to_f64(d.x, kind) if x_vals is None else x_vals
    xb = dr.embed(xv, ra, c.ldx, poison)
    yb = None if c.sym else dr.embed(dr.to_f64(d.y, kind), ra, c.ldy, poison)
    return h.debug_dense_gram(xb, c.n, yb, c.m, c.rows, np.full((c.n, c.m), np.nan), route=route, skip=skip)


def gemm_call(h, c, scalars, kind="int", poison=False, route=0, skip=False, x_vals=None, gemm_direct=None, x_skew=None):
    """(the whole out buffer, the expected values of its result region as doubles computed from the int64 reference)"""
    alpha, beta, mode = scalars
    d = dr.gemm_data(c, kind)
    ra = c.rows + dr.SURPLUS_ROWS
    xb = dr.embed(dr.to_f64(d.x, kind) if x_vals is None else x_vals, ra, c.ldx, poison)
    wb = dr.embed(dr.to_f64(d.w, kind), c.n, c.ldw, poison)
    cv = dr.to_f64(d.cin, kind)
    out, cin = np.full((ra, c.ldo), np.nan), None
    if mode == "in_place":
        out[: c.rows, : c.m] = cv
    elif mode == "separate":
        cin = dr.embed(cv, ra, c.ldc, poison)
    elif mode == "nan":
        cin = np.full((ra, c.ldc), np.nan)
    h.set_option("gemm_direct", c.gemm_direct if gemm_direct is None else gemm_direct)
    try:
        res = h.debug_dense_gemm(xb, c.n, wb, c.m, c.rows, out, alpha, beta, cin, mode == "in_place", route,
                                 c.x_skew if x_skew is None else x_skew, skip)
    finally:
        h.set_option("gemm_direct", 1)
    scale = 1.0 if kind == "int" else 2.0 ** (-2 * dr.DYADIC_SCALE)
    want = alpha * (d.exact.astype(np.float64) * scale) + (beta * cv if beta != 0.0 else 0.0)
    return res, want


def check_gemm_buffer(c, res, want, what):
    """the result region equals `want` bit for bit and everything else still holds the NaN sentinel"""
    inside = res[: c.rows, : c.m]
    assert not np.isnan(inside).any(), f"{what}: NaN in the result"
    assert np.array_equal(inside, want), f"{what}: {np.argwhere(inside != want)[:8].tolist()} differ"
    assert np.isnan(res[c.rows:]).all() and np.isnan(res[:, c.m:]).all(), f"{what}: wrote outside the result"


# ---- 1, 2, 4: exact class, poison, determinism --------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(dr.GRAM_NAMES), ids=lambda r: dr.GRAM_NAMES[r])
def test_gram_is_exact_with_clean_and_poisoned_padding(h, route):
    for c in (c for c in dr.GRAM_CASES if c.route == route):
        want = dr.gram_data(c, "int").exact.astype(np.float64)
        for poison in (False, True):
            got = gram_call(h, c, poison=poison)
            assert not np.isnan(got).any(), f"{dr.case_id(c)} poison={poison}: NaN or unwritten entries {np.argwhere(np.isnan(got))[:8].tolist()}"
            assert np.array_equal(got, want), f"{dr.case_id(c)} poison={poison}: {np.argwhere(got != want)[:8].tolist()} differ"
        again = gram_call(h, c, poison=True)
        assert np.array_equal(_bits(again), _bits(got)), f"{dr.case_id(c)}: not deterministic"
        if c.forced:
            assert np.array_equal(gram_call(h, c, poison=True, route=c.route), want), f"{dr.case_id(c)}: forced route"


@pytest.mark.parametrize("route", sorted(dr.GEMM_NAMES), ids=lambda r: dr.GEMM_NAMES[r])
def test_gemm_is_exact_with_clean_and_poisoned_padding(h, route):
    for c in (c for c in dr.GEMM_CASES if c.route == route):
        for scalars in dr.GEMM_SCALARS:
            for poison in (False, True):
                res, want = gemm_call(h, c, scalars, poison=poison)
                check_gemm_buffer(c, res, want, f"{dr.case_id(c)} {scalars} poison={poison}")
        again, _ = gemm_call(h, c, dr.GEMM_SCALARS[-1], poison=True)
        assert np.array_equal(_bits(again), _bits(res)), f"{dr.case_id(c)}: not deterministic"
        if c.forced:  # the same kernel forced under the default options, where the dispatcher would choose another
            for scalars in dr.GEMM_SCALARS:
                res, want = gemm_call(h, c, scalars, poison=True, route=c.route, gemm_direct=1, x_skew=0)
                check_gemm_buffer(c, res, want, f"{dr.case_id(c)} {scalars} forced")


def test_direct_and_lds_forms_agree_bitwise(h):
    """gemm_skinny_mfma_f64 names both the direct and the 256 x 64 LDS form in the profile: the direct cases once more with
    gemm_direct = 0 (the wave or LDS kernels) must give the same bits on the exact class"""
    for c in (c for c in dr.GEMM_CASES if c.route == dr.GEMM_DIRECT):
        a, want = gemm_call(h, c, dr.GEMM_SCALARS[2], poison=True, gemm_direct=1)
        b, _ = gemm_call(h, c, dr.GEMM_SCALARS[2], poison=True, gemm_direct=0)
        check_gemm_buffer(c, a, want, dr.case_id(c))
        assert np.array_equal(_bits(a), _bits(b)), dr.case_id(c)


def test_weighted_colsum_is_exact_and_the_compact_copy_is_the_panel(h):
    for c in dr.WCS_CASES:
        d = dr.wcs_data(c)
        ldw, ldc = c.l + 3, c.l + 2
        for poison in (False, True):
            xb = dr.embed(dr.to_f64(d.x, "int"), c.n, c.ldx, poison)
            w, xc = h.debug_weighted_colsum(dr.to_f64(d.b, "int"), xb, c.l, np.full((c.rank, ldw), np.nan),
                                            np.full((c.n, ldc), np.nan) if c.with_xc else None)
            what = f"{dr.case_id(c)} poison={poison}"
            assert np.array_equal(w[:, : c.l], d.exact.astype(np.float64)), what
            assert np.isnan(w[:, c.l:]).all(), f"{what}: wrote into the padding of w"
            if c.with_xc:
                assert np.array_equal(xc[:, : c.l], xb[:, : c.l]) and np.isnan(xc[:, c.l:]).all(), f"{what}: compact copy"
        w2, _ = h.debug_weighted_colsum(dr.to_f64(d.b, "int"), xb, c.l, np.full((c.rank, ldw), np.nan), None)
        assert np.array_equal(_bits(w2), _bits(w)), f"{dr.case_id(c)}: not deterministic, or the copy changes the sums"


# ---- 3: rounding class --------------------------------------------------------------------------------------------------------
def test_gram_rounding_stays_within_the_summation_bound(h):
    cases = dr.first_per_route([c for c in dr.GRAM_CASES if 64 <= c.rows <= dr.MAX_EXACT_ROWS and c.n >= 15], key=lambda c: (c.route, c.sym))
    assert {c.route for c in cases} == set(dr.GRAM_NAMES)
    unit = 2.0 ** (-2 * dr.DYADIC_SCALE)
    for c in cases:
        d = dr.gram_data(c, "dyadic")
        got = gram_call(h, c, kind="dyadic", poison=True)
        err = np.abs(got - d.exact.astype(np.float64) * unit)
        bound = dr.gamma(c.rows + 2) * (d.absref.astype(np.float64) * unit)
        print(f"{dr.case_id(c)}: max err / bound = {np.max(err / bound):.3g}")
        assert (err <= bound).all(), dr.case_id(c)


def test_gemm_rounding_stays_within_the_summation_bound(h, sa):
    def key(c):
        return (c.route,) + sa.debug_dense_route("gemm", c.n, c.m, c.rows, c.ldx, x_aligned16=c.x_skew == 0, flag=bool(c.gemm_direct))[1:2]

    cases = dr.first_per_route(dr.GEMM_CASES, key=key)
    assert len(cases) == 3 + 7 + 1 + 1  # NJ 1, 2, 4; NT 1..7; the two LDS forms
    alpha, beta = 0.5, 2.0
    unit = 2.0 ** (-2 * dr.DYADIC_SCALE - 1)  # alpha X W + beta Cin in units of 2**-41: x w + cin * 2**22, exact in int64
    for c in cases:
        d = dr.gemm_data(c, "dyadic")
        res, _ = gemm_call(h, c, (alpha, beta, "separate"), kind="dyadic", poison=True)
        exact = (d.exact + (d.cin << 22)).astype(np.float64) * unit
        absref = (d.absref + (np.abs(d.cin) << 22)).astype(np.float64) * unit
        err, bound = np.abs(res[: c.rows, : c.m] - exact), dr.gamma(c.n + 4) * absref
        print(f"{dr.case_id(c)}: max err / bound = {np.max(err / bound):.3g}")
        assert (err <= bound).all(), dr.case_id(c)
        assert np.isnan(res[c.rows:]).all() and np.isnan(res[:, c.m:]).all()


# ---- 5: the skip flag ---------------------------------------------------------------------------------------------------------
def test_a_set_skip_flag_leaves_every_output_untouched(h):
    for c in dr.GRAM_CASES:
        routes = {0} | ({c.route} if c.route != dr.GRAM_VEC else set())  # (gram_vec refuses a skip flag: its reducer has no test)
        for route in routes:
            assert np.isnan(gram_call(h, c, route=route, skip=True)).all(), f"{dr.case_id(c)} route {route}"
    for c in dr.GEMM_CASES:
        for route in {0, c.route if c.x_skew == 0 else 0}:
            res, _ = gemm_call(h, c, dr.GEMM_SCALARS[0], route=route, skip=True, gemm_direct=1 if route else None)
            assert np.isnan(res).all(), f"{dr.case_id(c)} route {route}"
    c = dr.GEMM_CASES[0]
    res, want = gemm_call(h, c, dr.GEMM_SCALARS[0])  # the flag is gone again afterwards
    check_gemm_buffer(c, res, want, "after skip")


# ---- 6: NaN locality ----------------------------------------------------------------------------------------------------------
def test_one_nan_in_x_stays_in_its_row(h):
    for c in dr.first_per_route([c for c in dr.GRAM_CASES if c.rows >= 9 and c.n >= 15], key=lambda c: (c.route, c.sym, c.n > 128)):
        d = dr.gram_data(c, "int")
        xv = dr.to_f64(d.x, "int")
        r, i = c.rows - 1, c.n - 1
        xv[r, i] = np.nan
        mask = np.zeros((c.n, c.m), dtype=bool)
        mask[i, :] = True
        if c.sym:
            mask[:, i] = True
        got = gram_call(h, c, poison=True, x_vals=xv)
        assert np.array_equal(np.isnan(got), mask), dr.case_id(c)
        assert np.array_equal(got[~mask], d.exact.astype(np.float64)[~mask]), dr.case_id(c)
    for c in dr.first_per_route([c for c in dr.GEMM_CASES if c.rows >= 16 and c.n >= 3]):
        xv = dr.to_f64(dr.gemm_data(c, "int").x, "int")
        r = c.rows - 2
        xv[r, c.n - 1] = np.nan
        res, want = gemm_call(h, c, dr.GEMM_SCALARS[0], poison=True, x_vals=xv)
        mask = np.zeros((c.rows, c.m), dtype=bool)
        mask[r, :] = True
        assert np.array_equal(np.isnan(res[: c.rows, : c.m]), mask), dr.case_id(c)
        assert np.array_equal(res[: c.rows, : c.m][~mask], want[~mask]), dr.case_id(c)


# ---- 7: the dispatcher ran the kernel it announced ------------------------------------------------------------------------------
def _ran(h, call):
    h.profile_enable(True)
    try:
        h.profile_reset()
        call()
        return {k for k, v in h.profile_get().items() if v["launches"] > 0}
    finally:
        h.profile_enable(False)


def test_route_zero_runs_the_kernel_the_dispatcher_announces(h, sa):
    for c in dr.GRAM_CASES:
        route = sa.debug_dense_route("gram", c.n, c.m, c.rows, c.ldx, c.ldy)[0]
        assert _ran(h, lambda: gram_call(h, c)) == {dr.GRAM_PROFILE[route]}, dr.case_id(c)
    for c in dr.GEMM_CASES:
        route = sa.debug_dense_route("gemm", c.n, c.m, c.rows, c.ldx, x_aligned16=c.x_skew == 0, flag=bool(c.gemm_direct))[0]
        assert _ran(h, lambda: gemm_call(h, c, dr.GEMM_SCALARS[0])) == {dr.GEMM_PROFILE[route]}, dr.case_id(c)
    c = dr.WCS_CASES[0]
    d = dr.wcs_data(c)
    assert _ran(h, lambda: h.debug_weighted_colsum(dr.to_f64(d.b, "int"), dr.embed(dr.to_f64(d.x, "int"), c.n, c.ldx, False), c.l,
                                                   np.zeros((c.rank, c.l)))) == {"weighted_colsum"}


# ---- 8: forced routes whose preconditions fail ------------------------------------------------------------------------------------
def test_a_forced_route_with_failing_preconditions_is_refused(h, sa):
    def refused(call):
        """SCANRS_ERR_ARGUMENT, and no kernel was launched"""
        h.profile_enable(True)
        try:
            h.profile_reset()
            with pytest.raises(sa.ScanrsError) as e:
                call()
            launched = {k for k, v in h.profile_get().items() if v["launches"] > 0}
        finally:
            h.profile_enable(False)
        return e.value.code == ERR_ARGUMENT and not launched

    x, c1 = np.ones((70, 8)), np.full((8, 1), np.nan)
    assert refused(lambda: h.debug_dense_gram(x, 8, np.ones((70, 2)), 2, 64, np.zeros((8, 2)), route=dr.GRAM_VEC))  # m != 1
    assert refused(lambda: h.debug_dense_gram(np.ones((70, 130)), 129, np.ones((70, 1)), 1, 64, np.zeros((129, 1)), route=dr.GRAM_VEC))
    assert refused(lambda: h.debug_dense_gram(x, 8, np.ones((70, 1)), 1, 64, c1, route=dr.GRAM_VEC, skip=True))
    assert refused(lambda: h.debug_dense_gram(np.ones((70, 9)), 8, np.ones((70, 2)), 2, 64, np.zeros((8, 2)), route=dr.GRAM_TILED))  # odd ldx
    assert refused(lambda: h.debug_dense_gram(x, 8, np.ones((70, 3)), 2, 64, np.zeros((8, 2)), route=dr.GRAM_TILED))  # odd ldy
    assert refused(lambda: h.debug_dense_gram(x, 8, None, 4, 64, np.zeros((8, 4))))  # Y is X needs the same shape
    assert refused(lambda: h.debug_dense_gram(x, 8, None, 8, 64, np.zeros((8, 8)), route=9))
    w, out = np.ones((16, 5)), np.full((70, 7), np.nan)
    x16 = np.ones((70, 16))
    assert refused(lambda: h.debug_dense_gemm(x16, 16, w, 5, 64, out, route=dr.GEMM_DIRECT, x_skew=1))  # X not 16-byte aligned
    assert refused(lambda: h.debug_dense_gemm(x, 8, np.ones((8, 5)), 5, 64, out, route=dr.GEMM_DIRECT))  # n < 16
    assert refused(lambda: h.debug_dense_gemm(x16, 16, w, 5, 63, out, route=dr.GEMM_DIRECT))  # rows < 64
    assert refused(lambda: h.debug_dense_gemm(x16, 16, w, 5, 64, out, route=9))
    for route in (0, dr.GEMM_WAVE, dr.GEMM_TILED, dr.GEMM_SKINNY_LDS, dr.GEMM_DIRECT):  # odd ldx, as launch_gemm_nn always answered
        assert refused(lambda: h.debug_dense_gemm(np.ones((70, 17)), 16, w, 5, 64, out, route=route))
    assert refused(lambda: h.debug_dense_gemm(x16, 16, w, 5, 64, out, beta=1.0))  # beta without a Cin
    # an Out that overlaps X (the wrapper copies `out`, so through the C entry point itself)
    import ctypes

    buf = np.ones(70 * 16)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    code = sa._lib.scanrs_debug_dense_gemm(h._h, ctypes.c_int(0), p(buf), ctypes.c_int(0), ctypes.c_uint32(16), ctypes.c_uint32(16), p(w),
                                           ctypes.c_uint32(5), ctypes.c_uint32(5), ctypes.c_uint64(64), ctypes.c_uint64(70), ctypes.c_double(1.0),
                                           ctypes.c_double(0.0), None, ctypes.c_uint32(0), p(buf[8:]), ctypes.c_uint32(7), ctypes.c_int(0),
                                           ctypes.c_int(0))
    assert code == ERR_ARGUMENT and np.array_equal(buf, np.ones(70 * 16))
    # a refused call leaves the handle usable, the skip flag and the output as they were
    got = h.debug_dense_gemm(x16, 16, w, 5, 64, out, route=dr.GEMM_DIRECT)
    assert np.array_equal(got[:64, :5], np.full((64, 5), 16.0)) and np.isnan(got[64:]).all() and np.isnan(got[:, 5:]).all()
    res = h.debug_dense_gram(x, 8, np.ones((70, 1)), 1, 64, c1, route=dr.GRAM_VEC)
    assert np.array_equal(res, np.full((8, 1), 64.0))
