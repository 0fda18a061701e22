"""The helper of the dense-kernel tests (tests/dense_ref.py) and the dispatch of the dense products on the host: the exact int64
reference against Python's big integers, every case of the grid against the route the library's dispatcher reports
(scanrs_debug_dense_route: gram_route / gemm_route of dense.hip, no device needed), the coverage of the grid, and the
neighbours of every threshold."""
import os
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import dense_ref as dr  # noqa: E402


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


@pytest.mark.parametrize("shape", [(1, 1, 1), (7, 3, 5), (33, 17, 2)])
@pytest.mark.parametrize("kind", ["int", "dyadic"])
def test_exact_reference_equals_big_integer_arithmetic(shape, kind):
    k, n, m = shape
    rng = np.random.default_rng([k, n, m])
    make = dr.int_inputs if kind == "int" else dr.dyadic_inputs
    a, b = make(rng, (n, k)), make(rng, (k, m))
    bound = dr.INT_MAX if kind == "int" else 2 ** dr.DYADIC_BITS - 1
    assert a.dtype == np.int64 and np.max(np.abs(a)) <= bound and np.max(np.abs(b)) <= bound
    exact, absref = dr.exact_matmul(a, b)
    for i in range(n):
        for j in range(m):
            assert int(exact[i, j]) == sum(int(a[i, t]) * int(b[t, j]) for t in range(k))
            assert int(absref[i, j]) == sum(abs(int(a[i, t])) * abs(int(b[t, j])) for t in range(k))
    # the doubles handed to the kernels carry the mantissas exactly
    scale = 1 if kind == "int" else 2 ** dr.DYADIC_SCALE
    assert np.array_equal((dr.to_f64(a, kind) * scale).astype(np.int64), a)


def test_exact_reference_refuses_what_could_overflow():
    big = np.full((1, dr.MAX_EXACT_ROWS), 2 ** dr.DYADIC_BITS - 1, dtype=np.int64)
    dr.exact_matmul(big, big.T.copy())  # 2**48 * 4300 < 2**63
    with pytest.raises(AssertionError):
        dr.exact_matmul(np.tile(big, (1, 8)), np.tile(big, (1, 8)).T.copy())


def test_inputs_and_poison_layout():
    rng = np.random.default_rng(0)
    d = dr.dyadic_inputs(rng, (4000,))
    assert np.max(np.abs(d)) < 2 ** 24 and np.min(np.abs(d)) >= 1 and (d < 0).any() and (d > 0).any()
    assert np.sum(np.abs(d) < 2 ** 12) > 1000  # log-uniform: half of the magnitudes below the square root of the range
    v = dr.to_f64(dr.int_inputs(rng, (5, 3)), "int")
    buf = dr.embed(v, 8, 6, True)
    assert np.array_equal(buf[:5, :3], v) and np.isnan(buf[5:]).all() and np.isnan(buf[:, 3:]).all()
    assert not dr.embed(v, 8, 6, False)[5:].any()


def _observed(sa, c):
    if isinstance(c, dr.GramCase):
        return sa.debug_dense_route("gram", c.n, c.m, c.rows, c.ldx, c.ldy, flag=False)
    return sa.debug_dense_route("gemm", c.n, c.m, c.rows, c.ldx, x_aligned16=c.x_skew == 0, flag=bool(c.gemm_direct))


def test_every_case_of_the_grid_reaches_its_route(sa):
    assert len(dr.GRAM_CASES) + len(dr.GEMM_CASES) + len(dr.WCS_CASES) <= 250
    for c in dr.GRAM_CASES:
        assert c.ldx >= c.n and c.ldy >= c.m and (not c.sym or (c.n == c.m and c.ldx == c.ldy))
        assert _observed(sa, c)[0] == c.route == dr.expected_gram_route(c.n, c.m, c.rows, c.ldx, c.ldy), dr.case_id(c)
    for c in dr.GEMM_CASES:
        assert c.ldx >= c.n and c.ldx % 2 == 0 and c.ldw >= c.m and c.ldw % 2 == 1 and c.ldo > c.m and c.ldc != c.ldo and c.ldc > c.m
        exp = dr.expected_gemm_route(c.n, c.m, c.rows, c.ldx, aligned=c.x_skew == 0, gemm_direct=bool(c.gemm_direct))
        assert _observed(sa, c) == exp and exp[0] == c.route, dr.case_id(c)
    for c in dr.WCS_CASES:
        assert c.ldx % 2 == 0 and c.ldx >= dr.even_up(c.l) and (not c.with_xc or c.l % 2 == 0)


def test_the_grid_covers_every_route_and_template_instance(sa):
    assert {_observed(sa, c)[0] for c in dr.GRAM_CASES} == {dr.GRAM_WAVE, dr.GRAM_VEC, dr.GRAM_TILED}
    seen = [_observed(sa, c) for c in dr.GEMM_CASES]
    assert {r for r, _, _ in seen} == {dr.GEMM_WAVE, dr.GEMM_TILED, dr.GEMM_SKINNY_LDS, dr.GEMM_DIRECT}
    assert {nt for r, nt, _ in seen if r == dr.GEMM_WAVE} == {1, 2, 4}
    assert {nt for r, nt, _ in seen if r == dr.GEMM_DIRECT} == {1, 2, 3, 4, 5, 6, 7}
    groups = {g for r, _, g in seen if r == dr.GEMM_DIRECT}
    assert {1, 2, 3} <= groups and max(groups) >= 4
    assert {g for r, _, g in seen if r == dr.GEMM_SKINNY_LDS} >= {1, 3} and {g for r, _, g in seen if r == dr.GEMM_TILED} >= {1, 2}
    # both the symmetric and the general tiled Gram, with one, two and three tile rows; the mirrored tiles need n > 128
    tiled = [c for c in dr.GRAM_CASES if c.route == dr.GRAM_TILED]
    assert {(c.n + 127) // 128 for c in tiled if c.sym} == {1, 2, 3} and any(not c.sym for c in tiled)
    # forced runs exist for every GEMM route that the default options would not reach at the same shape
    assert {c.route for c in dr.GEMM_CASES if c.forced} >= {dr.GEMM_WAVE, dr.GEMM_TILED, dr.GEMM_SKINNY_LDS}
    assert any(c.with_xc for c in dr.WCS_CASES) and any(not c.with_xc for c in dr.WCS_CASES)


def test_threshold_neighbours_route_as_documented(sa):
    gram = lambda n, m, rows, ldx, ldy, **kw: sa.debug_dense_route("gram", n, m, rows, ldx, ldy, **kw)[0]  # noqa: E731
    gemm = lambda n, m, rows, ldx, **kw: sa.debug_dense_route("gemm", n, m, rows, ldx, **kw)  # noqa: E731
    # Gram: LDS tiles from rows >= 2048, n >= 48, m >= 48, both leading dimensions even, not on a side stream
    assert gram(48, 48, 2047, 48, 48) == dr.GRAM_WAVE and gram(48, 48, 2048, 48, 48) == dr.GRAM_TILED
    assert gram(47, 48, 2048, 48, 48) == dr.GRAM_WAVE and gram(48, 47, 2048, 48, 48) == dr.GRAM_WAVE
    assert gram(48, 48, 2048, 49, 48) == dr.GRAM_WAVE and gram(48, 48, 2048, 48, 49) == dr.GRAM_WAVE
    assert gram(48, 48, 2048, 48, 48, side=True) == dr.GRAM_WAVE
    # ... the streaming form for one vector from rows >= 4096, at most 128 panel columns, never under a skip flag
    assert gram(64, 1, 4095, 64, 2) == dr.GRAM_WAVE and gram(64, 1, 4096, 64, 2) == dr.GRAM_VEC
    assert gram(128, 1, 4096, 128, 2) == dr.GRAM_VEC and gram(129, 1, 4096, 130, 2) == dr.GRAM_WAVE
    assert gram(64, 2, 4096, 64, 2) == dr.GRAM_WAVE and gram(64, 1, 4096, 64, 2, flag=True) == dr.GRAM_WAVE
    assert gram(64, 1, 4096, 64, 2, side=True) == dr.GRAM_VEC
    # GEMM: straight from memory from n >= 16 and rows >= 64 when X is 16-byte aligned and the option is on
    on = dict(flag=True)
    assert gemm(15, 20, 64, 16, **on)[0] == dr.GEMM_WAVE and gemm(16, 20, 64, 16, **on)[0] == dr.GEMM_DIRECT
    assert gemm(16, 20, 63, 16, **on)[0] == dr.GEMM_WAVE
    assert gemm(16, 20, 64, 16, x_aligned16=False, **on)[0] == dr.GEMM_WAVE and gemm(16, 20, 64, 16, flag=False)[0] == dr.GEMM_WAVE
    assert gemm(16, 4096, 64, 16, **on)[0] == dr.GEMM_DIRECT and gemm(16, 4097, 64, 16, **on)[0] == dr.GEMM_WAVE
    with pytest.raises(sa.ScanrsError) as e:  # odd ldx: the dispatcher refuses
        gemm(16, 20, 64, 17, **on)
    assert e.value.code == 6  # SCANRS_ERR_ARGUMENT
    # ... one column group up to 112 columns (NT = 7), groups of at most 64 beyond
    assert gemm(16, 112, 64, 16, **on) == (dr.GEMM_DIRECT, 7, 1) and gemm(16, 113, 64, 16, **on) == (dr.GEMM_DIRECT, 4, 2)
    assert gemm(16, 129, 64, 16, **on) == (dr.GEMM_DIRECT, 3, 3) and gemm(16, 200, 64, 16, **on) == (dr.GEMM_DIRECT, 4, 4)
    # ... else the LDS tiles from rows >= 2048, n >= 16, m >= 48: 256 x 64 when the last 128-column tile would be at most half full
    assert gemm(16, 48, 2047, 16)[0] == dr.GEMM_WAVE and gemm(16, 48, 2048, 16)[0] == dr.GEMM_SKINNY_LDS
    assert gemm(15, 48, 2048, 16)[0] == dr.GEMM_WAVE and gemm(16, 47, 2048, 16)[0] == dr.GEMM_WAVE
    assert gemm(16, 64, 2048, 16)[0] == dr.GEMM_SKINNY_LDS and gemm(16, 65, 2048, 16)[0] == dr.GEMM_TILED
    assert gemm(16, 128, 2048, 16)[0] == dr.GEMM_TILED and gemm(16, 129, 2048, 16) == (dr.GEMM_SKINNY_LDS, 0, 3)
    assert gemm(16, 192, 2048, 16)[0] == dr.GEMM_SKINNY_LDS and gemm(16, 193, 2048, 16) == (dr.GEMM_TILED, 0, 2)
    assert gemm(16, 65, 2048, 16, side=True)[0] == dr.GEMM_WAVE
    # ... else one wave per 16 rows with 1, 2 or 4 column tiles
    assert [gemm(4, m, 10, 4)[1:] for m in (16, 17, 32, 33, 64, 65)] == [(1, 1), (2, 1), (2, 1), (4, 1), (4, 1), (4, 2)]


def test_route_function_agrees_with_the_restated_rules_around_every_threshold(sa):
    for rows in (63, 64, 2047, 2048, 4095, 4096):
        for n in (15, 16, 47, 48, 128, 129):
            for m in (1, 47, 48, 64, 65, 112, 113, 192, 193):
                for ld_odd in (0, 1):
                    ldx, ldy = n + (n + ld_odd) % 2, m + (m + ld_odd) % 2
                    for flag in (False, True):
                        assert sa.debug_dense_route("gram", n, m, rows, ldx, ldy, flag=flag)[0] == \
                            dr.expected_gram_route(n, m, rows, ldx, ldy, skip=flag)
                        if ldx % 2 == 0:
                            for aligned in (False, True):
                                assert sa.debug_dense_route("gemm", n, m, rows, ldx, x_aligned16=aligned, flag=flag) == \
                                    dr.expected_gemm_route(n, m, rows, ldx, aligned=aligned, gemm_direct=flag)
