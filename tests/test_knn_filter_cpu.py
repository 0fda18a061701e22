"""The margin of the kNN filter (knn.hip) against its CPU model, no device needed: with the library's own constants
(scanrs_debug_knn_filter_params) the model of tests/knn_filter_ref.py loses no true neighbour on inputs built to make bf16 rounding
add up instead of cancel, with the margin the code had before (0.0021, derived from a unit roundoff of 2^-9) it does, and the
inputs are small enough for the candidate lists not to overflow (otherwise the fallback would be tested, not the filter)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import knn_filter_ref as kr  # noqa: E402

K = 15


@pytest.fixture(scope="module")
def params():
    import scanrs_amd as sa

    return sa.debug_knn_filter_params()


def test_library_constants_respect_the_floor_of_bf16_rounding(params):
    u = 2.0 ** -8  # 8 significant bits, round to nearest
    assert params["gamma"] >= u * (1 + 2.0 ** -9)  # (u + u^2 / 2): what rounding both operands costs before anything is summed
    assert params["gamma"] < 2 * kr.OLD_GAMMA  # and no blanket doubling beyond the derivation
    assert params["cap"] == 1024 and params["dmax"] == 58 and params["k_max"] == 64 and params["nq_min"] == 256
    # the window: squares of the largest coordinates stay clear of the 1e30 sentinels (145 M^2 < 9e29) and of f32's subnormals
    assert 145 * params["coord_max"] ** 2 < 9e29 and params["coord_min"] ** 2 > 2.0 ** -126 * 2.0 ** 24
    assert params["coord_min"] <= 2.0 ** -40 * 0.5 and params["coord_max"] >= 2.0 ** 40 * 4.0  # the scaled builder cases lie inside


def test_number_format_helpers():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -7, -3.999, 1e-30, 0.0], dtype=np.float32)
    b = kr.bf16_rne(x)
    assert b.tolist()[:4] == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]  # ties go to the even neighbour
    assert b[4] == -4.0 and b[6] == 0.0 and abs(b[5] / np.float32(1e-30) - 1) <= 2.0 ** -8
    assert np.all(b.view(np.uint32) & 0xFFFF == 0)
    v = np.array([np.pi, -1e29, 3e-5, 9e29], dtype=np.float32)
    h, m, lo = kr.split3(v)
    assert np.all(np.abs((h.astype(np.float64) + m + lo) - v) <= 2.0 ** -24 * np.abs(v))
    w = kr.worst_rounding(np.array([1.3, -2.7, 0.6]), 0.47)
    bw = kr.bf16_rne(w.astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(w) > np.abs(bw)) and np.allclose(np.abs(w - bw) / kr.bf16_ulp(bw), 0.47)
    w = kr.worst_rounding(np.array([1.3, -2.7, 0.6]), -0.47)
    assert np.all(np.abs(w) < np.abs(kr.bf16_rne(w.astype(np.float32))))


def test_exact_distances_are_the_fma_chain():
    from fractions import Fraction

    rng = np.random.default_rng(0)
    q, p = rng.standard_normal((3, 7)), rng.standard_normal((5, 7)) * 1e3
    got = kr.exact_d2(q, p)
    for i in range(3):
        for j in range(5):
            s = 0.0
            for c in range(7):
                t = p[j, c] - q[i, c]
                s = float(Fraction(t) * Fraction(t) + Fraction(s))  # one rounding per step: the fused multiply-add
            assert got[i, j] == s
    v = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [3.0, 3.0]])
    assert kr.rank(kr.exact_d2(v, v), 3, drop_self=True).tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [1, 2, 0]]
    assert kr.rank(kr.exact_d2(v, v[:2]), 3).tolist() == [[0, 1, kr.UMAX], [1, 0, kr.UMAX], [0, 1, kr.UMAX], [1, 0, kr.UMAX]]


@pytest.mark.parametrize("name", kr.CASES)
def test_model_with_the_library_margin_loses_no_neighbour(params, name):
    v, d2 = kr.case(name)
    assert params["coord_min"] <= np.max(np.abs(v)) <= params["coord_max"]
    rounds = kr.model_search(v, d2, K, params["gamma"], cap=params["cap"])
    assert rounds
    for st, cnt, lost in rounds:
        assert lost.sum() == 0, (name, st, int((lost > 0).sum()))
        if name in kr.SELECTIVE:  # a cap, not a measurement: shrink the case if a wider margin ever breaks it
            assert cnt.max() <= params["cap"], (name, st, int((cnt > params["cap"]).sum()))
    if name == "box_one_bf16_cell":  # every pair looks alike after rounding: every list overflows, the pure fallback case
        assert all(np.all(cnt > params["cap"]) for _, cnt, _ in rounds)


@pytest.mark.parametrize("name", kr.OLD_MARGIN_FAILS)
def test_model_with_the_old_margin_loses_neighbours(params, name):
    v, d2 = kr.case(name)
    lost_rows = sum(int((lost > 0).sum()) for _, _, lost in kr.model_search(v, d2, K, kr.OLD_GAMMA, cap=params["cap"]))
    assert lost_rows >= 1
    if name == "box_one_bf16_cell":
        assert lost_rows == v.shape[0]  # every list comes back empty


def test_model_threshold_edges(params):
    """tau = +inf lets every point through (and only the clamp, not an overflow to inf, does it); tau below every distance nothing"""
    v = kr.points("worst_2d")[:300]
    assert kr.filter_pass(v, v, np.full(300, np.inf), params["gamma"]).all()
    assert not kr.filter_pass(v + 100.0, v, np.zeros(300), params["gamma"]).any()
