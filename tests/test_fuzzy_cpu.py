"""fuzzy_simplicial_set without a device: the library's exponential against mpmath, the reference's own tables
(tests/golden/fuzzy_reference_tables.json, from umap-rs/src/fuzzy.rs:191-261) through the host entries, the host twin against the
plain-Python restatement (tests/fuzzy_ref.py) over the shared grid (tests/fuzzy_cases.py) - bit for bit with the library's
exponential, within a derived bound with the reference's -, the literal quirks, the refusals and the public surface."""
import ctypes
import gc
import json
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fuzzy_cases as cases  # noqa: E402
import fuzzy_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {
    "scanrs_fuzzy_simplicial_set": r"fuzzy\.rs:30-62",
    "scanrs_fuzzy_simplicial_set_device": r"fuzzy\.rs:30-62",
    "scanrs_umap_graph": r"umap\.rs:89-100",
    "scanrs_umap_graph_device": r"umap\.rs:89-100",
    "scanrs_host_fuzzy_simplicial_set": r"fuzzy\.rs:30-62",
    "scanrs_graph_info": r"fuzzy\.rs:39",
    "scanrs_graph_to_host": r"fuzzy\.rs:47",
    "scanrs_graph_sigmas_rhos": r"fuzzy\.rs:43",
    "scanrs_graph_device": r"fuzzy\.rs:47",
    "scanrs_graph_free": r"fuzzy\.rs:47",
    "scanrs_graph_edge_count": r"embedding\.rs:38-49",
    "scanrs_graph_edges": r"embedding\.rs:38-53, 75-85",
    "scanrs_host_fuzzy_exp": r"fuzzy\.rs:126, 171",
    "scanrs_host_smooth_knn_dist": r"fuzzy\.rs:117-145",
    "scanrs_host_membership_strengths": r"fuzzy\.rs:148-181",
}


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


@pytest.fixture(scope="module")
def tables():
    with open(os.path.join(ROOT, "tests", "golden", "fuzzy_reference_tables.json")) as f:
        return json.load(f)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool(np.all(a == b))


def lib_exp_many(sa):
    return lambda xs: sa.host_fuzzy_exp(np.array(xs, dtype=np.float64)).tolist()


def ulp_error(y, t):
    """|y - t| in units of the spacing of doubles at t (t: mpmath value, y: float)"""
    import mpmath

    tf = float(t)
    u = math.ulp(tf) if tf > 0.0 else 5e-324
    return float(abs(mpmath.mpf(y) - t) / u)


def test_the_exponential_is_within_one_ulp_of_mpmath(sa):
    """The largest error measured here: 0.803 ulp over 6000 arguments in [-746, 0], 0.705 ulp in the subnormal tail below -708.4 (where
    the last product rounds once more). Asserted: < 1 ulp everywhere."""
    import mpmath

    mpmath.mp.prec = 200
    rng = np.random.default_rng(5)
    xs = np.concatenate([-rng.uniform(0.0, 746.0, 2500), -rng.uniform(0.0, 2.0, 1500), -rng.uniform(708.0, 746.0, 1500),
                         -(2.0 ** -np.arange(0.0, 60.0)), -np.arange(0.0, 440.0) * 0.34657359027997264 / 220.0])
    ys = sa.host_fuzzy_exp(xs)
    worst, worst_tail = 0.0, 0.0
    for x, y in zip(xs.tolist(), ys.tolist()):
        e = ulp_error(y, mpmath.exp(mpmath.mpf(x)))
        worst = max(worst, e)
        if x < -708.4:
            worst_tail = max(worst_tail, e)
    print(f"fz_exp: largest error {worst:.3f} ulp over {len(xs)} arguments, {worst_tail:.3f} ulp in the subnormal tail")
    assert worst < 1.0
    special = sa.host_fuzzy_exp([0.0, -0.0, -np.inf, np.nan, -745.2, -1e300, -5e-324])
    assert same_bits(special[:3], [1.0, 1.0, 0.0]) and math.isnan(special[3]) and same_bits(special[4:], [0.0, 0.0, 1.0])
    tail = sa.host_fuzzy_exp([-708.5, -720.0, -740.0, -745.13])  # gradual underflow: subnormal, decreasing, positive
    assert np.all(tail > 0.0) and np.all(tail < 2.2250738585072014e-308) and np.all(np.diff(tail) < 0.0)
    assert tail[-1] == 5e-324


def test_the_references_tables(sa, tables):
    for t in tables["rhos"]:
        d = np.array(t["knn_distances"])
        n, k = d.shape
        idx = np.array([[(i + 1 + j) % n for j in range(k)] for i in range(n)], dtype=np.uint32)
        g = sa.host_fuzzy_simplicial_set(idx, d, t["local_connectivity"], 1.0, True, t["n_iter"], t["bandwidth"])
        assert same_bits(g.rhos, t["rhos"]), (t, g.rhos)
        g.close()
    m = tables["membership"]
    rows, cols, vals = sa.host_membership_strengths(m["knn_indices"], m["knn_distances"], m["sigmas"], m["rhos"])
    assert rows.tolist() == m["rows"] and cols.tolist() == m["cols"]
    assert same_bits(vals[:3], [0.0, 0.0, 0.0])
    for v, want in zip(vals.tolist(), m["values"]):
        assert abs(v - want) <= math.ulp(want), (v, want)
    s = tables["smooth_knn_dist"]
    sigma, iterations = sa.host_smooth_knn_dist(s["distances"], s["rho"], s["bandwidth"], s["n_iter"])
    psum = 0.0
    for v in s["distances"]:
        psum = psum + math.exp(-(max(max(v, -s["rho"]), 0.0) / sigma))
    assert psum - math.log2(s["k"]) * s["bandwidth"] <= s["tolerance"] and 1 <= iterations <= s["n_iter"]
    h = tables["shape"]
    g = sa.host_fuzzy_simplicial_set(h["knn_indices"], h["knn_distances"], h["local_connectivity"], h["set_op_mix_ratio"], h["apply_fuzzy_combine"],
                                     h["n_iter"], h["bandwidth"])
    assert list(g.shape) == h["shape"]
    g.close()


def twin(sa, case):
    """the twin's outputs, or ('refused', message)"""
    _, idx, dist, prm, n_epochs = case
    try:
        g = sa.host_fuzzy_simplicial_set(idx, dist, **prm)
    except sa.ScanrsError as e:
        return "refused", str(e)
    with g:
        indptr, indices, values = g.to_csr()
        assert g.nnz == len(values) and g.shape == (idx.shape[0], idx.shape[0])
        return dict(indptr=indptr, indices=indices, values=values, sigmas=g.sigmas, rhos=g.rhos, edges=g.edges(n_epochs))


def restated(case, exp_many, total):
    _, idx, dist, prm, _ = case
    try:
        return ref.fuzzy_simplicial_set(idx.tolist(), dist.tolist(), prm["local_connectivity"], prm["set_op_mix_ratio"], prm["apply_fuzzy_combine"],
                                        prm["n_iter"], prm["bandwidth"], exp_many, total)
    except ref.Refused as r:
        return r


_GRID = {}


def grid_by_size(sa):
    if not _GRID:
        for case in cases.grid(sa):
            _GRID.setdefault(case[1].shape[0], []).append(case)
    return _GRID


GRID_SIZES = (2, 3, 6, 65, 257, 1000, 1500)


@pytest.mark.parametrize("n", GRID_SIZES)
def test_the_twin_equals_the_restatement_with_the_same_exponential(sa, n):
    assert sorted(grid_by_size(sa)) == sorted(GRID_SIZES)
    n_refused = 0
    for case in grid_by_size(sa)[n]:
        name, idx, dist, prm, n_epochs = case
        want, got = restated(case, lib_exp_many(sa), "tree"), twin(sa, case)
        if isinstance(want, ref.Refused):
            assert isinstance(got, tuple) and f"row {want.row} " in got[1], (name, want.row, got)
            n_refused += 1
            continue
        assert not isinstance(got, tuple), (name, got)
        assert same_bits(got["rhos"], want["rhos"]), name
        assert same_bits(got["sigmas"], want["sigmas"]), name
        assert got["indptr"].tolist() == want["indptr"] and got["indices"].tolist() == want["indices"], name
        assert same_bits(got["values"], want["values"]), name
        head, tail, w, eps = ref.edges(want["indptr"], want["indices"], want["values"], n_epochs)
        assert got["edges"][0].tolist() == head and got["edges"][1].tolist() == tail, name
        assert same_bits(got["edges"][2], w) and same_bits(got["edges"][3], eps), name
        # the stated deviation: sigma of rows whose rho is not > 0 against the reference's sequential global mean
        seq = ref.sequential_global_floor(dist.tolist(), want["raw_sigmas"])
        k = idx.shape[1]
        for i in range(n):
            if not want["rhos"][i] > 0.0:
                assert abs(got["sigmas"][i] - seq[i]) <= 2 * n * k * 2.0 ** -53 * abs(seq[i]), (name, i)
    print(f"n = {n}: {len(grid_by_size(sa)[n])} cases, {n_refused} of them refused by both")


@pytest.mark.parametrize("n", GRID_SIZES)
def test_the_twin_against_the_restatement_with_the_references_exponential(sa, n):
    """Values within 2^-50 absolute: each membership is within 2 ulp <= 2^-52 of the other side's (both exponentials are within 1 ulp
    of the truth, values <= 1), and the union adds three roundings of quantities <= 2. sigma and the iteration counts in bits on every
    row that is not marginal; for the committed seed the restatement reports no marginal row at all, which is asserted."""
    n_rows = n_marginal = 0
    for case in grid_by_size(sa)[n]:
        name, idx, dist, prm, n_epochs = case
        want, got = restated(case, ref.math_exp_many, "sequential"), twin(sa, case)
        if isinstance(want, ref.Refused):
            assert isinstance(got, tuple) and f"row {want.row} " in got[1], (name, want.row, got)
            continue
        k = idx.shape[1]
        assert same_bits(got["rhos"], want["rhos"]), name
        n_rows += n
        n_marginal += sum(want["marginal"])
        for i in range(n):
            if want["marginal"][i]:
                continue
            raw, it = sa.host_smooth_knn_dist(dist[i], want["rhos"][i], prm["bandwidth"], prm["n_iter"])
            assert it == want["iterations"][i] and same_bits([raw], [want["raw_sigmas"][i]]), (name, i, it, want["iterations"][i])
            if want["rhos"][i] > 0.0:
                assert same_bits([got["sigmas"][i]], [want["sigmas"][i]]), (name, i)
            else:
                assert abs(got["sigmas"][i] - want["sigmas"][i]) <= 2 * n * k * 2.0 ** -53 * abs(want["sigmas"][i]), (name, i)
        (u_ptr, u_idx), (r_ptr, r_idx) = ref.union_pattern_scipy(idx.tolist(), n)
        s_ptr, s_idx = (u_ptr, u_idx) if prm["apply_fuzzy_combine"] else (r_ptr, r_idx)
        assert got["indptr"].tolist() == s_ptr and got["indices"].tolist() == s_idx, name
        assert got["indptr"].tolist() == want["indptr"] and got["indices"].tolist() == want["indices"], name
        both = np.array(want["values"])
        finite = np.isfinite(both) & np.isfinite(got["values"])
        assert np.all(np.isfinite(both) == np.isfinite(got["values"])), name
        assert np.all(np.abs(got["values"][finite] - both[finite]) <= 2.0 ** -50), (name, float(np.max(np.abs(got["values"][finite] - both[finite]))))
    print(f"n = {n}: {n_marginal} marginal rows of {n_rows}")
    assert n_marginal == 0, "choose another seed in tests/fuzzy_cases.py: the restatement reports marginal rows"


def test_psum_folds_v_not_v_minus_rho(sa):
    d, rho = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0], 1.0
    literal = ref.smooth_knn_dist(d, rho, 6, 1.0, 64, lib_exp_many(sa))
    repaired = ref.smooth_knn_dist(d, rho, 6, 1.0, 64, lib_exp_many(sa), repaired=True)
    got = sa.host_smooth_knn_dist(d, rho)
    assert same_bits([got[0]], [literal[0]]) and got[1] == literal[1]
    assert abs(literal[0] - repaired[0]) > 0.1 * literal[0]


def test_the_column_position_is_compared_with_the_index(sa):
    idx, dist = cases.column_is_index()
    with sa.host_fuzzy_simplicial_set(idx, dist, apply_fuzzy_combine=False) as g:
        indptr, indices, values = g.to_csr()
    r = {(row, int(indices[e])): values[e] for row in range(6) for e in range(int(indptr[row]), int(indptr[row + 1]))}
    for i in range(6):
        for j in range(3):
            c = int(idx[i, j])
            if j == c:
                assert r[c, i] == 0.0 and dist[i, j] > 0.0  # a "repaired" self test (i == c) would store exp(..) > 0 or 1 here
            else:
                assert r[c, i] > 0.0
    assert sum(1 for i in range(6) for j in range(3) if idx[i, j] == j) >= 4 and all(idx[i, j] != i for i in range(6) for j in range(3))


def test_an_entry_is_stored_at_row_neighbour_column_i(sa):
    idx = np.array([[1], [2], [1]], dtype=np.uint32)
    dist = np.array([[1.0], [2.0], [3.0]])
    with sa.host_fuzzy_simplicial_set(idx, dist, apply_fuzzy_combine=False) as g:
        indptr, indices, values = g.to_csr()
    assert indptr.tolist() == [0, 0, 2, 3] and indices.tolist() == [0, 2, 1]  # the transposed orientation: [0, 1, 2, 3] / [1, 2, 1]
    with sa.host_fuzzy_simplicial_set(idx, dist) as g:
        indptr, indices, values = g.to_csr()
    assert indptr.tolist() == [0, 1, 3, 4] and indices.tolist() == [1, 0, 2, 1]


def test_the_refusals_name_the_row_and_leave_nothing(sa):
    gc.collect()  # handles an earlier test dropped
    before = sa.device_memory_in_use()
    for name, idx, dist, kw, text in cases.refusal_cases():
        with pytest.raises(sa.ScanrsError) as e:
            h = ctypes.c_void_p()
            prm = sa._fuzzy_params(kw.get("local_connectivity", 1.0), kw.get("set_op_mix_ratio", 1.0), True, 0, 0.0)
            i32, f64 = np.ascontiguousarray(idx, np.uint32), np.ascontiguousarray(dist, np.float64)
            pad_i, pad_d = np.zeros(1, np.uint32), np.zeros(1)  # an empty array still gets an address
            sa._check(sa._lib.scanrs_host_fuzzy_simplicial_set(sa._p(i32 if i32.size else pad_i), sa._p(f64 if f64.size else pad_d),
                                                               ctypes.c_uint64(idx.shape[0]), ctypes.c_uint32(idx.shape[1]), ctypes.byref(prm),
                                                               ctypes.byref(h)))
        assert e.value.code == 6 and text in str(e.value) and h.value is None, (name, str(e.value))
    # n > 2^32 - 2 is refused before an array is looked at
    one_i, one_d, h = np.zeros(1, np.uint32), np.zeros(1), ctypes.c_void_p()
    prm = sa._fuzzy_params(1.0, 1.0, True, 0, 0.0)
    with pytest.raises(sa.ScanrsError, match="2\\^32 - 2"):
        sa._check(sa._lib.scanrs_host_fuzzy_simplicial_set(sa._p(one_i), sa._p(one_d), ctypes.c_uint64(2 ** 32 - 1), ctypes.c_uint32(1),
                                                           ctypes.byref(prm), ctypes.byref(h)))
    with sa.host_fuzzy_simplicial_set([[1], [0]], [[1.0], [1.0]]) as g:
        for bad in (0.0, -1.0, np.nan):
            with pytest.raises(sa.ScanrsError, match="n_epochs"):
                g.edges(bad)
            with pytest.raises(sa.ScanrsError, match="n_epochs"):
                g.edge_count(bad)
        with pytest.raises(sa.ScanrsError, match="host memory"):
            g.device_pointers()
        assert g.edge_count(200.0) == 2
    sa._lib.scanrs_graph_free(None)  # null is a no-op
    assert sa.device_memory_in_use() == before


def test_the_interface_is_declared_mirrored_and_exported(sa):
    hdr = open(os.path.join(ROOT, "include", "scanrs_amd.h")).read()
    hpp = open(os.path.join(ROOT, "include", "scanrs_amd.hpp")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(sa.LIB_PATH)
    for name, cite in NEW_SYMBOLS.items():
        assert re.search(r"\b(int|void) %s\s*\(" % name, code), f"{name} is not declared in scanrs_amd.h"
        assert name in hpp, f"{name} is not mirrored in scanrs_amd.hpp"
        assert name in sa.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"%s \(%s" % (name, cite), hdr), f"{name} does not cite the reference"
    assert "typedef struct scanrs_fuzzy_params" in code and "struct FuzzyParams" in hpp and "class FuzzyGraph" in hpp
    assert not re.search(r"NOT provided: everything after the neighbour lists", hdr)
    mk = open(os.path.join(ROOT, "scan-rs_amd", "csrc", "Makefile")).read()
    assert re.search(r"SRCS_HIP :=.*\bfuzzy\.hip", mk) and re.search(r"SRCS_CPP :=.*\bfuzzy_host\.cpp", mk)
    assert re.search(r"fuzzy\.o \$\(OBJ\)/fuzzy_host\.o: HIPFLAGS \+= -ffp-contract=off", mk)
    for fn in ("fuzzy_simplicial_set", "umap_graph", "umap_graph_device", "host_fuzzy_simplicial_set", "host_fuzzy_exp", "host_smooth_knn_dist",
               "host_membership_strengths"):
        assert callable(getattr(sa, fn)), fn
    for attr in ("shape", "nnz", "to_csr", "sigmas", "rhos", "edges", "close"):
        assert hasattr(sa.FuzzyGraph, attr), attr
