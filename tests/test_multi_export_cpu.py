"""The host side of scanrs_multi_to_adaptive: scanrs_host_plan_export against numpy, the argument checks that need
no device, and that the new source, symbols and mirrors are in place. No device."""
import ctypes
import os
import re

import numpy as np
import pytest

import reshard_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("scanrs_mat_to_adaptive_major", "scanrs_multi_to_adaptive", "scanrs_adaptive_export_multi_info", "scanrs_host_plan_export")
ARGUMENT = 6  # SCANRS_ERR_ARGUMENT
COUNTS = (1, 2, 3, 5, 16)


def edge_tables(n_src):
    """{name: counts (n_src x n_inner)}: the tables on which a plan can go wrong"""
    rng = np.random.default_rng(11 + n_src)
    one_nothing = rng.integers(0, 9, size=(n_src, 37)).astype(np.uint64)
    one_nothing[n_src // 2] = 0  # a source with nothing (the only one, for n_src == 1)
    few = np.zeros((n_src, 29), dtype=np.uint64)
    few[:, 4] = 3  # two nonzero vectors: more destinations than nonzero vectors from n_dst == 3 on
    few[n_src - 1, 17] = 1
    return {"all_zero": np.zeros((n_src, 23), dtype=np.uint64), "one_inner_position": rng.integers(0, 5, size=(n_src, 1)).astype(np.uint64),
            "one_inner_position_empty": np.zeros((n_src, 1), dtype=np.uint64), "a_source_with_nothing": one_nothing,
            "more_destinations_than_vectors": few, "no_inner_position": np.zeros((n_src, 0), dtype=np.uint64)}


def random_tables(n_src):
    rng = np.random.default_rng(101 + n_src)
    out = {}
    for n_inner in (2, 61, 1000):
        c = rng.integers(0, 50, size=(n_src, n_inner)).astype(np.uint64)
        c[rng.random((n_src, n_inner)) < 0.4] = 0
        c[0, n_inner // 2] += 20000  # one heavy vector: the cut falls around it
        out[f"random_{n_inner}"] = c
    return out


def reference_plan(counts, n_dst):
    counts = np.asarray(counts, dtype=np.uint64)
    tip = np.concatenate([[0], np.cumsum(counts.sum(axis=0, dtype=np.uint64), dtype=np.uint64)]).astype(np.uint64)
    sb = reshard_ref.plan_shards(tip, n_dst)
    moved = np.array([[int(counts[s, int(sb[d]):int(sb[d + 1])].sum(dtype=np.uint64)) for d in range(n_dst)] for s in range(counts.shape[0])],
                     dtype=np.uint64).reshape(counts.shape[0], n_dst)
    return tip, sb, moved


@pytest.mark.parametrize("n_src", COUNTS)
def test_host_plan_export_matches_numpy(n_src):
    import scanrs_amd as sa

    tables = dict(edge_tables(n_src), **random_tables(n_src))
    for name, counts in sorted(tables.items()):
        for n_dst in COUNTS:
            where = f"{name}, {n_src} -> {n_dst}"
            tip, sb, mv = sa.host_plan_export(counts, n_dst)
            rtip, rsb, rmv = reference_plan(counts, n_dst)
            assert tip.dtype == sb.dtype == mv.dtype == np.uint64, where
            assert np.array_equal(tip, rtip), where  # out_indptr = cumsum of the column sums
            assert np.array_equal(sb, rsb) and np.array_equal(sb, sa.plan_shards(tip, n_dst)), where
            assert mv.shape == (n_src, n_dst) and np.array_equal(mv, rmv), where  # moved = the block sums
            # every entry lies in exactly one slab
            assert int(mv.sum()) == int(counts.sum()) == int(tip[-1]), where
            assert np.array_equal(mv.sum(axis=0), tip[sb[1:].astype(np.int64)] - tip[sb[:-1].astype(np.int64)]), where
            assert int(sb[0]) == 0 and int(sb[-1]) == counts.shape[1] and np.all(np.diff(sb.astype(np.int64)) >= 0), where


def test_host_plan_export_on_a_hand_case():
    """Numbers worked out by hand: two sources over 4 inner positions, counts [3 0 2 5] and [1 0 0 2]."""
    import scanrs_amd as sa

    counts = [[3, 0, 2, 5], [1, 0, 0, 2]]
    tip, sb, mv = sa.host_plan_export(counts, 2)
    # column sums 4 0 2 7 -> indptr 0 4 4 6 13; floor(13 / 2) = 6: the first entry >= 6 is indptr[3] -> slab 0 holds positions 0 .. 2
    assert tip.tolist() == [0, 4, 4, 6, 13] and sb.tolist() == [0, 3, 4] and mv.tolist() == [[5, 5], [1, 2]]
    tip, sb, mv = sa.host_plan_export(counts, 3)
    # floor(13 / 3) = 4 -> indptr[1]; floor(26 / 3) = 8 -> indptr[4]: the last slab is empty
    assert sb.tolist() == [0, 1, 4, 4] and mv.tolist() == [[3, 7, 0], [1, 2, 0]]


def test_host_plan_export_outputs_may_be_null_and_refusals():
    import scanrs_amd as sa

    lib = sa._lib
    counts = np.array([[1, 2, 3], [4, 5, 6]], dtype=np.uint64)
    p = counts.ctypes.data_as(ctypes.c_void_p)
    tip, sb, mv = np.zeros(4, dtype=np.uint64), np.zeros(3, dtype=np.uint64), np.zeros((2, 2), dtype=np.uint64)

    def call(n_src, n_dst, a=None, b=None, c=None, table=p):
        return lib.scanrs_host_plan_export(table, ctypes.c_uint32(n_src), ctypes.c_uint64(3), ctypes.c_uint32(n_dst),
                                           None if a is None else a.ctypes.data_as(ctypes.c_void_p), None if b is None else b.ctypes.data_as(ctypes.c_void_p),
                                           None if c is None else c.ctypes.data_as(ctypes.c_void_p))

    assert call(2, 2) == 0
    assert call(2, 2, a=tip) == 0 and tip.tolist() == [0, 5, 12, 21]
    assert call(2, 2, b=sb) == 0 and sb.tolist() == [0, 2, 3]
    assert call(2, 2, c=mv) == 0 and mv.tolist() == [[3, 3], [9, 6]]
    for n_src, n_dst, word in ((0, 2, "n_src"), (17, 2, "n_src"), (2, 0, "n_dst"), (2, 17, "n_dst")):
        assert call(n_src, n_dst, a=tip) == ARGUMENT
        assert word in lib.scanrs_last_error().decode()
    assert call(2, 2, table=None) == ARGUMENT and "counts" in lib.scanrs_last_error().decode()
    with pytest.raises(sa.ScanrsError) as e:
        sa.host_plan_export(np.zeros(5, dtype=np.uint64), 2)
    assert e.value.code == ARGUMENT


def test_null_and_out_of_range_arguments_are_refused_without_a_device():
    """major, force_kind and null arguments are checked before any device work: the refusals need no device and no handle that
    could be used (a dummy non-null pointer is never dereferenced)."""
    import scanrs_amd as sa

    lib = sa._lib
    out = ctypes.c_void_p(7)
    dummy = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    for fn in (lib.scanrs_mat_to_adaptive_major, lib.scanrs_multi_to_adaptive):
        assert fn(None, ctypes.c_int(0), ctypes.c_int(-1), ctypes.byref(out)) == ARGUMENT and out.value is None
        assert "null" in lib.scanrs_last_error().decode()
        assert fn(dummy, ctypes.c_int(0), ctypes.c_int(-1), None) == ARGUMENT
        for major in (-1, 2):
            out = ctypes.c_void_p(7)
            assert fn(dummy, ctypes.c_int(major), ctypes.c_int(-1), ctypes.byref(out)) == ARGUMENT and out.value is None
            assert "major" in lib.scanrs_last_error().decode()
        for kind in (-2, 8):
            for major in (0, 1):
                assert fn(dummy, ctypes.c_int(major), ctypes.c_int(kind), ctypes.byref(out)) == ARGUMENT
                assert "force_kind" in lib.scanrs_last_error().decode()
    assert lib.scanrs_adaptive_export_multi_info(None, None, None, None, None) == ARGUMENT
    with pytest.raises(sa.ScanrsError):
        sa._export_major("outer")
    with pytest.raises(sa.ScanrsError):
        sa._export_kind("D5")


def test_sources_symbols_and_mirrors_are_in_place():
    import scanrs_amd as sa

    mk = open(os.path.join(ROOT, "scan-rs_amd", "csrc", "Makefile")).read()
    assert "export_multi.hip" in mk
    hdr = open(os.path.join(ROOT, "include", "scanrs_amd.h")).read()
    hpp = open(os.path.join(ROOT, "include", "scanrs_amd.hpp")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = ctypes.CDLL(sa.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in sa.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert name in hpp and name in integ, name
    assert "SCANRS_EXPORT_STORED = 0" in hdr and "SCANRS_EXPORT_INNER = 1" in hdr
    for key in ("export_plan_us", "export_pull_us", "export_encode_us"):
        assert f'"{key}"' in hdr, key
    for method in ("to_adaptive_vecs", "adaptive_info", "export_info"):
        assert hasattr(sa.MultiMat, method) and hasattr(sa.AdaptiveMat, method), method
    # the pull is written without atomics and guards every source read
    kernel = open(os.path.join(ROOT, "scan-rs_amd", "csrc", "export_multi.hip")).read()
    code = re.sub(r"//.*", "", kernel)
    assert "atomic" not in code and "src.nnz[s]" in code
