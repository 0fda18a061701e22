"""The host side of scanrs_multi_gather_outer / scanrs_multi_rebalance: scanrs_host_plan_gather against the numpy
restatement of tests/regather_ref.py, the argument checks of the five entry points, and that the new sources, symbols and mirrors are
in place. No device."""
import ctypes
import os
import re

import numpy as np
import pytest

import regather_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("scanrs_multi_gather_outer", "scanrs_multi_rebalance", "scanrs_multi_balance", "scanrs_multi_gather_info", "scanrs_host_plan_gather")
ARGUMENT = 6  # SCANRS_ERR_ARGUMENT, and SCANRS_ERR_INVALID under its other name


@pytest.mark.parametrize("n_src", ref.SHARDS)
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_host_plan_matches_reference(name, n_src):
    import scanrs_amd as sa

    n_outer, _, indptr, indices, data = ref.CASES[name]()
    src_bounds = sa.plan_shards(indptr, n_src)
    for list_name, idx in ref.lists(n_outer, src_bounds).items():
        for n_dst in ref.SHARDS + (16,):
            tip, bd, mv = sa.host_plan_gather(indptr, src_bounds, idx, n_dst)
            rtip, rbd, rmv = ref.plan_gather(indptr, src_bounds, idx, n_dst)
            where = f"{list_name}, {n_src} -> {n_dst}"
            assert np.array_equal(tip, rtip) and np.array_equal(bd, rbd) and np.array_equal(mv, rmv), where
            # the indptr is the selected triplet's, the cut is scanrs_plan_shards of it, and every nonzero is moved exactly once
            assert np.array_equal(tip, ref.select_outer(indptr, indices, data, idx)[0]) and np.array_equal(bd, sa.plan_shards(tip, n_dst)), where
            assert np.array_equal(mv.sum(axis=0), tip[bd[1:].astype(np.int64)] - tip[bd[:-1].astype(np.int64)]), where
            assert mv.shape == (n_src, n_dst) and int(mv.sum()) == int(tip[-1]), where


def test_host_plan_on_a_hand_case():
    """Numbers worked out by hand: 4 vectors of 3, 0, 2 and 5 entries on two source shards [0, 2) and [2, 4); the list 3 0 0 2."""
    import scanrs_amd as sa

    indptr, src_bounds, idx = [0, 3, 3, 5, 10], [0, 2, 4], [3, 0, 0, 2]
    for plan in (sa.host_plan_gather, ref.plan_gather):
        tip, bd, mv = plan(indptr, src_bounds, idx, 2)
        # lengths 5 3 3 2 -> indptr 0 5 8 11 13; floor(13 / 2) = 6: the first entry >= 6 is indptr[2] = 8 -> shard 0 holds vectors 0, 1
        # (5 entries from source shard 1, 3 from shard 0), shard 1 holds vectors 2, 3 (3 from shard 0, 2 from shard 1)
        assert tip.tolist() == [0, 5, 8, 11, 13] and bd.tolist() == [0, 2, 4] and mv.tolist() == [[3, 3], [5, 2]]
    # an identity list over source ranges that a filter left behind: the middle shard is empty
    tip, bd, mv = sa.host_plan_gather(indptr, [0, 3, 3, 4], [0, 1, 2, 3], 2)
    assert tip.tolist() == indptr and bd.tolist() == [0, 3, 4] and mv.tolist() == [[5, 0], [0, 0], [0, 5]]
    assert all(np.array_equal(a, b) for a, b in zip((tip, bd, mv), ref.plan_gather(indptr, [0, 3, 3, 4], [0, 1, 2, 3], 2)))


def _err(lib):
    return lib.scanrs_last_error().decode()


def test_host_plan_refusals():
    import scanrs_amd as sa

    lib = sa._lib
    indptr, sb = np.array([0, 3, 3, 5, 10], dtype=np.uint64), np.array([0, 2, 4], dtype=np.uint64)
    with pytest.raises(sa.ScanrsError) as e:
        sa.host_plan_gather(indptr, sb, [0, 4], 2)  # one past the last vector
    assert e.value.code == ARGUMENT and "idx" in str(e.value) and "entry 1 of the list is 4" in str(e.value) and "4 outer vectors" in str(e.value)
    with pytest.raises(sa.ScanrsError) as e:
        sa.host_plan_gather(indptr, sb, [-1], 2)
    assert e.value.code == ARGUMENT and "idx" in str(e.value)
    for n_dst in (0, 17):
        with pytest.raises(sa.ScanrsError) as e:
            sa.host_plan_gather(indptr, sb, [0], n_dst)
        assert e.value.code == ARGUMENT and "n_shards" in str(e.value)
    for bad in ([0, 2, 3], [1, 2, 4], [0, 3, 2, 4]):  # short of the extent, not from 0, descending
        with pytest.raises(sa.ScanrsError) as e:
            sa.host_plan_gather(indptr, bad, [0], 2)
        assert e.value.code == ARGUMENT and "src_bounds" in str(e.value)
    with pytest.raises(sa.ScanrsError) as e:
        sa.host_plan_gather([0, 3, 2, 5, 10], sb, [0], 2)
    assert e.value.code == ARGUMENT and "indptr" in str(e.value)
    # the C entry point itself: null arrays
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    idx, out = np.zeros(2, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    u64, u32 = ctypes.c_uint64, ctypes.c_uint32
    assert lib.scanrs_host_plan_gather(None, u64(4), p(sb), u32(2), p(idx), u64(2), u32(2), p(out), None, None) == ARGUMENT and "indptr" in _err(lib)
    assert lib.scanrs_host_plan_gather(p(indptr), u64(4), None, u32(2), p(idx), u64(2), u32(2), p(out), None, None) == ARGUMENT and "src_bounds" in _err(lib)
    assert lib.scanrs_host_plan_gather(p(indptr), u64(4), p(sb), u32(2), None, u64(2), u32(2), p(out), None, None) == ARGUMENT and "idx" in _err(lib)
    assert lib.scanrs_host_plan_gather(p(indptr), u64(4), p(sb), u32(2), None, u64(0), u32(2), p(out), None, None) == 0  # an empty list may be null
    assert out[0] == 0


def test_argument_checks_of_the_multi_entry_points():
    """What needs no device: a null handle and a null output are refused with the code and a message that names the argument, and a
    refused call leaves a NULL output behind."""
    import scanrs_amd as sa

    lib = sa._lib
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    idx = np.zeros(4, dtype=np.uint64)
    u64, u32 = ctypes.c_uint64, ctypes.c_uint32
    some = ctypes.c_void_p(0x1234)  # never dereferenced: the output is checked first
    out = ctypes.c_void_p(0x1234)
    assert lib.scanrs_multi_gather_outer(None, p(idx), u64(4), u32(2), None, ctypes.byref(out)) == ARGUMENT
    assert "mm" in _err(lib) and "null handle" in _err(lib) and out.value is None
    assert lib.scanrs_multi_gather_outer(some, p(idx), u64(4), u32(2), None, None) == ARGUMENT and "out" in _err(lib) and "null output" in _err(lib)
    out = ctypes.c_void_p(0x1234)
    assert lib.scanrs_multi_rebalance(None, u32(0), None, ctypes.byref(out)) == ARGUMENT
    assert "mm" in _err(lib) and "null handle" in _err(lib) and out.value is None
    assert lib.scanrs_multi_rebalance(some, u32(0), None, None) == ARGUMENT and "out" in _err(lib) and "null output" in _err(lib)
    nnz, imb = np.zeros(4, dtype=np.uint64), ctypes.c_double()
    assert lib.scanrs_multi_balance(None, p(nnz), ctypes.byref(imb)) == ARGUMENT and "mm" in _err(lib) and "null handle" in _err(lib)
    n_src = u32()
    assert lib.scanrs_multi_gather_info(None, ctypes.byref(n_src), None, None, None) == ARGUMENT and "mm" in _err(lib) and "null handle" in _err(lib)


def test_sources_symbols_and_mirrors():
    import scanrs_amd as sa

    mk = open(os.path.join(ROOT, "scan-rs_amd", "csrc", "Makefile")).read()
    assert "regather.hip" in re.search(r"^SRCS_HIP := (.*)$", mk, re.M).group(1).split()
    assert "regather_host.cpp" in re.search(r"^SRCS_CPP := (.*)$", mk, re.M).group(1).split()
    header = open(os.path.join(ROOT, "include", "scanrs_amd.h")).read()
    hpp = open(os.path.join(ROOT, "include", "scanrs_amd.hpp")).read()
    lib = ctypes.CDLL(sa.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header, name
        assert name + "(" in hpp, f"{name} is not mirrored in scanrs_amd.hpp"
        assert name in sa.EXPORTED_SYMBOLS and hasattr(lib, name), name
    for name in ("gather_outer", "rebalance", "balance", "gather_info"):
        assert callable(getattr(sa.MultiMat, name)), name
        assert re.search(r"\b" + name + r"\(", hpp), name
    assert callable(sa.host_plan_gather) and "host_plan_gather(" in hpp
    import inspect

    # the select calls keep the signatures tests/test_select_sharded_cpu.py pins; "through rebalance(), the intermediate freed" is a
    # keyword of rebalance() itself
    assert inspect.signature(sa.MultiMat.rebalance).parameters["consume"].default is False
    assert inspect.signature(sa.MultiMat.partition_on_thresholds) == inspect.signature(sa.AdaptiveMat.partition_on_thresholds)
    counters = sa.counter_names()  # the table of scan-rs_amd/csrc/options.cpp, as the library holds it
    for phase in ("plan", "pull", "finish"):
        assert f"regather_{phase}_us" in counters and f"regather_{phase}_us" in header, phase


def test_the_header_says_what_is_lifted_and_what_stays_out_of_scope():
    header = open(os.path.join(ROOT, "include", "scanrs_amd.h")).read()
    block = header[header.index("---- rebalance and any-order outer selection"):header.index("int scanrs_host_plan_gather(")]
    doc = " ".join(block.replace("*", " ").split())
    for word in ("DESIGN.md §7n", "ANY order", "repeats", "scanrs_multi_rebalance", "scanrs_multi_gather_outer", "scanrs_multi_create", "bit for bit",
                 "either order", "not modified", "host link", "peer", "identity map", "2^31 - 1", "SCANRS_ERR_INVALID", "SCANRS_ERR_ARGUMENT",
                 "before any device work", "NULL", "n_idx == 0", "host_bytes"):
        assert word in doc, word
    scope = doc[doc.index("Still out of scope:"):]
    assert "to_adaptive of a whole scanrs_multi" in scope and "RCCL" in scope and "host hook" in scope
    # the restrictions stay where they are for the select calls, and the inner-sharding block no longer lists rebalancing as missing
    multi = " ".join(header[header.index("int scanrs_multi_shape("):header.index("int scanrs_multi_select_rows(")].replace("*", " ").split())
    assert "NOT rebalanced" in multi and "must not descend" in multi
    inner = " ".join(header[header.index("---- cell-sharded scanrs_multi from feature-major input"):header.index("int scanrs_multi_create_inner(")]
                     .replace("*", " ").split())
    not_served = inner[inner.index("Not served:"):]
    assert "rebalancing an existing" not in not_served and "scanrs_multi_rebalance" in not_served
