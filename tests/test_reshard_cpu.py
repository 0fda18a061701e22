"""The host side of the inner-sharding constructors: scanrs_host_plan_inner against the numpy restatement of
tests/reshard_ref.py, its refusals, and that the new sources, symbols and mirrors are in place. No device."""
import os
import re

import numpy as np
import pytest

import reshard_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("scanrs_multi_create_inner", "scanrs_multi_create_adaptive_inner", "scanrs_multi_create_from_file", "scanrs_multi_create_info",
               "scanrs_host_plan_inner")


@pytest.mark.parametrize("world", ref.SHARDS + (16,))
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_host_plan_matches_reference(name, world):
    import scanrs_amd as sa

    n_outer, n_inner, indptr, indices, _ = ref.CASES[name]()
    sb, bd, mv = sa.host_plan_inner(indptr, indices, n_inner, world)
    rsb, rbd, rmv = ref.plan_inner(indptr, indices, n_inner, world)
    assert np.array_equal(sb, rsb) and np.array_equal(bd, rbd) and np.array_equal(mv, rmv)
    # the ranges are what scanrs_plan_shards gives for the two indptr arrays, and every stored entry is moved exactly once
    t_indptr, _, _ = ref.transposed_triplet(indptr, indices, np.ones(indices.size, dtype=np.uint32), n_outer, n_inner)
    assert np.array_equal(sb, sa.plan_shards(indptr, world)) and np.array_equal(bd, sa.plan_shards(t_indptr, world))
    assert int(mv.sum()) == indices.size
    assert np.array_equal(mv.sum(axis=1), indptr[sb[1:].astype(np.int64)] - indptr[sb[:-1].astype(np.int64)])
    assert np.array_equal(mv.sum(axis=0), t_indptr[bd[1:].astype(np.int64)] - t_indptr[bd[:-1].astype(np.int64)])


def test_host_plan_reference_on_a_hand_case():
    """The restatement itself, on numbers worked out by hand: 2 vectors over 4 positions, entries at (0: 0 1 3), (1: 1 2)."""
    indptr, indices = [0, 3, 5], [0, 1, 3, 1, 2]
    sb, bd, mv = ref.plan_inner(indptr, indices, 4, 2)
    # floor(5 / 2) = 2 entries: the first indptr entry >= 2 is indptr[1] = 3 -> slab 0 is vector 0; per position 1 2 1 1 -> prefix
    # 0 1 3 4 5: the first >= 2 is at 2 -> shard 0 owns positions 0 and 1
    assert sb.tolist() == [0, 1, 2] and bd.tolist() == [0, 2, 4] and mv.tolist() == [[2, 1], [1, 1]]


def test_host_plan_refusals():
    import scanrs_amd as sa

    indptr = np.array([0, 2, 4], dtype=np.uint64)
    ok = np.array([0, 3, 1, 2], dtype=np.uint32)
    sa.host_plan_inner(indptr, ok, 4, 2)
    message = "indices must be in range and strictly ascending within each outer vector"
    for bad in ([0, 3, 2, 1], [0, 3, 2, 2], [0, 4, 1, 2]):  # unsorted, repeated, out of range
        with pytest.raises(sa.ScanrsError) as e:
            sa.host_plan_inner(indptr, np.array(bad, dtype=np.uint32), 4, 2)
        assert e.value.code == 6 and message in str(e.value)
    with pytest.raises(sa.ScanrsError) as e:
        sa.host_plan_inner(indptr, ok, 4, 0)
    assert e.value.code == 6 and "world" in str(e.value)
    with pytest.raises(sa.ScanrsError) as e:
        sa.host_plan_inner(np.array([1, 2, 4], dtype=np.uint64), ok, 4, 2)
    assert e.value.code == 6 and "indptr[0] must be 0" in str(e.value)
    with pytest.raises(sa.ScanrsError) as e:
        sa.host_plan_inner(np.array([0, 3, 2, 4], dtype=np.uint64), ok, 4, 2)  # a decreasing indptr
    assert e.value.code == 6 and message in str(e.value)
    with pytest.raises(sa.ScanrsError) as e:
        sa.host_plan_inner(indptr, ok, 2**32 + 1, 2)
    assert "dimensions must fit in u32" in str(e.value)


def test_sources_symbols_and_mirrors():
    import scanrs_amd as sa

    mk = open(os.path.join(ROOT, "scan-rs_amd", "csrc", "Makefile")).read()
    assert "reshard.hip" in re.search(r"^SRCS_HIP := (.*)$", mk, re.M).group(1).split()
    assert "reshard_host.cpp" in re.search(r"^SRCS_CPP := (.*)$", mk, re.M).group(1).split()
    header = open(os.path.join(ROOT, "include", "scanrs_amd.h")).read()
    hpp = open(os.path.join(ROOT, "include", "scanrs_amd.hpp")).read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header, name
        assert name in hpp, f"{name} is not mirrored in scanrs_amd.hpp"
        assert name in sa.EXPORTED_SYMBOLS and hasattr(sa._lib, name), name
    for name in ("from_csmat_inner", "from_adaptive_vecs_inner", "from_file", "create_info"):
        assert callable(getattr(sa.MultiMat, name)), name
        assert name in hpp, name
    assert callable(sa.host_plan_inner) and "host_plan_inner" in hpp and "to_devices" in hpp
    from scanrs_amd import hdf5_io

    assert callable(hdf5_io.FeatureBarcodeMatrix.to_devices)
    cli = open(os.path.join(ROOT, "tools", "scan_rs_cmd.cpp")).read()
    assert "--gpus" in cli and "--devices" in cli
