"""kNN over a sharded point set without a device: the numpy model of the scheme, tests/knn_sharded_ref.py, against
the restatement of the reference's own oracle (oracle/knn_oracle.py, nn.rs:112-137) on the fixtures the GPU test uses, and the
library's merge rule (scan-rs_amd/csrc/knn_merge.hpp behind scanrs_host_knn_merge, the source the device kernel compiles too)
against the model's merge."""
import ctypes
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import knn_oracle  # noqa: E402
import knn_sharded_ref as ref  # noqa: E402

NEW_SYMBOLS = ("scanrs_knn_sharded", "scanrs_multi_knn", "scanrs_host_knn_merge")


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    return scanrs_amd


def test_the_interface_is_declared_mirrored_and_exported(sa):
    hdr = open(os.path.join(ROOT, "include", "scanrs_amd.h")).read()
    hpp = open(os.path.join(ROOT, "include", "scanrs_amd.hpp")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(sa.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, code), f"{name} is not declared in scanrs_amd.h"
        assert name in hpp, f"{name} is not mirrored in scanrs_amd.hpp"
        assert name in sa.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"%s \(nn\.rs:38-83" % name, hdr), f"{name} does not cite the reference"
    assert '"knn_block_rows"' in hdr and '"knn_blocks"' in hdr and '"knn_allreduces"' in hdr
    assert callable(sa.AdaptiveMat.knn_sharded) and callable(sa.MultiMat.knn) and callable(sa.host_knn_merge)


def test_the_fma_restatement_is_correctly_rounded():
    """fma(t, t, s) of the model against exact rational arithmetic, rounded to nearest even by float(Fraction)."""
    rng = np.random.default_rng(53)
    t = rng.standard_normal(4000) * np.exp2(rng.integers(-20, 20, size=4000))
    s = np.abs(rng.standard_normal(4000)) * np.exp2(rng.integers(-30, 30, size=4000))
    # near-halfway cases: s a power of two, t * t just above or below half an ulp of it
    t[:500] = np.sqrt(np.exp2(-53.0)) * (1.0 + rng.standard_normal(500) * 1e-9)
    s[:500] = 1.0
    got = ref.fma(t, t, s)
    want = np.array([float(Fraction(float(a)) * Fraction(float(a)) + Fraction(float(b))) for a, b in zip(t, s)])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def _oracle(points, k):
    """exhaustive_find_nn pads with u32::MAX when fewer than k other points exist (nn.rs:66)"""
    return knn_oracle.exhaustive_find_nn(points, points, k, include_self=False).astype(np.uint32)


@pytest.mark.parametrize("shards", sorted(ref.LATTICE_CUTS))
@pytest.mark.parametrize("block_rows", ref.LATTICE_BLOCKS)
def test_model_on_the_lattice_equals_the_oracle(shards, block_rows):
    pts = ref.lattice_points()
    assert len(np.unique(pts, axis=0)) < ref.LATTICE_N  # exact duplicates
    for k in ref.LATTICE_K:
        got, dist = ref.knn_sharded_model(pts, ref.LATTICE_CUTS[shards], block_rows, k)
        assert np.array_equal(got, _oracle(pts, k))
        one, dist1 = ref.knn_one_pass(pts, k)
        assert np.array_equal(got, one) and np.array_equal(dist, dist1)
        assert np.array_equal(dist, ref.sq_dist_pairs(pts, got))
        # equidistant neighbours in ascending global index
        for row_d, row_i in zip(dist, got.astype(np.int64)):
            assert np.all((np.diff(row_d) > 0) | ((np.diff(row_d) == 0) & (np.diff(row_i) > 0)))


def test_cuts_have_a_shard_with_fewer_points_than_k():
    for shards, cuts in ref.LATTICE_CUTS.items():
        assert cuts[0] == 0 and cuts[-1] == ref.LATTICE_N and len(cuts) == shards + 1
        if shards > 1:
            assert 2 in np.diff(cuts)
    plans = {b: ref.block_plan(ref.LATTICE_N, b) for b in ref.LATTICE_BLOCKS}
    assert len(plans[1000]) == 1 and plans[7][-1] == (91, 97) and len(plans[32]) == 4
    assert any(lo <= b0 and b1 <= hi for b0, b1 in plans[32] for lo, hi in zip(ref.LATTICE_CUTS[2][:-1], ref.LATTICE_CUTS[2][1:]))


def test_model_pads_when_fewer_than_k_other_points_exist():
    pts = ref.padding_points()
    got, dist = ref.knn_sharded_model(pts, ref.PADDING_CUTS, 4, ref.PADDING_K)
    assert np.array_equal(got, _oracle(pts, ref.PADDING_K))
    assert np.all(got[:, ref.PADDING_N - 1:] == ref.U32MAX) and np.all(np.isinf(dist[:, ref.PADDING_N - 1:]))
    for q in range(ref.PADDING_N):
        assert q not in got[q] and sorted(got[q, : ref.PADDING_N - 1]) == [i for i in range(ref.PADDING_N) if i != q]


def test_model_excludes_the_global_row_only():
    pts = ref.duplicated_points()
    h = ref.DUP_HALF
    got, dist = ref.knn_sharded_model(pts, [0, h, 2 * h], 10, 3)
    assert np.array_equal(got, _oracle(pts, 3))
    for q in range(2 * h):
        assert got[q, 0] == (q + h) % (2 * h) and dist[q, 0] == 0.0 and q not in got[q]


@pytest.mark.parametrize("case", ref.merge_cases(), ids=lambda c: c[0])
def test_host_knn_merge_equals_the_model(sa, case):
    _, da, ia, db, ib = case
    real_a, real_b = ia[ia != ref.U32MAX], ib[ib != ref.U32MAX]
    assert not set(real_a.tolist()) & set(real_b.tolist())  # the same index never in both lists
    want_d, want_i = ref.merge(da, ia, db, ib)
    for (xa, ya, xb, yb) in ((da, ia, db, ib), (db, ib, da, ia)):  # the rule is symmetric in its two lists
        got_d, got_i = sa.host_knn_merge(xa, ya, xb, yb)
        assert got_i.dtype == np.uint32 and np.array_equal(got_i, want_i)
        assert np.array_equal(got_d.view(np.uint64), want_d.view(np.uint64))


def test_host_knn_merge_refuses_k_above_128(sa):
    d, i = np.arange(129, dtype=np.float64), np.arange(129, dtype=np.uint32)
    with pytest.raises(sa.ScanrsError) as e:
        sa.host_knn_merge(d, i, d + 0.5, i + 1000)
    assert e.value.code == 6
