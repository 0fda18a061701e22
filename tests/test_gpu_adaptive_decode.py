"""The AdaptiveVec decoder on the device (scan-rs_amd/csrc/decode.hip, scanrs_mat_create_adaptive) against `iter()` of the oracle
(oracle/adaptive_vec.py, the reference's AbsIter). Every table is made by the oracle's constructors, never by the device encoder, so
forced encodings, the lengths at the layouts' edges and vectors no encoder emits are decoded too. Integer work: every comparison is
equality. The tables are those of tests/construct_ref.py, whose properties tests/test_construct_cpu.py checks."""
import gc
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
for p in (ROOT, os.path.join(ROOT, "oracle"), TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

import adaptive_vec as av  # noqa: E402
import construct_ref as cr  # noqa: E402

ORDER = "indices must be in range and strictly ascending within each outer vector"
ARGUMENT, SHAPE = 6, 1


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def in_use(sa):
    gc.collect()
    sa.release_cached_memory()
    return sa.device_memory_in_use()


def decode_both_flags(sa, vecs, length, where):
    """The table decoded as the rows of a CSR and as the columns of a CSC matrix: to_csmat() and nnz() against the oracle's iter()."""
    want = cr.decoded(vecs)
    pieces = [v.pieces() for v in vecs]
    n = len(vecs)
    for storage, rows, cols in ((sa.CSR, n, length), (sa.CSC, length, n)):
        h = sa.AdaptiveMat.from_adaptive_vecs(rows, cols, storage, pieces)
        assert h.shape() == [rows, cols] and h.storage() == storage, where
        assert h.nnz() == want[1].shape[0], (where, storage)
        got = h.to_csmat()
        assert same(got, want), (where, storage, [int(x) for x in np.nonzero(got[0] != want[0])[0][:5]])
    return want


@pytest.mark.parametrize("length", cr.DECODE_LENGTHS)
def test_every_forced_kind_decodes_to_the_oracles_iter(sa, length):
    grid = cr.decode_grid()[length]
    for kind in av.KINDS:
        vecs = [av.AdaptiveVec.with_kind(kind, length, v, i) for i, v in grid]
        assert len(vecs) == 25
        want = decode_both_flags(sa, vecs, length, (length, kind))
        assert want[1].shape[0] == sum(i.shape[0] for i, _ in grid)  # the grid stores no zeros: nothing is lost on the way


def test_mixed_table_of_all_kinds_with_empty_vectors(sa):
    vecs, _ = cr.mixed_table()
    want = decode_both_flags(sa, vecs, cr.MIXED_LENGTH, "mixed")
    assert want[1].shape[0] > 100000


def test_vectors_no_encoder_emits(sa):
    named = cr.foreign_vectors()
    vecs = [v for _, v in named]
    want = decode_both_flags(sa, vecs, vecs[0].length, "foreign")
    lens = np.diff(want[0].astype(np.int64))
    for (name, _), n in zip(named, lens):  # a vector of nothing but stored zeros or orphaned fields: equal indptr neighbours
        assert (n == 0) == name.startswith("only"), name
    for name, v in named:  # and every vector alone: first and last vector of its own table
        decode_both_flags(sa, [v], v.length, name)


@pytest.mark.parametrize("n_shards", [1, 3])
def test_sharded_decoder_call(sa, n_shards):
    vecs, _ = cr.mixed_table()
    n, length = len(vecs), cr.MIXED_LENGTH
    want = cr.transpose(n, length, *cr.decoded(vecs))
    mm = sa.MultiMat.from_adaptive_vecs_inner(n, length, sa.CSR, [v.pieces() for v in vecs], n_shards, devices=[0] * n_shards)
    assert mm.storage == sa.CSC and mm.shape() == [n, length] and mm.n_shards == n_shards
    assert mm.nnz() == want[1].shape[0] and same(mm.to_csmat(), want)
    mm.close()


def test_refusals_leave_no_device_memory(sa):
    length = 300
    rng = np.random.default_rng(5)
    idx = np.sort(rng.choice(length, size=60, replace=False)).astype(np.uint32)
    idx[-1] = 299  # the last entry lies in the second 256-index block
    val = rng.integers(1, 100000, size=60).astype(np.uint32)

    def pieces(of, **change):
        p = dict(av.AdaptiveVec.with_kind(of, length, val, idx).pieces())
        p.update(change)
        return p

    good = [pieces(k) for k in av.KINDS]
    assert same(sa.AdaptiveMat.from_adaptive_vecs(8, length, sa.CSR, good).to_csmat(),
                cr.decoded([av.AdaptiveVec.with_kind(k, length, val, idx) for k in av.KINDS]))
    before = in_use(sa)

    def refused(bad, code, text, storage=None, inner=length):
        """the malformed vector first, last and between sound ones, in both flags"""
        for table in ([bad] + good, good + [bad], good[:3] + [bad] + good[3:]):
            for st in ((sa.CSR, sa.CSC) if storage is None else (storage,)):
                n = len(table)
                with pytest.raises(sa.ScanrsError) as e:
                    sa.AdaptiveMat.from_adaptive_vecs(*((n, inner) if st == sa.CSR else (inner, n)), st, table)
                assert e.value.code == code and text in str(e.value), (str(e.value), text)
                assert in_use(sa) == before, text

    refused(pieces("D8", kind=8), ARGUMENT, "unknown AdaptiveVec encoding")
    refused(good[2], SHAPE, "length of the inner dimension", inner=length + 1)  # (every vector of the table: len != inner dimension)
    refused(pieces("D8", len=length - 1, n_units=length - 1), SHAPE, "length of the inner dimension")
    for kind in ("D3", "D4", "D8", "D16"):
        refused(pieces(kind, n_units=length - 1), SHAPE, "one field per position")
        refused(pieces(kind, n_units=length + 1), SHAPE, "one field per position")
        refused(pieces(kind, data=good[av.KIND_CODE[kind]]["data"][:-1]), ARGUMENT, "data buffer too short")
    for kind in ("S3", "S4", "S8"):
        g = good[av.KIND_CODE[kind]]
        refused(pieces(kind, data=g["data"][:-1]), ARGUMENT, "data buffer too short")
        refused(pieces(kind, block_starts=g["block_starts"][:-1]), ARGUMENT, "block_starts must hold")
        first, last = g["block_starts"].copy(), g["block_starts"].copy()
        first[0], last[-1] = 1, 59
        refused(pieces(kind, block_starts=first), ARGUMENT, "block_starts must run from 0")
        refused(pieces(kind, block_starts=last), ARGUMENT, "block_starts must run from 0")
    refused(pieces("V", n_units=59), SHAPE, "n_units must equal")
    refused(pieces("V", n_units=61), SHAPE, "n_units must equal")
    # a position beyond the vector: counted by the kernels, nothing is read or written outside a buffer
    beyond = idx.copy()
    beyond[-1] = length
    refused(pieces("V", fallback_indexes=beyond), ARGUMENT, "position beyond its length")
    byte = good[7]["index_bytes"].copy()
    assert int(good[7]["block_starts"][1]) <= 59 and byte[-1] == 299 - 256
    byte[-1] = 200  # block 1, byte 200: position 456 of 300
    refused(pieces("S8", index_bytes=byte), ARGUMENT, "position beyond its length")
    # descending positions in V decode as they stand; the validation that follows refuses them
    down = idx.copy()
    down[30], down[31] = down[31], down[30]
    refused(pieces("V", fallback_indexes=down), ARGUMENT, ORDER)
    twice = idx.copy()
    twice[1] = twice[0]
    refused(pieces("V", fallback_indexes=twice), ARGUMENT, ORDER)
