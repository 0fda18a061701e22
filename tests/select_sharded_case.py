"""The fixtures of tests/test_select_sharded_cpu.py and tests/test_gpu_select_sharded.py: tiny genes x cells count
matrices on which a sharded partition_on_thresholds can go wrong, with what tests/select_ref.py gives on them. Everything is an
integer; every comparison made with these is exact."""
import numpy as np
from scipy import sparse

import select_ref as sref

GENES, CELLS = 61, 157
SEED = 20261
NNZ = 948
THIN = (40, 70)  # cells thinned to density 0.02 with count 1: they fall below a small column threshold
EMPTY_CELLS, EMPTY_GENE = (3, 156), 17
N_GROUPS = 4

# (row threshold, col threshold) -> (rounds, excluded rows, excluded columns) of select_ref.partition_sets
SEEDED_CASES = {
    (34, 13): (6, 17, 66),        # several rounds, a partial result
    (36, 14): (6, GENES, CELLS),  # total collapse
    (3, 3): (2, 1, 30),
    (None, 8): (2, 0, 35),        # one threshold only, on each side
    (20, None): (2, 1, 0),
}

CASCADE_N, CASCADE_THRESHOLD = 12, 10  # 15 x 15, 13 rounds, rows and columns 0..11 fall one per round


def seeded_matrix():
    """61 genes x 157 cells, density 0.12, counts 1..5; cells 40..69 thinned; cells 3 and 156 and gene 17 empty. Canonical CSR."""
    rng = np.random.default_rng(SEED)
    mask = rng.random((GENES, CELLS)) < 0.12
    vals = rng.integers(1, 6, size=(GENES, CELLS))
    thin = rng.random((GENES, THIN[1] - THIN[0])) < 0.02
    a = np.where(mask, vals, 0)
    a[:, THIN[0]:THIN[1]] = thin.astype(np.int64)
    a[:, list(EMPTY_CELLS)] = 0
    a[EMPTY_GENE, :] = 0
    return sref.canonical(sparse.csr_matrix(a.astype(np.int64)))


def seeded_labels():
    """One group label per cell (-1: in no group), for the group sums over a filtered matrix."""
    rng = np.random.default_rng(SEED + 1)
    return rng.integers(-1, N_GROUPS, size=CELLS).astype(np.int16)


def cascade():
    """(15 x 15 canonical CSR, threshold, rounds, the rows = columns that fall)."""
    a, gone_r, gone_c, rounds = sref.cascade_matrix(CASCADE_N, CASCADE_THRESHOLD)
    assert np.array_equal(gone_r, gone_c)
    return sref.canonical(sparse.csr_matrix(a)), float(CASCADE_THRESHOLD), rounds, gone_r


def allreduce_bound(rounds, inner_threshold_given, outer_threshold_given):
    """The bound of DESIGN.md §7h on the exchange steps of one sharded partition: per round one all-reduce of the sums along the
    replicated (inner) dimension if it has a threshold and one of the round's flag if the sharded (outer) dimension has one, plus
    one for the mask of the sharded dimension at the end."""
    return rounds * (int(inner_threshold_given) + int(outer_threshold_given)) + 1
