"""The seeded fixture of the sharded-DE tests (tests/test_gpu_sseq_sharded.py, tests/test_sseq_sharded_cpu.py) and the split of its
tests between the exact and the asymptotic branch as the restatement tests/sseq_ref.py makes it.

67 genes x 203 cells. Counts are mostly 1 .. 15 with a heavy tail (one nonzero in twelve is 40 .. 4000), and five hot genes are nearly
dense, so that several (gene, group) sums pass `big_count` on both sides. Cells 7, 100 and 202 hold no nonzero (size factor 0), gene 13
holds none. Labels are -1 .. 4 for n_groups = 6: group 5 is empty, group 3 lies inside the first 40 cells (a shard behind them holds
none of it), about a tenth of the cells is in no group."""
import numpy as np
from scipy import sparse

GENES, CELLS, N_GROUPS = 67, 203, 6
EMPTY_CELLS, EMPTY_GENE = (7, 100, 202), 13
HOT_GENES = (0, 1, 2, 3, 4)
BIG_COUNTS = (None, 60)  # the default (900) and a low bound that sends many more tests to the asymptotic branch
SEED = 20260


def make_case():
    rng = np.random.default_rng(SEED)
    dense = np.zeros((GENES, CELLS), dtype=np.int64)
    mask = rng.random((GENES, CELLS)) < 0.3
    mask[list(HOT_GENES), :] = rng.random((len(HOT_GENES), CELLS)) < 0.9
    small = rng.integers(1, 16, (GENES, CELLS))
    tail = rng.integers(40, 4001, (GENES, CELLS))
    dense[mask] = np.where(rng.random((GENES, CELLS)) < 1.0 / 12.0, tail, small)[mask]
    dense[:, list(EMPTY_CELLS)] = 0
    dense[EMPTY_GENE, :] = 0
    labels = rng.choice(np.array([0, 1, 2, 4]), CELLS).astype(np.int16)
    first = rng.choice(np.array([0, 1, 2, 3, 4]), 40, p=[0.15, 0.15, 0.15, 0.4, 0.15]).astype(np.int16)
    labels[:40] = first
    labels[rng.random(CELLS) < 0.1] = -1
    mat = sparse.csc_matrix(dense.astype(np.uint32))
    mat.sort_indices()
    # an unsorted subset of the cells that no range of 10 consecutive cells escapes (it crosses every shard boundary), and UMI counts
    subset = rng.permutation(CELLS)[:150].astype(np.uint64)
    umi_all = rng.uniform(50.0, 4000.0, CELLS)
    umi_subset = rng.uniform(50.0, 4000.0, len(subset))
    return dict(mat=mat, labels=labels, subset=subset, umi_all=umi_all, umi_subset=umi_subset)


def n_tests(mode):
    return N_GROUPS if mode == 0 else 1 if mode == 1 else N_GROUPS - 1


def sides_of_tests(labels, mode):
    """(cells of side a, cells of side b) per test of a mode (0: each group against the rest, 1: group 0 against group 1, 2: each group
    1 .. against group 0)."""
    labels = np.asarray(labels)
    if mode == 0:
        return [(np.flatnonzero(labels == j), np.flatnonzero((labels >= 0) & (labels != j))) for j in range(N_GROUPS)]
    if mode == 1:
        return [(np.flatnonzero(labels == 0), np.flatnonzero(labels == 1))]
    return [(np.flatnonzero(labels == j), np.flatnonzero(labels == 0)) for j in range(1, N_GROUPS)]


def branch_counts(mat, labels, params, mode, big_count):
    """How the restatement (sseq_ref.de_from_sums) splits the genes x tests grid: (asymptotic, exact with a test to compute, settled at
    p = 1 by nb_exact_test's early returns)."""
    big = 900 if big_count is None else big_count
    mat = sparse.csc_matrix(mat)
    sf, use, phi = params["size_factors"], params["use_genes"], params["gene_phi"]
    asym = exact = settled = 0
    for a, b in sides_of_tests(labels, mode):
        fa, fb = float(np.sum(sf[a])), float(np.sum(sf[b]))
        sa = np.asarray(mat[:, a].sum(axis=1)).ravel()
        sb = np.asarray(mat[:, b].sum(axis=1)).ravel()
        for g in range(mat.shape[0]):
            if use[g] and sa[g] > big and sb[g] > big:
                asym += 1
            elif sa[g] + sb[g] == 0 or phi[g] == 0.0 or fa == 0.0 or fb == 0.0:
                settled += 1
            else:
                exact += 1
    return asym, exact, settled
