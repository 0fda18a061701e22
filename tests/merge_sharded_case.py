"""The fixtures of tests/test_gpu_merge_sharded.py: the planted-clusters construction of tests/test_gpu_merge_clusters.py (rebuilt
here: test files are not imported), and a medoid case whose clusters sit where a cut of the cells over shards can go wrong."""
import numpy as np
from scipy import sparse

SHARDS = (1, 2, 3, 5)


def planted(sizes, splits, genes, d, seed, marker_genes=30, effect=4.0):
    """Populations with their own expression profile (marker genes up by `effect`) and their own score centre; population p is
    cut into splits[p] labels along its first score coordinate. Returns (genes x cells CSR u32, cells x d scores, labels)."""
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    pop = np.repeat(np.arange(len(sizes)), sizes)
    base = rng.gamma(0.6, 0.5, genes)
    prof = np.tile(base, (len(sizes), 1))
    for p in range(len(sizes)):
        prof[p, rng.choice(genes, marker_genes, replace=False)] *= effect
    lib = rng.lognormal(0.0, 0.3, n)
    counts = rng.poisson(prof[pop].T * lib).astype(np.uint32)  # genes x cells
    centres = rng.standard_normal((len(sizes), d)) * 8.0
    scores = centres[pop] + rng.standard_normal((n, d))
    labels = np.zeros(n, dtype=np.int64)
    nxt = 0
    for p, k in enumerate(splits):
        idx = np.flatnonzero(pop == p)
        order = idx[np.argsort(scores[idx, 0], kind="stable")]
        for j, part in enumerate(np.array_split(order, k)):
            labels[part] = nxt + j
        nxt += k
    relabel = rng.permutation(nxt)  # label numbers unrelated to the populations
    return sparse.csr_matrix(counts), scores, relabel[labels].astype(np.int16)


def planted_default():
    """The case of tests/test_gpu_merge_clusters.py: 4 populations cut into 9 labels, plus one distinct population: 10 labels."""
    return planted([800, 700, 600, 500, 400], [3, 2, 2, 2, 1], 500, 6, 3)


def planted_shuffled():
    """The same with the cells in random order: every cluster has cells in every shard."""
    m, x, labels = planted_default()
    order = np.random.default_rng(9).permutation(len(labels))
    return sparse.csr_matrix(sparse.csc_matrix(m)[:, order]), x[order], labels[order]


# cluster -> size. 0: a singleton; 1: two cells far apart (an even count whose two middle elements lie in different shards at any cut
# into two or more); 2: 255 cells, the first 255 of the matrix (inside the first shard of up to five); 3, 4: 256 and 257 cells spread
# over everything; 5: the rest
MEDOID_SIZES = (1, 2, 255, 256, 257, 600)
MEDOID_CELLS = sum(MEDOID_SIZES)
MEDOID_PAIR = (300, 1300)  # the cells of cluster 1
MEDOID_D = 6


def medoid_case():
    """(genes x cells matrix with the same number of nonzeros in every cell, so that shards cut by nonzeros are equal ranges of cells;
    cells x d scores; labels). Columns: 0 normal, 1 rounded (ties), 2 signed zeros and ±1, 3 huge / tiny / denormal values of both signs,
    4 all negative, 5 one constant."""
    rng = np.random.default_rng(41)
    n = MEDOID_CELLS
    labels = np.full(n, -1, dtype=np.int64)
    labels[:255] = 2
    labels[list(MEDOID_PAIR)] = 1
    free = rng.permutation(np.flatnonzero(labels == -1))
    labels[free[0]] = 0
    labels[free[1:257]] = 3
    labels[free[257:514]] = 4
    labels[free[514:]] = 5
    assert tuple(np.bincount(labels)) == MEDOID_SIZES
    x = rng.standard_normal((n, MEDOID_D))
    x[:, 1] = np.round(x[:, 1])
    x[:, 2] = rng.choice([-0.0, 0.0, 1.0, -1.0], n)
    x[:, 3] = rng.choice([-1e300, 1e-300, -5e-324, 5e-324, 2.5e-310, -2.5e-310, 3.0], n)
    x[:, 4] = -np.abs(x[:, 4]) - 0.5
    x[:, 5] = 7.25
    counts = np.zeros((8, n), dtype=np.uint32)
    counts[:4] = rng.integers(1, 9, (4, n))  # four nonzeros per cell
    return sparse.csc_matrix(counts), x, labels.astype(np.int16)
