"""The fixture of tests/test_subset_sharded_cpu.py and tests/test_gpu_subset_sharded.py: one seeded genes x cells
count matrix on which the statistics over a list of columns of a SHARDED matrix can go wrong, the explicit cuts into shards, the
lists, and the three maps as dense f64 arrays of the mapped values. Everything here is numpy; nothing needs a device."""
import numpy as np
from scipy import sparse

GENES, CELLS = 37, 18500
SEED = 20267
DENSITY, MAX_COUNT = 0.06, 300
FULL_GENE, EMPTY_GENE = 5, 23        # a gene present in every cell that has anything / a gene without a count
EMPTY_CELLS = (7000, 7400)           # a run of cells without a count
ITEM_NNZ = 8192                      # the cut of a long vector into work items (common.hpp)

# the cells cut into ranks, by shard count: uneven cuts; at 5 one shard is exactly the run of empty cells. The full gene's vector in
# the transposed copy of a shard is longer than ITEM_NNZ (cut into slab pieces) at 1 and 2 shards and shorter at 3 and 5.
RANGES = {
    1: (0, CELLS),
    2: (0, 9300, CELLS),
    3: (0, 6000, 12100, CELLS),
    5: (0, 3000, 7000, 7400, 12000, CELLS),
}
# the genes cut into ranks (a matrix sharded over its genes): uneven, and at 5 one shard holds the empty gene alone
GENE_RANGES = {1: (0, GENES), 2: (0, 20, GENES), 3: (0, 5, 23, GENES), 5: (0, 6, 23, 24, 30, GENES)}

UMI_COUNT_SUM = 2000.0  # the GIVEN target of the log_normalize map


def matrix():
    """37 genes x 18 500 cells, canonical CSR of uint32 counts 1..300 at about 6 %."""
    rng = np.random.default_rng(SEED)
    a = np.where(rng.random((GENES, CELLS)) < DENSITY, rng.integers(1, MAX_COUNT + 1, size=(GENES, CELLS)), 0)
    a[FULL_GENE, :] = rng.integers(1, MAX_COUNT + 1, size=CELLS)
    a[EMPTY_GENE, :] = 0
    a[:, EMPTY_CELLS[0]:EMPTY_CELLS[1]] = 0
    m = sparse.csr_matrix(a.astype(np.uint32))
    m.sort_indices()
    return m


def cell_lists():
    """name -> ascending cell indices: every third cell; a list sharing half of the first; a list inside one shard (of every cut
    above); a list that skips a whole shard (shard 1 of the cut into 3, shards 2 and 3 of the cut into 5); the empty list; all cells."""
    third = np.arange(0, CELLS, 3)
    rng = np.random.default_rng(SEED + 1)
    others = np.setdiff1d(np.arange(CELLS), third)
    half = np.sort(np.concatenate([third[::2], rng.choice(others, third.size // 2, replace=False)]))
    inside = np.arange(12500, 18000, 2)
    skips = np.concatenate([np.arange(100, 5900, 5), np.arange(12100, CELLS, 7)])
    return {"third": third, "half": half, "inside": inside, "skips": skips, "empty": np.zeros(0, dtype=np.int64), "all": np.arange(CELLS)}


def gene_lists():
    """The same kinds over the genes (the cuts are GENE_RANGES)."""
    third = np.arange(0, GENES, 3)
    half = np.sort(np.concatenate([third[::2], np.array([1, 5, 8, 23, 31, 35])]))
    inside = np.arange(24, 30)
    skips = np.concatenate([np.arange(0, 5), np.arange(23, GENES, 2)])
    return {"third": third, "half": half, "inside": inside, "skips": skips, "empty": np.zeros(0, dtype=np.int64), "all": np.arange(GENES)}


def dual_pairs(lists):
    """The pairs of the dual form: overlapping, one empty, disjoint in their shards."""
    return [("third", "half"), ("empty", "skips"), ("inside", "all")]


def factors():
    """(per gene, per cell) scale factors of the ScaleAxis map: magnitudes over several binades, a third of them negative."""
    rng = np.random.default_rng(SEED + 2)
    fg = (rng.random(GENES) * 3.0 + 0.01) * np.where(rng.random(GENES) < 0.35, -1.0, 1.0)
    fc = np.ldexp(rng.random(CELLS) + 0.5, rng.integers(-6, 7, size=CELLS)) * np.where(rng.random(CELLS) < 0.3, -1.0, 1.0)
    return fg, fc


def size_factors():
    """GIVEN per-cell size factors of the log_normalize map (uint32, none zero)."""
    rng = np.random.default_rng(SEED + 3)
    return rng.integers(500, 6000, size=CELLS).astype(np.uint32)


def mapped_dense(m, which):
    """The genes x cells f64 array of the mapped values, zero where nothing is stored, with the operation order of eval_map
    (device_map.hpp): the links in the order they were composed, each `factor[position] * x`.
      raw     the counts
      scale   ScaleAxis(genes, fg) then ScaleAxis(cells, fc): fc[c] * (fg[g] * count) - products of doubles, exact in numpy
      log     log_normalize with the given target and size factors: log2((target / sf[c]) * count + 1)"""
    d = m.toarray().astype(np.float64)
    if which == "raw":
        return d
    if which == "scale":
        fg, fc = factors()
        return fc[None, :] * (fg[:, None] * d)
    if which == "log":
        scale = UMI_COUNT_SUM / size_factors().astype(np.float64)
        return np.where(d != 0.0, np.log2(scale[None, :] * d + 1.0), 0.0)
    raise ValueError(which)


def split_list(idx, bounds):
    """A global ascending list over ranges [bounds[r], bounds[r + 1]): per rank (entries of the list below the rank's range, the
    rank's entries rebased to local positions)."""
    idx = np.asarray(idx, dtype=np.int64)
    out = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        a, b = np.searchsorted(idx, lo), np.searchsorted(idx, hi)
        out.append((int(a), idx[a:b] - lo))
    return out


def shard_csc(m_csc, lo, hi):
    """(indptr u64, indices u32, data u32) of outer vectors [lo, hi) of a canonical CSC (or CSR) matrix."""
    ip = m_csc.indptr[lo:hi + 1].astype(np.uint64)
    a, b = int(ip[0]), int(ip[-1])
    return ip - ip[0], m_csc.indices[a:b].astype(np.uint32), m_csc.data[a:b].astype(np.uint32)
