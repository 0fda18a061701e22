"""The vectors the AdaptiveVec encoder tests share (tests/test_adaptive_export_cpu.py, tests/test_gpu_adaptive_export.py): for each
inner length a matrix of 25 outer vectors = 5 densities x 5 value ranges, every range with a 5 % tail drawn from [1, 100000) so that
all four fallback thresholds (7, 15, 255, 65535) are crossed inside one vector.

The lengths sit on the edges of the layouts: 1; 21 and 22 (one Dense3 word of 21 fields, and one field into the next); 300 (two
256-index blocks, odd nibble count at odd n); 5000 (20 blocks, most of them empty at density 0.004); 70001 (more than 34 work chunks
of 2048 entries at density 1, an odd length, 274 blocks). Density 0 gives empty vectors."""
import numpy as np

LENGTHS = (1, 21, 22, 300, 5000, 70001)
DENSITIES = (0.0, 0.004, 0.03, 0.3, 1.0)
RANGES = ((1, 6), (7, 15), (20, 200), (300, 60000), (60000, 200000))


def grid(seed=7):
    """{length: [(indices u32 ascending, values u32), ...25]} in the order densities x ranges."""
    rng = np.random.default_rng(seed)
    out = {}
    for length in LENGTHS:
        vecs = []
        for dens in DENSITIES:
            for lo, hi in RANGES:
                n = min(length, int(round(length * dens)))
                idx = np.sort(rng.choice(length, size=n, replace=False)).astype(np.uint32)
                val = rng.integers(lo, hi, size=n).astype(np.uint32)
                tail = rng.random(n) < 0.05
                val[tail] = rng.integers(1, 100000, size=int(tail.sum())).astype(np.uint32)
                vecs.append((idx, val))
        out[length] = vecs
    return out


def as_csmat(vecs):
    """(indptr u64, indices u32, data u32) of a matrix whose outer vectors are `vecs`."""
    indptr = np.zeros(len(vecs) + 1, dtype=np.uint64)
    indptr[1:] = np.cumsum([len(i) for i, _ in vecs])
    indices = np.concatenate([i for i, _ in vecs]).astype(np.uint32)
    data = np.concatenate([v for _, v in vecs]).astype(np.uint32)
    return indptr, indices, data
