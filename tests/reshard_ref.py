"""A numpy restatement of the plan of the inner-sharding constructors (scanrs_host_plan_inner and the device path of
scanrs_multi_create_inner), and the matrices of tests/test_reshard_cpu.py and tests/test_gpu_reshard.py. Everything is an integer;
every comparison made with these is exact."""
import numpy as np
from scipy import sparse

U32_MAX = 2**32 - 1


def plan_shards(indptr, world):
    """scanrs_plan_shards: bounds[r] = the first outer index whose prefix reaches floor(nnz * r / world), never descending."""
    indptr = [int(x) for x in indptr]
    n_outer = len(indptr) - 1
    nnz = indptr[-1] - indptr[0]
    bounds = [0] * (world + 1)
    for r in range(1, world):
        want = indptr[0] + (nnz * r) // world
        b = int(np.searchsorted(np.asarray(indptr, dtype=np.uint64), np.uint64(want), side="left"))
        bounds[r] = max(min(b, n_outer), bounds[r - 1])
    bounds[world] = n_outer
    return np.asarray(bounds, dtype=np.uint64)


def plan_inner(indptr, indices, n_inner, world):
    """(slab_bounds, bounds, moved) for a feature-major triplet: the slabs of the outer vectors by stored entries, the shard ranges of
    the inner dimension by stored entries per inner position (stored zeros count in both), and moved[s, d] = the stored entries of
    slab s whose inner index lies in [bounds[d], bounds[d + 1])."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    slab_bounds = plan_shards(indptr, world)
    t_indptr = np.concatenate([[0], np.cumsum(np.bincount(indices, minlength=n_inner))]) if n_inner else np.zeros(1, dtype=np.int64)
    bounds = plan_shards(t_indptr, world)
    moved = np.zeros((world, world), dtype=np.uint64)
    for s in range(world):
        idx = indices[indptr[int(slab_bounds[s])]:indptr[int(slab_bounds[s + 1])]]
        for d in range(world):
            moved[s, d] = int(np.count_nonzero((idx >= int(bounds[d])) & (idx < int(bounds[d + 1]))))
    return slab_bounds, bounds, moved


def triplet(m):
    """(indptr u64, indices u32, data u32) of a canonical scipy CSR / CSC matrix, stored zeros kept."""
    return m.indptr.astype(np.uint64), m.indices.astype(np.uint32), m.data.astype(np.uint32)


def transposed_triplet(indptr, indices, data, n_outer, n_inner):
    """The same entries with the other dimension outermost: what a caller who transposes on the host hands to scanrs_multi_create.
    Stable (the new inner indices ascend) and stored zeros stay stored."""
    indptr = np.asarray(indptr, dtype=np.int64)
    outer = np.repeat(np.arange(n_outer, dtype=np.int64), np.diff(indptr))
    order = np.argsort(np.asarray(indices, dtype=np.int64), kind="stable")
    t_indptr = np.concatenate([[0], np.cumsum(np.bincount(np.asarray(indices, dtype=np.int64), minlength=n_inner))]) if n_inner else np.zeros(1, dtype=np.int64)
    return t_indptr.astype(np.uint64), outer[order].astype(np.uint32), np.asarray(data)[order].astype(np.uint32)


def drop_zeros(indptr, indices, data):
    """What scanrs_mat_create keeps of a triplet: stored zeros dropped."""
    indptr = np.asarray(indptr, dtype=np.int64)
    keep = np.asarray(data) != 0
    kept_before = np.concatenate([[0], np.cumsum(keep)])
    return kept_before[indptr].astype(np.uint64), np.asarray(indices)[keep].astype(np.uint32), np.asarray(data)[keep].astype(np.uint32)


# ---- the matrices: (n_outer, n_inner, indptr, indices, data), feature-major (one outer vector per feature) ------------------------
def case_seeded():
    """(a) select_sharded_case.seeded_matrix(): 61 x 157, empty cells, an empty gene, thinned cells."""
    import select_sharded_case as case

    m = case.seeded_matrix()
    return (m.shape[0], m.shape[1]) + triplet(m)


LONG_INNER = 70001


def case_long_vector():
    """(b) 3 outer vectors x 70 001 inner positions; vector 1 has an entry at EVERY position: a run far longer than a block, more
    shards than vectors (empty slabs) and cuts inside one vector."""
    rng = np.random.default_rng(71)
    a = np.sort(rng.choice(LONG_INNER, size=900, replace=False))
    c = np.sort(rng.choice(LONG_INNER, size=333, replace=False))
    full = np.arange(LONG_INNER)
    indices = np.concatenate([a, full, c]).astype(np.uint32)
    indptr = np.array([0, a.size, a.size + full.size, indices.size], dtype=np.uint64)
    data = rng.integers(1, 9, size=indices.size).astype(np.uint32)
    return 3, LONG_INNER, indptr, indices, data


def case_one_position():
    """(c) every nonzero in ONE inner position: the bounds repeat, so there are empty shards."""
    n_outer, n_inner, at = 23, 41, 29
    rows = np.array([0, 1, 2, 5, 7, 11, 12, 13, 20, 22])
    lens = np.zeros(n_outer, dtype=np.int64)
    lens[rows] = 1
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return n_outer, n_inner, indptr, np.full(rows.size, at, dtype=np.uint32), np.arange(1, rows.size + 1, dtype=np.uint32)


def case_zeros_and_max():
    """(d) explicit stored zeros and a value of 2^32 - 1."""
    rng = np.random.default_rng(5)
    n_outer, n_inner = 19, 53
    mask = rng.random((n_outer, n_inner)) < 0.3
    m = sparse.csr_matrix(mask.astype(np.int64))
    m.sort_indices()
    data = rng.integers(0, 4, size=m.nnz).astype(np.uint64)  # about a quarter of the stored entries are zeros
    data[7] = U32_MAX
    data[0] = 0
    data[-1] = 0
    assert np.count_nonzero(data == 0) > 10
    return n_outer, n_inner, m.indptr.astype(np.uint64), m.indices.astype(np.uint32), data.astype(np.uint32)


def case_empty():
    """(e) nnz = 0."""
    n_outer, n_inner = 7, 11
    return n_outer, n_inner, np.zeros(n_outer + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32)


CASES = {"seeded": case_seeded, "long_vector": case_long_vector, "one_position": case_one_position, "zeros_and_max": case_zeros_and_max,
         "empty": case_empty}
SHARDS = (1, 2, 3, 5)
