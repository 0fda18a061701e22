"""A numpy restatement of scanrs_multi_gather_outer / scanrs_multi_rebalance (scanrs_host_plan_gather and the device
path of multi.cpp / regather.hip), and the matrices and lists of tests/test_regather_cpu.py and tests/test_gpu_regather.py. Everything
is an integer; every comparison made with these is exact."""
import numpy as np

import reshard_ref as ref
from reshard_ref import plan_shards  # noqa: F401  (the restated scanrs_plan_shards, reused)

TILE = 2048  # REGATHER_TILE: the output elements one workgroup of the pull owns


def select_outer(indptr, indices, data, idx):
    """The triplet whose outer vector j is vector idx[j] of the given CSR / CSC triplet (any order, repeats allowed)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    lens = indptr[idx + 1] - indptr[idx] if idx.size else np.zeros(0, dtype=np.int64)
    out_indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    # element e of output vector j sits at indptr[idx[j]] + (e - out_indptr[j]) in the source
    at = np.repeat(indptr[idx] - out_indptr[:-1], lens) + np.arange(int(out_indptr[-1]), dtype=np.int64) if idx.size else np.zeros(0, dtype=np.int64)
    return out_indptr.astype(np.uint64), np.asarray(indices)[at].astype(np.uint32), np.asarray(data)[at].astype(np.uint32)


def plan_gather(indptr, src_bounds, idx, n_dst):
    """(out_indptr, bounds, moved): the selected matrix's indptr, its cut by plan_shards, and moved[s, d] = the nonzeros of the output
    vectors of shard d whose source vector lies in [src_bounds[s], src_bounds[s + 1])."""
    indptr = np.asarray(indptr, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    sb = [int(x) for x in src_bounds]
    n_src = len(sb) - 1
    lens = indptr[idx + 1] - indptr[idx] if idx.size else np.zeros(0, dtype=np.int64)
    out_indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    bounds = plan_shards(out_indptr, n_dst)
    moved = np.zeros((n_src, n_dst), dtype=np.uint64)
    for d in range(n_dst):
        part_idx, part_len = idx[int(bounds[d]):int(bounds[d + 1])], lens[int(bounds[d]):int(bounds[d + 1])]
        for s in range(n_src):
            moved[s, d] = int(part_len[(part_idx >= sb[s]) & (part_idx < sb[s + 1])].sum())
    return out_indptr, bounds, moved


# ---- the matrices: (n_outer, n_inner, indptr, indices, data) with the SHARDED dimension outermost and no stored zeros --------------------
def _cells_outer(name):
    """A §7m matrix (feature-major: one outer vector per feature) as a caller hands it to MultiMat(...) with the cells sharded: the
    host-transposed triplet, stored zeros dropped (scanrs_mat_create drops them; to_csmat gives this back)."""
    n_outer, n_inner, ip, ix, vv = ref.CASES[name]()
    t = ref.drop_zeros(*ref.transposed_triplet(ip, ix, vv, n_outer, n_inner))
    return (n_inner, n_outer) + t


def case_heavy_vector():
    """One outer vector with more entries than any tile of the pull (2.5 tiles and an odd rest) and every other vector empty."""
    n_outer, n_inner, at = 37, 2 * TILE + TILE // 2 + 77, 19
    rng = np.random.default_rng(23)
    indptr = np.zeros(n_outer + 1, dtype=np.uint64)
    indptr[at + 1:] = n_inner
    return n_outer, n_inner, indptr, np.arange(n_inner, dtype=np.uint32), rng.integers(1, 2**31, size=n_inner).astype(np.uint32)


CASES = {name: (lambda name=name: _cells_outer(name)) for name in ref.CASES}
CASES["heavy_vector"] = case_heavy_vector
SHARDS = ref.SHARDS


def lists(n_outer, src_bounds):
    """The lists of the tests for a matrix of n_outer vectors cut at src_bounds, by name."""
    rng = np.random.default_rng(1009 + n_outer)
    ident = np.arange(n_outer, dtype=np.uint64)
    out = {"identity": ident, "reversed": ident[::-1].copy(), "shuffle": rng.permutation(n_outer).astype(np.uint64),
           "empty": np.zeros(0, dtype=np.uint64)}
    if n_outer:
        # repeats and omissions: a sample with replacement, about two thirds as long, so some vectors come twice and some never
        out["repeats"] = rng.integers(0, n_outer, size=max(2, (2 * n_outer) // 3)).astype(np.uint64)
        out["single"] = np.array([n_outer // 2], dtype=np.uint64)
        # nothing from one source shard: the widest range is left out, the rest comes back to front
        sb = [int(x) for x in src_bounds]
        w = int(np.argmax(np.diff(sb)))
        out["skip_shard"] = np.concatenate([ident[sb[w + 1]:], ident[:sb[w]]])[::-1].copy()
    return out
