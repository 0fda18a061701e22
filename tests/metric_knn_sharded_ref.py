"""TEST INFRASTRUCTURE ONLY: nearest_neighbors under pearson / cosine distance with a query set of its own and over a sharded point
set (umap-rs knn.rs:112-166, dist.rs:73-124), restated with numpy. Every operation is one IEEE f64 operation on
arrays (numpy never fuses), the folds run over the coordinates in order, so the bits are the reference's; the single-pair
restatement in plain Python floats is tests/metric_knn_ref.py, which tests/test_metric_knn_sharded_cpu.py holds this file to.

The block model is the scheme of the library: the global rows are cut into blocks of `block_rows`; a query searches one block at a
time for the block's k nearest rows other than its own GLOBAL row, drops what does not beat the k-th key it already holds (the
strict seed), and merges the rest into its running list by (key, global index) with the merge of tests/knn_sharded_ref.py."""
import numpy as np

import knn_sharded_ref as ks

U32MAX = ks.U32MAX


def prepare_rows(kind, x):
    """(C, s): the centred rows (pearson) or the rows (cosine), and s_xx of each."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    if kind == "pearson":
        mu = np.zeros(n)
        for j in range(d):
            mu = mu + x[:, j]
        mu = mu / float(d)
        c = x - mu[:, None]
    else:
        c = x.copy()
    s = np.zeros(n)
    with np.errstate(all="ignore"):
        for j in range(d):
            s = s + c[:, j] * c[:, j]
    return c, s


def keys_of(cq, sq, c, s):
    """(keys, D) of one prepared query against prepared points: dist.rs:77-83 / 117-123, then the square root."""
    with np.errstate(all="ignore"):
        sxy = np.zeros(c.shape[0])
        for j in range(c.shape[1]):
            sxy = sxy + cq[j] * c[:, j]
        v = 1.0 - sxy / np.sqrt(sq * s)
        v = np.where(v > 0.0, v, 0.0)  # f64::max(v, 0.0): a NaN operand loses
        v = np.where(sxy == 0.0, 1.0, v)
        v = np.where((sq == 0.0) & (s == 0.0), 0.0, v)
        return np.sqrt(v), v


def first_k(key, idx, k):
    """the first k of (key, index) in that order, padded with (+inf, UINT32_MAX)"""
    order = np.lexsort((idx, key))[:k]
    kk, ii = np.full(k, np.inf), np.full(k, U32MAX, dtype=np.uint32)
    kk[: len(order)], ii[: len(order)] = key[order], idx[order]
    return kk, ii


def nearest_neighbors_query(kind, queries, points, k, include_self):
    """(indices n_q x k u32, distances n_q x k): ordered by (key, index), padded with UINT32_MAX / +inf; include_self False drops the
    point whose index is the query's row number."""
    cq, sq = prepare_rows(kind, queries)
    cp, sp = prepare_rows(kind, points)
    n_q, n_p = cq.shape[0], cp.shape[0]
    idx, dist = np.zeros((n_q, k), dtype=np.uint32), np.zeros((n_q, k))
    rows = np.arange(n_p, dtype=np.uint32)
    for q in range(n_q):
        key, _ = keys_of(cq[q], sq[q], cp, sp)
        keep = np.ones(n_p, dtype=bool) if include_self else rows != q
        kk, idx[q] = first_k(key[keep], rows[keep], k)
        dist[q] = kk * kk
    return idx, dist


def search_block(keys, b0, b1, q_global, k, seed):
    """the k nearest rows of block [b0, b1) to global row q_global (keys: its key against every global row; a pair's key depends on
    the two rows only), that row excluded, among those whose key is below the seed (+inf: no seed, every key enters, +inf included):
    (keys, block-LOCAL indices), padded"""
    key = keys[b0:b1]
    local = np.arange(b1 - b0, dtype=np.uint32)
    keep = local + b0 != q_global
    if seed != np.inf:
        keep &= key < seed
    return first_k(key[keep], local[keep], k)


def sharded_model(kind, points, cuts, block_rows, k):
    """(n x k) u32 global indices and distances, rank by rank (cuts: the shard boundaries, 0 .. n) and block by block. Every rank
    prepares the rows itself; prepare_rows works row by row, so the cut cannot change a bit of them."""
    points = np.asarray(points, dtype=np.float64)
    n = points.shape[0]
    assert cuts[0] == 0 and cuts[-1] == n
    out, dist = np.zeros((n, k), dtype=np.uint32), np.zeros((n, k))
    c, s = prepare_rows(kind, points)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        for q in range(lo, hi):
            rk, ri = np.full(k, np.inf), np.full(k, U32MAX, dtype=np.uint32)
            keys, _ = keys_of(c[q], s[q], c, s)
            for b0, b1 in ks.block_plan(n, block_rows):
                bk, bi = search_block(keys, b0, b1, q, k, rk[k - 1])
                bi = np.where(bi == U32MAX, bi, bi + np.uint32(b0)).astype(np.uint32)
                rk, ri = ks.merge(rk, ri, bk, bi)
            out[q], dist[q] = ri, rk * rk
    return out, dist
