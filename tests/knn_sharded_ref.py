"""TEST INFRASTRUCTURE ONLY: a numpy model of the kNN over a sharded point set (scan-rs/src/nn.rs:38-83) and the
fixtures its CPU and GPU tests share.

The scheme: every rank owns the queries of its own rows; the global rows are cut into blocks of `block_rows` rows (the last one
short, the cut independent of the shard cut); a query searches one block at a time for the block's k nearest rows other than the
query's own GLOBAL row and merges them into its running list by (squared distance, global index). Lists are padded with
(+inf, UINT32_MAX). The squared distance is the library's: t = p_j - q_j, s = fma(t, t, s) in coordinate order (the policy Euclid of
scan-rs_amd/csrc/knn.hip under the kernels of knn_search.hpp), restated here with error-free transformations so that the BITS can be compared."""
import numpy as np

U32MAX = 0xFFFFFFFF


# ---- fma(a, b, c) = RN(a b + c), exactly, on float64 arrays --------------------------------------------------------------------------
# a b = ph + pl exactly (Dekker / Veltkamp); RN(ph + pl + c) by Boldo & Melquiond, "Emulation of a FMA and correctly rounded sums:
# proved algorithms using rounding to odd" (IEEE TC 2008): two error-free sums, the two low parts added with rounding to odd, one
# last rounding to nearest. Valid away from overflow and underflow, which the fixtures are (tests/test_knn_sharded_cpu.py checks this
# restatement against exact rational arithmetic).
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a  # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _add_round_to_odd(a, b):
    s, e = _two_sum(a, b)
    bits = np.ascontiguousarray(s).view(np.int64).copy()
    fix = (e != 0.0) & ((bits & 1) == 0)  # inexact and even: the odd neighbour on the side of the error
    away = (e > 0.0) == (s > 0.0)         # the exact sum is larger in magnitude than s
    bits = np.where(fix, np.where(away, bits + 1, bits - 1), bits)
    return bits.view(np.float64)


def fma(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    ph, pl = _two_prod(a, b)
    uh, ul = _two_sum(c, pl)
    th, tl = _two_sum(ph, uh)
    return th + _add_round_to_odd(tl, ul)


def sq_dist_rows(points, q):
    """Squared distances of every row of `points` to q, with the library's rounding."""
    points = np.asarray(points, dtype=np.float64)
    s = np.zeros(points.shape[0])
    for j in range(points.shape[1]):
        t = points[:, j] - q[j]
        s = fma(t, t, s)
    return s


def sq_dist_pairs(points, nbr):
    """(n x k) squared distances between row i of `points` and rows nbr[i, :] (+inf where nbr is UINT32_MAX)."""
    points = np.asarray(points, dtype=np.float64)
    nbr = np.asarray(nbr).astype(np.int64)
    pad = nbr == U32MAX
    idx = np.where(pad, 0, nbr)
    s = np.zeros(nbr.shape)
    for j in range(points.shape[1]):
        t = points[idx, j] - points[:, j][:, None]
        s = fma(t, t, s)
    return np.where(pad, np.inf, s)


# ---- the scheme ------------------------------------------------------------------------------------------------------------------------
def block_plan(n, block_rows):
    """[(begin, end)] of the global blocks: block_rows rows each, the last one short."""
    return [(b, min(b + block_rows, n)) for b in range(0, n, block_rows)]


def _first_k(d, i, k):
    order = np.lexsort((i, d))[:k]
    dd, ii = np.full(k, np.inf), np.full(k, U32MAX, dtype=np.uint32)
    dd[: len(order)], ii[: len(order)] = d[order], i[order]
    return dd, ii


def merge(da, ia, db, ib):
    """Two padded lists of k entries -> the first k of their union by (squared distance, index); padding stays padding."""
    da, db = np.asarray(da, dtype=np.float64), np.asarray(db, dtype=np.float64)
    ia, ib = np.asarray(ia, dtype=np.uint32), np.asarray(ib, dtype=np.uint32)
    return _first_k(np.concatenate([da, db]), np.concatenate([ia, ib]), len(da))


def search_block(points, b0, b1, q_global, k):
    """The k nearest rows of block [b0, b1) to global row q_global, that row itself excluded: (distances, global indices), padded."""
    d = sq_dist_rows(points[b0:b1], points[q_global])
    i = np.arange(b0, b1, dtype=np.uint32)
    keep = i != q_global
    return _first_k(d[keep], i[keep], k)


def knn_sharded_model(points, cuts, block_rows, k):
    """(n x k) u32 indices and squared distances, computed rank by rank (cuts: the shard boundaries, 0 .. n) and block by block."""
    points = np.asarray(points, dtype=np.float64)
    n = points.shape[0]
    assert cuts[0] == 0 and cuts[-1] == n
    out, dist = np.zeros((n, k), dtype=np.uint32), np.zeros((n, k))
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        for q in range(lo, hi):
            rd, ri = np.full(k, np.inf), np.full(k, U32MAX, dtype=np.uint32)
            for b0, b1 in block_plan(n, block_rows):
                bd, bi = search_block(points, b0, b1, q, k)
                rd, ri = merge(rd, ri, bd, bi)
            out[q], dist[q] = ri, rd
    return out, dist


def knn_one_pass(points, k):
    """The same answer without blocks or shards: one sort per query by (squared distance, index)."""
    points = np.asarray(points, dtype=np.float64)
    n = points.shape[0]
    out, dist = np.zeros((n, k), dtype=np.uint32), np.zeros((n, k))
    for q in range(n):
        dist[q], out[q] = search_block(points, 0, n, q, k)
    return out, dist


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------
LATTICE_N, LATTICE_D = 97, 3
LATTICE_K = (1, 5, 40)
LATTICE_BLOCKS = (7, 32, 1000)  # blocks that straddle the shard cuts / one block inside a shard / one block for everything
# explicit cuts per number of shards; every cut with more than one shard has a shard of 2 cells (fewer points than k = 5 or 40),
# the cut in five also one of a single cell
LATTICE_CUTS = {1: [0, 97], 2: [0, 95, 97], 3: [0, 40, 42, 97], 5: [0, 2, 33, 34, 70, 97]}


def lattice_points():
    """97 points on the integer lattice {0..3}^3: massive ties and many exact duplicates; distances are exact integers."""
    return np.random.default_rng(97).integers(0, 4, size=(LATTICE_N, LATTICE_D)).astype(np.float64)


PADDING_N, PADDING_K, PADDING_CUTS = 6, 9, [0, 2, 3, 6]


def padding_points():
    return np.random.default_rng(6).integers(0, 5, size=(PADDING_N, 2)).astype(np.float64)


DUP_HALF = 23


def duplicated_points():
    """A list of 23 distinct integer points concatenated with itself: row i and row 23 + i coincide, and two shards cut at 23 hold
    identical point lists (the duplicate of a query has the query's LOCAL row in the other shard)."""
    rng = np.random.default_rng(23)
    base = rng.permutation(64)[:DUP_HALF]
    half = np.stack([base // 16, (base // 4) % 4, base % 4], axis=1).astype(np.float64)  # distinct points of {0..3}^3
    return np.concatenate([half, half], axis=0)


def merge_cases():
    """[(name, da, ia, db, ib)] for the merge rule: ties across the lists, padding on either side, k = 1, k = 128."""
    inf, m = np.inf, U32MAX
    cases = [
        ("ties across the lists", [1.0, 1.0, 2.0, 2.0], [3, 9, 1, 8], [1.0, 1.0, 2.0, 3.0], [2, 5, 4, 0]),
        ("padding in a", [0.5, inf, inf], [7, m, m], [0.25, 0.5, 4.0], [9, 2, 1]),
        ("padding in b", [0.25, 0.5, 4.0], [9, 2, 1], [0.5, inf, inf], [7, m, m]),
        ("padding in both, fewer than k real entries", [1.0, inf, inf, inf], [4, m, m, m], [1.0, 3.0, inf, inf], [2, 6, m, m]),
        ("both empty", [inf, inf], [m, m], [inf, inf], [m, m]),
        ("k = 1, a wins", [1.0], [5], [2.0], [1]),
        ("k = 1, b wins a tie by index", [1.0], [5], [1.0], [1]),
        ("k = 1, b empty", [1.0], [5], [inf], [m]),
        ("zero distances", [0.0, 0.0, 1.0], [10, 30, 2], [0.0, 0.0, 0.0], [5, 20, 40]),
    ]
    rng = np.random.default_rng(128)
    for name, k, levels, real_a, real_b in (("k = 128, heavy ties", 128, 6, 128, 128), ("k = 128, short lists", 128, 4, 50, 3),
                                            ("k = 17, random", 17, 1000, 17, 11)):
        idx = rng.permutation(100000)[: real_a + real_b].astype(np.uint32)  # no index in both lists
        lists = []
        for real, ii in ((real_a, idx[:real_a]), (real_b, idx[real_a:])):
            d = rng.integers(0, levels, size=real).astype(np.float64)
            dd, ix = _first_k(d, ii, k)
            lists += [dd, ix]
        cases.append((name, *lists))
    return [(name, np.asarray(da, dtype=np.float64), np.asarray(ia, dtype=np.uint32), np.asarray(db, dtype=np.float64),
             np.asarray(ib, dtype=np.uint32)) for name, da, ia, db, ib in cases]
