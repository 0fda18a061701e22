"""Helpers of the hclust tests: a plain-Python restatement of what hclust/src/lib.rs does with a dendrogram (:74-239), an exact
evaluation of linkage heights from their definitions in np.longdouble, the test inputs, and a validity check of a dendrogram.

A dendrogram is four arrays of n - 1 entries (cluster1, cluster2, dissimilarity, size) in kodama's form: sorted by dissimilarity,
the cluster made by step i is named n + i."""
import numpy as np

METHODS = {"single": 0, "complete": 1, "average": 2, "weighted": 3, "ward": 4}
SHAPES = [(2, 3), (3, 1), (65, 7), (257, 50), (1500, 16)]
EPS = float(np.finfo(np.float64).eps)


def points(n, d, seed=None):
    """Standard-normal points with a fixed seed per shape."""
    rng = np.random.default_rng(1000 * n + d if seed is None else seed)
    return rng.standard_normal((n, d))


def tie_cases():
    """nn.rs::test_symmetry's 5 x 5 (identity with one entry 3.0) and a 6 x 6 integer grid (36 points in the plane)."""
    v = np.eye(5)
    v[0, 4] = 3.0
    gx, gy = np.meshgrid(np.arange(6.0), np.arange(6.0), indexing="ij")
    return {"symmetry5": v, "grid6": np.stack([gx.ravel(), gy.ravel()], axis=1)}


def overflow_cases():
    """Finite coordinates that do not make finite dissimilarities. "distance": squared differences beyond f64 (a 1e200 sentinel in
    the data). "ward_update": every squared distance is finite (at most 1.69e308), but Ward's update of the first merge computes
    (1 + 1) * 1e308."""
    return {"distance": np.array([[0.0], [1e200], [-1e200], [3e200]]), "ward_update": np.array([[0.0], [1.0], [1e154], [-0.3e154]])}


# ---- hclust/src/lib.rs:74-116 --------------------------------------------------------------------------------------------------
class SimpleOrdering:
    def __init__(self, n_obs):
        self.left = list(range(n_obs)) + [None] * (n_obs - 1)
        self.right = list(range(n_obs)) + [None] * (n_obs - 1)
        self.nb_left = [None] * n_obs
        self.nb_right = [None] * n_obs

    def observe(self, merged, left_cluster, right_cluster):
        self.left[merged] = self.left[left_cluster]
        self.right[merged] = self.right[right_cluster]
        self.nb_right[self.right[left_cluster]] = self.left[right_cluster]
        self.nb_left[self.left[right_cluster]] = self.right[left_cluster]

    def ordered_leaves(self):
        start = next(i for i, b in enumerate(self.nb_left) if b is None)
        leaves = [start]
        while self.nb_right[leaves[-1]] is not None:
            leaves.append(self.nb_right[leaves[-1]])
        assert len(leaves) == len(self.nb_left)
        return leaves


def relabel_vector(values):
    """:122-125: names 1, 2, .. in order of first appearance."""
    mapping = {}
    for v in values:
        if v not in mapping:
            mapping[v] = len(mapping) + 1
    return [mapping[v] for v in values]


def leaves(c1, c2, diss, ordering):
    """:150-206; ordering 0 = Naive, 1 = ModularSmallest."""
    n = len(c1) + 1
    order = SimpleOrdering(n)
    if ordering == 0:
        for i, (a, b) in enumerate(zip(c1, c2)):
            a, b = int(a), int(b)
            order.observe(n + i, min(a, b), max(a, b))
        return order.ordered_leaves()
    min_d = [np.finfo(np.float64).max] * (2 * n - 1)
    for i, (a, b, h) in enumerate(zip(c1, c2, diss)):
        min_d[n + i] = min(min(min_d[int(a)], min_d[int(b)]), float(h))
    for i, (a, b) in enumerate(zip(c1, c2)):
        a, b = int(a), int(b)
        left, right = (a, b) if min_d[a] <= min_d[b] else (b, a)
        order.observe(n + i, left, right)
    return order.ordered_leaves()


def merge_below(c1, c2, diss, threshold):
    """:210-227 with a union-find whose labeling is the representative of each observation."""
    n = len(c1) + 1
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            i = parent[i]
        return i

    to_old = {}
    for i, (a, b, h) in enumerate(zip(c1, c2, diss)):
        if not h < threshold:
            continue
        a, b = to_old.get(int(a), int(a)), to_old.get(int(b), int(b))
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[rb] = ra
        to_old[n + i] = find(a)
    return relabel_vector([find(i) for i in range(n)])


def fcluster(c1, c2, diss, k):
    """:231-239."""
    n = len(c1) + 1
    if k <= 1:
        return [1] * n
    return merge_below(c1, c2, diss, diss[max(n - k, 0)])


# ---- dendrograms ---------------------------------------------------------------------------------------------------------------
def check_dendrogram(c1, c2, diss, size):
    """Every cluster merged exactly once, children before parents, cluster1 < cluster2, sizes add up, heights sorted."""
    n = len(c1) + 1
    sz = [1] * n + [0] * (n - 1)
    used = set()
    for i in range(n - 1):
        a, b = int(c1[i]), int(c2[i])
        assert a < b < n + i, (i, a, b)
        assert a not in used and b not in used
        used.update((a, b))
        sz[n + i] = sz[a] + sz[b]
        assert int(size[i]) == sz[n + i]
    assert used == set(range(2 * n - 2))
    assert np.all(np.diff(np.asarray(diss)) >= 0), "heights must not decrease"


def scipy_steps(x, method):
    from scipy.cluster.hierarchy import linkage

    z = linkage(x, method)
    return z[:, 0].astype(np.uint32), z[:, 1].astype(np.uint32), z[:, 2].copy(), z[:, 3].astype(np.uint32)


def min_relative_gap(diss):
    h = np.sort(np.asarray(diss, dtype=np.float64))
    if len(h) < 2:
        return np.inf
    return float(np.min(np.diff(h) / h[1:]))


def exact_heights(x, method, c1, c2):
    """The heights of the given tree from the methods' definitions, in np.longdouble: Single / Complete the min / max of the member
    distances, Average their mean, Ward sqrt(2|A||B| / (|A| + |B|)) ||c_A - c_B||, Weighted its recursion d(A u B, K) = (d(A, K) +
    d(B, K)) / 2 (which depends on the tree only, not on the order of the merges)."""
    ld = np.longdouble
    x = np.asarray(x, dtype=ld)
    n = x.shape[0]
    diff = x[:, None, :] - x[None, :, :]
    dm = np.sqrt(np.sum(diff * diff, axis=2))
    members = [[i] for i in range(n)]
    out = np.zeros(n - 1, dtype=ld)
    if method == "weighted":
        full = np.zeros((2 * n - 1, 2 * n - 1), dtype=ld)
        full[:n, :n] = dm
    for i in range(n - 1):
        a, b = int(c1[i]), int(c2[i])
        ma, mb = members[a], members[b]
        if method in ("single", "complete", "average"):
            block = dm[np.ix_(ma, mb)]
            out[i] = block.min() if method == "single" else block.max() if method == "complete" else block.sum() / ld(block.size)
        elif method == "ward":
            ca, cb = x[ma].sum(axis=0) / ld(len(ma)), x[mb].sum(axis=0) / ld(len(mb))
            w = ld(2 * len(ma) * len(mb)) / ld(len(ma) + len(mb))
            out[i] = np.sqrt(w) * np.sqrt(np.sum((ca - cb) ** 2))
        else:
            out[i] = full[a, b]
            row = (full[a, :] + full[b, :]) / ld(2)
            full[n + i, :] = row
            full[:, n + i] = row
        members.append(ma + mb)
    return out


def max_relative_deviation(heights, exact):
    exact = np.asarray(exact, dtype=np.longdouble)
    return float(np.max(np.abs(np.asarray(heights, dtype=np.longdouble) - exact) / exact))
