"""The shared grid of the fuzzy_simplicial_set tests (tests/test_fuzzy_cpu.py, tests/test_gpu_fuzzy.py): neighbour
lists of small point sets (made by the host twin of nearest_neighbors, no device), hand-made lists, and the parameter combinations
each of them runs with. A case is (name, indices u32 n x k, distances f64 n x k, params dict, n_epochs)."""
import itertools

import numpy as np

NO_INDEX = 0xFFFFFFFF
SIZES = (2, 3, 65, 257, 1000)
DIMS = (2, 10)
WIDTHS = (1, 2, 15, 33, 128)
LOCAL_CONNECTIVITY = (0.0, 1.0, 1.5, 2.0, 3.25)
SET_OP_MIX_RATIO = (1.0, 0.5, 0.0)
N_ITER = (1, 3, 64)
BANDWIDTH = (1.0, 2.0)
N_EPOCHS = (200.0, 500.0, 7.0)
SEED = 0  # tests/test_fuzzy_cpu.py asserts that the restatement reports no marginal row for it


def points(n: int, d: int, seed: int = SEED) -> np.ndarray:
    """Gaussian points; from n >= 65 on a cluster of four identical points (their lists are all zeros for k <= 3 and start with three
    zeros otherwise) and a pair of identical points (lists that start with one zero)."""
    rng = np.random.default_rng(7919 * n + 31 * d + seed)
    x = rng.standard_normal((n, d))
    if n >= 65:
        x[1] = x[2] = x[3] = x[0]
        x[5] = x[4]
    return x


_LISTS = {}


def lists(sa, n: int, d: int, k: int, distance: str = "euclidean"):
    if (n, d, k, distance) not in _LISTS:
        _LISTS[n, d, k, distance] = sa.host_nearest_neighbors(points(n, d), k, distance)
    return _LISTS[n, d, k, distance]


def star(n: int = 1500):
    """every list names row 0 (in-degree n - 1, across any 1024-wide block); row 0 names rows 1 and 2"""
    idx = np.zeros((n, 2), dtype=np.uint32)
    dist = np.zeros((n, 2))
    for i in range(n):
        idx[i] = (1, 2) if i == 0 else (0, i + 1 if i < n - 1 else 1)
        dist[i] = (0.25 + (i % 7) / 8.0, 1.0 + (i % 5) / 4.0)
    return idx, dist


def padded():
    """n = 3 at the C-level width 5: what scanrs_nearest_neighbors writes for k = 5"""
    idx = np.full((3, 5), NO_INDEX, dtype=np.uint32)
    dist = np.full((3, 5), np.inf)
    idx[:, :2] = [[1, 2], [0, 2], [1, 0]]
    dist[:, :2] = [[0.5, 1.5], [0.5, 2.0], [1.5, 2.0]]
    return idx, dist


def column_is_index():
    """lists whose column j holds index j in some rows (the reference's `j == knn_indices[[i, j]]`)"""
    idx = np.array([[1, 2, 3], [2, 0, 3], [3, 1, 0], [0, 1, 2], [0, 3, 2], [4, 1, 0]], dtype=np.uint32)
    dist = np.array([[0.5, 1.0, 2.0], [0.25, 0.5, 0.75], [1.0, 1.5, 3.0], [0.5, 0.5, 0.5], [1.0, 2.0, 4.0], [0.125, 0.25, 8.0]])
    return idx, dist


def _params(lc, ratio, combine, n_iter, bandwidth):
    return dict(local_connectivity=lc, set_op_mix_ratio=ratio, apply_fuzzy_combine=combine, n_iter=n_iter, bandwidth=bandwidth)


def grid(sa):
    """Every point set with every width; every local_connectivity on each; the other parameters in full product on the small sets and
    rotating on the large ones, so that every value of each occurs with every list shape class."""
    out = []
    rot = itertools.count()
    for n, d in itertools.product(SIZES, DIMS):
        for k in sorted({min(k, n - 1) for k in WIDTHS}):
            if n == 1000 and (k not in (15, 128) or (k == 128 and d != 10)):
                continue
            idx, dist = lists(sa, n, d, k)
            for lc in LOCAL_CONNECTIVITY:
                if n == 1000 and k == 128 and lc not in (1.0, 1.5):
                    continue
                ratios = SET_OP_MIX_RATIO if n <= 65 else (SET_OP_MIX_RATIO[next(rot) % 3],)
                for ratio in ratios:
                    r = next(rot)
                    out.append((f"gauss-n{n}-d{d}-k{k}-lc{lc}-r{ratio}", idx, dist,
                                _params(lc, ratio, True, N_ITER[r % 3] if lc != 1.0 or ratio != 1.0 else 64, BANDWIDTH[r % 2]), N_EPOCHS[r % 3]))
            out.append((f"gauss-n{n}-d{d}-k{k}-R", idx, dist, _params(1.0, 1.0, False, 64, 1.0), N_EPOCHS[next(rot) % 3]))
    for name, (idx, dist) in (("star", star()), ("padded", padded()), ("column-is-index", column_is_index())):
        for lc in (1.0, 2.0):
            out.append((f"{name}-lc{lc}", idx, dist, _params(lc, 1.0, True, 64, 1.0), 200.0))
        out.append((f"{name}-mix", idx, dist, _params(1.0, 0.5, True, 3, 2.0), 7.0))
        out.append((f"{name}-R", idx, dist, _params(1.0, 1.0, False, 64, 1.0), 500.0))
    return out


def refusal_cases():
    """(name, indices, distances, keyword arguments, what the message must hold)"""
    idx, dist = np.array([[1, 2], [0, 2], [1, 0], [0, 1]], dtype=np.uint32), np.array([[0.5, 1.5], [0.5, 2.0], [1.5, 2.0], [1.0, 3.0]])

    def with_(i=None, d=None):
        a, b = idx.copy(), dist.copy()
        for (r, c), v in (i or {}).items():
            a[r, c] = v
        for (r, c), v in (d or {}).items():
            b[r, c] = v
        return a, b

    return [
        ("nan", *with_(d={(2, 1): np.nan}), {}, "row 2 "),
        ("nan first", *with_(d={(3, 0): np.nan, (1, 1): np.nan}), {}, "row 1 "),
        ("index", *with_(i={(1, 0): 4}), {}, "row 1 "),
        ("index huge", *with_(i={(3, 1): 0xFFFFFFFE}), {}, "row 3 "),
        ("repeat", *with_(i={(2, 1): 1}), {}, "row 2 "),
        ("rho index == len", *with_(d={(1, 0): 0.0}), dict(local_connectivity=1.5), "row 1 "),
        ("rho index == len, lc 2.5", idx, dist, dict(local_connectivity=2.5), "row 0 "),
        ("rho empty", *with_(d={(3, 0): 0.0, (3, 1): 0.0}), dict(local_connectivity=0.0), "row 3 "),
        ("rho empty lc 0.5", *with_(d={(2, 0): 0.0, (2, 1): -1.0}), dict(local_connectivity=0.5), "row 2 "),
        ("k == 0", np.zeros((4, 0), np.uint32), np.zeros((4, 0)), {}, "no rows or no columns"),
        ("n == 0", np.zeros((0, 2), np.uint32), np.zeros((0, 2)), {}, "no rows or no columns"),
        ("k > 128", np.zeros((2, 129), np.uint32), np.ones((2, 129)), {}, "128"),
        ("lc nan", idx, dist, dict(local_connectivity=np.nan), "local_connectivity"),
        ("lc inf", idx, dist, dict(local_connectivity=np.inf), "local_connectivity"),
        ("lc negative", idx, dist, dict(local_connectivity=-0.5), "local_connectivity"),
        ("ratio inf", idx, dist, dict(set_op_mix_ratio=np.inf), "set_op_mix_ratio"),
        ("ratio nan", idx, dist, dict(set_op_mix_ratio=np.nan), "set_op_mix_ratio"),
    ]
