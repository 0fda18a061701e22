"""Point sets for the tests of nearest_neighbors under pearson / cosine distance (tests/test_metric_knn_cpu.py,
tests/test_gpu_metric_knn.py): the special inputs of dist.rs:73-124 planted among ordinary rows, and clustered sets with planted
duplicates and near-ties for the filtered route."""
import numpy as np


def special_points(n: int, d: int, seed: int = 0) -> np.ndarray:
    """n x d: Gaussian rows, and from n >= 65 on (where the dimension allows) exact duplicates, constant and all-zero rows, exactly
    orthogonal rows, anti-correlated rows, a large common offset, rows of magnitude 1e200 and 1e-200, and near-ties."""
    rng = np.random.default_rng(1000 * n + d + seed)
    x = rng.standard_normal((n, d))
    if n == 3:
        x[2] = x[0]
    if n < 65:
        return x
    x[1] = x[0]  # exact duplicate: D = 0 up to the formula's own rounding
    x[2] = 2.0 * x[0]  # the same direction
    x[3] = 3.0  # constant rows: degenerate under pearson (s_xx == 0), D = 1 against others, 0 among themselves
    x[5] = -1.5
    x[4] = 0.0  # all-zero rows: degenerate under both kinds
    x[6] = 0.0
    if d >= 4:  # zero mean and exactly orthogonal: the s_xy == 0 branch under both kinds
        x[7] = 0.0
        x[8] = 0.0
        x[7, :4] = [1.0, -1.0, 1.0, -1.0]
        x[8, :4] = [1.0, 1.0, -1.0, -1.0]
    elif d >= 2:  # orthogonal under cosine
        x[7] = 0.0
        x[8] = 0.0
        x[7, :2] = [1.0, 1.0]
        x[8, :2] = [1.0, -1.0]
    x[9] = -x[10]  # anti-correlated: D near 2
    x[11:15] += 1e9  # a large common offset: cancellation in x - mu
    x[15] *= 1e200  # s_xx * s_yy overflows (and s_xy with it: inf / inf = NaN -> 0 by f64::max)
    x[17] *= 1e200
    x[16] *= 1e-200  # every square underflows: s_xx == 0 although the row is not zero
    x[18] *= 1e-100  # s_xx * s_yy underflows to 0 with s_xy != 0: division by zero, run literally (D = 0 or +inf)
    x[25] *= 1e-100
    x[19:24] = x[24] * (1.0 + 1e-9 * rng.standard_normal((5, d)))  # near-ties
    return x


def clustered_points(n: int, d: int, seed: int = 0) -> np.ndarray:
    """n x d for the filtered route: tight Gaussian clusters around random centres (so that neighbours are near-ties), every 97th row
    an exact duplicate of the row before, every 101st a near-duplicate at relative 1e-12 .. 1e-3, every 103rd the mirror image of the
    row before. No degenerate row, magnitudes of order 1."""
    rng = np.random.default_rng(77 * d + seed)
    centres = rng.standard_normal((32, d)) * 2.0
    x = centres[rng.integers(0, 32, size=n)] + 0.05 * rng.standard_normal((n, d))
    for r in range(97, n, 97):
        x[r] = x[r - 1]
    for i, r in enumerate(range(101, n, 101)):
        x[r] = x[r - 1] * (1.0 + 10.0 ** (-12 + i % 10) * rng.standard_normal(d))
    for r in range(103, n, 103):
        x[r] = -x[r - 1]
    if d == 2:  # under pearson two coordinates give rho = +-1 only: keep both kinds non-degenerate (x_0 != x_1)
        same = x[:, 0] == x[:, 1]
        x[same, 1] += 1.0
    return x
