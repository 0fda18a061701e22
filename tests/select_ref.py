"""numpy / scipy restatement of sqz::AdaptiveMat::select_rows, select_cols and partition_on_thresholds (sqz/src/mat.rs:766-888,
1004-1071), the checker of tests/test_select_cpu.py and tests/test_gpu_select.py. Counts are integers, so every comparison made
with it is exact."""
import numpy as np
from scipy import sparse


def quantile_threshold(sums, q=0.1):
    """The reference test's choice of threshold (mat.rs:1501-1504): the q-quantile of the axis sums, midpoint interpolation."""
    return float(np.quantile(np.asarray(sums, dtype=np.float64), q, method="midpoint"))


def partition_sets(m, row_threshold, col_threshold):
    """The loop of mat.rs:783-806 on a scipy matrix: (excluded rows mask, excluded columns mask, rounds). A round: the column sums
    over the rows not yet excluded, columns with sum < threshold join the excluded set; then the row sums over the columns not yet
    excluded (as just updated); until a round adds nothing. `rounds` counts that last round too. None = no threshold."""
    csr = sparse.csr_matrix(m).astype(np.int64)
    csc = csr.tocsc()
    rows, cols = csr.shape
    ex_r, ex_c = np.zeros(rows, dtype=bool), np.zeros(cols, dtype=bool)
    rounds = 0
    while True:
        updated = False
        if col_threshold is not None:
            s = np.asarray(csc.T @ (~ex_r).astype(np.int64)).ravel()  # exact integers
            new = (s.astype(np.float64) < col_threshold) & ~ex_c
            updated |= bool(new.any())
            ex_c |= new
        if row_threshold is not None:
            s = np.asarray(csr @ (~ex_c).astype(np.int64)).ravel()
            new = (s.astype(np.float64) < row_threshold) & ~ex_r
            updated |= bool(new.any())
            ex_r |= new
        rounds += 1
        if not updated:
            return ex_r, ex_c, rounds


def partition_on_thresholds(m, row_threshold, col_threshold):
    """(filtered, residual, selected_rows, selected_cols, rounds): filtered = kept rows x kept columns, residual = kept rows x
    excluded columns in ascending source order, both CSR scipy matrices with sorted indices."""
    ex_r, ex_c, rounds = partition_sets(m, row_threshold, col_threshold)
    csr = sparse.csr_matrix(m)
    sel_r, sel_c, gone_c = np.flatnonzero(~ex_r), np.flatnonzero(~ex_c), np.flatnonzero(ex_c)
    kept = csr[sel_r]
    return canonical(kept[:, sel_c]), canonical(kept[:, gone_c]), sel_r, sel_c, rounds


def partition_on_threshold(m, threshold):
    return partition_on_thresholds(m, threshold, threshold)


def partition_dense(dense, row_threshold, col_threshold):
    """The reference test's own dense procedure (mat.rs:1511-1554): dense sums over the non-excluded rows / columns, dense
    `select`. Both thresholds given. Returns (filtered, residual, selected_rows, selected_cols, rounds)."""
    dense = np.asarray(dense).astype(np.int64)
    rows, cols = dense.shape
    excl_rows, excl_cols = set(), set()
    rounds = 0
    while True:
        updated = False
        s = np.zeros(cols, dtype=np.int64)
        for r in range(rows):
            if r not in excl_rows:
                s += dense[r]
        for c in range(cols):
            if s[c] < col_threshold and c not in excl_cols:
                excl_cols.add(c)
                updated = True
        s = np.zeros(rows, dtype=np.int64)
        for c in range(cols):
            if c not in excl_cols:
                s += dense[:, c]
        for r in range(rows):
            if s[r] < row_threshold and r not in excl_rows:
                excl_rows.add(r)
                updated = True
        rounds += 1
        if not updated:
            break
    incl_rows = [r for r in range(rows) if r not in excl_rows]
    incl_cols = [c for c in range(cols) if c not in excl_cols]
    gone = sorted(excl_cols)
    filt = dense[incl_rows]
    return filt[:, incl_cols], filt[:, gone], np.array(incl_rows, dtype=np.int64), np.array(incl_cols, dtype=np.int64), rounds


def select_rows(m, idx):
    """Row i of the result is row idx[i] (any order, repeats allowed). Dense fancy indexing for dense input, `m[idx]` for sparse."""
    idx = np.asarray(idx, dtype=np.int64)
    if sparse.issparse(m):
        return canonical(sparse.csr_matrix(m)[idx])
    return np.asarray(m)[idx]


def select_cols(m, idx):
    idx = np.asarray(idx, dtype=np.int64)
    if sparse.issparse(m):
        return canonical(sparse.csc_matrix(m)[:, idx])
    return np.asarray(m)[:, idx]


def canonical(m, storage="csr"):
    """CSR (or CSC) with sorted indices, no stored zeros, no duplicates: the arrays `to_csmat` is compared with."""
    m = sparse.csr_matrix(m) if storage == "csr" else sparse.csc_matrix(m)
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    return m


def triplet(m, storage):
    """(indptr u64, indices u32, data u32) of a scipy matrix in the named storage ("csr" / "csc")."""
    c = canonical(m, storage)
    return c.indptr.astype(np.uint64), c.indices.astype(np.uint32), c.data.astype(np.uint32)


def cascade_matrix(n=4, threshold=10):
    """A hand-made cascade for `partition_on_threshold(threshold)`: a staircase a[r, r] = a[r, r + 1] = 6 (r < n) beside a block that
    stays. Only column 0 (sum 6, plus a stray 1) starts below 10; without it row 0 is left with 6, without row 0 column 1 is left with
    6, and so on: one column and one row per round, 2 n links, n + 1 rounds. Returns (dense matrix, excluded rows, excluded
    columns, rounds)."""
    assert threshold == 10 and n >= 3
    size = n + 3
    a = np.zeros((size, size), dtype=np.int64)
    for r in range(n):
        a[r, r] = 6
        a[r, r + 1] = 6
    a[n:, n:] += 10  # rows and columns of the block sum to 30 and more
    a[n + 1, 0] = 1  # entries that end up in the residual matrix
    a[n + 2, 2] = 2
    gone = np.arange(n, dtype=np.int64)
    return a, gone, gone.copy(), n + 1


def synth_genes_by_cells(n_cells, n_genes, density, seed=3, **kw):
    """genes x cells CSR from the package's generator (which makes cells x genes); arguments in the generator's order."""
    from scanrs_amd.synth import synth_counts_fast

    m = synth_counts_fast(n_cells, n_genes, density, seed, **kw)
    return canonical(m.T)
