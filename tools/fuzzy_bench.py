"""Time of fuzzy_simplicial_set (umap-rs fuzzy.rs:30-181) on synthetic PCA scores: n x d, lists of width k.

    python tools/fuzzy_bench.py N D K [--metric euclidean|pearson|cosine] [--ref-n M] [--twin-n M]

Reports, one call per figure:
 * the chain through host arrays: nearest_neighbors (lists to the host), then fuzzy_simplicial_set (lists back to the device);
 * the device-resident chain: umap_graph, the lists never leaving the device; and that the two graphs are equal in every bit;
 * fuzzy_simplicial_set alone, then once more in a fresh process with SCANRS_TRACE=1: every kernel stage with the bytes its code
   reads and writes against its time (tracing waits for the device behind every stage, so these add up to more than the call);
 * the pruned edge list (graph.edges(200));
 * the host twin on one thread, on the first --twin-n rows' lists (default 100000), and that the device equals it there;
 * the numpy/scipy restatement of the graph stage on --ref-n rows (default 20000), values compared at 2^-50."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import scanrs_amd as sa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=1_000_000)
ap.add_argument("d", nargs="?", type=int, default=50)
ap.add_argument("k", nargs="?", type=int, default=15)
ap.add_argument("--metric", default="euclidean", choices=["euclidean", "pearson", "cosine"])
ap.add_argument("--ref-n", type=int, default=20_000)
ap.add_argument("--twin-n", type=int, default=100_000)
ap.add_argument("--stages-from", default="")  # internal: the traced run of the graph stage on saved lists
args = ap.parse_args()


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t0) * 1e3


def graph_bits(g):
    indptr, indices, values = g.to_csr()
    return indptr, indices, values.view(np.uint64), g.sigmas.view(np.uint64), g.rhos.view(np.uint64)


def equal(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


if args.stages_from:
    z = np.load(args.stages_from)
    for _ in range(2):  # the first call loads the code objects and fills the allocator's cache
        sa.fuzzy_simplicial_set(z["idx"], z["dist"]).close()
    sys.exit(0)

n, d, k = args.n, args.d, args.k
rng = np.random.default_rng(0)
centres = rng.standard_normal((20, d)) * 2.0
v = (centres[rng.integers(0, 20, size=n)] + rng.standard_normal((n, d))) * np.linspace(1.0, 0.4, d)
sa.umap_graph(v[:2000], k, args.metric).close()  # loads the code objects
(idx, dist), t_knn = timed(lambda: sa.nearest_neighbors(v, k, args.metric))
g_host, t_graph = timed(lambda: sa.fuzzy_simplicial_set(idx, dist))
g_dev, t_chain = timed(lambda: sa.umap_graph(v, k, args.metric))
print(f"fuzzy_bench n={n} d={d} k={k} {args.metric}: through host arrays {t_knn + t_graph:.1f} ms (nearest_neighbors {t_knn:.1f} + "
      f"fuzzy_simplicial_set {t_graph:.1f}, both incl. PCIe); device-resident umap_graph {t_chain:.1f} ms incl. PCIe of the points; "
      f"nnz {g_dev.nnz}; the two graphs equal in every bit: {equal(graph_bits(g_host), graph_bits(g_dev))}", flush=True)
g_dev.close()
(_, t_edges) = timed(lambda: g_host.edges(200.0))
print(f"  edges(200): {g_host.edge_count(200.0)} of {g_host.nnz} entries, {t_edges:.1f} ms incl. the edge arrays to the host", flush=True)
g_host.close()

tmp = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"fuzzy_bench_{os.getpid()}.npz")
np.savez(tmp, idx=idx, dist=dist)
try:
    env = dict(os.environ, SCANRS_TRACE="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), str(n), str(d), str(k), "--stages-from", tmp], env=env, capture_output=True,
                         text=True, timeout=900)
    lines = [ln for ln in out.stderr.splitlines() if "fuzzy stage" in ln]
    per_call = len(lines) // 2  # the first half belongs to the warm-up call
    print("  stages of fuzzy_simplicial_set (traced, a fresh process; stage, ms, bytes moved by the stage's code, GB/s):")
    for ln in lines[per_call:]:
        print("   ", ln.split("fuzzy stage", 1)[1].strip())
    if out.returncode != 0:
        print("  the traced run failed:", out.stderr[-500:])
finally:
    os.remove(tmp)

m = min(n, args.twin_n)
# (lists cut out of a larger set would name rows that are gone: they are made again on the subset)
ti, td = (idx, dist) if m == n else sa.nearest_neighbors(v[:m], k, args.metric)
g_twin, t_twin = timed(lambda: sa.host_fuzzy_simplicial_set(ti, td))
with sa.fuzzy_simplicial_set(ti, td) as g_m:
    same = equal(graph_bits(g_twin), graph_bits(g_m))
print(f"  host twin, one thread, {m} rows: {t_twin:.1f} ms ({t_twin * n / m:.0f} ms scaled to n); the device equals it in every bit: {same}", flush=True)
g_twin.close()

r = min(n, args.ref_n)
ri, rd = (ti, td) if r == m else sa.nearest_neighbors(v[:r], k, args.metric)


def restatement():
    """the graph stage in numpy / scipy.sparse: vectorised bisection with numpy's exponential, R + R^T - R * R^T"""
    import scipy.sparse as sp

    nz = np.where(rd > 0.0, rd, np.inf)
    rho = np.where(np.isfinite(nz.min(axis=1)), np.take_along_axis(rd, np.argmax(rd > 0.0, axis=1)[:, None], 1)[:, 0], 0.0)
    target = np.log2(k)
    lo, mid, hi = np.zeros(r), np.ones(r), np.full(r, np.finfo(float).max)
    live = np.ones(r, bool)
    for _ in range(64):
        psum = np.exp(-np.maximum(rd, 0.0) / mid[:, None]).sum(axis=1)
        live &= ~(np.abs(psum - target) < 1e-5)
        up = live & (psum > target)
        down = live & ~(psum > target)
        hi = np.where(up, mid, hi)
        lo = np.where(down, mid, lo)
        grow = down & (hi == np.finfo(float).max)
        new = np.where(grow, mid * 2.0, lo + (hi - lo) / 2.0)
        mid = np.where(live, new, mid)
    sigma = np.where(rho > 0.0, np.maximum(mid, 1e-3 * rd.mean(axis=1)), np.maximum(mid, 1e-3 * rd.mean()))
    e = rd - rho[:, None]
    val = np.where((e <= 0.0) | (sigma[:, None] == 0.0), 1.0, np.exp(-e / sigma[:, None]))
    val = np.where(ri == np.arange(k)[None, :], 0.0, val)
    rows, cols = ri.ravel(), np.repeat(np.arange(r), k)
    R = sp.csr_matrix((val.ravel() + 1e-300, (rows, cols)), shape=(r, r))  # (explicit zeros would be dropped by the sum below)
    T = sp.csr_matrix(R.T)
    U = sp.csr_matrix(R + T - R.multiply(T))
    U.sort_indices()
    return U


U, t_ref = timed(restatement)
with sa.fuzzy_simplicial_set(ri, rd) as g_r:
    indptr, indices, values = g_r.to_csr()
ok = np.array_equal(indptr, U.indptr) and np.array_equal(indices, U.indices) and bool(np.all(np.abs(values - U.data) <= 2.0 ** -50 + 2e-300))
print(f"  numpy/scipy restatement, {r} rows: {t_ref:.1f} ms ({t_ref * n / r:.0f} ms scaled to n); structure equal and values within 2^-50: {ok}", flush=True)
