"""Time hclust on the device against scipy on the host: `python tools/hclust_bench.py N D METHOD` clusters N standard-normal points
in D dimensions and prints one JSON line: n, d, method, the device distance pass and chain in milliseconds (HIP events), chain steps and
kernel launches, the wall time of the whole call, and scipy's pdist and linkage seconds on the host (--no-scipy leaves them out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("d", type=int)
    ap.add_argument("method")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import scanrs_amd as sa
    from scanrs_amd.hclust import HierarchicalCluster

    x = np.random.default_rng(a.seed).standard_normal((a.n, a.d))
    HierarchicalCluster(x[:64], a.method)  # loads the code object
    t0 = time.perf_counter()
    h = HierarchicalCluster(x, a.method)
    wall = time.perf_counter() - t0
    info = h.info()
    out = {"n": a.n, "d": a.d, "method": a.method, "pdist_ms": info["pdist_ms"], "chain_ms": info["chain_ms"], "chain_steps": info["chain_steps"],
           "launches": info["launches"], "batches": info["batches"], "matrix_bytes": info["matrix_bytes"], "device_call_s": round(wall, 4)}
    if not a.no_scipy:
        from scipy.cluster.hierarchy import linkage
        from scipy.spatial.distance import pdist

        t0 = time.perf_counter()
        y = pdist(x)
        t1 = time.perf_counter()
        z = linkage(y, a.method)
        t2 = time.perf_counter()
        out["scipy_pdist_s"] = round(t1 - t0, 4)
        out["scipy_linkage_s"] = round(t2 - t1, 4)
        s = h.steps
        out["same_tree_as_scipy"] = bool(np.array_equal(s.cluster1, z[:, 0].astype(np.uint32)) and np.array_equal(s.cluster2, z[:, 1].astype(np.uint32)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
