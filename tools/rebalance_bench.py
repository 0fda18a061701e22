#!/usr/bin/env python
"""MultiMat.rebalance / gather_outer at the benchmark size - the device-generated 1 M cells x 33 k genes matrix of
bench.py (synth_counts_torch, seed 0, 3 %), genes x cells CSC, the cells sharded - against the route a caller had before them:
to_csmat to the host, scipy, MultiMat(...) of the result.

    python tools/rebalance_bench.py [--shards 1,2,4,8] [--cells 1000000] [--genes 33000] [--density 0.03] [--reps 3]

One JSON line per shard count with three legs:
  (a) partition_on_threshold(3) as tools/select_bench.py runs it, then rebalance(): balance() before and after, the median wall clock
      of `--reps` calls after one warm-up and the phases of the last one (plan; the slowest shard's thread in pull and finish). The
      synthetic matrix is uniform, so that filter leaves the shards as even as they were; (a') is the same after a filter that does
      not: select_cols keeps every cell of the first half and every fourth of the second;
  (b) gather_outer of a shuffled half of the cells, timed the same way;
  (c) the host route for the same two results, timed once: to_csmat, scipy (nothing for (a), a column selection for (b)), MultiMat(...).
and whether every shard of (a) and (b) equals the host route's arrays, the `moved` totals and host_bytes. ALL SHARDS RUN ON ONE
DEVICE: the figures measure the scheme (what goes over the host link and what the pull costs on one GPU), not a speed-up over several."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PHASES = ("plan", "pull", "finish")


def timed(fn, reps):
    """(median ms of `reps` calls after one warm-up, the last result); every call returns synchronised"""
    fn().close()
    ts, out = [], None
    for _ in range(reps):
        if out is not None:
            out.close()
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def report(mm, ms):
    info, n = mm.gather_info(), mm.n_shards
    nnz = mm.nnz()
    phases = {p: round(max(mm.counter(f"regather_{p}_us", i) for i in range(n)) / 1e3, 3) for p in PHASES}
    moved = info["moved"]
    out = {"ms": round(ms, 3), "phase_ms": phases, "nnz": nnz, "moved_total": int(moved.sum()),
           "moved_between_shards": int(moved.sum() - np.trace(moved)) if moved.shape[0] == moved.shape[1] else None,
           "host_bytes": [int(x) for x in info["host_bytes"]], "host_bytes_per_nnz": round(float(info["host_bytes"].sum()) / max(nnz, 1), 6)}
    if phases["pull"] > 0:
        out["pull_GB_per_s"] = round(16.0 * nnz / (phases["pull"] * 1e-3) / 1e9, 1)  # every nonzero read and written, 8 bytes each way
    return out


def rebalance_leg(sa, f, n, devs, reps):
    """rebalance() of the filtered MultiMat f against f.to_csmat() + MultiMat(...)"""
    before = f.balance()
    ms, fb = timed(f.rebalance, reps)
    after = fb.balance()
    leg = report(fb, ms)
    leg.update({"shard_nnz_before": [int(x) for x in before["shard_nnz"]], "imbalance_before": round(before["imbalance"], 4),
                "shard_nnz_after": [int(x) for x in after["shard_nnz"]], "imbalance_after": round(after["imbalance"], 4)})
    t1 = time.perf_counter()
    fip, fix, fvv = f.to_csmat()
    t_down = time.perf_counter() - t1
    host = sa.MultiMat(f.shape()[0], f.shape()[1], sa.CSC, fip, fix, fvv, n, devices=devs)
    leg["host_route_ms"] = round((time.perf_counter() - t1) * 1e3, 1)
    leg["host_route_to_csmat_ms"] = round(t_down * 1e3, 1)
    leg["equals_host_route"] = shards_equal(fb, host)
    host.close()
    fb.close()
    return leg


def shards_equal(a, b):
    return bool(a.shard_ranges() == b.shard_ranges() and all(
        all(np.array_equal(x, y) for x, y in zip(a.shard_csmat(i), b.shard_csmat(i))) for i in range(a.n_shards)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shards", default="1,2,4,8")
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--genes", type=int, default=33_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import scipy.sparse as sp
    import torch

    import scanrs_amd as sa
    from scanrs_amd.synth import synth_counts_torch

    if not sa.device_available():
        raise SystemExit("rebalance_bench needs a gfx950 device")
    t0 = time.perf_counter()
    sa.init()
    dev = torch.device("cuda", 0)
    ip, ix, vv = synth_counts_torch(a.cells, a.genes, a.density, a.seed, dev)
    torch.cuda.synchronize()
    base = sa.AdaptiveMat.from_device(a.genes, a.cells, sa.CSC, ip.data_ptr(), ix.data_ptr(), vv.data_ptr())
    del ip, ix, vv
    torch.cuda.empty_cache()
    hip, hix, hvv = base.to_csmat()  # what a caller hands to MultiMat(...)
    del base
    half = np.random.default_rng(a.seed).permutation(a.cells)[: a.cells // 2].astype(np.uint64)
    print(json.dumps({"genes": a.genes, "cells": a.cells, "nnz": int(hix.shape[0]), "storage": "csc", "all_shards_on_device": 0, "reps": a.reps,
                      "setup_s": round(time.perf_counter() - t0, 2)}), flush=True)
    for n in [int(x) for x in a.shards.split(",")]:
        devs = [0] * n
        sa.release_cached_memory()
        mm = sa.MultiMat(a.genes, a.cells, sa.CSC, hip, hix, hvv, n, devices=devs)
        out = {"shards": n}
        # (a) the filter of select_bench.py, then rebalance()
        f, _, _, _ = mm.partition_on_thresholds(3.0, 3.0, residual=False)
        out["filter_then_rebalance"] = rebalance_leg(sa, f, n, devs, a.reps)  # with (c) for the same result
        f.close()
        sa.release_cached_memory()
        # (a') a filter that hits the second half of the cells harder
        f = mm.select_cols(np.concatenate([np.arange(a.cells // 2), np.arange(a.cells // 2, a.cells, 4)]))
        out["skewed_filter_then_rebalance"] = rebalance_leg(sa, f, n, devs, a.reps)
        f.close()
        sa.release_cached_memory()
        # (b) a shuffled half of the cells
        ms, g = timed(lambda: mm.gather_outer(half), a.reps)
        leg = report(g, ms)
        t1 = time.perf_counter()
        wip, wix, wvv = mm.to_csmat()
        t_down = time.perf_counter() - t1
        whole = sp.csc_matrix((wvv, wix.astype(np.int32), wip.astype(np.int64)), shape=(a.genes, a.cells))
        whole.has_sorted_indices = True
        picked = whole[:, half.astype(np.int64)]
        t_scipy = time.perf_counter() - t1 - t_down
        host = sa.MultiMat(a.genes, half.shape[0], sa.CSC, picked.indptr, picked.indices, picked.data, n, devices=devs)
        leg["host_route_ms"] = round((time.perf_counter() - t1) * 1e3, 1)
        leg["host_route_to_csmat_ms"] = round(t_down * 1e3, 1)
        leg["host_route_scipy_ms"] = round(t_scipy * 1e3, 1)
        leg["equals_host_route"] = shards_equal(g, host)
        out["gather_shuffled_half"] = leg
        host.close()
        g.close()
        mm.close()
        del whole, picked, wip, wix, wvv
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
