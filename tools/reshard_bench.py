#!/usr/bin/env python
"""The inner-sharding constructor (MultiMat.from_csmat_inner) against the route a caller had before it: scipy's
tocsc() of the feature-major matrix on one host thread, then MultiMat(...) of the transposed triplet.

    python tools/reshard_bench.py [--shards 1,2,4,8] [--cells 1000000] [--genes 33000] [--density 0.03]

Prints one JSON line per shard count: the wall clock of both routes, the phases of the new one (the slowest shard's thread in upload /
count / split / exchange / transposition), the peak device bytes per nonzero of both, the `moved` totals and whether every shard equals
the host route's arrays. ALL SHARDS RUN ON ONE DEVICE: the figures measure the scheme (what is uploaded, counted, exchanged and
sorted, and what it costs on one GPU), not a speed-up over several."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PHASES = ("upload", "count", "split", "exchange", "transpose")


class PeakMemory:
    """device bytes in use by the library, sampled from a side thread while a route runs (scanrs_device_memory_in_use)"""

    def __init__(self, sa, period=0.002):
        self.sa, self.period, self.peak, self._stop = sa, period, 0, threading.Event()
        self._t = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        while not self._stop.is_set():
            self.peak = max(self.peak, self.sa.device_memory_in_use())
            time.sleep(self.period)

    def __enter__(self):
        self.base = self.sa.device_memory_in_use()
        self.peak = self.base
        self._t.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._t.join()
        self.peak = max(self.peak, self.sa.device_memory_in_use())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shards", default="1,2,4,8")
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--genes", type=int, default=33_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()
    import scanrs_amd as sa
    from scanrs_amd.synth import synth_counts_fast

    if not sa.device_available():
        raise SystemExit("reshard_bench needs a gfx950 device")
    t0 = time.perf_counter()
    m = synth_counts_fast(args.cells, args.genes, args.density, args.seed)  # cells x genes CSR = genes x cells CSC
    fm = m.T.tocsr()  # the feature-major matrix a reader hands over: genes x cells CSR (made outside the timed region)
    fm.sort_indices()
    del m
    ip, ix, vv = fm.indptr.astype(np.uint64), fm.indices.astype(np.uint32), fm.data.astype(np.uint32)
    genes, cells, nnz = fm.shape[0], fm.shape[1], int(fm.nnz)
    print(json.dumps({"genes": genes, "cells": cells, "nnz": nnz, "input": "genes x cells CSR", "all_shards_on_device": 0,
                      "setup_s": round(time.perf_counter() - t0, 2)}), flush=True)
    sa.init()
    for n in [int(x) for x in args.shards.split(",")]:
        dev = [0] * n
        sa.release_cached_memory()
        # the route of today: transpose on one host thread, hand the cell-major triplet over
        with PeakMemory(sa) as mem_host:
            t0 = time.perf_counter()
            t = fm.tocsc()
            t_transpose = time.perf_counter() - t0
            tip, tix, tvv = t.indptr.astype(np.uint64), t.indices.astype(np.uint32), t.data.astype(np.uint32)
            t1 = time.perf_counter()
            host = sa.MultiMat(genes, cells, sa.CSC, tip, tix, tvv, n, devices=dev)
            t_host_create = time.perf_counter() - t1
            t_host = time.perf_counter() - t0
        host_shards = [host.shard_csmat(i) for i in range(n)]
        host_ranges = host.shard_ranges()
        host.close()
        del t, tip, tix, tvv
        sa.release_cached_memory()
        with PeakMemory(sa) as mem_new:
            t0 = time.perf_counter()
            mm = sa.MultiMat.from_csmat_inner(genes, cells, sa.CSR, ip, ix, vv, n, devices=dev)
            t_new = time.perf_counter() - t0
        equal = mm.shard_ranges() == host_ranges and all(
            all(np.array_equal(a, b) for a, b in zip(mm.shard_csmat(i), host_shards[i])) for i in range(n))
        info = mm.create_info()
        phases = {p: round(max(mm.counter(f"reshard_{p}_us", i) for i in range(n)) / 1e3, 2) for p in PHASES}
        moved = info["moved"]
        print(json.dumps({
            "shards": n, "host_route_s": round(t_host, 3), "host_tocsc_s": round(t_transpose, 3), "host_create_s": round(t_host_create, 3),
            "inner_route_s": round(t_new, 3), "phase_ms_slowest_shard": phases,
            "peak_device_bytes_per_nnz": {"host_route": round((mem_host.peak - mem_host.base) / nnz, 2), "inner_route": round((mem_new.peak - mem_new.base) / nnz, 2)},
            "uploaded_bytes": int(info["uploaded_bytes"].sum()), "moved_total": int(moved.sum()), "moved_off_diagonal": int(moved.sum() - np.trace(moved)),
            "shards_equal_host_route": bool(equal)}), flush=True)
        mm.close()
        del host_shards


if __name__ == "__main__":
    main()
