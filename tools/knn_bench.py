"""Throughput of the exact kNN (scan_rs::nn::knn) on synthetic PCA scores: n x d, k neighbours; the matrix-core filter path
(bf16 MFMA filter + exact f64 rerank) against the exhaustive f64 kernel (global option "knn_exhaustive"), results compared.

    python tools/knn_bench.py N D K [both] [--shards S[,S...]] [--block-rows R]
    python tools/knn_bench.py N D K --metric euclidean|pearson|cosine [--shards S[,S...]] [--block-rows R]

--metric: nearest_neighbors (umap-rs knn.rs:112-166) on the same points instead: the route, the filter rounds with their
candidates per query, and the time of the call; up to 20000 points the result is compared with the host twin bit for bit. With
--shards also MultiMat.nearest_neighbors on S shards of device 0: time, blocks, blocks searched through the filter per shard,
exchange steps, communicator bytes, shard 0's device time by scope, and the bit comparison with the unsharded call.

--shards: the same points through a MultiMat whose S shards share device 0: time per call, the blocks and exchange
steps, the bytes that went through a shard's communicator, the candidates per query of the last block searched, the share of shard
0's device time in exchange / search / merge, and whether the indices equal the unsharded call's bit for bit."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import scanrs_amd as sa

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=100_000)
ap.add_argument("d", nargs="?", type=int, default=50)
ap.add_argument("k", nargs="?", type=int, default=15)
ap.add_argument("both", nargs="?", default="")
ap.add_argument("--shards", default="")
ap.add_argument("--block-rows", type=int, default=0)
ap.add_argument("--metric", default="", choices=["", "euclidean", "pearson", "cosine"])
args = ap.parse_args()
n, d, k = args.n, args.d, args.k
also_exhaustive = args.both == "both" or n <= 300_000
rng = np.random.default_rng(0)
centres = rng.standard_normal((20, d)) * 2.0
v = (centres[rng.integers(0, 20, size=n)] + rng.standard_normal((n, d))) * np.linspace(1.0, 0.4, d)
sa.knn(v[:1000], k)
if args.metric:
    sa.nearest_neighbors(v[:1000], k, args.metric)
    t0 = time.perf_counter()
    idx, dist = sa.nearest_neighbors(v, k, args.metric)
    dt = time.perf_counter() - t0
    st = sa.debug_knn_last_stats()
    rounds = ", ".join(f"stride {r['stride']}: {r['cand_sum'] / n:.1f} (max {r['cand_max']}, {r['overflowed']} overflowed)" for r in st["rounds"])
    print(f"nearest_neighbors[{args.metric}] n={n} d={d} k={k}: {dt*1e3:.1f} ms incl. PCIe of the points, {n/dt:.0f} cells/s; "
          f"route {'filtered' if st['filtered'] else 'exhaustive'}, {len(st['rounds'])} filter rounds, candidates per query {rounds or '-'}; "
          f"first row {idx[0][:5]} {dist[0][:3]}", flush=True)
    if n <= 20000:
        hi, hd = sa.host_nearest_neighbors(v, k, args.metric)
        print("equals the host twin:", bool(np.array_equal(idx, hi) and np.array_equal(dist.view(np.uint64), hd.view(np.uint64))))
    if args.block_rows:
        sa.set_global_option("knn_block_rows", args.block_rows)
    for shards in [int(x) for x in args.shards.split(",") if x]:  # the same call through a MultiMat whose shards share device 0 (§7q)
        mm = sa.MultiMat(1, n, sa.CSC, np.arange(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.uint32), np.ones(n, dtype=np.uint32), shards,
                         devices=[0] * shards)
        before = mm.comm_info(0)
        mm.profile_enable(True)
        t0 = time.perf_counter()
        sidx, sdist = mm.nearest_neighbors(k, v, args.metric)
        dt = time.perf_counter() - t0
        prof = {name: c["total_ms"] for name, c in mm.profile_get(0).items()}
        after = mm.comm_info(0)
        total = sum(prof.values()) or 1.0
        share = ", ".join(f"{name} {prof.get(name, 0.0):.1f} ms ({100.0 * prof.get(name, 0.0) / total:.0f} %)"
                          for name in ("allreduce_u64", "knn_search", "knn_merge"))
        equal = bool(np.array_equal(sidx, idx) and np.array_equal(sdist.view(np.uint64), dist.view(np.uint64)))
        print(f"nearest_neighbors[{args.metric}, sharded x{shards}] n={n} d={d} k={k}: {dt*1e3:.1f} ms incl. PCIe of the points, {n/dt:.0f} cells/s; "
              f"knn_blocks {mm.counter('knn_blocks')}, knn_blocks_filtered {[mm.counter('knn_blocks_filtered', shard=i) for i in range(shards)]}, "
              f"knn_allreduces {mm.counter('knn_allreduces')}, "
              f"communicator of shard 0: {after['allreduce_calls'] - before['allreduce_calls']} all-reduces, "
              f"{(after['allreduce_bytes'] - before['allreduce_bytes']) / 2**20:.1f} MiB; "
              f"shard 0 device time: {share}; equals the unsharded call in indices and distance bits: {equal}", flush=True)
        mm.close()
    sys.exit(0)
res = {}
for mode in (["filter", "exhaustive"] if also_exhaustive else ["filter"]):
    sa.set_global_option("knn_exhaustive", 1 if mode == "exhaustive" else 0)
    t0 = time.perf_counter()
    out = sa.knn(v, k)
    dt = time.perf_counter() - t0
    res[mode] = out
    flops = 3.0 * n * n * d  # subtract + fused multiply-add per coordinate pair
    print(f"knn[{mode}] n={n} d={d} k={k}: {dt*1e3:.1f} ms incl. PCIe of the points, {n/dt:.0f} cells/s, "
          f"{flops/dt/1e12:.2f} TFLOP/s f64-equivalent, first row {out[0][:5]}", flush=True)
if len(res) == 2:
    print("identical:", bool(np.array_equal(res["filter"], res["exhaustive"])))
sa.set_global_option("knn_exhaustive", 0)


if args.block_rows:
    sa.set_global_option("knn_block_rows", args.block_rows)
for shards in [int(x) for x in args.shards.split(",") if x]:
    ones = np.ones(n, dtype=np.uint32)  # a genes x cells CSC matrix with one count per cell: the handle gives the cut and the transport
    mm = sa.MultiMat(1, n, sa.CSC, np.arange(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.uint32), ones, shards, devices=[0] * shards)
    before = mm.comm_info(0)
    mm.profile_enable(True)
    t0 = time.perf_counter()
    out = mm.knn(k, v)
    dt = time.perf_counter() - t0
    prof = {name: c["total_ms"] for name, c in mm.profile_get(0).items()}
    after = mm.comm_info(0)
    st = sa.debug_knn_last_stats()
    per_q = n / shards
    rounds = ", ".join(f"stride {r['stride']}: {r['cand_sum'] / per_q:.1f} (max {r['cand_max']}, {r['overflowed']} overflowed)" for r in st["rounds"])
    total = sum(prof.values()) or 1.0
    share = ", ".join(f"{name} {prof.get(name, 0.0):.1f} ms ({100.0 * prof.get(name, 0.0) / total:.0f} %)"
                      for name in ("allreduce_u64", "knn_search", "knn_merge"))
    print(f"knn[sharded x{shards}] n={n} d={d} k={k}: {dt*1e3:.1f} ms incl. PCIe of the points, {n/dt:.0f} cells/s; "
          f"knn_blocks {mm.counter('knn_blocks')}, knn_allreduces {mm.counter('knn_allreduces')}, "
          f"communicator of shard 0: {after['allreduce_calls'] - before['allreduce_calls']} all-reduces, "
          f"{(after['allreduce_bytes'] - before['allreduce_bytes']) / 2**20:.1f} MiB; "
          f"last block searched {'filtered' if st['filtered'] else 'exhaustive'}, candidates per query (about {per_q:.0f} queries) {rounds or '-'}; "
          f"shard 0 device time: {share}; equals the unsharded call: {bool(np.array_equal(out, res['filter']))}", flush=True)
    mm.close()
