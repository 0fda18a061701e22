#!/usr/bin/env python3
"""bench.py — cells/sec for top-k PCA (CellRanger normalisation + BkSvd) on a synthetic sparse count matrix.

One "step" = one pass of the hot path over the whole matrix already resident in HBM:
reset the lazy map -> normalize(CellRanger) -> BkSvd{2.0, 5}.run_pca(k), through the C ABI
(include/scanrs_amd.h). Default workload = BASELINE.json configs[2]: 1M cells x 33k genes @ 3 % nnz, k = 50, 1 GPU.

`python bench.py --gpus N` works as typed: with N > 1 and no WORLD_SIZE in the environment it starts
`python -m torch.distributed.run --nproc-per-node N bench.py ...` as a child BEFORE anything touches the GPU and relays
rank 0's JSON line; under torchrun (the driver's form) every rank takes LOCAL_RANK's GPU. The same global matrix is
range-partitioned over the ranks by nonzeros (scanrs_plan_shards; strong scaling); the exchange steps run inside the
library (RCCL over xGMI, `scanrs_comm_*`), torch.distributed (gloo) is only the control plane (id broadcast, barriers,
max over ranks). Rank 0 prints ONE JSON line.

`value` is what a caller of `run_pca` gets: the rate of steps that return U, sigma and V as host arrays, as the reference's
signature does (scan-rs/src/dim_red/mod.rs:47); `config.device_resident_cells_per_s` is the rate with U and V left in HBM
(scanrs_pca_result_device) for device-side consumers, `config.first_call_s` the cold create -> normalize -> run_pca on a
fresh handle (the transposed copy and the tile layouts of the hybrid product are built there).

A plain run sets up, warms up, times the K steps and prints the line; everything else is measured with `--full` only:
the device-resident rate (a second pass of K steps with per-launch HIP events), the step with fresh result arrays,
RandSvd, IRLBA, the replicated / sharded split, the heavy-tailed profile, roofline — HBM roofline of the dominant kernel,
algorithmic bytes per launch / average launch duration measured with HIP events on the library's stream — and
cpu_baseline — the CPU oracle (port of the reference's serial schedule) on 1 core and on all cores, bounded samples,
rank 0 at N = 1 only. `--dump-outputs DIR` writes U, sigma and V of the last timed step as .npy files.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s (spec)
LDS_PEAK_TBS = 150.0   # MI355X_MICROARCH.md, LDS: ds_read_b128 = 256 B/clk/CU, "aggregate with every CU streaming (~2.4 GHz): ~150 TB/s"
LDS_SURVEY_TBS = 78.6  # SURVEY.md §8d's estimate (128 B/clk/CU x 256 CUs x 2.4 GHz), kept beside it
PMC_PROFILE = "r06i_pmc_traffic.json"  # committed PMC passes (separate --pmc runs) the `traffic` field is read from
KERNEL_SOURCES = ("scan-rs_amd/csrc/tiles.hip", "scan-rs_amd/csrc/tiles_dense.inc", "scan-rs_amd/csrc/tile_dense_body.inc", "scan-rs_amd/csrc/tile_dense_body_tabo.inc",
                  "scan-rs_amd/csrc/tile_dense_body_tabi.inc", "scan-rs_amd/csrc/kernels.hip",
                  "scan-rs_amd/csrc/device_map.hpp")


SHARDED_KERNEL_PREFIXES = ("spmm_", "tile_weights", "row_reduce", "col_moments", "col_sums", "materialize_map_values")  # work over the rank's own cells only
DUMP_BYTES = 60_000_000  # --dump-outputs: all files together stay under 64 MB, .npy headers included; U may take half of it
DUMP_SEED = 20240917


def dump_rows(n_rows, row_bytes, budget):
    """Rows of an n_rows-row factor that --dump-outputs writes: None (all of them) when they fit the budget, otherwise a sample
    drawn from a fixed seed, sorted - the same rows in every run with the same arguments."""
    import numpy as np

    if n_rows * row_bytes <= budget:
        return None
    return np.sort(np.random.default_rng(DUMP_SEED).choice(n_rows, size=budget // row_bytes, replace=False))


def split_replicated_sharded(ms_full, ms_part, frac):
    """A step on a cell range of share f of the matrix takes t(f) = replicated + sharded * f: what does not shrink with the range
    (gene-side chains, the q x q eigenproblem, U's delivery) and what does (sparse passes, cell-side dense work, V's delivery).
    From the step on the whole matrix (f = 1) and on a part of it (f = frac): the two terms at f = 1, clamped to [0, ms_full]."""
    sharded = (ms_full - ms_part) / (1.0 - frac)
    sharded = min(max(sharded, 0.0), ms_full)
    return {"replicated_ms_per_step": round(ms_full - sharded, 2), "sharded_ms_per_step": round(sharded, 2)}


def sharded_share_of_rank(sharded_ms, nnz_rank, nnz_total):
    """the sharded term of one rank of a cell-range partition: the ranges are cut by nonzeros (scanrs_plan_shards)"""
    return sharded_ms * nnz_rank / max(1, nnz_total)


def kernel_source_hash():
    """sha256 over the sources of the sparse kernels: the committed PMC file carries the hash of the sources it was measured on, and
    `traffic` is only quoted from it when the sources loaded now are the same (profiles/summarize.py writes it)."""
    import hashlib

    h = hashlib.sha256()
    for rel in KERNEL_SOURCES:
        with open(os.path.join(ROOT, rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--genes", type=int, default=33_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cpu-cells", type=int, default=16000, help="cells of the 1-core CPU-baseline sample")
    ap.add_argument("--cpu-cells-all", type=int, default=100000, help="cells of the all-core CPU-baseline sample")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-reserve", action="store_true", help="do not reserve device memory ahead of the handle (scanrs_reserve_device_memory)")
    ap.add_argument("--reserve-bytes-per-nnz", type=float, default=None,
                    help="size of that reserve per nonzero of the shard (+ 1 GB). Default: computed from what the handle keeps after its first PCA - per nonzero "
                         "both copies of the matrix 16 B, both tile layouts 2 x 4.7 B (records only: the map is evaluated inside the kernel since round 6), 2 B of small change; per cell the solver's two projection panels "
                         "(2 x 8 B x 2 k n_iter) and six b-wide panels - with the builds' temporaries in the room the panels take later")
    ap.add_argument("--no-heavy-tailed", action="store_true", help="skip the second, clearly labelled measurement on the heavy-tailed gene profile")
    ap.add_argument("--no-host-delivery", action="store_true", help="leave U and V in HBM in every step (value is then the device-resident rate)")
    ap.add_argument("--f32-panels", action="store_true",
                    help="opt-in fast mode: gathered panels rounded to f32, f64 sums (NOT the headline configuration)")
    ap.add_argument("--spmm-path", type=int, default=0, help="0 auto, 1 plain gather, 2 L2-blocked gather")
    ap.add_argument("--also-randsvd", action="store_true", help="(default at 1 GPU since round 5) also time one RandSvd{10, 2} PCA (SURVEY.md §8d: reported alongside)")
    ap.add_argument("--no-randsvd", action="store_true", help="skip the RandSvd measurement")
    ap.add_argument("--no-irlba", action="store_true", help="skip the IRLBA measurement")
    ap.add_argument("--no-split-probe", action="store_true", help="skip the replicated / sharded split of the step (a second matrix with half the cells)")
    ap.add_argument("--also-irlba", action="store_true",
                    help="also time one Irlba{tol 1e-4, 50} run on the log-normalised (un-centred) matrix, the only input irlba.rs takes")
    ap.add_argument("--also-knn", type=int, default=0, metavar="K", help="also time scanrs_knn_device (K neighbours) on the device-resident scores")
    ap.add_argument("--force-collective", action="store_true",
                    help="N=1 only: serve the exchange steps through RCCL (world 1) anyway, to price the transport itself")
    ap.add_argument("--events-in-timed-region", action="store_true",
                    help="record the per-launch HIP events inside the K timed steps instead of in a second pass of K steps")
    ap.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE", help="scanrs_mat_set_option on the handle (experiments)")
    ap.add_argument("--sqz-bench", action="store_true",
                    help="instead: the reference's only benchmark (sqz/benches/my_benchmark.rs): u32 CSR / CSC 1000 x 10000 times 10000 x 16")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything besides the headline figure: device-resident rate, fresh result arrays, RandSvd, IRLBA, "
                         "replicated / sharded split, heavy-tailed profile, roofline, CPU baseline (each still switched off by its --no-* option)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write U, sigma and V of the last one as DIR/{u,s,v}.npy (float64); a factor whose rows "
                         f"exceed its share of {DUMP_BYTES // 10**6} MB is written as a fixed seeded sample of its rows, in row order")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


class Watchdog:
    """Every rank: if no stage marker is set for `limit` seconds, print where every stage started and leave with a non-zero
    code (os._exit: the main thread may be stuck inside a collective) — a hung multi-rank run ends with a reason, not a kill."""

    def __init__(self, rank, limit):
        import threading

        self.rank, self.limit, self.stages, self.done = rank, limit, [("start", time.time())], False
        threading.Thread(target=self._run, daemon=True).start()

    def stage(self, name):
        self.stages.append((name, time.time()))

    def _run(self):
        while not self.done:
            time.sleep(2.0)
            name, t = self.stages[-1]
            if time.time() - t > self.limit and not self.done:
                t0 = self.stages[0][1]
                trail = "; ".join(f"{n} @ {tt - t0:.1f}s" for n, tt in self.stages[-12:])
                sys.stderr.write(f"[bench rank {self.rank}] WATCHDOG: stage '{name}' has run for more than {self.limit:.0f} s — {trail}\n")
                sys.stderr.flush()
                os._exit(3)


def self_launch(args):
    """`python bench.py --gpus N` typed by hand (no torchrun): start the N ranks as a CHILD process group before this
    process has touched the GPU (never exec after HIP initialisation) and relay their single JSON line."""
    port = 29500 + (os.getpid() % 2000)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in p.stdout.splitlines():
        if ln.startswith("{") and '"metric"' in ln:
            line = ln
    if line:
        print(line)
    else:
        sys.stderr.write(p.stdout)
    sys.exit(p.returncode if p.returncode else (0 if line else 1))


def sqz_bench(args):
    """sqz/benches/my_benchmark.rs:7-35: `mat_densemat_mult` of a random 1000 x 10000 u32 AdaptiveMat (gen_rand.rs:24-61:
    every vector keeps Uniform(0, len) index draws from [1, len), deduplicated; values in [1, 50)) with a dense
    10000 x 16 u32 matrix (values in [0, 100)), once stored CSR and once CSC."""
    import numpy as np

    import scanrs_amd as sa

    rows, cols, rng_range, cols2 = 1000, 10000, 50, 16
    rng = np.random.default_rng(0)
    res = {}
    for name, storage in (("csr-mul 1k", sa.CSR), ("csc-mul 1k", sa.CSC)):
        n_outer, n_inner = (rows, cols) if storage == sa.CSR else (cols, rows)
        ip, ix, vv = [0], [], []
        for _ in range(n_outer):
            nnz = int(rng.integers(0, n_inner)) if n_inner else 0
            idx = np.unique(rng.integers(1, n_inner, size=nnz)) if nnz else np.zeros(0, dtype=np.int64)
            ix.append(idx.astype(np.uint32))
            vv.append(rng.integers(1, rng_range, size=idx.shape[0]).astype(np.uint32))
            ip.append(ip[-1] + idx.shape[0])
        ip, ix, vv = np.array(ip, dtype=np.uint64), np.concatenate(ix), np.concatenate(vv)
        m2 = rng.integers(0, 100, size=(cols, cols2)).astype(np.uint32)
        g = sa.AdaptiveMat.from_csmat(rows, cols, storage, ip, ix, vv)
        out = g.dot(m2)  # warm (uploads, transposed copy where the kernel wants it)
        g.profile_reset()
        g.profile_enable(True)
        t0 = time.perf_counter()
        reps = 20
        for _ in range(reps):
            out = g.dot(m2)
        wall = (time.perf_counter() - t0) / reps
        g.profile_enable(False)
        prof = g.profile_get()
        kern = sum(v["total_ms"] for k, v in prof.items() if "spmm" in k or "slab" in k) / reps
        cpu = None
        if not args.no_cpu_baseline:  # the CPU port timed beside it (and used as the checker of the device result)
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
            import scanrs_oracle as so

            o = so.AdaptiveMat(rows, cols, so.CSR if storage == sa.CSR else so.CSC, ip, ix, vv)
            so.build()
            t0 = time.perf_counter()
            ref = o.dot(m2)
            cpu = time.perf_counter() - t0
            assert np.array_equal(out, ref), "u32 product differs from the oracle"
        nnz = int(ip[-1])
        res[name] = {"nnz": nnz, "gpu_call_ms": round(wall * 1e3, 3), "gpu_kernel_ms": round(kern, 4), "cpu_port_1core_ms": None if cpu is None else round(cpu * 1e3, 2),
                     "kernel_GBps_algorithmic": round((nnz * 8 + (n_outer + 1) * 8 + (cols + rows) * cols2 * 4) / (kern * 1e-3) / 1e9, 1) if kern > 0 else None}
    print(json.dumps({"metric": "sqz/benches/my_benchmark.rs mirror: u32 mat_densemat_mult 1000x10000 (x) 10000x16", "unit": "ms per product",
                      "results": res, "note": "gpu_call_ms includes the host->device copy of the dense operand and the device->host copy of "
                      "the result (scanrs_mat_dot_u32 takes host pointers as prod.rs takes ArrayViews); bit-exact against the oracle"}))


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)
    import numpy as np
    import torch

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))

    wd = Watchdog(rank, float(os.environ.get("SCANRS_BENCH_WATCHDOG_S", "600")))

    def dbg(msg):  # stage markers: kept for the watchdog, printed with SCANRS_BENCH_DEBUG=1 (where does a multi-rank run stop?)
        wd.stage(msg)
        if os.environ.get("SCANRS_BENCH_DEBUG"):
            print(f"[bench rank {rank}] {msg} t={time.time():.3f}", file=sys.stderr, flush=True)

    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # SCANRS_BENCH_SHARED_GPU=1 (tests only): every rank uses GPU 0 and the exchange steps go through the host hook on
    # gloo (RCCL cannot put two ranks on one device), so the N > 1 flow runs end to end on a 1-GPU box. Never set by the driver.
    shared_gpu = os.environ.get("SCANRS_BENCH_SHARED_GPU") == "1"
    if shared_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    free_at_start = torch.cuda.mem_get_info(dev)[0]
    dist = None
    if world > 1:
        import torch.distributed as dist_mod

        dist = dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("gloo", rank=rank, world_size=world)  # control plane only
    # the image exports NCCL_DEBUG=VERSION and RCCL prints that banner with printf on stdout in every rank — stdout
    # carries the ONE JSON line, so the banner level (only that one) is switched off; INFO/TRACE etc. are left alone
    if os.environ.get("NCCL_DEBUG", "").upper() == "VERSION":
        os.environ["NCCL_DEBUG"] = ""

    import scanrs_amd as sa
    from scanrs_amd.synth import synth_counts_torch

    if not sa.device_available():
        raise SystemExit("bench.py needs a gfx950 device (no CPU fallback)")
    t_i = time.perf_counter()
    sa.init()  # loads the library's code objects, starts the one-off table computation of the seeded start panels (include/scanrs_amd.h)
    t_init = time.perf_counter() - t_i
    if args.sqz_bench:
        return sqz_bench(args)

    # ---- synthetic shard, generated in device memory; partition balanced by nonzeros ----------------------------
    from scanrs_amd.dist import shard_bounds

    lo, hi = shard_bounds(args.cells, world)[rank]
    t0 = time.time()
    dbg("datagen")
    def generate(lo_, hi_):
        # ranks that share one GPU (test mode) take turns: four processes generating at once on one device were measured
        # ~170x slower than one after the other (172 s instead of ~1 s for 50 k cells each; round 2's "hung" runs were this)
        if shared_gpu and dist is not None:
            out = None
            for r in range(world):
                if r == rank:
                    out = synth_counts_torch(args.cells, args.genes, args.density, args.seed, dev, lo_, hi_)
                    torch.cuda.synchronize()
                dist.barrier()
            return out
        return synth_counts_torch(args.cells, args.genes, args.density, args.seed, dev, lo_, hi_)

    indptr, indices, values = generate(lo, hi)
    dbg("datagen done")
    if world > 1:
        # scanrs_plan_shards on the global per-cell counts (every rank holds the counts of its equal-count range)
        counts = (indptr[1:] - indptr[:-1]).cpu()
        per = (args.cells + world - 1) // world
        padded = torch.zeros(per, dtype=torch.int64)
        padded[: counts.shape[0]] = counts
        gathered = [torch.zeros(per, dtype=torch.int64) for _ in range(world)]
        dbg("all_gather counts")
        dist.all_gather(gathered, padded)
        dbg("all_gather done")
        allc = torch.cat(gathered)[: args.cells].numpy()
        gip = np.zeros(args.cells + 1, dtype=np.uint64)
        np.cumsum(allc, out=gip[1:])
        bounds = sa.plan_shards(gip, world)
        nlo, nhi = int(bounds[rank]), int(bounds[rank + 1])
        moved = torch.tensor([int((nlo, nhi) != (lo, hi))])
        dist.all_reduce(moved, op=dist.ReduceOp.MAX)  # every rank takes the same branch (generate() has barriers in test mode)
        if int(moved.item()):
            del indptr, indices, values
            torch.cuda.empty_cache()
            lo, hi = nlo, nhi
            dbg("datagen for the balanced partition")
            indptr, indices, values = generate(lo, hi)
    torch.cuda.synchronize()
    t_gen = time.time() - t0
    nnz_local = int(indptr[-1].item())
    n_local = hi - lo

    # One allocation ahead of the handle (scanrs_reserve_device_memory): a caller knows the size of its matrix before the first PCA.
    # On a box whose memory another process has just freed, the driver is still scrubbing it and an allocation waits for that
    # (profiles/microbench/alloc_probe2: 0.24 s per 8 GB) — environment, not the path measured here; config.reserve_s reports it.
    t_r = time.perf_counter()
    reserve_bytes = 0
    if not args.no_reserve:
        if args.reserve_bytes_per_nnz is not None:
            reserve_bytes = int(args.reserve_bytes_per_nnz * nnz_local)
        else:
            b_cols = 2 * args.k  # BkSvd: k_multiplier 2, n_iter 5
            reserve_bytes = int(27.5 * nnz_local) + n_local * (2 * 8 * b_cols * 5 + 6 * 8 * b_cols)
        sa.reserve_device_memory(reserve_bytes + (1 << 30))
    t_reserve = time.perf_counter() - t_r
    # genes x cells (Cell Ranger orientation), stored cell-major = CSC
    dbg(f"shard [{lo}, {hi}) nnz {nnz_local}: create handle")
    torch.cuda.synchronize()
    t0 = time.time()
    t_first = {"t0": time.perf_counter()}
    mat = sa.AdaptiveMat.from_device(args.genes, n_local, sa.CSC, indptr.data_ptr(), indices.data_ptr(), values.data_ptr())
    mat.sync()
    t_first["create_handle"] = time.perf_counter()
    # the generator's arrays go back to torch's allocator, NOT to the driver: VRAM that was just freed is scrubbed in the background and
    # an allocation that lands on it waits for the scrubber (profiles/microbench/alloc_probe2) — a caller that uploads from host memory
    # (Cell Ranger) frees nothing on the device before its first PCA either. torch's cache is emptied after the first call.
    del indptr, indices, values

    comm = None
    transport = "none (1 GPU)"
    if world > 1 or args.force_collective:
        # Transport of the exchange steps, decided IDENTICALLY on every rank (a rank that went another way would leave the others
        # inside their first collective for ever):
        #  1. pre-flight, no collective involved: can this rank load RCCL through the library at all (it maps torch's librccl with
        #     RTLD_NOLOAD, comm.cpp)? SCANRS_BENCH_FAIL_COMM_RANK=r injects a failure on rank r (tests); ranks that share one GPU
        #     (SCANRS_BENCH_SHARED_GPU=1, tests only) count as failed: RCCL refuses two ranks on one device. The flags are gathered;
        #  2. only if every rank passed: rank 0's id is broadcast and every rank calls ncclCommInitRank together; the outcomes are
        #     gathered again;
        #  3. otherwise (or if step 2 failed anywhere): the same schedule with the exchange steps served through the library's all-reduce
        #     hook by the host program's own group — RCCL (backend "nccl") on device buffers, or gloo through host memory when the
        #     ranks share a GPU.
        comm_err = ""
        my_uid = None
        try:
            if os.environ.get("SCANRS_BENCH_FAIL_COMM_RANK", "") == str(rank):
                raise sa.ScanrsError(4, f"injected pre-flight failure on rank {rank} (SCANRS_BENCH_FAIL_COMM_RANK)")
            my_uid = sa.Comm.unique_id()  # loads RCCL; only rank 0's id is used
        except sa.ScanrsError as e:
            comm_err = str(e)
        ok = my_uid is not None
        errs = [comm_err]
        if dist is not None:
            flags = [None] * world
            dist.all_gather_object(flags, (ok, comm_err))
            ok = all(f[0] for f in flags)
            errs = [f"rank {r}: {f[1]}" for r, f in enumerate(flags) if not f[0]]
        if ok and shared_gpu and world > 1:
            ok, errs = False, ["ranks share one GPU (test mode): RCCL cannot place two ranks on one device"]
        if ok:
            uid = [my_uid if rank == 0 else None]
            if dist is not None:
                dist.broadcast_object_list(uid, src=0)
            try:
                comm = sa.Comm(uid[0], rank, world)
            except sa.ScanrsError as e:
                comm_err = str(e)
            ok = comm is not None
            if dist is not None:
                flags = [None] * world
                dist.all_gather_object(flags, (ok, comm_err))
                ok = all(f[0] for f in flags)
                errs = [f"rank {r}: {f[1]}" for r, f in enumerate(flags) if not f[0]]
        if ok:
            mat.set_shard_comm(comm, lo, args.cells)
            transport = "RCCL all-reduce enqueued by the library on its own stream (scanrs_comm_*)"
        elif dist is None:
            raise SystemExit(f"bench.py: library RCCL communicator failed: {comm_err}")
        else:
            from scanrs_amd.dist import make_allreduce

            if comm is not None:
                comm.close()
                comm = None
            why = "; ".join(errs)[:300]
            if shared_gpu:
                mat.set_shard(rank, world, lo, args.cells, make_allreduce(dist, dev, stage_through_host=True))
                transport = f"host hook over gloo (library communicator not used: {why})"
            else:
                nccl_group = dist.new_group(backend="nccl")
                mat.set_shard(rank, world, lo, args.cells, make_allreduce(dist, dev, group=nccl_group))
                transport = f"torch.distributed RCCL group through the library's all-reduce hook (library communicator not used: {why})"

    dbg(f"transport: {transport}")
    if args.f32_panels:
        mat.set_panel_precision(1)
    if args.spmm_path:
        mat.set_spmm_path(args.spmm_path)
    for kv in args.opt:
        key, val = kv.split("=")
        mat.set_option(key, float(val))
    bk = sa.BkSvd()  # k_multiplier 2.0, n_iter 5: the solver scan-rs-cmd uses (tools/src/bin/cmd.rs:70)

    # U and V land in caller-allocated row-major buffers, as the boundary specifies ("outputs written into
    # caller-allocated row-major f64 buffers"; include/scanrs_amd.h scanrs_pca_bk) — the same two arrays in every step, like a caller
    # that keeps its result buffers; config.fresh_result_arrays_ms_per_step is the step with new arrays per call (page faults of
    # 413 MB of untouched pages + their munmap, the Python wrapper's default)
    out_u, out_v = np.zeros((args.genes, args.k)), np.zeros((n_local, args.k))
    out_u.fill(0.0)  # touched once here (np.zeros hands out untouched pages): the caller's buffers exist before the timed steps
    out_v.fill(0.0)

    def step(download=False, fresh=False):
        mat.reset_map()
        sa.normalize(mat, sa.Normalization.CellRanger)
        if download:
            return bk.run_pca(mat, args.k) if fresh else bk.run_pca(mat, args.k, out=(out_u, out_v))
        s, _res = bk.run_pca_device(mat, args.k)
        return None, s, None

    def barrier():
        torch.cuda.synchronize()
        mat.sync()
        if dist is not None:
            dist.barrier()

    # First call on the fresh handle, as Cell Ranger makes it (one PCA per matrix, tools/src/bin/cmd.rs:61-70): handle
    # creation (device-to-device copy of the triplet here, validation, work items), normalize, PCA with U and V delivered to host
    # arrays; the transposed (gene-major) copy and the tile layouts of the hybrid product are built inside it (the second
    # orientation by a helper thread beside the normalisation passes and the first product).
    dbg("first call")
    mat.reset_map()
    sa.normalize(mat, sa.Normalization.CellRanger)
    mat.sync()
    t_first["normalize"] = time.perf_counter()
    if args.no_host_delivery:
        bk.run_pca_device(mat, args.k)
    else:
        bk.run_pca(mat, args.k)  # fresh arrays: what a first call pays
    t_first["run_pca"] = time.perf_counter()
    barrier()
    t_setup = time.time() - t0
    # where the first call went: wall-clock segments of the caller + the library's own host-side accounting inside run_pca
    # (scanrs_mat_get_counter, microseconds of the calling thread); "solver" is what is left of run_pca: the 11 sparse passes and the
    # dense steps, i.e. a warm step minus its normalize and delivery
    cnt = {k_: mat.counter(k_) / 1e3 for k_ in ("t_layout_us", "t_side_wait_us", "t_start_panel_us", "t_delivery_us")}
    run_pca_ms = (t_first["run_pca"] - t_first["normalize"]) * 1e3
    first_breakdown = {
        "create_handle": round((t_first["create_handle"] - t_first["t0"]) * 1e3, 2),
        "normalize": round((t_first["normalize"] - t_first["create_handle"]) * 1e3, 2),
        "run_pca.tile_layouts_built_by_the_calling_thread": round(cnt["t_layout_us"], 2),
        "run_pca.waits_for_the_helper_thread(first tile layout, transposed copy, second tile layout)": round(cnt["t_side_wait_us"], 2),
        "run_pca.start_panel": round(cnt["t_start_panel_us"], 2),
        "run_pca.delivery_of_U_and_V_to_host_arrays": round(cnt["t_delivery_us"], 2),
        "run_pca.solver(11 sparse passes + dense steps + weights of both layouts)": round(run_pca_ms - sum(cnt.values()), 2),
        "barrier_after": round((time.time() - t0) * 1e3 - (t_first["run_pca"] - t_first["t0"]) * 1e3, 2),
    }
    torch.cuda.empty_cache()
    sa.release_cached_memory()  # blocks the library keeps for reuse (the transposition's temporaries) are not resident data
    mem_after_first = sa.device_memory_in_use()  # everything the handle keeps: both copies, layouts, scratch (the library's own count of its live buffers)
    for i in range(max(0, args.warmup - 1)):
        dbg(f"warmup {i + 1}")
        step(download=not args.no_host_delivery)
    barrier()
    # Timed region: exactly K steps between barriers, each returning host arrays like run_pca. The per-launch HIP events
    # that feed the roofline leg put a marker packet before and after every launch of a step, which costs a few percent of
    # wall time, so with --full they are recorded in a second pass of K steps right after the timed one (same inputs, same
    # launches, results left in HBM: that pass is also the device-resident rate); --events-in-timed-region records them
    # inside the timed steps instead.
    mat.profile_reset()
    mat.profile_enable(bool(args.events_in_timed_region))
    dbg("timed steps")
    barrier()
    t0 = time.perf_counter()
    sig = None
    for _ in range(args.steps):
        _, sig, _ = step(download=not args.no_host_delivery)
    barrier()
    elapsed = time.perf_counter() - t0
    elapsed_local = elapsed
    mat.profile_enable(False)
    if args.dump_outputs:
        # what the last timed step handed its caller: U (genes x k), sigma, V (cells x k). V's rows are sampled by their global
        # cell index and gathered on rank 0 in cell order, so the files do not depend on the number of ranks.
        dbg("dump outputs")
        if args.no_host_delivery:
            res = sa.pca_result_device(mat)
            u_all = torch.as_tensor(sa.DevArray(res.d_u, args.genes * res.ld_u), device=dev).view(args.genes, res.ld_u)[:, : res.k]
            v_loc = torch.as_tensor(sa.DevArray(res.d_v, n_local * res.ld_v), device=dev).view(n_local, res.ld_v)[:, : res.k]
        else:
            u_all, v_loc = torch.from_numpy(out_u), torch.from_numpy(out_v)
        u_rows = dump_rows(args.genes, 8 * args.k, DUMP_BYTES // 2)
        u_bytes = 8 * args.k * (args.genes if u_rows is None else len(u_rows))
        v_rows = dump_rows(args.cells, 8 * args.k, DUMP_BYTES - u_bytes - 8 * args.k)
        if v_rows is not None:
            v_loc = v_loc[torch.as_tensor(v_rows[(v_rows >= lo) & (v_rows < hi)] - lo, device=v_loc.device)]
        v_dump = [v_loc.cpu().numpy()]
        if dist is not None:
            parts = [None] * world if rank == 0 else None
            dist.gather_object(v_dump[0], parts, dst=0)
            v_dump = parts
        if rank == 0:
            os.makedirs(args.dump_outputs, exist_ok=True)
            u_dump = u_all if u_rows is None else u_all[torch.as_tensor(u_rows, device=u_all.device)]
            for name, a in (("u", u_dump.cpu().numpy()), ("s", sig), ("v", np.concatenate(v_dump))):
                np.save(os.path.join(args.dump_outputs, f"{name}.npy"), np.ascontiguousarray(a, dtype=np.float64))
    events_elapsed = None
    if args.full:
        dbg("device-resident steps")
        mat.profile_enable(not args.events_in_timed_region)
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        barrier()
        events_elapsed = time.perf_counter() - t0
        mat.profile_enable(False)
    fresh_ms = None
    if args.full and not args.no_host_delivery:  # the same step handing out NEW host arrays every time (the Python wrapper's default form)
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(download=True, fresh=True)
        barrier()
        fresh_ms = (time.perf_counter() - t0) / args.steps * 1e3
    dbg("reductions over ranks")
    rank_ms = [elapsed_local / args.steps * 1e3]
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        if events_elapsed is not None:
            t = torch.tensor([events_elapsed], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            events_elapsed = float(t.item())
        nn = torch.tensor([nnz_local], dtype=torch.int64)
        gl = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
        dist.all_gather(gl, nn)
        nnz_ranks = [int(x.item()) for x in gl]
        tl = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(tl, torch.tensor([rank_ms[0]], dtype=torch.float64))
        rank_ms = [float(x.item()) for x in tl]
    else:
        nnz_ranks = [nnz_local]
    nnz_global = sum(nnz_ranks)
    prof = mat.profile_get()
    # per rank: the time of the kernels that work the rank's own cells (events pass), to be read against per_rank_nnz
    my_sharded_kernel_ms = sum(v_["total_ms"] for k_, v_ in prof.items() if k_.startswith(SHARDED_KERNEL_PREFIXES) and "gather2d_ov" not in k_) / args.steps
    rank_sharded_kernel_ms = [my_sharded_kernel_ms]
    if dist is not None:
        tl2 = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(tl2, torch.tensor([my_sharded_kernel_ms], dtype=torch.float64))
        rank_sharded_kernel_ms = [float(x.item()) for x in tl2]
    # what the transport itself saw (VERDICT r5 item 5 i): ranks as RCCL counts them (ncclCommCount on the library's communicator; the
    # host program's own group when the all-reduce hook serves), this rank's all-reduce calls / payload and their time per step (HIP
    # events around every ncclAllReduce on the handle's stream, events pass)
    my_ar_ms = sum(v_["total_ms"] for k_, v_ in prof.items() if k_.startswith("allreduce")) / args.steps
    my_ar_calls = sum(v_["launches"] for k_, v_ in prof.items() if k_.startswith("allreduce")) / args.steps
    my_ar_bytes = sum(v_["algorithmic_bytes"] for k_, v_ in prof.items() if k_.startswith("allreduce")) / args.steps
    if comm is not None:
        ci = comm.info()
        rccl_seen = {"source": "ncclCommCount / ncclCommUserRank on the library's communicator", "nranks": ci["rccl_nranks"], "rank": ci["rccl_rank"]}
    elif dist is not None and world > 1:
        rccl_seen = {"source": "the host program's torch.distributed group behind the all-reduce hook", "nranks": dist.get_world_size(), "rank": dist.get_rank()}
    else:
        rccl_seen = {"source": "single rank: no collective", "nranks": 1, "rank": 0}
    rank_ar = [(my_ar_ms, my_ar_calls, my_ar_bytes, float(rccl_seen["nranks"]))]
    if dist is not None:
        tl3 = [torch.zeros(4, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(tl3, torch.tensor(list(rank_ar[0]), dtype=torch.float64))
        rank_ar = [tuple(float(y) for y in x) for x in tl3]
    ms_per_step = elapsed / args.steps * 1e3
    value = args.cells * args.steps / elapsed

    # the factors of the timed steps are reachable: PcaResult in HBM (Missing #4 of the round-1 verdict)
    res = sa.pca_result_device(mat)
    v_col_norm_err = None
    if args.full:
        v_t = torch.as_tensor(sa.DevArray(res.d_v, n_local * res.ld_v), device=dev).view(n_local, res.ld_v)[:, : res.k]
        vnorm = (v_t * v_t).sum(dim=0).cpu()
        if dist is not None:
            dist.all_reduce(vnorm)
        v_col_norm_err = float((vnorm - 1.0).abs().max().item())

    knn_ms = None
    if args.also_knn and world == 1:
        barrier()
        t0 = time.perf_counter()
        sa.knn_device(res.d_v, n_local, res.ld_v, res.k, args.also_knn)
        knn_ms = (time.perf_counter() - t0) * 1e3

    randsvd_ms = None
    randsvd_kernels = irlba_kernels = None
    if args.full and not args.no_randsvd and world == 1:
        import ctypes

        s_out = np.zeros(args.k)
        mat.reset_map()
        sa.normalize(mat, sa.Normalization.CellRanger)
        run_rand = lambda: sa._check(sa._lib.scanrs_pca_rand(mat._h, ctypes.c_uint32(args.k), ctypes.c_double(10.0), ctypes.c_uint32(2), ctypes.c_uint64(0),
                                                             None, None, s_out.ctypes.data_as(ctypes.c_void_p), None))
        barrier()
        t0 = time.perf_counter()
        run_rand()
        barrier()
        randsvd_ms = (time.perf_counter() - t0) * 1e3
        mat.profile_reset()  # which kernels it ran: a second call with the per-launch events on (not the timed one)
        mat.profile_enable(True)
        run_rand()
        barrier()
        randsvd_kernels = {k_: round(v_["total_ms"], 2) for k_, v_ in sorted(mat.profile_get().items()) if v_["total_ms"] >= 0.5}
        mat.profile_enable(False)

    irlba_ms = irlba_mprod = None
    if args.full and not args.no_irlba and world == 1:
        import ctypes

        s_out = np.zeros(args.k)
        mat.reset_map()
        sa.log_normalize_with_size_factor(mat, None, sa.FN_LOG2_1P)
        mp = ctypes.c_uint32()
        u_out, v_out = np.zeros((args.genes, args.k)), np.zeros((n_local, args.k))  # irlba returns host arrays (irlba.rs:71-76)
        run_irlba = lambda: sa._check(sa._lib.scanrs_pca_irlba(mat._h, ctypes.c_uint32(args.k), ctypes.c_double(1e-4), ctypes.c_uint32(50), None, None,
                                                               u_out.ctypes.data_as(ctypes.c_void_p), s_out.ctypes.data_as(ctypes.c_void_p),
                                                               v_out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(mp)))
        barrier()
        t0 = time.perf_counter()
        run_irlba()
        barrier()
        irlba_ms, irlba_mprod = (time.perf_counter() - t0) * 1e3, int(mp.value)
        mat.profile_reset()
        mat.profile_enable(True)
        run_irlba()
        barrier()
        irlba_kernels = {k_: round(v_["total_ms"], 2) for k_, v_ in sorted(mat.profile_get().items()) if v_["total_ms"] >= 0.5}
        mat.profile_enable(False)

    # ---- replicated / sharded split of the step, visible from one GPU ----------------------------------------------------------------
    # The same step on a second matrix with HALF the cells (same model, same genes): t(1/2) against t(1) gives the term that shrinks
    # with the cell range and the one that does not - the floor of the step on 8 GPUs is replicated + sharded / 8 + the exchanges.
    split = None
    if args.full and world == 1 and not args.no_split_probe and args.cells >= 4096:
        dbg("split probe")
        hc = args.cells // 2
        pip_, pix_, pvv_ = synth_counts_torch(hc, args.genes, args.density, args.seed, dev)
        pmat = sa.AdaptiveMat.from_device(args.genes, hc, sa.CSC, pip_.data_ptr(), pix_.data_ptr(), pvv_.data_ptr())
        p_nnz = int(pip_[-1].item())
        del pip_, pix_, pvv_
        for kv in args.opt:
            key, val = kv.split("=")
            pmat.set_option(key, float(val))
        out_vp = np.zeros((hc, args.k))
        out_vp.fill(0.0)

        def pstep():
            pmat.reset_map()
            sa.normalize(pmat, sa.Normalization.CellRanger)
            return bk.run_pca(pmat, args.k, out=(out_u, out_vp)) if not args.no_host_delivery else bk.run_pca_device(pmat, args.k)

        pstep()
        pstep()
        torch.cuda.synchronize()
        pmat.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            pstep()
        torch.cuda.synchronize()
        pmat.sync()
        ms_half = (time.perf_counter() - t0) / args.steps * 1e3
        split = split_replicated_sharded(elapsed / args.steps * 1e3, ms_half, p_nnz / max(1, nnz_local))
        split["split_probe"] = {"cells": hc, "nnz": p_nnz, "ms_per_step": round(ms_half, 2),
                                "method": "t(f) = replicated + sharded f from the step at f = 1 and at f = nnz share of a second matrix with half the cells"}
        split["floor_8_gpus_ms_per_step"] = round(split["replicated_ms_per_step"] + split["sharded_ms_per_step"] / 8.0, 2)
        del pmat

    # ---- the same step on a heavy-tailed gene profile (NOT the headline) ----------------------------------------------------------
    # SURVEY.md §8d's synthetic has a nearly flat gene popularity; a real 10x matrix has a few thousand genes detected in most cells and
    # most genes in almost none (sqz/src/lib.rs:5-8). tools/pass_bench.py's model of that (Gamma(0.1) gene rates, one profile shared by
    # all clusters: ~2 900 genes above 10 % detection holding 3/4 of the nonzeros) at the same shape and density, same step.
    heavy = None
    if args.full and world == 1 and not args.no_heavy_tailed:
        dbg("heavy-tailed profile")
        hip_, hix_, hvv_ = synth_counts_torch(args.cells, args.genes, args.density, args.seed, dev, gene_shape=0.1, shared_profile=1.0)
        per_gene = torch.bincount(hix_.long(), minlength=args.genes).float() / args.cells
        hmat = sa.AdaptiveMat.from_device(args.genes, args.cells, sa.CSC, hip_.data_ptr(), hix_.data_ptr(), hvv_.data_ptr())
        h_nnz = int(hip_[-1].item())
        del hip_, hix_, hvv_

        def hstep():
            hmat.reset_map()
            sa.normalize(hmat, sa.Normalization.CellRanger)
            return bk.run_pca(hmat, args.k, out=(out_u, out_v)) if not args.no_host_delivery else bk.run_pca_device(hmat, args.k)

        hstep()
        hstep()
        torch.cuda.synchronize()
        hmat.sync()
        t0 = time.perf_counter()
        for _ in range(max(1, min(args.steps, 5))):
            hstep()
        hmat.sync()
        h_ms = (time.perf_counter() - t0) / max(1, min(args.steps, 5)) * 1e3
        heavy = {"ms_per_step": round(h_ms, 2), "cells_per_s": round(args.cells / (h_ms * 1e-3), 1), "nnz": h_nnz,
                 "genes_detected_in_over_10pct_of_cells": int((per_gene > 0.1).sum()),
                 "their_share_of_the_nonzeros": round(float(per_gene[per_gene > 0.1].sum() / per_gene.sum()), 3),
                 "model": "tools/pass_bench.py gene_shape=0.1 shared_profile=1 (Gamma(0.1) gene rates shared by all clusters), same cells x genes x density, same step"}
        del hmat
        torch.cuda.empty_cache()

    # ---- roofline of the dominant kernel -------------------------------------------------------------------
    roof = None
    if args.full and prof:
        # the dominant kernel of the critical path: the overflow gather of the hybrid product ("_ov") and the dense kernels the
        # solver queues on its second stream run BESIDE the sparse passes (their event durations are stretched by the sharing)
        side = ("spmm_gather2d_ov", "gemm_tiled", "gram_tiled", "gemm_skinny", "allreduce")
        kern = {k: v for k, v in prof.items() if not k.startswith(side)} or {k: v for k, v in prof.items() if not k.startswith("allreduce")}
        dom = max(kern.items(), key=lambda kv: kv[1]["total_ms"])
        name, st = dom
        achieved = st["algorithmic_bytes"] / (st["total_ms"] * 1e-3) / 1e9 if st["total_ms"] > 0 else 0.0
        traffic = traffic_src = None
        try:  # HBM bytes per launch from the committed PMC passes (profiles/, separate --pmc runs), headline workload only
            with open(os.path.join(ROOT, "profiles", PMC_PROFILE)) as f:
                pj = json.load(f)
            pm = pj["kernels"].get(name) or pj["kernels"].get(name.split("/")[0])  # the tile kernel is one class in the trace (both orientations)
            have, want = kernel_source_hash(), pj.get("kernel_source_sha256_16")
            if not (pm and args.cells == 1_000_000 and args.genes == 33_000 and world == 1):
                traffic_src = f"profiles/{PMC_PROFILE} holds the headline workload on 1 GPU only"
            elif want != have:
                traffic_src = (f"null on purpose: profiles/{PMC_PROFILE} was measured on kernel sources {want} (commit {pj.get('commit', '?')}), the sources "
                               f"loaded now hash to {have} - re-run tools/profile_round.sh")
            else:
                traffic = round(pm["hbm_bytes_per_launch_corrected"])
                traffic_src = (f"profiles/{PMC_PROFILE}: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command at commit {pj.get('commit', '?')}, same kernel "
                               f"sources ({have}); not measured inside this run")
        except (OSError, ValueError, KeyError) as e:
            traffic, traffic_src = None, f"profiles/{PMC_PROFILE} unreadable: {e}"
        alg_per_launch = st["algorithmic_bytes"] / max(1, st["launches"])
        lds_per_launch = st["onchip_gather_bytes"] / max(1, st["launches"])
        avg_s = st["total_ms"] / max(1, st["launches"]) * 1e-3
        # SURVEY.md section 8(d), to the letter: B_pass(l) = 8 Z + 8 (R + 1) + 2 G l 8 with R cells, G genes - the gene-side panel read
        # once and written once, the cell-side panel NOT counted (the survey's pass is the fused X^T (X B); this build runs its two
        # halves as two launches, each of which moves one gene-side and one cell-side panel: `algorithmic_bytes_per_launch_unfused`).
        # One launch of the dominant kernel works the share of the nonzeros the tile layout serves.
        l_pass = 2 * args.k
        z_loc, r_loc, g_all = float(nnz_local), float(n_local), float(args.genes)
        served = 1.0 - mat.counter("tile_overflow_nonzeros") / max(1, 2 * nnz_local) if name.startswith("spmm_tile_kernel") else 1.0
        b_pass = lambda l: 8.0 * z_loc + 8.0 * (r_loc + 1.0) + 16.0 * g_all * l
        alg_8d = b_pass(l_pass) * served if name.startswith("spmm_tile_kernel") else alg_per_launch
        # the whole PCA by the survey's schedule: 2 statistics passes + n_iter fused passes at l = b + 1 fused pass at l = 5 b + 1 projection pass
        pca_8d = ((8.0 * z_loc + 8.0 * (r_loc + 1.0) + 4.0 * r_loc) + (8.0 * z_loc + 8.0 * (r_loc + 1.0) + 8.0 * r_loc + 16.0 * g_all)
                  + 5.0 * b_pass(l_pass) + b_pass(5 * l_pass) + (8.0 * z_loc + 8.0 * g_all * args.k + 8.0 * r_loc * args.k))
        prof_ms = None  # the same kernel's average duration in the committed rocprofv3 kernel trace (same source-hash rule as `traffic`)
        try:
            with open(os.path.join(ROOT, "profiles", PMC_PROFILE.replace("traffic", "counters"))) as f:
                cj0 = json.load(f)
            if cj0.get("kernel_source_sha256_16") == kernel_source_hash():
                prof_ms = cj0.get("avg_launch_ms", {}).get(name.split("/")[0])
        except (OSError, ValueError, KeyError):
            prof_ms = None
        # LDS-array and vector-pipe occupancy of the same kernel from the committed counter passes (same source-hash rule as `traffic`):
        # SQ_LDS_IDX_ACTIVE = LDS-array cycles (4 per ds_read_b128, idle lanes included), SQ_INSTS_VALU x 4 clk per SIMD, against the
        # cycles the launch had at the shader clock the run held (SQ_BUSY_CYCLES / 32 shader engines / duration: the kernel is
        # power-limited well below the 2.4 GHz the peaks are quoted at) - measured in the profile run, with ITS launch duration
        occupancy = None
        try:
            if traffic is not None:
                with open(os.path.join(ROOT, "profiles", PMC_PROFILE.replace("traffic", "counters"))) as f:
                    cj = json.load(f)
                ck = cj["kernels"].get(name) or cj["kernels"].get(name.split("/")[0])
                if cj.get("kernel_source_sha256_16") == kernel_source_hash() and ck and cj.get("avg_launch_ms", {}).get(name.split("/")[0]):
                    t_prof = cj["avg_launch_ms"][name.split("/")[0]] * 1e-3
                    clk = ck["SQ_BUSY_CYCLES"]["avg_per_launch"] / 32.0 / t_prof
                    occupancy = {
                        "source": f"profiles/{PMC_PROFILE.replace('traffic', 'counters')} (separate --pmc passes, same kernel sources), launch {round(t_prof * 1e3, 2)} ms there",
                        "shader_clock_ghz_held": round(clk / 1e9, 2),
                        "lds_array_busy": round(ck["SQ_LDS_IDX_ACTIVE"]["avg_per_launch"] / (256 * clk * t_prof), 3),
                        "valu_busy": round(ck["SQ_INSTS_VALU"]["avg_per_launch"] * 4.0 / (1024 * clk * t_prof), 3),
                        "valu_instructions_per_lds_read": round(ck["SQ_INSTS_VALU"]["avg_per_launch"] / ck["SQ_INSTS_LDS"]["avg_per_launch"], 2),
                    }
        except (OSError, ValueError, KeyError, ZeroDivisionError):
            occupancy = None
        roof = {
            "bound": "hbm",
            "kernel": name,
            # achieved / frac follow SURVEY.md section 8(d)'s bytes; the unfused count this build's launches
            # really move (both panels of a half pass) stands beside them under its own name
            "achieved": round(alg_8d / avg_s / 1e9, 2) if avg_s > 0 else 0.0,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": round(alg_8d / avg_s / 1e9 / HBM_PEAK_GBS, 5) if avg_s > 0 else 0.0,
            "frac_8d": round(alg_8d / avg_s / 1e9 / HBM_PEAK_GBS, 5) if avg_s > 0 else 0.0,
            "traffic": traffic,
            "traffic_source": traffic_src,
            "launches_per_step": st["launches"] / args.steps,
            "avg_launch_ms": round(st["total_ms"] / max(1, st["launches"]), 4),
            "avg_launch_ms_is": "HIP events on the library's stream around every launch of the timed steps, in this run",
            "avg_launch_ms_rocprof": prof_ms,
            "avg_launch_ms_rocprof_is": f"the same kernel in profiles/{PMC_PROFILE.replace('traffic', 'counters')} (rocprofv3 --kernel-trace of this command, first-call launches included; null when the kernel sources differ)",
            "algorithmic_bytes_per_launch": round(alg_8d),
            "algorithmic_bytes_per_launch_is": "SURVEY 8(d): (8 Z + 8 (R + 1) + 16 G l) x the share of the nonzeros the tile layout serves; l = 2 k",
            "algorithmic_bytes_per_launch_unfused": round(alg_per_launch),
            "achieved_unfused": round(achieved, 2),
            "frac_unfused": round(achieved / HBM_PEAK_GBS, 5),
            "unfused_is": "8 Z + 8 (R + 1) + 8 G l + 8 R l: a half pass also reads or writes the cell-side panel, which the survey's fused pass keeps on chip",
            # the whole PCA by the survey's schedule (2 statistics + 5 fused + 1 wide + 1 projection pass) over the step's wall time
            "pca": {"bytes_8d": round(pca_8d), "achieved": round(pca_8d / (ms_per_step * 1e-3) / 1e9, 2), "unit": "GB/s",
                    "frac": round(pca_8d / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS / world, 5)},
            # HBM bytes the counters saw per algorithmic byte (re-reads, staging through L2 misses): the first thing to fix when >> 1
            "wasted_traffic_ratio": round(traffic / alg_8d, 2) if traffic and alg_8d else None,
            # the ceiling that actually binds this kernel: panel rows read from LDS (one 16-byte read per lane and record position)
            # against the LDS bandwidth of the chip; HBM is far from it by construction (800 B of panel row per 8 B of matrix)
            "onchip": {
                "unit": "TB/s of LDS row reads",
                "bytes_per_launch": round(lds_per_launch),
                "achieved": round(lds_per_launch / avg_s / 1e12, 2) if avg_s > 0 and lds_per_launch else None,
                "peak": LDS_PEAK_TBS,
                "frac": round(lds_per_launch / avg_s / 1e12 / LDS_PEAK_TBS, 4) if avg_s > 0 and lds_per_launch else None,
                "frac_of_survey_estimate_78.6": round(lds_per_launch / avg_s / 1e12 / LDS_SURVEY_TBS, 4) if avg_s > 0 and lds_per_launch else None,
                "occupancy_from_counters": occupancy,
                # bytes_per_launch counts the rows of SERVED nonzeros only (round 5; before: every record position, padding included)
                "positions_per_served_nonzero": round(mat.counter("tile_positions") / max(1, mat.counter("tile_served_nonzeros")), 4),
                "overflow_share_of_nonzeros": round(mat.counter("tile_overflow_nonzeros") / max(1, 2 * nnz_local), 5),
            },
            "kernel_ms_per_step": {k: round(v["total_ms"] / args.steps, 3) for k, v in sorted(prof.items())},
            "launches_per_step_all": {k: round(v["launches"] / args.steps, 1) for k, v in sorted(prof.items())},
            "events_pass_ms_per_step": round(events_elapsed / args.steps * 1e3, 2),
            "beside_the_critical_path": [k for k in sorted(prof) if k.startswith(side)],
        }

    # ---- CPU baseline: the oracle (the reference's serial schedule) on bounded samples: 1 core, then all cores -------
    cpu = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import scanrs_oracle as so
        import scipy.linalg  # noqa: F401  (the LAPACK of the oracle's dense steps: loaded now so that threadpool_info sees its pool)
        from threadpoolctl import threadpool_info, threadpool_limits

        so.build()
        # the cores this process may use: its CPU affinity, and no more than OMP_NUM_THREADS where the host sets it
        nproc = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        if os.environ.get("OMP_NUM_THREADS", "").isdigit():
            nproc = max(1, min(nproc, int(os.environ["OMP_NUM_THREADS"])))
        # OpenBLAS cannot grow its thread pool past the size it started with (asked for more, it crashes in the next LAPACK call)
        blas_pool = min([p["num_threads"] for p in threadpool_info() if p["user_api"] == "blas"] or [nproc])

        def cpu_run(nc, threads, lapack_threads):
            ip, ix, vv = synth_counts_torch(args.cells, args.genes, args.density, args.seed, dev, 0, nc)
            ip, ix, vv = ip.cpu().numpy().astype(np.uint64), ix.cpu().numpy().astype(np.uint32), vv.cpu().numpy().astype(np.uint32)
            so.set_threads(threads)
            try:
                om = so.AdaptiveMat(args.genes, nc, so.CSC, ip, ix, vv)
                if threads > 1:
                    om.other_copy()  # the gene-major copy the threaded products gather from: layout preparation, as on the device
                with threadpool_limits(limits=lapack_threads):
                    t0 = time.perf_counter()
                    a = so.normalize(om, "cellranger")
                    so.BkSvd().run_pca(a, min(args.k, nc))
                    return time.perf_counter() - t0
            finally:
                so.set_threads(1)

        nc1 = min(args.cpu_cells, args.cells)
        t1 = cpu_run(nc1, 1, 1)
        cpu = {
            "value": round(nc1 / t1, 2),
            "unit": "cells/s",
            "cores": 1,
            "kind": "port",
            "host_cores_available": nproc,
            "sample": f"first {nc1} cells of the same synthetic matrix ({args.genes} genes, {args.density:.0%} nnz), "
                      f"normalize(CellRanger) + BkSvd k={min(args.k, nc1)}, oracle C loops + LAPACK pinned to 1 thread "
                      f"(the reference is single-threaded with sequential MKL), {t1:.1f} s",
        }
        if nproc > 1:
            nca = min(args.cpu_cells_all, args.cells)
            nth = nproc if nproc <= 64 else nproc // 2  # one thread per physical core on an SMT-2 host
            nla = min(32, nth, blas_pool)
            ta = cpu_run(nca, nth, nla)
            cpu["all_cores"] = {
                "value": round(nca / ta, 2), "unit": "cells/s", "cores": nth, "kind": "port",
                "sample": f"first {nca} cells, same schedule with the outer vectors of every sparse loop dealt over {nth} OpenMP threads "
                          f"(the scatter-form products gather from a gene-major copy built beforehand, as the device path does) and "
                          f"LAPACK on {nla} threads, {ta:.1f} s",
            }

    if rank == 0:
        ar_ms = sum(v["total_ms"] for k, v in prof.items() if k.startswith("allreduce")) / args.steps if prof else None  # per-launch events: --full
        out = {
            "metric": f"cells/sec for top-{args.k} PCA on {args.cells}x{args.genes} @{args.density:.0%} nnz; achieved HBM GB/s vs roofline",
            "value": round(value, 1),
            "unit": "cells/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 2),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64" if not args.f32_panels else "f64 sums over f32-rounded gather panels (opt-in fast mode)",
            "data": "synthetic",
            "config": {
                "workload": f"{args.cells} cells x {args.genes} genes, {args.density:.0%} nnz synthetic sqz CSC, "
                            f"normalize(CellRanger) + BkSvd(k_multiplier=2, n_iter=5) top-{args.k} PCA",
                "nnz": nnz_global,
                "parallelism": f"cells range-partitioned by nonzeros over {world} GPU(s)" + (", one sum all-reduce per contracting product" if world > 1 else ""),
                "transport": transport,
                "result_delivery": ("value: every step delivers U, sigma, V into caller-allocated host arrays (the C ABI's form, reused across steps); "
                                    "fresh_result_arrays_ms_per_step: new host arrays per step; device_resident_*: the same steps with U, V "
                                    "left in HBM (scanrs_pca_result_device)") if not args.no_host_delivery else "--no-host-delivery: U, V left in HBM in every step",
                "fresh_result_arrays_ms_per_step": round(fresh_ms, 2) if fresh_ms is not None else None,
                "device_resident_cells_per_s": round(args.cells * args.steps / events_elapsed, 1) if events_elapsed else None,
                "device_resident_ms_per_step": round(events_elapsed / args.steps * 1e3, 2) if events_elapsed else None,
                "v_col_norm_err_device_result": v_col_norm_err,
                "first_call_s": round(t_setup, 3),
                "first_call_cells_per_s": round(args.cells / t_setup, 1),
                "first_call_includes": "handle creation from device-resident arrays (copy, validation, work items), normalize, PCA with host delivery; inside: the transposed (gene-major) copy and the tile layouts of the hybrid product (both orientations). Not included: scanrs_init (library_init_s)",
                "first_call_breakdown_ms": first_breakdown,
                # what a fresh process pays before its first PCA result: scanrs_init + the reserve (waits for the VRAM scrubber when another
                # tenant has just exited: 0 or about 2 s, environment) + the first call
                "first_call_from_process_start_s": round(t_init + t_reserve + t_setup, 3),
                "heavy_tailed_ms_per_step": heavy["ms_per_step"] if heavy else None,
                "heavy_tailed_profile": heavy,
                "library_init_s": round(t_init, 3),
                "reserve_s": round(t_reserve, 3),
                "reserve_bytes_per_nonzero": round((reserve_bytes + (1 << 30)) / max(1, nnz_local), 1) if reserve_bytes else 0.0,
                "resident_bytes_per_nonzero": round(mem_after_first / max(1, nnz_local), 1) if mem_after_first else None,
                "datagen_s": round(t_gen, 2),
                "sigma_top3": [round(float(x), 6) for x in (sig[:3] if sig is not None else [])],
                "per_rank_ms_per_step": [round(x, 2) for x in rank_ms],
                "per_rank_nnz": nnz_ranks,
                "per_rank_sharded_kernel_ms_per_step": [round(x, 2) for x in rank_sharded_kernel_ms] if prof else None,
                "allreduce_ms_per_step_rank0": round(ar_ms, 3) if prof else None,
                "rccl": {"source": rccl_seen["source"], "nranks_seen_per_rank": [int(x[3]) for x in rank_ar],
                         "allreduce_ms_per_step_per_rank": [round(x[0], 3) for x in rank_ar] if prof else None,
                         "allreduce_calls_per_step_per_rank": [round(x[1], 1) for x in rank_ar] if prof else None,
                         "allreduce_bytes_per_step_per_rank": [int(x[2]) for x in rank_ar] if prof else None},
            },
            "roofline": roof,
            "cpu_baseline": cpu,
        }
        if knn_ms is not None:
            out["config"][f"knn{args.also_knn}_device_scores_ms"] = round(knn_ms, 1)
        if randsvd_ms is not None:  # "with RandSvd reported alongside" (rand_svd.rs:54-129: l = 10 k = 500 columns, 2 power iterations)
            out["config"]["randsvd_ms"] = out["config"]["randsvd_l10_it2_ms"] = round(randsvd_ms, 1)
            out["config"]["randsvd_kernels_ms"] = randsvd_kernels
        if irlba_ms is not None:  # irlba.rs:71-215 on the un-centred log-normalized matrix (tol 1e-4, at most 50 restarts)
            out["config"]["irlba_ms"] = out["config"]["irlba_tol1e-4_ms"] = round(irlba_ms, 1)
            out["config"]["irlba_matrix_products"] = irlba_mprod
            out["config"]["irlba_kernels_ms"] = irlba_kernels
        if split is not None:
            out["config"].update(split)
        print(json.dumps(out))
    wd.done = True
    del mat
    if comm is not None:
        comm.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
