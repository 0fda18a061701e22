"""The two ways a matrix leaves the device, timed in one process on the same handle: (a) scanrs_mat_to_csmat, the triplet (8 bytes a
nonzero over the host link, and the caller still has to run AdaptiveVec::new over every vector), and (b) scanrs_mat_to_adaptive, the
encoders of encode.hip plus the download of the two arenas. The matrix is bench.py's device-generated 1 M cells x 33 k genes at 3 %
(synth_counts_torch, seed 0), genes x cells held cell-major (CSC: one vector per cell); the same again on the filtered matrix of a
partition_on_threshold. Per handle one JSON line: bytes over the link, kernel ms of (b) from the scanrs_profile_* classes
"encode_plan" and "encode_emit", wall ms of both routes (median of --reps calls after one warm-up, each call returns synchronised)
and the kind histogram.

    python tools/adaptive_export_bench.py [--cells 1000000] [--genes 33000] [--density 0.03] [--threshold 2500] [--reps 3]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import scanrs_amd as sa  # noqa: E402
from scanrs_amd.synth import synth_counts_torch  # noqa: E402


def copied_bytes(e, n_outer):
    """What scanrs_mat_to_adaptive brought over the link for this export: the two arenas (in the byte arena every piece is padded to
    8 bytes) and, per vector, 24 bytes of the plan's table and its two 8-byte offsets (+ the two totals)."""
    table = ctypes.POINTER(sa.AdaptiveVecDesc)()
    sa._check(sa._lib.scanrs_adaptive_export_vecs(e, ctypes.byref(table)))
    if not n_outer:
        return 16
    words = ctypes.sizeof(sa.AdaptiveVecDesc) // 8
    t = np.ctypeslib.as_array(ctypes.cast(table, ctypes.POINTER(ctypes.c_uint64)), shape=(n_outer, words))
    off = {name: getattr(sa.AdaptiveVecDesc, name).offset // 8 for name, _ in sa.AdaptiveVecDesc._fields_}
    kind = t[:, off["kind"]] & 0xFFFFFFFF
    pad8 = lambda x: (x + 7) & ~np.uint64(7)  # noqa: E731
    arena_bytes = np.where(kind != 4, pad8(t[:, off["data_bytes"]]), 0).sum() + np.where(kind >= 5, pad8(t[:, off["n_units"]]), 0).sum()
    arena_words = (2 * t[:, off["n_fallback"]] + t[:, off["n_block_starts"]]).sum()
    return int(arena_bytes) + 4 * int(arena_words) + 40 * n_outer + 16


def measure(name, h, reps):
    n_outer = h.cols() if h.storage() == sa.CSC else h.rows()
    nnz = h.nnz()

    def route_a():
        t0 = time.perf_counter()
        out = h.to_csmat()
        ms = (time.perf_counter() - t0) * 1e3
        del out
        return ms

    def route_b():
        h.profile_reset()
        t0 = time.perf_counter()
        e = h._export(None)
        ms = (time.perf_counter() - t0) * 1e3
        total, counts = ctypes.c_uint64(), (ctypes.c_uint64 * 8)()
        sa._check(sa._lib.scanrs_adaptive_export_info(e, None, ctypes.byref(total), counts))
        link = copied_bytes(e, n_outer)
        sa._lib.scanrs_adaptive_export_free(e)
        prof = h.profile_get()
        kernel_ms = {k: prof[k]["total_ms"] for k in ("encode_plan", "encode_emit")}
        return ms, kernel_ms, int(total.value), [int(c) for c in counts], link

    h.profile_enable(True)
    route_a(), route_b()  # warm-up: code objects, the pinned staging ring
    a_ms = float(np.median([route_a() for _ in range(reps)]))
    runs = [route_b() for _ in range(reps)]
    b_ms = float(np.median([r[0] for r in runs]))
    k_plan = float(np.median([r[1]["encode_plan"] for r in runs]))
    k_emit = float(np.median([r[1]["encode_emit"] for r in runs]))
    total, counts, link = runs[0][2], runs[0][3], runs[0][4]
    h.profile_enable(False)
    triplet_bytes = 8 * nnz + 8 * (n_outer + 1)
    print(json.dumps({
        "matrix": name, "outer_vectors": n_outer, "inner_length": h.rows() if h.storage() == sa.CSC else h.cols(), "nnz": nnz, "reps": reps,
        "to_csmat": {"link_bytes": triplet_bytes, "wall_ms": round(a_ms, 2)},
        "to_adaptive": {"encoded_bytes": total, "link_bytes": link, "link_bytes_plan_table": 40 * n_outer + 16, "wall_ms": round(b_ms, 2),
                        "kernel_ms": round(k_plan + k_emit, 3), "kernel_ms_plan": round(k_plan, 3), "kernel_ms_emit": round(k_emit, 3),
                        "copy_and_host_ms": round(b_ms - k_plan - k_emit, 2),
                        "kinds": dict(zip(sa.ADAPTIVE_KINDS, counts))},
        "link_bytes_adaptive_over_csmat": round(link / max(triplet_bytes, 1), 4),
        "to_adaptive_faster": bool(b_ms < a_ms), "wall_ratio_adaptive_over_csmat": round(b_ms / max(a_ms, 1e-9), 3),
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--genes", type=int, default=33_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--threshold", type=float, default=2500.0)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch

    dev = torch.device("cuda", 0)
    sa.init()
    ip, ix, vv = synth_counts_torch(a.cells, a.genes, a.density, a.seed, dev)
    torch.cuda.synchronize()
    base = sa.AdaptiveMat.from_device(a.genes, a.cells, sa.CSC, ip.data_ptr(), ix.data_ptr(), vv.data_ptr())
    del ip, ix, vv
    torch.cuda.empty_cache()
    measure("synthetic", base, a.reps)
    f, _, _, _ = base.partition_on_thresholds(a.threshold, a.threshold, residual=False)
    measure(f"partition_on_threshold({a.threshold:g}).filtered", f, a.reps)


if __name__ == "__main__":
    main()
