"""The two ways a matrix leaves the device, timed in one process on the same handle: (a) scanrs_mat_to_csmat, the triplet (8 bytes a
nonzero over the host link, and the caller still has to run AdaptiveVec::new over every vector), and (b) scanrs_mat_to_adaptive, the
encoders of encode.hip plus the download of the two arenas. The matrix is bench.py's device-generated 1 M cells x 33 k genes at 3 %
(synth_counts_torch, seed 0), genes x cells held cell-major (CSC: one vector per cell); the same again on the filtered matrix of a
partition_on_threshold. Per handle one JSON line: bytes over the link, kernel ms of (b) from the scanrs_profile_* classes
"encode_plan" and "encode_emit", wall ms of both routes (median of --reps calls after one warm-up, each call returns synchronised)
and the kind histogram.

    python tools/adaptive_export_bench.py [--cells 1000000] [--genes 33000] [--density 0.03] [--threshold 2500] [--reps 3]

With --shards N [--major inner|stored] the same matrix is held as a MultiMat over N shards (all on device 0) and ONE JSON line reports
scanrs_multi_to_adaptive: wall ms (median of --reps calls after the first, which for `inner` also builds the shards'
transposed copies and is reported on its own), the phase counters export_{plan,pull,encode}_us of the slowest shard, encoded bytes,
arena_bytes and moved, the byte comparison against the unsharded export, and beside them the route a caller has without it:
MultiMat.to_csmat(), plus scipy's transposition for `inner`.

    python tools/adaptive_export_bench.py --shards 4 --major inner
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


# ---- the whole MultiMat (--shards N, --major inner|stored) ---------------------------------------------------------------
_OFF = {name: getattr(sa.AdaptiveVecDesc, name).offset // 8 for name, _ in sa.AdaptiveVecDesc._fields_}
_SIZES = ("len", "n_units", "data_bytes", "n_fallback", "n_block_starts")


def export_table(e):
    """The table of an export as u64 words (n_vecs x words of scanrs_adaptive_vec), borrowed from the export."""
    n, table = ctypes.c_uint64(), ctypes.POINTER(sa.AdaptiveVecDesc)()
    sa._check(sa._lib.scanrs_adaptive_export_info(e, ctypes.byref(n), None, None))
    sa._check(sa._lib.scanrs_adaptive_export_vecs(e, ctypes.byref(table)))
    words = ctypes.sizeof(sa.AdaptiveVecDesc) // 8
    if not n.value:
        return np.zeros((0, words), dtype=np.uint64)
    return np.ctypeslib.as_array(ctypes.cast(table, ctypes.POINTER(ctypes.c_uint64)), shape=(int(n.value), words))


def arena_views(t, bounds):
    """The two host arenas behind the table rows [bounds[d], bounds[d + 1]) of every part d, as numpy views: a part's pieces lie in
    vector order, every piece of the byte arena padded to 8 bytes (data, then index_bytes of S*; nothing for V), the word arena
    holding fallback indexes, fallback values and block_starts. The pointers of the table are checked against that layout."""
    pad8 = lambda x: (x + np.uint64(7)) & ~np.uint64(7)  # noqa: E731
    out = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        r = t[int(lo):int(hi)]
        if not r.shape[0]:
            out.append((np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint32)))
            continue
        kind = r[:, _OFF["kind"]] & np.uint64(0xFFFFFFFF)
        bsz = np.where(kind != 4, pad8(r[:, _OFF["data_bytes"]]), 0).astype(np.uint64) + np.where(kind >= 5, pad8(r[:, _OFF["n_units"]]), 0).astype(np.uint64)
        wsz = (2 * r[:, _OFF["n_fallback"]] + r[:, _OFF["n_block_starts"]]).astype(np.uint64)
        boff = np.concatenate([[0], np.cumsum(bsz)]).astype(np.uint64)
        woff = np.concatenate([[0], np.cumsum(wsz)]).astype(np.uint64)
        wbase = int(r[0, _OFF["fallback_indexes"]])
        assert np.array_equal(r[:, _OFF["fallback_indexes"]], np.uint64(wbase) + 4 * woff[:-1]), "the word arena is not laid out in vector order"
        words = np.ctypeslib.as_array(ctypes.cast(wbase, ctypes.POINTER(ctypes.c_uint32)), shape=(int(woff[-1]),)) if woff[-1] else np.zeros(0, dtype=np.uint32)
        has = np.nonzero(kind != 4)[0]
        if has.size and boff[-1]:
            bbase = int(r[has[0], _OFF["data"]]) - int(boff[has[0]])
            assert np.array_equal(r[has, _OFF["data"]], np.uint64(bbase) + boff[:-1][has]), "the byte arena is not laid out in vector order"
            bts = np.ctypeslib.as_array(ctypes.cast(bbase, ctypes.POINTER(ctypes.c_uint8)), shape=(int(boff[-1]),))
        else:
            bts = np.zeros(0, dtype=np.uint8)
        out.append((bts, words))
    return out


def exports_equal(e_multi, slab_bounds, e_single):
    """Byte comparison of two exports of the same matrix: every size field of the tables, then the arenas, the multi export's parts
    against the matching stretch of the single one's."""
    tm, ts = export_table(e_multi), export_table(e_single)
    if tm.shape != ts.shape:
        return False
    cols = [_OFF[k] for k in _SIZES]
    if not (np.array_equal(tm[:, cols], ts[:, cols]) and np.array_equal(tm[:, _OFF["kind"]] & np.uint64(0xFFFFFFFF), ts[:, _OFF["kind"]] & np.uint64(0xFFFFFFFF))):
        return False
    (sb, sw), = arena_views(ts, [0, ts.shape[0]])
    b_at = w_at = 0
    for pb, pw in arena_views(tm, slab_bounds):
        if not (np.array_equal(pb, sb[b_at:b_at + pb.shape[0]]) and np.array_equal(pw, sw[w_at:w_at + pw.shape[0]])):
            return False
        b_at, w_at = b_at + pb.shape[0], w_at + pw.shape[0]
    return b_at == sb.shape[0] and w_at == sw.shape[0]


def measure_multi(a, triplet):
    """MultiMat.to_adaptive_vecs' export (scanrs_multi_to_adaptive) over --shards shards of ONE device against (1) the unsharded
    export of the same matrix, byte for byte, and (2) the route a caller has without it: MultiMat.to_csmat(), plus scipy's
    transposition for `inner` (AdaptiveVec::new per vector on the host would still follow: it is not timed). One JSON line."""
    import scipy.sparse as sp

    n, major = a.shards, a.major
    hip, hix, hvv = triplet
    mm = sa.MultiMat(a.genes, a.cells, sa.CSC, hip, hix, hvv, n, devices=[0] * n)
    single = sa.AdaptiveMat.from_csmat(a.genes, a.cells, sa.CSC, hip, hix, hvv)

    def timed_export(x):
        t0 = time.perf_counter()
        e = x._export(None, major)
        return (time.perf_counter() - t0) * 1e3, e

    first_ms, e = timed_export(mm)  # (inner: settles the shards' transposed copies, which they keep)
    sa._lib.scanrs_adaptive_export_free(e)
    runs = []
    for _ in range(a.reps):
        ms, e = timed_export(mm)
        phases = {p: round(max(mm.counter(f"export_{p}_us", i) for i in range(n)) / 1e3, 3) for p in ("plan", "pull", "encode")}
        runs.append((ms, phases))
        sa._lib.scanrs_adaptive_export_free(e)
    multi_ms = float(np.median([r[0] for r in runs]))
    ms, e = timed_export(mm)
    info = sa._export_multi_info(e)
    total, counts = sa._export_totals(e)
    s_first_ms, es = timed_export(single)
    sa._lib.scanrs_adaptive_export_free(es)
    single_runs = []
    for _ in range(a.reps):
        s_ms, es = timed_export(single)
        sa._lib.scanrs_adaptive_export_free(es)
        single_runs.append(s_ms)
    single_ms = float(np.median(single_runs))
    _, es = timed_export(single)
    equal = exports_equal(e, info["slab_bounds"], es)
    n_vecs = int(export_table(e).shape[0])
    sa._lib.scanrs_adaptive_export_free(es)
    sa._lib.scanrs_adaptive_export_free(e)
    del single
    # the route a caller has today
    t0 = time.perf_counter()
    wip, wix, wvv = mm.to_csmat()
    csmat_ms = (time.perf_counter() - t0) * 1e3
    scipy_ms = 0.0
    if major == "inner":
        t1 = time.perf_counter()
        whole = sp.csc_matrix((wvv, wix.astype(np.int32), wip.astype(np.int64)), shape=(a.genes, a.cells))
        whole.has_sorted_indices = True
        by_gene = whole.tocsr()
        scipy_ms = (time.perf_counter() - t1) * 1e3
        del whole, by_gene
    nnz = int(wix.shape[0])
    moved = info["moved"]
    print(json.dumps({
        "matrix": "synthetic", "major": major, "shards": n, "all_shards_on_device": 0, "vectors": n_vecs, "len": a.cells if major == "inner" else a.genes,
        "nnz": nnz, "reps": a.reps,
        "multi_to_adaptive": {"wall_ms": round(multi_ms, 2), "first_call_wall_ms": round(first_ms, 2), "phase_ms": runs[-1][1], "encoded_bytes": total,
                              "arena_bytes": [int(x) for x in info["arena_bytes"]], "moved_total": int(moved.sum()),
                              "moved_between_shards": int(moved.sum() - np.trace(moved)), "kinds": dict(zip(sa.ADAPTIVE_KINDS, counts))},
        "unsharded_to_adaptive": {"wall_ms": round(single_ms, 2), "first_call_wall_ms": round(s_first_ms, 2)},
        "equals_unsharded_export": bool(equal),
        "host_route": {"to_csmat_ms": round(csmat_ms, 2), "scipy_transpose_ms": round(scipy_ms, 2), "wall_ms": round(csmat_ms + scipy_ms, 2),
                       "link_bytes": 8 * nnz + 8 * (a.cells + 1), "adaptive_vec_new_on_the_host": "not timed"},
        "link_bytes_multi_over_host_route": round(float(info["arena_bytes"].sum()) / max(8 * nnz, 1), 4),
        "multi_faster_than_host_route": bool(multi_ms < csmat_ms + scipy_ms),
        "wall_ratio_multi_over_host_route": round(multi_ms / max(csmat_ms + scipy_ms, 1e-9), 4),
    }), flush=True)
    mm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--genes", type=int, default=33_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--threshold", type=float, default=2500.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shards", type=int, default=0, help="N > 0: the export of a MultiMat over N shards (all on device 0) instead of one handle's")
    ap.add_argument("--major", choices=("inner", "stored"), default=None, help="with --shards: the orientation of the table (default stored)")
    a = ap.parse_args()
    if a.major is not None and a.shards <= 0:
        ap.error("--major needs --shards N")
    import torch

    dev = torch.device("cuda", 0)
    sa.init()
    ip, ix, vv = synth_counts_torch(a.cells, a.genes, a.density, a.seed, dev)
    torch.cuda.synchronize()
    base = sa.AdaptiveMat.from_device(a.genes, a.cells, sa.CSC, ip.data_ptr(), ix.data_ptr(), vv.data_ptr())
    del ip, ix, vv
    torch.cuda.empty_cache()
    if a.shards > 0:
        a.major = a.major or "stored"
        triplet = base.to_csmat()  # what a caller hands to MultiMat(...)
        del base
        measure_multi(a, triplet)
        return
    measure("synthetic", base, a.reps)
    f, _, _, _ = base.partition_on_thresholds(a.threshold, a.threshold, residual=False)
    measure(f"partition_on_threshold({a.threshold:g}).filtered", f, a.reps)


if __name__ == "__main__":
    main()
