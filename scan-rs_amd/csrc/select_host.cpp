// Host side of select_rows / select_cols / partition_on_thresholds (sqz/src/mat.rs:730-888, 1004-1071): the order of the passes,
// the per-round flag, and the small index tables. Kernels: select.hip. All of it works on the copy it is given (the handle's own
// storage) and queues on the handle's main stream.
#include "common.hpp"
#include "shard_exchange.hpp"

#include <algorithm>

namespace scanrs {

namespace {
template <typename T>
void upload(Storage &st, DevBuf<T> &d, const std::vector<T> &h) {
    d.alloc(std::max<size_t>(1, h.size()));
    if (!h.empty()) SCANRS_HIP(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st.stream));
}

// out.indptr holds the lengths of out.n_outer vectors: offsets, nnz, and room for the nonzeros
void offsets_and_room(Storage &st, SparseCopy &out) {
    select_scan_offsets(st.stream, reinterpret_cast<unsigned long long *>(out.indptr.p), out.n_outer);
    out.nnz = SCANRS_D2H_VALUE(out.indptr.p + out.n_outer, st.stream);
    out.indices.alloc(std::max<uint64_t>(1, out.nnz));
    out.values.alloc(std::max<uint64_t>(1, out.nnz));
}

void start_copy(Storage &st, const SparseCopy &cp, SparseCopy &out, uint64_t n_outer, uint64_t n_inner) {
    if (n_outer > 0xFFFFFFFFull || n_inner > 0xFFFFFFFFull) fail(SCANRS_ERR_SHAPE, "dimensions must fit in u32 (AdaptiveVec limit)");
    out.n_outer = n_outer;
    out.n_inner = n_inner;
    out.max_value = cp.max_value; // a bound is all the later passes ask for
    out.indptr.alloc(n_outer + 1);
    SCANRS_HIP(hipMemsetAsync(out.indptr.p, 0, (n_outer + 1) * 8, st.stream));
}

std::vector<uint32_t> checked_indices(const uint64_t *idx, uint64_t n_idx, uint64_t extent, const char *axis) {
    if (n_idx && !idx) fail(SCANRS_ERR_ARGUMENT, "null index list");
    std::vector<uint32_t> h(n_idx);
    for (uint64_t i = 0; i < n_idx; i++) {
        if (idx[i] >= extent)
            fail(SCANRS_ERR_INVALID, "index out of range: entry %llu of the list is %llu, the matrix has %llu %s", (unsigned long long)i,
                 (unsigned long long)idx[i], (unsigned long long)extent, axis);
        h[i] = (uint32_t)idx[i];
    }
    return h;
}
} // namespace

void select_outer(Storage &st, const SparseCopy &cp, const uint64_t *idx, uint64_t n_idx, SparseCopy &out) {
    const std::vector<uint32_t> h = checked_indices(idx, n_idx, cp.n_outer, "outer vectors");
    start_copy(st, cp, out, n_idx, cp.n_inner);
    DevBuf<uint32_t> d_idx;
    upload(st, d_idx, h);
    launch_gather_len(st.stream, cp, d_idx.p, n_idx, reinterpret_cast<unsigned long long *>(out.indptr.p));
    offsets_and_room(st, out);
    launch_gather_copy(st.stream, cp, d_idx.p, n_idx, out.indptr.p, out.indices.p, out.values.p);
    SCANRS_SYNC(st.stream); // the index list is released on return
}

void select_outer_sharded(Storage &st, const SparseCopy &cp, const uint64_t *idx, uint64_t n_idx, SparseCopy &out, uint64_t *out_begin) {
    // the list and the rank's own range decide everything, and every rank sees the same list: the refusals below come on every rank,
    // before any device work, and no exchange is needed
    checked_indices(idx, n_idx, st.shard.outer_global, "outer vectors");
    for (uint64_t i = 1; i < n_idx; i++)
        if (idx[i] < idx[i - 1])
            fail(SCANRS_ERR_ARGUMENT,
                 "the list along the sharded dimension must not descend: entry %llu is %llu after %llu (moving vectors between ranks is not supported)",
                 (unsigned long long)i, (unsigned long long)idx[i], (unsigned long long)idx[i - 1]);
    const uint64_t lo = st.shard.outer_begin, hi = lo + cp.n_outer;
    const uint64_t *first = std::lower_bound(idx, idx + n_idx, lo), *last = std::lower_bound(first, idx + n_idx, hi);
    std::vector<uint64_t> local(first, last);
    for (uint64_t &x : local) x -= lo;
    *out_begin = (uint64_t)(first - idx);
    select_outer(st, cp, local.data(), local.size(), out);
}

void select_inner(Storage &st, const SparseCopy &cp, const uint64_t *idx, uint64_t n_idx, SparseCopy &out) {
    const std::vector<uint32_t> h = checked_indices(idx, n_idx, cp.n_inner, "positions on that axis");
    start_copy(st, cp, out, cp.n_outer, n_idx);
    // the inverse list: for every source position its places in idx, ascending (a counting sort keeps them so)
    std::vector<uint32_t> inv_ptr(cp.n_inner + 1, 0), inv_pos(n_idx);
    bool ascending = true;
    for (uint64_t i = 0; i < n_idx; i++) {
        inv_ptr[h[i] + 1ull]++;
        if (i && h[i] <= h[i - 1]) ascending = false;
    }
    for (uint64_t j = 0; j < cp.n_inner; j++) inv_ptr[j + 1] += inv_ptr[j];
    {
        std::vector<uint32_t> at(inv_ptr.begin(), inv_ptr.end() - 1);
        for (uint64_t i = 0; i < n_idx; i++) inv_pos[at[h[i]]++] = (uint32_t)i;
    }
    DevBuf<uint32_t> d_ptr, d_pos;
    upload(st, d_ptr, inv_ptr);
    upload(st, d_pos, inv_pos);
    launch_expand_count(st.stream, cp, d_ptr.p, reinterpret_cast<unsigned long long *>(out.indptr.p));
    offsets_and_room(st, out);
    launch_expand_fill(st.stream, cp, d_ptr.p, d_pos.p, out.indptr.p, out.indices.p, out.values.p);
    SCANRS_SYNC(st.stream);
    // a strictly ascending list emits every vector in ascending order already; otherwise the new indices (distinct within a vector)
    // are sorted per vector, the repair scanrs_mat_create_unsorted applies
    if (!ascending) sort_outer_vectors(st, out);
}

uint64_t partition_on_thresholds(Storage &st, const SparseCopy &cp, const double *thr_outer, const double *thr_inner, bool cols_inner,
                                 std::vector<uint8_t> &excl_outer, std::vector<uint8_t> &excl_inner, SparseCopy *filtered, SparseCopy *residual,
                                 PartitionShard *sh) {
    hipStream_t s = st.stream;
    const uint64_t no = cp.n_outer, ni = cp.n_inner;
    // sh: cp is this rank's shard of outer_global outer vectors. The inner positions, their mask and the round's flag are
    // replicated: every rank marks them from the same reduced sums. The outer vectors, their sums and their mask stay local.
    const uint64_t no_all = sh ? st.shard.outer_global : no;
    if (no_all >= 0x7FFFFFFFull || ni >= 0x7FFFFFFFull) fail(SCANRS_ERR_SHAPE, "partition_on_thresholds needs dimensions below 2^31 - 1");
    // (the counts of the three exchanges below are the same on every rank: the inner extent, one flag, the global outer extent)
    ShardExchange ex{st, st.partition_allreduces};
    DevBuf<uint8_t> d_eo(std::max<uint64_t>(1, no)), d_ei(std::max<uint64_t>(1, ni)), d_no(std::max<uint64_t>(1, no)), d_ni(std::max<uint64_t>(1, ni));
    DevBuf<unsigned long long> d_so(std::max<uint64_t>(1, no)), d_si(std::max<uint64_t>(1, ni));
    DevBuf<unsigned long long> d_sr; // sharded: the reduced copy of the inner sums (d_si keeps this rank's own, for the subtraction)
    if (sh && thr_inner) d_sr.alloc(std::max<uint64_t>(1, ni));
    DevBuf<uint32_t> d_flag(2); // (8 bytes: a sharded call sums the flag over the ranks as one u64)
    SCANRS_HIP(hipMemsetAsync(d_eo.p, 0, d_eo.n, s));
    SCANRS_HIP(hipMemsetAsync(d_ei.p, 0, d_ei.n, s));
    SCANRS_HIP(hipMemsetAsync(d_no.p, 0, d_no.n, s));
    SCANRS_HIP(hipMemsetAsync(d_ni.p, 0, d_ni.n, s));
    bool inner_sums_made = false;
    // the sums of the outer vectors over the inner positions not yet excluded: a full masked pass
    auto step_outer = [&] {
        if (!thr_outer) return;
        launch_sel_outer_sums(s, cp, d_eo.p, d_ei.p, d_so.p);
        launch_sel_mark(s, d_so.p, no, *thr_outer, d_eo.p, d_no.p, d_flag.p);
    };
    // the sums per inner position over the outer vectors not yet excluded: made once, then the vectors excluded since are taken out
    auto step_inner = [&] {
        if (!thr_inner) return;
        if (!inner_sums_made) {
            SCANRS_HIP(hipMemsetAsync(d_si.p, 0, d_si.n * 8, s));
            launch_sel_inner_sums(s, cp, d_eo.p, 0, false, d_ei.p, d_si.p);
            inner_sums_made = true;
        } else {
            launch_sel_inner_sums(s, cp, d_no.p, 1, true, d_ei.p, d_si.p);
        }
        SCANRS_HIP(hipMemsetAsync(d_no.p, 0, d_no.n, s));
        const unsigned long long *sums = d_si.p;
        if (sh) {
            if (ni) {
                SCANRS_HIP(hipMemcpyAsync(d_sr.p, d_si.p, ni * 8, hipMemcpyDeviceToDevice, s));
                ex.sum(d_sr.p, ni);
            }
            sums = d_sr.p;
        }
        launch_sel_mark(s, sums, ni, *thr_inner, d_ei.p, d_ni.p, d_flag.p);
    };
    uint64_t rounds = 0;
    for (;;) { // mat.rs:783-806: columns first, then rows over the columns as just updated, until a round adds nothing
        SCANRS_HIP(hipMemsetAsync(d_flag.p, 0, 8, s));
        if (cols_inner) {
            step_inner();
            step_outer();
        } else {
            step_outer();
            step_inner();
        }
        rounds++;
        // the outer marks are local news: the ranks agree on the flag before they read it, and so stop in the same round (the inner
        // marks come from replicated sums and set the same flag everywhere)
        if (sh && thr_outer) ex.sum(reinterpret_cast<unsigned long long *>(d_flag.p), 1);
        if (!SCANRS_D2H_VALUE(d_flag.p, s)) break; // the one value a round sends back
    }
    excl_outer.assign(no, 0);
    excl_inner.assign(ni, 0);
    if (no) SCANRS_D2H(excl_outer.data(), d_eo.p, no, s);
    if (ni) SCANRS_D2H(excl_inner.data(), d_ei.p, ni, s);
    SCANRS_SYNC(s);
    if (sh) {
        // the outer mask of the whole matrix: every rank puts its bytes at its place in a zero-filled array of u64 words; one
        // contributor per byte, so the sum is a copy (no carries)
        const uint64_t words = (no_all + 7) / 8;
        DevBuf<unsigned long long> d_all(std::max<uint64_t>(1, words));
        SCANRS_HIP(hipMemsetAsync(d_all.p, 0, words * 8, s));
        if (no) SCANRS_HIP(hipMemcpyAsync(reinterpret_cast<uint8_t *>(d_all.p) + st.shard.outer_begin, d_eo.p, no, hipMemcpyDeviceToDevice, s));
        if (words) ex.sum(d_all.p, words);
        sh->excl_outer_all.assign(no_all, 0);
        if (no_all) SCANRS_D2H(sh->excl_outer_all.data(), d_all.p, no_all, s);
        SCANRS_SYNC(s);
    }
    if (!filtered && !residual) return rounds;

    // where every vector and every inner position goes (part_count_kernel / part_fill_kernel)
    std::vector<int32_t> pos_a(std::max<uint64_t>(1, no), -1), pos_b(std::max<uint64_t>(1, no), -1), remap(std::max<uint64_t>(1, ni), -1);
    int32_t kept_o = 0, gone_o = 0, kept_i = 0, gone_i = 0;
    for (uint64_t j = 0; j < ni; j++) remap[j] = excl_inner[j] ? ~(gone_i++) : kept_i++;
    for (uint64_t o = 0; o < no; o++) {
        if (!excl_outer[o]) {
            if (filtered) pos_a[o] = kept_o;
            if (residual && cols_inner) pos_b[o] = kept_o;
            kept_o++;
        } else {
            if (residual && !cols_inner) pos_b[o] = gone_o;
            gone_o++;
        }
    }
    DevBuf<int32_t> d_pa, d_pb, d_rm;
    upload(st, d_pa, pos_a);
    upload(st, d_pb, pos_b);
    upload(st, d_rm, remap);
    SparseCopy none_a, none_b; // stand-ins for a matrix that is not wanted: no vector is sent there
    SparseCopy &fa = filtered ? *filtered : none_a, &rb = residual ? *residual : none_b;
    start_copy(st, cp, fa, filtered ? (uint64_t)kept_o : 0, (uint64_t)kept_i);
    start_copy(st, cp, rb, residual ? (uint64_t)(cols_inner ? kept_o : gone_o) : 0, (uint64_t)(cols_inner ? gone_i : kept_i));
    launch_part_count(s, cp, d_pa.p, d_pb.p, d_rm.p, cols_inner, reinterpret_cast<unsigned long long *>(fa.indptr.p),
                      reinterpret_cast<unsigned long long *>(rb.indptr.p));
    offsets_and_room(st, fa);
    offsets_and_room(st, rb);
    launch_part_fill(s, cp, d_pa.p, d_pb.p, d_rm.p, cols_inner, fa.indptr.p, fa.indices.p, fa.values.p, rb.indptr.p, rb.indices.p, rb.values.p);
    SCANRS_SYNC(s);
    return rounds;
}

} // namespace scanrs
