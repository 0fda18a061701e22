// Construction of a SparseCopy on the device for gfx950 (MI355X): validation, the work items of the gather kernels, the repair
// of unsorted or zero-holding input, and the transposed copy (key pack / unpack around rocprim's radix sort).
#include "common.hpp"
#include "launch_util.hpp"
#include "transpose_plan.hpp"

#include <algorithm>
#include <rocprim/rocprim.hpp>

namespace scanrs {

// transpose helpers
// packed[p] = (outer id << 32) | count: one wave per work item (a run of at most ITEM_NNZ nonzeros of one outer vector), so the
// outer id is known without a search and the nonzeros stream (a binary search in indptr per nonzero took 17 ms at 10^9)
__global__ __launch_bounds__(256) void pack_outer_kernel(const Item *__restrict__ items, uint32_t n_items, const uint32_t *__restrict__ values,
                                                         unsigned long long *__restrict__ packed) {
    const uint32_t wid = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (wid >= n_items) return;
    const Item it = items[wid];
    const unsigned long long hi = (unsigned long long)it.row << 32;
    for (uint32_t k = lane; k < it.len; k += 64u) packed[it.start + k] = hi | values[it.start + k];
}
// One 64-bit sort key per nonzero when (inner index, outer id, count) fit together: key = inner << (ob + cb) | outer << cb | count,
// sorted on the inner bits only (stable: ascending outer ids inside an inner vector are kept). 8 bytes per nonzero and pass instead
// of the 12 of a (u32 key, u64 value) pair sort, and two 8 GB buffers instead of 24 GB of temporaries at 10^9 nonzeros.
__global__ __launch_bounds__(256) void pack_key_kernel(const Item *__restrict__ items, uint32_t n_items, const uint32_t *__restrict__ indices,
                                                       const uint32_t *__restrict__ values, uint32_t ob, uint32_t cb,
                                                       unsigned long long *__restrict__ keys) {
    const uint32_t wid = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (wid >= n_items) return;
    const Item it = items[wid];
    const unsigned long long mid = (unsigned long long)it.row << cb;
    for (uint32_t k = lane; k < it.len; k += 64u)
        keys[it.start + k] = ((unsigned long long)indices[it.start + k] << (ob + cb)) | mid | values[it.start + k];
}
__global__ void unpack_key_kernel(const unsigned long long *__restrict__ keys, uint64_t nnz, uint32_t ob, uint32_t cb, uint32_t *__restrict__ ind,
                                  uint32_t *__restrict__ val) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const unsigned long long x = keys[p];
    ind[p] = (uint32_t)((x >> cb) & ((1ull << ob) - 1ull));
    val[p] = (uint32_t)(x & ((1ull << cb) - 1ull));
}
__global__ void lower_bound_key_kernel(const unsigned long long *__restrict__ keys, uint64_t nnz, uint64_t n_inner, uint32_t shift,
                                       uint64_t *__restrict__ indptr) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_inner) return;
    uint64_t lo = 0, hi = nnz;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if ((keys[mid] >> shift) < i)
            lo = mid + 1;
        else
            hi = mid;
    }
    indptr[i] = lo;
}
__global__ void unpack_kernel(const unsigned long long *__restrict__ packed, uint64_t nnz, uint32_t *__restrict__ ind,
                              uint32_t *__restrict__ val) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const unsigned long long x = packed[p];
    ind[p] = (uint32_t)(x >> 32);
    val[p] = (uint32_t)x;
}
__global__ void lower_bound_kernel(const uint32_t *__restrict__ keys, uint64_t nnz, uint64_t n_inner,
                                   uint64_t *__restrict__ indptr) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_inner) return;
    uint64_t lo = 0, hi = nnz;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (keys[mid] < i)
            lo = mid + 1;
        else
            hi = mid;
    }
    indptr[i] = lo;
}
// Validation as two passes that both stream: (a) over the nonzeros, 4 per thread: stored zeros, indices out of range, and
// DESCENTS — positions whose index is not above its predecessor's, wherever they are; (b) over the outer vectors: a descent at the
// first nonzero of a vector is no violation (it compares with the previous vector's last index) and is taken off again, and
// indptr itself must not decrease. violations = out of range + descents - descents at vector starts + decreasing indptr entries.
// (One thread per outer vector walking its nonzeros, the round-1 form, read every line a dozen times: 45 ms at 10^9 nonzeros.)
__global__ __launch_bounds__(256) void validate_stream_kernel(const uint32_t *__restrict__ indices, const uint32_t *__restrict__ values, uint64_t nnz,
                                                              uint64_t n_inner, unsigned long long *__restrict__ counters) {
    unsigned long long zeros = 0, bad = 0;
    uint32_t vmax = 0;
    const uint4 *I4 = reinterpret_cast<const uint4 *>(indices), *V4 = reinterpret_cast<const uint4 *>(values);
    const uint64_t n4 = (nnz + 3) / 4; // the arrays are padded (DevBuf): the last chunk may be read whole
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n4; c += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 ix = I4[c], vv = V4[c];
        const uint32_t prev = c ? indices[c * 4 - 1] : 0u;
        const uint32_t i[4] = {ix.x, ix.y, ix.z, ix.w}, v[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint64_t p = c * 4 + k;
            if (p >= nnz) break;
            zeros += v[k] == 0u;
            vmax = v[k] > vmax ? v[k] : vmax;
            bad += (uint64_t)i[k] >= n_inner;
            if (p > 0) bad += i[k] <= (k ? i[k - 1] : prev);
        }
    }
    // wave sums, then one set of atomics per WORKGROUP of a grid of a few thousand (every wave of a 65 536-block grid adding to the
    // same four words was 13 of the pass's 18 ms: same-address atomics are served one after the other)
    for (int off = 32; off > 0; off >>= 1) {
        zeros += __shfl_down(zeros, off);
        bad += __shfl_down(bad, off);
        const uint32_t o = __shfl_down(vmax, off);
        vmax = o > vmax ? o : vmax;
    }
    __shared__ unsigned long long sz[4], sb[4];
    __shared__ uint32_t sm[4];
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) {
        sz[w] = zeros;
        sb[w] = bad;
        sm[w] = vmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long z = sz[0] + sz[1] + sz[2] + sz[3], b = sb[0] + sb[1] + sb[2] + sb[3];
        const uint32_t m = max(max(sm[0], sm[1]), max(sm[2], sm[3]));
        if (z) atomicAdd(&counters[0], z);
        if (b) atomicAdd(&counters[1], b);
        atomicMax(&counters[3], (unsigned long long)m); // the largest count: bounds the mapped values (col_moments_kernel) and sizes the transposed copy's sort key
    }
}
__global__ void validate_starts_kernel(const uint64_t *__restrict__ indptr, uint64_t n_outer, const uint32_t *__restrict__ indices, uint64_t nnz,
                                       unsigned long long *__restrict__ counters) {
    const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool broken = false, start_descent = false;
    if (o < n_outer) {
        const uint64_t a = indptr[o], b = indptr[o + 1];
        broken = b < a || b > nnz;
        // the first nonzero of a non-empty vector that follows another nonzero: a descent there was counted by the streaming pass
        start_descent = !broken && b > a && a > 0 && indices[a] <= indices[a - 1];
    }
    // nearly EVERY vector start is such a descent (a cell's first gene lies below the previous cell's last one): one atomic per wave,
    // not per vector (10^6 adds to one word took 10 ms)
    const unsigned long long nb = __popcll(__builtin_amdgcn_ballot_w64(broken)), nd = __popcll(__builtin_amdgcn_ballot_w64(start_descent));
    if ((threadIdx.x & 63u) == 0) {
        if (nb) atomicAdd(&counters[1], nb);
        if (nd) atomicAdd(&counters[2], nd);
    }
}

// Work items of the gather kernels, built on the device: per outer vector the number of pieces (1, or ceil(len / ITEM_NNZ) for a
// long vector, which also gets a MultiRow and slab rows), two exclusive scans, one fill pass — the host only reads the three
// totals (it used to walk indptr on one core: 8 MB down, a loop over every vector, 24 MB of items up, ~15 ms at 10^6 cells).
__global__ void item_count_kernel(const uint64_t *__restrict__ indptr, uint64_t n_outer, unsigned long long *__restrict__ pieces,
                                  unsigned long long *__restrict__ multi_slab) {
    const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o > n_outer) return;
    if (o == n_outer) { // the scans run over n_outer + 1 entries: the last one receives the totals
        pieces[o] = 0;
        multi_slab[o] = 0;
        return;
    }
    const uint64_t len = indptr[o + 1] - indptr[o];
    const bool multi = len > ITEM_NNZ;
    const unsigned long long np = multi ? (len + ITEM_NNZ - 1) / ITEM_NNZ : 1ull;
    pieces[o] = np;
    multi_slab[o] = multi ? (1ull | (np << 32)) : 0ull; // low word: MultiRows so far, high word: slab rows so far
}
__global__ void item_fill_kernel(const uint64_t *__restrict__ indptr, uint64_t n_outer, const unsigned long long *__restrict__ item_off,
                                 const unsigned long long *__restrict__ multi_slab_off, Item *__restrict__ items, MultiRow *__restrict__ multi) {
    const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n_outer) return;
    const uint64_t a = indptr[o], b = indptr[o + 1], len = b - a;
    const uint64_t at = item_off[o];
    if (len <= ITEM_NNZ) {
        items[at] = Item{a, (uint32_t)o, (uint32_t)len, NO_SLAB, 0};
        return;
    }
    const uint32_t pieces = (uint32_t)((len + ITEM_NNZ - 1) / ITEM_NNZ);
    const unsigned long long ms = multi_slab_off[o];
    const uint32_t slab0 = (uint32_t)(ms >> 32);
    multi[(uint32_t)ms] = MultiRow{(uint32_t)o, slab0, pieces, 0};
    for (uint32_t k = 0; k < pieces; k++) {
        const uint64_t s0 = a + (uint64_t)k * ITEM_NNZ;
        const uint64_t ln = b - s0 < ITEM_NNZ ? b - s0 : ITEM_NNZ;
        items[at + k] = Item{s0, (uint32_t)o, (uint32_t)ln, slab0 + k, 0};
    }
}

void SparseCopy::build_items(hipStream_t s) {
    n_items = n_multi = n_slab = 0;
    if (n_outer == 0) {
        items.alloc(0);
        multi.alloc(0);
        return;
    }
    const size_t n = (size_t)n_outer + 1;
    DevBuf<unsigned long long> cnt(2 * n), off(2 * n);
    const dim3 grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(item_count_kernel, grid, dim3(256), 0, s, indptr.p, n_outer, cnt.p, cnt.p + n);
    size_t tmp_bytes = 0;
    SCANRS_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, cnt.p, off.p, 0ull, n, rocprim::plus<unsigned long long>(), s));
    DevBuf<char> tmp(std::max<size_t>(tmp_bytes, 16));
    SCANRS_HIP(rocprim::exclusive_scan(tmp.p, tmp_bytes, cnt.p, off.p, 0ull, n, rocprim::plus<unsigned long long>(), s));
    SCANRS_HIP(rocprim::exclusive_scan(tmp.p, tmp_bytes, cnt.p + n, off.p + n, 0ull, n, rocprim::plus<unsigned long long>(), s));
    const unsigned long long tot[2] = {SCANRS_D2H_VALUE(off.p + n_outer, s), SCANRS_D2H_VALUE(off.p + n + n_outer, s)};
    if (tot[0] > 0xFFFFFFFFull) fail(SCANRS_ERR_SHAPE, "matrix needs more than 2^32 - 1 work items");
    n_items = (uint32_t)tot[0];
    n_multi = (uint32_t)tot[1];
    n_slab = (uint32_t)(tot[1] >> 32);
    items.alloc(n_items);
    multi.alloc(n_multi);
    hipLaunchKernelGGL(item_fill_kernel, grid, dim3(256), 0, s, indptr.p, n_outer, off.p, off.p + n, items.p, multi.p);
    SCANRS_HIP(hipGetLastError());
    SCANRS_SYNC(s); // the temporaries are released on return
}

void validate_copy(Storage &st, SparseCopy &cp, uint64_t *zeros, uint64_t *bad) {
    DevBuf<unsigned long long> c(4);
    SCANRS_HIP(hipMemsetAsync(c.p, 0, 4 * sizeof(unsigned long long), st.stream));
    if (cp.n_outer) {
        hipLaunchKernelGGL(validate_starts_kernel, grid1(cp.n_outer, 256), dim3(256), 0, st.stream, cp.indptr.p, cp.n_outer, cp.indices.p, cp.nnz, c.p);
        // a broken indptr first: the streaming pass below trusts nnz only, the later passes trust indptr
        const unsigned long long h1 = SCANRS_D2H_VALUE(c.p + 1, st.stream);
        if (h1) {
            *zeros = 0;
            *bad = h1;
            return;
        }
    }
    if (cp.nnz) {
        const uint64_t n4 = (cp.nnz + 3) / 4;
        int dev = 0, n_cu = 256;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
        const unsigned blocks = (unsigned)std::min<uint64_t>((n4 + 255) / 256, (uint64_t)n_cu * 16u);
        hipLaunchKernelGGL(validate_stream_kernel, dim3(blocks), dim3(256), 0, st.stream, cp.indices.p, cp.values.p, cp.nnz, cp.n_inner, c.p);
    }
    struct H4 {
        unsigned long long v[4];
    };
    const H4 h4 = SCANRS_D2H_VALUE(reinterpret_cast<const H4 *>(c.p), st.stream);
    const unsigned long long *h = h4.v;
    *zeros = h[0];
    *bad = h[1] - std::min(h[1], h[2]);
    if (cp.nnz) cp.max_value = (uint32_t)std::max<unsigned long long>(1ull, h[3]);
}

void compact_nonzeros(Storage &st, SparseCopy &cp) {
    // Rare path (AbsIter skips stored zeros, sqz/src/vec.rs:113): rebuild on the host.
    std::vector<uint64_t> ip(cp.n_outer + 1);
    std::vector<uint32_t> ind(cp.nnz), val(cp.nnz);
    SCANRS_HIP(hipMemcpy(ip.data(), cp.indptr.p, ip.size() * 8, hipMemcpyDeviceToHost));
    if (cp.nnz) {
        SCANRS_HIP(hipMemcpy(ind.data(), cp.indices.p, cp.nnz * 4, hipMemcpyDeviceToHost));
        SCANRS_HIP(hipMemcpy(val.data(), cp.values.p, cp.nnz * 4, hipMemcpyDeviceToHost));
    }
    std::vector<uint64_t> np(cp.n_outer + 1, 0);
    uint64_t w = 0;
    for (uint64_t o = 0; o < cp.n_outer; o++) {
        np[o] = w;
        for (uint64_t p = ip[o]; p < ip[o + 1]; p++)
            if (val[p] != 0) {
                ind[w] = ind[p];
                val[w] = val[p];
                w++;
            }
    }
    np[cp.n_outer] = w;
    cp.nnz = w;
    SCANRS_HIP(hipMemcpy(cp.indptr.p, np.data(), np.size() * 8, hipMemcpyHostToDevice));
    if (w) {
        SCANRS_HIP(hipMemcpy(cp.indices.p, ind.data(), w * 4, hipMemcpyHostToDevice));
        SCANRS_HIP(hipMemcpy(cp.values.p, val.data(), w * 4, hipMemcpyHostToDevice));
    }
    (void)st;
}

// Sorts (index, count) pairs by index inside every outer vector: the repair the reference applies to 10x matrix files
// whose indices are unsorted within a cell (`new_from_unsorted_csc`, hdf5-io/src/matrix.rs:66-75).
void sort_outer_vectors(Storage &st, SparseCopy &cp) {
    if (cp.nnz == 0) return;
    if (cp.nnz > 0xFFFFFFFFull || cp.n_outer > 0xFFFFFFFFull) fail(SCANRS_ERR_SHAPE, "unsorted input beyond 2^32-1 nonzeros is not supported");
    DevBuf<uint32_t> keys_out, vals_out;
    keys_out.alloc(cp.nnz);
    vals_out.alloc(cp.nnz);
    uint32_t end_bit = 1;
    while (end_bit < 32u && (cp.n_inner >> end_bit) != 0) end_bit++;
    size_t tmp_bytes = 0;
    SCANRS_HIP(rocprim::segmented_radix_sort_pairs(nullptr, tmp_bytes, cp.indices.p, keys_out.p, cp.values.p, vals_out.p, (unsigned)cp.nnz,
                                                   (unsigned)cp.n_outer, cp.indptr.p, cp.indptr.p + 1, 0u, end_bit, st.stream));
    DevBuf<unsigned char> tmp;
    tmp.alloc(tmp_bytes ? tmp_bytes : 1);
    SCANRS_HIP(rocprim::segmented_radix_sort_pairs(tmp.p, tmp_bytes, cp.indices.p, keys_out.p, cp.values.p, vals_out.p, (unsigned)cp.nnz,
                                                   (unsigned)cp.n_outer, cp.indptr.p, cp.indptr.p + 1, 0u, end_bit, st.stream));
    SCANRS_HIP(hipMemcpyAsync(cp.indices.p, keys_out.p, cp.nnz * 4, hipMemcpyDeviceToDevice, st.stream));
    SCANRS_HIP(hipMemcpyAsync(cp.values.p, vals_out.p, cp.nnz * 4, hipMemcpyDeviceToDevice, st.stream));
    SCANRS_SYNC(st.stream);
}

void build_transposed_copy(Storage &st, const SparseCopy &src, SparseCopy &dst, hipStream_t stream) {
    hipStream_t s = stream ? stream : st.stream;
    Tick tick("transposed copy build");
    dst.n_outer = src.n_inner;
    dst.n_inner = src.n_outer;
    dst.nnz = src.nnz;
    dst.indptr.alloc(dst.n_outer + 1);
    dst.indices.alloc(std::max<uint64_t>(1, dst.nnz));
    dst.values.alloc(std::max<uint64_t>(1, dst.nnz));
    const uint64_t nnz = src.nnz;
    if (nnz == 0) {
        SCANRS_HIP(hipMemsetAsync(dst.indptr.p, 0, (dst.n_outer + 1) * 8, s));
        dst.build_items(s);
        st.transpose_route = (uint64_t)TRANSPOSE_NONE; // nothing to sort
        return;
    }
    // which sort: transpose_plan.hpp (max_value is known for every copy that went through validation; an adopted copy carries a bound)
    const TransposePlan plan = transpose_plan(src.n_outer, src.n_inner, src.max_value);
    const uint32_t ob = plan.ob, cb = plan.cb;
    dst.max_value = src.max_value;
    st.transpose_route = (uint64_t)plan.route;
    if (plan.route == TRANSPOSE_PACKED_KEY) {
        // one packed 64-bit key per nonzero, sorted on its inner-index bits (see pack_key_kernel; a key of all 64 bits: transpose_plan.hpp)
        DevBuf<unsigned long long> ka(nnz), kb2(nnz);
        hipLaunchKernelGGL(pack_key_kernel, dim3((src.n_items + 3u) / 4u), dim3(256), 0, s, src.items.p, src.n_items, src.indices.p, src.values.p, ob, cb, ka.p);
        rocprim::double_buffer<unsigned long long> kb(ka.p, kb2.p);
        size_t tmp_bytes = 0;
        SCANRS_HIP(rocprim::radix_sort_keys(nullptr, tmp_bytes, kb, (size_t)nnz, plan.sort_begin, plan.sort_end, s));
        DevBuf<char> tmp(std::max<size_t>(tmp_bytes, 16));
        SCANRS_HIP(rocprim::radix_sort_keys(tmp.p, tmp_bytes, kb, (size_t)nnz, plan.sort_begin, plan.sort_end, s));
        hipLaunchKernelGGL(unpack_key_kernel, grid1(nnz, 256), dim3(256), 0, s, kb.current(), nnz, ob, cb, dst.indices.p, dst.values.p);
        hipLaunchKernelGGL(lower_bound_key_kernel, grid1(dst.n_outer + 1, 256), dim3(256), 0, s, kb.current(), nnz, dst.n_outer, ob + cb, dst.indptr.p);
        SCANRS_HIP(hipGetLastError());
        SCANRS_SYNC(s);
    } else {
        // stable LSD radix sort of (inner index, (outer id, value)): inner vectors come out with
        // ascending outer ids, the order the reference's CSC kernel accumulates in (prod.rs:190-214).
        DevBuf<uint32_t> keys_a(nnz), keys_b(nnz);
        DevBuf<unsigned long long> vals_a(nnz), vals_b(nnz);
        SCANRS_HIP(hipMemcpyAsync(keys_a.p, src.indices.p, nnz * 4, hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(pack_outer_kernel, dim3((src.n_items + 3u) / 4u), dim3(256), 0, s, src.items.p, src.n_items, src.values.p, vals_a.p);
        unsigned end_bit = 1;
        while (end_bit < 32 && (1ull << end_bit) < src.n_inner) end_bit++;
        rocprim::double_buffer<uint32_t> kb(keys_a.p, keys_b.p);
        rocprim::double_buffer<unsigned long long> vb(vals_a.p, vals_b.p);
        size_t tmp_bytes = 0;
        SCANRS_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, kb, vb, (size_t)nnz, 0u, end_bit, s));
        DevBuf<char> tmp(std::max<size_t>(tmp_bytes, 16));
        SCANRS_HIP(rocprim::radix_sort_pairs(tmp.p, tmp_bytes, kb, vb, (size_t)nnz, 0u, end_bit, s));
        hipLaunchKernelGGL(unpack_kernel, grid1(nnz, 256), dim3(256), 0, s, vb.current(), nnz, dst.indices.p,
                           dst.values.p);
        hipLaunchKernelGGL(lower_bound_kernel, grid1(dst.n_outer + 1, 256), dim3(256), 0, s, kb.current(), nnz,
                           dst.n_outer, dst.indptr.p);
        SCANRS_HIP(hipGetLastError());
        SCANRS_SYNC(s);
    }
    dst.build_items(s);
}

// scanrs_init(): loads this file's code object (library_warm_up, kernels.hip)
__global__ void warm_copy_build_kernel() {}
void warm_copy_build(hipStream_t s) { hipLaunchKernelGGL(warm_copy_build_kernel, dim3(1), dim3(64), 0, s); }

} // namespace scanrs
