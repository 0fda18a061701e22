// encode.hip — sqz::AdaptiveVec encoders on the device: the inverse of decode.hip (`AdaptiveMat::from_csmat`, sqz/src/mat.rs:92-124;
// `AdaptiveVec::new`, vec.rs:1086-1160).
//
// Input is a handle's own triplet (indptr u64, indices u32, values u32); output is two arenas, 64-bit words that hold the byte
// pieces (`data`, `index_bytes`; every piece starts on a word and is padded to one, the padding is zero) and 32-bit words (fallback
// indexes / values, `block_starts`, the indexes and values of V). Everything is integer work and every output word is stored once,
// by one lane that depends on the data alone: the arenas are the same bits whatever the launch geometry, there is no atomic.
//
//   enc_count_kernel     a block per chunk of CH stored entries of the flat `values` array: how many reach the markers 7, 15, 255 and
//                        65535 (four 16-bit counts in one u64, one block scan for the four), and the same prefix at every vector
//                        boundary that falls into the chunk. With the scanned chunk counts this is P_w(e), the entries before e that
//                        reach marker w — the per-vector counts AND the places in the fallback lists come from it
//   enc_plan_kernel      a thread per vector: counts = P(end) - P(start), choose_storage (adaptive_choose.hpp) or the forced kind, the
//                        sizes of its pieces in both arenas. Two exclusive scans of the sizes give every vector's offsets
//   enc_bytes_kernel     a thread per 64-bit word of the byte arena: 21 / 16 / 8 / 4 fields of `data` or 8 index bytes. S*: the
//                        fields of consecutive entries; D*: a lower bound of the word's first position in the vector's ascending
//                        indices, then a walk; words without entries are zero
//   enc_words_kernel     a thread per 32-bit word outside the fallback lists: `block_starts[b]` = lower bound of 256 b, the last one
//                        = n; the copy of indices and values for V
//   enc_fallback_kernel  the chunks of enc_count_kernel again: an entry that reaches its vector's marker goes to place
//                        P_w(e) - P_w(vector start) of the fallback list, keyed by position (D*) or entry number (S*): a stream
//                        compaction in a fixed order
//
// A lane finds the vector that owns its word (or entry) by a search in the scanned offsets, narrowed to the vectors its block
// touches (two lanes search the whole table, the rest a handful of entries).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "adaptive_choose.hpp"
#include "common.hpp"
#include "launch_util.hpp"

#include <rocprim/rocprim.hpp>

namespace scanrs {

namespace {

constexpr uint32_t CH = 2048; // entries per chunk: the four counts of a chunk fit 16 bits each
constexpr uint32_t PER_T = CH / 256;

__device__ __forceinline__ unsigned long long pack_over(uint32_t v) {
    return (unsigned long long)(v >= 7u) | ((unsigned long long)(v >= 15u) << 16) | ((unsigned long long)(v >= 255u) << 32) |
           ((unsigned long long)(v >= 65535u) << 48);
}
__device__ __forceinline__ uint64_t field16(unsigned long long packed, uint32_t w) { return (packed >> (16u * w)) & 0xFFFFull; }

// first i in [0, n) with a[i] >= key (n when none)
template <typename T>
__device__ __forceinline__ uint64_t lower_bound_dev(const T *__restrict__ a, uint64_t n, uint64_t key) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if ((uint64_t)a[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
// the last o in [lo, hi] with offs[o] <= pos; one exists. Among vectors that start at the same offset this is the last one, the
// only one that can be non-empty: the owner of `pos` whenever pos lies below the total.
__device__ __forceinline__ uint64_t owner_of(const uint64_t *__restrict__ offs, uint64_t lo, uint64_t hi, uint64_t pos) {
    uint64_t a = lo, b = hi + 1; // first index in [lo, hi + 1) with offs > pos
    while (a < b) {
        const uint64_t mid = (a + b) >> 1;
        if (offs[mid] <= pos)
            a = mid + 1;
        else
            b = mid;
    }
    return a - 1;
}
// the owners of the block's first and last position, found once per block
__device__ __forceinline__ void block_owner_range(const uint64_t *__restrict__ offs, uint64_t n_vecs, uint64_t first, uint64_t last, uint64_t *sh) {
    if (threadIdx.x == 0) sh[0] = owner_of(offs, 0, n_vecs - 1, first);
    if (threadIdx.x == 64) sh[1] = owner_of(offs, 0, n_vecs - 1, last);
    __syncthreads();
}

// The chunk's entries of this thread (entries beyond nnz count as 0; every buffer of a copy has DevBuf::SLACK behind it), their packed
// flags, and the block-wide exclusive prefix of the flags in front of the thread's first entry. total: the whole chunk.
__device__ __forceinline__ unsigned long long chunk_prefix(const uint32_t *__restrict__ values, uint64_t nnz, uint64_t e0, uint32_t val[PER_T],
                                                           unsigned long long *wave_tot, unsigned long long &total) {
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if (e0 < nnz) { // (reads at most 7 entries past the end: inside the slack)
        lo = *reinterpret_cast<const uint4 *>(values + e0);
        hi = *reinterpret_cast<const uint4 *>(values + e0 + 4);
    }
    const uint32_t raw[PER_T] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    unsigned long long mine = 0;
#pragma unroll
    for (uint32_t q = 0; q < PER_T; q++) {
        val[q] = e0 + q < nnz ? raw[q] : 0u;
        mine += pack_over(val[q]);
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(incl, o, 64);
        if ((int)lane >= o) incl += t;
    }
    if (lane == 63u) wave_tot[wave] = incl;
    __syncthreads();
    unsigned long long before = 0;
    total = 0;
    for (uint32_t w = 0; w < 4u; w++) {
        if (w < wave) before += wave_tot[w];
        total += wave_tot[w];
    }
    return before + incl - mine;
}

__global__ __launch_bounds__(256) void enc_count_kernel(const uint64_t *__restrict__ indptr, uint64_t n_outer, const uint32_t *__restrict__ values,
                                                        uint64_t nnz, uint64_t n_chunks, unsigned long long *__restrict__ cnt,
                                                        unsigned long long *__restrict__ part) {
    __shared__ unsigned long long wave_tot[4];
    __shared__ unsigned long long pre[CH];
    __shared__ uint64_t bound[2];
    const uint64_t chunk = blockIdx.x, base = chunk * CH;
    uint32_t val[PER_T];
    unsigned long long total;
    unsigned long long run = chunk_prefix(values, nnz, base + (uint64_t)threadIdx.x * PER_T, val, wave_tot, total);
    if (threadIdx.x < 4u) cnt[(uint64_t)threadIdx.x * (n_chunks + 1) + chunk] = field16(total, threadIdx.x);
#pragma unroll
    for (uint32_t q = 0; q < PER_T; q++) {
        pre[threadIdx.x * PER_T + q] = run;
        run += pack_over(val[q]);
    }
    // the vector boundaries inside [base, base + CH): their prefix within the chunk (a boundary at nnz beyond the last chunk keeps 0)
    if (threadIdx.x == 0) bound[0] = lower_bound_dev(indptr, n_outer + 1, base);
    if (threadIdx.x == 64) bound[1] = lower_bound_dev(indptr, n_outer + 1, base + CH);
    __syncthreads();
    for (uint64_t o = bound[0] + threadIdx.x; o < bound[1]; o += 256u) part[o] = pre[indptr[o] - base];
}

__global__ __launch_bounds__(256) void enc_plan_kernel(const uint64_t *__restrict__ indptr, uint64_t n_outer, uint64_t len, uint64_t n_chunks,
                                                       const unsigned long long *__restrict__ cnt, const unsigned long long *__restrict__ part,
                                                       int force_kind, EncodedVec *__restrict__ desc, unsigned long long *__restrict__ bytes_sz,
                                                       unsigned long long *__restrict__ words_sz) {
    const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n_outer) return;
    const uint64_t a = indptr[o], b = indptr[o + 1], n = b - a;
    uint64_t pa[4], over[4];
#pragma unroll
    for (uint32_t w = 0; w < 4u; w++) {
        pa[w] = cnt[(uint64_t)w * (n_chunks + 1) + a / CH] + field16(part[o], w);
        over[w] = cnt[(uint64_t)w * (n_chunks + 1) + b / CH] + field16(part[o + 1], w) - pa[w];
    }
    const uint32_t kind = force_kind >= 0 ? (uint32_t)force_kind : adaptive::choose_storage(len, n, over, nullptr);
    EncodedVec d;
    d.kind = kind;
    d.n = (uint32_t)n;
    d._pad = 0;
    uint64_t nb = 0, nw = 0;
    if (kind == adaptive::V) {
        d.n_fb = (uint32_t)n;
        d.fb_base = 0;
        nw = 2 * n;
    } else {
        const uint32_t w = adaptive::width_of(kind);
        d.n_fb = (uint32_t)over[w];
        d.fb_base = pa[w];
        nb = (adaptive::data_bytes(kind, adaptive::is_dense(kind) ? len : n) + 7ull) & ~7ull;
        nw = 2 * over[w];
        if (adaptive::is_sparse(kind)) {
            nb += (n + 7ull) & ~7ull;
            nw += adaptive::n_block_starts(len);
        }
    }
    desc[o] = d;
    bytes_sz[o] = nb;
    words_sz[o] = nw;
}

__global__ __launch_bounds__(256) void enc_bytes_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                        const uint32_t *__restrict__ values, uint64_t n_outer, uint64_t len,
                                                        const EncodedVec *__restrict__ desc, const uint64_t *__restrict__ byte_off, uint64_t n_words64,
                                                        uint64_t *__restrict__ arena) {
    __shared__ uint64_t range[2];
    const uint64_t w0 = (uint64_t)blockIdx.x * 256u, w = w0 + threadIdx.x;
    block_owner_range(byte_off, n_outer, w0 * 8u, std::min<uint64_t>(w0 + 255u, n_words64 - 1) * 8u, range);
    if (w >= n_words64) return;
    const uint64_t o = owner_of(byte_off, range[0], range[1], w * 8u);
    const EncodedVec d = desc[o];
    const uint64_t a = indptr[o], n = d.n, rel = w * 8u - byte_off[o];
    const bool dense = adaptive::is_dense(d.kind);
    const uint64_t data_sz = (adaptive::data_bytes(d.kind, dense ? len : n) + 7ull) & ~7ull;
    uint64_t out = 0;
    if (rel < data_sz) {
        const uint32_t wd = adaptive::width_of(d.kind), bits = adaptive::bits_of(wd), marker = adaptive::marker_of(wd);
        const uint64_t per = adaptive::fields_per_u64(wd), u0 = (rel >> 3) * per;
        if (!dense) { // the fields of entries u0 .. u0 + per
            for (uint64_t i = 0; i < per && u0 + i < n; i++) out |= (uint64_t)std::min(values[a + u0 + i], marker) << (bits * (uint32_t)i);
        } else { // the fields of positions u0 .. u0 + per
            for (uint64_t e = lower_bound_dev(indices + a, n, u0); e < n; e++) {
                const uint64_t p = indices[a + e];
                if (p >= u0 + per) break;
                out |= (uint64_t)std::min(values[a + e], marker) << (bits * (uint32_t)(p - u0));
            }
        }
    } else { // index_bytes of entries u0 .. u0 + 8 (S* only)
        const uint64_t u0 = rel - data_sz;
        for (uint64_t i = 0; i < 8u && u0 + i < n; i++) out |= (uint64_t)(indices[a + u0 + i] & 255u) << (8u * (uint32_t)i);
    }
    arena[w] = out;
}

__global__ __launch_bounds__(256) void enc_words_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                        const uint32_t *__restrict__ values, uint64_t n_outer, uint64_t len,
                                                        const EncodedVec *__restrict__ desc, const uint64_t *__restrict__ word_off, uint64_t n_words,
                                                        uint32_t *__restrict__ arena) {
    __shared__ uint64_t range[2];
    const uint64_t x0 = (uint64_t)blockIdx.x * 256u, x = x0 + threadIdx.x;
    block_owner_range(word_off, n_outer, x0, std::min<uint64_t>(x0 + 255u, n_words - 1), range);
    if (x >= n_words) return;
    const uint64_t o = owner_of(word_off, range[0], range[1], x);
    const EncodedVec d = desc[o];
    const uint64_t a = indptr[o], n = d.n, rel = x - word_off[o];
    if (d.kind == adaptive::V) { // SimpleSparse: the indexes, then the values
        arena[x] = rel < n ? indices[a + rel] : values[a + rel - n];
        return;
    }
    if (rel < 2ull * d.n_fb) return; // the fallback lists: enc_fallback_kernel
    const uint64_t b = rel - 2ull * d.n_fb;
    arena[x] = b + 1 == adaptive::n_block_starts(len) ? (uint32_t)n : (uint32_t)lower_bound_dev(indices + a, n, 256ull * b);
}

__global__ __launch_bounds__(256) void enc_fallback_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                           const uint32_t *__restrict__ values, uint64_t n_outer, uint64_t nnz, uint64_t n_chunks,
                                                           const unsigned long long *__restrict__ cnt, const EncodedVec *__restrict__ desc,
                                                           const uint64_t *__restrict__ word_off, uint32_t *__restrict__ arena) {
    __shared__ unsigned long long wave_tot[4];
    __shared__ uint64_t range[2];
    const uint64_t chunk = blockIdx.x, base = chunk * CH, e0 = base + (uint64_t)threadIdx.x * PER_T;
    uint32_t val[PER_T];
    unsigned long long total;
    unsigned long long run = chunk_prefix(values, nnz, e0, val, wave_tot, total);
    if ((total & 0xFFFFull) == 0) return; // nothing in the chunk reaches even the smallest marker (the same for every lane)
    block_owner_range(indptr, n_outer, base, std::min<uint64_t>(base + CH, nnz) - 1, range);
    if (e0 >= nnz) return;
    uint64_t o = owner_of(indptr, range[0], range[1], e0), end = indptr[o + 1];
    EncodedVec d = desc[o];
#pragma unroll
    for (uint32_t q = 0; q < PER_T; q++) {
        const uint64_t e = e0 + q;
        if (e >= nnz) break;
        if (val[q] >= 7u) {
            if (e >= end) { // (looked up only where a value can matter: most entries are below every marker)
                o = owner_of(indptr, o, range[1], e);
                end = indptr[o + 1];
                d = desc[o];
            }
            const uint32_t w = adaptive::width_of(d.kind);
            if (d.kind != adaptive::V && val[q] >= adaptive::marker_of(w)) {
                const uint64_t rank = cnt[(uint64_t)w * (n_chunks + 1) + chunk] + field16(run, w) - d.fb_base;
                const uint64_t dst = word_off[o] + rank;
                arena[dst] = adaptive::is_dense(d.kind) ? indices[e] : (uint32_t)(e - indptr[o]);
                arena[dst + d.n_fb] = val[q];
            }
        }
        run += pack_over(val[q]);
    }
}

// A launch holds fewer than 2^32 threads: at most 2^24 - 1 blocks of 256 (34e9 stored entries, a 32 GB byte arena, a 16 GB word arena)
constexpr uint64_t MAX_BLOCKS = 0xFFFFFFull;

// in place on the stream, no wait: d[0 .. count) -> its exclusive prefix sums. tmp is shared by the scans of one call
void scan_in_place(hipStream_t s, DevBuf<char> &tmp, unsigned long long *d, uint64_t count) {
    size_t bytes = tmp.n;
    SCANRS_HIP(rocprim::exclusive_scan(tmp.p, bytes, d, d, 0ull, (size_t)count, rocprim::plus<unsigned long long>(), s));
}
size_t scan_temp_bytes(uint64_t count) {
    size_t bytes = 0;
    SCANRS_HIP(rocprim::exclusive_scan(nullptr, bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, 0ull, (size_t)count,
                                       rocprim::plus<unsigned long long>(), (hipStream_t) nullptr));
    return std::max<size_t>(bytes, 16);
}

} // namespace

// Encodes cp's outer vectors (force_kind -1: choose_storage; 0..7: that encoding for all). The per-vector table and the offsets
// (n_outer + 1 entries each; bytes / 32-bit words) come back to the host; the arenas stay on the device for the caller to fetch.
void encode_adaptive_vectors(Storage &st, const SparseCopy &cp, int force_kind, std::vector<EncodedVec> &vecs, std::vector<uint64_t> &byte_off,
                             std::vector<uint64_t> &word_off, DevBuf<uint64_t> &d_bytes, DevBuf<uint32_t> &d_words) {
    hipStream_t s = st.stream;
    const uint64_t no = cp.n_outer, nnz = cp.nnz, n_chunks = (nnz + CH - 1) / CH;
    if (n_chunks > MAX_BLOCKS || no > MAX_BLOCKS * 256ull) fail(SCANRS_ERR_SHAPE, "matrix too large for the encoders");
    // chunk_prefix reads `values` with 16-byte loads, up to 7 entries past nnz (the contract of SparseCopy in common.hpp)
    static_assert(DevBuf<uint32_t>::SLACK >= 8 * sizeof(uint32_t), "the slack behind a copy's arrays covers the last load of a chunk");
    if (reinterpret_cast<uintptr_t>(cp.values.p) % 16u) fail(SCANRS_ERR_ARGUMENT, "internal: the values of a copy must start on a 16-byte boundary");
    vecs.assign(no, EncodedVec{});
    byte_off.assign(no + 1, 0);
    word_off.assign(no + 1, 0);
    if (!no) return;
    DevBuf<unsigned long long> cnt(4 * (n_chunks + 1)), part(no + 1), bsz(no + 1), wsz(no + 1);
    DevBuf<EncodedVec> desc(no);
    DevBuf<char> tmp(scan_temp_bytes(std::max<uint64_t>(cnt.n, no + 1))); // (lives until the wait below)
    if (st.prof.on) st.prof.begin(s, "encode_plan", (double)nnz * 4.0 + (double)no * 56.0);
    SCANRS_HIP(hipMemsetAsync(cnt.p, 0, cnt.n * 8, s));
    SCANRS_HIP(hipMemsetAsync(part.p, 0, part.n * 8, s));
    SCANRS_HIP(hipMemsetAsync(bsz.p, 0, bsz.n * 8, s));
    SCANRS_HIP(hipMemsetAsync(wsz.p, 0, wsz.n * 8, s));
    if (n_chunks) {
        hipLaunchKernelGGL(enc_count_kernel, dim3((unsigned)n_chunks), dim3(256), 0, s, cp.indptr.p, no, cp.values.p, nnz, n_chunks, cnt.p, part.p);
        // one scan over the four arrays of chunk counts (each ends with a spare zero): array w then starts at the total of the
        // arrays before it, a constant that drops out wherever P_w is used, which is always as a difference of two of its values
        scan_in_place(s, tmp, cnt.p, cnt.n);
    }
    hipLaunchKernelGGL(enc_plan_kernel, grid1(no, 256), dim3(256), 0, s, cp.indptr.p, no, cp.n_inner, n_chunks, cnt.p, part.p, force_kind, desc.p, bsz.p,
                       wsz.p);
    SCANRS_HIP(hipGetLastError());
    scan_in_place(s, tmp, bsz.p, no + 1);
    scan_in_place(s, tmp, wsz.p, no + 1);
    if (st.prof.on) st.prof.end(s);
    SCANRS_D2H(vecs.data(), desc.p, no * sizeof(EncodedVec), s);
    SCANRS_D2H(byte_off.data(), bsz.p, (no + 1) * 8, s);
    SCANRS_D2H(word_off.data(), wsz.p, (no + 1) * 8, s);
    SCANRS_SYNC(s);
    const uint64_t n_bytes = byte_off[no], n_words = word_off[no];
    if (n_words > MAX_BLOCKS * 256ull || n_bytes / 8 > MAX_BLOCKS * 256ull) fail(SCANRS_ERR_SHAPE, "encoded matrix too large for the encoders");
    d_bytes.alloc(std::max<uint64_t>(1, n_bytes / 8));
    d_words.alloc(std::max<uint64_t>(1, n_words));
    if (st.prof.on) st.prof.begin(s, "encode_emit", (double)nnz * 8.0 + (double)n_bytes + (double)n_words * 4.0);
    const uint64_t *boff = reinterpret_cast<const uint64_t *>(bsz.p), *woff = reinterpret_cast<const uint64_t *>(wsz.p);
    if (n_bytes)
        hipLaunchKernelGGL(enc_bytes_kernel, grid1(n_bytes / 8, 256), dim3(256), 0, s, cp.indptr.p, cp.indices.p, cp.values.p, no, cp.n_inner, desc.p, boff,
                           n_bytes / 8, d_bytes.p);
    if (n_words) {
        hipLaunchKernelGGL(enc_words_kernel, grid1(n_words, 256), dim3(256), 0, s, cp.indptr.p, cp.indices.p, cp.values.p, no, cp.n_inner, desc.p, woff,
                           n_words, d_words.p);
        if (n_chunks)
            hipLaunchKernelGGL(enc_fallback_kernel, dim3((unsigned)n_chunks), dim3(256), 0, s, cp.indptr.p, cp.indices.p, cp.values.p, no, nnz, n_chunks,
                               cnt.p, desc.p, woff, d_words.p);
    }
    SCANRS_HIP(hipGetLastError());
    if (st.prof.on) st.prof.end(s);
    SCANRS_SYNC(s); // the plan's buffers are released on return
}

} // namespace scanrs
