// export_multi.hip — the device side of scanrs_multi_to_adaptive with major = SCANRS_EXPORT_INNER (multi.cpp): a
// destination assembles the CSR of its slab of INNER positions over all outer positions of the whole matrix, out of the source shards'
// transposed copies, read in place (its own device's memory, or a peer's through the peer mapping). Vector g of the result is the
// concatenation over the sources s = 0, 1, ... of vector g of T_s with every index raised by the source's outer_begin: the shards hold
// contiguous ascending ranges, so the result ascends. Integer work only; no atomics; every output element is written once, by a lane
// that the plan alone determines (element e of a slab belongs to tile e / REGATHER_TILE, lane e % 256 of that tile's workgroup),
// whatever the launch geometry. All offsets are 64-bit: a slab may hold more than 2^32 entries.
#include "common.hpp"

namespace scanrs {

namespace {

constexpr uint32_t TILE_THREADS = 256, TILE_ITEMS = 8;
static_assert(TILE_THREADS * TILE_ITEMS == REGATHER_TILE, "a workgroup owns one tile of the output");

// the stored entries source s holds of inner position g (0 where its indptr is not what the plan saw: every read stays inside nnz[s])
__device__ inline uint64_t source_count(const RegatherSources &src, uint32_t s, uint64_t g) {
    const uint64_t a = src.indptr[s][g], b = src.indptr[s][g + 1];
    return (b >= a && b <= src.nnz[s]) ? b - a : 0;
}

// A lane per slab vector j (inner position g0 + j): its length over all sources. len has n_vec + 1 entries (select_scan_offsets turns
// them into the slab's indptr in place).
__global__ __launch_bounds__(256) void export_len_kernel(RegatherSources src, uint64_t g0, uint64_t n_vec, unsigned long long *__restrict__ len) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n_vec) return;
    unsigned long long n = 0;
    if (j < n_vec)
        for (uint32_t s = 0; s < src.n; s++) n += source_count(src, s, g0 + j);
    len[j] = n; // (j == n_vec: the spare entry of the scan)
}

// A lane per slab vector j: start[s * n_vec + j] = where source s's piece of the vector begins in the slab,
// indptr[j] + the counts of the sources before s; row n_src is the vector's end.
__global__ __launch_bounds__(256) void export_start_kernel(RegatherSources src, uint64_t g0, uint64_t n_vec, const uint64_t *__restrict__ indptr,
                                                           uint64_t *__restrict__ start) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_vec) return;
    uint64_t at = indptr[j];
    for (uint32_t s = 0; s < src.n; s++) {
        start[(uint64_t)s * n_vec + j] = at;
        at += source_count(src, s, g0 + j);
    }
    start[(uint64_t)src.n * n_vec + j] = at;
}

// the slab vector that holds element e: the last v in [lo, hi] with indptr[v] <= e (indptr[lo] <= e < indptr[hi + 1])
__device__ inline uint64_t vector_of(const uint64_t *__restrict__ indptr, uint64_t lo, uint64_t hi, uint64_t e) {
    while (lo < hi) {
        const uint64_t m = lo + ((hi - lo + 1) >> 1);
        if (indptr[m] <= e)
            lo = m;
        else
            hi = m - 1;
    }
    return lo;
}

// A workgroup per tile of REGATHER_TILE consecutive slab elements, as regather_pull_kernel: the tile's first and last vector from two
// searches that are the same in every lane, then one search per element between the two, and a scan over the (at most 16) rows of the
// start table for the source that holds it. Lane i takes elements i, i + 256, ...: the stores are coalesced, and so are the loads
// inside a source's piece of a vector.
__global__ __launch_bounds__(256) void export_pull_kernel(RegatherSources src, uint64_t g0, const uint64_t *__restrict__ indptr,
                                                          const uint64_t *__restrict__ start, uint64_t n_vec, uint64_t nnz, uint64_t outer_global,
                                                          uint32_t *__restrict__ out_idx, uint32_t *__restrict__ out_val) {
    const uint64_t base = (uint64_t)blockIdx.x * REGATHER_TILE;
    if (base >= nnz || n_vec == 0) return;
    const uint64_t last = (nnz - base < REGATHER_TILE ? nnz : base + REGATHER_TILE) - 1;
    const uint64_t v_lo = vector_of(indptr, 0, n_vec - 1, base);
    const uint64_t v_hi = vector_of(indptr, v_lo, n_vec - 1, last);
#pragma unroll
    for (uint32_t k = 0; k < TILE_ITEMS; k++) {
        const uint64_t e = base + (uint64_t)k * TILE_THREADS + threadIdx.x;
        if (e > last) continue;
        const uint64_t v = v_lo == v_hi ? v_lo : vector_of(indptr, v_lo, v_hi, e);
        uint32_t s = 0; // the last source whose piece begins at or before e (empty pieces repeat a start)
        for (uint32_t t = 1; t < src.n; t++)
            if (start[(uint64_t)t * n_vec + v] <= e) s = t;
        const uint64_t first = start[(uint64_t)s * n_vec + v];
        uint64_t j = 0;
        uint32_t x = 0;
        if (e >= first && e < start[(uint64_t)(s + 1) * n_vec + v]) { // (always: the table came from the same indptr arrays)
            const uint64_t at = src.indptr[s][g0 + v] + (e - first);
            if (at < src.nnz[s]) {
                j = (uint64_t)src.indices[s][at] + src.bounds[s];
                x = src.values[s][at];
            }
        }
        if (j >= outer_global) j = 0, x = 0; // (never: a shard's indices lie below its own extent) the encoders index by j
        out_idx[e] = (uint32_t)j;
        out_val[e] = x;
    }
}

uint64_t per_vector_blocks(uint64_t n_vec) {
    const uint64_t blocks = (n_vec + 1 + 255) / 256;
    if (blocks * 256 >= (1ull << 32)) fail(SCANRS_ERR_DEVICE, "a per-vector launch over %llu vectors exceeds the 2^32 work-items of one dispatch", (unsigned long long)n_vec);
    return blocks;
}

} // namespace

void launch_export_len(hipStream_t s, const RegatherSources &src, uint64_t g0, uint64_t n_vec, unsigned long long *d_len) {
    hipLaunchKernelGGL(export_len_kernel, dim3((unsigned)per_vector_blocks(n_vec)), dim3(256), 0, s, src, g0, n_vec, d_len);
    SCANRS_HIP(hipGetLastError());
}

void launch_export_start(hipStream_t s, const RegatherSources &src, uint64_t g0, uint64_t n_vec, const uint64_t *d_indptr, uint64_t *d_start) {
    if (!n_vec) return;
    hipLaunchKernelGGL(export_start_kernel, dim3((unsigned)per_vector_blocks(n_vec)), dim3(256), 0, s, src, g0, n_vec, d_indptr, d_start);
    SCANRS_HIP(hipGetLastError());
}

void launch_export_pull(hipStream_t s, const RegatherSources &src, uint64_t g0, const uint64_t *d_indptr, const uint64_t *d_start, uint64_t n_vec,
                        uint64_t nnz, uint64_t outer_global, uint32_t *d_out_idx, uint32_t *d_out_val) {
    if (!nnz || !n_vec) return;
    const uint64_t tiles = (nnz + REGATHER_TILE - 1) / REGATHER_TILE;
    if (tiles >= (1ull << 31)) fail(SCANRS_ERR_DEVICE, "%llu nonzeros in one export slab need more tiles than one dispatch has workgroups", (unsigned long long)nnz);
    hipLaunchKernelGGL(export_pull_kernel, dim3((unsigned)tiles), dim3(TILE_THREADS), 0, s, src, g0, d_indptr, d_start, n_vec, nnz, outer_global, d_out_idx,
                       d_out_val);
    SCANRS_HIP(hipGetLastError());
}

} // namespace scanrs
