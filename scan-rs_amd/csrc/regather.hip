// regather.hip — the device side of scanrs_multi_gather_outer / scanrs_multi_rebalance (multi.cpp): a destination shard
// pulls its outer vectors out of the source shards' arrays, in place (its own device's memory, or a peer's through the peer mapping).
// Integer work only; no atomics; every output element is written once, by a lane that the plan alone determines (output element e of
// a destination belongs to tile e / REGATHER_TILE, lane e % 256 of that tile's workgroup), whatever the launch geometry.
#include "common.hpp"

namespace scanrs {

namespace {

constexpr uint32_t TILE_THREADS = 256, TILE_ITEMS = 8;
static_assert(TILE_THREADS * TILE_ITEMS == REGATHER_TILE, "a workgroup owns one tile of the output");
constexpr int SHARD_SHIFT = 60; // a source place: the shard in the top 4 bits (at most 16 sources), the offset in its arrays below
constexpr uint64_t OFFSET_MASK = (1ull << SHARD_SHIFT) - 1ull;

// A lane per output vector j: its source shard (the one whose range holds list[j]), its length, and where it begins in that shard's
// arrays. len has n_vec + 1 entries (select_scan_offsets turns them into the destination's indptr in place).
__global__ __launch_bounds__(256) void regather_len_kernel(RegatherSources src, const uint32_t *__restrict__ list, uint64_t n_vec,
                                                           unsigned long long *__restrict__ len, uint64_t *__restrict__ place) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n_vec) return;
    if (j == n_vec) { // the spare entry of the scan
        len[j] = 0;
        return;
    }
    const uint64_t g = list[j];
    uint32_t s = 0; // the last shard whose range begins at or before g and is not empty there (empty ranges repeat a bound)
    for (uint32_t t = 1; t < src.n; t++)
        if (src.bounds[t] <= g) s = t;
    unsigned long long n = 0;
    uint64_t a = 0;
    if (g >= src.bounds[s] && g < src.bounds[s + 1]) { // (always: the list was checked against the outer extent on the host)
        const uint64_t *ip = src.indptr[s] + (g - src.bounds[s]);
        a = ip[0];
        const uint64_t b = ip[1];
        if (b >= a && b <= src.nnz[s]) n = b - a;
    }
    len[j] = n;
    place[j] = ((uint64_t)s << SHARD_SHIFT) | a;
}

// the output vector that holds element e: the last v in [lo, hi] with indptr[v] <= e (indptr[lo] <= e < indptr[hi + 1])
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

// A workgroup per tile of REGATHER_TILE consecutive output elements. The tile's first and last vector come from two searches over the
// whole indptr (the same in every lane: the addresses depend on the block alone); a lane then places each of its elements by a search
// between the two, so the work of a tile is bounded by log2 of the vectors it touches however the nonzeros are spread: one vector
// over many tiles costs no search, a run of empty vectors is stepped over by the search. Lane i takes elements i, i + 256, ...: the
// stores are coalesced, and so are the loads inside a source vector.
__global__ __launch_bounds__(256) void regather_pull_kernel(RegatherSources src, const uint64_t *__restrict__ indptr, const uint64_t *__restrict__ place,
                                                            uint64_t n_vec, uint64_t nnz, uint32_t *__restrict__ out_idx, uint32_t *__restrict__ out_val) {
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
        const uint64_t p = place[v];
        const uint32_t s = (uint32_t)(p >> SHARD_SHIFT);
        const uint64_t at = (p & OFFSET_MASK) + (e - indptr[v]);
        uint32_t j = 0, x = 0;
        if (s < src.n && at < src.nnz[s]) { // (always: the lengths came from the same indptr arrays)
            j = src.indices[s][at];
            x = src.values[s][at];
        }
        out_idx[e] = j;
        out_val[e] = x;
    }
}

} // namespace

void launch_regather_len(hipStream_t s, const RegatherSources &src, const uint32_t *d_list, uint64_t n_vec, unsigned long long *d_len, uint64_t *d_place) {
    const uint64_t blocks = (n_vec + 1 + 255) / 256;
    if (blocks * 256 >= (1ull << 32)) fail(SCANRS_ERR_DEVICE, "a per-element launch over %llu elements exceeds the 2^32 work-items of one dispatch", (unsigned long long)n_vec);
    hipLaunchKernelGGL(regather_len_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, d_list, n_vec, d_len, d_place);
    SCANRS_HIP(hipGetLastError());
}

void launch_regather_pull(hipStream_t s, const RegatherSources &src, const uint64_t *d_indptr, const uint64_t *d_place, uint64_t n_vec, uint64_t nnz,
                          uint32_t *d_out_idx, uint32_t *d_out_val) {
    if (!nnz || !n_vec) return;
    const uint64_t tiles = (nnz + REGATHER_TILE - 1) / REGATHER_TILE;
    if (tiles >= (1ull << 31)) fail(SCANRS_ERR_DEVICE, "%llu nonzeros in one shard need more tiles than one dispatch has workgroups", (unsigned long long)nnz);
    hipLaunchKernelGGL(regather_pull_kernel, dim3((unsigned)tiles), dim3(TILE_THREADS), 0, s, src, d_indptr, d_place, n_vec, nnz, d_out_idx, d_out_val);
    SCANRS_HIP(hipGetLastError());
}

} // namespace scanrs
