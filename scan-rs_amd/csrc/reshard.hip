// reshard.hip — the device side of the inner-sharding constructors (multi.cpp, scanrs_multi_create_inner).
// A slab is a run of outer vectors of the matrix as the caller holds it (genes of a genes x cells CSR matrix); the shards of the
// result own ranges of its INNER positions (cells). Everything here is integer work whose result does not depend on the launch
// geometry: the only atomics are integer additions, and every output element of the gather is written once, by a lane that the data
// alone determines. All four kernels run after the slab has passed validate_copy (indices in range and strictly ascending).
#include "common.hpp"

namespace scanrs {

namespace {

constexpr uint32_t WAVES_PER_BLOCK = 4;
// a wave per vector, strided: the grid is capped, the loop covers the rest
inline dim3 wave_grid_capped(uint64_t n_vec) { return dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_vec + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 65536))); }

// counts[j] += 1 for every stored entry with inner index j (stored zeros too). n_outer fits u32, so a count does.
__global__ __launch_bounds__(256) void reshard_count_kernel(const uint32_t *__restrict__ indices, uint64_t nnz, uint64_t n_inner,
                                                            uint32_t *__restrict__ counts) {
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t j = indices[e];
        if (j < n_inner) atomicAdd(&counts[j], 1u); // (validated before; the test costs nothing and keeps the write in bounds whatever happens)
    }
}

// first position in [a, b) whose index is >= key
__device__ inline uint64_t lower_bound_idx(const uint32_t *__restrict__ indices, uint64_t a, uint64_t b, uint64_t key) {
    while (a < b) {
        const uint64_t m = a + ((b - a) >> 1);
        if ((uint64_t)indices[m] < key)
            a = m + 1;
        else
            b = m;
    }
    return a;
}

// A lane per (vector o, destination d): indices ascend inside a vector, so its entries for d are the run between two lower bounds.
// start[d * n_vec + o], d = 0 .. world: where d's run begins in the slab's arrays (row `world`: where the vector ends);
// moved[d] += the run's length, stored zeros included.
__global__ __launch_bounds__(256) void reshard_split_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices, uint64_t n_vec,
                                                            const uint64_t *__restrict__ bounds, uint32_t world, uint64_t *__restrict__ start,
                                                            unsigned long long *__restrict__ moved) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_vec * world) return;
    const uint64_t o = t / world;
    const uint32_t d = (uint32_t)(t % world);
    const uint64_t a = indptr[o], b = indptr[o + 1];
    const uint64_t lo = d == 0 ? a : lower_bound_idx(indices, a, b, bounds[d]);
    const uint64_t hi = d + 1 == world ? b : lower_bound_idx(indices, lo, b, bounds[d + 1]);
    start[(uint64_t)d * n_vec + o] = lo;
    if (d + 1 == world) start[(uint64_t)world * n_vec + o] = hi;
    if (hi > lo) atomicAdd(&moved[d], (unsigned long long)(hi - lo));
}

// The destination's side of the exchange. It reads a source's slab in place (its own device's memory, or a peer's through the
// peer mapping): `from` / `to` are the rows d and d + 1 of that source's start table.
// len[o] = entries of vector o's run that the result keeps (stored zeros are dropped, as scanrs_mat_create drops them)
__global__ __launch_bounds__(256) void reshard_len_kernel(const uint64_t *__restrict__ from, const uint64_t *__restrict__ to,
                                                          const uint32_t *__restrict__ values, uint64_t n_vec, int has_zeros,
                                                          unsigned long long *__restrict__ len) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_waves = (uint64_t)gridDim.x * WAVES_PER_BLOCK;
    for (uint64_t o = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6); o < n_vec; o += n_waves) {
        const uint64_t a = from[o], b = to[o];
        unsigned long long n = b - a;
        if (has_zeros) {
            n = 0;
            for (uint64_t base = a; base < b; base += 64u) { // wave-uniform trip count
                const uint64_t e = base + lane;
                const bool keep = e < b && values[e] != 0u;
                n += __popcll(__builtin_amdgcn_ballot_w64(keep));
            }
        }
        if (lane == 0) len[o] = n;
    }
}

// copies the kept entries of every run behind out_ptr[o], the index rebased to the destination's range
__global__ __launch_bounds__(256) void reshard_pull_kernel(const uint64_t *__restrict__ from, const uint64_t *__restrict__ to,
                                                           const uint32_t *__restrict__ indices, const uint32_t *__restrict__ values, uint64_t n_vec,
                                                           uint32_t rebase, const uint64_t *__restrict__ out_ptr, uint32_t *__restrict__ out_idx,
                                                           uint32_t *__restrict__ out_val) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_waves = (uint64_t)gridDim.x * WAVES_PER_BLOCK;
    for (uint64_t o = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6); o < n_vec; o += n_waves) {
        const uint64_t a = from[o], b = to[o];
        uint64_t w = out_ptr[o];
        const uint64_t w_end = out_ptr[o + 1];
        for (uint64_t base = a; base < b; base += 64u) { // wave-uniform trip count: a ballot over the lanes inside
            const uint64_t e = base + lane;
            uint32_t j = 0, x = 0;
            if (e < b) {
                j = indices[e];
                x = values[e];
            }
            const bool keep = e < b && x != 0u;
            const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
            const uint64_t at = w + __popcll(mask & ((1ull << lane) - 1ull));
            if (keep && at < w_end) { // (at < w_end always holds: the lengths come from the same values)
                out_idx[at] = j - rebase;
                out_val[at] = x;
            }
            w += __popcll(mask);
        }
    }
}

} // namespace

void launch_reshard_count(hipStream_t s, const SparseCopy &slab, uint32_t *d_counts) {
    if (!slab.nnz || !slab.n_inner) return;
    const unsigned blocks = (unsigned)std::min<uint64_t>((slab.nnz + 255) / 256, 16384);
    hipLaunchKernelGGL(reshard_count_kernel, dim3(blocks), dim3(256), 0, s, slab.indices.p, slab.nnz, slab.n_inner, d_counts);
    SCANRS_HIP(hipGetLastError());
}

void launch_reshard_split(hipStream_t s, const SparseCopy &slab, const uint64_t *d_bounds, uint32_t world, uint64_t *d_start,
                          unsigned long long *d_moved) {
    if (!slab.n_outer || !world) return;
    const uint64_t lanes = slab.n_outer * world, blocks = (lanes + 255) / 256;
    if (blocks * 256 >= (1ull << 32)) fail(SCANRS_ERR_DEVICE, "a per-element launch over %llu elements exceeds the 2^32 work-items of one dispatch", (unsigned long long)lanes);
    hipLaunchKernelGGL(reshard_split_kernel, dim3((unsigned)blocks), dim3(256), 0, s, slab.indptr.p, slab.indices.p, slab.n_outer, d_bounds, world, d_start,
                       d_moved);
    SCANRS_HIP(hipGetLastError());
}

void launch_reshard_len(hipStream_t s, const uint64_t *d_from, const uint64_t *d_to, const uint32_t *d_values, uint64_t n_vec, bool has_zeros,
                        unsigned long long *d_len) {
    if (!n_vec) return;
    hipLaunchKernelGGL(reshard_len_kernel, wave_grid_capped(n_vec), dim3(256), 0, s, d_from, d_to, d_values, n_vec, has_zeros ? 1 : 0, d_len);
    SCANRS_HIP(hipGetLastError());
}

void launch_reshard_pull(hipStream_t s, const uint64_t *d_from, const uint64_t *d_to, const uint32_t *d_indices, const uint32_t *d_values,
                         uint64_t n_vec, uint32_t rebase, const uint64_t *d_out_ptr, uint32_t *d_out_idx, uint32_t *d_out_val) {
    if (!n_vec) return;
    hipLaunchKernelGGL(reshard_pull_kernel, wave_grid_capped(n_vec), dim3(256), 0, s, d_from, d_to, d_indices, d_values, n_vec, rebase, d_out_ptr,
                       d_out_idx, d_out_val);
    SCANRS_HIP(hipGetLastError());
}

} // namespace scanrs
