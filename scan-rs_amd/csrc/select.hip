// HIP kernels of select_rows / select_cols / partition_on_thresholds (sqz/src/mat.rs:730-888, 1004-1071) + their launchers.
// Host logic: select_host.cpp. Everything here is integer work on the raw counts of ONE compressed copy (the handle's own storage:
// no transposition is built), so every result is defined bit for bit.
//
//   sel_outer_sums_kernel     masked sums of the outer vectors: a wave per vector, u64, entries at excluded inner positions left out
//   sel_inner_sums_kernel     masked sums per inner position: the vectors picked by a byte mask are added to (or taken from) u64
//                             sums with 64-bit integer atomics. Round 1 of a partition adds every vector; later rounds subtract the
//                             vectors that have just been excluded (integers: exactly the sums of a full masked pass)
//   sel_mark_kernel           sum < threshold -> excluded, newly excluded, and the round's one flag
//   part_count_kernel         per outer vector the length of its part in the filtered and in the residual matrix, one walk
//   part_fill_kernel          remapped indices and values of both matrices, one walk (order kept: ranks from wave ballots)
//   gather_len / gather_copy  outer-axis selection: lengths of the picked vectors, then a segment copy (16 B per lane)
//   expand_count / _fill      inner-axis selection: a nonzero at source position j is emitted once per position p with idx[p] == j
//                             (the inverse list), with new index p
//
// A wave reads a vector in aligned 16-byte pieces per lane (4 indices, 4 counts): the walk starts at the vector's start rounded down
// to a multiple of 4 and masks what lies outside [start, end) — every buffer of a copy has slack behind its end (DevBuf::SLACK).
#include "common.hpp"
#include "launch_util.hpp"

#include <rocprim/rocprim.hpp>

namespace scanrs {

namespace {
constexpr int WAVES_PER_BLOCK = 4;
inline dim3 wave_grid(uint64_t n_vec) { return dim3((unsigned)((n_vec + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK)); }

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t lanes_below(unsigned long long ballot, int lane) { return (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull)); }
__device__ __forceinline__ uint32_t elem(const uint4 &v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
} // namespace

// ---- masked sums -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sel_outer_sums_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                             const uint32_t *__restrict__ values, uint64_t n_outer,
                                                             const uint8_t *__restrict__ excl_outer, const uint8_t *__restrict__ excl_inner,
                                                             unsigned long long *__restrict__ out) {
    const uint64_t o = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (o >= n_outer) return;
    unsigned long long acc = 0;
    if (!excl_outer[o]) {
        const uint64_t a = indptr[o], b = indptr[o + 1];
        for (uint64_t e = (a & ~3ull) + (uint64_t)lane * 4u; e < b; e += 256u) {
            const uint4 i4 = *reinterpret_cast<const uint4 *>(indices + e);
            const uint4 v4 = *reinterpret_cast<const uint4 *>(values + e);
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (e + k >= a && e + k < b && !excl_inner[elem(i4, k)]) acc += elem(v4, k);
        }
        acc = wave_sum_u64(acc);
    }
    if (lane == 0) out[o] = acc;
}

// sums[j] += (or -=) the counts at inner position j of every outer vector o with pick[o] == want
__global__ __launch_bounds__(256) void sel_inner_sums_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                             const uint32_t *__restrict__ values, uint64_t n_outer,
                                                             const uint8_t *__restrict__ pick, uint8_t want, int subtract,
                                                             const uint8_t *__restrict__ excl_inner, unsigned long long *__restrict__ sums) {
    const uint64_t o = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (o >= n_outer || pick[o] != want) return;
    const uint64_t a = indptr[o], b = indptr[o + 1];
    for (uint64_t e = (a & ~3ull) + (uint64_t)lane * 4u; e < b; e += 256u) {
        const uint4 i4 = *reinterpret_cast<const uint4 *>(indices + e);
        const uint4 v4 = *reinterpret_cast<const uint4 *>(values + e);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (e + k < a || e + k >= b) continue;
            const uint32_t j = elem(i4, k);
            if (excl_inner[j]) continue; // the sum of an excluded position is never looked at again
            const unsigned long long x = elem(v4, k);
            atomicAdd(&sums[j], subtract ? 0ull - x : x); // (two's complement: exact)
        }
    }
}

__global__ __launch_bounds__(256) void sel_mark_kernel(const unsigned long long *__restrict__ sums, uint64_t n, double threshold,
                                                       uint8_t *__restrict__ excl, uint8_t *__restrict__ newly, uint32_t *__restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || excl[i]) return;
    if ((double)sums[i] < threshold) { // (a NaN threshold excludes nothing)
        excl[i] = 1;
        newly[i] = 1;
        *flag = 1u;
    }
}

// ---- the two matrices of a partition ---------------------------------------------------------------------------------------------
// pos_a[o] / pos_b[o]: the outer position of vector o in the filtered / residual matrix, or -1. remap[j] >= 0: inner position j is
// kept, with that new index; < 0: excluded, ~remap[j] is its rank among the excluded ones. cols_inner: the residual holds the
// excluded INNER positions of the kept vectors; else the kept inner positions of the excluded vectors.
__global__ __launch_bounds__(256) void part_count_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices, uint64_t n_outer,
                                                         const int32_t *__restrict__ pos_a, const int32_t *__restrict__ pos_b,
                                                         const int32_t *__restrict__ remap, int cols_inner, unsigned long long *__restrict__ len_a,
                                                         unsigned long long *__restrict__ len_b) {
    const uint64_t o = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (o >= n_outer) return;
    const int32_t pa = pos_a[o], pb = pos_b[o];
    if (pa < 0 && pb < 0) return;
    const uint64_t a = indptr[o], b = indptr[o + 1];
    unsigned long long kept = 0, excl = 0;
    for (uint64_t e = (a & ~3ull) + (uint64_t)lane * 4u; e < b; e += 256u) {
        const uint4 i4 = *reinterpret_cast<const uint4 *>(indices + e);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (e + k >= a && e + k < b) {
                if (remap[elem(i4, k)] >= 0)
                    kept++;
                else
                    excl++;
            }
    }
    kept = wave_sum_u64(kept);
    excl = wave_sum_u64(excl);
    if (lane == 0) {
        if (pa >= 0) len_a[pa] = kept;
        if (pb >= 0) len_b[pb] = cols_inner ? excl : kept;
    }
}

__global__ __launch_bounds__(256) void part_fill_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                        const uint32_t *__restrict__ values, uint64_t n_outer, const int32_t *__restrict__ pos_a,
                                                        const int32_t *__restrict__ pos_b, const int32_t *__restrict__ remap, int cols_inner,
                                                        const uint64_t *__restrict__ ip_a, uint32_t *__restrict__ idx_a, uint32_t *__restrict__ val_a,
                                                        const uint64_t *__restrict__ ip_b, uint32_t *__restrict__ idx_b, uint32_t *__restrict__ val_b) {
    const uint64_t o = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (o >= n_outer) return;
    const int32_t pa = pos_a[o], pb = pos_b[o];
    if (pa < 0 && pb < 0) return;
    const uint64_t a = indptr[o], b = indptr[o + 1];
    uint64_t wa = pa >= 0 ? ip_a[pa] : 0, wb = pb >= 0 ? ip_b[pb] : 0; // next free place of this vector in each output
    for (uint64_t base = a & ~3ull; base < b; base += 256u) {           // (wave-uniform trip count: ballots inside)
        const uint64_t e = base + (uint64_t)lane * 4u;
        uint4 i4 = make_uint4(0, 0, 0, 0), v4 = make_uint4(0, 0, 0, 0);
        if (e < b) {
            i4 = *reinterpret_cast<const uint4 *>(indices + e);
            v4 = *reinterpret_cast<const uint4 *>(values + e);
        }
        bool in_a[4], in_b[4];
        int32_t r[4];
        uint32_t mine_a = 0, mine_b = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool valid = e + k >= a && e + k < b;
            r[k] = valid ? remap[elem(i4, k)] : 0;
            in_a[k] = valid && pa >= 0 && r[k] >= 0;
            in_b[k] = valid && pb >= 0 && (cols_inner ? r[k] < 0 : r[k] >= 0);
            mine_a += in_a[k];
            mine_b += in_b[k];
        }
        // rank of this lane's first element among the wave's: the lanes below hold the lower source positions
        uint32_t before_a = 0, before_b = 0, total_a = 0, total_b = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned long long ba = __ballot(in_a[k]), bb = __ballot(in_b[k]);
            before_a += lanes_below(ba, lane);
            before_b += lanes_below(bb, lane);
            total_a += (uint32_t)__popcll(ba);
            total_b += (uint32_t)__popcll(bb);
        }
        uint64_t qa = wa + before_a, qb = wb + before_b;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (in_a[k]) {
                idx_a[qa] = (uint32_t)r[k];
                val_a[qa] = elem(v4, k);
                qa++;
            }
            if (in_b[k]) {
                idx_b[qb] = (uint32_t)(cols_inner ? ~r[k] : r[k]);
                val_b[qb] = elem(v4, k);
                qb++;
            }
        }
        wa += total_a;
        wb += total_b;
    }
}

// ---- outer-axis selection: gather of whole vectors -----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_len_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ idx, uint64_t n_idx,
                                                         unsigned long long *__restrict__ len) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_idx) len[i] = indptr[idx[i] + 1ull] - indptr[idx[i]];
}

namespace {
struct __attribute__((packed, aligned(4))) U4Unaligned { // a 16-byte load from a 4-byte aligned address
    uint32_t x, y, z, w;
};
// dst[0 .. n) = src[0 .. n) by one wave: 16-byte stores to aligned places of dst, the source read as it lies
__device__ __forceinline__ void wave_copy_u32(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, uint64_t n, int lane) {
    uint64_t head = ((16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / 4u;
    if (head > n) head = n;
    if ((uint64_t)lane < head) dst[lane] = src[lane];
    const uint64_t n4 = (n - head) / 4u;
    uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
    const U4Unaligned *s4 = reinterpret_cast<const U4Unaligned *>(src + head);
    for (uint64_t i = lane; i < n4; i += 64u) {
        const U4Unaligned v = s4[i];
        d4[i] = make_uint4(v.x, v.y, v.z, v.w);
    }
    const uint64_t done = head + n4 * 4u;
    if (done + lane < n) dst[done + lane] = src[done + lane];
}
} // namespace

__global__ __launch_bounds__(256) void gather_copy_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                          const uint32_t *__restrict__ values, const uint32_t *__restrict__ idx, uint64_t n_idx,
                                                          const uint64_t *__restrict__ ip_out, uint32_t *__restrict__ idx_out,
                                                          uint32_t *__restrict__ val_out) {
    const uint64_t i = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n_idx) return;
    const uint64_t a = indptr[idx[i]], n = indptr[idx[i] + 1ull] - a, w = ip_out[i];
    wave_copy_u32(idx_out + w, indices + a, n, lane);
    wave_copy_u32(val_out + w, values + a, n, lane);
}

// ---- inner-axis selection: expansion through the inverse list --------------------------------------------------------------------
// inv_ptr (n_inner + 1) / inv_pos: the positions p with idx[p] == j, ascending, for every source position j
__global__ __launch_bounds__(256) void expand_count_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices, uint64_t n_outer,
                                                           const uint32_t *__restrict__ inv_ptr, unsigned long long *__restrict__ len) {
    const uint64_t o = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (o >= n_outer) return;
    const uint64_t a = indptr[o], b = indptr[o + 1];
    unsigned long long acc = 0;
    for (uint64_t e = (a & ~3ull) + (uint64_t)lane * 4u; e < b; e += 256u) {
        const uint4 i4 = *reinterpret_cast<const uint4 *>(indices + e);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (e + k >= a && e + k < b) {
                const uint32_t j = elem(i4, k);
                acc += inv_ptr[j + 1u] - inv_ptr[j];
            }
    }
    acc = wave_sum_u64(acc);
    if (lane == 0) len[o] = acc;
}

__global__ __launch_bounds__(256) void expand_fill_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                          const uint32_t *__restrict__ values, uint64_t n_outer, const uint32_t *__restrict__ inv_ptr,
                                                          const uint32_t *__restrict__ inv_pos, const uint64_t *__restrict__ ip_out,
                                                          uint32_t *__restrict__ idx_out, uint32_t *__restrict__ val_out) {
    const uint64_t o = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (o >= n_outer) return;
    const uint64_t a = indptr[o], b = indptr[o + 1];
    uint64_t w = ip_out[o];
    for (uint64_t base = a; base < b; base += 64u) { // (wave-uniform trip count: a scan over the lanes inside)
        const uint64_t e = base + lane;
        uint32_t first = 0, m = 0, x = 0;
        if (e < b) {
            const uint32_t j = indices[e];
            first = inv_ptr[j];
            m = inv_ptr[j + 1u] - first;
            x = values[e];
        }
        uint32_t incl = m; // inclusive scan of the multiplicities over the lanes
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        const uint32_t total = __shfl(incl, 63, 64);
        uint64_t q = w + (incl - m);
        for (uint32_t t = 0; t < m; t++, q++) {
            idx_out[q] = inv_pos[first + t];
            val_out[q] = x;
        }
        w += total;
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
void launch_sel_outer_sums(hipStream_t s, const SparseCopy &cp, const uint8_t *excl_outer, const uint8_t *excl_inner, unsigned long long *out) {
    if (!cp.n_outer) return;
    hipLaunchKernelGGL(sel_outer_sums_kernel, wave_grid(cp.n_outer), dim3(256), 0, s, cp.indptr.p, cp.indices.p, cp.values.p, cp.n_outer, excl_outer,
                       excl_inner, out);
    SCANRS_HIP(hipGetLastError());
}
void launch_sel_inner_sums(hipStream_t s, const SparseCopy &cp, const uint8_t *pick, uint8_t want, bool subtract, const uint8_t *excl_inner,
                           unsigned long long *sums) {
    if (!cp.n_outer) return;
    hipLaunchKernelGGL(sel_inner_sums_kernel, wave_grid(cp.n_outer), dim3(256), 0, s, cp.indptr.p, cp.indices.p, cp.values.p, cp.n_outer, pick, want,
                       subtract ? 1 : 0, excl_inner, sums);
    SCANRS_HIP(hipGetLastError());
}
void launch_sel_mark(hipStream_t s, const unsigned long long *sums, uint64_t n, double threshold, uint8_t *excl, uint8_t *newly, uint32_t *flag) {
    if (!n) return;
    hipLaunchKernelGGL(sel_mark_kernel, grid1(n, 256), dim3(256), 0, s, sums, n, threshold, excl, newly, flag);
    SCANRS_HIP(hipGetLastError());
}

// in place: lengths (n entries followed by one unused entry) -> offsets, the total in entry n
void select_scan_offsets(hipStream_t s, unsigned long long *d, uint64_t n) {
    size_t tmp_bytes = 0;
    SCANRS_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, d, d, 0ull, (size_t)n + 1, rocprim::plus<unsigned long long>(), s));
    DevBuf<char> tmp(std::max<size_t>(tmp_bytes, 16));
    SCANRS_HIP(rocprim::exclusive_scan(tmp.p, tmp_bytes, d, d, 0ull, (size_t)n + 1, rocprim::plus<unsigned long long>(), s));
    SCANRS_SYNC(s); // the temporary is released on return
}

void launch_part_count(hipStream_t s, const SparseCopy &cp, const int32_t *pos_a, const int32_t *pos_b, const int32_t *remap, bool cols_inner,
                       unsigned long long *len_a, unsigned long long *len_b) {
    if (!cp.n_outer) return;
    hipLaunchKernelGGL(part_count_kernel, wave_grid(cp.n_outer), dim3(256), 0, s, cp.indptr.p, cp.indices.p, cp.n_outer, pos_a, pos_b, remap,
                       cols_inner ? 1 : 0, len_a, len_b);
    SCANRS_HIP(hipGetLastError());
}
void launch_part_fill(hipStream_t s, const SparseCopy &cp, const int32_t *pos_a, const int32_t *pos_b, const int32_t *remap, bool cols_inner,
                      const uint64_t *ip_a, uint32_t *idx_a, uint32_t *val_a, const uint64_t *ip_b, uint32_t *idx_b, uint32_t *val_b) {
    if (!cp.n_outer) return;
    hipLaunchKernelGGL(part_fill_kernel, wave_grid(cp.n_outer), dim3(256), 0, s, cp.indptr.p, cp.indices.p, cp.values.p, cp.n_outer, pos_a, pos_b,
                       remap, cols_inner ? 1 : 0, ip_a, idx_a, val_a, ip_b, idx_b, val_b);
    SCANRS_HIP(hipGetLastError());
}
void launch_gather_len(hipStream_t s, const SparseCopy &cp, const uint32_t *d_idx, uint64_t n_idx, unsigned long long *len) {
    if (!n_idx) return;
    hipLaunchKernelGGL(gather_len_kernel, grid1(n_idx, 256), dim3(256), 0, s, cp.indptr.p, d_idx, n_idx, len);
    SCANRS_HIP(hipGetLastError());
}
void launch_gather_copy(hipStream_t s, const SparseCopy &cp, const uint32_t *d_idx, uint64_t n_idx, const uint64_t *ip_out, uint32_t *idx_out,
                        uint32_t *val_out) {
    if (!n_idx) return;
    hipLaunchKernelGGL(gather_copy_kernel, wave_grid(n_idx), dim3(256), 0, s, cp.indptr.p, cp.indices.p, cp.values.p, d_idx, n_idx, ip_out, idx_out,
                       val_out);
    SCANRS_HIP(hipGetLastError());
}
void launch_expand_count(hipStream_t s, const SparseCopy &cp, const uint32_t *inv_ptr, unsigned long long *len) {
    if (!cp.n_outer) return;
    hipLaunchKernelGGL(expand_count_kernel, wave_grid(cp.n_outer), dim3(256), 0, s, cp.indptr.p, cp.indices.p, cp.n_outer, inv_ptr, len);
    SCANRS_HIP(hipGetLastError());
}
void launch_expand_fill(hipStream_t s, const SparseCopy &cp, const uint32_t *inv_ptr, const uint32_t *inv_pos, const uint64_t *ip_out,
                        uint32_t *idx_out, uint32_t *val_out) {
    if (!cp.n_outer) return;
    hipLaunchKernelGGL(expand_fill_kernel, wave_grid(cp.n_outer), dim3(256), 0, s, cp.indptr.p, cp.indices.p, cp.values.p, cp.n_outer, inv_ptr,
                       inv_pos, ip_out, idx_out, val_out);
    SCANRS_HIP(hipGetLastError());
}

} // namespace scanrs
