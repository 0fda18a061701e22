// HIP kernels of the batched pairwise DE with per-pair sSeq parameters (scanrs_sseq_de_pairs) + their launchers. Host logic:
// sseq_pairs_host.cpp. The passes over the nonzeros are the existing ones (sseq_cell_totals_kernel, the fused pass of cluster.hip);
// what runs here turns their sums into every pair's parameters without a copy of the accumulators to the host:
//
//   pairs_gather_kernel        the totals of the labelled cells, group by group (the host's counting sort of the labels gives the order);
//                              rocPRIM's segmented radix sort then orders every group's segment
//   pairs_group_stats_kernel   per group Σ u_c (u64) and Σ 1/u_c over u_c > 0 (128-bit fixed point): integer sums, order-free
//   pairs_header_kernel        one thread per pair: the interpolated median m_S of the union of two sorted segments (the two order
//                              statistics percentile_of_sorted(.., 50) reads, stat.rs:140-162, by binary search), n_S, Σ 1/sf, sf_a, sf_b
//   pairs_moments_kernel       one thread per (gene, pair): 128-bit add of the two groups' accumulators, mean, variance, use_genes and
//                              the method-of-moments dispersion (diff_exp.rs:377-407) through sf_c = u_c / m_S
//   pairs_shrink_kernel        one workgroup per pair: zeta_hat = the interpolated percentile of the used dispersions by radix select
//                              on order-preserving keys (two ranks, integer histograms, as medoid_select_kernel), their mean and the two
//                              sums of squared deviations in a fixed order, delta and gene_phi (diff_exp.rs:409-441)
//   pairs_acc_split / _join    the grouped accumulators of a sharded handle as u64 planes that a sum all-reduce cannot overflow, and
//                              back with the carries propagated; also used by merge_clusters' fused route
//
// No float atomics. A pair's numbers come from its own two groups only, through integer sums and fixed reduction trees: they do not
// depend on the other pairs of the call, on launch timing, or on which copy of the matrix the passes walked.
#include "common.hpp"
#include "fixed128.hpp"

#include <rocprim/rocprim.hpp>

// the parameters restate host arithmetic (cluster_host.cpp's from_sums, sseq_params_from_moments) that is not contracted
#pragma clang fp contract(off)

namespace scanrs {

constexpr uint32_t PAIRS_THREADS = 256;

__global__ __launch_bounds__(256) void pairs_gather_kernel(const unsigned long long *__restrict__ tot, const uint32_t *__restrict__ perm, uint64_t n,
                                                           unsigned long long *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = tot[perm[i]];
}

// block g: the segment [off[g], off[g + 1]) of the grouped totals; stats (zeroed by the launcher) [g * 3] = Σ u, [g * 3 + 1 .. 2] = Σ 1/u
__global__ __launch_bounds__(256) void pairs_group_stats_kernel(const unsigned long long *__restrict__ u, const uint32_t *__restrict__ off, double scale,
                                                                unsigned long long *__restrict__ stats) {
    const uint32_t g = blockIdx.x, lane = threadIdx.x & 63u;
    const uint32_t b = off[g], e = off[g + 1];
    unsigned long long s = 0ull;
    U128 inv{0ull, 0ull};
    for (uint32_t i = b + threadIdx.x; i < e; i += blockDim.x) {
        const unsigned long long v = u[i];
        s += v;
        if (v) add128(inv, to_fixed(1.0 / (double)v, scale));
    }
    for (int o = 32; o > 0; o >>= 1) {
        s += (unsigned long long)__shfl_down((long long)s, o);
        add128(inv, shfl_down128(inv, o));
    }
    if (lane == 0) {
        if (s) atomicAdd(&stats[(uint64_t)g * 3], s);
        if (inv.lo | inv.hi) atomic_add128(&stats[(uint64_t)g * 3 + 1], inv);
    }
}

// the k-th smallest (0-based) of the union of two ascending lists, k < na + nb (cluster_host.cpp's union_median)
__device__ __forceinline__ unsigned long long pairs_kth(const unsigned long long *__restrict__ a, uint64_t na, const unsigned long long *__restrict__ b,
                                                         uint64_t nb, uint64_t k) {
    uint64_t lo = k > nb ? k - nb : 0, hi = k < na ? k : na;
    while (lo < hi) { // the number i of elements taken from a
        const uint64_t i = (lo + hi) / 2, j = k - i;
        if (j > 0 && i < na && b[j - 1] > a[i])
            lo = i + 1;
        else
            hi = i;
    }
    const uint64_t i = lo, j = k - i;
    if (i >= na) return b[j];
    if (j >= nb) return a[i];
    return a[i] < b[j] ? a[i] : b[j];
}

__global__ __launch_bounds__(64) void pairs_header_kernel(const unsigned long long *__restrict__ sorted, const uint32_t *__restrict__ off,
                                                          const unsigned long long *__restrict__ stats, const uint32_t *__restrict__ pair_a,
                                                          const uint32_t *__restrict__ pair_b, uint32_t n_pairs, double scale,
                                                          SseqPairHeader *__restrict__ hdr) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_pairs) return;
    const uint32_t ga = pair_a[j], gb = pair_b[j];
    const unsigned long long *a = sorted + off[ga], *b = sorted + off[gb];
    const uint64_t na = off[ga + 1] - off[ga], nb = off[gb + 1] - off[gb], len = na + nb; // len >= 1: the host refuses an empty union
    double m_s;
    if (len == 1) {
        m_s = (double)pairs_kth(a, na, b, nb, 0);
    } else {
        const double length = (double)(len - 1);
        const double rank = (50.0 / 100.0) * length;
        const double l_rank = floor(rank);
        const double dd = rank - l_rank;
        const uint64_t n = (uint64_t)l_rank;
        const double lo = (double)pairs_kth(a, na, b, nb, n), hi = (double)pairs_kth(a, na, b, nb, n + 1); // n + 1 <= len - 1
        m_s = lo + (hi - lo) * dd;
    }
    U128 inv{stats[(uint64_t)ga * 3 + 1], stats[(uint64_t)ga * 3 + 2]};
    add128(inv, U128{stats[(uint64_t)gb * 3 + 1], stats[(uint64_t)gb * 3 + 2]});
    SseqPairHeader h;
    h.m_s = m_s;
    h.n_s = (double)len;
    h.sum_sf = m_s * from_fixed(&inv.lo, scale); // Σ 1/sf_c = m_S Σ 1/u_c
    h.sf_a = (double)stats[(uint64_t)ga * 3] / m_s;
    h.sf_b = (double)stats[(uint64_t)gb * 3] / m_s;
    h.n_a = na;
    h.n_b = nb;
    h.a = ga;
    h.b = gb;
    // the literal route: no finite size factor, or a cell total of the union so large that a count of 1 in that cell would not keep its
    // bits under the call's quantum (fixed128.hpp): the reference's own calls give every gene a quantum of its own there
    const unsigned long long top_a = na ? a[na - 1] : 0ull, top_b = nb ? b[nb - 1] : 0ull;
    h.literal = (m_s == 0.0 || !fixed_totals_quantum_keeps(top_a > top_b ? top_a : top_b, scale)) ? 1u : 0u;
    h.pad = 0u;
    hdr[j] = h;
}

// acc: n_groups x genes x 5 u64 (launch_merge_pass); outputs genes x n_pairs. The expressions are cluster_host.cpp's from_sums and
// sseq_params_from_moments' first loop, in their order
__global__ __launch_bounds__(256) void pairs_moments_kernel(const unsigned long long *__restrict__ acc, const SseqPairHeader *__restrict__ hdr,
                                                            uint64_t genes, uint32_t n_pairs, double scale, double *__restrict__ mean_o,
                                                            double *__restrict__ var_o, uint8_t *__restrict__ use_o, double *__restrict__ phi_mm_o,
                                                            unsigned long long *__restrict__ sums_a, unsigned long long *__restrict__ sums_b) {
    const uint64_t total = genes * n_pairs;
    for (uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t g = o / n_pairs;
        const uint32_t j = (uint32_t)(o - g * n_pairs);
        const SseqPairHeader h = hdr[j];
        const unsigned long long *a = acc + ((uint64_t)h.a * genes + g) * 5, *b = acc + ((uint64_t)h.b * genes + g) * 5;
        U128 s1{a[1], a[2]}, s2{a[3], a[4]};
        add128(s1, U128{b[1], b[2]});
        add128(s2, U128{b[3], b[4]});
        // Σ x/sf = m_S Σ x/u_c, Σ (x/sf)² = m_S² Σ (x/u_c)²; V[X] = E[X²] - E[X]² (sqz/src/mat.rs:333-380)
        const double mean = h.m_s * from_fixed(&s1.lo, scale) / h.n_s;
        const double var = h.m_s * h.m_s * from_fixed(&s2.lo, scale) / h.n_s - mean * mean;
        const bool use = var > 0.0;
        double res = 0.0;
        if (use) {
            const double t = (h.n_s * var - mean * h.sum_sf) / (mean * mean * h.sum_sf);
            res = 0.0 < t ? t : 0.0; // max(0.0, t) as the host takes it: a NaN gives 0
        }
        mean_o[o] = mean;
        var_o[o] = var;
        use_o[o] = use ? 1 : 0;
        phi_mm_o[o] = res;
        sums_a[o] = a[0];
        sums_b[o] = b[0];
    }
}

__device__ __forceinline__ unsigned long long pairs_order_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double pairs_from_order_key(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

// Σ of one value per thread over the workgroup, the same tree whatever the timing: a butterfly inside each wave, the waves in order
__device__ __forceinline__ double pairs_block_sum(double v, double *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
    for (uint32_t w = 1; w < PAIRS_THREADS / 64; w++) s += red[w];
    return s;
}

// block j: column j of phi_mm / use (genes x n_pairs); zd[2j] = zeta_hat, zd[2j + 1] = delta; phi column j
__global__ __launch_bounds__(PAIRS_THREADS) void pairs_shrink_kernel(const double *__restrict__ phi_mm, const uint8_t *__restrict__ use, uint64_t genes,
                                                                     uint32_t n_pairs, double pct, double *__restrict__ zd,
                                                                     double *__restrict__ phi) {
    __shared__ uint32_t hist[2][256];
    __shared__ unsigned long long prefix[2];
    __shared__ uint64_t rank[2];
    __shared__ uint32_t n_used_s, any_pos_s;
    __shared__ double red[PAIRS_THREADS / 64];
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    const uint64_t ld = n_pairs;
    if (tid == 0) n_used_s = any_pos_s = 0u;
    for (uint32_t i = tid; i < 512; i += blockDim.x) (&hist[0][0])[i] = 0u;
    __syncthreads();
    uint32_t cnt = 0, pos = 0;
    for (uint64_t g = tid; g < genes; g += blockDim.x)
        if (use[g * ld + j]) {
            cnt++;
            if (phi_mm[g * ld + j] > 0.0) pos = 1;
        }
    if (cnt) atomicAdd(&n_used_s, cnt);
    if (pos) atomicOr(&any_pos_s, 1u);
    __syncthreads();
    const uint64_t n_used = n_used_s;
    const bool cond = any_pos_s != 0u;
    if (n_used == 0) { // no gene with variance: zeta_hat = delta = 0 and every dispersion 0 (diff_exp.rs:409-441)
        for (uint64_t g = tid; g < genes; g += blockDim.x) phi[g * ld + j] = 0.0;
        if (tid == 0) zd[2 * (uint64_t)j] = zd[2 * (uint64_t)j + 1] = 0.0;
        return;
    }
    // percentile_of_sorted (stat.rs:140-162): the two ranks it reads and the weight between them
    double frac = 0.0;
    uint64_t r0 = n_used - 1, r1 = n_used - 1; // a single value, or pct == 100: the last element
    if (n_used > 1 && pct != 100.0) {
        const double length = (double)(n_used - 1);
        const double rk = (pct / 100.0) * length;
        const double l_rank = floor(rk);
        frac = rk - l_rank;
        r0 = (uint64_t)l_rank;
        r1 = r0 + 1 < n_used ? r0 + 1 : n_used - 1;
    }
    if (tid < 2) {
        prefix[tid] = 0ull;
        rank[tid] = tid == 0 ? r0 : r1;
    }
    __syncthreads();
    for (int shift = 56; shift >= 0; shift -= 8) {
        const unsigned long long hi_mask = shift == 56 ? 0ull : ~0ull << (shift + 8);
        const unsigned long long p0 = prefix[0], p1 = prefix[1];
        for (uint64_t g = tid; g < genes; g += blockDim.x) {
            if (!use[g * ld + j]) continue;
            const unsigned long long key = pairs_order_key(phi_mm[g * ld + j]);
            const uint32_t digit = (uint32_t)(key >> shift) & 255u;
            if ((key & hi_mask) == p0) atomicAdd(&hist[0][digit], 1u);
            if ((key & hi_mask) == p1) atomicAdd(&hist[1][digit], 1u);
        }
        __syncthreads();
        // wave h finds the bucket of rank h: lane l holds bins 4l .. 4l+3, an inclusive scan over the lanes
        const uint32_t wave = tid >> 6, lane = tid & 63u;
        if (wave < 2) {
            const uint32_t *hb = hist[wave];
            const uint32_t c0 = hb[4 * lane], c1 = hb[4 * lane + 1], c2 = hb[4 * lane + 2], c3 = hb[4 * lane + 3];
            const uint64_t local = (uint64_t)c0 + c1 + c2 + c3;
            uint64_t incl = local;
            for (int o = 1; o < 64; o <<= 1) {
                const uint64_t v = (uint64_t)__shfl_up((long long)incl, o);
                if ((int)lane >= o) incl += v;
            }
            const uint64_t excl = incl - local, r = rank[wave];
            if (excl <= r && r < incl) {
                uint64_t cum = excl;
                uint32_t d = 0;
                if (cum + c0 <= r) {
                    cum += c0;
                    d = 1;
                    if (cum + c1 <= r) {
                        cum += c1;
                        d = 2;
                        if (cum + c2 <= r) {
                            cum += c2;
                            d = 3;
                        }
                    }
                }
                rank[wave] = r - cum;
                prefix[wave] |= (unsigned long long)(4 * lane + d) << shift;
            }
        }
        __syncthreads();
        for (uint32_t i = tid; i < 512; i += blockDim.x) (&hist[0][0])[i] = 0u;
        __syncthreads();
    }
    const double s_lo = pairs_from_order_key(prefix[0]), s_hi = pairs_from_order_key(prefix[1]);
    const double zh = r0 == r1 ? s_lo : s_lo + (s_hi - s_lo) * frac;
    // the mean of the used dispersions and the two sums of squared deviations: a thread's genes in ascending order, then the fixed tree
    double t = 0.0;
    for (uint64_t g = tid; g < genes; g += blockDim.x)
        if (use[g * ld + j]) t += phi_mm[g * ld + j];
    const double mean_phi = pairs_block_sum(t, red) / (double)n_used;
    double ta = 0.0, tb = 0.0;
    for (uint64_t g = tid; g < genes; g += blockDim.x)
        if (use[g * ld + j]) {
            const double x = phi_mm[g * ld + j];
            ta += (x - mean_phi) * (x - mean_phi);
            tb += (x - zh) * (x - zh);
        }
    const double a = pairs_block_sum(ta, red), b = pairs_block_sum(tb, red);
    const double n_genes = (double)genes;
    const double dl = (a / (n_genes - 1.0)) / (b / (n_genes - 2.0));
    for (uint64_t g = tid; g < genes; g += blockDim.x)
        phi[g * ld + j] = (cond && use[g * ld + j]) ? (1.0 - dl) * phi_mm[g * ld + j] + dl * zh : 0.0;
    if (tid == 0) {
        zd[2 * (uint64_t)j] = zh;
        zd[2 * (uint64_t)j + 1] = dl;
    }
}

// ---- the grouped accumulators across shards ----------------------------------------------------------------------------
// Every rank holds partial sums of the (group, gene) table: 5 u64 per entry, [Σ x, Σ x/u lo, hi, Σ (x/u)² lo, hi]. Σ x reduces as it
// is; a u64 sum of the low words would lose their carries. A tile of entries is therefore written as SSEQ_ACC_PLANES planes of u64
// that cannot overflow under a sum over up to 2^31 ranks: Σ x, then for each moment the two 32-bit halves of lo and hi whole (the
// scale of the pass keeps the sum over ALL cells below 2^126, so the hi words of the ranks add up below 2^62). After the all-reduce
// the join propagates the carries of the halves into hi. Both kernels are streams: a workgroup moves SSEQ_ACC_BLOCK entries, the
// 40-byte entries go through LDS so that every global access is a 16-byte one at consecutive addresses, and a thread owns two
// neighbouring entries, which makes the plane accesses 16 bytes wide as well. No atomics.
constexpr uint32_t SSEQ_ACC_BLOCK = 512; // entries per workgroup of 256 threads: 20 KB of LDS
constexpr unsigned long long LIMB_MASK = 0xFFFFFFFFull;

// acc: the tile's first entry (an even entry of the table: 16-byte aligned); planes: SSEQ_ACC_PLANES x ne_pad, ne_pad = ne rounded up to even
__global__ __launch_bounds__(256) void pairs_acc_split_kernel(const unsigned long long *__restrict__ acc, uint64_t ne, uint64_t ne_pad,
                                                              unsigned long long *__restrict__ planes) {
    __shared__ ulonglong2 stage[SSEQ_ACC_BLOCK * 5 / 2];
    const uint32_t tid = threadIdx.x;
    const uint64_t e0 = (uint64_t)blockIdx.x * SSEQ_ACC_BLOCK;
    const uint64_t n_words = (ne - e0 < SSEQ_ACC_BLOCK ? ne - e0 : SSEQ_ACC_BLOCK) * 5; // ne > e0: the launcher sizes the grid
    const unsigned long long *src = acc + e0 * 5;
    for (uint32_t i = tid; i < SSEQ_ACC_BLOCK * 5 / 2; i += 256) {
        ulonglong2 v = make_ulonglong2(0ull, 0ull); // the entries behind the table's end read as zeros
        if (2ull * i + 1 < n_words)
            v = reinterpret_cast<const ulonglong2 *>(src)[i];
        else if (2ull * i < n_words)
            v.x = src[2ull * i];
        stage[i] = v;
    }
    __syncthreads();
    const uint64_t e = e0 + 2ull * tid;
    if (e >= ne_pad) return;
    const unsigned long long *w = reinterpret_cast<const unsigned long long *>(stage) + 10u * tid; // entries e and e + 1
    ulonglong2 out[SSEQ_ACC_PLANES];
    out[0] = make_ulonglong2(w[0], w[5]);
#pragma unroll
    for (uint32_t m = 0; m < 2; m++) {
        const unsigned long long lo_a = w[1 + 2 * m], lo_b = w[6 + 2 * m];
        out[1 + 3 * m] = make_ulonglong2(lo_a & LIMB_MASK, lo_b & LIMB_MASK);
        out[2 + 3 * m] = make_ulonglong2(lo_a >> 32, lo_b >> 32);
        out[3 + 3 * m] = make_ulonglong2(w[2 + 2 * m], w[7 + 2 * m]);
    }
#pragma unroll
    for (uint32_t p = 0; p < SSEQ_ACC_PLANES; p++) *reinterpret_cast<ulonglong2 *>(planes + p * ne_pad + e) = out[p];
}

__global__ __launch_bounds__(256) void pairs_acc_join_kernel(const unsigned long long *__restrict__ planes, uint64_t ne, uint64_t ne_pad,
                                                             unsigned long long *__restrict__ acc) {
    __shared__ ulonglong2 stage[SSEQ_ACC_BLOCK * 5 / 2];
    const uint32_t tid = threadIdx.x;
    const uint64_t e0 = (uint64_t)blockIdx.x * SSEQ_ACC_BLOCK;
    const uint64_t e = e0 + 2ull * tid;
    if (e < ne_pad) {
        ulonglong2 in[SSEQ_ACC_PLANES];
#pragma unroll
        for (uint32_t p = 0; p < SSEQ_ACC_PLANES; p++) in[p] = *reinterpret_cast<const ulonglong2 *>(planes + p * ne_pad + e);
        unsigned long long *w = reinterpret_cast<unsigned long long *>(stage) + 10u * tid;
        w[0] = in[0].x;
        w[5] = in[0].y;
#pragma unroll
        for (uint32_t m = 0; m < 2; m++) {
            // a sum of low halves is below 2^63 and its carry below 2^31: no step overflows
            const unsigned long long ca = (in[1 + 3 * m].x >> 32) + in[2 + 3 * m].x, cb = (in[1 + 3 * m].y >> 32) + in[2 + 3 * m].y;
            w[1 + 2 * m] = (in[1 + 3 * m].x & LIMB_MASK) | (ca << 32);
            w[2 + 2 * m] = in[3 + 3 * m].x + (ca >> 32);
            w[6 + 2 * m] = (in[1 + 3 * m].y & LIMB_MASK) | (cb << 32);
            w[7 + 2 * m] = in[3 + 3 * m].y + (cb >> 32);
        }
    }
    __syncthreads();
    const uint64_t n_words = (ne - e0 < SSEQ_ACC_BLOCK ? ne - e0 : SSEQ_ACC_BLOCK) * 5;
    unsigned long long *dst = acc + e0 * 5;
    for (uint32_t i = tid; i < SSEQ_ACC_BLOCK * 5 / 2; i += 256) {
        if (2ull * i + 1 < n_words)
            reinterpret_cast<ulonglong2 *>(dst)[i] = stage[i];
        else if (2ull * i < n_words)
            dst[2ull * i] = stage[i].x;
    }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
void launch_pairs_acc_split(hipStream_t s, const unsigned long long *d_acc_tile, uint64_t ne, unsigned long long *d_planes) {
    if (!ne) return;
    const uint64_t ne_pad = (ne + 1) & ~1ull;
    hipLaunchKernelGGL(pairs_acc_split_kernel, dim3((uint32_t)((ne + SSEQ_ACC_BLOCK - 1) / SSEQ_ACC_BLOCK)), dim3(256), 0, s, d_acc_tile, ne, ne_pad,
                       d_planes);
    SCANRS_HIP(hipGetLastError());
}

void launch_pairs_acc_join(hipStream_t s, const unsigned long long *d_planes, uint64_t ne, unsigned long long *d_acc_tile) {
    if (!ne) return;
    const uint64_t ne_pad = (ne + 1) & ~1ull;
    hipLaunchKernelGGL(pairs_acc_join_kernel, dim3((uint32_t)((ne + SSEQ_ACC_BLOCK - 1) / SSEQ_ACC_BLOCK)), dim3(256), 0, s, d_planes, ne, ne_pad,
                       d_acc_tile);
    SCANRS_HIP(hipGetLastError());
}

static inline uint32_t pairs_grid(uint64_t items, uint32_t per_block, uint32_t cap) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(cap, (items + per_block - 1) / per_block));
}

void launch_pairs_group_stats(hipStream_t s, const unsigned long long *d_tot, const uint32_t *d_perm, const uint32_t *d_off, uint32_t n_groups,
                              uint64_t n_labelled, double scale, unsigned long long *d_gathered, unsigned long long *d_sorted,
                              unsigned long long *d_stats, DevBuf<char> &sort_tmp) {
    SCANRS_HIP(hipMemsetAsync(d_stats, 0, (size_t)n_groups * 3 * 8, s));
    if (n_labelled) {
        hipLaunchKernelGGL(pairs_gather_kernel, dim3(pairs_grid(n_labelled, 256, 16384)), dim3(256), 0, s, d_tot, d_perm, n_labelled, d_gathered);
        SCANRS_HIP(hipGetLastError());
        size_t tmp_bytes = 0;
        SCANRS_HIP(rocprim::segmented_radix_sort_keys(nullptr, tmp_bytes, d_gathered, d_sorted, (unsigned int)n_labelled, n_groups, d_off, d_off + 1, 0,
                                                      64, s));
        sort_tmp.alloc(std::max<size_t>(1, tmp_bytes)); // the caller keeps it until the stream has been waited for
        SCANRS_HIP(rocprim::segmented_radix_sort_keys(sort_tmp.p, tmp_bytes, d_gathered, d_sorted, (unsigned int)n_labelled, n_groups, d_off, d_off + 1, 0, 64,
                                                      s));
    }
    hipLaunchKernelGGL(pairs_group_stats_kernel, dim3(n_groups), dim3(256), 0, s, (const unsigned long long *)d_sorted, d_off, scale, d_stats);
    SCANRS_HIP(hipGetLastError());
}

void launch_pairs_headers(hipStream_t s, const unsigned long long *d_sorted, const uint32_t *d_off, const unsigned long long *d_stats,
                          const uint32_t *d_pair_a, const uint32_t *d_pair_b, uint32_t n_pairs, double scale, SseqPairHeader *d_hdr) {
    hipLaunchKernelGGL(pairs_header_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, s, d_sorted, d_off, d_stats, d_pair_a, d_pair_b, n_pairs, scale,
                       d_hdr);
    SCANRS_HIP(hipGetLastError());
}

void launch_pairs_moments(hipStream_t s, const unsigned long long *d_acc, const SseqPairHeader *d_hdr, uint64_t genes, uint32_t n_pairs,
                          double scale, double *d_mean, double *d_var, uint8_t *d_use, double *d_phi_mm, unsigned long long *d_sums_a,
                          unsigned long long *d_sums_b) {
    if (!genes) return;
    hipLaunchKernelGGL(pairs_moments_kernel, dim3(pairs_grid(genes * n_pairs, 256, 65536)), dim3(256), 0, s, d_acc, d_hdr, genes, n_pairs, scale,
                       d_mean, d_var, d_use, d_phi_mm, d_sums_a, d_sums_b);
    SCANRS_HIP(hipGetLastError());
}

void launch_pairs_shrink(hipStream_t s, const double *d_phi_mm, const uint8_t *d_use, uint64_t genes, uint32_t n_pairs, double pct, double *d_zd,
                         double *d_phi) {
    hipLaunchKernelGGL(pairs_shrink_kernel, dim3(n_pairs), dim3(PAIRS_THREADS), 0, s, d_phi_mm, d_use, genes, n_pairs, pct, d_zd, d_phi);
    SCANRS_HIP(hipGetLastError());
}

} // namespace scanrs
