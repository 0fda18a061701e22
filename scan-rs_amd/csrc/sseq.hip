// HIP kernels of sSeq differential expression (diff-exp/src/diff_exp.rs, dist.rs) + their launchers. Host logic: sseq_host.cpp.
//
//   sseq_gene_major_kernel   one pass over the nonzeros of the gene-major copy: a wave owns a gene, gathers the labels of its
//                            cells and adds the counts into a per-wave LDS row of n_groups u64 sums (integer LDS atomics);
//                            optionally Σ x/sf_c and Σ (x/sf_c)² over the labelled cells (the moments of compute_sseq_params)
//   sseq_cell_major_kernel   the same sums from the cell-major copy: a wave owns a cell (one label), the sums are scattered
//                            over the genes with u64 global atomics
//   sseq_cell_totals_kernel  per-cell count totals (size factors) from either copy
//   sseq_mom_split / _join   the 128-bit moments as 32-bit limbs around the u64 all-reduce of a sharded handle
//   sseq_exact_*_kernel      the exact NB test (dist.rs:74-118, 259-310) over a flat list of fixed-size term chunks
//   sseq_asymptotic_kernel   the beta approximation (dist.rs:226-257), one thread per test
//   sseq_ratio_*_kernel      the Ratio backend of the exact test (dist.rs:116-215): sseq_ratio.inc
//
// No float atomics. The moments are accumulated as 128-bit FIXED-POINT integers (two u64 words, carry counted
// with an integer atomic): every term x/sf_c is rounded once to a quantum of 2^-E, and the integer sum is exact, so the result
// depends neither on the order in which the waves arrive nor on which copy of the matrix was walked: both orientations give the
// same bits. E is chosen per launch from a bound of the sums (every sum fits below 2^124) where the smallest possible term keeps
// its bits under that quantum, and per gene otherwise, from the class of the gene's largest term (sseq_term_class_kernel, one
// more walk; fixed128.hpp has the rule and sseq_host.cpp the choice): every gene's mean comes back within 1e-12 relative and its
// variance within 1e-10 of its own Σ (x/sf_c)² / m, whatever the other genes hold.
#include "common.hpp"
#include "fixed128.hpp"
#include "special.hpp"

namespace scanrs {

// d_mom (rows x 4 u64): [lo, hi] of Σ x/sf, [lo, hi] of Σ (x/sf)²; d_bad: per gene, a term was not finite (sf = 0 with x > 0)
// MOM: 0 the group sums only; 1 the moments under the launch's two scales; 2 under every gene's own scales, from its class gcls[g]
template <int MOM>
__global__ __launch_bounds__(256) void sseq_gene_major_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                              const uint32_t *__restrict__ values, uint64_t n_genes,
                                                              const int16_t *__restrict__ labels, uint32_t n_groups,
                                                              unsigned long long *__restrict__ sums, const double *__restrict__ sf,
                                                              double scale1, double scale2, unsigned long long *__restrict__ mom,
                                                              uint32_t *__restrict__ bad, const uint32_t *__restrict__ gcls, int log2m) {
    extern __shared__ unsigned long long gm_acc[]; // [wave][group]
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    unsigned long long *acc = gm_acc + (size_t)wave * n_groups;
    for (uint64_t g0 = (uint64_t)blockIdx.x * n_waves; g0 < n_genes; g0 += (uint64_t)gridDim.x * n_waves) {
        const uint64_t g = g0 + wave;
        for (uint32_t j = lane; j < n_groups; j += 64) acc[j] = 0ull;
        __syncthreads();
        U128 s1{0, 0}, s2{0, 0};
        uint32_t nonfinite = 0;
        if (g < n_genes) {
            const uint64_t p0 = indptr[g], p1 = indptr[g + 1];
            if (MOM == 2) { // uniform over the wave
                scale1 = fixed_class_scale1(gcls[g], log2m);
                scale2 = fixed_class_scale2(gcls[g], log2m);
            }
            for (uint64_t p = p0 + lane; p < p1; p += 64) {
                const uint32_t c = indices[p];
                const int l = labels[c];
                if (l < 0) continue;
                const uint32_t x = values[p];
                atomicAdd(&acc[l], (unsigned long long)x);
                if (MOM) {
                    const double t = (double)x / sf[c];
                    if (!isfinite(t)) {
                        nonfinite = 1;
                        continue;
                    }
                    add128(s1, to_fixed(t, scale1));
                    add128(s2, to_fixed(t * t, scale2));
                }
            }
        }
        __syncthreads();
        if (g < n_genes) {
            for (uint32_t j = lane; j < n_groups; j += 64) sums[g * n_groups + j] = acc[j];
            if (MOM) {
                for (int off = 32; off > 0; off >>= 1) {
                    add128(s1, shfl_down128(s1, off));
                    add128(s2, shfl_down128(s2, off));
                    nonfinite |= (uint32_t)__shfl_down((int)nonfinite, off);
                }
                if (lane == 0) {
                    mom[g * 4 + 0] = s1.lo;
                    mom[g * 4 + 1] = s1.hi;
                    mom[g * 4 + 2] = s2.lo;
                    mom[g * 4 + 3] = s2.hi;
                    bad[g] = nonfinite;
                }
            }
        }
    }
}

// sums and mom are zeroed by the launcher
template <int MOM>
__global__ __launch_bounds__(256) void sseq_cell_major_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                              const uint32_t *__restrict__ values, uint64_t n_cells,
                                                              const int16_t *__restrict__ labels, uint32_t n_groups,
                                                              unsigned long long *__restrict__ sums, const double *__restrict__ sf,
                                                              double scale1, double scale2, unsigned long long *__restrict__ mom,
                                                              uint32_t *__restrict__ bad, const uint32_t *__restrict__ gcls, int log2m) {
    const uint32_t lane = threadIdx.x & 63u, n_waves = blockDim.x >> 6;
    for (uint64_t c = (uint64_t)blockIdx.x * n_waves + (threadIdx.x >> 6); c < n_cells; c += (uint64_t)gridDim.x * n_waves) {
        const int l = labels[c];
        if (l < 0) continue; // uniform over the wave
        const double sfc = MOM ? sf[c] : 1.0;
        const uint64_t p0 = indptr[c], p1 = indptr[c + 1];
        for (uint64_t p = p0 + lane; p < p1; p += 64) {
            const uint32_t g = indices[p], x = values[p];
            atomicAdd(&sums[(uint64_t)g * n_groups + l], (unsigned long long)x);
            if (MOM) {
                const double t = (double)x / sfc;
                if (!isfinite(t)) {
                    bad[g] = 1u;
                    continue;
                }
                if (MOM == 2) {
                    const uint32_t k = gcls[g];
                    scale1 = fixed_class_scale1(k, log2m);
                    scale2 = fixed_class_scale2(k, log2m);
                }
                atomic_add128(&mom[(uint64_t)g * 4 + 0], to_fixed(t, scale1));
                atomic_add128(&mom[(uint64_t)g * 4 + 2], to_fixed(t * t, scale2));
            }
        }
    }
}

// per-cell totals: from the cell-major copy a wave sums its cell; from the gene-major copy the counts are scattered (u64 atomics)
__global__ __launch_bounds__(256) void sseq_cell_totals_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                               const uint32_t *__restrict__ values, uint64_t n_outer, int outer_is_cell,
                                                               unsigned long long *__restrict__ tot) {
    const uint32_t lane = threadIdx.x & 63u, n_waves = blockDim.x >> 6;
    for (uint64_t o = (uint64_t)blockIdx.x * n_waves + (threadIdx.x >> 6); o < n_outer; o += (uint64_t)gridDim.x * n_waves) {
        const uint64_t p0 = indptr[o], p1 = indptr[o + 1];
        unsigned long long s = 0;
        for (uint64_t p = p0 + lane; p < p1; p += 64) {
            if (outer_is_cell)
                s += values[p];
            else
                atomicAdd(&tot[indices[p]], (unsigned long long)values[p]);
        }
        if (outer_is_cell) {
            for (int off = 32; off > 0; off >>= 1) s += (unsigned long long)__shfl_down((long long)s, off);
            if (lane == 0) tot[o] = s;
        }
    }
}

// The class of every gene's moment sums (fixed128.hpp: from the largest finite x/sf_c over its labelled cells), from either copy: a
// wave owns an outer vector; a gene's wave reduces and stores, a cell's wave scatters with an integer atomicMax. cls is zeroed by the
// launcher. The squares need no class of their own: the largest square is the square of the largest term.
__global__ __launch_bounds__(256) void sseq_term_class_kernel(const uint64_t *__restrict__ indptr, const uint32_t *__restrict__ indices,
                                                              const uint32_t *__restrict__ values, uint64_t n_outer, int outer_is_gene,
                                                              const int16_t *__restrict__ labels, const double *__restrict__ sf,
                                                              uint32_t *__restrict__ cls) {
    const uint32_t lane = threadIdx.x & 63u, n_waves = blockDim.x >> 6;
    for (uint64_t o = (uint64_t)blockIdx.x * n_waves + (threadIdx.x >> 6); o < n_outer; o += (uint64_t)gridDim.x * n_waves) {
        if (!outer_is_gene && labels[o] < 0) continue; // uniform over the wave
        const uint64_t p0 = indptr[o], p1 = indptr[o + 1];
        uint32_t k = 0;
        for (uint64_t p = p0 + lane; p < p1; p += 64) {
            const uint32_t i = indices[p];
            if (outer_is_gene && labels[i] < 0) continue;
            const double t = (double)values[p] / sf[outer_is_gene ? i : o];
            if (!isfinite(t)) continue;
            if (outer_is_gene)
                k = max(k, fixed_term_class(t));
            else
                atomicMax(&cls[i], fixed_term_class(t));
        }
        if (outer_is_gene) {
            for (int off = 32; off > 0; off >>= 1) k = max(k, (uint32_t)__shfl_xor((int)k, off));
            if (lane == 0) cls[o] = k;
        }
    }
}

__global__ void sseq_max_u32_kernel(const uint32_t *__restrict__ v, uint64_t n, uint32_t *__restrict__ out) {
    uint32_t m = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) m = max(m, v[i]);
    for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
    if ((threadIdx.x & 63u) == 0) atomicMax(out, m);
}

// ---- the moments across shards ---------------------------------------------------------------------------------------------------
// A sum all-reduce of u64 words would lose the carries between the two words of a 128-bit sum. Each rank therefore splits its two
// sums per gene into 32-bit limbs held in u64 (limbs: genes x SSEQ_LIMB_STRIDE: 4 limbs of Σ x/sf, 4 of Σ (x/sf)², the bad flag);
// the limbs of up to 2^31 ranks add up without overflow, and the join propagates the carries. The scale of the launch keeps the
// sum over ALL cells below 2^126 (fixed128.hpp), so the top limb's carry is zero and the join is exact.
__global__ void sseq_mom_split_kernel(const unsigned long long *__restrict__ mom, const uint32_t *__restrict__ bad, uint64_t n_genes,
                                      unsigned long long *__restrict__ limbs) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_genes) return;
    unsigned long long *out = limbs + g * SSEQ_LIMB_STRIDE;
#pragma unroll
    for (uint32_t w = 0; w < 4; w++) {
        const unsigned long long v = mom[g * 4 + w];
        out[2 * w] = v & 0xFFFFFFFFull;
        out[2 * w + 1] = v >> 32;
    }
    out[8] = bad[g] ? 1ull : 0ull;
}

__global__ void sseq_mom_join_kernel(const unsigned long long *__restrict__ limbs, uint64_t n_genes, unsigned long long *__restrict__ mom,
                                     uint32_t *__restrict__ bad) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_genes) return;
    const unsigned long long *in = limbs + g * SSEQ_LIMB_STRIDE;
#pragma unroll
    for (uint32_t s = 0; s < 2; s++) {
        unsigned long long c = 0, r[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            c = (c >> 32) + in[4 * s + k]; // carry < 2^32 and a limb sum < 2^63: no overflow
            r[k] = c & 0xFFFFFFFFull;
        }
        mom[g * 4 + 2 * s] = r[0] | (r[1] << 32);
        mom[g * 4 + 2 * s + 1] = r[2] | (r[3] << 32);
    }
    bad[g] = in[8] ? 1u : 0u;
}

// ---- exact test --------------------------------------------------------------------------------------------------------------
// The terms k = 0 .. n of every test are cut into chunks of SSEQ_CHUNK; chunk c of the launch belongs to the test whose
// chunk0 <= c < next chunk0. A workgroup computes one chunk's (max, Σ exp(t - max)) for all terms and for the extreme terms
// (t <= the observed term) with a fixed reduction tree; the combine kernel folds a test's chunks in chunk order. A test's
// result depends only on its own inputs: not on the grid, nor on the other tests of the launch.
__device__ __forceinline__ double wave_max(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ void sseq_exact_obs_kernel(const SseqExactTest *__restrict__ tests, uint32_t n_tests, double *__restrict__ obs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tests) return;
    const SseqExactTest t = tests[i];
    obs[i] = special::nb_term(t.xa, t.n, t.sar, t.sbr, t.add_total);
}

__global__ __launch_bounds__(SSEQ_CHUNK_THREADS) void sseq_exact_chunk_kernel(const SseqExactTest *__restrict__ tests, uint32_t n_tests,
                                                                               const double *__restrict__ obs, uint64_t n_chunks,
                                                                               double4 *__restrict__ part) {
    __shared__ double red[SSEQ_CHUNK_THREADS / 64][2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        // the test owning chunk c: last i with chunk0 <= c
        uint32_t lo = 0, hi = n_tests;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (tests[mid].chunk0 <= c)
                lo = mid;
            else
                hi = mid;
        }
        const SseqExactTest t = tests[lo];
        const double o = obs[lo];
        const uint64_t k0 = (c - t.chunk0) * SSEQ_CHUNK;
        double v[SSEQ_TERMS_PER_THREAD];
        double m_all = -INFINITY, m_ext = -INFINITY;
#pragma unroll
        for (uint32_t j = 0; j < SSEQ_TERMS_PER_THREAD; j++) {
            const uint64_t k = k0 + (uint64_t)j * SSEQ_CHUNK_THREADS + tid;
            v[j] = k <= t.n ? special::nb_term(k, t.n, t.sar, t.sbr, t.add_total) : NAN;
            if (k <= t.n) {
                m_all = fmax(m_all, v[j]);
                if (v[j] <= o) m_ext = fmax(m_ext, v[j]);
            }
        }
        m_all = wave_max(m_all);
        m_ext = wave_max(m_ext);
        if (lane == 0) {
            red[wave][0] = m_all;
            red[wave][1] = m_ext;
        }
        __syncthreads();
        m_all = red[0][0];
        m_ext = red[0][1];
        for (uint32_t w = 1; w < SSEQ_CHUNK_THREADS / 64; w++) {
            m_all = fmax(m_all, red[w][0]);
            m_ext = fmax(m_ext, red[w][1]);
        }
        __syncthreads();
        double s_all = 0.0, s_ext = 0.0;
#pragma unroll
        for (uint32_t j = 0; j < SSEQ_TERMS_PER_THREAD; j++) {
            const uint64_t k = k0 + (uint64_t)j * SSEQ_CHUNK_THREADS + tid;
            if (k <= t.n) {
                s_all += exp(v[j] - m_all);
                if (v[j] <= o) s_ext += exp(v[j] - m_ext);
            }
        }
        s_all = wave_sum(s_all);
        s_ext = wave_sum(s_ext);
        if (lane == 0) {
            red[wave][0] = s_all;
            red[wave][1] = s_ext;
        }
        __syncthreads();
        if (tid == 0) {
            s_all = red[0][0];
            s_ext = red[0][1];
            for (uint32_t w = 1; w < SSEQ_CHUNK_THREADS / 64; w++) {
                s_all += red[w][0];
                s_ext += red[w][1];
            }
            part[c] = make_double4(m_all, s_all, m_ext, s_ext);
        }
        __syncthreads();
    }
}

// log-sum-exp of a test's chunks, folded in chunk order; p = exp(lse_ext - lse_all) (dist.rs:114-117)
__global__ void sseq_exact_combine_kernel(const SseqExactTest *__restrict__ tests, uint32_t n_tests, uint64_t n_chunks,
                                          const double4 *__restrict__ part, double *__restrict__ p_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tests) return;
    const uint64_t c0 = tests[i].chunk0, c1 = i + 1 < n_tests ? tests[i + 1].chunk0 : n_chunks;
    double ma = -INFINITY, sa = 0.0, me = -INFINITY, se = 0.0;
    for (uint64_t c = c0; c < c1; c++) {
        const double4 q = part[c];
        if (q.y > 0.0) {
            const double m = fmax(ma, q.x);
            sa = (sa > 0.0 ? sa * exp(ma - m) : 0.0) + q.y * exp(q.x - m);
            ma = m;
        }
        if (q.w > 0.0) {
            const double m = fmax(me, q.z);
            se = (se > 0.0 ? se * exp(me - m) : 0.0) + q.w * exp(q.z - m);
            me = m;
        }
    }
    const double lse_all = log(sa) + ma, lse_ext = log(se) + me;
    p_out[tests[i].out] = exp(lse_ext - lse_all);
}

__global__ void sseq_asymptotic_kernel(const SseqAsymTest *__restrict__ tests, uint32_t n_tests, double *__restrict__ p_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tests) return;
    const SseqAsymTest t = tests[i];
    p_out[t.out] = special::nb_asymptotic(t.xa, t.xb, t.sf_a, t.sf_b, t.mu, t.phi);
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
static inline uint32_t blocks_for(uint64_t items, uint32_t per_block, uint32_t cap) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(cap, (items + per_block - 1) / per_block));
}

uint32_t sseq_max_count(Storage &st, const SparseCopy &cp) {
    uint32_t *d = st.scratch.get<uint32_t>("sseq_max", 1);
    SCANRS_HIP(hipMemsetAsync(d, 0, 4, st.stream));
    if (cp.nnz) hipLaunchKernelGGL(sseq_max_u32_kernel, dim3(blocks_for(cp.nnz, 256, 4096)), dim3(256), 0, st.stream, cp.values.p, cp.nnz, d);
    SCANRS_HIP(hipGetLastError());
    return d2h_value(d, st.stream, __func__, __FILE__, __LINE__);
}

void launch_sseq_cell_totals(Storage &st, const SparseCopy &cp, bool gene_major, uint64_t n_cells, unsigned long long *d_tot) {
    SCANRS_HIP(hipMemsetAsync(d_tot, 0, std::max<uint64_t>(1, n_cells) * 8, st.stream));
    if (cp.n_outer)
        hipLaunchKernelGGL(sseq_cell_totals_kernel, dim3(blocks_for(cp.n_outer, 4, 16384)), dim3(256), 0, st.stream, cp.indptr.p, cp.indices.p,
                           cp.values.p, cp.n_outer, gene_major ? 0 : 1, d_tot);
    SCANRS_HIP(hipGetLastError());
}

void launch_sseq_group_pass(Storage &st, const SparseCopy &cp, bool gene_major, uint64_t n_genes, const int16_t *d_labels, uint32_t n_groups,
                            unsigned long long *d_sums, const double *d_sf, double scale1, double scale2, unsigned long long *d_mom,
                            uint32_t *d_bad, const uint32_t *d_cls, int log2m) {
    const bool mom = d_mom != nullptr;
    if (mom) {
        SCANRS_HIP(hipMemsetAsync(d_mom, 0, std::max<uint64_t>(1, n_genes) * 32, st.stream));
        SCANRS_HIP(hipMemsetAsync(d_bad, 0, std::max<uint64_t>(1, n_genes) * 4, st.stream));
    }
    if (gene_major) {
        // a wave's LDS row holds n_groups u64: up to 4 waves per workgroup within 64 KB
        const uint32_t waves = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(4, 8192 / std::max<uint32_t>(1, n_groups)));
        const size_t lds = (size_t)waves * n_groups * 8;
        const dim3 grid(blocks_for(n_genes, waves, st.opt.sseq_grid_cap)), block(64 * waves);
        if (mom && d_cls)
            hipLaunchKernelGGL(sseq_gene_major_kernel<2>, grid, block, lds, st.stream, cp.indptr.p, cp.indices.p, cp.values.p, n_genes, d_labels,
                               n_groups, d_sums, d_sf, scale1, scale2, d_mom, d_bad, d_cls, log2m);
        else if (mom)
            hipLaunchKernelGGL(sseq_gene_major_kernel<1>, grid, block, lds, st.stream, cp.indptr.p, cp.indices.p, cp.values.p, n_genes, d_labels,
                               n_groups, d_sums, d_sf, scale1, scale2, d_mom, d_bad, d_cls, log2m);
        else
            hipLaunchKernelGGL(sseq_gene_major_kernel<0>, grid, block, lds, st.stream, cp.indptr.p, cp.indices.p, cp.values.p, n_genes, d_labels,
                               n_groups, d_sums, d_sf, scale1, scale2, d_mom, d_bad, d_cls, log2m);
    } else {
        SCANRS_HIP(hipMemsetAsync(d_sums, 0, std::max<uint64_t>(1, n_genes * n_groups) * 8, st.stream));
        const dim3 grid(blocks_for(cp.n_outer, 4, st.opt.sseq_grid_cap)), block(256);
        if (cp.n_outer) {
            if (mom && d_cls)
                hipLaunchKernelGGL(sseq_cell_major_kernel<2>, grid, block, 0, st.stream, cp.indptr.p, cp.indices.p, cp.values.p, cp.n_outer, d_labels,
                                   n_groups, d_sums, d_sf, scale1, scale2, d_mom, d_bad, d_cls, log2m);
            else if (mom)
                hipLaunchKernelGGL(sseq_cell_major_kernel<1>, grid, block, 0, st.stream, cp.indptr.p, cp.indices.p, cp.values.p, cp.n_outer, d_labels,
                                   n_groups, d_sums, d_sf, scale1, scale2, d_mom, d_bad, d_cls, log2m);
            else
                hipLaunchKernelGGL(sseq_cell_major_kernel<0>, grid, block, 0, st.stream, cp.indptr.p, cp.indices.p, cp.values.p, cp.n_outer,
                                   d_labels, n_groups, d_sums, d_sf, scale1, scale2, d_mom, d_bad, d_cls, log2m);
        }
    }
    SCANRS_HIP(hipGetLastError());
}

void launch_sseq_term_class(Storage &st, const SparseCopy &cp, bool gene_major, uint64_t n_genes, const int16_t *d_labels, const double *d_sf,
                            uint32_t *d_cls) {
    SCANRS_HIP(hipMemsetAsync(d_cls, 0, std::max<uint64_t>(1, n_genes) * 4, st.stream));
    if (cp.n_outer)
        hipLaunchKernelGGL(sseq_term_class_kernel, dim3(blocks_for(cp.n_outer, 4, st.opt.sseq_grid_cap)), dim3(256), 0, st.stream, cp.indptr.p, cp.indices.p,
                           cp.values.p, cp.n_outer, gene_major ? 1 : 0, d_labels, d_sf, d_cls);
    SCANRS_HIP(hipGetLastError());
}

void launch_sseq_mom_split(Storage &st, const unsigned long long *d_mom, const uint32_t *d_bad, uint64_t n_genes, unsigned long long *d_limbs) {
    if (!n_genes) return;
    hipLaunchKernelGGL(sseq_mom_split_kernel, dim3((uint32_t)((n_genes + 255) / 256)), dim3(256), 0, st.stream, d_mom, d_bad, n_genes, d_limbs);
    SCANRS_HIP(hipGetLastError());
}

void launch_sseq_mom_join(Storage &st, const unsigned long long *d_limbs, uint64_t n_genes, unsigned long long *d_mom, uint32_t *d_bad) {
    if (!n_genes) return;
    hipLaunchKernelGGL(sseq_mom_join_kernel, dim3((uint32_t)((n_genes + 255) / 256)), dim3(256), 0, st.stream, d_limbs, n_genes, d_mom, d_bad);
    SCANRS_HIP(hipGetLastError());
}

void launch_sseq_exact(hipStream_t s, const SseqExactTest *d_tests, uint32_t n_tests, uint64_t n_chunks, double *d_obs, double4 *d_part,
                       double *d_p) {
    if (!n_tests) return;
    hipLaunchKernelGGL(sseq_exact_obs_kernel, dim3((n_tests + 255) / 256), dim3(256), 0, s, d_tests, n_tests, d_obs);
    hipLaunchKernelGGL(sseq_exact_chunk_kernel, dim3(blocks_for(n_chunks, 1, 65536)), dim3(SSEQ_CHUNK_THREADS), 0, s, d_tests, n_tests,
                       (const double *)d_obs, n_chunks, d_part);
    hipLaunchKernelGGL(sseq_exact_combine_kernel, dim3((n_tests + 63) / 64), dim3(64), 0, s, d_tests, n_tests, n_chunks,
                       (const double4 *)d_part, d_p);
    SCANRS_HIP(hipGetLastError());
}

void launch_sseq_asymptotic(hipStream_t s, const SseqAsymTest *d_tests, uint32_t n_tests, double *d_p) {
    if (!n_tests) return;
    hipLaunchKernelGGL(sseq_asymptotic_kernel, dim3((n_tests + 63) / 64), dim3(64), 0, s, d_tests, n_tests, d_p);
    SCANRS_HIP(hipGetLastError());
}

} // namespace scanrs

#include "sseq_ratio.inc"
