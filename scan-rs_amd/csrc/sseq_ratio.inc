// The Ratio backend of the exact NB test (nb_exact_test_ratio, dist.rs:116-215) on the device. Included at the end of sseq.hip;
// the test list (and each test's anchor) is built in sseq_host.cpp.
//
// The reference anchors U[anchor] = 1 at the first k whose step T(k+1)/T(k) drops below 1 and sweeps outward in both
// directions: U[anchor + t] = Π_{s=1..t} step(anchor + s - 1), U[anchor - t] = Π_{s=1..t} 1 / step(anchor - s). Both sides are
// the same thing in the local index t = 1, 2, ..: a running product of "outward factors" f(t). A side's terms are cut into
// chunks of SSEQ_CHUNK in t, so every chunk starts at its anchor-side end; a test's chunks are its down side (k < anchor)
// first, then its up side (k > anchor), each outward from the anchor. The anchor's own term (1.0) is added by the combine.
//
//   sseq_ratio_prod_kernel    pass A: one workgroup per chunk, the product of the chunk's factors (fixed tree)
//   sseq_ratio_scale_kernel   one thread per test folds its chunk products outward: prod[c] becomes the chunk's scale, the
//                             term just inside of it relative to U[anchor] = 1
//   sseq_ratio_terms_kernel   <true>: one workgroup per test evaluates the chunk holding x_a and keeps U[x_a];
//                             <false>: pass B, every chunk's Σ U and Σ {U <= U[x_a]} (fixed tree). Both instances evaluate
//                             the terms with ratio_chunk_terms, so U <= U[x_a] holds with equality at k = x_a
//   sseq_ratio_combine_kernel one thread per test adds its chunks in chunk order: p = Σ_ext / Σ_all, or SSEQ_RATIO_FALLBACK
//
// One rule is the library's own: with sar == sbr bit for bit the terms k and n - k are equal in exact arithmetic, and the mirror n - x_a
// of the observed term is extreme whatever the roundings of the two sweeps made of it (the reference's `<=` drops it in some cases).
//
// Range: in the unimodal case every outward factor is <= 1, so every partial product is <= 1 and a product that underflows
// does so where the serial sweep's term does; in the U-shaped case (sa_r, sb_r < 1) the anchor is a boundary and the terms
// stay within N^|sa_r - sb_r| < N of it (dist.rs:136-146). A test whose U[x_a] is not finite or below 2^-970 is not
// partitioned here: the terms at and below such a U[x_a] are denormal and carry too few bits. It goes to the LogSpace kernels.
namespace scanrs {
#pragma clang fp contract(off) // factors and products are evaluated as written, the same in every instance

constexpr double SSEQ_RATIO_MIN_OBS = 0x1p-970;

struct RatioChunk {
    bool up;        // k = anchor + t (else anchor - t)
    uint64_t t0;    // the chunk's terms are t = t0 + 1 .. t0 + cnt
    uint32_t cnt;   // 1 .. SSEQ_CHUNK
};

// chunk cl (0-based within the test) of test t
__device__ __forceinline__ RatioChunk ratio_chunk_of(const SseqRatioTest &t, uint64_t cl) {
    const uint64_t n_down = (t.anchor + SSEQ_CHUNK - 1) / SSEQ_CHUNK;
    RatioChunk c;
    c.up = cl >= n_down;
    const uint64_t j = c.up ? cl - n_down : cl, len = c.up ? t.n - t.anchor : t.anchor;
    c.t0 = j * SSEQ_CHUNK;
    c.cnt = (uint32_t)min((uint64_t)SSEQ_CHUNK, len - c.t0);
    return c;
}

// the outward factor U(t) / U(t - 1) of a side: nb_exact_ratio_step (dist.rs:124-126) going up, its reciprocal going down
__device__ __forceinline__ double ratio_factor(bool up, double anchor, double t, double nn, double sar, double sbr) {
    if (up) {
        const double k = anchor + t - 1.0;
        return (sar + k) * (nn - k) / ((k + 1.0) * (sbr + nn - k - 1.0));
    }
    const double k = anchor - t;
    return (k + 1.0) * (sbr + nn - k - 1.0) / ((sar + k) * (nn - k));
}

// a thread's SSEQ_TERMS_PER_THREAD consecutive factors as running products p[j] = f(first) .. f(first + j); 1.0 past the chunk's end
__device__ __forceinline__ void ratio_thread_products(const SseqRatioTest &t, const RatioChunk &c, uint32_t tid, double *p) {
    const double anchor = (double)t.anchor, nn = (double)t.n;
    double run = 1.0;
#pragma unroll
    for (uint32_t j = 0; j < SSEQ_TERMS_PER_THREAD; j++) {
        const uint32_t l = tid * SSEQ_TERMS_PER_THREAD + j; // 0-based within the chunk
        if (l < c.cnt) run = run * ratio_factor(c.up, anchor, (double)(c.t0 + l + 1), nn, t.sar, t.sbr);
        p[j] = run;
    }
}

// v[j] = U of the thread's j-th term: scale x (waves before) x (lanes before) x the thread's running product.
// wtot: SSEQ_CHUNK_THREADS / 64 doubles of LDS; every thread of the workgroup calls this (it synchronizes).
__device__ __forceinline__ void ratio_chunk_terms(const SseqRatioTest &t, const RatioChunk &c, double scale, double *wtot, double *v) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    double p[SSEQ_TERMS_PER_THREAD];
    ratio_thread_products(t, c, tid, p);
    // inclusive scan of the threads' products over the wave, the inner side on the left
    double incl = p[SSEQ_TERMS_PER_THREAD - 1];
    for (int off = 1; off < 64; off <<= 1) {
        const double y = __shfl_up(incl, off);
        if ((int)lane >= off) incl = y * incl;
    }
    double excl = __shfl_up(incl, 1);
    if (lane == 0) excl = 1.0;
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    double base = scale;
    for (uint32_t w = 0; w < wave; w++) base = base * wtot[w];
    base = base * excl;
#pragma unroll
    for (uint32_t j = 0; j < SSEQ_TERMS_PER_THREAD; j++) v[j] = base * p[j];
    __syncthreads(); // wtot may be written again
}

// the test owning chunk c: last i with chunk0 <= c
__device__ __forceinline__ uint32_t ratio_owner(const SseqRatioTest *__restrict__ tests, uint32_t n_tests, uint64_t c) {
    uint32_t lo = 0, hi = n_tests;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tests[mid].chunk0 <= c)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(SSEQ_CHUNK_THREADS) void sseq_ratio_prod_kernel(const SseqRatioTest *__restrict__ tests, uint32_t n_tests,
                                                                              uint64_t n_chunks, double *__restrict__ prod) {
    __shared__ double wtot[SSEQ_CHUNK_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const SseqRatioTest t = tests[ratio_owner(tests, n_tests, c)];
        const RatioChunk ch = ratio_chunk_of(t, c - t.chunk0);
        double p[SSEQ_TERMS_PER_THREAD];
        ratio_thread_products(t, ch, tid, p);
        double q = p[SSEQ_TERMS_PER_THREAD - 1];
        for (int off = 32; off > 0; off >>= 1) q = q * __shfl_xor(q, off);
        if (lane == 0) wtot[wave] = q;
        __syncthreads();
        if (tid == 0) {
            q = wtot[0];
            for (uint32_t w = 1; w < SSEQ_CHUNK_THREADS / 64; w++) q = q * wtot[w];
            prod[c] = q;
        }
        __syncthreads();
    }
}

__global__ void sseq_ratio_scale_kernel(const SseqRatioTest *__restrict__ tests, uint32_t n_tests, uint64_t n_chunks,
                                        double *__restrict__ prod) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tests) return;
    const uint64_t c0 = tests[i].chunk0, c1 = i + 1 < n_tests ? tests[i + 1].chunk0 : n_chunks;
    const uint64_t c_up = c0 + (tests[i].anchor + SSEQ_CHUNK - 1) / SSEQ_CHUNK;
    double s = 1.0;
    for (uint64_t c = c0; c < c1; c++) {
        if (c == c_up) s = 1.0; // the up side starts again from the anchor
        const double q = prod[c];
        prod[c] = s;
        s = s * q;
    }
}

template <bool OBS>
__global__ __launch_bounds__(SSEQ_CHUNK_THREADS) void sseq_ratio_terms_kernel(const SseqRatioTest *__restrict__ tests, uint32_t n_tests,
                                                                               uint64_t n_chunks, const double *__restrict__ scale,
                                                                               double *__restrict__ obs, double2 *__restrict__ part) {
    __shared__ double wtot[SSEQ_CHUNK_THREADS / 64];
    __shared__ double red[SSEQ_CHUNK_THREADS / 64][2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    double v[SSEQ_TERMS_PER_THREAD];
    if (OBS) {
        for (uint32_t i = blockIdx.x; i < n_tests; i += gridDim.x) {
            const SseqRatioTest t = tests[i];
            if (t.xa == t.anchor) {
                if (tid == 0) obs[i] = 1.0;
                continue;
            }
            const bool up = t.xa > t.anchor;
            const uint64_t tt = up ? t.xa - t.anchor : t.anchor - t.xa; // local index of x_a, >= 1
            const uint64_t cl = (tt - 1) / SSEQ_CHUNK + (up ? (t.anchor + SSEQ_CHUNK - 1) / SSEQ_CHUNK : 0);
            const RatioChunk ch = ratio_chunk_of(t, cl);
            ratio_chunk_terms(t, ch, scale[t.chunk0 + cl], wtot, v);
            const uint32_t l = (uint32_t)(tt - 1 - ch.t0);
            if (l / SSEQ_TERMS_PER_THREAD == tid) {
#pragma unroll
                for (uint32_t j = 0; j < SSEQ_TERMS_PER_THREAD; j++)
                    if (j == l % SSEQ_TERMS_PER_THREAD) obs[i] = v[j];
            }
        }
    } else {
        for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
            const uint32_t i = ratio_owner(tests, n_tests, c);
            const double o = obs[i];
            if (!(isfinite(o) && o >= SSEQ_RATIO_MIN_OBS)) continue; // falls back; uniform over the workgroup
            const SseqRatioTest t = tests[i];
            const RatioChunk ch = ratio_chunk_of(t, c - t.chunk0);
            ratio_chunk_terms(t, ch, scale[c], wtot, v);
            // sar == sbr: the mirror n - x_a of the observed term equals it in exact arithmetic and is extreme whatever the two sweeps' roundings
            // made of it; its local index on this chunk's side, or 0 (no term: t >= 1) when it lies on the other side or at the anchor
            const uint64_t mk = t.n - t.xa;
            const uint64_t mt = t.sar != t.sbr ? 0 : ch.up ? (mk > t.anchor ? mk - t.anchor : 0) : (mk < t.anchor ? t.anchor - mk : 0);
            double s_all = 0.0, s_ext = 0.0;
#pragma unroll
            for (uint32_t j = 0; j < SSEQ_TERMS_PER_THREAD; j++) {
                const uint32_t l = tid * SSEQ_TERMS_PER_THREAD + j;
                if (l < ch.cnt) {
                    s_all += v[j];
                    if (v[j] <= o || ch.t0 + l + 1 == mt) s_ext += v[j];
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
                part[c] = make_double2(s_all, s_ext);
            }
            __syncthreads();
        }
    }
}

// p = Σ_ext / Σ_all (dist.rs:205-214) with the anchor's term 1.0 first, then the chunks in chunk order
__global__ void sseq_ratio_combine_kernel(const SseqRatioTest *__restrict__ tests, uint32_t n_tests, uint64_t n_chunks,
                                          const double *__restrict__ obs, const double2 *__restrict__ part, double *__restrict__ p_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tests) return;
    const double o = obs[i];
    double p = SSEQ_RATIO_FALLBACK;
    if (isfinite(o) && o >= SSEQ_RATIO_MIN_OBS) {
        const uint64_t c0 = tests[i].chunk0, c1 = i + 1 < n_tests ? tests[i + 1].chunk0 : n_chunks;
        // the anchor's own term: extreme when it is the observed one's mirror too
        double s_all = 1.0, s_ext = (1.0 <= o || (tests[i].sar == tests[i].sbr && tests[i].n - tests[i].xa == tests[i].anchor)) ? 1.0 : 0.0;
        for (uint64_t c = c0; c < c1; c++) {
            const double2 q = part[c];
            s_all += q.x;
            s_ext += q.y;
        }
        if (isfinite(s_all)) p = s_ext / s_all;
    }
    p_out[tests[i].out] = p;
}

// d_scale: n_chunks doubles, d_part: n_chunks double2, d_obs: n_tests doubles. d_p gets the p-value of every test, or
// SSEQ_RATIO_FALLBACK where the caller has to run the LogSpace kernels
void launch_sseq_ratio(hipStream_t s, const SseqRatioTest *d_tests, uint32_t n_tests, uint64_t n_chunks, double *d_obs, double *d_scale,
                       double2 *d_part, double *d_p) {
    if (!n_tests) return;
    const uint32_t chunk_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(65536, n_chunks));
    hipLaunchKernelGGL(sseq_ratio_prod_kernel, dim3(chunk_grid), dim3(SSEQ_CHUNK_THREADS), 0, s, d_tests, n_tests, n_chunks, d_scale);
    hipLaunchKernelGGL(sseq_ratio_scale_kernel, dim3((n_tests + 63) / 64), dim3(64), 0, s, d_tests, n_tests, n_chunks, d_scale);
    hipLaunchKernelGGL(sseq_ratio_terms_kernel<true>, dim3(std::min<uint32_t>(65536, n_tests)), dim3(SSEQ_CHUNK_THREADS), 0, s, d_tests, n_tests,
                       n_chunks, (const double *)d_scale, d_obs, (double2 *)nullptr);
    hipLaunchKernelGGL(sseq_ratio_terms_kernel<false>, dim3(chunk_grid), dim3(SSEQ_CHUNK_THREADS), 0, s, d_tests, n_tests, n_chunks,
                       (const double *)d_scale, d_obs, d_part);
    hipLaunchKernelGGL(sseq_ratio_combine_kernel, dim3((n_tests + 63) / 64), dim3(64), 0, s, d_tests, n_tests, n_chunks, (const double *)d_obs,
                       (const double2 *)d_part, d_p);
    SCANRS_HIP(hipGetLastError());
}
} // namespace scanrs
