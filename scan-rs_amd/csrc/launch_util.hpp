// Launch and wave helpers shared by the .hip files: the checked one-thread-per-element grid, the profile scope of a launch, and
// the butterfly sums of a wave (64 lanes).
#pragma once
#include "common.hpp"

namespace scanrs {

// One thread per element. The dispatch packet's grid size is 32 bits of WORK-ITEMS (not blocks), and a launch past it silently runs
// the low 32 bits' worth — refuse instead.
inline dim3 grid1(uint64_t n, uint32_t block) {
    const uint64_t blocks = (n + block - 1) / block;
    if (blocks * block >= (1ull << 32)) fail(SCANRS_ERR_DEVICE, "a per-element launch over %llu elements exceeds the 2^32 work-items of one dispatch", (unsigned long long)n);
    return dim3((unsigned)blocks);
}

struct ProfScope {
    Storage &st;
    ProfScope(Storage &s, const char *name, double bytes, double onchip = 0.0) : st(s) {
        if (st.prof.on) st.prof.begin(st.stream, name, bytes, onchip);
    }
    ~ProfScope() {
        if (st.prof.on) st.prof.end(st.stream);
    }
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
    return v;
}

} // namespace scanrs
