// `AdaptiveVec::choose_storage` (sqz/src/vec.rs:1086-1131) and the sizes of the pieces of each encoding, written once for host and
// device: the same source runs in the plan kernel of encode.hip and behind scanrs_host_choose_storage, which the CPU test-suite
// checks against the oracle.
//
// The choice needs five numbers per vector: the stored entries n and how many of their values reach 7, 15, 255 and 65535 (the
// markers of the 3-, 4-, 8- and 16-bit fields: a value at or above the marker goes to the fallback list, 8 bytes an entry).
#pragma once
#include <cstdint>

#ifndef SCANRS_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SCANRS_HD __host__ __device__
#else
#define SCANRS_HD
#endif
#endif

namespace scanrs {
namespace adaptive {

enum : uint32_t { D3 = 0, D4, D8, D16, V, S3, S4, S8 }; // declaration order of `enum AdaptiveVec` (vec.rs:1029-1053)

// field width class of an encoding: 0 = 3 bits, 1 = 4 bits, 2 = 8 bits, 3 = 16 bits (V has no fields)
SCANRS_HD inline uint32_t width_of(uint32_t kind) { return kind == D3 || kind == S3 ? 0u : kind == D4 || kind == S4 ? 1u : kind == D16 ? 3u : 2u; }
SCANRS_HD inline uint32_t marker_of(uint32_t width) { return width == 0 ? 7u : width == 1 ? 15u : width == 2 ? 255u : 65535u; }
SCANRS_HD inline uint32_t bits_of(uint32_t width) { return width == 0 ? 3u : width == 1 ? 4u : width == 2 ? 8u : 16u; }
SCANRS_HD inline uint32_t fields_per_u64(uint32_t width) { return width == 0 ? 21u : width == 1 ? 16u : width == 2 ? 8u : 4u; }
SCANRS_HD inline bool is_dense(uint32_t kind) { return kind <= D16; }
SCANRS_HD inline bool is_sparse(uint32_t kind) { return kind >= S3; }

// bytes of `data` over L fields (L = len for D*, the stored entries for S*): Dense3::construct, Dense4::construct, DenseW::construct
SCANRS_HD inline uint64_t data_bytes(uint32_t kind, uint64_t L) {
    switch (width_of(kind)) {
    case 0: return 8ull * (L / 21ull + 1ull);
    case 1: return L / 2ull + 1ull;
    case 2: return L;
    default: return 2ull * L;
    }
}
// entries of `block_starts` (CompressedIndexSparse::construct, vec.rs:335-397)
SCANRS_HD inline uint64_t n_block_starts(uint64_t len) {
    const uint64_t blocks = (len + 255ull) / 256ull;
    return (blocks ? blocks : 1ull) + 1ull;
}

// over[w]: stored values >= marker_of(w). Returns the kind; *min_size is the second member of the reference's result: the smallest
// estimate among D3, D4, D8, D16, S3, S4 (the S8 and V branches change the kind without lowering it, vec.rs:1120-1128).
SCANRS_HD inline uint32_t choose_storage(uint64_t len, uint64_t n, const uint64_t over[4], uint64_t *min_size) {
    const uint64_t blocks = (len / 256ull) * 4ull;                 // CompressedIndexSparse::estimate_size, vec.rs:327-333
    uint32_t opt = D3;
    uint64_t best = (len / 21ull + 1ull) * 8ull + over[0] * 8ull;  // Dense3, vec.rs:965-970
    uint64_t sz = len / 2ull + over[1] * 8ull;                     // Dense4, vec.rs:830-835
    if (sz < best) opt = D4, best = sz;
    sz = len + over[2] * 8ull;                                     // DenseW<u8>, vec.rs:723-728
    if (sz < best) opt = D8, best = sz;
    sz = 2ull * len + over[3] * 8ull;                              // DenseW<u16>
    if (sz < best) opt = D16, best = sz;
    sz = (n / 21ull + 1ull) * 8ull + over[0] * 8ull + n + blocks;
    if (sz < best) opt = S3, best = sz;
    sz = n / 2ull + over[1] * 8ull + n + blocks;
    if (sz < best) opt = S4, best = sz;
    sz = n + over[2] * 8ull + n + blocks;
    if (sz < best) opt = S8; // `best` stays (vec.rs:1120-1123)
    if (n * 8ull < best) opt = V;
    if (min_size) *min_size = best;
    return opt;
}

} // namespace adaptive
} // namespace scanrs
