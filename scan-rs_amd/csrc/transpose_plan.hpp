// transpose_plan.hpp — which sort the transposed copy of a SparseCopy runs through: host code only, no launch, no device call.
// build_transposed_copy (copy_build.hip) asks transpose_plan() and switches on the answer; scanrs_host_transpose_plan exposes the
// same function to the CPU test-suite (tests/test_construct_cpu.py), and the handle counter "transpose_route" reports the route a
// build actually took, so a GPU test can assert both (tests/test_gpu_construct.py). DESIGN.md section 3.
//
// One 64-bit key per nonzero, inner index | outer id | count, when the three fields fit together; otherwise a (u32 key, u64 value)
// pair sort. The count's width comes from the largest stored count of the source (SparseCopy::max_value: validate_copy reduces it,
// an adopted copy inherits a bound): a width below the true maximum would cut counts, so 0 ("not known") takes the full 32 bits.
#pragma once
#include <cstdint>

namespace scanrs {

enum TransposeRoute : int { TRANSPOSE_NONE = 0, TRANSPOSE_PACKED_KEY = 1, TRANSPOSE_PAIR_SORT = 2 };

struct TransposePlan {
    TransposeRoute route;
    uint32_t ib, ob, cb;          // bits of the inner index, the outer id and the count in the packed key
    uint32_t sort_begin, sort_end; // the bits of the packed key the radix sort runs over (packed route only)
};

inline uint32_t transpose_bits_for(uint64_t maxv) { // bits that hold 0 .. maxv (at least 1)
    uint32_t b = 1;
    while (b < 64 && (maxv >> b) != 0) b++;
    return b;
}

inline TransposePlan transpose_plan(uint64_t n_outer, uint64_t n_inner, uint32_t max_value) {
    TransposePlan p;
    p.ib = transpose_bits_for(n_inner ? n_inner - 1 : 0);
    p.ob = transpose_bits_for(n_outer ? n_outer - 1 : 0);
    p.cb = max_value ? transpose_bits_for(max_value) : 32u;
    p.route = p.ib + p.ob + p.cb <= 64u ? TRANSPOSE_PACKED_KEY : TRANSPOSE_PAIR_SORT;
    // The sort is stable and runs over the inner bits alone. A key that fills all 64 bits is sorted whole instead: (inner, outer)
    // occurs once, so the order is the same one, and rocprim's merge-sort comparator (inputs up to its merge_sort_limit) builds the
    // mask of a bit range that ends at bit 64 with a shift by 64 and then compares the bits BELOW the range - the copy of a
    // 65536 x 65536 matrix with a count of 2^31 or more came out ordered by outer id (tests/test_gpu_construct.py, edge_64).
    p.sort_begin = p.ob + p.cb, p.sort_end = p.ob + p.cb + p.ib;
    if (p.sort_end >= 64u) p.sort_begin = 0u, p.sort_end = 64u;
    return p;
}

} // namespace scanrs
