// Host side of scanrs_mat_to_adaptive (`AdaptiveMat::from_csmat` run backwards, sqz/src/mat.rs:92-124): the export object, the
// download of the two arenas encode.hip fills, and the table of scanrs_adaptive_vec that points into them. The export of a whole
// scanrs_multi (multi.cpp) is the same object with one pair of arenas per shard; its host plan is here too.
#include <algorithm>
#include <cstdlib>

#include "adaptive_choose.hpp"
#include "common.hpp"

namespace scanrs {
namespace {
// A host arena from the pinned pool (device_memory.cpp). After a wait that gave up a copy may still be landing in it: it is then
// left alone instead of going back to the pool. The pool keeps four idle buffers and hands out the smallest that fits, so an arena
// below POOLED_FROM stays out of it: it would hold a handle's 72 MB staging ring for a few bytes, or fill the idle slots with
// buffers nothing else can use. Such an arena is plain heap memory, and an empty one is no allocation at all.
struct PinnedArena {
    static constexpr size_t POOLED_FROM = (size_t)1 << 20;
    void *p = nullptr;
    size_t cap = 0; // of a pooled buffer; 0: heap or the shared empty arena
    bool heap = false;
    PinnedArena() = default;
    PinnedArena(const PinnedArena &) = delete;
    PinnedArena &operator=(const PinnedArena &) = delete;
    void take(size_t bytes) {
        alignas(8) static const unsigned char nothing[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // (the table's pointers are never null)
        if (!bytes) {
            p = const_cast<unsigned char *>(nothing);
        } else if (bytes < POOLED_FROM) {
            p = std::malloc(bytes);
            if (!p) fail(SCANRS_ERR_DEVICE, "out of host memory");
            heap = true;
        } else {
            p = pinned_take(bytes, &cap);
        }
    }
    ~PinnedArena() {
        if (heap)
            std::free(p);
        else if (cap && !device_lost())
            pinned_give(p, cap);
    }
};
} // namespace
} // namespace scanrs

struct scanrs_adaptive_export {
    std::vector<scanrs_adaptive_vec> vecs;
    // one pair of host arenas per part: the single one of scanrs_mat_to_adaptive, one per shard of scanrs_multi_to_adaptive
    struct Part {
        scanrs::PinnedArena bytes, words;
        uint64_t total_bytes = 0;
        uint64_t kind_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    };
    std::vector<std::unique_ptr<Part>> parts;
    uint64_t total_bytes = 0;
    uint64_t kind_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // what scanrs_multi_to_adaptive did (scanrs_adaptive_export_multi_info); null on an export of a single handle
    struct MultiInfo {
        std::vector<uint64_t> slab_bounds, moved, arena_bytes;
    };
    std::unique_ptr<MultiInfo> multi;
};

namespace scanrs {

scanrs_adaptive_export *adaptive_export_new(uint64_t n_vecs, uint32_t n_parts) {
    std::unique_ptr<scanrs_adaptive_export> e(new scanrs_adaptive_export());
    e->vecs.resize(n_vecs);
    if (n_vecs) std::memset(e->vecs.data(), 0, n_vecs * sizeof(scanrs_adaptive_vec));
    for (uint32_t i = 0; i < n_parts; i++) e->parts.emplace_back(new scanrs_adaptive_export::Part());
    return e.release();
}

void adaptive_export_encode(scanrs_adaptive_export *e, uint32_t part, Storage &st, const SparseCopy &cp, int force_kind, uint64_t first_vec,
                            uint64_t *arena_bytes) {
    scanrs_adaptive_export::Part &pt = *e->parts[part];
    if (first_vec + cp.n_outer > e->vecs.size()) fail(SCANRS_ERR_DEVICE, "internal: an export part does not fit the table");
    std::vector<EncodedVec> vecs;
    std::vector<uint64_t> byte_off, word_off;
    {
        DevBuf<uint64_t> d_bytes;
        DevBuf<uint32_t> d_words;
        encode_adaptive_vectors(st, cp, force_kind, vecs, byte_off, word_off, d_bytes, d_words);
        const uint64_t n_bytes = byte_off[cp.n_outer], n_words = word_off[cp.n_outer];
        pt.bytes.take(n_bytes);
        pt.words.take(n_words * 4);
        // one copy per arena, straight into the pinned memory the export owns
        if (n_bytes) SCANRS_HIP(hipMemcpyAsync(pt.bytes.p, d_bytes.p, n_bytes, hipMemcpyDeviceToHost, st.stream));
        if (n_words) SCANRS_HIP(hipMemcpyAsync(pt.words.p, d_words.p, n_words * 4, hipMemcpyDeviceToHost, st.stream));
        SCANRS_SYNC(st.stream);
        if (arena_bytes) *arena_bytes = n_bytes + n_words * 4;
        d_bytes.release();
        d_words.release();
        device_free_flush();
    }
    const uint64_t len = cp.n_inner, n_bs = adaptive::n_block_starts(len);
    const uint8_t *hb = static_cast<const uint8_t *>(pt.bytes.p);
    const uint32_t *hw = static_cast<const uint32_t *>(pt.words.p);
    for (uint64_t o = 0; o < cp.n_outer; o++) {
        const EncodedVec &d = vecs[o];
        scanrs_adaptive_vec &v = e->vecs[first_vec + o];
        std::memset(&v, 0, sizeof v);
        v.kind = d.kind;
        v.len = len;
        v.n_fallback = d.n_fb;
        v.fallback_indexes = hw + word_off[o];
        v.fallback_values = hw + word_off[o] + d.n_fb;
        pt.kind_counts[d.kind]++;
        if (d.kind == adaptive::V) {
            v.n_units = d.n;
            pt.total_bytes += 8ull * d.n;
            continue;
        }
        v.n_units = adaptive::is_dense(d.kind) ? len : d.n;
        v.data = hb + byte_off[o];
        v.data_bytes = adaptive::data_bytes(d.kind, v.n_units);
        pt.total_bytes += v.data_bytes + 8ull * d.n_fb;
        if (adaptive::is_sparse(d.kind)) {
            v.index_bytes = hb + byte_off[o] + ((v.data_bytes + 7ull) & ~7ull);
            v.block_starts = hw + word_off[o] + 2ull * d.n_fb;
            v.n_block_starts = n_bs;
            pt.total_bytes += d.n + 4ull * n_bs;
        }
    }
}

static void sum_parts(scanrs_adaptive_export *e) {
    e->total_bytes = 0;
    std::memset(e->kind_counts, 0, sizeof e->kind_counts);
    for (const auto &pt : e->parts) {
        e->total_bytes += pt->total_bytes;
        for (int k = 0; k < 8; k++) e->kind_counts[k] += pt->kind_counts[k];
    }
}

void adaptive_export_finish(scanrs_adaptive_export *e, const std::vector<uint64_t> &slab_bounds, const std::vector<uint64_t> &moved,
                            const std::vector<uint64_t> &arena_bytes) {
    sum_parts(e);
    e->multi.reset(new scanrs_adaptive_export::MultiInfo{slab_bounds, moved, arena_bytes});
}

void adaptive_check_export_args(const void *handle, int major, int force_kind, scanrs_adaptive_export **out) {
    if (out) *out = nullptr;
    if (!handle || !out) fail(SCANRS_ERR_ARGUMENT, "null argument");
    if (major != SCANRS_EXPORT_STORED && major != SCANRS_EXPORT_INNER)
        fail(SCANRS_ERR_ARGUMENT, "major must be 0 (SCANRS_EXPORT_STORED: one vector per stored outer vector) or 1 (SCANRS_EXPORT_INNER: one per inner position)");
    if (force_kind < -1 || force_kind > 7) fail(SCANRS_ERR_ARGUMENT, "force_kind must be -1 (choose_storage) or 0..7 (D3, D4, D8, D16, V, S3, S4, S8)");
}

void export_host_plan(const uint64_t *counts, uint32_t n_src, uint64_t n_inner, uint32_t n_dst, uint64_t *out_indptr, uint64_t *slab_bounds,
                      uint64_t *moved) {
    if (n_src == 0 || n_src > REGATHER_MAX_SHARDS) fail(SCANRS_ERR_ARGUMENT, "n_src: 1 <= n_src <= 16 is required (%u given)", n_src);
    if (n_dst == 0 || n_dst > REGATHER_MAX_SHARDS) fail(SCANRS_ERR_ARGUMENT, "n_dst: 1 <= n_dst <= 16 is required (%u given)", n_dst);
    if (n_inner && !counts) fail(SCANRS_ERR_ARGUMENT, "counts: null table");
    std::vector<uint64_t> tip(n_inner + 1, 0), sb(n_dst + 1, 0);
    for (uint32_t s = 0; s < n_src; s++)
        for (uint64_t g = 0; g < n_inner; g++) tip[g + 1] += counts[(uint64_t)s * n_inner + g];
    for (uint64_t g = 0; g < n_inner; g++) tip[g + 1] += tip[g];
    if (scanrs_plan_shards(tip.data(), n_inner, n_dst, sb.data()) != SCANRS_OK) throw Failure{SCANRS_ERR_ARGUMENT};
    if (out_indptr) std::copy(tip.begin(), tip.end(), out_indptr);
    if (slab_bounds) std::copy(sb.begin(), sb.end(), slab_bounds);
    if (moved)
        for (uint32_t s = 0; s < n_src; s++)
            for (uint32_t d = 0; d < n_dst; d++) {
                uint64_t z = 0;
                for (uint64_t g = sb[d]; g < sb[d + 1]; g++) z += counts[(uint64_t)s * n_inner + g];
                moved[(uint64_t)s * n_dst + d] = z;
            }
}

} // namespace scanrs

using namespace scanrs;

extern "C" {
int scanrs_mat_to_adaptive_major(scanrs_mat *m, int major, int force_kind, scanrs_adaptive_export **out) {
    return guard([&] {
        adaptive_check_export_args(m, major, force_kind, out);
        Storage &st = *m->st;
        if (major == SCANRS_EXPORT_INNER && st.shard.active())
            fail(SCANRS_ERR_ARGUMENT, "to_adaptive: a sharded handle holds its own outer vectors only, so the vectors of the inner dimension are not whole on one rank; scanrs_multi_to_adaptive(mm, SCANRS_EXPORT_INNER, ...) exports them");
        need_device();
        CurrentHandle cur(&st);
        // a transposed view's storage flag is the other one: the same arrays (as scanrs_mat_to_csmat). INNER: the handle's other copy,
        // built on first use as the products build it
        const SparseCopy &cp = major == SCANRS_EXPORT_INNER ? st.copy_with_outer_rows(st.storage != SCANRS_CSR) : st.primary;
        std::unique_ptr<scanrs_adaptive_export> e(adaptive_export_new(cp.n_outer, 1));
        adaptive_export_encode(e.get(), 0, st, cp, force_kind, 0, nullptr);
        sum_parts(e.get());
        *out = e.release();
    });
}
int scanrs_mat_to_adaptive(scanrs_mat *m, int force_kind, scanrs_adaptive_export **out) {
    return scanrs_mat_to_adaptive_major(m, SCANRS_EXPORT_STORED, force_kind, out);
}
int scanrs_adaptive_export_multi_info(const scanrs_adaptive_export *e, uint32_t *n_shards, uint64_t *slab_bounds, uint64_t *moved, uint64_t *arena_bytes) {
    return guard([&] {
        if (!e) fail(SCANRS_ERR_ARGUMENT, "null export");
        if (!e->multi) fail(SCANRS_ERR_ARGUMENT, "export_multi_info: this export was not made by scanrs_multi_to_adaptive");
        const scanrs_adaptive_export::MultiInfo &info = *e->multi;
        if (n_shards) *n_shards = (uint32_t)info.arena_bytes.size();
        if (slab_bounds) std::copy(info.slab_bounds.begin(), info.slab_bounds.end(), slab_bounds);
        if (moved) std::copy(info.moved.begin(), info.moved.end(), moved);
        if (arena_bytes) std::copy(info.arena_bytes.begin(), info.arena_bytes.end(), arena_bytes);
    });
}
int scanrs_host_plan_export(const uint64_t *counts, uint32_t n_src, uint64_t n_inner, uint32_t n_dst, uint64_t *out_indptr, uint64_t *slab_bounds,
                            uint64_t *moved) {
    return guard([&] { export_host_plan(counts, n_src, n_inner, n_dst, out_indptr, slab_bounds, moved); });
}
int scanrs_adaptive_export_info(const scanrs_adaptive_export *e, uint64_t *n_vecs, uint64_t *total_bytes, uint64_t kind_counts[8]) {
    return guard([&] {
        if (!e) fail(SCANRS_ERR_ARGUMENT, "null export");
        if (n_vecs) *n_vecs = e->vecs.size();
        if (total_bytes) *total_bytes = e->total_bytes;
        if (kind_counts) std::memcpy(kind_counts, e->kind_counts, sizeof e->kind_counts);
    });
}
int scanrs_adaptive_export_vecs(const scanrs_adaptive_export *e, const scanrs_adaptive_vec **vecs) {
    return guard([&] {
        if (!e || !vecs) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *vecs = e->vecs.data();
    });
}
void scanrs_adaptive_export_free(scanrs_adaptive_export *e) { delete e; }

int scanrs_host_choose_storage(uint64_t len, const uint32_t *values, uint64_t n, int *kind, uint64_t *min_size) {
    return guard([&] {
        if ((n && !values) || !kind) fail(SCANRS_ERR_ARGUMENT, "null argument");
        uint64_t over[4] = {0, 0, 0, 0};
        for (uint64_t i = 0; i < n; i++)
            for (uint32_t w = 0; w < 4u; w++) over[w] += values[i] >= adaptive::marker_of(w);
        *kind = (int)adaptive::choose_storage(len, n, over, min_size);
    });
}
} // extern "C"
