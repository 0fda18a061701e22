// Host side of scanrs_mat_to_adaptive (`AdaptiveMat::from_csmat` run backwards, sqz/src/mat.rs:92-124): the export object, the
// download of the two arenas encode.hip fills, and the table of scanrs_adaptive_vec that points into them.
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
    scanrs::PinnedArena bytes, words;
    uint64_t total_bytes = 0;
    uint64_t kind_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

using namespace scanrs;

extern "C" {
int scanrs_mat_to_adaptive(scanrs_mat *m, int force_kind, scanrs_adaptive_export **out) {
    return guard([&] {
        if (!m || !out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *out = nullptr;
        if (force_kind < -1 || force_kind > 7) fail(SCANRS_ERR_ARGUMENT, "force_kind must be -1 (choose_storage) or 0..7 (D3, D4, D8, D16, V, S3, S4, S8)");
        need_device();
        Storage &st = *m->st;
        const SparseCopy &cp = st.primary; // a transposed view's storage flag is the other one: the same arrays (as scanrs_mat_to_csmat)
        std::unique_ptr<scanrs_adaptive_export> e(new scanrs_adaptive_export());
        std::vector<EncodedVec> vecs;
        std::vector<uint64_t> byte_off, word_off;
        {
            CurrentHandle cur(&st);
            DevBuf<uint64_t> d_bytes;
            DevBuf<uint32_t> d_words;
            encode_adaptive_vectors(st, cp, force_kind, vecs, byte_off, word_off, d_bytes, d_words);
            const uint64_t n_bytes = byte_off[cp.n_outer], n_words = word_off[cp.n_outer];
            e->bytes.take(n_bytes);
            e->words.take(n_words * 4);
            // one copy per arena, straight into the pinned memory the export owns
            if (n_bytes) SCANRS_HIP(hipMemcpyAsync(e->bytes.p, d_bytes.p, n_bytes, hipMemcpyDeviceToHost, st.stream));
            if (n_words) SCANRS_HIP(hipMemcpyAsync(e->words.p, d_words.p, n_words * 4, hipMemcpyDeviceToHost, st.stream));
            SCANRS_SYNC(st.stream);
            d_bytes.release();
            d_words.release();
            device_free_flush();
        }
        const uint64_t len = cp.n_inner, n_bs = adaptive::n_block_starts(len);
        const uint8_t *hb = static_cast<const uint8_t *>(e->bytes.p);
        const uint32_t *hw = static_cast<const uint32_t *>(e->words.p);
        e->vecs.resize(cp.n_outer);
        for (uint64_t o = 0; o < cp.n_outer; o++) {
            const EncodedVec &d = vecs[o];
            scanrs_adaptive_vec &v = e->vecs[o];
            std::memset(&v, 0, sizeof v);
            v.kind = d.kind;
            v.len = len;
            v.n_fallback = d.n_fb;
            v.fallback_indexes = hw + word_off[o];
            v.fallback_values = hw + word_off[o] + d.n_fb;
            e->kind_counts[d.kind]++;
            if (d.kind == adaptive::V) {
                v.n_units = d.n;
                e->total_bytes += 8ull * d.n;
                continue;
            }
            v.n_units = adaptive::is_dense(d.kind) ? len : d.n;
            v.data = hb + byte_off[o];
            v.data_bytes = adaptive::data_bytes(d.kind, v.n_units);
            e->total_bytes += v.data_bytes + 8ull * d.n_fb;
            if (adaptive::is_sparse(d.kind)) {
                v.index_bytes = hb + byte_off[o] + ((v.data_bytes + 7ull) & ~7ull);
                v.block_starts = hw + word_off[o] + 2ull * d.n_fb;
                v.n_block_starts = n_bs;
                e->total_bytes += d.n + 4ull * n_bs;
            }
        }
        *out = e.release();
    });
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
