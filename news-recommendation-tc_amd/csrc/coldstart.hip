// coldstart.hip -- ColdStartRecaller on gfx950.
//
// Reference: src/recall/coldstart_recaller.py.  _apply_filtering (:54-126)
// walks every (user, candidate) pair of a base recall in Python and keeps the
// pairs that pass four rules -- the item's category is in the user's history,
// the item was never clicked, its word count is within 200 of the user's
// mean, its (normalised) creation time within 0.25 of the user's last click's
// -- and recall (:128-147) sorts a user's survivors stably by score.
//
// Layout (built by nrk/recall/coldstart_recaller.py): the lists as a CSR over
// dense item rows, one profile row per list, four item tables (about 21 bytes
// per item: they stay in cache; the list stream is the traffic).  One wave
// per list walks it in 64-entry chunks; cs_keep is the one predicate both
// kernels share.  The filter writes a byte per pair and a count per list;
// the recall compacts the survivors (ballot + prefix, so they stay in list
// order) into the wave's LDS as (score, position) and ranks them with the
// wave LDS bitonic sort on (score desc, position asc), which is Python's
// stable descending sort: IEEE == puts -0.0 and +0.0 in one tie.
// A few gathers and fp64 compares per pair: latency-bound, no MFMA.
#include "nrk_common.h"

namespace nrk {

constexpr int CS_MAX = 2048;  // survivors per user, and topk (CF_TOPK_MAX, FUSE_WMAX)

struct CsTables {
    const int64_t* cat_off;      // [n_prof + 1]
    const int32_t* cat;          // every user's category codes, ascending
    const double* mean_words;    // [n_prof]
    const double* last_created;  // [n_prof]
    int64_t n_prof;
    const int32_t* item_type;    // [n_items]
    const double* item_words;
    const double* item_created;
    const uint8_t* item_clicked;
    int64_t n_items;
    double words_tol, time_tol;
};

// one list's profile row, read once per wave
struct CsProfile {
    int64_t c0, c1;  // the user's slice of cat
    double mean_words, last_created;
};

__device__ __forceinline__ CsProfile cs_profile(const CsTables& t, int32_t p) {
    return CsProfile{t.cat_off[p], t.cat_off[p + 1], t.mean_words[p], t.last_created[p]};
}

// The four rules for one pair (:86-115).  `it` is an item row or -1; a row
// outside the tables counts as missing.  The negated > keeps a pair whose
// mean or time is NaN, as the reference's comparison does.  The rules are
// independent, so they run narrowest table first: the clicked byte and the
// category (5 bytes per item) settle most pairs before the two f64 gathers.
__device__ __forceinline__ bool cs_keep(const CsTables& t, const CsProfile& u, int32_t it) {
    if (it < 0 || it >= t.n_items) return false;
    const uint8_t clicked = t.item_clicked[it];
    const int32_t ty = t.item_type[it];  // both gathers in flight together
    if (clicked) return false;
    int64_t lo = u.c0, hi = u.c1;
    while (lo < hi) {  // first code >= ty
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (t.cat[mid] < ty) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= u.c1 || t.cat[lo] != ty) return false;
    const double words = t.item_words[it], created = t.item_created[it];
    return !(fabs(words - u.mean_words) > t.words_tol) && !(fabs(created - u.last_created) > t.time_tol);
}

// one wave per list, four lists per workgroup
__global__ __launch_bounds__(256) void coldstart_filter_kernel(
    const int64_t* __restrict__ list_off, int64_t n_lists, const int32_t* __restrict__ item,
    const int32_t* __restrict__ prof, CsTables t, uint8_t* __restrict__ keep, int32_t* __restrict__ kept) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int64_t l = (int64_t)blockIdx.x * 4 + wv; l < n_lists; l += (int64_t)gridDim.x * 4) {
        const int64_t b = list_off[l], n = list_off[l + 1] - b;
        const int32_t p = prof[l];
        const bool known = p >= 0 && p < t.n_prof;  // wave-uniform
        CsProfile u{0, 0, 0.0, 0.0};
        if (known) u = cs_profile(t, p);
        int cnt = 0;
        for (int64_t base = 0; base < n; base += WAVE) {
            const int64_t i = base + lane;
            const bool k = i < n && known && cs_keep(t, u, item[b + i]);
            if (i < n) keep[b + i] = k ? 1 : 0;
            cnt += __popcll(__ballot(k));
        }
        if (lane == 0) kept[l] = cnt;
    }
}

// one wave per query user; x [nw] Cands of dynamic LDS, nw = pow2_at_least(cap, 64)
__global__ __launch_bounds__(64) void coldstart_recall_kernel(
    const int64_t* __restrict__ q, int64_t n_query, const int64_t* __restrict__ list_off, int64_t n_lists,
    const int32_t* __restrict__ item, const double* __restrict__ score, const int32_t* __restrict__ prof,
    CsTables t, int cap, int topk, int32_t* __restrict__ out_pos, double* __restrict__ out_score,
    int32_t* __restrict__ out_cnt) {
    extern __shared__ __attribute__((aligned(16))) uint8_t dyn[];
    Cand* x = reinterpret_cast<Cand*>(dyn);
    const int lane = threadIdx.x;
    for (int64_t qi = blockIdx.x; qi < n_query; qi += gridDim.x) {
        const int64_t l = q[qi];
        int cnt = 0;  // survivors, wave-uniform
        if (l >= 0 && l < n_lists) {
            const int64_t b = list_off[l], n = list_off[l + 1] - b;
            const int32_t p = prof[l];
            if (p >= 0 && p < t.n_prof) {
                const CsProfile u = cs_profile(t, p);
                for (int64_t base = 0; base < n; base += WAVE) {
                    const int64_t i = base + lane;
                    const bool k = i < n && cs_keep(t, u, item[b + i]);
                    const unsigned long long m = __ballot(k);
                    const int slot = cnt + __popcll(m & ((1ull << lane) - 1ull));
                    if (k && slot < cap) x[slot] = Cand{score[b + i], (int32_t)i};
                    cnt += __popcll(m);
                }
            }
        }
        const bool over = cnt > cap;
        int ns = 0;  // sorted slots
        if (!over && cnt > 0) {
            ns = WAVE;
            while (ns < cnt) ns <<= 1;  // <= nw: cnt <= cap
            for (int i = cnt + lane; i < ns; i += WAVE) x[i] = Cand{-INFINITY, INT32_MAX};
            wave_lds_sort(x, ns);
        }
        const int have = over ? 0 : cnt;
        for (int i = lane; i < topk; i += WAVE) {
            const bool ok = i < have;
            out_pos[qi * topk + i] = ok ? x[i].row : -1;
            out_score[qi * topk + i] = ok ? x[i].s : 0.0;
        }
        if (lane == 0) out_cnt[qi] = over ? -1 : (cnt < topk ? cnt : topk);
        wave_sync_lds();  // the next user's survivors overwrite x
    }
}

// the size and pointer checks both entry points share; fn names the caller
static int cs_check(const char* fn, const int64_t* list_off, int64_t n_lists, const int32_t* item,
                    int64_t n_entries, const int32_t* prof, const int64_t* cat_off, const int32_t* cat,
                    int64_t n_cat, const double* mean_words, const double* last_created, int64_t n_prof,
                    const int32_t* item_type, const double* item_words, const double* item_created,
                    const uint8_t* item_clicked, int64_t n_items) {
    if (n_lists < 0 || n_entries < 0 || n_cat < 0 || n_prof < 0 || n_items < 0)
        return fail_as(fn, NRK_EINVAL, "negative size");
    if (n_entries >= (1ll << 31) || n_prof >= (1ll << 31) || n_items >= (1ll << 31))
        return fail_as(fn, NRK_EINVAL, "n_entries, n_prof and n_items must be < 2^31");
    if (!list_off || !cat_off || (n_lists > 0 && !prof) || (n_entries > 0 && !item) || (n_cat > 0 && !cat) ||
        (n_prof > 0 && !(mean_words && last_created)) ||
        (n_items > 0 && !(item_type && item_words && item_created && item_clicked)))
        return fail_as(fn, NRK_EINVAL, "null pointer");
    return NRK_OK;
}

}  // namespace nrk

using namespace nrk;

extern "C" {

int nrk_coldstart_filter(const int64_t* list_off, int64_t n_lists, const int32_t* item, int64_t n_entries,
                         const int32_t* prof, const int64_t* cat_off, const int32_t* cat, int64_t n_cat,
                         const double* mean_words, const double* last_created, int64_t n_prof,
                         const int32_t* item_type, const double* item_words, const double* item_created,
                         const uint8_t* item_clicked, int64_t n_items, double words_tol, double time_tol,
                         uint8_t* keep, int32_t* kept, nrk_stream_t stream) {
    clear_error();
    const int rc = cs_check(__func__, list_off, n_lists, item, n_entries, prof, cat_off, cat, n_cat, mean_words,
                            last_created, n_prof, item_type, item_words, item_created, item_clicked, n_items);
    if (rc != NRK_OK) return rc;
    NRK_REQUIRE(kept || n_lists == 0, "null pointer");
    NRK_REQUIRE(keep || n_entries == 0, "null pointer");
    if (n_lists == 0) return NRK_OK;
    const CsTables t{cat_off,    cat,          mean_words,   last_created, n_prof,   item_type,
                     item_words, item_created, item_clicked, n_items,      words_tol, time_tol};
    coldstart_filter_kernel<<<grid_for(n_lists, 4, 1 << 20), 256, 0, as_stream(stream)>>>(list_off, n_lists, item,
                                                                                         prof, t, keep, kept);
    NRK_CHECK_LAUNCH();
    return NRK_OK;
}

int nrk_coldstart_recall(const int64_t* q, int64_t n_query, const int64_t* list_off, int64_t n_lists,
                         const int32_t* item, const double* score, int64_t n_entries, const int32_t* prof,
                         const int64_t* cat_off, const int32_t* cat, int64_t n_cat, const double* mean_words,
                         const double* last_created, int64_t n_prof, const int32_t* item_type,
                         const double* item_words, const double* item_created, const uint8_t* item_clicked,
                         int64_t n_items, double words_tol, double time_tol, int cap, int topk, int32_t* out_pos,
                         double* out_score, int32_t* out_cnt, nrk_stream_t stream) {
    clear_error();
    NRK_REQUIRE(n_query >= 0, "negative size");
    NRK_REQUIRE(topk >= 1 && topk <= CS_MAX, "topk must be in [1, 2048]");
    NRK_REQUIRE(cap >= 1 && cap <= CS_MAX, "cap must be in [1, 2048]");
    const int rc = cs_check(__func__, list_off, n_lists, item, n_entries, prof, cat_off, cat, n_cat, mean_words,
                            last_created, n_prof, item_type, item_words, item_created, item_clicked, n_items);
    if (rc != NRK_OK) return rc;
    if (n_query == 0) return NRK_OK;
    NRK_REQUIRE(q && out_pos && out_score && out_cnt && (score || n_entries == 0), "null pointer");
    const CsTables t{cat_off,    cat,          mean_words,   last_created, n_prof,   item_type,
                     item_words, item_created, item_clicked, n_items,      words_tol, time_tol};
    // at most CS_MAX Cands: 32 KB, inside the default dynamic-LDS limit
    const size_t lds = (size_t)pow2_at_least(cap, WAVE) * sizeof(Cand);
    static_assert(pow2_at_least(CS_MAX, WAVE) * sizeof(Cand) <= 65536, "coldstart_recall_kernel LDS");
    coldstart_recall_kernel<<<grid_for(n_query, 1, 1 << 20), 64, lds, as_stream(stream)>>>(
        q, n_query, list_off, n_lists, item, score, prof, t, cap, topk, out_pos, out_score, out_cnt);
    NRK_CHECK_LAUNCH();
    return NRK_OK;
}

}  // extern "C"
