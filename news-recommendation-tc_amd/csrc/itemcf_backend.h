// itemcf_backend.h -- internal (non-ABI) access to the recall back end that
// itemcf.hip defines: the stable (key, slot) radix sort, the ordered
// per-(query, item) sums, the hot fill and the stable top-k.  A recall channel
// writes its candidates in rc_cand_kernel's format -- key (q << bj | item) or
// the sentinel for an item of the query's own history, the global sequence
// number, the contribution -- into the buffers rc_back_buffers names, then
// calls rc_back_finish.  usercf.hip is the second user.
#pragma once

#include <cmath>

#include "nrk_common.h"

namespace nrk {

// alpha^x as exp(x ln alpha), ln alpha formed once on the host (the note above
// their use in itemcf.hip has the error bound); ln is NaN (-> the device pow)
// unless alpha is positive and finite
static inline double cf_ln(double alpha) {
    return alpha > 0.0 && std::isfinite(alpha) ? std::log(alpha) : NAN;
}
__device__ __forceinline__ double cf_apow(double alpha, double ln_alpha, double x) {
    return ln_alpha == ln_alpha ? exp(x * ln_alpha) : pow(alpha, x);
}

struct RcBack {
    uint64_t* keys;   // [n_cand] key per candidate
    int32_t* slots;   // [n_cand] global sequence number (= its index)
    double* contrib;  // [n_cand] contribution
    uint64_t sentinel;
    int bj;           // key = q << bj | item
};

size_t rc_back_bytes(int64_t n_cand);
// false: n_query * n_items does not fit a 64-bit key
bool rc_back_buffers(void* workspace, int64_t n_query, int32_t n_items, int64_t n_cand, RcBack* out);
// Everything after the candidates are written (same stream).  offsets / items:
// the query users' histories (hot-fill exclusion); q_slot < 0: cold start.
// Returns NRK_OK or NRK_EHIP (message set).
int rc_back_finish(const int64_t* q_slot, int64_t n_query, const int64_t* offsets, const int32_t* items,
                   int32_t n_items, const int32_t* hot, int n_hot, const int64_t* cand_off, int64_t n_cand, int topk,
                   int32_t* out_items, double* out_scores, int32_t* out_src, int32_t* out_cnt, void* workspace,
                   hipStream_t s);
// in-place exclusive int64 scan, v[n] = total (one workgroup, no workspace)
void rc_scan_exclusive(int64_t* v, int64_t n, hipStream_t s);
// the largest topn / topk of the back end, and of nrk_itemcf_recall's n_cand
constexpr int RC_TOPK_MAX = 2048;
constexpr int64_t RC_CAND_MAX = (int64_t(1) << 31) - 4096;

}  // namespace nrk
