// tower_common.h -- the YouTubeDNN user tower's shape contract, the dispatch
// on the embedding dim and the history-mean gather, shared by the forward
// (tower.hip) and the training step (tower_train.hip).
#pragma once

#include <type_traits>

#include "nrk_common.h"

namespace nrk {

// user_tower = [Linear(in_l, w_l), ReLU, Dropout] per layer
// (youtubednn_hidden_units is a list, youtubednn_recaller.py:105-112)
constexpr int TT_MAXL = 8, TT_MAXW = 256;
struct TtLayers {
    int n;
    int w[TT_MAXL];
};

constexpr const char* TT_LAST_WIDTH = "last hidden width must equal the embedding dim "
                                      "(youtubednn_recaller.py:461-465)";

// The contract: dim in {16, 32, 64} and, where the entry point takes a layer
// list (ly != nullptr, filled here), 1 to 8 layers of width 1 to 256, the
// last one dim wide.  fn names the entry point in the error.
static inline int tt_check_shape(const char* fn, int dim, int n_layers = 0, const int* widths = nullptr,
                                 TtLayers* ly = nullptr) {
    if (!(dim == 16 || dim == 32 || dim == 64)) return fail_as(fn, NRK_EUNSUPPORTED, "dim must be 16, 32 or 64");
    if (!ly) return NRK_OK;
    if (!widths) return fail_as(fn, NRK_EINVAL, "null widths");
    if (n_layers < 1 || n_layers > TT_MAXL) return fail_as(fn, NRK_EUNSUPPORTED, "1 to 8 hidden layers are compiled");
    ly->n = n_layers;
    for (int l = 0; l < n_layers; ++l) {
        if (widths[l] < 1 || widths[l] > TT_MAXW)
            return fail_as(fn, NRK_EUNSUPPORTED, "hidden widths must be in [1, 256]");
        ly->w[l] = widths[l];
    }
    if (widths[n_layers - 1] != dim) return fail_as(fn, NRK_EINVAL, TT_LAST_WIDTH);
    return NRK_OK;
}

// f(integral_constant<int, dim>), and what it returns, for a dim that passed
// tt_check_shape
template <class F>
static inline auto tt_for_dim(int dim, F&& f) {
    if (dim == 16) return f(std::integral_constant<int, 16>{});
    if (dim == 32) return f(std::integral_constant<int, 32>{});
    return f(std::integral_constant<int, 64>{});
}

// Mean of a user's first len history rows, one wave: lane t holds the row
// index of slot t in hv (valid for t < tmax, len <= tmax <= 64).  Lane
// d = lane % D of phase ph = lane / D adds the rows t = ph, ph + P, ...
// (P = 64 / D rows per round, t ascending), the phases are folded by an xor
// butterfly, and every lane returns sum[d] / (len + 1e-8f).  A slot past len
// loads row 0 and is not added: the training kernel used to load its user's
// first history row for such a slot and did not add it either, so the sums
// are the same bits.  tt_user_kernel keeps a software-pipelined form of this.
template <int D>
__device__ __forceinline__ float tt_hist_mean(const float* __restrict__ item_table, int32_t hv, int len, int tmax,
                                              int lane) {
    constexpr int P = WAVE / D;
    const int d = lane % D, ph = lane / D;
    float sum = 0.0f;
    const int nit = (len + P - 1) / P;  // wave-uniform
    for (int i = 0; i < nit; ++i) {
        const int t = ph + P * i;
        const int32_t r = __shfl(hv, t < tmax ? t : 0, WAVE);
        const float v = item_table[(int64_t)(t < len ? r : 0) * D + d];
        if (t < len) sum += v;  // t ascending
    }
#pragma unroll
    for (int off = D; off < WAVE; off <<= 1) sum += __shfl_xor(sum, off, WAVE);
    return sum / ((float)len + 1e-8f);
}

}  // namespace nrk
