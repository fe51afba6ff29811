// profile.hip -- user profiles, item popularity, MinMax columns and labels on
// gfx950.
//
// Reference: src/features/feature_extractor.py.  _extract_user_profile_features
// (:296-389) makes five per-user columns with pandas groupbys and a Python
// loop over every group, _extract_item_features (:391-438) filters the
// popularity frame once per article, _add_labels (:752-836) merges the
// recalled pairs with every user's last click.
//
// Layout (built by nrk/profile.py): the click log as a CSR by dense user row
// (u_off [U + 1]; inside a user the clicks in frame order): item row, click
// timestamp, dense device-group code.  `sorted_item` is the same CSR with
// every user's item rows ascending (the wrapper's one key sort), so a user's
// distinct articles are the positions that differ from their predecessor:
// linear in the clicks, and a repeat that straddles two 64-click chunks is
// one global load away.  One wave per user, four users per workgroup; a few
// loads and integer reductions per click: latency-bound, no MFMA.
//
// The exact-sum argument of the mean timestamp: pandas' group_mean is a Kahan
// sum of the float64-cast values in frame order.  While no value is negative
// and the exact integer sum is below 2^53, every value and every partial sum
// is an integer below 2^53, so every addition is exact, every compensation
// term is 0 and the result is (double)sum / n in any order.  Otherwise one
// lane repeats pandas' loop step by step.
#include "nrk_common.h"

// Every double operation below is one rounded operation of the reference, in
// its association.  hipcc's default contraction fuses x * scale + min_ into
// an FMA (one rounding instead of sklearn's two: other bits), also through
// __dmul_rn / __dadd_rn, which are plain operators in this toolchain's headers
// and keep the header's contraction state when inlined.  So contraction is off
// for the whole file and the arithmetic is written with plain operators.
#pragma clang fp contract(off)

namespace nrk {

constexpr int PF_MAX_CODES = 64;            // device-group codes: one lane each
constexpr uint64_t PF_EXACT = 1ull << 53;   // below it every integer is a double

__device__ __forceinline__ int64_t wave_shfl_xor_i64(int64_t v, int m) {
    const uint64_t b = (uint64_t)v;
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)b, m, WAVE);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(b >> 32), m, WAVE);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += wave_shfl_xor_i64(v, m);
    return v;
}
__device__ __forceinline__ int64_t wave_min_i64(int64_t v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const int64_t o = wave_shfl_xor_i64(v, m);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int64_t wave_max_i64(int64_t v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const int64_t o = wave_shfl_xor_i64(v, m);
        v = o > v ? o : v;
    }
    return v;
}

// pandas' group_mean for one group (_libs/groupby.pyx): Kahan summation of
// the float64-cast values in frame order, then sumx / nobs
__device__ double pf_kahan_mean(const int64_t* __restrict__ ts, int64_t n) {
    double sumx = 0.0, comp = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        const double y = (double)ts[i] - comp;
        const double t = sumx + y;
        comp = (t - sumx) - y;
        if (comp != comp) comp = 0.0;
        sumx = t;
    }
    return sumx / (double)n;
}

// one wave per user, four users per workgroup
__global__ __launch_bounds__(256) void profile_user_kernel(
    const int64_t* __restrict__ u_off, int64_t n_users, const int32_t* __restrict__ item,
    const int64_t* __restrict__ ts, const int32_t* __restrict__ dev_code, int n_codes,
    const int32_t* __restrict__ sorted_item, const int64_t* __restrict__ words, int64_t n_items,
    int64_t* __restrict__ out_count, double* __restrict__ out_gap, double* __restrict__ out_mean_ts,
    int32_t* __restrict__ out_mode, double* __restrict__ out_words, int32_t* __restrict__ out_last) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int64_t u = (int64_t)blockIdx.x * 4 + wv; u < n_users; u += (int64_t)gridDim.x * 4) {
        const int64_t b = u_off[u], n = u_off[u + 1] - b;
        if (n <= 0) {  // no click: no group in the reference; zeros, no last click
            if (lane == 0) {
                out_count[u] = 0;
                out_gap[u] = 0.0;
                out_mean_ts[u] = 0.0;
                out_mode[u] = -1;
                out_words[u] = 0.0;
                out_last[u] = -1;
            }
            continue;
        }
        int64_t tmin = INT64_MAX, tmax = INT64_MIN, best_pos = -1;  // best = (tmax of this lane, latest position)
        uint64_t tsum = 0;   // this lane's exact sum while `inexact` is false
        bool inexact = false;
        int64_t wsum = 0;
        int ndist = 0, code_cnt = 0;  // lane c counts device code c
        for (int64_t base = 0; base < n; base += WAVE) {
            const int64_t i = base + lane;
            const bool in = i < n;
            int32_t code = -1;
            if (in) {
                const int64_t t = ts[b + i];
                code = dev_code[b + i];
                tmin = t < tmin ? t : tmin;
                if (t >= tmax) {  // positions ascend inside a lane: >= keeps the later one
                    tmax = t;
                    best_pos = i;
                }
                if (t < 0 || (uint64_t)t >= PF_EXACT) inexact = true;
                else {
                    tsum += (uint64_t)t;  // both below 2^53: no wrap
                    if (tsum >= PF_EXACT) {
                        inexact = true;
                        tsum = 0;
                    }
                }
                const int32_t it = sorted_item[b + i];
                if (i == 0 || sorted_item[b + i - 1] != it) {
                    ++ndist;
                    if (it >= 0 && it < n_items) wsum += words[it];
                }
            }
            for (int c = 0; c < n_codes; ++c) {
                const int k = __popcll(__ballot(code == c));
                if (lane == c) code_cnt += k;
            }
        }
        // last click: (timestamp, position) maximal
        const int64_t wmax = wave_max_i64(tmax), wmin = wave_min_i64(tmin);
        const int64_t last_pos = wave_max_i64(tmax == wmax ? best_pos : -1);
        // mode: (count desc, code asc); n >= 1, so some count is positive
        const int64_t key = ((int64_t)code_cnt << 8) | (int64_t)(255 - lane);
        const int64_t kbest = wave_max_i64(lane < n_codes ? key : -1);
        const int64_t total_words = wave_sum_i64(wsum), total_dist = wave_sum_i64(ndist);
        const bool any_inexact = __ballot(inexact) != 0ull;
        const uint64_t total_ts = (uint64_t)wave_sum_i64((int64_t)tsum);  // 64 lanes below 2^53 each: no wrap
        if (lane == 0) {
            out_count[u] = n;
            out_gap[u] = n > 1 ? (double)(wmax - wmin) / (double)(n - 1) : 0.0;
            out_mean_ts[u] = (any_inexact || total_ts >= PF_EXACT) ? pf_kahan_mean(ts + b, n)
                                                                    : (double)total_ts / (double)n;
            out_mode[u] = (kbest >> 8) > 0 ? 255 - (int32_t)(kbest & 255) : -1;
            out_words[u] = (double)total_words / (double)total_dist;
            out_last[u] = item[b + last_pos];
        }
    }
}

__global__ __launch_bounds__(256) void profile_item_count_kernel(const int32_t* __restrict__ item, int64_t n,
                                                                 int64_t n_items,
                                                                 unsigned long long* __restrict__ cnt) {
    // Popularity is Zipf: a tenth of all clicks land on one article, and one
    // atomic per click serialises on its counter (1.88 ms for 1.6M clicks).
    // The lanes of a wave that hold the same row send one add of their count.
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < n;  // wave-uniform
         base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + lane;
        const int32_t it = i < n ? item[i] : -1;
        bool todo = it >= 0 && it < n_items;
        for (unsigned long long m = __ballot(todo); m; m = __ballot(todo)) {
            const int leader = __ffsll((long long)m) - 1;
            const int32_t v = __shfl(it, leader, WAVE);
            const unsigned long long same = __ballot(todo && it == v);
            if (lane == leader) atomicAdd(cnt + v, (unsigned long long)__popcll(same));
            if (it == v) todo = false;
        }
    }
}

// sklearn's MinMaxScaler (preprocessing/_data.py): fit's scale_ and min_ from
// the column's min / max, transform's X *= scale_; X += min_ as two rounded
// operations
__global__ __launch_bounds__(256) void profile_scale_kernel(const double* __restrict__ x, int64_t n,
                                                            const double* __restrict__ minmax, int skip_zero,
                                                            double* __restrict__ out) {
    const double lo = minmax[0], range = minmax[1] - lo;
    // _handle_zeros_in_scale: 10 * np.finfo(float64).eps
    const double scale = 1.0 / (range < 10.0 * 2.220446049250313e-16 ? 1.0 : range);
    const double min_ = 0.0 - lo * scale;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double v = x[i];
        out[i] = (skip_zero && v == 0.0) ? 0.0 : v * scale + min_;
    }
}

__global__ __launch_bounds__(256) void profile_labels_kernel(const int32_t* __restrict__ user,
                                                             const int32_t* __restrict__ item, int64_t n,
                                                             const int32_t* __restrict__ last_item, int64_t n_users,
                                                             int offline, int32_t* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int32_t y = -1;  // online mode (:761-765)
        if (offline) {
            const int32_t u = user[i], it = item[i];
            y = (u >= 0 && u < n_users && it >= 0 && last_item[u] == it) ? 1 : 0;
        }
        out[i] = y;
    }
}

}  // namespace nrk

using namespace nrk;

extern "C" {

int nrk_profile_user(const int64_t* u_off, int64_t n_users, const int32_t* item, const int64_t* ts,
                     const int32_t* dev_code, int64_t n_clicks, int n_codes, const int32_t* sorted_item,
                     const int64_t* words, int64_t n_items, int64_t* out_count, double* out_gap,
                     double* out_mean_ts, int32_t* out_mode, double* out_words, int32_t* out_last,
                     nrk_stream_t stream) {
    clear_error();
    NRK_REQUIRE(n_users >= 0 && n_clicks >= 0 && n_items >= 0 && n_codes >= 0, "negative size");
    NRK_REQUIRE(n_clicks < (1ll << 31) && n_items < (1ll << 31), "n_clicks and n_items must be < 2^31");
    if (n_codes > PF_MAX_CODES) NRK_UNSUPPORTED("more than 64 device-group codes");
    NRK_REQUIRE(u_off, "null pointer");
    NRK_REQUIRE(n_clicks == 0 || (item && ts && dev_code && sorted_item), "null pointer");
    NRK_REQUIRE(n_items == 0 || words, "null pointer");
    NRK_REQUIRE(n_users == 0 || (out_count && out_gap && out_mean_ts && out_mode && out_words && out_last),
                "null pointer");
    if (n_users == 0) return NRK_OK;
    profile_user_kernel<<<grid_for(n_users, 4, 1 << 20), 256, 0, as_stream(stream)>>>(
        u_off, n_users, item, ts, dev_code, n_codes, sorted_item, words, n_items, out_count, out_gap, out_mean_ts,
        out_mode, out_words, out_last);
    NRK_CHECK_LAUNCH();
    return NRK_OK;
}

int nrk_profile_item_count(const int32_t* item, int64_t n_clicks, int64_t n_items, int64_t* out_count,
                           nrk_stream_t stream) {
    clear_error();
    NRK_REQUIRE(n_clicks >= 0 && n_items >= 0, "negative size");
    NRK_REQUIRE(n_items < (1ll << 31), "n_items must be < 2^31");
    NRK_REQUIRE((n_clicks == 0 || item) && (n_items == 0 || out_count), "null pointer");
    if (n_items == 0) return NRK_OK;
    NRK_FILL(__func__, out_count, 0, (size_t)n_items * sizeof(int64_t), as_stream(stream));
    if (n_clicks == 0) return NRK_OK;
    profile_item_count_kernel<<<grid_for(n_clicks, 256, 1 << 16), 256, 0, as_stream(stream)>>>(
        item, n_clicks, n_items, reinterpret_cast<unsigned long long*>(out_count));
    NRK_CHECK_LAUNCH();
    return NRK_OK;
}

int nrk_profile_scale(const double* x, int64_t n, const double* minmax, int skip_zero, double* out,
                      nrk_stream_t stream) {
    clear_error();
    NRK_REQUIRE(n >= 0, "negative size");
    NRK_REQUIRE(skip_zero == 0 || skip_zero == 1, "skip_zero must be 0 or 1");
    if (n == 0) return NRK_OK;
    NRK_REQUIRE(x && minmax && out, "null pointer");
    profile_scale_kernel<<<grid_for(n, 256, 1 << 16), 256, 0, as_stream(stream)>>>(x, n, minmax, skip_zero, out);
    NRK_CHECK_LAUNCH();
    return NRK_OK;
}

int nrk_profile_labels(const int32_t* user, const int32_t* item, int64_t n_pairs, const int32_t* last_item,
                       int64_t n_users, int offline, int32_t* out, nrk_stream_t stream) {
    clear_error();
    NRK_REQUIRE(n_pairs >= 0 && n_users >= 0, "negative size");
    NRK_REQUIRE(offline == 0 || offline == 1, "offline must be 0 or 1");
    if (n_pairs == 0) return NRK_OK;
    NRK_REQUIRE(out, "null pointer");
    NRK_REQUIRE(!offline || (user && item && (last_item || n_users == 0)), "null pointer");
    profile_labels_kernel<<<grid_for(n_pairs, 256, 1 << 16), 256, 0, as_stream(stream)>>>(
        user, item, n_pairs, last_item, n_users, offline, out);
    NRK_CHECK_LAUNCH();
    return NRK_OK;
}

}  // extern "C"
