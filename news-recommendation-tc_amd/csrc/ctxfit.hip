// ctxfit.hip -- the order statistics behind CtxSpec.fit_device on gfx950.
//
// Reference: FeatureExtractor._apply_binning (src/features/feature_extractor.py
// :838-898) and the context LabelEncoders (src/rank/DIN.py:603-613).  Per
// feature it runs pandas nunique / median / fillna and sklearn's
// KBinsDiscretizer, whose quantile strategy is np.percentile at n_bins + 1
// points.  All of that is a function of the column's sorted values: the count
// of distinct values, the two middle values, and the values at the <= 22 ranks
// numpy interpolates between.  This file sorts every requested column and picks
// those values; the interpolation itself (a handful of rounded operations per
// edge) stays in numpy on the host (nrk/features.py _finish_edges).
//
//   a. ctxfit_keys     raw [n, ld] f64 rows -> one plane of order-preserving
//                      u64 keys per requested column (column-major)
//   b. 8 x (ctxfit_hist, ctxfit_scan, ctxfit_scatter)
//                      keys-only LSD radix sort of the n_cols equal-length
//                      segments, 8 bits per pass, grid (tile, column)
//   c. ctxfit_distinct adjacent-differs count (integer atomics)
//      ctxfit_summary  one wave per column: bisections and picks
//   d. ctxfit_count_below (nrk_ctx_fit_count_below, on the sorted planes the
//                      workspace still holds) valid values below each
//                      candidate bin edge: the rows per bin
//
// Everything the device does is integer comparison and selection, except the
// even-count median's one add-and-halve, so the result is a pure function of
// the input multiset.  ItemCF's radix sort (itemcf.hip) moves a (key, slot)
// pair through one unsegmented run with the slot plane staged in LDS beside
// the keys; this one carries no payload and runs (tile, column) grids over
// many segments, so it has its own three pass kernels.
#include "nrk_common.h"

// the median is one rounded add and one rounded halving in the column's dtype
#pragma clang fp contract(off)

namespace nrk {

constexpr int FIT_THREADS = 256;
constexpr int FIT_ITEMS = 16;
constexpr int FIT_TILE = FIT_THREADS * FIT_ITEMS;  // 4,096 keys: 32 KB of LDS in the scatter
constexpr int FIT_MAX_COLS = 64;
constexpr int FIT_MAX_RANKS = 64;
constexpr int FIT_SMALL = 21;
constexpr uint64_t FIT_NAN_KEY = ~0ull;
constexpr uint64_t FIT_SIGN = 1ull << 63;

static_assert(sizeof(nrk_ctx_fit_col) == 8 * (10 + FIT_SMALL), "nrk_ctx_fit_col is plain 8-byte fields");

struct FitCols {
    int32_t col[FIT_MAX_COLS];
    int32_t kind[FIT_MAX_COLS];
};
struct FitRanks {
    int64_t r[FIT_MAX_RANKS];
};

// f64 -> u64 whose unsigned order is the values' order: -0.0 is +0.0, every
// NaN is the one key that sorts last (+inf is 0xFFF0...0, below it)
__device__ __forceinline__ uint64_t fit_key(double v) {
    if (v != v) return FIT_NAN_KEY;
    if (v == 0.0) return FIT_SIGN;
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b & FIT_SIGN) ? ~b : (b | FIT_SIGN);
}
__device__ __forceinline__ double fit_value(uint64_t k) {
    const uint64_t b = (k & FIT_SIGN) ? (k ^ FIT_SIGN) : ~k;
    return __longlong_as_double((long long)b);
}

// ---------------------------------------------------------------- a. keys --
// One thread per row.  A row's requested columns lie within ld * 8 contiguous
// bytes (128 B for the 16 context features): the lanes' loads of one column
// stride by the row, and the row's other columns are served from the lines
// that load brought in.  Each plane is written with consecutive addresses
// across the lanes.
__global__ __launch_bounds__(FIT_THREADS) void ctxfit_keys(const double* __restrict__ raw, int64_t n, int32_t ld,
                                                           FitCols c, int n_cols, uint64_t* __restrict__ keys,
                                                           int32_t* __restrict__ inexact) {
    for (int64_t i = (int64_t)blockIdx.x * FIT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * FIT_THREADS) {
        const double* row = raw + (size_t)i * (size_t)ld;
        for (int j = 0; j < n_cols; ++j) {
            const double v = row[c.col[j]];
            keys[(size_t)j * (size_t)n + (size_t)i] = fit_key(v);
            bool bad = false;
            if (v == v) {
                if (c.kind[j] == 1) bad = (double)(float)v != v;  // +-inf is a float32
                else if (c.kind[j] == 2) bad = !(fabs(v) <= 9007199254740992.0) || v != rint(v);
            }
            if (bad) inexact[j] = 1;  // every writer stores the same value
        }
    }
}

// ---------------------------------------------------------------- b. sort --
// counts is [column][digit][tile], so each (column, digit) row scans
// contiguously.  Positions are inside a column: n < 2^31 fits uint32.
__global__ __launch_bounds__(FIT_THREADS) void ctxfit_hist(const uint64_t* __restrict__ keys, int64_t n, int shift,
                                                           int nblk, uint32_t* __restrict__ counts) {
    __shared__ uint32_t hist[256];
    const int tid = threadIdx.x;
    const uint64_t* k = keys + (size_t)blockIdx.y * (size_t)n;
    hist[tid] = 0;
    __syncthreads();
    const int64_t t0 = (int64_t)blockIdx.x * FIT_TILE;
#pragma unroll 4
    for (int r = 0; r < FIT_ITEMS; ++r) {
        const int64_t e = t0 + r * FIT_THREADS + tid;
        if (e < n) atomicAdd(&hist[(k[e] >> shift) & 255], 1u);  // LDS integer atomics
    }
    __syncthreads();
    counts[((size_t)blockIdx.y * 256 + tid) * nblk + blockIdx.x] = hist[tid];
}

// one workgroup per (digit, column): exclusive scan of its row in place + the row total
__global__ __launch_bounds__(256) void ctxfit_scan(uint32_t* __restrict__ counts, int nblk,
                                                   uint32_t* __restrict__ totals) {
    __shared__ uint32_t part[256];
    const int tid = threadIdx.x;
    const size_t rowi = (size_t)blockIdx.y * 256 + blockIdx.x;
    uint32_t* row = counts + rowi * nblk;
    const int chunk = (nblk + 255) / 256;
    const int a = tid * chunk < nblk ? tid * chunk : nblk, e = a + chunk < nblk ? a + chunk : nblk;
    uint32_t s = 0;
    for (int k = a; k < e; ++k) s += row[k];
    part[tid] = s;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint32_t v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint32_t run = part[tid] - s;
    for (int k = a; k < e; ++k) {
        const uint32_t c = row[k];
        row[k] = run;
        run += c;
    }
    if (tid == 255) totals[rowi] = part[255];
}

__device__ __forceinline__ uint64_t fit_lanemask_lt() {
    const int lane = threadIdx.x & 63;
    return lane == 0 ? 0ull : (~0ull >> (64 - lane));
}

// Stable scatter of one tile of one column.  Each round of 256 keys is ranked
// by wave ballots (the lanes of a wave that hold the same digit, in lane
// order), the waves' counts are chained through LDS, and the tile is laid out
// digit-major in LDS before it is written, so consecutive threads store
// consecutive addresses of a digit's run.
__global__ __launch_bounds__(FIT_THREADS) void ctxfit_scatter(const uint64_t* __restrict__ kin,
                                                              uint64_t* __restrict__ kout, int64_t n, int shift,
                                                              int nblk, const uint32_t* __restrict__ counts,
                                                              const uint32_t* __restrict__ totals) {
    __shared__ uint64_t sk[FIT_TILE];
    __shared__ uint32_t sg[256], sl[256];
    __shared__ uint32_t base[256];  // global start of digit d minus its tile-local start
    __shared__ uint16_t run[256];   // tile-local write position of digit d
    __shared__ uint16_t wc[4][256];
    const int tid = threadIdx.x, wv = tid >> 6;
    const uint64_t* ki = kin + (size_t)blockIdx.y * (size_t)n;
    uint64_t* ko = kout + (size_t)blockIdx.y * (size_t)n;
    const uint32_t* cnt = counts + (size_t)blockIdx.y * 256 * nblk;
    {
        const uint32_t t = totals[(size_t)blockIdx.y * 256 + tid];
        const uint32_t cb = cnt[(size_t)tid * nblk + blockIdx.x];
        const uint32_t cn = (blockIdx.x + 1 < (unsigned)nblk ? cnt[(size_t)tid * nblk + blockIdx.x + 1] : t) - cb;
        sg[tid] = t;
        sl[tid] = cn;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const uint32_t vg = tid >= d ? sg[tid - d] : 0, vl = tid >= d ? sl[tid - d] : 0;
            __syncthreads();
            sg[tid] += vg;
            sl[tid] += vl;
            __syncthreads();
        }
        const uint32_t lstart = sl[tid] - cn;
        base[tid] = (sg[tid] - t) + cb - lstart;  // mod 2^32: base + local position = global position
        run[tid] = (uint16_t)lstart;
    }
    const int64_t t0 = (int64_t)blockIdx.x * FIT_TILE;
    uint64_t kr[FIT_ITEMS];
#pragma unroll
    for (int r = 0; r < FIT_ITEMS; ++r) {
        const int64_t e = t0 + r * FIT_THREADS + tid;
        kr[r] = e < n ? ki[e] : 0;
    }
#pragma unroll
    for (int r = 0; r < FIT_ITEMS; ++r) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) wc[k][tid] = 0;
        const bool ok = t0 + r * FIT_THREADS + tid < n;
        const uint64_t key = kr[r];
        const uint32_t d = (uint32_t)(key >> shift) & 255u;
        uint64_t m = __ballot(ok);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool on = (d >> bit) & 1u;
            const uint64_t bb = __ballot(on);
            m &= on ? bb : ~bb;
        }
        const uint32_t rank = (uint32_t)__popcll(m & fit_lanemask_lt());
        __syncthreads();
        if (ok && rank == 0) wc[wv][d] = (uint16_t)__popcll(m);
        __syncthreads();
        {
            const uint32_t c0 = wc[0][tid], c1 = wc[1][tid], c2 = wc[2][tid], c3 = wc[3][tid];
            const uint32_t r0 = run[tid];
            wc[0][tid] = (uint16_t)r0;
            wc[1][tid] = (uint16_t)(r0 + c0);
            wc[2][tid] = (uint16_t)(r0 + c0 + c1);
            wc[3][tid] = (uint16_t)(r0 + c0 + c1 + c2);
            run[tid] = (uint16_t)(r0 + c0 + c1 + c2 + c3);
        }
        __syncthreads();
        if (ok) {
            const uint32_t lp = wc[wv][d] + rank;
            if (lp < (uint32_t)FIT_TILE) sk[lp] = key;  // always true for consistent counts
        }
    }
    __syncthreads();
    const int nloc = n - t0 < FIT_TILE ? (int)(n - t0) : FIT_TILE;
    for (int i = tid; i < nloc; i += FIT_THREADS) {
        const uint64_t key = sk[i];
        const uint32_t gp = base[(uint32_t)(key >> shift) & 255u] + (uint32_t)i;
        if (gp < (uint64_t)n) ko[gp] = key;  // always true for consistent counts; never store past the plane
    }
}

// ------------------------------------------------------------- c. summary --
// distinct valid values of every sorted plane: positions that differ from
// their predecessor.  Integer atomics: the sum does not depend on the order.
__global__ __launch_bounds__(FIT_THREADS) void ctxfit_distinct(const uint64_t* __restrict__ keys, int64_t n,
                                                               unsigned long long* __restrict__ n_distinct) {
    __shared__ uint32_t part[FIT_THREADS / WAVE];
    const uint64_t* k = keys + (size_t)blockIdx.y * (size_t)n;
    uint32_t c = 0;  // at most ceil(n / stride) < 2^31 per thread
    for (int64_t i = (int64_t)blockIdx.x * FIT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * FIT_THREADS) {
        const uint64_t v = k[i];
        if (v != FIT_NAN_KEY && (i == 0 || k[i - 1] != v)) ++c;
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) c += (uint32_t)__shfl_xor((int)c, m, WAVE);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < FIT_THREADS / WAVE; ++w) s += part[w];
        if (s) atomicAdd(n_distinct + blockIdx.y, (unsigned long long)s);
    }
}

// first position in k[0, n) whose key is >= x (upper = false) or > x (upper = true)
__device__ int64_t fit_bound(const uint64_t* __restrict__ k, int64_t n, uint64_t x, bool upper) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const uint64_t v = k[mid];
        if (upper ? v <= x : v < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one wave per column
__global__ __launch_bounds__(WAVE) void ctxfit_summary(const uint64_t* __restrict__ keys, int64_t n, FitCols c,
                                                       FitRanks rk, int n_ranks,
                                                       const unsigned long long* __restrict__ n_distinct,
                                                       const int32_t* __restrict__ inexact,
                                                       nrk_ctx_fit_col* __restrict__ out_stats,
                                                       double* __restrict__ out_picks) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const uint64_t* k = keys + (size_t)j * (size_t)n;
    // every lane repeats the few bisections: no broadcast, no divergence
    const int64_t nv = fit_bound(k, n, FIT_NAN_KEY, false);
    const int64_t n_nan = n - nv;
    double vmin = 0.0, vmax = 0.0, mid_lo = 0.0, mid_hi = 0.0, fill = 0.0;
    int64_t n_lt = 0, n_eq = 0;
    if (nv > 0) {
        vmin = fit_value(k[0]);
        vmax = fit_value(k[nv - 1]);
        mid_lo = fit_value(k[(nv - 1) >> 1]);
        mid_hi = fit_value(k[nv >> 1]);
        if (nv & 1) fill = mid_lo;
        else if (c.kind[j] == 1) fill = (double)(((float)mid_lo + (float)mid_hi) / 2.0f);
        else fill = (mid_lo + mid_hi) / 2.0;
        if (fill == fill) {  // a NaN fill (-inf and +inf in the middle) equals no key
            const uint64_t fk = fit_key(fill);
            n_lt = fit_bound(k, nv, fk, false);
            n_eq = fit_bound(k, nv, fk, true) - n_lt;
        } else {
            n_lt = nv;
        }
    }
    nrk_ctx_fit_col* st = out_stats + j;
    if (lane == 0) {
        st->n_valid = nv;
        st->n_distinct = (int64_t)n_distinct[j];
        st->vmin = vmin;
        st->vmax = vmax;
        st->mid_lo = mid_lo;
        st->mid_hi = mid_hi;
        st->fill = fill;
        st->n_lt_fill = n_lt;
        st->n_eq_fill = n_eq;
        st->inexact = inexact[j];
        // the smallest distinct values: hop from each value's first position past its run
        int64_t pos = 0;
        for (int s = 0; s < FIT_SMALL; ++s) {
            double v = 0.0;
            if (pos < nv) {
                const uint64_t key = k[pos];
                v = fit_value(key);
                pos = fit_bound(k, nv, key, true);
            }
            st->small[s] = v;
        }
    }
    // the filled column: the sorted valid values with n_nan copies of fill at its place
    for (int r = 0; r < n_ranks; ++r) {  // uniform index into the kernel argument; lane r stores
        const int64_t q = rk.r[r];
        double v;
        if (q < n_lt) v = fit_value(k[q]);
        else if (q < n_lt + n_eq + n_nan) v = fill;
        else v = fit_value(k[q - n_nan]);  // q < n, so q - n_nan < nv
        if (lane == (r & (WAVE - 1))) out_picks[(size_t)j * n_ranks + r] = v;
    }
}

// valid values of column j below each of its probes: which bins of a fitted
// column hold a row (the classes its LabelEncoder sees).  A NaN probe counts 0.
__global__ __launch_bounds__(WAVE) void ctxfit_count_below(const uint64_t* __restrict__ keys, int64_t n,
                                                           const double* __restrict__ probes, int n_probes,
                                                           int64_t* __restrict__ out) {
    const int j = blockIdx.x;
    const uint64_t* k = keys + (size_t)j * (size_t)n;
    const int64_t nv = fit_bound(k, n, FIT_NAN_KEY, false);
    for (int p = threadIdx.x; p < n_probes; p += WAVE) {
        const double x = probes[(size_t)j * n_probes + p];
        out[(size_t)j * n_probes + p] = x == x ? fit_bound(k, nv, fit_key(x), false) : 0;
    }
}

// -------------------------------------------------------------- workspace --
struct FitWs {
    uint64_t *ka, *kb;
    uint32_t *counts, *totals;
    unsigned long long* n_distinct;  // [n_cols], then int32 inexact [n_cols]: one memset clears both
    int32_t* inexact;
    size_t clear_bytes, bytes;
};

static FitWs fit_ws_layout(void* base, int64_t n_rows, int32_t n_cols) {
    FitWs w;
    Arena a(base);
    const size_t n = (size_t)(n_rows > 0 ? n_rows : 1), c = (size_t)(n_cols > 0 ? n_cols : 1);
    const size_t nblk = (n + FIT_TILE - 1) / FIT_TILE;
    w.ka = (uint64_t*)a.take(n * c * 8);
    w.kb = (uint64_t*)a.take(n * c * 8);
    w.counts = (uint32_t*)a.take(c * 256 * nblk * 4);
    w.totals = (uint32_t*)a.take(c * 256 * 4);
    w.clear_bytes = c * 8 + c * 4;
    w.n_distinct = (unsigned long long*)a.take(w.clear_bytes);
    w.inexact = w.n_distinct ? reinterpret_cast<int32_t*>(w.n_distinct + c) : nullptr;
    w.bytes = a.bytes;
    return w;
}

}  // namespace nrk

using namespace nrk;

extern "C" {

size_t nrk_ctx_fit_workspace_bytes(int64_t n_rows, int32_t n_cols) {
    if (n_rows < 0 || n_rows >= (1ll << 31) || n_cols < 1 || n_cols > FIT_MAX_COLS) return 0;
    return fit_ws_layout(nullptr, n_rows, n_cols).bytes;
}

int32_t nrk_ctx_fit_tile(void) { return FIT_TILE; }

int nrk_ctx_fit_stats(const double* raw, int64_t n_rows, int32_t ld, const int32_t* cols, const int32_t* col_kind,
                      int32_t n_cols, const int64_t* ranks, int32_t n_ranks, nrk_ctx_fit_col* out_stats,
                      double* out_picks, void* workspace, size_t workspace_bytes, nrk_stream_t stream) {
    clear_error();
    NRK_REQUIRE(n_rows >= 0, "negative size");
    NRK_REQUIRE(n_cols >= 1 && n_cols <= FIT_MAX_COLS, "n_cols must be in [1, 64]");
    NRK_REQUIRE(n_ranks >= 0 && n_ranks <= FIT_MAX_RANKS, "n_ranks must be in [0, 64]");
    NRK_REQUIRE(raw && cols && col_kind && out_stats, "null pointer");
    NRK_REQUIRE(n_ranks == 0 || (ranks && out_picks), "null pointer");
    FitCols c = {};
    for (int j = 0; j < n_cols; ++j) {
        NRK_REQUIRE(cols[j] >= 0 && (int64_t)ld >= (int64_t)cols[j] + 1, "ld must exceed every column index");
        NRK_REQUIRE(col_kind[j] >= 0 && col_kind[j] <= 2, "col_kind must be 0 (f64), 1 (f32) or 2 (integer)");
        c.col[j] = cols[j];
        c.kind[j] = col_kind[j];
    }
    if (n_rows == 0) return NRK_OK;
    if (n_rows >= (1ll << 31)) NRK_UNSUPPORTED("n_rows must be < 2^31");
    FitRanks rk = {};
    for (int r = 0; r < n_ranks; ++r) {
        NRK_REQUIRE(ranks[r] >= 0 && ranks[r] < n_rows, "rank out of [0, n_rows)");
        NRK_REQUIRE(r == 0 || ranks[r] >= ranks[r - 1], "ranks must ascend");
        rk.r[r] = ranks[r];
    }
    NRK_REQUIRE(workspace, "null pointer");
    const FitWs ws = fit_ws_layout(workspace, n_rows, n_cols);
    NRK_REQUIRE(workspace_bytes >= ws.bytes, "workspace too small (nrk_ctx_fit_workspace_bytes)");
    hipStream_t s = as_stream(stream);
    const int nblk = (int)((n_rows + FIT_TILE - 1) / FIT_TILE);
    NRK_FILL(__func__, ws.n_distinct, 0, ws.clear_bytes, s);
    ctxfit_keys<<<grid_for(n_rows, FIT_THREADS, 1 << 16), FIT_THREADS, 0, s>>>(raw, n_rows, ld, c, n_cols, ws.ka,
                                                                               ws.inexact);
    uint64_t *kin = ws.ka, *kout = ws.kb;
    for (int shift = 0; shift < 64; shift += 8) {
        ctxfit_hist<<<dim3(nblk, n_cols), FIT_THREADS, 0, s>>>(kin, n_rows, shift, nblk, ws.counts);
        ctxfit_scan<<<dim3(256, n_cols), 256, 0, s>>>(ws.counts, nblk, ws.totals);
        ctxfit_scatter<<<dim3(nblk, n_cols), FIT_THREADS, 0, s>>>(kin, kout, n_rows, shift, nblk, ws.counts,
                                                                  ws.totals);
        std::swap(kin, kout);
    }
    // eight passes: the sorted planes are back in ka (= kin)
    ctxfit_distinct<<<dim3(grid_for(n_rows, FIT_THREADS * 8, 256), n_cols), FIT_THREADS, 0, s>>>(kin, n_rows,
                                                                                               ws.n_distinct);
    ctxfit_summary<<<n_cols, WAVE, 0, s>>>(kin, n_rows, c, rk, n_ranks, ws.n_distinct, ws.inexact, out_stats,
                                           out_picks);
    NRK_CHECK_LAUNCH();
    return NRK_OK;
}

int nrk_ctx_fit_count_below(int64_t n_rows, int32_t n_cols, const double* probes, int32_t n_probes,
                            int64_t* out_counts, const void* workspace, size_t workspace_bytes,
                            nrk_stream_t stream) {
    clear_error();
    NRK_REQUIRE(n_rows >= 0, "negative size");
    NRK_REQUIRE(n_cols >= 1 && n_cols <= FIT_MAX_COLS, "n_cols must be in [1, 64]");
    NRK_REQUIRE(n_probes >= 0 && n_probes <= FIT_MAX_RANKS, "n_probes must be in [0, 64]");
    if (n_rows == 0 || n_probes == 0) return NRK_OK;
    if (n_rows >= (1ll << 31)) NRK_UNSUPPORTED("n_rows must be < 2^31");
    NRK_REQUIRE(probes && out_counts && workspace, "null pointer");
    const FitWs ws = fit_ws_layout(const_cast<void*>(workspace), n_rows, n_cols);
    NRK_REQUIRE(workspace_bytes >= ws.bytes, "workspace too small (nrk_ctx_fit_workspace_bytes)");
    ctxfit_count_below<<<n_cols, WAVE, 0, as_stream(stream)>>>(ws.ka, n_rows, probes, n_probes, out_counts);
    NRK_CHECK_LAUNCH();
    return NRK_OK;
}

}  // extern "C"
