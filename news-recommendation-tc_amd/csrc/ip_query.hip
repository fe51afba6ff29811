// ip_query.hip -- exact top-k for small user batches: the CATALOG is split
// across the chip, not the users (nrk_ip_topk gives 1,024 users to a
// workgroup, so a handful of users runs on one CU and waits for a whole
// catalog pass).  Same contract as nrk_ip_topk: rows by (score desc, row asc),
// fp32 scores = the rounding of the exact fp64 score.
//
//   1. ip_query_slice_kernel: grid (G, user tiles of IQ_UQ).  Workgroup g
//      walks the rounds g, g + G, ... of 256 consecutive items, one item per
//      lane; the lane loads its row once per round and scores it against the
//      tile's users (fp64 copies in LDS) with exact_dot_tile.  No screen, no
//      epsilon, no packed catalog: every score is the exact one.  Each
//      (workgroup, user) keeps a streaming top-k in LDS and leaves its sorted
//      list (<= k entries) in the workspace.
//   2. ip_query_merge_kernel: one workgroup per user runs the same streaming
//      top-k over the user's G lists, rank-major (every list's best entry
//      first, so the threshold rises early), and writes the outputs.
//
// The streaming top-k (topk_round / topk_trim): a list of IQ_CAP entries, of
// which the first k are the sorted survivors once it has been trimmed; a
// candidate passes when better(c, kth) -- the full order, rows are unique, so
// there are no ties and no fallback: an all-zero user keeps its first k rows.
// Passing candidates are appended behind the survivors by ballot; once
// IQ_SLACK of them are in (or, at large k, a round of 256 may no longer fit)
// the list is sorted, cut to k and kth moves.
#include "nrk_common.h"
#include "exact_dot.h"

#include <float.h>
#include <math.h>

#include <algorithm>
#include <atomic>

namespace nrk {

constexpr int IQ_UQ = 8;        // users per workgroup tile (one fp64 accumulator each)
constexpr int IQ_ROUND = 256;   // items per round = threads per workgroup
constexpr int IQ_CAP = 512;     // list capacity
constexpr int IQ_SLACK = 64;    // a list is cut at k + IQ_SLACK entries (24 .. 200 measured)
constexpr int IQ_KMAX = 128;    // larger k stays with nrk_ip_topk's exact path
constexpr int IQ_GMAX = 512;    // most workgroups along the catalog
constexpr int IQ_GRID = 1024;   // workgroups aimed at over both grid axes
static_assert(IQ_CAP >= IQ_KMAX + IQ_ROUND && (IQ_CAP & (IQ_CAP - 1)) == 0, "a trimmed list takes one more round");
static_assert(IQ_ROUND == 4 * WAVE, "topk_round: four waves");

__device__ __forceinline__ Cand worst_cand() { return Cand{-INFINITY, INT32_MAX}; }

// One wave: sort the list's *cnt entries best first, keep min(*cnt, k) and
// set *kth to the k-th (worst_cand while the list is shorter than k)
__device__ inline void topk_trim(Cand* ent, int* cnt, Cand* kth, int k) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int n = *cnt;
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int i = n + lane; i < n2; i += WAVE) ent[i] = worst_cand();
    wave_lds_sort(ent, n2);
    if (lane == 0) {
        const int keep = n < k ? n : k;
        *cnt = keep;
        *kth = keep == k ? ent[k - 1] : worst_cand();
    }
    wave_sync_lds();
}

// One round of the streaming top-k of nq <= NQ lists (ent[q * IQ_CAP ...],
// cnt[q], kth[q] in LDS), called by the whole workgroup: every thread offers
// one candidate (sc[q], row) to each list (none when !valid).  The lists'
// order is left to the atomics, their contents are not: a round's passes
// depend on kth alone, and kth moves only in topk_trim, at counts that do not
// depend on the order.
template <int NQ>
__device__ __forceinline__ void topk_round(Cand* ent, int* cnt, Cand* kth, const double (&sc)[NQ], int32_t row,
                                           bool valid, int nq, int k) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    for (int q = wave; q < nq; q += 4) {
        // IQ_SLACK entries behind the k survivors, or no room for another
        // round: a fresh threshold lets the later rounds pass fewer
        if (cnt[q] >= k + IQ_SLACK || cnt[q] + IQ_ROUND > IQ_CAP) topk_trim(ent + q * IQ_CAP, cnt + q, kth + q, k);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        if (q < nq) {
            const Cand c{sc[q], row};
            const bool pass = valid && better(c, kth[q]);
            const unsigned long long bal = __ballot(pass);
            if (bal) {
                const int lead = __ffsll((long long)bal) - 1;
                int base = 0;
                if (lane == lead) base = atomicAdd(&cnt[q], __popcll(bal));
                base = __shfl(base, lead, WAVE);
                if (pass) ent[q * IQ_CAP + base + __popcll(bal & ((1ull << lane) - 1ull))] = c;
            }
        }
    }
    __syncthreads();
}

// Dynamic LDS: nq lists of IQ_CAP entries, then nq user rows of ustride
// doubles (nq = min(IQ_UQ, n_users), ustride = dim rounded up to even).
// Workspace: ws_list[(u * k + rank) * G + g] (rank-major per user, the
// merge's reading order), ws_cnt[u * G + g].
__global__ __launch_bounds__(256) void ip_query_slice_kernel(
    const float* __restrict__ users, int n_users, const float* __restrict__ items, int n_items, int dim, int k,
    Cand* __restrict__ ws_list, int32_t* __restrict__ ws_cnt) {
    extern __shared__ __attribute__((aligned(16))) uint8_t dyn[];
    __shared__ int cnt[IQ_UQ];
    __shared__ Cand kth[IQ_UQ];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int G = gridDim.x, g = blockIdx.x, u0 = blockIdx.y * IQ_UQ;
    const int nq = min(IQ_UQ, n_users - u0), ustride = (dim + 1) & ~1;
    Cand* ent = reinterpret_cast<Cand*>(dyn);
    double* ud = reinterpret_cast<double*>(dyn + (size_t)min(IQ_UQ, n_users) * IQ_CAP * sizeof(Cand));
    for (int i = tid; i < nq * dim; i += IQ_ROUND) {
        const int q = i / dim, t = i - q * dim;
        ud[q * ustride + t] = (double)users[(int64_t)(u0 + q) * dim + t];
    }
    if (tid < nq) {
        cnt[tid] = 0;
        kth[tid] = worst_cand();
    }
    __syncthreads();
    const int n_rounds = (n_items + IQ_ROUND - 1) / IQ_ROUND;
    for (int rd = g; rd < n_rounds; rd += G) {
        const int r = rd * IQ_ROUND + tid;
        const bool valid = r < n_items;
        double acc[IQ_UQ] = {};
        if (valid) exact_dot_tile<IQ_UQ>(items + (int64_t)r * dim, ud, ustride, dim, nq, acc);
        topk_round<IQ_UQ>(ent, cnt, kth, acc, r, valid, nq, k);
    }
    for (int q = wave; q < nq; q += 4) topk_trim(ent + q * IQ_CAP, cnt + q, kth + q, k);
    __syncthreads();
    for (int q = 0; q < nq; ++q) {
        const int n = cnt[q];
        const int64_t u = u0 + q;
        for (int i = tid; i < n; i += IQ_ROUND) ws_list[(u * k + i) * G + g] = ent[q * IQ_CAP + i];
        if (tid == 0) ws_cnt[u * G + g] = n;
    }
}

__global__ __launch_bounds__(256) void ip_query_merge_kernel(
    const Cand* __restrict__ ws_list, const int32_t* __restrict__ ws_cnt, int G, int n_items, int k,
    int64_t row_offset, float* __restrict__ out_s, int32_t* __restrict__ out_r, double* __restrict__ out_e) {
    __shared__ Cand ent[IQ_CAP];
    __shared__ int gcnt[IQ_GMAX];
    __shared__ int cnt[1];
    __shared__ Cand kth[1];
    const int tid = threadIdx.x;
    const int64_t u = blockIdx.x;
    for (int i = tid; i < G; i += IQ_ROUND) gcnt[i] = min(max(ws_cnt[u * G + i], 0), k);
    if (tid == 0) {
        cnt[0] = 0;
        kth[0] = worst_cand();
    }
    __syncthreads();
    const int kk = n_items < k ? n_items : k;  // no list is longer
    const int total = kk * G;
    for (int e0 = 0; e0 < total; e0 += IQ_ROUND) {
        const int e = e0 + tid, rank = e / G, gi = e - rank * G;
        const bool valid = e < total && rank < gcnt[gi];
        Cand c = worst_cand();
        if (valid) c = ws_list[(u * k + rank) * G + gi];
        const double sc[1] = {c.s};
        topk_round<1>(ent, cnt, kth, sc, c.row, valid, 1, k);
    }
    if (tid < WAVE) topk_trim(ent, cnt, kth, k);
    __syncthreads();
    const int n = cnt[0];
    for (int i = tid; i < k; i += IQ_ROUND) {
        // past min(k, n_items): ip_exact_kernel's padding
        const bool ok = i < n;
        out_s[u * k + i] = ok ? (float)ent[i].s : -FLT_MAX;
        out_r[u * k + i] = ok ? (int32_t)(ent[i].row + row_offset) : -1;
        if (out_e) out_e[u * k + i] = ok ? ent[i].s : -INFINITY;
    }
}

// ------------------------------------------------------------------ host --
// Workgroups along the catalog: IQ_GRID over the user tiles, at most one per
// round and IQ_GMAX
static int iq_grid_g(int64_t n_users, int64_t n_items) {
    const int64_t rounds = std::max<int64_t>(1, (n_items + IQ_ROUND - 1) / IQ_ROUND);
    const int64_t tiles = std::max<int64_t>(1, (n_users + IQ_UQ - 1) / IQ_UQ);
    return (int)std::min(std::max<int64_t>(1, IQ_GRID / tiles), std::min<int64_t>(rounds, IQ_GMAX));
}

// n_users * iq_grid_g(...) is not monotone in n_users (G steps down as tiles
// are added); the workspace is sized by this bound of it, which is:
// G <= min(rounds, IQ_GMAX), and G <= IQ_GRID / tiles or G = 1
static int64_t iq_lists_bound(int64_t n_users, int64_t n_items) {
    const int64_t rounds = std::max<int64_t>(1, (n_items + IQ_ROUND - 1) / IQ_ROUND);
    const int64_t by_g = n_users * std::min<int64_t>(rounds, IQ_GMAX);
    return std::max<int64_t>(1, std::max(n_users, std::min<int64_t>(by_g, (int64_t)IQ_GRID * IQ_UQ)));
}

struct IqWs {
    Cand* list;
    int32_t* cnt;
    size_t bytes;
};
static IqWs iq_ws_layout(void* base, int64_t n_users, int64_t n_items, int k) {
    Arena a(base);
    const int64_t lists = iq_lists_bound(n_users, n_items);
    IqWs w;
    w.list = static_cast<Cand*>(a.take((size_t)lists * k * sizeof(Cand)));
    w.cnt = static_cast<int32_t*>(a.take((size_t)lists * sizeof(int32_t)));
    w.bytes = a.bytes;
    return w;
}

static bool iq_sizes_ok(int64_t n_users, int64_t n_items, int dim, int k) {
    return n_users >= 0 && n_users <= NRK_IP_QUERY_MAX_USERS && n_items >= 0 && n_items < (1ll << 30) && dim >= 1 &&
           dim <= 256 && k >= 1 && k <= IQ_KMAX;
}

}  // namespace nrk

using namespace nrk;

extern "C" {

size_t nrk_ip_query_workspace_bytes(int64_t n_users, int64_t n_items, int dim, int k) {
    if (!iq_sizes_ok(n_users, n_items, dim, k)) return 0;
    return iq_ws_layout(nullptr, n_users, n_items, k).bytes;
}

int nrk_ip_query_plan(int64_t n_users, int64_t n_items, int dim, int k, int32_t out[4]) {
    clear_error();
    NRK_REQUIRE(out != nullptr, "out is null");
    NRK_REQUIRE(iq_sizes_ok(n_users, n_items, dim, k), "sizes outside nrk_ip_query's range");
    out[0] = IQ_UQ;
    out[1] = IQ_ROUND;
    out[2] = iq_grid_g(n_users, n_items);
    out[3] = IQ_CAP;
    return NRK_OK;
}

int nrk_ip_query(const float* users, int64_t n_users, const float* items, int64_t n_items, int dim, int k,
                 int64_t row_offset, float* out_scores, int32_t* out_rows, double* out_exact, void* workspace,
                 size_t workspace_bytes, nrk_stream_t stream) {
    clear_error();
    NRK_REQUIRE(n_users >= 0 && n_items >= 0, "negative sizes");
    NRK_REQUIRE(n_items < (1ll << 30), "n_items must be < 2^30");
    NRK_REQUIRE(dim > 0 && dim <= 256, "dim must be in [1, 256]");
    NRK_REQUIRE(k >= 1, "k must be >= 1");
    if (k > IQ_KMAX) NRK_UNSUPPORTED("k > 128 is nrk_ip_topk's exact path");
    NRK_REQUIRE(n_users <= NRK_IP_QUERY_MAX_USERS, "n_users must be <= NRK_IP_QUERY_MAX_USERS (4096): use nrk_ip_topk");
    if (n_users == 0) return NRK_OK;
    NRK_REQUIRE(users && workspace, "null pointer");
    NRK_REQUIRE(out_scores && out_rows, "null output");
    NRK_REQUIRE(n_items == 0 || items, "items null");
    const IqWs w = iq_ws_layout(workspace, n_users, n_items, k);
    NRK_REQUIRE(workspace_bytes >= w.bytes, "workspace too small");
    hipStream_t s = as_stream(stream);
    const int G = iq_grid_g(n_users, n_items);
    const int nq = (int)std::min<int64_t>(IQ_UQ, n_users), ustride = (dim + 1) & ~1;
    const size_t lds = (size_t)nq * (IQ_CAP * sizeof(Cand) + ustride * sizeof(double));
    constexpr size_t lds_max = (size_t)IQ_UQ * (IQ_CAP * sizeof(Cand) + 256 * sizeof(double));
    static_assert(lds_max <= CU_LDS_BYTES, "ip_query_slice LDS");
    static std::atomic<uint64_t> slice_set{0};
    lds_limit_once(slice_set, (const void*)ip_query_slice_kernel, lds_max);
    const dim3 grid((unsigned)G, (unsigned)((n_users + IQ_UQ - 1) / IQ_UQ));
    ip_query_slice_kernel<<<grid, IQ_ROUND, lds, s>>>(users, (int)n_users, items, (int)n_items, dim, k, w.list, w.cnt);
    ip_query_merge_kernel<<<(unsigned)n_users, IQ_ROUND, 0, s>>>(w.list, w.cnt, G, (int)n_items, k, row_offset,
                                                                out_scores, out_rows, out_exact);
    NRK_CHECK_LAUNCH();
    return NRK_OK;
}

}  // extern "C"
