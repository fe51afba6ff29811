// usercf.hip -- UserCF user-to-user similarity and recall on gfx950.
//
// Reference: UserCFSimilarity.calculate, src/similarity/user_cf.py:31-66
// (weights.py activation_weight / log_penalty); UserCFRecaller.recall,
// src/recall/usercf_recaller.py:37-118.
//
// Similarity.  The reference walks the items in ascending id, and for every
// entry u of an item's click list and every entry v != u does
//   u2u[u][v] += (50.0 * (act[u] + act[v])) * (1.0 / log(len(list) + 1))
// then divides by sqrt(cnt[u] * cnt[v]).  Row u therefore receives its terms
// in (item asc, u's entry, v's entry) order, and its dict holds v in the order
// of v's first slot: the smallest index into the item->user CSR at which v
// stands in an item that u clicked.  The stable sorts downstream break the
// (very common) exact ties by that order, so the sums must be bit-exact:
//   * one workgroup owns a row; it steps through u's clicks in item-ascending
//     order (a doubly-clicked item is two steps), one step after the other,
//     the lanes of a step running over the item's entries v;
//   * every destination (u, v) is a slot of the workgroup's own dense
//     accumulator in global memory (fp64 sum + int64 first slot per user), so
//     it receives its terms in the reference's order by plain owner
//     read-modify-write.  Two lanes meet on one slot within a step only when
//     v clicked that item more than once (uc_dup_kernel flags those entries
//     from v's item-sorted click list): the addends are then identical, their
//     order cannot matter, and exactly those entries use an atomic add / min.
//     Nothing else races and no float atomic crosses a step or a workgroup;
//   * a touched list makes the finish visit, and reset, only the non-zeros;
//   * the arithmetic is __dmul_rn / __dadd_rn / __ddiv_rn / __dsqrt_rn in the
//     reference's association (hipcc would contract a * b + c into an FMA).
// The finish either emits the whole row (nrk_usercf_sim) or selects its
// top-n by (value desc, first slot asc) in LDS (nrk_usercf_topn): the u2u
// matrix is never materialised; the workspace is UC_GRID dense rows.
//
// Recall.  uc_cand_kernel walks (neighbour rank, position in the neighbour's
// history) for a batch of query users and writes (key, sequence number,
// contribution) in rc_cand_kernel's format; the stable radix sort, the
// ordered per-(query, item) sums, the hot fill and the stable top-k are
// ItemCF's back end (itemcf_backend.h), unchanged.
#include "itemcf_backend.h"
#include "nrk_common.h"

#include <climits>
#include <cmath>

namespace nrk {

constexpr int UC_THREADS = 256;
constexpr int UC_GRID = 512;   // resident workgroups = dense rows in the workspace (2 per CU on 256 CUs)
constexpr int UC_SEL = 1024;   // largest topn of the direct top-n
constexpr int64_t UC_NONE = INT64_MAX;

// The dense rows are read and written at agent scope (relaxed): plain
// accesses could leave a line in the CU's L1 that a later atomic, performed at
// L2, would not update.
__device__ __forceinline__ double uc_ldf(const double* p) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p),
                                                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void uc_stf(double* p, double v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int64_t uc_ldi(const int64_t* p) {
    return (int64_t)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void uc_sti(int64_t* p, int64_t v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// dupf[e] = 1 when the user of entry e clicked e's item more than once: its
// item-sorted click list then holds the item twice in a row.
__global__ __launch_bounds__(256) void uc_dup_kernel(const int64_t* __restrict__ i_off, int32_t n_items,
                                                     const int32_t* __restrict__ i_users,
                                                     const int64_t* __restrict__ u_off,
                                                     const int32_t* __restrict__ u_items, int64_t n_clicks,
                                                     uint8_t* __restrict__ dupf) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n_clicks; e += (int64_t)gridDim.x * 256) {
        int32_t lo = 0, hi = n_items;  // the last item with i_off[item] <= e
        while (hi - lo > 1) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            if (i_off[mid] <= e) lo = mid;
            else hi = mid;
        }
        const int32_t i = lo;
        const int32_t v = i_users[e];
        int64_t a = u_off[v], b = u_off[v + 1];
        const int64_t end = b;
        while (a < b) {  // first position of i in v's sorted clicks
            const int64_t mid = (a + b) >> 1;
            if (u_items[mid] < i) a = mid + 1;
            else b = mid;
        }
        dupf[e] = (a + 1 < end && u_items[a] == i && u_items[a + 1] == i) ? 1 : 0;
    }
}

__device__ __forceinline__ bool uc_better(double as, int64_t af, double bs, int64_t bf) {
    return as > bs || (as == bs && af < bf);
}

struct UcSel {  // the selection's LDS: [0, K) the best so far, [K, 2K) the incoming entries
    double s[2 * UC_SEL];
    int64_t f[2 * UC_SEL];
    int32_t c[2 * UC_SEL];
};

// sorts [0, 2K) best first, clears [K, 2K); every thread of the workgroup
__device__ inline void uc_merge(UcSel& x, int K, int* s_in) {
    const int tid = threadIdx.x, n = 2 * K;
    __syncthreads();
    for (int sz = 2; sz <= n; sz <<= 1) {
        for (int st = sz >> 1; st > 0; st >>= 1) {
            for (int i = tid; i < n / 2; i += UC_THREADS) {
                const int lo = 2 * st * (i / st) + (i % st), hi = lo + st;
                const bool up = (lo & sz) == 0;
                const double as = x.s[lo], bs = x.s[hi];
                const int64_t af = x.f[lo], bf = x.f[hi];
                if (up ? uc_better(bs, bf, as, af) : uc_better(as, af, bs, bf)) {
                    const int32_t ac = x.c[lo], bc = x.c[hi];
                    x.s[lo] = bs; x.f[lo] = bf; x.c[lo] = bc;
                    x.s[hi] = as; x.f[hi] = af; x.c[hi] = ac;
                }
            }
            __syncthreads();
        }
    }
    for (int i = K + tid; i < n; i += UC_THREADS) {
        x.s[i] = -INFINITY;
        x.f[i] = UC_NONE;
        x.c[i] = -1;
    }
    if (tid == 0) *s_in = 0;
    __syncthreads();
}

// One workgroup per row u (grid-strided); FULL: every (v, value, first slot)
// of the row at row_off[u] (touched order); else the row's top-n and nnz.
template <bool FULL>
__global__ __launch_bounds__(UC_THREADS) void uc_rows_kernel(
    const int64_t* __restrict__ i_off, const int32_t* __restrict__ i_users, const int64_t* __restrict__ u_off,
    const int32_t* __restrict__ u_items, const double* __restrict__ act, const double* __restrict__ pen,
    const uint8_t* __restrict__ dupf, int64_t n_users, double* __restrict__ acc_all,
    int64_t* __restrict__ first_all, int32_t* __restrict__ touched_all, int topn, int K,
    int32_t* __restrict__ out_cols, double* __restrict__ out_vals, int64_t* __restrict__ out_cnt,
    int32_t* __restrict__ out_nnz, const int64_t* __restrict__ row_off, int32_t* __restrict__ out_v,
    double* __restrict__ out_s, int64_t* __restrict__ out_f) {
    __shared__ UcSel sel;
    __shared__ int s_cnt, s_in;
    const int tid = threadIdx.x;
    double* acc = acc_all + (int64_t)blockIdx.x * n_users;
    int64_t* first = first_all + (int64_t)blockIdx.x * n_users;
    int32_t* touched = touched_all + (int64_t)blockIdx.x * n_users;
    for (int64_t v = tid; v < n_users; v += UC_THREADS) {
        uc_stf(acc + v, 0.0);
        uc_sti(first + v, UC_NONE);
    }
    for (int64_t u = blockIdx.x; u < n_users; u += gridDim.x) {
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        const int64_t ub = u_off[u], ue = u_off[u + 1];
        const double au = act[u];
        for (int64_t st = ub; st < ue; ++st) {
            const int32_t i = u_items[st];
            const int64_t eb = i_off[i], ee = i_off[i + 1];
            const double pi = pen[i];
            for (int64_t e = eb + tid; e < ee; e += UC_THREADS) {
                const int32_t v = i_users[e];
                if (v == (int32_t)u) continue;
                // activation_weight(act[u] + act[v]) * (1.0 / log_penalty(n_i))
                const double t = __dmul_rn(__dmul_rn(50.0, __dadd_rn(au, act[v])), pi);
                int64_t old;
                if (dupf[e]) {
                    atomicAdd(acc + v, t);
                    old = (int64_t)atomicMin(reinterpret_cast<long long*>(first + v), (long long)e);
                } else {
                    uc_stf(acc + v, __dadd_rn(uc_ldf(acc + v), t));
                    old = uc_ldi(first + v);
                    if (e < old) uc_sti(first + v, e);
                }
                if (old == UC_NONE) touched[atomicAdd(&s_cnt, 1)] = v;
            }
            __syncthreads();  // the next step's terms come after this one's
        }
        const int T = s_cnt;
        const int64_t cu = ue - ub;
        auto take = [&](int k, int32_t& v, double& val, int64_t& f) {
            v = touched[k];
            const int64_t cv = u_off[v + 1] - u_off[v];
            val = __ddiv_rn(uc_ldf(acc + v), __dsqrt_rn((double)(cu * cv)));
            f = uc_ldi(first + v);
            uc_stf(acc + v, 0.0);
            uc_sti(first + v, UC_NONE);
        };
        if constexpr (FULL) {
            const int64_t r0 = row_off[u];
            for (int k = tid; k < T; k += UC_THREADS) {
                int32_t v;
                double val;
                int64_t f;
                take(k, v, val, f);
                out_v[r0 + k] = v;
                out_s[r0 + k] = val;
                out_f[r0 + k] = f;
            }
        } else {
            for (int i = tid; i < 2 * K; i += UC_THREADS) {
                sel.s[i] = -INFINITY;
                sel.f[i] = UC_NONE;
                sel.c[i] = -1;
            }
            if (tid == 0) s_in = 0;
            __syncthreads();
            for (int k0 = 0; k0 < T; k0 += UC_THREADS) {
                const int held = s_in;  // read by every thread before any of them appends
                __syncthreads();
                if (held + UC_THREADS > K) uc_merge(sel, K, &s_in);
                const int k = k0 + tid;
                if (k < T) {
                    int32_t v;
                    double val;
                    int64_t f;
                    take(k, v, val, f);
                    // once topn entries are held, only a better one can enter
                    if (sel.c[topn - 1] < 0 || uc_better(val, f, sel.s[topn - 1], sel.f[topn - 1])) {
                        const int p = K + atomicAdd(&s_in, 1);
                        sel.s[p] = val;
                        sel.f[p] = f;
                        sel.c[p] = v;
                    }
                }
                __syncthreads();
            }
            uc_merge(sel, K, &s_in);
            const int m = T < topn ? T : topn;
            for (int r = tid; r < topn; r += UC_THREADS) {
                out_cols[u * topn + r] = r < m ? sel.c[r] : -1;
                out_vals[u * topn + r] = r < m ? sel.s[r] : 0.0;
            }
            if (tid == 0) {
                out_nnz[u] = T;
                out_cnt[u] = cu;
            }
        }
        __syncthreads();  // sel / touched / s_cnt are rewritten by the next row
    }
}

// ------------------------------------------------------------- recall --
// C_q = the summed history lengths of the query's neighbours
__global__ __launch_bounds__(256) void uc_count_kernel(const int64_t* __restrict__ q_slot, int64_t nq,
                                                       const int64_t* __restrict__ offsets,
                                                       const int32_t* __restrict__ nbr_cols,
                                                       const int32_t* __restrict__ nbr_cnt, int topn,
                                                       int64_t* __restrict__ cnt) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < nq; q += nw) {
        const int64_t sl = q_slot[q];
        int64_t c = 0;
        if (sl >= 0)
            for (int x = lane; x < nbr_cnt[sl]; x += 64) {
                const int32_t nb = nbr_cols[sl * topn + x];
                c += offsets[nb + 1] - offsets[nb];
            }
#pragma unroll
        for (int k = 32; k > 0; k >>= 1) c += __shfl_xor(c, k, WAVE);
        if (lane == 0) cnt[q] = c;
    }
}

struct UcParams {
    double created_alpha, ln_created;
    int topn, ke, bj;
};

__device__ __forceinline__ bool uc_find(const int32_t* __restrict__ cols, const double* __restrict__ vals, int n,
                                        int32_t key, double& v) {
    for (int x = 0; x < n; ++x)
        if (cols[x] == key) {
            v = vals[x];
            return true;
        }
    return false;
}

// One wave per query.  Neighbours in chunks of 64, one per lane; the
// (neighbour, position) candidates of a chunk are flattened over the wave,
// lane f taking flat candidate f0 + f (its neighbour by a binary search of
// the lane-scanned history lengths, as rc_gen_query does for positions).
// Every candidate i not in the query's history H contributes
//   ((loc_w * content_w) * created_w) * w_uv          (usercf_recaller.py:76-102)
// with content_w and created_w summed over H in history order.
__global__ __launch_bounds__(256) void uc_cand_kernel(
    const int64_t* __restrict__ q_slot, int64_t nq, const int64_t* __restrict__ offsets,
    const int32_t* __restrict__ items, const int32_t* __restrict__ nbr_cols, const double* __restrict__ nbr_vals,
    const int32_t* __restrict__ nbr_cnt, const double* __restrict__ loc_w, const double* __restrict__ created,
    const int32_t* __restrict__ emb_cols, const double* __restrict__ emb_vals, const int32_t* __restrict__ emb_cnt,
    UcParams prm, const int64_t* __restrict__ cand_off, uint64_t sentinel, uint64_t* __restrict__ keys,
    int32_t* __restrict__ slots, double* __restrict__ contrib) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < nq; q += nw) {
        const int64_t sl = q_slot[q];
        if (sl < 0) continue;
        const int64_t hb = offsets[sl], L = offsets[sl + 1] - hb;
        const double lw = loc_w[sl];
        const int nn = nbr_cnt[sl];
        int64_t c = cand_off[q];
        for (int x0 = 0; x0 < nn; x0 += 64) {
            const bool has = x0 + lane < nn;
            const int32_t nb = has ? nbr_cols[sl * prm.topn + x0 + lane] : 0;
            const double wl = has ? nbr_vals[sl * prm.topn + x0 + lane] : 0.0;
            const int64_t nbb = has ? offsets[nb] : 0;
            const int nl = has ? (int)(offsets[nb + 1] - nbb) : 0;
            int inc = nl;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(inc, d, 64);
                if (lane >= d) inc += t;
            }
            const int total = __shfl(inc, 63, 64);
            for (int f0 = 0; f0 < total; f0 += 64) {  // uniform: the shuffles run converged
                const int f = f0 + lane;
                int x = 0;
#pragma unroll
                for (int step = 32; step >= 1; step >>= 1)
                    if (__shfl(inc, x + step - 1, 64) <= f) x += step;
                x = x < 63 ? x : 63;  // lanes past total
                const int64_t pb = __shfl(nbb, x, 64);
                const int p = f - (__shfl(inc, x, 64) - __shfl(nl, x, 64));
                const double wuv = __shfl(wl, x, 64);
                if (f >= total) continue;
                const int32_t i = items[pb + p];
                const double ci = created[i];
                bool inh = false;
                double content = 1.0, crt = 1.0;
                for (int64_t l = 0; l < L; ++l) {
                    const int32_t j = items[hb + l];
                    inh |= j == i;
                    if (prm.ke > 0) {
                        double e;
                        if (uc_find(emb_cols + (int64_t)i * prm.ke, emb_vals + (int64_t)i * prm.ke, emb_cnt[i], j, e))
                            content = __dadd_rn(content, e);
                        if (uc_find(emb_cols + (int64_t)j * prm.ke, emb_vals + (int64_t)j * prm.ke, emb_cnt[j], i, e))
                            content = __dadd_rn(content, e);
                    }
                    // time_decay_weight(created_i, created_j, alpha = 0.8)
                    crt = __dadd_rn(crt, exp(cf_apow(prm.created_alpha, prm.ln_created, fabs(ci - created[j]))));
                }
                const double v = inh ? 0.0 : __dmul_rn(__dmul_rn(__dmul_rn(lw, content), crt), wuv);
                keys[c + f] = inh ? sentinel : (((uint64_t)q << prm.bj) | (uint32_t)i);
                slots[c + f] = (int32_t)(c + f);
                contrib[c + f] = v;
            }
            c += total;
        }
    }
}

struct UcWs {
    uint8_t* dupf;
    double* acc;
    int64_t* first;
    int32_t* touched;
    int grid;
    size_t bytes;
};

static UcWs uc_ws_layout(void* base, int64_t n_users, int64_t n_clicks) {
    UcWs w;
    Arena a(base);
    const size_t nu = (size_t)(n_users > 0 ? n_users : 1);
    w.grid = (int)(nu < (size_t)UC_GRID ? nu : (size_t)UC_GRID);
    w.dupf = (uint8_t*)a.take((size_t)(n_clicks > 0 ? n_clicks : 1));
    w.acc = (double*)a.take(nu * w.grid * 8);
    w.first = (int64_t*)a.take(nu * w.grid * 8);
    w.touched = (int32_t*)a.take(nu * w.grid * 4);
    w.bytes = a.bytes;
    return w;
}

static inline int uc_sel_k(int topn) {
    int k = UC_THREADS;
    while (k < topn) k <<= 1;
    return k;
}

}  // namespace nrk

using namespace nrk;

extern "C" {

size_t nrk_usercf_workspace_bytes(int64_t n_users, int64_t n_clicks, int topn) {
    if (n_users < 0 || n_clicks < 0 || topn < 1) return 0;
    return uc_ws_layout(nullptr, n_users, n_clicks).bytes;
}

#define UC_CHECK_INPUTS()                                                                               \
    NRK_REQUIRE(n_users >= 0 && n_clicks >= 0 && n_items >= 0, "negative size");                        \
    NRK_REQUIRE(n_users < INT32_MAX && n_clicks < (int64_t(1) << 40), "n_users / n_clicks too large"); \
    NRK_REQUIRE(i_off && u_off, "null pointer");                                                        \
    NRK_REQUIRE(n_clicks == 0 || (i_users && u_items && act && pen && workspace), "null pointer")

int nrk_usercf_topn(const int64_t* i_off, int32_t n_items, const int32_t* i_users, const int64_t* u_off,
                    int64_t n_users, const int32_t* u_items, int64_t n_clicks, const double* act, const double* pen,
                    int topn, int32_t* out_cols, double* out_vals, int64_t* out_cnt, int32_t* out_nnz,
                    void* workspace, size_t workspace_bytes, nrk_stream_t stream) {
    clear_error();
    NRK_REQUIRE(topn >= 1, "topn must be >= 1");
    if (topn > UC_SEL) NRK_UNSUPPORTED("topn must be <= 1024");
    UC_CHECK_INPUTS();
    if (n_users == 0) return NRK_OK;
    NRK_REQUIRE(out_cols && out_vals && out_cnt && out_nnz && act && pen && workspace, "null pointer");
    const UcWs w = uc_ws_layout(workspace, n_users, n_clicks);
    NRK_REQUIRE(workspace_bytes >= w.bytes, "workspace too small");
    hipStream_t s = as_stream(stream);
    if (n_clicks > 0) {
        uc_dup_kernel<<<grid_for(n_clicks, 256, 4096), 256, 0, s>>>(i_off, n_items, i_users, u_off, u_items, n_clicks,
                                                                    w.dupf);
    }
    uc_rows_kernel<false><<<w.grid, UC_THREADS, 0, s>>>(i_off, i_users, u_off, u_items, act, pen, w.dupf, n_users,
                                                        w.acc, w.first, w.touched, topn, uc_sel_k(topn), out_cols,
                                                        out_vals, out_cnt, out_nnz, nullptr, nullptr, nullptr,
                                                        nullptr);
    NRK_CHECK_LAUNCH();
    return NRK_OK;
}

int nrk_usercf_sim(const int64_t* i_off, int32_t n_items, const int32_t* i_users, const int64_t* u_off,
                   int64_t n_users, const int32_t* u_items, int64_t n_clicks, const double* act, const double* pen,
                   const int64_t* row_off, int64_t n_entries, int32_t* out_v, double* out_s, int64_t* out_first,
                   void* workspace, size_t workspace_bytes, nrk_stream_t stream) {
    clear_error();
    UC_CHECK_INPUTS();
    NRK_REQUIRE(n_entries >= 0, "negative size");
    if (n_users == 0 || n_entries == 0) return NRK_OK;
    NRK_REQUIRE(row_off && out_v && out_s && out_first && act && pen && workspace, "null pointer");
    const UcWs w = uc_ws_layout(workspace, n_users, n_clicks);
    NRK_REQUIRE(workspace_bytes >= w.bytes, "workspace too small");
    hipStream_t s = as_stream(stream);
    if (n_clicks > 0) {
        uc_dup_kernel<<<grid_for(n_clicks, 256, 4096), 256, 0, s>>>(i_off, n_items, i_users, u_off, u_items, n_clicks,
                                                                    w.dupf);
    }
    uc_rows_kernel<true><<<w.grid, UC_THREADS, 0, s>>>(i_off, i_users, u_off, u_items, act, pen, w.dupf, n_users,
                                                       w.acc, w.first, w.touched, 1, UC_THREADS, nullptr, nullptr,
                                                       nullptr, nullptr, row_off, out_v, out_s, out_first);
    NRK_CHECK_LAUNCH();
    return NRK_OK;
}

int nrk_usercf_recall_offsets(const int64_t* q_slot, int64_t n_query, const int64_t* offsets,
                              const int32_t* nbr_cols, const int32_t* nbr_cnt, int topn, int64_t* cand_off,
                              nrk_stream_t stream) {
    clear_error();
    NRK_REQUIRE(n_query >= 0, "n_query < 0");
    NRK_REQUIRE(topn >= 1, "topn must be >= 1");
    NRK_REQUIRE(cand_off, "null pointer");
    hipStream_t s = as_stream(stream);
    if (n_query > 0) {
        NRK_REQUIRE(q_slot && offsets && nbr_cols && nbr_cnt, "null pointer");
        uc_count_kernel<<<grid_for(n_query, 4, 65536), 256, 0, s>>>(q_slot, n_query, offsets, nbr_cols, nbr_cnt, topn,
                                                                    cand_off);
    }
    rc_scan_exclusive(cand_off, n_query, s);
    NRK_CHECK_LAUNCH();
    return NRK_OK;
}

size_t nrk_usercf_recall_workspace_bytes(int64_t n_cand) {
    if (n_cand < 0) return 0;
    return rc_back_bytes(n_cand);
}

int nrk_usercf_recall(const int64_t* q_slot, int64_t n_query, const int64_t* offsets, const int32_t* items,
                      const int32_t* nbr_cols, const double* nbr_vals, const int32_t* nbr_cnt, int topn,
                      const double* loc_w, const double* created, int32_t n_items, const int32_t* hot, int n_hot,
                      const int32_t* emb_cols, const double* emb_vals, const int32_t* emb_cnt, int ke,
                      double created_alpha, const int64_t* cand_off, int64_t n_cand, int topk, int32_t* out_items,
                      double* out_scores, int32_t* out_src, int32_t* out_cnt, void* workspace,
                      size_t workspace_bytes, nrk_stream_t stream) {
    clear_error();
    NRK_REQUIRE(n_query >= 0 && n_cand >= 0 && n_hot >= 0, "negative size");
    NRK_REQUIRE(topk >= 1, "topk must be >= 1");
    if (topk > RC_TOPK_MAX) NRK_UNSUPPORTED("topk must be <= 2048");
    NRK_REQUIRE(topn >= 1 && n_items >= 1 && ke >= 0, "bad sizes");
    NRK_REQUIRE(n_cand < RC_CAND_MAX, "n_cand must be < 2^31");
    if (n_query == 0) return NRK_OK;
    NRK_REQUIRE(q_slot && offsets && items && nbr_cols && nbr_vals && nbr_cnt && loc_w && created && cand_off &&
                    out_items && out_scores && out_src && out_cnt && workspace,
                "null pointer");
    NRK_REQUIRE(n_hot == 0 || hot, "hot is null");
    NRK_REQUIRE(ke == 0 || (emb_cols && emb_vals && emb_cnt), "emb arrays null");
    NRK_REQUIRE(workspace_bytes >= rc_back_bytes(n_cand), "workspace too small");
    hipStream_t s = as_stream(stream);
    RcBack bk;
    if (!rc_back_buffers(workspace, n_query, n_items, n_cand, &bk))
        NRK_UNSUPPORTED("n_query * n_items too large for 64-bit keys");
    const UcParams prm{created_alpha, cf_ln(created_alpha), topn, ke, bk.bj};
    if (n_cand > 0)
        uc_cand_kernel<<<grid_for(n_query, 4, 65536), 256, 0, s>>>(
            q_slot, n_query, offsets, items, nbr_cols, nbr_vals, nbr_cnt, loc_w, created, emb_cols, emb_vals,
            emb_cnt, prm, cand_off, bk.sentinel, bk.keys, bk.slots, bk.contrib);
    return rc_back_finish(q_slot, n_query, offsets, items, n_items, hot, n_hot, cand_off, n_cand, topk, out_items,
                          out_scores, out_src, out_cnt, workspace, s);
}

}  // extern "C"
