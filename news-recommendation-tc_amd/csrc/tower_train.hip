// tower_train.hip -- YouTubeDNN training step on gfx950: fused forward + BCE
// loss + backward, a bitwise-reproducible scatter of the embedding gradients,
// a dense-semantics Adam sweep, and the sample generator.
//
// Replaces YoutubeDNNRecaller.train's loop body and _prepare_data
// (src/recall/youtubednn_recaller.py:211-423).  A batch of 256 samples
// touches at most 256 x 32 embedding rows and an MLP that fits in LDS: the
// step is bound by launch count and latency, so it is
//   1. tt_train_fb_kernel    one wave per sample: gather, forward, loss and
//                            the backward down to dx; stores the layer
//                            inputs, the layer deltas and three dim-vectors
//                            per sample (d user row, d history row, d target)
//   2. tt_wgrad_kernel       dW_l = delta_l^T A_{l-1}, db_l, and the mean
//                            loss: fixed batch slices, fixed tree
//   3. tt_emb_sort_kernel    per chunk of samples and per table: keys
//                            (row, contribution) sorted in LDS, one sum per
//                            destination row in ascending contribution order
//  (4. mark / count / compact / merge only when the batch spans several chunks)
//   5. adam_sweep_kernel     one sweep over weights and both tables
//                            (train_common.h)
// No floating-point atomics anywhere, so every output is bitwise reproducible.
#include <algorithm>

#include "tower_common.h"
#include "train_common.h"

namespace nrk {

constexpr int TR_MAXB = 8192, TR_MAXT = 64;
constexpr int TR_KEYS = 8192;  // keys one workgroup sorts in LDS (6 bytes each)

// ------------------------------------------------------------ generator --
// Counter-based: a pure function of (seed, a, b, c, d), splitmix64's
// finaliser over the folded counters.  Dropout keeps a unit iff the draw is
// >= thr = p * 2^32; the backward pass recomputes nothing because a kept
// unit is recognisable from its stored activation (> 0).
__host__ __device__ inline uint64_t tr_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t tr_key(uint64_t seed, uint64_t a, uint32_t b, uint32_t c) {
    const uint64_t k = tr_mix(seed + 0x9E3779B97F4A7C15ull * (a + 1));
    return tr_mix(k ^ (((uint64_t)b << 32) | c));
}
__host__ __device__ inline uint32_t tr_draw(uint64_t key, uint32_t d) {
    return (uint32_t)(tr_mix(key + 0x9E3779B97F4A7C15ull * ((uint64_t)d + 1)) >> 32);
}
static inline uint32_t tr_threshold(float p) {
    const double t = (double)p * 4294967296.0;
    return (uint32_t)std::min(t, 4294967295.0);
}

// --------------------------------------------- 1. forward + loss + backward --
// LDS: per wave [layer inputs A_0 .. A_L (asz) | two delta rows (2 x 256)],
// then, when it fits, the packed weights with each row padded by one float
// (lane o reads row o in the forward; an odd stride spreads the banks, and
// the backward's lane q reads consecutive words).
template <int D>
__global__ __launch_bounds__(256) void tt_train_fb_kernel(
    const float* __restrict__ user_table, const float* __restrict__ item_table, const float* __restrict__ wts,
    TtLayers ly, const int64_t* __restrict__ log_off, const int32_t* __restrict__ log_items,
    const int32_t* __restrict__ s_user, const int32_t* __restrict__ s_pos, const int32_t* __restrict__ s_target,
    const float* __restrict__ s_label, int B, int T, float scale, uint32_t thr, uint64_t seed, uint64_t step,
    int asz, int dsz, int staged, float* __restrict__ loss_b, float* __restrict__ act, float* __restrict__ delta,
    float* __restrict__ gU, float* __restrict__ gH, float* __restrict__ gT) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* sa = lds + wave * (asz + 2 * TT_MAXW);
    float* sd[2] = {sa + asz, sa + asz + TT_MAXW};
    float* sw = lds + 4 * (asz + 2 * TT_MAXW);
    if (staged) {
        int in = 2 * D;
        const float* src = wts;
        float* dst = sw;
        for (int l = 0; l < ly.n; ++l) {
            const int wo = ly.w[l];
            for (int i = threadIdx.x; i < wo * in; i += blockDim.x) dst[(i / in) * (in + 1) + i % in] = src[i];
            for (int i = threadIdx.x; i < wo; i += blockDim.x) dst[wo * (in + 1) + i] = src[wo * in + i];
            src += wo * in + wo;
            dst += wo * (in + 1) + wo;
            in = wo;
        }
        __syncthreads();
    }
    const float* wbase = staged ? sw : wts;
    const int pad = staged ? 1 : 0;
    const float invB = 1.0f / (float)B;
    for (int b = blockIdx.x * 4 + wave; b < B; b += gridDim.x * 4) {
        const int u = s_user[b];
        const int len = min(s_pos[b], T);
        const int32_t tgt = s_target[b];
        const float y = s_label[b];
        const int64_t base = log_off[u];
        const int32_t hv = lane < len ? log_items[base + lane] : 0;
        const float xu = user_table[(int64_t)u * D + lane % D];
        const float tv = lane < D ? item_table[(int64_t)tgt * D + lane] : 0.0f;
        const float xm = tt_hist_mean<D>(item_table, hv, len, len, lane);
        const float cnt = (float)len + 1e-8f;  // the mean's denominator, again in the backward
        if (lane < D) {
            sa[lane] = xu;
            sa[D + lane] = xm;
        }
        wave_sync_lds();
        // forward: A_{l+1} = dropout(relu(W_l A_l + b_l))
        int in = 2 * D, aoff = 0;
        const float* wl = wbase;
        for (int l = 0; l < ly.n; ++l) {
            const int wo = ly.w[l], ws = in + pad;
            const float* bl = wl + (size_t)wo * ws;
            const float* a = sa + aoff;
            float* o_ = sa + aoff + in;
            const uint64_t key = thr ? tr_key(seed, step, (uint32_t)l, (uint32_t)b) : 0;
            for (int o = lane; o < wo; o += WAVE) {
                // not shared with the forward kernels: theirs run with contraction off, this one may fuse
                float z = bl[o];
                const float* wr = wl + (size_t)o * ws;
                for (int q = 0; q < in; ++q) z += wr[q] * a[q];
                float r = fmaxf(z, 0.0f);
                if (thr) r = tr_draw(key, (uint32_t)o) >= thr ? r * scale : 0.0f;
                o_[o] = r;
            }
            wave_sync_lds();
            wl = bl + wo;
            aoff += in;
            in = wo;
        }
        // heads: u = x / max(|x|, eps), v = e / max(|e|, eps), logit = u . v
        const float x = lane < D ? sa[aoff + lane] : 0.0f;
        const float nx = sqrtf(wave_sum_f32(x * x));
        const float uh = x / fmaxf(nx, 1e-12f);
        const float nt = sqrtf(wave_sum_f32(tv * tv));
        const float vh = tv / fmaxf(nt, 1e-12f);
        const float logit = wave_sum_f32(uh * vh);
        // BCE with logits, overflow-safe: max(x, 0) - x y + log1p(exp(-|x|))
        const float e = expf(-fabsf(logit));
        if (lane == 0) loss_b[b] = fmaxf(logit, 0.0f) - logit * y + log1pf(e);
        const float sig = logit >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e);
        const float dl = (sig - y) * invB;
        const float du = dl * vh, dv = dl * uh;
        // normalize backward with the clamp: below eps the denominator is the
        // constant eps and there is no norm term
        const float su = wave_sum_f32(uh * du), sv = wave_sum_f32(vh * dv);
        const float dx = nx >= 1e-12f ? (du - uh * su) / nx : du / 1e-12f;
        const float dt = nt >= 1e-12f ? (dv - vh * sv) / nt : dv / 1e-12f;
        if (lane < D) {
            gT[(int64_t)b * D + lane] = dt;
            sd[0][lane] = dx;
        }
        wave_sync_lds();
        // backward: delta_l = dA_{l+1} * scale where the unit is alive and
        // kept (A_{l+1} > 0; ReLU'(0) = 0), dA_l = W_l^T delta_l
        int cur = 0, doff = dsz;
        for (int l = ly.n - 1; l >= 0; --l) {
            const int wo = ly.w[l];
            in = l ? ly.w[l - 1] : 2 * D;
            const int ws = in + pad;
            aoff -= in;  // A_l starts here, A_{l+1} at aoff + in
            wl -= (size_t)wo * ws + wo;
            doff -= wo;
            const float* aout = sa + aoff + in;
            for (int o = lane; o < wo; o += WAVE) {
                const float g = aout[o] > 0.0f ? sd[cur][o] * scale : 0.0f;
                sd[cur][o] = g;
                delta[(int64_t)b * dsz + doff + o] = g;
            }
            wave_sync_lds();
            for (int q = lane; q < in; q += WAVE) {
                float s = 0.0f;
                for (int o = 0; o < wo; ++o) s += wl[(size_t)o * ws + q] * sd[cur][o];
                sd[cur ^ 1][q] = s;
            }
            wave_sync_lds();
            cur ^= 1;
        }
        if (lane < D) {
            gU[(int64_t)b * D + lane] = sd[cur][lane];
            gH[(int64_t)b * D + lane] = sd[cur][D + lane] / cnt;
        }
        for (int i = lane; i < asz; i += WAVE) act[(int64_t)b * asz + i] = sa[i];
        wave_sync_lds();  // sa / sd are rewritten for the next sample
    }
}

// ------------------------------------------- 2. weight gradients + the loss --
// Block = 64 consecutive packed weights x 16 batch slices (one wave each,
// b ascending inside a slice); the 16 partials are added in slice order.
// The last block reduces the per-sample losses the same way.
__global__ __launch_bounds__(1024) void tt_wgrad_kernel(const float* __restrict__ act,
                                                        const float* __restrict__ delta,
                                                        const float* __restrict__ loss_b, TtLayers ly, int D,
                                                        int B, int asz, int dsz, int n_w,
                                                        float* __restrict__ w_grad, float* __restrict__ loss) {
    __shared__ float part[16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per = (B + 15) / 16, b0 = wave * per, b1 = min(B, b0 + per);
    float s = 0.0f;
    const bool loss_block = blockIdx.x == gridDim.x - 1;
    const int e = blockIdx.x * 64 + lane;
    if (loss_block) {
        for (int b = b0 + lane; b < b1; b += WAVE) s += loss_b[b];
    } else if (e < n_w) {
        int in = 2 * D, off = 0, aoff = 0, doff = 0, l = 0;
        while (e >= off + ly.w[l] * (in + 1)) {
            off += ly.w[l] * (in + 1);
            aoff += in;
            doff += ly.w[l];
            in = ly.w[l];
            ++l;
        }
        const int r = e - off;
        if (r < ly.w[l] * in) {
            const float* dp = delta + doff + r / in;
            const float* ap = act + aoff + r % in;
            for (int b = b0; b < b1; ++b) s += dp[(int64_t)b * dsz] * ap[(int64_t)b * asz];
        } else {
            const float* dp = delta + doff + (r - ly.w[l] * in);
            for (int b = b0; b < b1; ++b) s += dp[(int64_t)b * dsz];
        }
    }
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0) {
        float t = 0.0f;
        for (int k = 0; k < 16; ++k) t += part[k][lane];
        if (loss_block) {
            t = wave_sum_f32(t);  // xor butterfly: a fixed tree
            if (lane == 0) *loss = t / (float)B;
        } else if (e < n_w) {
            w_grad[e] = t;
        }
    }
}

// ------------------------------------------------ 3. embedding gradients --
// Exclusive scan of one int per thread over a 1024-thread block.
__device__ inline int tr_block_scan(int v, int* tmp /* [17] */, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const int y = __shfl_up(x, off, WAVE);
        if (lane >= off) x += y;
    }
    if (lane == WAVE - 1) tmp[wave] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0;
        for (int w = 0; w < 16; ++w) {
            const int t = tmp[w];
            tmp[w] = a;
            a += t;
        }
        tmp[16] = a;
    }
    __syncthreads();
    const int r = x - v + tmp[wave];
    total = tmp[16];
    __syncthreads();
    return r;
}

struct TrTable {
    int32_t* rows;  // [chunk][cap]
    float* vals;    // [chunk][cap][D]
    int32_t* count; // [chunk]
    int cap;
};

// grid (chunks, 2): y = 0 the user table (one key per sample), y = 1 the item
// table (min(pos, T) history keys and one target key per sample).  A key is
// (row, contribution id); contribution id = local sample * (T + 1) + slot, so
// a row's contributions are summed in (sample, slot) order.
__global__ __launch_bounds__(1024) void tt_emb_sort_kernel(
    const int64_t* __restrict__ log_off, const int32_t* __restrict__ log_items, const int32_t* __restrict__ s_user,
    const int32_t* __restrict__ s_pos, const int32_t* __restrict__ s_target, int B, int T, int CS, int D,
    const float* __restrict__ gU, const float* __restrict__ gH, const float* __restrict__ gT, TrTable tu,
    TrTable ti) {
    extern __shared__ __attribute__((aligned(16))) unsigned char raw[];
    __shared__ int s_off[256], s_len[256], tmp[17];
    __shared__ int64_t s_base[256];
    uint32_t* krow = reinterpret_cast<uint32_t*>(raw);
    uint16_t* kcid = reinterpret_cast<uint16_t*>(raw + (size_t)TR_KEYS * 4);
    const bool item = blockIdx.y == 1;
    const TrTable tb = item ? ti : tu;
    const int chunk = blockIdx.x, bb = chunk * CS, nb = min(CS, B - bb), tid = threadIdx.x;
    int32_t* rows = tb.rows + (size_t)chunk * tb.cap;
    float* vals = tb.vals + (size_t)chunk * tb.cap * D;
    int len = 0;
    if (tid < nb) {
        len = min(s_pos[bb + tid], T);
        s_len[tid] = len;
        s_base[tid] = log_off[s_user[bb + tid]];
    }
    int total;
    const int off = tr_block_scan(tid < nb ? (item ? len + 1 : 1) : 0, tmp, total);
    if (tid < nb) s_off[tid] = off;
    int n2 = 128;  // a wave sorts aligned groups of 128 keys on its own (below)
    while (n2 < total) n2 <<= 1;
    for (int i = tid; i < n2; i += blockDim.x) {
        krow[i] = 0xFFFFFFFFu;  // sentinels sort behind every real row
        kcid[i] = 0xFFFFu;
    }
    __syncthreads();
    if (item) {
        for (int i = tid; i < nb * (T + 1); i += blockDim.x) {
            const int bl = i / (T + 1), t = i % (T + 1), l = s_len[bl];
            if (t < l) {
                krow[s_off[bl] + t] = (uint32_t)log_items[s_base[bl] + t];
                kcid[s_off[bl] + t] = (uint16_t)i;
            } else if (t == T) {
                krow[s_off[bl] + l] = (uint32_t)s_target[bb + bl];
                kcid[s_off[bl] + l] = (uint16_t)i;
            }
        }
    } else if (tid < nb) {
        krow[off] = (uint32_t)s_user[bb + tid];
        kcid[off] = (uint16_t)tid;
    }
    __syncthreads();
    // Bitonic sort, ascending (row, cid).  A stage of distance j <= 64 pairs
    // keys inside one aligned group of 128, so a wave runs those stages over
    // its own groups with wave-level synchronisation only; the workgroup
    // meets at a barrier for the stages of distance >= 128 alone (21 instead
    // of 91 barriers at 8,192 keys).
    auto exchange = [&](int lo, int j, int k) {
        const int hi = lo + j;
        const uint32_t ra = krow[lo], rb = krow[hi];
        const uint16_t ca = kcid[lo], cb = kcid[hi];
        const bool gt = ra > rb || (ra == rb && ca > cb);
        if (gt == ((lo & k) == 0)) {
            krow[lo] = rb;
            krow[hi] = ra;
            kcid[lo] = cb;
            kcid[hi] = ca;
        }
    };
    const int lane = tid & 63, wave = tid >> 6;
    auto wave_stages = [&](int k, int j0) {  // distances j0, j0 / 2, ..., 1 of merge size k; j0 <= 64
        for (int base = wave * 128; base < n2; base += 16 * 128) {
            for (int j = j0; j > 0; j >>= 1) {
                exchange(base + 2 * j * (lane / j) + (lane % j), j, k);
                wave_sync_lds();
            }
        }
    };
    for (int k = 2; k <= 128; k <<= 1) wave_stages(k, k >> 1);
    for (int k = 256; k <= n2; k <<= 1) {
        for (int j = k >> 1; j >= 128; j >>= 1) {
            __syncthreads();
            for (int i = tid; i < n2 / 2; i += blockDim.x) exchange(2 * j * (i / j) + (i % j), j, k);
        }
        __syncthreads();
        wave_stages(k, 64);
    }
    __syncthreads();
    // segment heads -> unique rows (ascending) and segment starts
    // (each thread keeps its 8 keys' rows; once every thread has looked, the
    // sorted rows are no longer needed and krow[slot] takes the segment start)
    constexpr int PER = TR_KEYS / 1024;
    uint32_t mine[PER];
    unsigned head_mask = 0;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const int i = tid * PER + e;
        mine[e] = i < total ? krow[i] : 0;
        if (i < total && (i == 0 || mine[e] != krow[i - 1])) head_mask |= 1u << e;
    }
    int nuniq;
    int slot = tr_block_scan(__popc(head_mask), tmp, nuniq);  // its barriers end the reads of krow
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        if (head_mask >> e & 1) {
            rows[slot] = (int32_t)mine[e];
            krow[slot] = (uint32_t)(tid * PER + e);  // slot <= position
            ++slot;
        }
    }
    if (tid == 0) tb.count[chunk] = nuniq;
    __syncthreads();
    for (int i = tid; i < nuniq * D; i += blockDim.x) {
        const int s = i / D, d = i % D;
        float acc = 0.0f;
        const int end = s + 1 < nuniq ? (int)krow[s + 1] : total;
        for (int k = (int)krow[s]; k < end; ++k) {
            const int cid = kcid[k];
            const float* src;
            if (item) {
                const int bl = cid / (T + 1);
                src = (cid % (T + 1) == T ? gT : gH) + (int64_t)(bb + bl) * D;
            } else {
                src = gU + (int64_t)(bb + cid) * D;
            }
            acc += src[d];
        }
        vals[(size_t)s * D + d] = acc;
    }
}

// ---- 4. several chunks: the union of their rows through a dense mark array --
__global__ __launch_bounds__(256) void tt_emb_mark_kernel(TrTable tu, TrTable ti, int32_t* __restrict__ mark_u,
                                                          int32_t* __restrict__ mark_i) {
    const TrTable tb = blockIdx.y ? ti : tu;
    int32_t* mark = blockIdx.y ? mark_i : mark_u;
    const int n = tb.count[blockIdx.x];
    const int32_t* rows = tb.rows + (size_t)blockIdx.x * tb.cap;
    for (int i = threadIdx.x; i < n; i += blockDim.x) mark[rows[i]] = 1;
}

// Compaction of the mark arrays in tiles of TR_CT rows (grid (tiles, 2),
// thread t owns 4 consecutive rows): the first pass counts each tile's marks,
// the second adds the counts of the tiles before its own and writes the rows.
constexpr int TR_CT = 4096;
__global__ __launch_bounds__(1024) void tt_emb_count_kernel(const int32_t* __restrict__ mark_u, int64_t n_u,
                                                            const int32_t* __restrict__ mark_i, int64_t n_i,
                                                            int32_t* __restrict__ blk_u,
                                                            int32_t* __restrict__ blk_i) {
    __shared__ int tmp[17];
    const int32_t* mark = blockIdx.y ? mark_i : mark_u;
    const int64_t n = blockIdx.y ? n_i : n_u, r0 = (int64_t)blockIdx.x * TR_CT + threadIdx.x * 4;
    if ((int64_t)blockIdx.x * TR_CT >= n) return;  // block-uniform
    int c = 0;
    for (int e = 0; e < 4; ++e) c += r0 + e < n && mark[r0 + e] != 0;
    int total;
    tr_block_scan(c, tmp, total);
    if (threadIdx.x == 0) (blockIdx.y ? blk_i : blk_u)[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void tt_emb_compact_kernel(const int32_t* __restrict__ mark_u, int64_t n_u,
                                                              const int32_t* __restrict__ mark_i, int64_t n_i,
                                                              const int32_t* __restrict__ blk_u,
                                                              const int32_t* __restrict__ blk_i,
                                                              int32_t* __restrict__ u_rows,
                                                              int32_t* __restrict__ u_count,
                                                              int32_t* __restrict__ i_rows,
                                                              int32_t* __restrict__ i_count) {
    __shared__ int tmp[17];
    __shared__ int before;
    const int32_t* mark = blockIdx.y ? mark_i : mark_u;
    const int32_t* blk = blockIdx.y ? blk_i : blk_u;
    int32_t* out = blockIdx.y ? i_rows : u_rows;
    const int64_t n = blockIdx.y ? n_i : n_u, r0 = (int64_t)blockIdx.x * TR_CT + threadIdx.x * 4;
    if ((int64_t)blockIdx.x * TR_CT >= n) return;  // block-uniform
    if (threadIdx.x < WAVE) {
        int s = 0;
        for (int t = threadIdx.x; t < (int)blockIdx.x; t += WAVE) s += blk[t];
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m, WAVE);
        if (threadIdx.x == 0) before = s;
    }
    int c = 0;
    for (int e = 0; e < 4; ++e) c += r0 + e < n && mark[r0 + e] != 0;
    int total;
    int slot = tr_block_scan(c, tmp, total) + before;  // the scan's barriers publish `before`
    for (int e = 0; e < 4; ++e)
        if (r0 + e < n && mark[r0 + e]) out[slot++] = (int32_t)(r0 + e);
    if (threadIdx.x == 0 && ((int64_t)blockIdx.x + 1) * TR_CT >= n) *(blockIdx.y ? i_count : u_count) = before + total;
}

// out_vals[slot] = sum over the chunks, in chunk order, of the chunk's value
// for that row (binary search in the chunk's ascending rows)
__global__ __launch_bounds__(256) void tt_emb_merge_kernel(TrTable tu, TrTable ti, int n_chunks, int D,
                                                           const int32_t* __restrict__ u_rows,
                                                           const int32_t* __restrict__ u_count,
                                                           float* __restrict__ u_vals,
                                                           const int32_t* __restrict__ i_rows,
                                                           const int32_t* __restrict__ i_count,
                                                           float* __restrict__ i_vals) {
    const TrTable tb = blockIdx.y ? ti : tu;
    const int32_t* orow = blockIdx.y ? i_rows : u_rows;
    float* oval = blockIdx.y ? i_vals : u_vals;
    const int64_t n = (int64_t)*(blockIdx.y ? i_count : u_count) * D;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / D;
        const int d = (int)(i % D);
        const int32_t row = orow[s];
        float acc = 0.0f;
        for (int c = 0; c < n_chunks; ++c) {
            const int32_t* rows = tb.rows + (size_t)c * tb.cap;
            int lo = 0, hi = tb.count[c];
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (rows[mid] < row) lo = mid + 1;
                else hi = mid;
            }
            if (lo < tb.count[c] && rows[lo] == row) acc += tb.vals[((size_t)c * tb.cap + lo) * D + d];
        }
        oval[i] = acc;
    }
}

// ------------------------------------------------------------- 5. dropout --
__global__ __launch_bounds__(256) void tt_dropout_mask_kernel(uint64_t seed, uint64_t step, int layer, int batch,
                                                              int width, uint32_t thr, float* __restrict__ out) {
    const int64_t n = (int64_t)batch * width;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / width), o = (int)(i % width);
        out[i] = !thr || tr_draw(tr_key(seed, step, (uint32_t)layer, (uint32_t)b), (uint32_t)o) >= thr ? 1.0f : 0.0f;
    }
}

// ------------------------------------------------------------- 6. samples --
__device__ __forceinline__ int64_t tr_n_pos(int64_t n) {
    if (n < 2) return 0;
    const int64_t test = std::max<int64_t>(1, (int64_t)((double)n * 0.2));  // max(1, int(n * 0.2))
    return std::max<int64_t>(0, n - test - 1);                              // i in [1, train_end)
}

__global__ __launch_bounds__(1024) void tt_sample_count_kernel(const int64_t* __restrict__ log_off, int64_t n_users,
                                                               int64_t* __restrict__ pos_off) {
    __shared__ int64_t tot[1024];
    const int64_t per = (n_users + 1023) / 1024, u0 = std::min<int64_t>(n_users, threadIdx.x * per),
                  u1 = std::min<int64_t>(n_users, u0 + per);
    int64_t c = 0;
    for (int64_t u = u0; u < u1; ++u) c += tr_n_pos(log_off[u + 1] - log_off[u]);
    tot[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t a = 0;
        for (int t = 0; t < 1024; ++t) {
            const int64_t x = tot[t];
            tot[t] = a;
            a += x;
        }
        pos_off[n_users] = a;
    }
    __syncthreads();
    c = tot[threadIdx.x];
    for (int64_t u = u0; u < u1; ++u) {
        pos_off[u] = c;
        c += tr_n_pos(log_off[u + 1] - log_off[u]);
    }
}

__global__ __launch_bounds__(256) void tt_make_samples_kernel(
    const int64_t* __restrict__ log_off, const int32_t* __restrict__ log_items, int64_t n_users,
    const int64_t* __restrict__ pos_off, int64_t n_pos, int neg, const int32_t* __restrict__ pool, int64_t n_pool,
    uint64_t seed, int32_t* __restrict__ s_user, int32_t* __restrict__ s_pos, int32_t* __restrict__ s_target,
    float* __restrict__ s_label) {
    const int64_t n = n_pos * (1 + neg);
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = j / (1 + neg);
        const int k = (int)(j % (1 + neg));
        int64_t lo = 0, hi = n_users;  // the last user with pos_off[user] <= p
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (pos_off[mid] <= p) lo = mid;
            else hi = mid;
        }
        const int64_t i = 1 + p - pos_off[lo];
        s_user[j] = (int32_t)lo;
        s_pos[j] = (int32_t)i;
        s_label[j] = k == 0 ? 1.0f : 0.0f;
        if (k == 0) {
            s_target[j] = log_items[log_off[lo] + i];
        } else {
            const uint32_t r = tr_draw(tr_key(seed, (uint64_t)p, 0xFFFFFFFFu, (uint32_t)k), 0);
            s_target[j] = pool[(int64_t)(((uint64_t)r * (uint64_t)n_pool) >> 32)];
        }
    }
}

// ------------------------------------------------------------------ host --
struct TrWs {
    float *loss_b, *act, *delta, *gU, *gH, *gT;
    int32_t *crow_u, *ccnt_u, *crow_i, *ccnt_i, *mark_u, *mark_i, *blk_u, *blk_i;
    float *cval_u, *cval_i;
    int CS, n_chunks, cap_i, asz, dsz;
    size_t mark_bytes, bytes;
};

static TrWs tr_layout(void* base, int64_t U, int64_t I, int D, const TtLayers& ly, int T, int B) {
    TrWs w{};
    w.asz = 2 * D;
    for (int l = 0; l < ly.n; ++l) {
        w.asz += ly.w[l];
        w.dsz += ly.w[l];
    }
    w.CS = std::min(256, TR_KEYS / (T + 1));
    w.n_chunks = (B + w.CS - 1) / w.CS;
    w.cap_i = w.CS * (T + 1);
    Arena a(base);
    w.loss_b = (float*)a.take(sizeof(float) * B);
    w.act = (float*)a.take(sizeof(float) * (size_t)B * w.asz);
    w.delta = (float*)a.take(sizeof(float) * (size_t)B * w.dsz);
    w.gU = (float*)a.take(sizeof(float) * (size_t)B * D);
    w.gH = (float*)a.take(sizeof(float) * (size_t)B * D);
    w.gT = (float*)a.take(sizeof(float) * (size_t)B * D);
    if (w.n_chunks > 1) {
        w.crow_u = (int32_t*)a.take(sizeof(int32_t) * (size_t)w.n_chunks * w.CS);
        w.cval_u = (float*)a.take(sizeof(float) * (size_t)w.n_chunks * w.CS * D);
        w.ccnt_u = (int32_t*)a.take(sizeof(int32_t) * w.n_chunks);
        w.crow_i = (int32_t*)a.take(sizeof(int32_t) * (size_t)w.n_chunks * w.cap_i);
        w.cval_i = (float*)a.take(sizeof(float) * (size_t)w.n_chunks * w.cap_i * D);
        w.ccnt_i = (int32_t*)a.take(sizeof(int32_t) * w.n_chunks);
        w.mark_u = (int32_t*)a.take(sizeof(int32_t) * (size_t)(U + I));  // mark_u | mark_i: one memset
        w.mark_i = w.mark_u ? w.mark_u + U : nullptr;
        w.mark_bytes = sizeof(int32_t) * (size_t)(U + I);
        w.blk_u = (int32_t*)a.take(sizeof(int32_t) * (size_t)((U + TR_CT - 1) / TR_CT));
        w.blk_i = (int32_t*)a.take(sizeof(int32_t) * (size_t)((I + TR_CT - 1) / TR_CT));
    }
    w.bytes = a.bytes;
    return w;
}

static int tr_check_shapes(const char* fn, int64_t U, int64_t I, int dim, int n_layers, const int* widths,
                           int seq_len, int batch, TtLayers* ly) {
    if (!(U > 0 && I > 0)) return fail_as(fn, NRK_EINVAL, "empty embedding tables");
    if (!(U <= INT32_MAX && I <= INT32_MAX)) return fail_as(fn, NRK_EINVAL, "more than 2^31 - 1 table rows");
    if (!(seq_len >= 1 && seq_len <= TR_MAXT)) return fail_as(fn, NRK_EINVAL, "seq_len must be in [1, 64]");
    if (!(batch >= 1 && batch <= TR_MAXB)) return fail_as(fn, NRK_EINVAL, "batch must be in [1, 8192]");
    return tt_check_shape(fn, dim, n_layers, widths, ly);
}

}  // namespace nrk

using namespace nrk;

extern "C" {

size_t nrk_tt_train_workspace_bytes(int64_t n_user_rows, int64_t n_item_rows, int dim, int n_layers,
                                    const int* widths, int seq_len, int batch) {
    clear_error();
    TtLayers ly{};
    if (tr_check_shapes(__func__, n_user_rows, n_item_rows, dim, n_layers, widths, seq_len, batch, &ly) != NRK_OK)
        return 0;
    return tr_layout(nullptr, n_user_rows, n_item_rows, dim, ly, seq_len, batch).bytes;
}

int nrk_tt_train_grad(const float* user_table, int64_t n_user_rows, const float* item_table,
                      int64_t n_item_rows, int dim, const float* weights, int n_layers, const int* widths,
                      const int64_t* log_off, const int32_t* log_items, const int32_t* s_user,
                      const int32_t* s_pos, const int32_t* s_target, const float* s_label, int batch,
                      int seq_len, float p, uint64_t seed, int64_t step, float* loss, float* w_grad,
                      int32_t* u_rows, float* u_vals, int32_t* u_count, int32_t* i_rows, float* i_vals,
                      int32_t* i_count, void* workspace, size_t workspace_bytes, nrk_stream_t stream) {
    clear_error();
    TtLayers ly{};
    const int rc = tr_check_shapes(__func__, n_user_rows, n_item_rows, dim, n_layers, widths, seq_len, batch, &ly);
    if (rc != NRK_OK) return rc;
    NRK_REQUIRE(p >= 0.0f && p < 1.0f, "dropout p must be in [0, 1)");
    NRK_REQUIRE(step >= 0, "step must be >= 0");
    NRK_REQUIRE(user_table && item_table && weights && log_off && log_items && s_user && s_pos && s_target &&
                    s_label && loss && w_grad && u_rows && u_vals && u_count && i_rows && i_vals && i_count &&
                    workspace,
                "null pointer");
    const int D = dim, T = seq_len, B = batch;
    TrWs w = tr_layout(workspace, n_user_rows, n_item_rows, D, ly, T, B);
    NRK_REQUIRE(workspace_bytes >= w.bytes, "workspace too small (nrk_tt_train_workspace_bytes)");
    hipStream_t s = as_stream(stream);
    int n_w = 0, in = 2 * D, staged_floats = 0;
    for (int l = 0; l < ly.n; ++l) {
        n_w += ly.w[l] * (in + 1);
        staged_floats += ly.w[l] * (in + 2);
        in = ly.w[l];
    }
    // the weights ride in LDS when they fit beside the four waves' rows
    const size_t wave_floats = (size_t)4 * (w.asz + 2 * TT_MAXW);
    const int staged = (wave_floats + staged_floats) * sizeof(float) <= 60 * 1024;
    const size_t lds = sizeof(float) * (wave_floats + (staged ? staged_floats : 0));
    const uint32_t thr = p > 0.0f ? std::max<uint32_t>(1u, tr_threshold(p)) : 0u;
    const float scale = p > 0.0f ? 1.0f / (1.0f - p) : 1.0f;
    const int grid = (B + 3) / 4;
    tt_for_dim(D, [&](auto dc) {
        tt_train_fb_kernel<decltype(dc)::value><<<grid, 256, lds, s>>>(
            user_table, item_table, weights, ly, log_off, log_items, s_user, s_pos, s_target, s_label, B, T, scale, thr,
            seed, (uint64_t)step, w.asz, w.dsz, staged, w.loss_b, w.act, w.delta, w.gU, w.gH, w.gT);
    });
    NRK_CHECK_LAUNCH();
    tt_wgrad_kernel<<<(n_w + 63) / 64 + 1, 1024, 0, s>>>(w.act, w.delta, w.loss_b, ly, D, B, w.asz, w.dsz, n_w,
                                                        w_grad, loss);
    NRK_CHECK_LAUNCH();
    const bool one = w.n_chunks == 1;
    TrTable tu{one ? u_rows : w.crow_u, one ? u_vals : w.cval_u, one ? u_count : w.ccnt_u, w.CS};
    TrTable ti{one ? i_rows : w.crow_i, one ? i_vals : w.cval_i, one ? i_count : w.ccnt_i, w.cap_i};
    if (!one) NRK_FILL(__func__, w.mark_u, 0, w.mark_bytes, s);
    tt_emb_sort_kernel<<<dim3(w.n_chunks, 2), 1024, (size_t)TR_KEYS * 6, s>>>(
        log_off, log_items, s_user, s_pos, s_target, B, T, w.CS, D, w.gU, w.gH, w.gT, tu, ti);
    NRK_CHECK_LAUNCH();
    if (!one) {
        tt_emb_mark_kernel<<<dim3(w.n_chunks, 2), 256, 0, s>>>(tu, ti, w.mark_u, w.mark_i);
        NRK_CHECK_LAUNCH();
        const dim3 cg((unsigned)((std::max(n_user_rows, n_item_rows) + TR_CT - 1) / TR_CT), 2);
        tt_emb_count_kernel<<<cg, 1024, 0, s>>>(w.mark_u, n_user_rows, w.mark_i, n_item_rows, w.blk_u, w.blk_i);
        NRK_CHECK_LAUNCH();
        tt_emb_compact_kernel<<<cg, 1024, 0, s>>>(w.mark_u, n_user_rows, w.mark_i, n_item_rows, w.blk_u, w.blk_i,
                                                  u_rows, u_count, i_rows, i_count);
        NRK_CHECK_LAUNCH();
        const int64_t most = (int64_t)B * (T + 1) * D;
        const unsigned mg = grid_for(most, 256, 4096);
        tt_emb_merge_kernel<<<dim3(mg, 2), 256, 0, s>>>(tu, ti, w.n_chunks, D, u_rows, u_count, u_vals, i_rows,
                                                        i_count, i_vals);
        NRK_CHECK_LAUNCH();
    }
    return NRK_OK;
}

int nrk_tt_dropout_mask(uint64_t seed, int64_t step, int layer, int batch, int width, float p, float* out,
                        nrk_stream_t stream) {
    clear_error();
    NRK_REQUIRE(batch >= 1 && batch <= TR_MAXB, "batch must be in [1, 8192]");
    NRK_REQUIRE(width >= 1 && width <= TT_MAXW, "width must be in [1, 256]");
    NRK_REQUIRE(layer >= 0 && layer < TT_MAXL, "layer must be in [0, 8)");
    NRK_REQUIRE(p >= 0.0f && p < 1.0f, "dropout p must be in [0, 1)");
    NRK_REQUIRE(step >= 0, "step must be >= 0");
    NRK_REQUIRE(out, "null pointer");
    const uint32_t thr = p > 0.0f ? std::max<uint32_t>(1u, tr_threshold(p)) : 0u;
    const int64_t n = (int64_t)batch * width;
    tt_dropout_mask_kernel<<<grid_for(n, 256, 2048), 256, 0, as_stream(stream)>>>(
        seed, (uint64_t)step, layer, batch, width, thr, out);
    NRK_CHECK_LAUNCH();
    return NRK_OK;
}

int nrk_tt_adam_step(float* weights, float* w_m, float* w_v, const float* w_grad, int64_t n_weights,
                     float* user_table, float* u_m, float* u_v, int64_t n_user_rows, const int32_t* u_rows,
                     const float* u_vals, const int32_t* u_count, float* item_table, float* i_m, float* i_v,
                     int64_t n_item_rows, const int32_t* i_rows, const float* i_vals, const int32_t* i_count,
                     int dim, double lr, double beta1, double beta2, double eps, int64_t t,
                     nrk_stream_t stream) {
    clear_error();
    if (const int rc = tt_check_shape(__func__, dim)) return rc;
    NRK_REQUIRE(n_weights > 0 && n_weights < ((int64_t)1 << 31), "bad n_weights");
    NRK_REQUIRE(n_user_rows > 0 && n_item_rows > 0 && n_user_rows <= INT32_MAX && n_item_rows <= INT32_MAX,
                "bad table sizes");
    AdamK k;
    if (const int rc = adam_scalars(__func__, lr, beta1, beta2, eps, t, &k)) return rc;
    NRK_REQUIRE(weights && w_m && w_v && w_grad && user_table && u_m && u_v && u_rows && u_vals && u_count &&
                    item_table && i_m && i_v && i_rows && i_vals && i_count,
                "null pointer");
    const AdamSegs<2> segs{{{user_table, u_m, u_v, u_rows, u_vals, u_count, n_user_rows},
                            {item_table, i_m, i_v, i_rows, i_vals, i_count, n_item_rows}}};
    const char* fn = __func__;  // inside the lambda it would name operator()
    return tt_for_dim(dim, [&](auto dc) {
        return adam_sweep<decltype(dc)::value>(fn, weights, w_m, w_v, w_grad, n_weights, segs, k, as_stream(stream));
    });
}

int nrk_tt_make_samples_count(const int64_t* log_off, int64_t n_users, int64_t* pos_off, nrk_stream_t stream) {
    clear_error();
    NRK_REQUIRE(n_users > 0 && n_users <= INT32_MAX, "bad n_users");
    NRK_REQUIRE(log_off && pos_off, "null pointer");
    tt_sample_count_kernel<<<1, 1024, 0, as_stream(stream)>>>(log_off, n_users, pos_off);
    NRK_CHECK_LAUNCH();
    return NRK_OK;
}

int nrk_tt_make_samples(const int64_t* log_off, const int32_t* log_items, int64_t n_users,
                        const int64_t* pos_off, int64_t n_pos, int negsample, const int32_t* pool,
                        int64_t n_pool, uint64_t seed, int32_t* s_user, int32_t* s_pos, int32_t* s_target,
                        float* s_label, nrk_stream_t stream) {
    clear_error();
    NRK_REQUIRE(n_users > 0 && n_users <= INT32_MAX, "bad n_users");
    NRK_REQUIRE(n_pos >= 0 && negsample >= 0 && negsample <= 1024, "bad sizes (negsample must be in [0, 1024])");
    NRK_REQUIRE(negsample == 0 || (n_pool > 0 && n_pool <= INT32_MAX), "negatives need a non-empty pool");
    if (n_pos == 0) return NRK_OK;
    NRK_REQUIRE(log_off && log_items && pos_off && s_user && s_pos && s_target && s_label && (negsample == 0 || pool),
                "null pointer");
    const int64_t n = n_pos * (1 + negsample);
    tt_make_samples_kernel<<<grid_for(n, 256, 8192), 256, 0, as_stream(stream)>>>(
        log_off, log_items, n_users, pos_off, n_pos, negsample, pool, n_pool, seed, s_user, s_pos, s_target, s_label);
    NRK_CHECK_LAUNCH();
    return NRK_OK;
}

}  // extern "C"
