// din_train.hip -- one DIN training step on gfx950: DINModel.forward in
// train mode (src/rank/DIN.py:214-286), mean BCELoss, the whole backward, a
// bitwise-reproducible reduction of the embedding gradients and a
// dense-semantics Adam sweep (DINRanker.train's loop body, DIN.py:907-912).
// Everything stored is fp32 and nothing is shared with the inference forward
// (din.hip: no split-fp16 products here).  Long sums are blocked: a block's
// products are added in fp32, the blocks, the batch / history / contribution
// sums and the Dice statistics in fp64, rounded once.
//
// A Dice layer normalises with the statistics of the batch, and they carry
// gradient, so both directions split into phases at every Dice:
//   forward   dt_att_fwd      z[b,t,h] = W [k, q, q-k, q*k] + b in the folded
//                             form (W_k - W_d) k + (W_q + W_d) q + W_p (q*k):
//                             per sample W_eff = (W_k - W_d) + W_p q in LDS
//             dt_colstat      mean and unbiased std of every (t,h) column
//             dt_att_out      Dice, Linear(36 -> 1), mask, sum_t w k, and the
//                             MLP input row [user | ctx | candidate | history]
//             per hidden layer dt_gemm, then dt_colstat / dt_dice_fwd (Dice)
//             or dt_prelu_fwd (PReLU); the last layer's activation is
//             dt_head's (loss)
//   backward  per hidden layer, last first: dt_dice_sums + dt_dice_bwd (Dice)
//             or dt_prelu_bwd + dt_slope_final (PReLU), dt_gemm for dW / dA
//             dt_att_ds       d score[b,t]
//             dt_dice_sums    the two column sums of the attention Dice
//             dt_att_bwd      d z (in place), d k, d q, and per block the
//                             partial sums of dz^T k and dz^T (q*k)
//             dt_att_final    partials in block order -> d att_w0
//   tables    dt_emb_keys, a stable radix sort of (row, contribution) pairs
//             (rocprim), dt_emb_heads/starts, dt_emb_piece, dt_emb_long: every
//             destination row is the sum of its contributions in ascending
//             contribution order, pieces of 512 first, then the pieces in
//             order, so a pad row with 10^5 terms is a 512-term chain and a
//             chain over its ~200 pieces, never one thread over all of them.
// A masked position contributes nothing through w * mask but does through
// the mean and std of its (t,h) columns; no kernel skips it.
// Every sum has a fixed order and no output is written by a floating-point
// atomic: the same call twice gives the same bits.
//
// The matrix products run on the vector ALUs in 64 x 64 LDS tiles
// (dt_gemm_kernel), not yet on v_mfma_f32_32x32x2_f32.
//
// Out of contract: a Dice column whose batch std is exactly 0 (torch's own
// gradient is NaN there; the std term is dropped here), and |logit| so large
// that p (1 - p) underflows in BCELoss (|x| >~ 15).  Loss and gradients stay
// finite in both cases; parity with torch is not claimed.
//
// The final MLP has 1 to 4 hidden layers, all Dice or all nn.PReLU() (one
// trained slope per layer, torch's convention at the kink: y = x > 0 ? x : a x,
// dx = x > 0 ? g : a g, da = sum (x > 0 ? 0 : x g)).  A PReLU layer has no batch
// statistics and launches none of the Dice passes; the attention unit is Dice
// under either activation (DIN.py:188).
//
// The Adam sweep is train_common.h's, with one table.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "din_common.h"
#include "train_common.h"

namespace nrk {

constexpr int DT_MAXT = 128, DT_MAXB = 8192, DT_MAXH = 1024, DT_MAXF = 64;
constexpr int DT_PIECE = 512;  // contributions one 32-lane group sums in a chain
constexpr int DT_CB = 8;       // samples per dt_att_bwd block
constexpr double DT_EPS = 1e-8;

struct DtIdx {
    const float* table;
    const int64_t* row_base;
    const int32_t *user, *item, *hist, *ctx;
    const float* mask;
    int Fu, Fc, B, T;
};

// Dice (DIN.py:39-44): p = sigmoid((x - mean) / (std + eps)), y = p x + (1 - p) 0.01 x.
// The statistics, p and the backward's combination are formed in fp64: with a
// small batch the three terms of the backward cancel (at B = 2 the normalised
// value does not depend on x at all), and fp32 statistics would leave their
// own rounding, multiplied by dz / std, in the result.
__device__ __forceinline__ double dt_dice_p(float x, double mu, double sd) {
    return 1.0 / (1.0 + exp(-((double)x - mu) / (sd + DT_EPS)));
}
__device__ __forceinline__ float dt_dice(float x, double mu, double sd) {
    const double p = dt_dice_p(x, mu, sd);
    return (float)(p * x + (1.0 - p) * 0.01 * x);
}

// d x of one Dice element given the upstream g and its column's two sums
// (s1 = sum_b dz / (std + eps), s2 = sum_b dz (x - mean) / (std + eps)^2)
__device__ __forceinline__ float dt_dice_dx(float x, double mu, double sd, float g, double s1, double s2, int B) {
    const double den = sd + DT_EPS, xc = (double)x - mu;
    const double p = dt_dice_p(x, mu, sd);
    const double dz = 0.99 * g * x * (p * (1.0 - p));
    const double direct = g * (p + 0.01 * (1.0 - p));
    const double via_sd = sd > 0.0 ? s2 * xc / ((double)(B - 1) * sd) : 0.0;
    return (float)(direct + dz / den - s1 / (double)B - via_sd);
}

// ------------------------------------------------------------ tiled GEMM --
// C[m, n] = sum_k A(m, k) Bm(k, n) (+ bias[n]), A(m, k) = A[m sam + k sak],
// Bm(k, n) = Bm[k sbk + n sbn]; k ascending.  gridDim.z > 1 splits k into
// slices of kper whose results go to part[z][M][N] (dt_sum_parts adds them in
// slice order).
struct DtGemm {
    const float *A, *Bm, *bias;
    float* C;
    double* part;
    int64_t sam, sak, sbk, sbn;
    int M, N, K, ldc, kper;
};

__global__ __launch_bounds__(256) void dt_gemm_kernel(DtGemm g) {
    __shared__ float As[16][68], Bs[16][68];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int k0 = blockIdx.z * g.kper, k1 = min(g.K, k0 + g.kper);
    // a tile's 16 products are added in fp32, the tiles in fp64: the error of a
    // long k stays that of a blocked sum, not of one fp32 chain
    double acc[4][4] = {};
    for (int kb = k0; kb < k1; kb += 16) {
        for (int i = tid; i < 1024; i += 256) {
            int mm, kk;
            if (g.sak == 1) {
                kk = i & 15;
                mm = i >> 4;
            } else {
                mm = i & 63;
                kk = i >> 6;
            }
            const int m = m0 + mm, k = kb + kk;
            As[kk][mm] = (m < g.M && k < k1) ? g.A[m * g.sam + k * g.sak] : 0.0f;
        }
        for (int i = tid; i < 1024; i += 256) {
            int nn, kk;
            if (g.sbk == 1) {
                kk = i & 15;
                nn = i >> 4;
            } else {
                nn = i & 63;
                kk = i >> 6;
            }
            const int n = n0 + nn, k = kb + kk;
            Bs[kk][nn] = (n < g.N && k < k1) ? g.Bm[k * g.sbk + n * g.sbn] : 0.0f;
        }
        __syncthreads();
        float tile[4][4] = {};
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = As[kk][ty * 4 + i];
                b[i] = Bs[kk][tx * 4 + i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) tile[i][j] = fmaf(a[i], b[j], tile[i][j]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] += (double)tile[i][j];
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = m0 + ty * 4 + i, n = n0 + tx * 4 + j;
            if (m < g.M && n < g.N) {
                if (gridDim.z == 1) g.C[(int64_t)m * g.ldc + n] = (float)(acc[i][j] + (g.bias ? (double)g.bias[n] : 0.0));
                else g.part[((int64_t)blockIdx.z * g.M + m) * g.N + n] = acc[i][j];
            }
        }
    }
}

__global__ __launch_bounds__(256) void dt_sum_parts_kernel(const double* __restrict__ part, int S, int M, int N,
                                                           int ldc, float* __restrict__ C) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M * N) return;
    double t = 0.0;
    for (int s = 0; s < S; ++s) t += part[(int64_t)s * M * N + i];
    C[(int64_t)(i / N) * ldc + i % N] = (float)t;
}

// ------------------------------------------------------- column reductions --
// Block = 16 columns x 64 row slices (rows ascending inside a slice), the 64
// partials added in slice order.
template <class F>
__device__ __forceinline__ F dt_col_combine(F (*part)[16], F s) {
    const int tid = threadIdx.x;
    __syncthreads();
    part[tid >> 4][tid & 15] = s;
    __syncthreads();
    F t = 0;
    for (int r = 0; r < 64; ++r) t += part[r][tid & 15];
    return t;  // every thread of a column holds the column's sum
}

// out[c] = sum_b x[b, c]
__global__ __launch_bounds__(1024) void dt_colsum_kernel(const float* __restrict__ x, int B, int C,
                                                         float* __restrict__ out) {
    __shared__ double part[64][16];
    const int tid = threadIdx.x, c = blockIdx.x * 16 + (tid & 15), r = tid >> 4;
    const int per = (B + 63) / 64, b0 = min(B, r * per), b1 = min(B, b0 + per);
    double s = 0.0;
    if (c < C)
        for (int b = b0; b < b1; ++b) s += (double)x[(int64_t)b * C + c];
    s = dt_col_combine(part, s);
    if (r == 0 && c < C) out[c] = (float)s;
}

// mean and unbiased std (torch.std) of every column of x [B, C], in fp64
__global__ __launch_bounds__(1024) void dt_colstat_kernel(const float* __restrict__ x, int B, int C,
                                                          double* __restrict__ mu, double* __restrict__ sd) {
    __shared__ double part[64][16];
    const int tid = threadIdx.x, c = blockIdx.x * 16 + (tid & 15), r = tid >> 4;
    const int per = (B + 63) / 64, b0 = min(B, r * per), b1 = min(B, b0 + per);
    double s = 0.0;
    if (c < C)
        for (int b = b0; b < b1; ++b) s += (double)x[(int64_t)b * C + c];
    const double m = dt_col_combine(part, s) / (double)B;
    s = 0.0;
    if (c < C)
        for (int b = b0; b < b1; ++b) {
            const double d = (double)x[(int64_t)b * C + c] - m;
            s += d * d;
        }
    s = dt_col_combine(part, s);
    if (r == 0 && c < C) {
        mu[c] = m;
        sd[c] = sqrt(s / (double)(B - 1));
    }
}

// The column sums of a Dice backward over x [B, C] with upstream
// g[b, c] = G[b gs + c / gdiv] * (w ? w[c % gdiv] : 1):
//   S[0][c] = sum_b dz / (std + eps), S[1][c] = sum_b dz (x - mean) / (std + eps)^2,
//   S[2][c] = sum_b G[b, c / gdiv] * dice(x)   (d of the weight w)
__global__ __launch_bounds__(1024) void dt_dice_sums_kernel(const float* __restrict__ x,
                                                            const double* __restrict__ mu,
                                                            const double* __restrict__ sd,
                                                            const float* __restrict__ G, int gs, int gdiv,
                                                            const float* __restrict__ w, int B, int C,
                                                            double* __restrict__ S) {
    __shared__ double part[64][16];
    const int tid = threadIdx.x, c = blockIdx.x * 16 + (tid & 15), r = tid >> 4;
    const int per = (B + 63) / 64, b0 = min(B, r * per), b1 = min(B, b0 + per);
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (c < C) {
        const double m = mu[c], sdc = sd[c], den = sdc + DT_EPS;
        const float wv = w ? w[c % gdiv] : 1.0f;
        const int gc = c / gdiv;
        for (int b = b0; b < b1; ++b) {
            const float xv = x[(int64_t)b * C + c], g0 = G[(int64_t)b * gs + gc], g = g0 * wv;
            const double xc = (double)xv - m, p = dt_dice_p(xv, m, sdc);
            const double dz = 0.99 * g * xv * (p * (1.0 - p));
            s1 += dz / den;
            s2 += dz * xc / (den * den);
            s3 += (double)g0 * (p * xv + (1.0 - p) * 0.01 * xv);
        }
    }
    s1 = dt_col_combine(part, s1);
    s2 = dt_col_combine(part, s2);
    s3 = dt_col_combine(part, s3);
    if (r == 0 && c < C) {
        S[c] = s1;
        S[C + c] = s2;
        S[2 * C + c] = s3;
    }
}

__global__ __launch_bounds__(256) void dt_dice_fwd_kernel(const float* __restrict__ x, const double* __restrict__ mu,
                                                          const double* __restrict__ sd, int64_t n, int C,
                                                          float* __restrict__ y) {
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        y[i] = dt_dice(x[i], mu[c], sd[c]);
    }
}

// g [B, C] (d of the Dice output) -> d of the Dice input, in place
__global__ __launch_bounds__(256) void dt_dice_bwd_kernel(const float* __restrict__ x, const double* __restrict__ mu,
                                                          const double* __restrict__ sd, const double* __restrict__ S,
                                                          int B, int C, float* __restrict__ g) {
    const int64_t n = (int64_t)B * C;
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        g[i] = dt_dice_dx(x[i], mu[c], sd[c], g[i], S[c], S[C + c], B);
    }
}

// ------------------------------------------------------------------ PReLU --
// nn.PReLU() with its one slope, torch's convention at the kink (x = 0 takes
// the slope's side in the forward and in both gradients).
__device__ __forceinline__ float dt_prelu(float x, float a) { return x > 0.0f ? x : a * x; }

__global__ __launch_bounds__(256) void dt_prelu_fwd_kernel(const float* __restrict__ x,
                                                           const float* __restrict__ slope, int64_t n,
                                                           float* __restrict__ y) {
    const float a = slope[0];
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        y[i] = dt_prelu(x[i], a);
}

constexpr int DT_SLOPE_BLOCKS = 256;  // blocks of dt_prelu_bwd: the partials dt_slope_final adds in order

// g [n] (d of the PReLU output) -> d of its input, in place, and the block's
// part of d slope = sum (x > 0 ? 0 : x g): a thread's elements ascending in
// fp64, the wave tree, the four waves in order.
__global__ __launch_bounds__(256) void dt_prelu_bwd_kernel(const float* __restrict__ x,
                                                           const float* __restrict__ slope, int64_t n,
                                                           float* __restrict__ g, double* __restrict__ part) {
    __shared__ double wp[4];
    const float a = slope[0];
    double s = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float xv = x[i], gv = g[i];
        if (!(xv > 0.0f)) {
            s += (double)xv * (double)gv;
            g[i] = a * gv;
        }
    }
    s = wave_sum_f64(s);
    if ((threadIdx.x & 63) == 0) wp[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((wp[0] + wp[1]) + wp[2]) + wp[3];
}

// d slope: the block partials in block order, rounded once
__global__ void dt_slope_final_kernel(const double* __restrict__ part, int nblk, float* __restrict__ g_slope) {
    if (threadIdx.x || blockIdx.x) return;
    double t = 0.0;
    for (int k = 0; k < nblk; ++k) t += part[k];
    g_slope[0] = (float)t;
}

// ------------------------------------------------------------------- head --
// One wave per sample over the last hidden layer: a = act(z) (ACT: Dice with
// the column statistics, or PReLU with the layer's slope), logit = w . a + b,
// p = sigmoid, BCELoss (log clamped at -100) and its gradient as torch forms
// it: (p - y) / max((1 - p) p, 1e-12) / B, then sigmoid's (1 - p) p.
// hb[b] = [g a | g] (column sums: d w, d b), da[b] = g w.
template <int ACT>
__global__ __launch_bounds__(256) void dt_head_kernel(const float* __restrict__ z, const double* __restrict__ mu,
                                                      const double* __restrict__ sd, const float* __restrict__ slope,
                                                      const float* __restrict__ w, const float* __restrict__ bo,
                                                      const float* __restrict__ label, int B, int H,
                                                      float* __restrict__ loss_b, float* __restrict__ hb,
                                                      float* __restrict__ da) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const float sl = ACT == DIN_ACT_PRELU ? slope[0] : 0.0f;
    auto act = [&](int c) {
        const float x = z[(int64_t)b * H + c];
        if constexpr (ACT == DIN_ACT_PRELU) return dt_prelu(x, sl);
        else return dt_dice(x, mu[c], sd[c]);
    };
    double s = 0.0;
    for (int c = lane; c < H; c += WAVE) s += (double)w[c] * (double)act(c);
    const float logit = (float)(wave_sum_f64(s) + (double)bo[0]);
    const float p = 1.0f / (1.0f + expf(-logit)), y = label[b];
    if (lane == 0) loss_b[b] = -(y * fmaxf(logf(p), -100.0f) + (1.0f - y) * fmaxf(log1pf(-p), -100.0f));
    const float gi = (1.0f / (float)B) * (p - y) / fmaxf((1.0f - p) * p, 1e-12f);
    const float g = gi * (1.0f - p) * p;
    for (int c = lane; c < H; c += WAVE) {
        hb[(int64_t)b * (H + 1) + c] = g * act(c);
        da[(int64_t)b * H + c] = g * w[c];
    }
    if (lane == 0) hb[(int64_t)b * (H + 1) + H] = g;
}

// mean of the per-sample losses: 16 slices, fixed tree (as tt_wgrad_kernel)
__global__ __launch_bounds__(1024) void dt_loss_kernel(const float* __restrict__ loss_b, int B,
                                                       float* __restrict__ loss) {
    __shared__ double part[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per = (B + 15) / 16, b0 = min(B, wave * per), b1 = min(B, b0 + per);
    double s = 0.0;
    for (int b = b0 + lane; b < b1; b += WAVE) s += (double)loss_b[b];
    s = wave_sum_f64(s);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < 16; ++k) t += part[k];
        *loss = (float)(t / (double)B);
    }
}

// -------------------------------------------------------------- attention --
// Per-sample staging shared by the attention kernels: the candidate row q,
// the absolute table rows of the history, and W_eff = (W_k - W_d) + W_p q
// (row stride Di + 1: lanes of different h fall into different banks).
template <int NI>
__device__ __forceinline__ void dt_stage_sample(const DtIdx& ix, int b, float* q, int* hrow) {
    constexpr int Di = NI * 32;
    for (int d = threadIdx.x; d < Di; d += 256) {
        const int f = d >> 5;
        q[d] = ix.table[(ix.row_base[ix.Fu + f] + ix.item[(int64_t)b * NI + f]) * 32 + (d & 31)];
    }
    for (int i = threadIdx.x; i < ix.T * NI; i += 256)
        hrow[i] = (int)(ix.row_base[ix.Fu + i % NI] + ix.hist[(int64_t)b * ix.T * NI + i]);
}
template <int NI>
__device__ __forceinline__ void dt_build_weff(const float* __restrict__ W, const float* q, float* weff) {
    constexpr int Di = NI * 32, WS = Di + 1;
    for (int i = threadIdx.x; i < 36 * Di; i += 256) {
        const int h = i / Di, d = i % Di;
        const float* w = W + (size_t)h * 4 * Di;
        weff[h * WS + d] = fmaf(w[3 * Di + d], q[d], w[d] - w[2 * Di + d]);
    }
}
template <int NI>
__device__ __forceinline__ float dt_k(const DtIdx& ix, const int* hrow, int t, int d) {
    return ix.table[(int64_t)hrow[t * NI + (d >> 5)] * 32 + (d & 31)];
}

template <int NI>
__global__ __launch_bounds__(256) void dt_att_fwd_kernel(DtIdx ix, const float* __restrict__ W,
                                                         const float* __restrict__ b0, float* __restrict__ z) {
    constexpr int Di = NI * 32, WS = Di + 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* weff = lds;
    float* q = weff + 36 * WS;
    float* c = q + Di;
    int* hrow = reinterpret_cast<int*>(c + 36);
    const int b = blockIdx.x, T = ix.T;
    dt_stage_sample<NI>(ix, b, q, hrow);
    __syncthreads();
    dt_build_weff<NI>(W, q, weff);
    if (threadIdx.x < 36) {
        const float* w = W + (size_t)threadIdx.x * 4 * Di;
        double acc = b0[threadIdx.x];
        for (int d = 0; d < Di; ++d) acc += (double)(w[Di + d] + w[2 * Di + d]) * (double)q[d];
        c[threadIdx.x] = (float)acc;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < T * 36; o += 256) {
        const int t = o / 36, h = o % 36;
        double acc = c[h];  // a feature's 32 products in fp32, the features in fp64
        for (int f = 0; f < NI; ++f) {
            const float4* kr = reinterpret_cast<const float4*>(ix.table + (int64_t)hrow[t * NI + f] * 32);
            const float* wr = weff + h * WS + f * 32;
            float part = 0.0f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float4 kv = kr[e];
                part = fmaf(wr[4 * e], kv.x, part);
                part = fmaf(wr[4 * e + 1], kv.y, part);
                part = fmaf(wr[4 * e + 2], kv.z, part);
                part = fmaf(wr[4 * e + 3], kv.w, part);
            }
            acc += (double)part;
        }
        z[((int64_t)b * T) * 36 + o] = (float)acc;
    }
}

// Dice, Linear(36 -> 1), mask, the weighted history and the MLP input row
template <int NI>
__global__ __launch_bounds__(256) void dt_att_out_kernel(DtIdx ix, const float* __restrict__ z,
                                                         const double* __restrict__ mu, const double* __restrict__ sd,
                                                         const float* __restrict__ w1, const float* __restrict__ b1,
                                                         int IN, float* __restrict__ wbuf, float* __restrict__ x0) {
    constexpr int Di = NI * 32;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* y = lds;                // [T][36]
    float* s = y + ix.T * 36;      // [T]
    float* q = s + ix.T;           // [Di]
    int* hrow = reinterpret_cast<int*>(q + Di);
    const int b = blockIdx.x, T = ix.T, Fu = ix.Fu, Fc = ix.Fc;
    dt_stage_sample<NI>(ix, b, q, hrow);
    for (int o = threadIdx.x; o < T * 36; o += 256) y[o] = dt_dice(z[(int64_t)b * T * 36 + o], mu[o], sd[o]);
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += 256) {
        double a = b1[0];
        for (int h = 0; h < 36; ++h) a += (double)w1[h] * (double)y[t * 36 + h];
        const float acc = (float)a * ix.mask[(int64_t)b * T + t];
        s[t] = acc;
        wbuf[(int64_t)b * T + t] = acc;
    }
    __syncthreads();
    float* xr = x0 + (int64_t)b * IN;
    for (int i = threadIdx.x; i < (Fu + Fc) * 32; i += 256) {
        const int f = i >> 5;
        const int64_t row = f < Fu ? ix.row_base[f] + ix.user[(int64_t)b * Fu + f]
                                   : ix.row_base[NI + f] + ix.ctx[(int64_t)b * Fc + (f - Fu)];
        xr[i] = ix.table[row * 32 + (i & 31)];
    }
    for (int d = threadIdx.x; d < Di; d += 256) {
        xr[(Fu + Fc) * 32 + d] = q[d];
        double acc = 0.0;
        for (int t = 0; t < T; ++t) acc += (double)s[t] * (double)dt_k<NI>(ix, hrow, t, d);
        xr[(Fu + Fc) * 32 + Di + d] = (float)acc;
    }
}

// d score[b, t] = mask * sum_d d wh[d] k[t, d]
template <int NI>
__global__ __launch_bounds__(256) void dt_att_ds_kernel(DtIdx ix, const float* __restrict__ dx0, int IN,
                                                        float* __restrict__ ds) {
    constexpr int Di = NI * 32;
    __shared__ float dwh[Di];
    __shared__ int hrow[DT_MAXT * NI];
    const int b = blockIdx.x, T = ix.T;
    for (int d = threadIdx.x; d < Di; d += 256) dwh[d] = dx0[(int64_t)b * IN + (ix.Fu + ix.Fc) * 32 + Di + d];
    for (int i = threadIdx.x; i < T * NI; i += 256)
        hrow[i] = (int)(ix.row_base[ix.Fu + i % NI] + ix.hist[(int64_t)b * T * NI + i]);
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += 256) {
        double acc = 0.0;
        for (int d = 0; d < Di; ++d) acc += (double)dwh[d] * (double)dt_k<NI>(ix, hrow, t, d);
        ds[(int64_t)b * T + t] = (float)acc * ix.mask[(int64_t)b * T + t];
    }
}

// DT_CB samples per block.  Per sample: d z[t,h] (written over z), A[h] =
// sum_t dz, d k[t,d] = sum_h dz W_eff + w[t] d wh[d], U[h,d] = sum_t dz k,
// d q[d] = sum_h A (W_q + W_d) + sum_h W_p U, added to the candidate part of
// dx0.  Over the block's samples (ascending): sum U and sum q U in registers,
// stored as gpart[block][2][36][Di].
template <int NI>
__global__ __launch_bounds__(256) void dt_att_bwd_kernel(DtIdx ix, const float* __restrict__ W,
                                                         const float* __restrict__ w1, const double* __restrict__ mu,
                                                         const double* __restrict__ sd, const double* __restrict__ S,
                                                         const float* __restrict__ ds, const float* __restrict__ wbuf,
                                                         int IN, float* __restrict__ z, float* __restrict__ dx0,
                                                         float* __restrict__ dk, float* __restrict__ Abuf,
                                                         double* __restrict__ gpart) {
    constexpr int Di = NI * 32, WS = Di + 1, HG = 256 / Di, HPG = (36 + HG - 1) / HG;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* weff = lds;                 // [36][WS]
    float* q = weff + 36 * WS;         // [Di]
    float* dwh = q + Di;               // [Di]
    float* uq = dwh + Di;              // [HG][Di] = 256
    float* As = uq + 256;              // [36] (+4 pad)
    float* wrow = As + 40;             // [T]
    float* dzp = wrow + ix.T;          // [T][36]
    int* hrow = reinterpret_cast<int*>(dzp + ix.T * 36);
    const int T = ix.T, B = ix.B, C = T * 36, tid = threadIdx.x;
    const int d_own = tid % Di, hg = tid / Di, cand = (ix.Fu + ix.Fc) * 32;
    double gk[HPG], gp[HPG];
#pragma unroll
    for (int i = 0; i < HPG; ++i) gk[i] = gp[i] = 0.0;
    for (int b = blockIdx.x * DT_CB; b < min(B, (int)(blockIdx.x + 1) * DT_CB); ++b) {
        __syncthreads();  // the previous sample's LDS is no longer read
        dt_stage_sample<NI>(ix, b, q, hrow);
        for (int d = tid; d < Di; d += 256) dwh[d] = dx0[(int64_t)b * IN + cand + Di + d];
        for (int t = tid; t < T; t += 256) wrow[t] = wbuf[(int64_t)b * T + t];
        for (int o = tid; o < C; o += 256) {
            const int64_t zi = (int64_t)b * C + o;
            const float g = ds[(int64_t)b * T + o / 36] * w1[o % 36];
            const float v = dt_dice_dx(z[zi], mu[o], sd[o], g, S[o], S[C + o], B);
            dzp[o] = v;
            z[zi] = v;
        }
        __syncthreads();
        dt_build_weff<NI>(W, q, weff);
        if (tid < 36) {
            double a = 0.0;
            for (int t = 0; t < T; ++t) a += (double)dzp[t * 36 + tid];
            As[tid] = (float)a;
            Abuf[(int64_t)b * 36 + tid] = (float)a;
        }
        float U[HPG];
#pragma unroll
        for (int i = 0; i < HPG; ++i) U[i] = 0.0f;
        for (int t = 0; t < T; ++t) {
            const float kv = dt_k<NI>(ix, hrow, t, d_own);
#pragma unroll
            for (int i = 0; i < HPG; ++i) {
                const int h = hg * HPG + i;
                if (h < 36) U[i] = fmaf(dzp[t * 36 + h], kv, U[i]);
            }
        }
        {
            float part = 0.0f;
            const float qv = q[d_own];
#pragma unroll
            for (int i = 0; i < HPG; ++i) {
                const int h = hg * HPG + i;
                if (h < 36) {
                    gk[i] += (double)U[i];
                    gp[i] += (double)qv * (double)U[i];
                    part = fmaf(W[(size_t)h * 4 * Di + 3 * Di + d_own], U[i], part);
                }
            }
            uq[hg * Di + d_own] = part;
        }
        __syncthreads();  // weff, As, uq complete
        for (int o = tid; o < T * Di; o += 256) {
            const int t = o / Di, d = o % Di;
            float acc = 0.0f;
            for (int h = 0; h < 36; ++h) acc = fmaf(dzp[t * 36 + h], weff[h * WS + d], acc);
            dk[((int64_t)b * T) * Di + o] = fmaf(wrow[t], dwh[d], acc);
        }
        if (tid < Di) {
            double dq = 0.0;
            for (int h = 0; h < 36; ++h) {
                const float* w = W + (size_t)h * 4 * Di;
                dq += (double)As[h] * (double)(w[Di + tid] + w[2 * Di + tid]);
            }
            for (int g = 0; g < HG; ++g) dq += (double)uq[g * Di + tid];
            dx0[(int64_t)b * IN + cand + tid] = (float)((double)dx0[(int64_t)b * IN + cand + tid] + dq);
        }
    }
    double* gp_out = gpart + (size_t)blockIdx.x * 2 * 36 * Di;
#pragma unroll
    for (int i = 0; i < HPG; ++i) {
        const int h = hg * HPG + i;
        if (h < 36) {
            gp_out[h * Di + d_own] = gk[i];
            gp_out[36 * Di + h * Di + d_own] = gp[i];
        }
    }
}

// d att_w0 [36, 4 Di] = [G_k | G_q | G_q - G_k | G_p], the block partials in
// block order; d att_w1[h] = sum_t S3[t, h]; d att_b1 = sum_t dsT[t]
__global__ __launch_bounds__(256) void dt_att_final_kernel(const double* __restrict__ gpart, int nblk, int Di,
                                                           const float* __restrict__ Gq,
                                                           const double* __restrict__ S3, const float* __restrict__ dsT,
                                                           int T, float* __restrict__ g_w0, float* __restrict__ g_w1,
                                                           float* __restrict__ g_b1) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 36 * Di) {
        double gk = 0.0, gp = 0.0;
        for (int k = 0; k < nblk; ++k) {
            gk += gpart[(size_t)k * 2 * 36 * Di + i];
            gp += gpart[(size_t)k * 2 * 36 * Di + 36 * Di + i];
        }
        const int h = i / Di, d = i % Di;
        const double gq = Gq[i];
        float* o = g_w0 + (size_t)h * 4 * Di;
        o[d] = (float)gk;
        o[Di + d] = (float)gq;
        o[2 * Di + d] = (float)(gq - gk);
        o[3 * Di + d] = (float)gp;
    } else if (i < 36 * Di + 36) {
        const int h = i - 36 * Di;
        double s = 0.0;
        for (int t = 0; t < T; ++t) s += S3[t * 36 + h];
        g_w1[h] = (float)s;
    } else if (i == 36 * Di + 36) {
        double s = 0.0;
        for (int t = 0; t < T; ++t) s += (double)dsT[t];
        g_b1[0] = (float)s;
    }
}

// ------------------------------------------------------ embedding gradients --
// Contribution id = b * S + slot, slot over [user f | ctx f | candidate f |
// history (t, f)], S = Fu + Fc + NI + T NI: the first Fu + Fc + NI slots are
// 32-float pieces of dx0[b] in its own order, the rest of dk[b].
__global__ __launch_bounds__(256) void dt_emb_keys_kernel(DtIdx ix, int NI, int64_t n, uint32_t* __restrict__ keys,
                                                          int32_t* __restrict__ cid) {
    const int Fu = ix.Fu, Fc = ix.Fc, T = ix.T, S = Fu + Fc + NI + T * NI;
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / S;
        const int s = (int)(i % S);
        int64_t row;
        if (s < Fu) row = ix.row_base[s] + ix.user[b * Fu + s];
        else if (s < Fu + Fc) row = ix.row_base[NI + s] + ix.ctx[b * Fc + (s - Fu)];
        else if (s < Fu + Fc + NI) row = ix.row_base[Fu + (s - Fu - Fc)] + ix.item[b * NI + (s - Fu - Fc)];
        else {
            const int j = s - Fu - Fc - NI;
            row = ix.row_base[Fu + j % NI] + ix.hist[b * T * NI + j];
        }
        keys[i] = (uint32_t)row;
        cid[i] = (int32_t)i;
    }
}

__global__ __launch_bounds__(256) void dt_emb_heads_kernel(const uint32_t* __restrict__ keys, int64_t n,
                                                           int32_t* __restrict__ flag) {
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        flag[i] = i == 0 || keys[i] != keys[i - 1];
}

// seg = inclusive scan of flag: segment index + 1 of every sorted position
__global__ __launch_bounds__(256) void dt_emb_starts_kernel(const uint32_t* __restrict__ keys,
                                                            const int32_t* __restrict__ flag,
                                                            const int32_t* __restrict__ seg, int64_t n,
                                                            int32_t* __restrict__ starts, int32_t* __restrict__ rows,
                                                            int32_t* __restrict__ count) {
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (flag[i]) {
            starts[seg[i] - 1] = (int32_t)i;
            rows[seg[i] - 1] = (int32_t)keys[i];
        }
        if (i == n - 1) {
            starts[seg[i]] = (int32_t)n;
            *count = seg[i];
        }
    }
}

struct DtSrc {
    const float *dx0, *dk;
    int IN, S, head, T, NI;  // head = Fu + Fc + NI
};
__device__ __forceinline__ const float* dt_src(const DtSrc& s, int32_t cid) {
    const int b = cid / s.S, slot = cid % s.S;
    return slot < s.head ? s.dx0 + (int64_t)b * s.IN + slot * 32
                         : s.dk + ((int64_t)b * s.T * s.NI + (slot - s.head)) * 32;
}

// One 32-lane group per sorted position that starts a piece (every DT_PIECE-th
// position of its segment): the piece's sum in ascending contribution order.
// A segment of one piece is finished here; otherwise the piece goes to
// part[2 tile + (segment starts inside the tile)], tile = position / DT_PIECE
// (a tile holds at most one piece start of a segment that began before it and
// one of a longer-than-a-piece segment that begins in it).
__global__ __launch_bounds__(256) void dt_emb_piece_kernel(const int32_t* __restrict__ cid,
                                                           const int32_t* __restrict__ seg,
                                                           const int32_t* __restrict__ starts, int64_t n, DtSrc src,
                                                           float* __restrict__ vals, double* __restrict__ part) {
    const int d = threadIdx.x & 31;
    for (int64_t i = blockIdx.x * (int64_t)8 + (threadIdx.x >> 5); i < n; i += (int64_t)gridDim.x * 8) {
        const int s = seg[i] - 1, st = starts[s];
        if (((int)i - st) % DT_PIECE) continue;
        const int en = starts[s + 1], e = min(en, (int)i + DT_PIECE);
        double acc = 0.0;
#pragma unroll 8  // eight (id, value) load pairs in flight: the chain is latency otherwise
        for (int j = (int)i; j < e; ++j) acc += (double)dt_src(src, cid[j])[d];
        if (en - st <= DT_PIECE) {
            vals[(int64_t)s * 32 + d] = (float)acc;
        } else {
            const int tile = (int)i / DT_PIECE;
            part[((int64_t)2 * tile + (st >= tile * DT_PIECE ? 1 : 0)) * 32 + d] = acc;
        }
    }
}

__global__ __launch_bounds__(256) void dt_emb_long_kernel(const int32_t* __restrict__ starts,
                                                          const int32_t* __restrict__ count,
                                                          const double* __restrict__ part, float* __restrict__ vals) {
    const int d = threadIdx.x & 31, n = *count;
    for (int s = blockIdx.x * 8 + (threadIdx.x >> 5); s < n; s += gridDim.x * 8) {
        const int st = starts[s], en = starts[s + 1];
        if (en - st <= DT_PIECE) continue;
        double acc = 0.0;
        for (int i = st; i < en; i += DT_PIECE) {
            const int tile = i / DT_PIECE;
            acc += part[((int64_t)2 * tile + (st >= tile * DT_PIECE ? 1 : 0)) * 32 + d];
        }
        vals[(int64_t)s * 32 + d] = (float)acc;
    }
}

// ------------------------------------------------------------------- host --
// L hidden layers of widths H[0 .. L), layer n reading K(n) inputs; act: DIN_ACT_*
struct DtShape {
    int Fu, NI, Fc, L, H[DIN_MAX_LAYERS], act, B, T, Di, IN, S;
    int64_t R, N;
    int K(int n) const { return n ? H[n - 1] : IN; }
};

// packed weights: att_w0 [36, 4 Di] | att_b0 [36] | att_w1 [36] | att_b1 [1] |
// per hidden layer n: w[n] [H[n], K(n)] | b[n] [H[n]] | (PReLU: slope[n] [1]) |
// then w_out [H[L - 1]] | b_out [1]
struct DtOff {
    int64_t aw0, ab0, aw1, ab1, w[DIN_MAX_LAYERS], b[DIN_MAX_LAYERS], slope[DIN_MAX_LAYERS], w_out, b_out, n;
};
static DtOff dt_offsets(const DtShape& s) {
    DtOff o{};
    int64_t p = 0;
    auto take = [&](int64_t n) {
        const int64_t r = p;
        p += n;
        return r;
    };
    o.aw0 = take((int64_t)36 * 4 * s.Di);
    o.ab0 = take(36);
    o.aw1 = take(36);
    o.ab1 = take(1);
    for (int n = 0; n < s.L; ++n) {
        o.w[n] = take((int64_t)s.H[n] * s.K(n));
        o.b[n] = take(s.H[n]);
        if (s.act == DIN_ACT_PRELU) o.slope[n] = take(1);
    }
    o.w_out = take(s.H[s.L - 1]);
    o.b_out = take(1);
    o.n = p;
    return o;
}

// `dice_only`: nrk_din_train_grad's own refusal of any activation but Dice
static int dt_check(const char* fn, int64_t n_rows, int dim, int table_dtype, int n_user, int n_item, int n_ctx,
                    int n_layers, const int32_t* widths, int activation, bool dice_only, int64_t batch, int seq_len,
                    DtShape* s) {
    auto fail = [&](int rc, const char* msg) {
        set_error(std::string(fn) + ": " + msg);
        return rc;
    };
    if (dim != DIN_E) return fail(NRK_EUNSUPPORTED, "training is built for din_embedding_dim == 32");
    if (table_dtype != 0) return fail(NRK_EUNSUPPORTED, "training needs fp32 tables");
    if (dice_only && activation != 0) return fail(NRK_EUNSUPPORTED, "training implements the Dice activation only");
    if (activation != DIN_ACT_DICE && activation != DIN_ACT_PRELU)
        return fail(NRK_EINVAL, "activation must be 0 (dice) or 1 (prelu)");
    if (!(n_item == 1 || n_item == 2 || n_item == 4 || n_item == 8))
        return fail(NRK_EUNSUPPORTED, "n_item must be 1, 2, 4 or 8");
    if (n_user < 1 || n_user > DT_MAXF || n_ctx < 0 || n_ctx > DT_MAXF)
        return fail(NRK_EUNSUPPORTED, "n_user must be in [1, 64] and n_ctx in [0, 64]");
    if (n_layers < 1 || n_layers > DIN_MAX_LAYERS) return fail(NRK_EUNSUPPORTED, "n_layers must be in [1, 4]");
    if (!widths) return fail(NRK_EINVAL, "null pointer (widths)");
    for (int n = 0; n < n_layers; ++n)
        if (widths[n] < 1 || widths[n] > DT_MAXH)
            return fail(NRK_EUNSUPPORTED, dice_only ? "MLP hidden widths must be in [1, 1024]"
                                                    : "hidden widths must be in [1, 1024]");
    if (batch < 2 || batch > DT_MAXB)
        return fail(NRK_EUNSUPPORTED, "batch must be in [2, 8192] (Dice uses the batch std)");
    if (seq_len < 1 || seq_len > DT_MAXT) return fail(NRK_EUNSUPPORTED, "seq_len must be in [1, 128]");
    if (n_rows < 1 || n_rows > (int64_t)INT32_MAX / 32) return fail(NRK_EINVAL, "bad n_table_rows");
    s->Fu = n_user;
    s->NI = n_item;
    s->Fc = n_ctx;
    s->L = n_layers;
    for (int n = 0; n < n_layers; ++n) s->H[n] = widths[n];
    s->act = activation;
    s->B = (int)batch;
    s->T = seq_len;
    s->Di = n_item * 32;
    s->IN = 32 * (n_user + n_ctx + 2 * n_item);
    s->S = n_user + n_ctx + n_item + seq_len * n_item;
    s->R = n_rows;
    s->N = batch * s->S;
    return NRK_OK;
}

struct DtWs {
    float *z, *wbuf, *ds, *dsT, *Abuf, *Gq, *x0, *dx0, *hb, *loss_b, *dk;
    // per hidden layer: pre-activation, activation (not the last layer's: the head forms it), d activation
    float *zn[DIN_MAX_LAYERS], *an[DIN_MAX_LAYERS], *dan[DIN_MAX_LAYERS];
    double *gpart, *gemm_part, *epart, *spart;  // partial sums that a later kernel adds in order
    double *mu_a, *sd_a, *S_a;                  // Dice statistics and backward sums: the attention's,
    double *mu[DIN_MAX_LAYERS], *sd[DIN_MAX_LAYERS], *Sn[DIN_MAX_LAYERS];  // and a Dice layer's
    uint32_t *keys, *keys2;
    int32_t *cid, *cid2, *flag, *seg, *starts;
    void* sort_tmp;
    size_t sort_tmp_bytes, bytes;
    int nblk, ksplit;
};

// upper bound of rocprim's temporary storage for the sort and the scan over n
// pairs (queried exactly when a device is present, dt_sort_tmp_bytes)
static size_t dt_sort_tmp_bound(int64_t n) { return (size_t)n * 16 + ((size_t)8 << 20); }

static int dt_sort_bits(int64_t R) {
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < R) ++bits;
    return bits;
}

static DtWs dt_layout(void* base, const DtShape& s) {
    DtWs w{};
    Arena a(base);
    const size_t f = sizeof(float), B = s.B, C = (size_t)s.T * 36;
    w.nblk = (s.B + DT_CB - 1) / DT_CB;
    w.ksplit = std::max(1, std::min(16, s.B / 256));
    w.z = (float*)a.take(f * B * C);
    w.mu_a = (double*)a.take(8 * C);
    w.sd_a = (double*)a.take(8 * C);
    w.S_a = (double*)a.take(8 * 3 * C);
    w.wbuf = (float*)a.take(f * B * s.T);
    w.ds = (float*)a.take(f * B * s.T);
    w.dsT = (float*)a.take(f * s.T);
    w.Abuf = (float*)a.take(f * B * 36);
    w.Gq = (float*)a.take(f * 36 * s.Di);
    w.gpart = (double*)a.take(8 * (size_t)w.nblk * 2 * 36 * s.Di);
    w.x0 = (float*)a.take(f * B * s.IN);
    w.dx0 = (float*)a.take(f * B * s.IN);
    int maxH = 36, maxK = s.IN;  // gemm_part holds the split-K slices of the largest dW (and of Gq [36, Di])
    for (int n = 0; n < s.L; ++n) {
        const size_t H = s.H[n];
        maxH = std::max(maxH, s.H[n]);
        maxK = std::max(maxK, s.K(n));
        w.zn[n] = (float*)a.take(f * B * H);
        if (s.act == DIN_ACT_DICE) {
            w.mu[n] = (double*)a.take(8 * H);
            w.sd[n] = (double*)a.take(8 * H);
        }
        if (n < s.L - 1) w.an[n] = (float*)a.take(f * B * H);
        w.dan[n] = (float*)a.take(f * B * H);
        if (s.act == DIN_ACT_DICE) w.Sn[n] = (double*)a.take(8 * 3 * H);
    }
    if (s.act == DIN_ACT_PRELU) w.spart = (double*)a.take(8 * DT_SLOPE_BLOCKS);
    w.hb = (float*)a.take(f * B * (s.H[s.L - 1] + 1));
    w.loss_b = (float*)a.take(f * B);
    w.gemm_part = (double*)a.take(8 * (size_t)w.ksplit * maxH * maxK);
    w.dk = (float*)a.take(f * B * s.T * s.Di);
    w.epart = (double*)a.take(8 * 2 * 32 * (size_t)((s.N + DT_PIECE - 1) / DT_PIECE));
    w.keys = (uint32_t*)a.take(4 * (size_t)s.N);
    w.keys2 = (uint32_t*)a.take(4 * (size_t)s.N);
    w.cid = (int32_t*)a.take(4 * (size_t)s.N);
    w.cid2 = (int32_t*)a.take(4 * (size_t)s.N);
    w.flag = (int32_t*)a.take(4 * (size_t)s.N);
    w.seg = (int32_t*)a.take(4 * (size_t)s.N);
    w.starts = (int32_t*)a.take(4 * (size_t)(s.N + 1));
    w.sort_tmp_bytes = dt_sort_tmp_bound(s.N);
    w.sort_tmp = a.take(w.sort_tmp_bytes);
    w.bytes = a.bytes;
    return w;
}

static int dt_gemm(hipStream_t st, const float* A, int64_t sam, int64_t sak, const float* Bm, int64_t sbk, int64_t sbn,
                   const float* bias, float* C, int ldc, int M, int N, int K, int split, double* part) {
    DtGemm g{A, Bm, bias, C, part, sam, sak, sbk, sbn, M, N, K, ldc, 0};
    split = std::max(1, std::min(split, (K + 15) / 16));
    g.kper = ((K + split - 1) / split + 15) / 16 * 16;
    split = (K + g.kper - 1) / g.kper;
    dt_gemm_kernel<<<dim3((N + 63) / 64, (M + 63) / 64, split), 256, 0, st>>>(g);
    if (split > 1) dt_sum_parts_kernel<<<(M * N + 255) / 256, 256, 0, st>>>(part, split, M, N, ldc, C);
    return hipGetLastError() == hipSuccess ? NRK_OK : NRK_EHIP;
}

template <int NI>
static int dt_run(const DtShape& s, const DtWs& w, const DtIdx& ix, const float* wts, const float* labels, float* loss,
                  float* wg, int32_t* rows, float* vals, int32_t* count, hipStream_t st) {
    const DtOff o = dt_offsets(s);
    const int B = s.B, T = s.T, Di = s.Di, IN = s.IN, L = s.L, C = T * 36, WS = Di + 1;
    const bool dice = s.act == DIN_ACT_DICE;
    auto eg = [](int64_t n) { return grid_for(n, 256, 2048); };  // the grid-stride elementwise kernels
    // ---- forward
    const size_t lds_fwd = sizeof(float) * (36 * WS + Di + 36) + sizeof(int) * T * NI;
    dt_att_fwd_kernel<NI><<<B, 256, lds_fwd, st>>>(ix, wts + o.aw0, wts + o.ab0, w.z);
    dt_colstat_kernel<<<(C + 15) / 16, 1024, 0, st>>>(w.z, B, C, w.mu_a, w.sd_a);
    const size_t lds_out = sizeof(float) * (T * 36 + T + Di) + sizeof(int) * T * NI;
    dt_att_out_kernel<NI><<<B, 256, lds_out, st>>>(ix, w.z, w.mu_a, w.sd_a, wts + o.aw1, wts + o.ab1, IN, w.wbuf, w.x0);
    NRK_CHECK_LAUNCH();
    // hidden layer n: z_n = a_{n-1} W_n^T + b_n (a_{-1} = x0), the Dice statistics of its columns,
    // a_n = act(z_n); the last layer's activation belongs to the head
    for (int n = 0; n < L; ++n) {
        const int H = s.H[n], K = s.K(n);
        const int64_t BH = (int64_t)B * H;
        const float* in = n ? w.an[n - 1] : w.x0;
        if (dt_gemm(st, in, K, 1, wts + o.w[n], 1, K, wts + o.b[n], w.zn[n], H, B, H, K, 1, nullptr)) return NRK_EHIP;
        if (dice) dt_colstat_kernel<<<(H + 15) / 16, 1024, 0, st>>>(w.zn[n], B, H, w.mu[n], w.sd[n]);
        if (n == L - 1) break;
        if (dice) dt_dice_fwd_kernel<<<eg(BH), 256, 0, st>>>(w.zn[n], w.mu[n], w.sd[n], BH, H, w.an[n]);
        else dt_prelu_fwd_kernel<<<eg(BH), 256, 0, st>>>(w.zn[n], wts + o.slope[n], BH, w.an[n]);
    }
    {
        const int n = L - 1, H = s.H[n];
        if (dice)
            dt_head_kernel<DIN_ACT_DICE><<<(B + 3) / 4, 256, 0, st>>>(w.zn[n], w.mu[n], w.sd[n], nullptr, wts + o.w_out,
                                                                      wts + o.b_out, labels, B, H, w.loss_b, w.hb,
                                                                      w.dan[n]);
        else
            dt_head_kernel<DIN_ACT_PRELU><<<(B + 3) / 4, 256, 0, st>>>(w.zn[n], nullptr, nullptr, wts + o.slope[n],
                                                                       wts + o.w_out, wts + o.b_out, labels, B, H,
                                                                       w.loss_b, w.hb, w.dan[n]);
        dt_loss_kernel<<<1, 1024, 0, st>>>(w.loss_b, B, loss);
        NRK_CHECK_LAUNCH();
        // ---- backward: MLP
        dt_colsum_kernel<<<(H + 1 + 15) / 16, 1024, 0, st>>>(w.hb, B, H + 1, wg + o.w_out);  // d w_out | d b_out
    }
    // dan[n] holds d a_n and becomes d z_n in place; then d b_n, d W_n and d a_{n-1} (d x0 for n = 0)
    for (int n = L - 1; n >= 0; --n) {
        const int H = s.H[n], K = s.K(n);
        const int64_t BH = (int64_t)B * H;
        float* dz = w.dan[n];
        if (dice) {
            dt_dice_sums_kernel<<<(H + 15) / 16, 1024, 0, st>>>(w.zn[n], w.mu[n], w.sd[n], dz, H, 1, nullptr, B, H,
                                                                w.Sn[n]);
            dt_dice_bwd_kernel<<<eg(BH), 256, 0, st>>>(w.zn[n], w.mu[n], w.sd[n], w.Sn[n], B, H, dz);
        } else {
            const unsigned nb = grid_for(BH, 256, DT_SLOPE_BLOCKS);
            dt_prelu_bwd_kernel<<<nb, 256, 0, st>>>(w.zn[n], wts + o.slope[n], BH, dz, w.spart);
            dt_slope_final_kernel<<<1, 64, 0, st>>>(w.spart, (int)nb, wg + o.slope[n]);
        }
        dt_colsum_kernel<<<(H + 15) / 16, 1024, 0, st>>>(dz, B, H, wg + o.b[n]);
        if (dt_gemm(st, dz, 1, H, n ? w.an[n - 1] : w.x0, K, 1, nullptr, wg + o.w[n], K, H, K, B, w.ksplit,
                    w.gemm_part))
            return NRK_EHIP;
        if (dt_gemm(st, dz, H, 1, wts + o.w[n], K, 1, nullptr, n ? w.dan[n - 1] : w.dx0, K, B, K, H, 1, nullptr))
            return NRK_EHIP;
    }
    NRK_CHECK_LAUNCH();
    // ---- backward: attention
    dt_att_ds_kernel<NI><<<B, 256, 0, st>>>(ix, w.dx0, IN, w.ds);
    dt_colsum_kernel<<<(T + 15) / 16, 1024, 0, st>>>(w.ds, B, T, w.dsT);
    dt_dice_sums_kernel<<<(C + 15) / 16, 1024, 0, st>>>(w.z, w.mu_a, w.sd_a, w.ds, T, 36, wts + o.aw1, B, C, w.S_a);
    const size_t lds_bwd = sizeof(float) * (36 * WS + 2 * Di + 256 + 40 + T + T * 36) + sizeof(int) * T * NI;
    dt_att_bwd_kernel<NI><<<w.nblk, 256, lds_bwd, st>>>(ix, wts + o.aw0, wts + o.aw1, w.mu_a, w.sd_a, w.S_a, w.ds,
                                                        w.wbuf, IN, w.z, w.dx0, w.dk, w.Abuf, w.gpart);
    NRK_CHECK_LAUNCH();
    dt_colsum_kernel<<<(36 + 15) / 16, 1024, 0, st>>>(w.Abuf, B, 36, wg + o.ab0);
    if (dt_gemm(st, w.Abuf, 1, 36, w.x0 + (s.Fu + s.Fc) * 32, IN, 1, nullptr, w.Gq, Di, 36, Di, B, w.ksplit,
                w.gemm_part))
        return NRK_EHIP;
    dt_att_final_kernel<<<(36 * Di + 37 + 255) / 256, 256, 0, st>>>(w.gpart, w.nblk, Di, w.Gq, w.S_a + 2 * C, w.dsT,
                                                                     T, wg + o.aw0, wg + o.aw1, wg + o.ab1);
    NRK_CHECK_LAUNCH();
    // ---- embedding gradients
    const int64_t N = s.N;
    dt_emb_keys_kernel<<<eg(N), 256, 0, st>>>(ix, NI, N, w.keys, w.cid);
    NRK_CHECK_LAUNCH();
    size_t need = 0;
    const int bits = dt_sort_bits(s.R);
    if (rocprim::radix_sort_pairs(nullptr, need, w.keys, w.keys2, w.cid, w.cid2, (size_t)N, 0u, (unsigned)bits, st) !=
            hipSuccess ||
        need > w.sort_tmp_bytes) {
        set_error("nrk_din_train_grad: radix sort temporary storage exceeds the workspace bound");
        return NRK_EHIP;
    }
    need = w.sort_tmp_bytes;
    if (rocprim::radix_sort_pairs(w.sort_tmp, need, w.keys, w.keys2, w.cid, w.cid2, (size_t)N, 0u, (unsigned)bits,
                                  st) != hipSuccess) {
        set_error("nrk_din_train_grad: radix sort failed");
        return NRK_EHIP;
    }
    dt_emb_heads_kernel<<<eg(N), 256, 0, st>>>(w.keys2, N, w.flag);
    need = 0;
    if (rocprim::inclusive_scan(nullptr, need, w.flag, w.seg, (size_t)N, rocprim::plus<int32_t>(), st) != hipSuccess ||
        need > w.sort_tmp_bytes) {
        set_error("nrk_din_train_grad: scan temporary storage exceeds the workspace bound");
        return NRK_EHIP;
    }
    need = w.sort_tmp_bytes;
    if (rocprim::inclusive_scan(w.sort_tmp, need, w.flag, w.seg, (size_t)N, rocprim::plus<int32_t>(), st) !=
        hipSuccess) {
        set_error("nrk_din_train_grad: scan failed");
        return NRK_EHIP;
    }
    dt_emb_starts_kernel<<<eg(N), 256, 0, st>>>(w.keys2, w.flag, w.seg, N, w.starts, rows, count);
    DtSrc src{w.dx0, w.dk, IN, s.S, s.Fu + s.Fc + NI, T, NI};
    const unsigned pg = grid_for(N, 8, 8192);
    dt_emb_piece_kernel<<<pg, 256, 0, st>>>(w.cid2, w.seg, w.starts, N, src, vals, w.epart);
    dt_emb_long_kernel<<<pg, 256, 0, st>>>(w.starts, count, w.epart, vals);
    NRK_CHECK_LAUNCH();
    return NRK_OK;
}

}  // namespace nrk

using namespace nrk;

extern "C" {

// The one dispatch path of both entry points, after dt_check (ws_fn: the caller's workspace query).
static int dt_grad(const char* fn, const char* ws_fn, const DtShape& s, const float* table, const int64_t* row_base,
                   const float* weights, const int32_t* user_idx, const int32_t* item_idx, const int32_t* hist_idx,
                   const int32_t* ctx_idx, const float* mask, const float* labels, float* loss, float* w_grad,
                   int32_t* t_rows, float* t_vals, int32_t* t_count, void* workspace, size_t workspace_bytes,
                   nrk_stream_t stream) {
    auto fail = [&](const char* msg) {
        set_error(std::string(fn) + ": " + msg);
        return NRK_EINVAL;
    };
    if (!(table && row_base && weights && user_idx && item_idx && hist_idx && (ctx_idx || s.Fc == 0) && mask &&
          labels && loss && w_grad && t_rows && t_vals && t_count && workspace))
        return fail("null pointer");
    const DtWs w = dt_layout(workspace, s);
    if (workspace_bytes < w.bytes) return fail((std::string("workspace too small (") + ws_fn + ")").c_str());
    const DtIdx ix{table, row_base, user_idx, item_idx, hist_idx, ctx_idx, mask, s.Fu, s.Fc, s.B, s.T};
    hipStream_t st = as_stream(stream);
    switch (s.NI) {
        case 1: return dt_run<1>(s, w, ix, weights, labels, loss, w_grad, t_rows, t_vals, t_count, st);
        case 2: return dt_run<2>(s, w, ix, weights, labels, loss, w_grad, t_rows, t_vals, t_count, st);
        case 4: return dt_run<4>(s, w, ix, weights, labels, loss, w_grad, t_rows, t_vals, t_count, st);
        default: return dt_run<8>(s, w, ix, weights, labels, loss, w_grad, t_rows, t_vals, t_count, st);
    }
}

size_t nrk_din_train_workspace_bytes(int64_t n_table_rows, int dim, int table_dtype, int n_user, int n_item,
                                     int n_ctx, int h1, int h2, int activation, int64_t batch, int seq_len) {
    clear_error();
    DtShape s{};
    const int32_t widths[2] = {h1, h2};
    if (dt_check(__func__, n_table_rows, dim, table_dtype, n_user, n_item, n_ctx, 2, widths, activation, true, batch,
                 seq_len, &s) != NRK_OK)
        return 0;
    return dt_layout(nullptr, s).bytes;
}

int nrk_din_train_grad(const float* table, int64_t n_table_rows, int dim, int table_dtype, const int64_t* row_base,
                       int n_user, int n_item, int n_ctx, const float* weights, int h1, int h2, int activation,
                       const int32_t* user_idx, const int32_t* item_idx, const int32_t* hist_idx,
                       const int32_t* ctx_idx, const float* mask, const float* labels, int64_t batch, int seq_len,
                       float* loss, float* w_grad, int32_t* t_rows, float* t_vals, int32_t* t_count, void* workspace,
                       size_t workspace_bytes, nrk_stream_t stream) {
    clear_error();
    DtShape s{};
    const int32_t widths[2] = {h1, h2};
    const int rc = dt_check(__func__, n_table_rows, dim, table_dtype, n_user, n_item, n_ctx, 2, widths, activation,
                            true, batch, seq_len, &s);
    if (rc != NRK_OK) return rc;
    return dt_grad(__func__, "nrk_din_train_workspace_bytes", s, table, row_base, weights, user_idx, item_idx,
                   hist_idx, ctx_idx, mask, labels, loss, w_grad, t_rows, t_vals, t_count, workspace, workspace_bytes,
                   stream);
}

size_t nrk_din_train_mlp_workspace_bytes(int64_t n_table_rows, int dim, int table_dtype, int n_user, int n_item,
                                         int n_ctx, int n_layers, const int32_t* widths, int activation,
                                         int64_t batch, int seq_len) {
    clear_error();
    DtShape s{};
    if (dt_check(__func__, n_table_rows, dim, table_dtype, n_user, n_item, n_ctx, n_layers, widths, activation, false,
                 batch, seq_len, &s) != NRK_OK)
        return 0;
    return dt_layout(nullptr, s).bytes;
}

int64_t nrk_din_train_mlp_n_weights(int dim, int n_user, int n_item, int n_ctx, int n_layers, const int32_t* widths,
                                    int activation) {
    clear_error();
    DtShape s{};
    if (dt_check(__func__, 1, dim, 0, n_user, n_item, n_ctx, n_layers, widths, activation, false, 2, 1, &s) != NRK_OK)
        return 0;
    return dt_offsets(s).n;
}

int nrk_din_train_grad_mlp(const float* table, int64_t n_table_rows, int dim, int table_dtype, const int64_t* row_base,
                           int n_user, int n_item, int n_ctx, const float* weights, int n_layers,
                           const int32_t* widths, int activation, const int32_t* user_idx, const int32_t* item_idx,
                           const int32_t* hist_idx, const int32_t* ctx_idx, const float* mask, const float* labels,
                           int64_t batch, int seq_len, float* loss, float* w_grad, int32_t* t_rows, float* t_vals,
                           int32_t* t_count, void* workspace, size_t workspace_bytes, nrk_stream_t stream) {
    clear_error();
    DtShape s{};
    const int rc = dt_check(__func__, n_table_rows, dim, table_dtype, n_user, n_item, n_ctx, n_layers, widths,
                            activation, false, batch, seq_len, &s);
    if (rc != NRK_OK) return rc;
    return dt_grad(__func__, "nrk_din_train_mlp_workspace_bytes", s, table, row_base, weights, user_idx, item_idx,
                   hist_idx, ctx_idx, mask, labels, loss, w_grad, t_rows, t_vals, t_count, workspace, workspace_bytes,
                   stream);
}

int nrk_din_adam_step(float* weights, float* w_m, float* w_v, const float* w_grad, int64_t n_weights, float* table,
                      float* t_m, float* t_v, int64_t n_table_rows, int dim, const int32_t* t_rows,
                      const float* t_vals, const int32_t* t_count, double lr, double beta1, double beta2, double eps,
                      int64_t t, nrk_stream_t stream) {
    clear_error();
    if (dim != DIN_E) NRK_UNSUPPORTED("training is built for din_embedding_dim == 32");
    NRK_REQUIRE(n_weights > 0 && n_weights < ((int64_t)1 << 31), "bad n_weights");
    NRK_REQUIRE(n_table_rows > 0 && n_table_rows <= (int64_t)INT32_MAX / 32, "bad n_table_rows");
    AdamK k;
    if (const int rc = adam_scalars(__func__, lr, beta1, beta2, eps, t, &k)) return rc;
    NRK_REQUIRE(weights && w_m && w_v && w_grad && table && t_m && t_v && t_rows && t_vals && t_count, "null pointer");
    const AdamSegs<1> seg{{{table, t_m, t_v, t_rows, t_vals, t_count, n_table_rows}}};
    return adam_sweep<DIN_E>(__func__, weights, w_m, w_v, w_grad, n_weights, seg, k, as_stream(stream));
}

}  // extern "C"
