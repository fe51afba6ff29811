// din_tail.hip -- the final MLP of DINModel.forward past the first hidden
// layer's pre-activation z1, for 1 to 4 hidden layers and either activation
// (DIN.py:196-212: Linear, then Dice or nn.PReLU() per hidden layer, then
// Linear(h_L -> 1); :282-284 sigmoid).  With act_n the activation behind
// layer n (Dice with the batch statistics of z_n, or PReLU with layer n's one
// slope):
//   z_n   = act_{n-1}(z_{n-1}) W_{n-1}^T + b_{n-1}      n = 2..L   din_layer
//   logit = act_L(z_L) . w_out + b_out, prob = sigmoid              din_tail_head
// The activation is applied on load, so no activated copy is ever written.
// Two-layer Dice models keep din.hip's din_mlp2 / din_gemm<true> / din_head;
// din.hip's dispatch sends every other (depth, activation) here:
//   din_layer<Dice>   din_gemm<true>'s f32 MFMA product, writes the fp64
//                     column partials of its output for the next col_stats;
//   din_layer<PReLU>  the same product, no partials: nothing past z1 needs a
//                     statistic, so a PReLU tail runs no col_stats pass;
//   din_mlp2_prelu    din_mlp2's packed split-fp16 product for L = 2,
//                     h1 <= 256, h2 <= 128, T <= 64 (the shipped [200, 80]);
//   din_tail_head     din_head with the activation as a parameter.
// The PReLU slope is a device float read by the kernel (a trained parameter
// of the checkpoint), never a host or compile-time value.
#include "din_common.h"

namespace nrk {

template <int ACT>
__device__ __forceinline__ float tail_act(float x, float p0, float p1) {
    if constexpr (ACT == DIN_ACT_DICE) return dice_fast(x, p0, p1);  // (mean, 1 / (std + 1e-8))
    else return x > 0.0f ? x : p0 * x;                                // nn.PReLU: p0 = slope
}

// --------------------------------------------------------------- layer --
// C[M][N] = act(A)[M][K] W[N][K]^T + bias on v_mfma_f32_32x32x2_f32, the tile
// and k order of din_gemm_kernel (din.hip): workgroup = 8 waves = 64x64
// outputs, waves (wm, wn) own 32x32 blocks, kh splits K into two interleaved
// halves added in a fixed order through LDS; lane half h of chunk c takes
// k = 16c + 8h + [0, 8) of its A row and W row (two float4 each, scalar loads
// when K is no multiple of 4 or the chunk is cut).  Every sum's order is fixed
// by the shape: run-to-run deterministic.
typedef float tail_f16v __attribute__((ext_vector_type(16)));

template <int ACT>
__device__ __forceinline__ void tail_load(const float* __restrict__ A, const float2* __restrict__ astats, float slope,
                                          const float* __restrict__ W, int64_t m, bool mok, int n, bool nok, int K,
                                          int k, float (&a)[8], float (&w)[8]) {
    const bool full = k + 8 <= K;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        a[e] = 0.0f;
        w[e] = 0.0f;
    }
    if (full && ((K & 3) == 0)) {
        if (mok) {
            const float4 x = *reinterpret_cast<const float4*>(A + m * K + k);
            const float4 y = *reinterpret_cast<const float4*>(A + m * K + k + 4);
            a[0] = x.x; a[1] = x.y; a[2] = x.z; a[3] = x.w;
            a[4] = y.x; a[5] = y.y; a[6] = y.z; a[7] = y.w;
        }
        if (nok) {
            const float4 x = *reinterpret_cast<const float4*>(W + (int64_t)n * K + k);
            const float4 y = *reinterpret_cast<const float4*>(W + (int64_t)n * K + k + 4);
            w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
            w[4] = y.x; w[5] = y.y; w[6] = y.z; w[7] = y.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (k + e < K) {
                if (mok) a[e] = A[m * K + k + e];
                if (nok) w[e] = W[(int64_t)n * K + k + e];
            }
        }
    }
    if (mok) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (k + e < K) {
                if constexpr (ACT == DIN_ACT_DICE) {
                    const float2 st = astats[k + e];
                    a[e] = tail_act<ACT>(a[e], st.x, st.y);
                } else {
                    a[e] = tail_act<ACT>(a[e], slope, 0.0f);
                }
            }
    }
}

template <int ACT>
__global__ __launch_bounds__(512) void din_layer_kernel(
    const float* __restrict__ A, const float2* __restrict__ astats_all, const float* __restrict__ slope_p,
    const float* __restrict__ W, const float* __restrict__ bias, int64_t M, int64_t S, int N, int K,
    float* __restrict__ C, double* __restrict__ partial) {
    constexpr bool STATS = ACT == DIN_ACT_DICE;  // the consumer of C has this layer's activation kind
    __shared__ float red[4][16][64];
    __shared__ double cs[2][2][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv & 1, wn = (wv >> 1) & 1, kh = wv >> 2;
    const int64_t m = (int64_t)blockIdx.x * 64 + wm * 32 + (lane & 31);
    const int n = blockIdx.y * 64 + wn * 32 + (lane & 31);
    const bool mok = m < M, nok = n < N;
    const float2* astats = STATS ? astats_all + (mok ? m / S : 0) * K : nullptr;  // row m's Dice batch
    const float slope = STATS ? 0.0f : *slope_p;
    const int half = lane >> 5;
    tail_f16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    // chunks c = kh, kh + 2, ... of 16 k each, loads two chunks ahead
    const int nch = (K + 15) / 16;
    float a0[8], w0[8], a1[8], w1[8];
    int c = kh;
    if (c < nch) tail_load<ACT>(A, astats, slope, W, m, mok, n, nok, K, 16 * c + 8 * half, a0, w0);
    if (c + 2 < nch) tail_load<ACT>(A, astats, slope, W, m, mok, n, nok, K, 16 * (c + 2) + 8 * half, a1, w1);
    for (; c < nch; c += 4) {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[e], w0[e], acc, 0, 0, 0);
        if (c + 4 < nch) tail_load<ACT>(A, astats, slope, W, m, mok, n, nok, K, 16 * (c + 4) + 8 * half, a0, w0);
        if (c + 2 < nch) {
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[e], w1[e], acc, 0, 0, 0);
            if (c + 6 < nch) tail_load<ACT>(A, astats, slope, W, m, mok, n, nok, K, 16 * (c + 6) + 8 * half, a1, w1);
        }
    }
    // K halves: kh = 1 hands its accumulator to kh = 0 (fixed order)
    if (kh == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wv - 4][r][lane] = acc[r];
    }
    __syncthreads();
    if (kh == 0) {
        const int64_t mrow0 = (int64_t)blockIdx.x * 64 + wm * 32;
        double s = 0.0, ss = 0.0;
        const float bn = nok ? bias[n] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t mr = mrow0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            const float v = (acc[r] + red[wv][r][lane]) + bn;
            if (nok && mr < M) {
                C[mr * N + n] = v;
                if constexpr (STATS) {
                    s += (double)v;
                    ss += (double)v * (double)v;
                }
            }
        }
        if constexpr (STATS) {
            s += __shfl_xor(s, 32, WAVE);
            ss += __shfl_xor(ss, 32, WAVE);
            if (lane < 32) {
                cs[0][wm][wn * 32 + lane] = s;
                cs[1][wm][wn * 32 + lane] = ss;
            }
        }
    }
    if constexpr (STATS) {
        __syncthreads();
        if (tid < 64) {
            const int nn = blockIdx.y * 64 + tid;
            if (nn < N) {
                partial[((size_t)blockIdx.x * N + nn) * 2] = cs[0][0][tid] + cs[0][1][tid];
                partial[((size_t)blockIdx.x * N + nn) * 2 + 1] = cs[1][0][tid] + cs[1][1][tid];
            }
        }
    }
}

// ------------------------------------------------- mlp2 (fast), PReLU --
// z2 = PReLU(z1) W1^T + b1 on din_mlp2_kernel's split-fp16 MFMA (din.hip): the
// whole packed W1 in LDS, 128-row blocks (4 waves x 32 rows) walked by a
// persistent grid, the next k-step's A in flight.  The A scale comes from
// max(1, |a|) max |z1| of the Dice batch: |PReLU(x)| <= max(1, |a|) |x| and a
// trained slope may exceed 1, so max |z1| alone could push a scaled value past
// fp16.  No statistics of z2: its consumer is a PReLU head.
template <int NT>
__global__ __launch_bounds__(256, 2) void din_mlp2_prelu_kernel(
    const float* __restrict__ A, const float* __restrict__ slope_p, const unsigned int* __restrict__ amax,
    const unsigned int* __restrict__ wmax, const din_u4* __restrict__ wpack, const float* __restrict__ bias,
    int64_t M, int64_t S, int K, int N, float* __restrict__ C) {
    extern __shared__ __attribute__((aligned(16))) din_u4 wl[];
    const int KS = (K + DIN_E - 1) / DIN_E;
    const int CH = KS * NT * 128;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, q = lane >> 4;
    for (int c = tid; c < CH; c += 256) wl[c] = wpack[c];
    __syncthreads();
    const din_half8* wb = reinterpret_cast<const din_half8*>(wl);
    const float s_w = pow2_scale(__uint_as_float(*wmax));
    const float slope = *slope_p;
    const float grow = fmaxf(1.0f, fabsf(slope));
    float bns[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = 16 * j + (lane & 15);
        bns[j] = bias[n < N ? n : N - 1];
    }
    const int64_t nrb = (M + MLP1_ROWS - 1) / MLP1_ROWS;
    typedef float f4n __attribute__((ext_vector_type(4)));
    for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
        const int64_t m0 = rb * MLP1_ROWS + wv * 32;
        const int64_t seg = (m0 < M ? m0 : M - 1) / S;
        const float s_a = pow2_scale(fminf(grow * __uint_as_float(amax[seg]), 3.0e38f));
        int64_t mrow[2];
        bool mok[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            mrow[a] = m0 + 16 * a + (lane & 15);
            mok[a] = mrow[a] < M;
        }
        auto load = [&](int s, int a, f4n (&x)[2]) {
            const int k = DIN_E * s + 8 * q;
            x[0] = x[1] = f4n{0.0f, 0.0f, 0.0f, 0.0f};
            if (!mok[a]) return;
            const float* p = A + mrow[a] * K + k;
            if (k + 8 <= K && (K & 3) == 0) {
                x[0] = *reinterpret_cast<const f4n*>(p);
                x[1] = *reinterpret_cast<const f4n*>(p + 4);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (k + e < K) x[e >> 2][e & 3] = p[e];
            }
        };
        din_f4 acc[2][NT];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[a][j] = din_f4{0.0f, 0.0f, 0.0f, 0.0f};
        f4n cur[2][2], nxt[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a) load(0, a, cur[a]);
        for (int s = 0; s < KS; ++s) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
                if (s + 1 < KS) load(s + 1, a, nxt[a]);
            din_half8 ahi[2], alo[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                float v[8];
                // (columns past K were loaded as 0, and PReLU(0) = 0)
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = tail_act<DIN_ACT_PRELU>(cur[a][e >> 2][e & 3], slope, 0.0f);
                split8(v, s_a, ahi[a], alo[a]);
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const din_half8 bh = wb[((s * NT + j) * 2) * 64 + lane];
                const din_half8 bl = wb[((s * NT + j) * 2 + 1) * 64 + lane];
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    acc[a][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi[a], bh, acc[a][j], 0, 0, 0);
                    acc[a][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi[a], bl, acc[a][j], 0, 0, 0);
                    acc[a][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo[a], bh, acc[a][j], 0, 0, 0);
                }
            }
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                cur[a][0] = nxt[a][0];
                cur[a][1] = nxt[a][1];
            }
        }
        // epilogue: C = acc / (s_a s_w) + bias (row 16a + 4q + r, column 16j + (lane & 15))
        const float inv = 1.0f / (s_a * s_w);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int n = 16 * j + (lane & 15);
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t m = m0 + 16 * a + 4 * q + r;
                    if (n < N && m < M) C[m * N + n] = acc[a][j][r] * inv + bns[j];
                }
        }
    }
}

// ---------------------------------------------------------------- head --
// din_head_kernel's shape (din.hip): 16 lanes per sample, lane l16 takes
// j = l16, l16 + 16, ... in order, the 16 partial sums combined by the fixed
// DPP tree of row16_sum; grid-strided over the samples.
template <int ACT>
__global__ __launch_bounds__(256) void din_tail_head_kernel(const float* __restrict__ Z,
                                                            const float2* __restrict__ zstats_all,
                                                            const float* __restrict__ slope_p, int64_t B, int64_t S,
                                                            int H, const float* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ probs,
                                                            float* __restrict__ logits) {
    const int l16 = threadIdx.x & 15;
    const float b0 = bias[0];
    const float slope = ACT == DIN_ACT_PRELU ? *slope_p : 0.0f;
    for (int64_t b = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4; b < B; b += (int64_t)gridDim.x * 16) {
        const float* zr = Z + b * H;
        float s = 0.0f;
        if constexpr (ACT == DIN_ACT_DICE) {
            const float2* zstats = zstats_all + (b / S) * H;
            for (int j = l16; j < H; j += 16) {
                const float2 st = zstats[j];
                s += w[j] * tail_act<ACT>(zr[j], st.x, st.y);
            }
        } else {
            for (int j = l16; j < H; j += 16) s += w[j] * tail_act<ACT>(zr[j], slope, 0.0f);
        }
        s = row16_sum(s);
        if (l16 == 0) {
            const float lg = s + b0;
            if (logits) logits[b] = lg;
            probs[b] = 1.0f / (1.0f + expf(-lg));
        }
    }
}

// ----------------------------------------------------------- launchers --
void din_tail_layer(int act, const float* A, const float2* stats, const float* slope, const float* W,
                    const float* bias, int64_t M, int64_t S, int N, int K, float* C, double* partial,
                    hipStream_t s) {
    const dim3 grid((unsigned)((M + 63) / 64), (unsigned)((N + 63) / 64));
    if (act == DIN_ACT_DICE)
        din_layer_kernel<DIN_ACT_DICE><<<grid, 512, 0, s>>>(A, stats, nullptr, W, bias, M, S, N, K, C, partial);
    else
        din_layer_kernel<DIN_ACT_PRELU><<<grid, 512, 0, s>>>(A, nullptr, slope, W, bias, M, S, N, K, C, nullptr);
}

template <int NT>
static void launch_mlp2_prelu(const float* A, const float* slope, const unsigned int* amax,
                              const unsigned int* wmax, const din_u4* wpack, const float* bias, int64_t M, int64_t S,
                              int K, int N, float* C, hipStream_t s) {
    auto lds = [](int ks) { return (size_t)ks * NT * 2048; };  // the packed W1
    static std::atomic<uint64_t> lds_set{0};
    lds_limit_once(lds_set, (const void*)din_mlp2_prelu_kernel<NT>, lds(256 / DIN_E));  // K <= 256
    din_mlp2_prelu_kernel<NT><<<grid_for(M, MLP1_ROWS, 512), 256, lds((K + DIN_E - 1) / DIN_E), s>>>(
        A, slope, amax, wmax, wpack, bias, M, S, K, N, C);
}

void din_tail_mlp2_prelu(int nt, const float* A, const float* slope, const unsigned int* amax,
                         const unsigned int* wmax, const din_u4* wpack, const float* bias, int64_t M, int64_t S,
                         int K, int N, float* C, hipStream_t s) {
    // nt = din_mlp2_nt(N): 2, 4, 5 or 8 column tiles of 16
    if (nt <= 2) launch_mlp2_prelu<2>(A, slope, amax, wmax, wpack, bias, M, S, K, N, C, s);
    else if (nt <= 4) launch_mlp2_prelu<4>(A, slope, amax, wmax, wpack, bias, M, S, K, N, C, s);
    else if (nt <= 5) launch_mlp2_prelu<5>(A, slope, amax, wmax, wpack, bias, M, S, K, N, C, s);
    else launch_mlp2_prelu<8>(A, slope, amax, wmax, wpack, bias, M, S, K, N, C, s);
}

void din_tail_head(int act, const float* Z, const float2* stats, const float* slope, int64_t B, int64_t S, int H,
                   const float* w, const float* bias, float* probs, float* logits, hipStream_t s) {
    const unsigned grid = grid_for(B, 16, 8192);
    if (act == DIN_ACT_DICE)
        din_tail_head_kernel<DIN_ACT_DICE><<<grid, 256, 0, s>>>(Z, stats, nullptr, B, S, H, w, bias, probs, logits);
    else
        din_tail_head_kernel<DIN_ACT_PRELU><<<grid, 256, 0, s>>>(Z, nullptr, slope, B, S, H, w, bias, probs, logits);
}

}  // namespace nrk
