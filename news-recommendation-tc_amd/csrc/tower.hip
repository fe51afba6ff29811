// tower.hip -- YouTubeDNN two-tower forward (eval) on gfx950.
//
// User tower: YoutubeDNN.forward (src/recall/youtubednn_recaller.py:129-178)
// as _extract_embeddings drives it (:425-470), fused with the numpy
// re-normalisation of :467-470.  Item tower: get_item_embedding (:184-188)
// fused with :485-489.  Memory-bound gathers (1 + T rows of D fp32 per user)
// feeding a 2-layer MLP that fits in LDS; four users per wave pass at
// h0 <= 64 (tt_user_kernel_pass), one wave per user otherwise.
#include "tower_common.h"

namespace nrk {

template <int D>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void tt_user_kernel(
    const float* __restrict__ user_table, const float* __restrict__ item_table,
    const int32_t* __restrict__ uid, const int32_t* __restrict__ hist,
    const int32_t* __restrict__ hist_len, int64_t n, int T, const float* __restrict__ w0,
    const float* __restrict__ b0, int h0, const float* __restrict__ w1,
    const float* __restrict__ b1, int h1, float* __restrict__ out) {
    // the 4-wide reads of sx / the weight rows below stay 16-B aligned and
    // inside their own row only while 2D is a multiple of 4 (the host allows
    // D = 16, 32, 64 only)
    static_assert(D % 2 == 0 && D >= 16 && D <= 64 && (D & (D - 1)) == 0, "tt_user_kernel: D in {16, 32, 64}");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // weight rows padded to a multiple of 4 floats + 4: lane o reads row o, so
    // an unpadded power-of-two row stride would put all 64 lanes on one LDS
    // bank; with the padding the rows are 16-B aligned for the 4-wide reads
    // and lane o's row starts 4 banks after lane o - 1's
    const int S0 = 2 * D + 4, h0p = (h0 + 3) & ~3, S1 = h0p + 4, h1p = (h1 + 3) & ~3;
    float* sw0 = lds;               // [h0][S0]
    float* sb0 = sw0 + h0 * S0;     // [h0] (h0p)
    float* sw1 = sb0 + h0p;         // [h1][S1]
    float* sb1 = sw1 + h1 * S1;     // [h1] (h1p)
    // per-wave broadcast rows for the two matvecs: [x (2D) | y0 (h0)]; every
    // lane reads the same word (LDS broadcast) instead of a v_readlane per term
    float* sx = sb1 + h1p + (threadIdx.x >> 6) * (2 * D + 128);
    for (int i = threadIdx.x; i < h0 * 2 * D; i += blockDim.x) sw0[(i / (2 * D)) * S0 + i % (2 * D)] = w0[i];
    for (int i = threadIdx.x; i < h0; i += blockDim.x) sb0[i] = b0[i];
    for (int i = threadIdx.x; i < h1 * h0; i += blockDim.x) sw1[(i / h0) * S1 + i % h0] = w1[i];
    for (int i = threadIdx.x; i < h1; i += blockDim.x) sb1[i] = b1[i];
    __syncthreads();  // the only block barrier: the user loop below is per wave

    constexpr int P = WAVE / D;  // history phases per lane group
    // history rows in flight per lane (a config-2 user, T = 30 at D = 32, has
    // up to 15 per lane: two rounds).  All 16 at once measured slower in the
    // bench (tower 0.330-0.334 vs 0.294-0.295 ms, one box, two pairs): a
    // round issues CH unconditional loads per lane, and most histories are short
    constexpr int CH = 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int d = lane % D, ph = lane / D;
    const int64_t wstride = (int64_t)gridDim.x * 4;
    // software pipeline over this wave's users: the next user's length, id and
    // history indices (lane t holds index t; T <= 64) are loaded while this
    // user's rows are summed, and the rows themselves are issued CH at a time
    // (unconditional loads: slots past the length read row 0 and are not
    // added), so no load waits on another in flight.
    auto meta = [&](int64_t uu, int& len, int32_t& uidv, int32_t& hv) {
        const bool ok = uu < n;
        len = ok ? hist_len[uu] : 0;
        uidv = ok ? uid[uu] : 0;
        hv = ok && lane < T ? hist[uu * T + lane] : 0;
    };
    int64_t u = (int64_t)blockIdx.x * 4 + wave;
    int len, uidv;
    int32_t hv;
    meta(u, len, uidv, hv);
    // user u's output row is stored during user u + wstride, after that
    // user's first gathers are issued: a store counts in vmcnt, so one issued
    // at the end of a user made the next user's first wait a full store round
    // trip; issued behind the gathers its acknowledgement overlaps them
    float pout = 0.0f;
    int64_t pu = -1;
    for (; u < n; u += wstride) {
        int nlen, nuid;
        int32_t nhv;
        meta(u + wstride, nlen, nuid, nhv);
        const float xu = user_table[(int64_t)uidv * D + d];
        float sum = 0.0f;
        const int nit = (len + P - 1) / P;  // wave-uniform
        for (int i0 = 0; i0 < nit; i0 += CH) {
            float v[CH];
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                const int t = ph + P * (i0 + e);
                const int32_t r = __shfl(hv, t < T ? t : 0, WAVE);
                v[e] = item_table[(int64_t)(t < len ? r : 0) * D + d];
            }
            if (i0 == 0 && pu >= 0) {
                if (lane < h1) out[pu * h1 + lane] = pout;
                pu = -1;
            }
#pragma unroll
            for (int e = 0; e < CH; ++e)
                if (ph + P * (i0 + e) < len) sum += v[e];  // t ascending, as before
        }
#pragma unroll
        for (int off = D; off < WAVE; off <<= 1) sum += __shfl_xor(sum, off, WAVE);
        // lane q < D holds x[q] = E_u[uid][q] and x[D + q] = mean[q]
        const float xm = sum / ((float)len + 1e-8f);
        // layer 0: lane o (and o + 64) owns output o; same order as a
        // q-ascending dot (inputs broadcast from LDS)
        if (lane < D) {
            sx[lane] = xu;
            sx[D + lane] = xm;
        }
        __builtin_amdgcn_wave_barrier();
        float y0 = 0.0f, y1 = 0.0f;
        {
            // product and sum rounded separately in every chain of both
            // layers (see tt_user_mlp_kernel): left to the compiler, the
            // 4-wide loops below became packed multiplies + adds, the
            // h0 > 64 pair and layer 1's tail loop fmas
#pragma clang fp contract(off)
            float z0 = lane < h0 ? sb0[lane] : 0.0f;
            float z1 = lane + WAVE < h0 ? sb0[lane + WAVE] : 0.0f;
            const float* wr0 = sw0 + (lane < h0 ? lane : 0) * S0;
            const float* wr1 = sw0 + (lane + WAVE < h0 ? lane + WAVE : 0) * S0;
            // 4 inputs (broadcast) and 4 weights per LDS read; the
            // chain still runs q = 0, 1, 2, ... in order.  Outputs 64 ..
            // only when h0 > 64 (round 6: the second chain ran, on row 0,
            // for every h0)
            if (h0 > WAVE) {
#pragma unroll 2
                for (int q = 0; q < 2 * D; q += 4) {
                    const float4 xq = *reinterpret_cast<const float4*>(sx + q);
                    const float4 a = *reinterpret_cast<const float4*>(wr0 + q);
                    const float4 b = *reinterpret_cast<const float4*>(wr1 + q);
                    z0 += a.x * xq.x;
                    z0 += a.y * xq.y;
                    z0 += a.z * xq.z;
                    z0 += a.w * xq.w;
                    z1 += b.x * xq.x;
                    z1 += b.y * xq.y;
                    z1 += b.z * xq.z;
                    z1 += b.w * xq.w;
                }
            } else {
#pragma unroll 2
                for (int q = 0; q < 2 * D; q += 4) {
                    const float4 xq = *reinterpret_cast<const float4*>(sx + q);
                    const float4 a = *reinterpret_cast<const float4*>(wr0 + q);
                    z0 += a.x * xq.x;
                    z0 += a.y * xq.y;
                    z0 += a.z * xq.z;
                    z0 += a.w * xq.w;
                }
            }
            y0 = fmaxf(z0, 0.0f);
            y1 = fmaxf(z1, 0.0f);
        }
        // layer 1: lane o < h1 owns output o
        float* sy = sx + 2 * D;
        if (lane < h0) sy[lane] = y0;
        if (lane + WAVE < h0) sy[lane + WAVE] = y1;
        __builtin_amdgcn_wave_barrier();
        float v = 0.0f;
        {
#pragma clang fp contract(off)
            float z = lane < h1 ? sb1[lane] : 0.0f;
            const float* wr = sw1 + (lane < h1 ? lane : 0) * S1;
            int q = 0;
            for (; q + 4 <= h0; q += 4) {
                const float4 yq = *reinterpret_cast<const float4*>(sy + q);
                const float4 a = *reinterpret_cast<const float4*>(wr + q);
                z += a.x * yq.x;
                z += a.y * yq.y;
                z += a.z * yq.z;
                z += a.w * yq.w;
            }
            for (; q < h0; ++q) z += wr[q] * sy[q];
            v = lane < h1 ? fmaxf(z, 0.0f) : 0.0f;
        }
        __builtin_amdgcn_wave_barrier();  // sx / sy are rewritten for the next user
        const float nn = sqrtf(wave_sum_f32(v * v));
        v = v / fmaxf(nn, 1e-12f);
        float n2 = sqrtf(wave_sum_f32(v * v));
        if (n2 == 0.0f) n2 = 1.0f;
        if (pu >= 0 && lane < h1) out[pu * h1 + lane] = pout;  // no gathers this user (len == 0)
        pout = v / n2;
        pu = u;
        len = nlen;
        uidv = nuid;
        hv = nhv;
    }
    if (pu >= 0 && lane < h1) out[pu * h1 + lane] = pout;
}

// tt_user_kernel at h0 <= 64 with TT_PASS_G users per wave pass: the
// one-user form re-reads both layers' weights from LDS for every user, adds
// one scalar term per instruction and runs layer 1 on D of the 64 lanes.  Here
// a weight read is shared by the pass's four users, the chains advance two
// users per packed instruction and layer 1 fills the wave (lane l: output
// l % D of the 4 D / 64 users of group l / D).  Every user's arithmetic is
// tt_user_kernel's, operation for operation: the per-phase t-ascending history
// sums, the xor fold of the phases, / (len + 1e-8f), the q-ascending chains
// z = z + RN(w[q] * x[q]) from the bias, and the two norms as that kernel is
// compiled: wave_sum_f32's first level is fma(v, v, the other half's square)
// there, which at D < 64 adds the idle half's +0.0f to the square and changes
// no bit, as do the levels down to D; the levels below D are plain adds.
// (The name starts with tt_user_kernel so that the bench's busy report, which
// looks the tower up by that prefix, finds whichever of the two ran.)
constexpr int TT_PASS_G = 4;
constexpr int tt_pass_tile(int dim) { return 2 * dim * TT_PASS_G + 64 * TT_PASS_G; }  // floats per wave: xs | ys
template <int N>
using fvec = float __attribute__((ext_vector_type(N)));
typedef fvec<2> f32x2;
typedef fvec<4> f32x4;

template <int D>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void tt_user_kernel_pass(
    const float* __restrict__ user_table, const float* __restrict__ item_table,
    const int32_t* __restrict__ uid, const int32_t* __restrict__ hist,
    const int32_t* __restrict__ hist_len, int64_t n, int T, const float* __restrict__ w0,
    const float* __restrict__ b0, int h0, const float* __restrict__ w1,
    const float* __restrict__ b1, float* __restrict__ out) {
    static_assert(D == 16 || D == 32 || D == 64, "tt_user_kernel_pass: D in {16, 32, 64}");
    constexpr int G = TT_PASS_G, h1 = D;
    constexpr int P = WAVE / D;       // history phases, and lane groups of layer 1
    constexpr int UL = G * D / WAVE;  // users a lane carries in layer 1 and the norms
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // weights and biases laid out as in tt_user_kernel (padded rows)
    const int S0 = 2 * D + 4, h0p = (h0 + 3) & ~3, S1 = h0p + 4;
    float* sw0 = lds;            // [h0][S0]
    float* sb0 = sw0 + h0 * S0;  // [h0] (h0p)
    float* sw1 = sb0 + h0p;      // [h1][S1]
    float* sb1 = sw1 + h1 * S1;  // [h1]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // per-wave tile.  xs[q][g]: input q of the pass's user g, so one broadcast
    // 16-B read returns term q for all four.  ys[group][q][UL]: y0[q] of the
    // group's users, 4 / UL q per 16-B read; before layer 0 the same words
    // hold the pass's history indices (as bits), [g][phase][t / P]
    float* xs = sb1 + h1 + wave * tt_pass_tile(D);
    float* ys = xs + 2 * D * G;
    for (int i = threadIdx.x; i < h0 * 2 * D; i += blockDim.x) sw0[(i / (2 * D)) * S0 + i % (2 * D)] = w0[i];
    for (int i = threadIdx.x; i < h0; i += blockDim.x) sb0[i] = b0[i];
    for (int i = threadIdx.x; i < h1 * h0; i += blockDim.x) sw1[(i / h0) * S1 + i % h0] = w1[i];
    for (int i = threadIdx.x; i < h1; i += blockDim.x) sb1[i] = b1[i];
    __syncthreads();  // the only block barrier: the pass loop below is per wave

    constexpr int CH = 4;  // history rows in flight per lane and user (8 slots a round)
    const int d = lane % D, ph = lane / D;
    const int64_t npass = (n + G - 1) / G, pstride = (int64_t)__builtin_amdgcn_readfirstlane(gridDim.x) * 4;
    // the next pass's lengths, ids (wave-uniform) and history indices (lane t
    // holds slot t) are loaded while this pass runs; users past n: len 0, row 0
    auto meta = [&](int64_t pp, int (&len)[G], int32_t (&uidv)[G], int32_t (&hv)[G]) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int64_t uu = pp * G + g;
            const bool ok = uu < n;
            len[g] = ok ? hist_len[uu] : 0;
            uidv[g] = ok ? uid[uu] : 0;
            hv[g] = ok && lane < T ? hist[uu * T + lane] : 0;
        }
    };
    int64_t p = (int64_t)blockIdx.x * 4 + wave;
    int len[G];
    int32_t uidv[G], hv[G];
    meta(p, len, uidv, hv);
    // a pass's rows are stored during the next pass, behind its first gathers
    // (see tt_user_kernel); lane l keeps column l % D of its group's UL rows
    float pout[UL] = {};
    int64_t prev = -1;  // the pass whose rows are pending
    auto store_rows = [&]() {
        const int64_t r0 = prev * G + UL * ph;
#pragma unroll
        for (int j = 0; j < UL; ++j)
            if (r0 + j < n) out[(r0 + j) * h1 + d] = pout[j];
        prev = -1;
    };
    for (; p < npass; p += pstride) {
        int nlen[G];
        int32_t nuid[G], nhv[G];
        meta(p + pstride, nlen, nuid, nhv);
        float xu[G], sum[G];
        int nit[G], nl[G], nitmax = 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            xu[g] = user_table[(int64_t)uidv[g] * D + d];
            ys[g * 64 + (lane % P) * D + lane / P] = __int_as_float(hv[g]);
            sum[g] = 0.0f;
            // a length past T (outside the contract) gathers T slots: the
            // index tile holds no more
            const int ln = len[g] < T ? len[g] : T;
            nit[g] = (ln + P - 1) / P;      // slots of phase 0, wave-uniform
            nl[g] = (ln + P - 1 - ph) / P;  // live slots of this lane's phase
            nitmax = nit[g] > nitmax ? nit[g] : nitmax;
        }
        wave_sync_lds();
        // slot t = ph + P i of user g; a user's rounds stop at its own nit, a
        // slot past the length reads row 0 and is not added
        for (int i0 = 0; i0 < nitmax; i0 += CH) {
            float v[G][CH];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (i0 < nit[g]) {
                    const f32x4 r4 = *reinterpret_cast<const f32x4*>(ys + g * 64 + ph * D + i0);
#pragma unroll
                    for (int e = 0; e < CH; ++e) {
                        const uint32_t r = i0 + e < nl[g] ? (uint32_t)__float_as_int(r4[e]) : 0u;
                        v[g][e] = item_table[(int64_t)r * D + d];
                    }
                }
            }
            if (i0 == 0 && prev >= 0) store_rows();
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (i0 < nit[g]) {
#pragma unroll
                    for (int e = 0; e < CH; ++e)
                        if (i0 + e < nl[g]) sum[g] += v[g][e];  // t ascending
                }
            }
        }
        f32x4 xu4, xm4;
#pragma unroll
        for (int g = 0; g < G; ++g) {
#pragma unroll
            for (int off = D; off < WAVE; off <<= 1) sum[g] += __shfl_xor(sum[g], off, WAVE);
            xu4[g] = xu[g];
            xm4[g] = sum[g] / ((float)len[g] + 1e-8f);
        }
        wave_sync_lds();  // the indices in ys are read
        if (lane < D) {  // x[q] = E_u[uid][q], x[D + q] = mean[q]
            *reinterpret_cast<f32x4*>(xs + lane * G) = xu4;
            *reinterpret_cast<f32x4*>(xs + (D + lane) * G) = xm4;
        }
        wave_sync_lds();
        {
            // product and sum rounded separately in every chain of both
            // layers, and in the norms below (left to the compiler, their
            // first add would fuse with the square at every D)
#pragma clang fp contract(off)
            // layer 0: lane o owns output o for the four users
            const int o = lane < h0 ? lane : 0;
            const float* wr0 = sw0 + o * S0;
            const float bz = lane < h0 ? sb0[lane] : 0.0f;
            f32x2 z01 = {bz, bz}, z23 = {bz, bz};
#pragma unroll 2
            for (int q = 0; q < 2 * D; q += 4) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(wr0 + q);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 x = *reinterpret_cast<const f32x4*>(xs + (q + j) * G);
                    const f32x2 w = {a[j], a[j]};
                    z01 = z01 + w * x.xy;
                    z23 = z23 + w * x.zw;
                }
            }
            if (lane < h0) {  // user g: group g / UL, slot g % UL
                const f32x4 y = {fmaxf(z01.x, 0.0f), fmaxf(z01.y, 0.0f), fmaxf(z23.x, 0.0f), fmaxf(z23.y, 0.0f)};
                if constexpr (UL == 4) {
                    *reinterpret_cast<f32x4*>(ys + lane * 4) = y;
                } else if constexpr (UL == 2) {
                    *reinterpret_cast<f32x2*>(ys + lane * 2) = y.xy;
                    *reinterpret_cast<f32x2*>(ys + 128 + lane * 2) = y.zw;
                } else {
#pragma unroll
                    for (int g = 0; g < G; ++g) ys[g * 64 + lane] = y[g];
                }
            }
            wave_sync_lds();
            // layer 1: lane l owns output l % D for the UL users of group l / D
            const float* wr = sw1 + d * S1;
            const float* yp = ys + ph * (64 * UL);
            fvec<UL> z = (fvec<UL>)(sb1[d]);
            int q = 0;
            for (; q + 4 <= h0; q += 4) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(wr + q);
                float yb[4 * UL];
#pragma unroll
                for (int k = 0; k < UL; ++k) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(yp + q * UL + 4 * k);
#pragma unroll
                    for (int j = 0; j < 4; ++j) yb[4 * k + j] = t[j];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    fvec<UL> y;
#pragma unroll
                    for (int k = 0; k < UL; ++k) y[k] = yb[j * UL + k];
                    z = z + (fvec<UL>)(a[j]) * y;
                }
            }
            for (; q < h0; ++q) z = z + (fvec<UL>)(wr[q]) * *reinterpret_cast<const fvec<UL>*>(yp + q * UL);
            float v[UL], nrm[UL];
#pragma unroll
            for (int j = 0; j < UL; ++j) v[j] = fmaxf(z[j], 0.0f);
            wave_sync_lds();  // xs / ys are rewritten by the next pass
            auto norms = [&]() {
#pragma unroll
                for (int j = 0; j < UL; ++j) {
                    float s = v[j] * v[j];
                    if constexpr (D == WAVE) s = __builtin_fmaf(v[j], v[j], __shfl_xor(s, 32, WAVE));
#pragma unroll
                    for (int m = (D == WAVE ? 16 : D / 2); m > 0; m >>= 1) s = s + __shfl_xor(s, m, WAVE);
                    nrm[j] = sqrtf(s);
                }
            };
            norms();
#pragma unroll
            for (int j = 0; j < UL; ++j) v[j] = v[j] / fmaxf(nrm[j], 1e-12f);
            norms();
            if (prev >= 0) store_rows();  // no gathers this pass (every len == 0)
#pragma unroll
            for (int j = 0; j < UL; ++j) pout[j] = v[j] / (nrm[j] == 0.0f ? 1.0f : nrm[j]);
        }
        prev = p;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            len[g] = nlen[g];
            uidv[g] = nuid[g];
            hv[g] = nhv[g];
        }
    }
    if (prev >= 0) store_rows();
}

// Any depth (TtLayers, tower_common.h).  Same gather (tt_hist_mean) and
// re-normalisation as tt_user_kernel; the layers run from one packed
// weight buffer (per layer W_l [w_l, in_l] row-major, then b_l [w_l]) read
// through the caches, lane o owning outputs o, o + 64, ..., inputs broadcast
// from a per-wave LDS row; each output is the same q-ascending chain as the
// two-layer kernel, z = z + w[q] * x[q] with the product rounded before the
// sum (fp contract off in both), so [h0, D] gives the same bits from either.
template <int D>
__global__ __launch_bounds__(256) void tt_user_mlp_kernel(
    const float* __restrict__ user_table, const float* __restrict__ item_table,
    const int32_t* __restrict__ uid, const int32_t* __restrict__ hist,
    const int32_t* __restrict__ hist_len, int64_t n, int T, const float* __restrict__ wts, TtLayers ly,
    float* __restrict__ out) {
    __shared__ float sx[4][2][TT_MAXW > 2 * D ? TT_MAXW : 2 * D];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t wstride = (int64_t)gridDim.x * 4;
    for (int64_t u = (int64_t)blockIdx.x * 4 + wave; u < n; u += wstride) {
        const int32_t hv = lane < T ? hist[u * T + lane] : 0;
        const float xu = user_table[(int64_t)uid[u] * D + lane % D];
        const float xm = tt_hist_mean<D>(item_table, hv, hist_len[u], T, lane);
        if (lane < D) {
            sx[wave][0][lane] = xu;
            sx[wave][0][D + lane] = xm;
        }
        wave_sync_lds();
        int in = 2 * D, cur = 0;
        const float* wl = wts;
        for (int l = 0; l < ly.n; ++l) {
            const int wo = ly.w[l];
            const float* bl = wl + (size_t)wo * in;
            for (int o = lane; o < wo; o += WAVE) {
                // as in tt_user_kernel: the two kernels give the same bits
#pragma clang fp contract(off)
                float z = bl[o];
                const float* wr = wl + (size_t)o * in;
                for (int qq = 0; qq < in; ++qq) z += wr[qq] * sx[wave][cur][qq];
                sx[wave][cur ^ 1][o] = fmaxf(z, 0.0f);
            }
            wave_sync_lds();
            wl = bl + wo;
            in = wo;
            cur ^= 1;
        }
        const float v = lane < D ? sx[wave][cur][lane] : 0.0f;
        const float nn = sqrtf(wave_sum_f32(v * v));
        const float v1 = v / fmaxf(nn, 1e-12f);
        float n2 = sqrtf(wave_sum_f32(v1 * v1));
        if (n2 == 0.0f) n2 = 1.0f;
        if (lane < D) out[u * D + lane] = v1 / n2;
        wave_sync_lds();  // sx is rewritten for the next user
    }
}

template <int D>
__global__ __launch_bounds__(256) void tt_item_kernel(const float* __restrict__ table,
                                                      const int32_t* __restrict__ ids, int64_t n,
                                                      float* __restrict__ out) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n;
         r += (int64_t)gridDim.x * blockDim.x) {
        const float* src = table + (int64_t)ids[r] * D;
        float v[D];
        float s = 0.0f;
#pragma unroll
        for (int q = 0; q < D; ++q) {
            v[q] = src[q];
            s += v[q] * v[q];
        }
        const float inv = fmaxf(sqrtf(s), 1e-12f);
        float s2 = 0.0f;
#pragma unroll
        for (int q = 0; q < D; ++q) {
            v[q] = v[q] / inv;
            s2 += v[q] * v[q];
        }
        const float n2 = sqrtf(s2);
#pragma unroll
        for (int q = 0; q < D; ++q) out[r * D + q] = v[q] / n2;
    }
}

}  // namespace nrk

using namespace nrk;

// workgroups of 256 threads resident at once on the device, at most one per 4 users
static int tt_grid(const void* fn, size_t lds, int64_t n) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((n + 3) / 4, resident_blocks(fn, 256, lds)));
}

// tt_user_kernel's dynamic LDS: both layers' padded weights and biases, then
// the four waves' rows.  It grows with h0, so h0 = 128 (the entry point's
// limit) is an instantiation's most: 106,240 bytes at dim 64
constexpr size_t tt_user_lds(int dim, int h0, int h1) {
    const size_t h0p = (size_t)((h0 + 3) & ~3), h1p = (size_t)((h1 + 3) & ~3);
    return sizeof(float) *
           ((size_t)h0 * (2 * dim + 4) + h0p + (size_t)h1 * (h0p + 4) + h1p + (size_t)4 * (2 * dim + 128));
}
constexpr int TT_H0_MAX = 128;

// tt_user_kernel_pass's: the same weights, then each wave's tile (2 KB at dim 32)
constexpr size_t tt_pass_lds(int dim, int h0) {
    const size_t h0p = (size_t)((h0 + 3) & ~3);
    return sizeof(float) * ((size_t)h0 * (2 * dim + 4) + h0p + (size_t)dim * (h0p + 4) + dim +
                            (size_t)4 * tt_pass_tile(dim));
}
// users per wave pass of the kernel nrk_tt_user_fwd runs at h0, 0 for tt_user_kernel
static int tt_pass_users(int h0) { return h0 <= WAVE ? TT_PASS_G : 0; }

extern "C" {

int nrk_tt_user_fwd(const float* user_table, int64_t n_user_rows, const float* item_table,
                    int64_t n_item_rows, int dim, const int32_t* uid, const int32_t* hist,
                    const int32_t* hist_len, int64_t n, int seq_len, const float* w0,
                    const float* b0, int h0, const float* w1, const float* b1, int h1,
                    float* out, nrk_stream_t stream) {
    clear_error();
    NRK_REQUIRE(n >= 0 && seq_len >= 1 && seq_len <= 64, "bad sizes (seq_len must be in [1, 64])");
    NRK_REQUIRE(n_user_rows > 0 && n_item_rows > 0, "empty embedding tables");
    if (const int rc = tt_check_shape(__func__, dim)) return rc;
    NRK_REQUIRE(h0 >= 1 && h0 <= TT_H0_MAX, "h0 must be in [1, 128]");
    NRK_REQUIRE(h1 == dim, TT_LAST_WIDTH);
    if (n == 0) return NRK_OK;
    NRK_REQUIRE(user_table && item_table && uid && hist && hist_len && w0 && b0 && w1 && b1 && out,
                "null pointer");
    const size_t lds = tt_user_lds(dim, h0, h1);
    hipStream_t s = as_stream(stream);
    // persistent grid of resident workgroups only (the weights' LDS admits 4 or
    // 5 per CU): a grid larger than the resident set left the queued
    // workgroups to run after the first ones finished, on a thinner machine
    if (tt_pass_users(h0)) {
        const size_t plds = tt_pass_lds(dim, h0);
        // at most one workgroup per 4 passes of TT_PASS_G users
        const int64_t want = (n + 4 * TT_PASS_G - 1) / (4 * TT_PASS_G);
        tt_for_dim(dim, [&](auto dc) {
            constexpr int DD = decltype(dc)::value;
            static_assert(tt_pass_lds(DD, WAVE) <= 65536, "tt_user_kernel_pass LDS: under the default limit");
            const int grid = (int)std::max<int64_t>(
                1, std::min(want, resident_blocks((const void*)tt_user_kernel_pass<DD>, 256, plds)));
            tt_user_kernel_pass<DD><<<grid, 256, plds, s>>>(user_table, item_table, uid, hist, hist_len, n, seq_len, w0,
                                                            b0, h0, w1, b1, out);
        });
        NRK_CHECK_LAUNCH();
        return NRK_OK;
    }
    tt_for_dim(dim, [&](auto dc) {
        constexpr int DD = decltype(dc)::value;
        constexpr size_t lds_max = tt_user_lds(DD, TT_H0_MAX, DD);  // h1 == dim
        static_assert(lds_max <= CU_LDS_BYTES, "tt_user_kernel LDS");
        static std::atomic<uint64_t> lds_set{0};
        lds_limit_once(lds_set, (const void*)tt_user_kernel<DD>, lds_max);
        const int grid = tt_grid((const void*)tt_user_kernel<DD>, lds, n);
        tt_user_kernel<DD><<<grid, 256, lds, s>>>(user_table, item_table, uid, hist, hist_len, n, seq_len, w0, b0, h0,
                                                  w1, b1, h1, out);
    });
    NRK_CHECK_LAUNCH();
    return NRK_OK;
}

int nrk_tt_user_pass_users(int dim, int h0) {
    clear_error();
    if (tt_check_shape(__func__, dim)) return 0;
    if (h0 < 1 || h0 > TT_H0_MAX) {
        fail_as(__func__, NRK_EINVAL, "h0 must be in [1, 128]");
        return 0;
    }
    return tt_pass_users(h0);
}

int nrk_tt_user_fwd_layers(const float* user_table, int64_t n_user_rows, const float* item_table,
                           int64_t n_item_rows, int dim, const int32_t* uid, const int32_t* hist,
                           const int32_t* hist_len, int64_t n, int seq_len, const float* weights, int n_layers,
                           const int* widths, float* out, nrk_stream_t stream) {
    clear_error();
    NRK_REQUIRE(n >= 0 && seq_len >= 1 && seq_len <= 64, "bad sizes (seq_len must be in [1, 64])");
    NRK_REQUIRE(n_user_rows > 0 && n_item_rows > 0, "empty embedding tables");
    TtLayers ly{};
    if (const int rc = tt_check_shape(__func__, dim, n_layers, widths, &ly)) return rc;
    if (n == 0) return NRK_OK;
    NRK_REQUIRE(user_table && item_table && uid && hist && hist_len && weights && out, "null pointer");
    hipStream_t s = as_stream(stream);
    const unsigned grid = grid_for(n, 4, 2048);
    tt_for_dim(dim, [&](auto dc) {
        tt_user_mlp_kernel<decltype(dc)::value><<<grid, 256, 0, s>>>(user_table, item_table, uid, hist, hist_len, n,
                                                                     seq_len, weights, ly, out);
    });
    NRK_CHECK_LAUNCH();
    return NRK_OK;
}

int nrk_tt_item_fwd(const float* item_table, int64_t n_item_rows, int dim, const int32_t* ids,
                    int64_t n, float* out, nrk_stream_t stream) {
    clear_error();
    NRK_REQUIRE(n >= 0 && n_item_rows > 0, "bad sizes");
    if (const int rc = tt_check_shape(__func__, dim)) return rc;
    if (n == 0) return NRK_OK;
    NRK_REQUIRE(item_table && ids && out, "null pointer");
    hipStream_t s = as_stream(stream);
    const unsigned grid = grid_for(n, 256, 4096);
    tt_for_dim(dim, [&](auto dc) { tt_item_kernel<decltype(dc)::value><<<grid, 256, 0, s>>>(item_table, ids, n, out); });
    NRK_CHECK_LAUNCH();
    return NRK_OK;
}

}  // extern "C"
