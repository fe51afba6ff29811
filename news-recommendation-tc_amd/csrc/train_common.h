// train_common.h -- the exact-Adam update and its sweep over packed weights
// and embedding tables, shared by the two trainers (tower_train.hip,
// din_train.hip).  Not for din.hip or ip_topk.hip: those are compiled with
// -fno-honor-nans.
#pragma once

#include <cmath>

#include "nrk_common.h"

namespace nrk {

// torch/optim/adam.py _single_tensor_adam, fp32 element by element:
//   m.lerp_(g, 1 - beta1)            fma(w, g - m, m)
//   v.mul_(beta2).addcmul_(g, g, 1 - beta2)
//                                    fma((1 - beta2) g, g, beta2 v)
//   denom = sqrt(v) / sqrt(bc2) + eps
//   p.addcdiv_(m, denom, -lr / bc1)  p + (value m) / denom
// The two fused multiply-adds are where torch's CPU kernels fuse (lerp's
// vec::fmadd, addcmul's contracted self + value t1 t2: found by replaying
// the step in numpy against torch.optim.Adam); contraction is off
// so that nothing else is fused.
struct AdamK {
    float w1, beta2, w2, bc2_sqrt, eps, neg_step;
};
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float g, const AdamK& k) {
#pragma clang fp contract(off)
    m = __fmaf_rn(k.w1, g - m, m);
    v = __fmaf_rn(k.w2 * g, g, v * k.beta2);
    const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
    p = p + (k.neg_step * m) / denom;
}

// One table of n_rows x D and its gradient as a compact list: *count
// ascending rows and [count, D] values.
struct AdamSeg {
    float *p, *m, *v;
    const int32_t* rows;
    const float* vals;
    const int32_t* count;
    int64_t n_rows;
};
template <int NSEG>
struct AdamSegs {
    AdamSeg s[NSEG];
};

// Blocks [0, wblocks): the packed weights, one element per thread, dense g.
// Then segment 0's blocks0 blocks, then (NSEG = 2) segment 1's: one float4
// per thread; the row's gradient is found by binary search in the compact
// list (absent: g = 0, still updated: dense semantics; with m = v = 0 as
// well the row is left untouched).  NSEG is a template parameter because a
// one-table sweep handed an empty second segment measured 0.3-0.5 us of 50
// slower over DIN's 513k rows than the instantiation without one (three
// alternating pairs, B = 256 and 4096): every wave loads the second segment
// too and branches on a block count that is never reached.
template <int D, int NSEG>
__global__ __launch_bounds__(256) void adam_sweep_kernel(float* __restrict__ w, float* __restrict__ w_m,
                                                         float* __restrict__ w_v, const float* __restrict__ w_g,
                                                         int64_t n_w, int wblocks, AdamSegs<NSEG> segs,
                                                         int64_t blocks0, AdamK k) {
    constexpr int Q = D / 4, QL = Q == 4 ? 2 : Q == 8 ? 3 : 4;  // float4s per row: a shift and a mask
    static_assert(D == 16 || D == 32 || D == 64, "adam_sweep_kernel: D in {16, 32, 64}");
    static_assert(NSEG == 1 || NSEG == 2, "adam_sweep_kernel: one or two tables");
    int64_t blk = blockIdx.x;
    if (blk < wblocks) {
        const int64_t e = blk * 256 + threadIdx.x;
        if (e < n_w) {
            float p = w[e], m = w_m[e], v = w_v[e];
            adam_update(p, m, v, w_g[e], k);
            w[e] = p;
            w_m[e] = m;
            w_v[e] = v;
        }
        return;
    }
    blk -= wblocks;
    AdamSeg sg = segs.s[0];
    if constexpr (NSEG == 2) {
        if (blk >= blocks0) {
            sg = segs.s[1];
            blk -= blocks0;
        }
    }
    const int64_t e4 = blk * 256 + threadIdx.x;  // float4 index
    const int64_t row = e4 >> QL;
    if (row >= sg.n_rows) return;
    int lo = 0, hi = *sg.count;
    const int n = hi;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sg.rows[mid] < row) lo = mid + 1;
        else hi = mid;
    }
    const bool has = lo < n && sg.rows[lo] == row;
    float4 m = reinterpret_cast<float4*>(sg.m)[e4], v = reinterpret_cast<float4*>(sg.v)[e4];
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (has) g = reinterpret_cast<const float4*>(sg.vals)[(int64_t)lo * Q + (e4 & (Q - 1))];
    else if (m.x == 0.0f && m.y == 0.0f && m.z == 0.0f && m.w == 0.0f && v.x == 0.0f && v.y == 0.0f &&
             v.z == 0.0f && v.w == 0.0f)
        return;  // m = v = g = 0: the update changes nothing
    float4 p = reinterpret_cast<float4*>(sg.p)[e4];
    // p's load is issued before the arithmetic on m and v.  Left to itself the scheduler sank it 80
    // instructions into the one-table instantiation, 35 before its use: DIN's sweep at B = 4096, where
    // most rows move, took 69.7 us against 66.6 us with the barrier
    __builtin_amdgcn_sched_barrier(0);
    adam_update(p.x, m.x, v.x, g.x, k);
    adam_update(p.y, m.y, v.y, g.y, k);
    adam_update(p.z, m.z, v.z, g.z, k);
    adam_update(p.w, m.w, v.w, g.w, k);
    reinterpret_cast<float4*>(sg.p)[e4] = p;
    reinterpret_cast<float4*>(sg.m)[e4] = m;
    reinterpret_cast<float4*>(sg.v)[e4] = v;
}

// The step number and hyper-parameter checks of both *_adam_step entry points
// (fn names the caller in the error), and the scalars as _single_tensor_adam
// forms them: in double, then one rounding to fp32.
static inline int adam_scalars(const char* fn, double lr, double beta1, double beta2, double eps, int64_t t, AdamK* k) {
    if (!(t >= 1)) return fail_as(fn, NRK_EINVAL, "t is the 1-based step number");
    if (!(lr > 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0))
        return fail_as(fn, NRK_EINVAL, "bad hyper-parameters");
    const double bc1 = 1.0 - std::pow(beta1, (double)t), bc2 = 1.0 - std::pow(beta2, (double)t);
    *k = AdamK{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)std::sqrt(bc2), (float)eps,
               (float)(-(lr / bc1))};
    return NRK_OK;
}

// One launch over the weights and the NSEG tables.
template <int D, int NSEG>
static int adam_sweep(const char* fn, float* w, float* w_m, float* w_v, const float* w_g, int64_t n_w,
                      const AdamSegs<NSEG>& segs, const AdamK& k, hipStream_t st) {
    const int wblocks = (int)((n_w + 255) / 256);
    int64_t blocks0 = 0, blocks = wblocks;
    for (int i = 0; i < NSEG; ++i) {
        const int64_t b = (segs.s[i].n_rows * (D / 4) + 255) / 256;
        if (i == 0) blocks0 = b;
        blocks += b;
    }
    if (!(blocks < ((int64_t)1 << 31))) return fail_as(fn, NRK_EINVAL, "tables too large for one sweep");
    adam_sweep_kernel<D, NSEG><<<(unsigned)blocks, 256, 0, st>>>(w, w_m, w_v, w_g, n_w, wblocks, segs, blocks0, k);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? NRK_OK : fail_as(fn, NRK_EHIP, hipGetErrorString(e));
}

}  // namespace nrk
