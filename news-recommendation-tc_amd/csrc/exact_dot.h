// exact_dot.h -- the exact score of the top-k paths (ip_topk.hip's refine and
// exact path, ip_query.hip): sequential fp64 sums of fp32 products in
// ascending d, then + 0.0.  A product of two fp32 values is exact in fp64, so
// FMA contraction cannot change a bit; only the order of the sums matters, and
// both forms below keep it.
#pragma once

#include "nrk_common.h"

namespace nrk {

__device__ __forceinline__ double exact_dot(const float* __restrict__ a, const float* __restrict__ b,
                                            int dim) {
    double s = 0.0;
    if ((dim & 31) == 0) {
        // 8 float4 of both rows in flight per step (a runtime-dim loop
        // otherwise waits on each row piece in turn); same sequential order
        const float4* a4 = reinterpret_cast<const float4*>(a);
        const float4* b4 = reinterpret_cast<const float4*>(b);
        for (int t0 = 0; t0 < dim / 4; t0 += 8) {
            float4 x[8], y[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                x[t] = a4[t0 + t];
                y[t] = b4[t0 + t];
            }
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                s += (double)x[t].x * (double)y[t].x;
                s += (double)x[t].y * (double)y[t].y;
                s += (double)x[t].z * (double)y[t].z;
                s += (double)x[t].w * (double)y[t].w;
            }
        }
    } else if ((dim & 3) == 0) {
        const float4* a4 = reinterpret_cast<const float4*>(a);
        const float4* b4 = reinterpret_cast<const float4*>(b);
        for (int t = 0; t < dim / 4; ++t) {
            const float4 x = a4[t], y = b4[t];
            s += (double)x.x * (double)y.x;
            s += (double)x.y * (double)y.y;
            s += (double)x.z * (double)y.z;
            s += (double)x.w * (double)y.w;
        }
    } else {
        for (int t = 0; t < dim; ++t) s += (double)a[t] * (double)b[t];
    }
    return s + 0.0;
}

// exact_dot of one fp32 row against NQ user rows at once: acc[q] =
// exact_dot(row, user q) for q < nq (nq is uniform over the workgroup; the
// other acc stay 0).  The user rows are fp64 copies in LDS, ud[q * ustride +
// t] (the conversion is exact), read as broadcasts; the row is loaded once, 8
// float4 per step, and reused for every user.  The same three forms: float4
// steps of 32 while they fit and single float4 after them when dim % 4 == 0,
// scalars otherwise -- each acc[q] is summed in ascending t all the same.
template <int NQ>
__device__ __forceinline__ void exact_dot_tile(const float* __restrict__ row, const double* ud, int ustride,
                                               int dim, int nq, double (&acc)[NQ]) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    if ((dim & 3) == 0) {
        const float4* r4 = reinterpret_cast<const float4*>(row);
        int t = 0;
        for (; t + 32 <= dim; t += 32) {
            float4 x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = r4[t / 4 + j];
            double xd[32];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                xd[4 * j] = (double)x[j].x;
                xd[4 * j + 1] = (double)x[j].y;
                xd[4 * j + 2] = (double)x[j].z;
                xd[4 * j + 3] = (double)x[j].w;
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                if (q < nq) {
                    const double* uq = ud + q * ustride + t;
#pragma unroll
                    for (int e = 0; e < 32; ++e) acc[q] += xd[e] * uq[e];
                }
            }
        }
        for (; t < dim; t += 4) {
            const float4 x = r4[t / 4];
            const double x0 = (double)x.x, x1 = (double)x.y, x2 = (double)x.z, x3 = (double)x.w;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                if (q < nq) {
                    const double* uq = ud + q * ustride + t;
                    acc[q] += x0 * uq[0];
                    acc[q] += x1 * uq[1];
                    acc[q] += x2 * uq[2];
                    acc[q] += x3 * uq[3];
                }
            }
        }
    } else {
        for (int t = 0; t < dim; ++t) {
            const double x0 = (double)row[t];
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (q < nq) acc[q] += x0 * ud[q * ustride + t];
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] += 0.0;
}

}  // namespace nrk
