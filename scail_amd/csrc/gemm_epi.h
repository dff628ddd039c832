// Shared by the bf16 (gemm.hip) and fp8 (gemm_fp8.hip) GEMM kernels: the parameter block and the fused epilogue
// y = epi(acc + bias) with SCAIL_EPI_BIAS / _GELU_TANH / _GELU_ERF / _RESID (gated or not, resid may alias y).
#pragma once
#include "common.h"

struct GemmParams {
    const u16* x; int64_t lda;
    const u16* w;
    const float* bias;
    u16* y; int64_t ldc;
    int M, N, K;
    const u16* resid; int64_t ldr;
    const float* gate; int64_t gate_stride; int64_t rows_per_batch;
    int group_m;   // m-tiles per tile group of the block -> tile map (q8 kernel; others use GROUP_M)
};

// Fused epilogue of the bf16 and fp8 kernels.  A lane holds output column m (= row of x) and, per 32x32
// accumulator fragment, rows n = nbase + 8 rr + 4 g + e.  All loads of one pass (bias once; residual and
// gate per output row) are issued before their first use: one memory round trip per pass.
template <int EPI, int MI, int NI, int WTM, int WTN>
__device__ __forceinline__ void gemm_epilogue(f32x16 (&acc)[NI][MI], const GemmParams& p, int m0, int n0, int wm, int wn,
                                              int l31, int g) {
    float4 bb[NI][4];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int n = n0 + wn * WTN + ni * 32 + 8 * rr + 4 * g;
            bb[ni][rr] = (p.bias != nullptr && n < p.N) ? *reinterpret_cast<const float4*>(p.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int m = m0 + wm * WTM + mi * 32 + l31;
        if (m >= p.M) continue;
        uint2 rv[NI][4];
        float4 gt[NI][4];
        if (EPI == SCAIL_EPI_RESID) {
            const int64_t bidx = (p.gate != nullptr) ? (int64_t)m / p.rows_per_batch : 0;
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int n = n0 + wn * WTN + ni * 32 + 8 * rr + 4 * g;
                    const bool ok = n < p.N;
                    rv[ni][rr] = ok ? *reinterpret_cast<const uint2*>(p.resid + (int64_t)m * p.ldr + n) : make_uint2(0, 0);
                    gt[ni][rr] = (ok && p.gate != nullptr) ? *reinterpret_cast<const float4*>(p.gate + bidx * p.gate_stride + n)
                                                           : make_float4(1.f, 1.f, 1.f, 1.f);
                }
        }
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int n = n0 + wn * WTN + ni * 32 + 8 * rr + 4 * g;
                if (n >= p.N) continue;
                float v[4];
                v[0] = acc[ni][mi][4 * rr + 0] + bb[ni][rr].x;
                v[1] = acc[ni][mi][4 * rr + 1] + bb[ni][rr].y;
                v[2] = acc[ni][mi][4 * rr + 2] + bb[ni][rr].z;
                v[3] = acc[ni][mi][4 * rr + 3] + bb[ni][rr].w;
                if (EPI == SCAIL_EPI_GELU_TANH) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = gelu_tanh_f(v[e]);
                } else if (EPI == SCAIL_EPI_GELU_ERF) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = gelu_erf_f(v[e]);
                } else if (EPI == SCAIL_EPI_RESID) {
                    v[0] = bf_lo(rv[ni][rr].x) + gt[ni][rr].x * v[0];
                    v[1] = bf_hi(rv[ni][rr].x) + gt[ni][rr].y * v[1];
                    v[2] = bf_lo(rv[ni][rr].y) + gt[ni][rr].z * v[2];
                    v[3] = bf_hi(rv[ni][rr].y) + gt[ni][rr].w * v[3];
                }
                uint2 o;
                o.x = pack_bf16x2(v[0], v[1]);
                o.y = pack_bf16x2(v[2], v[3]);
                *reinterpret_cast<uint2*>(p.y + (int64_t)m * p.ldc + n) = o;
            }
        }
    }
}
