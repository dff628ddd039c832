// Row-wise / elementwise kernels of the SCAIL DiT hot path (all HBM-bound): fused
// LayerNorm+modulate, affine LayerNorm, full-width RMSNorm (+3D RoPE), V transpose staging,
// timestep embedding, tiny linears, AdaLN tables, patchify / unpatchify, CFG+Euler.
// One 256-thread workgroup per row for the norm kernels; every bf16 access is a 16-byte vector.
#include "common.h"
#include <algorithm>
#include <atomic>
#include <cstring>

#define ROW_THREADS 256
#define ROW_MAXV 3  // D <= 256 * 8 * 3 = 6144 kept in registers

// ------------------------------------------------------------------------------------------------
// LayerNorm (+ modulate | + affine)
// ------------------------------------------------------------------------------------------------
template <int MODE>  // 0: modulate (shift/scale per batch), 1: affine (w, b)
__global__ __launch_bounds__(ROW_THREADS) void ln_kernel(
    const u16* __restrict__ x, int64_t ldx, u16* __restrict__ y, int64_t ldy,
    const float* __restrict__ p0, const float* __restrict__ p1, int64_t mod_stride,
    int64_t rows_out, int64_t src_rows_per_batch, int64_t src_row_offset, int D, float eps) {
    __shared__ float red[4];
    const int64_t r = blockIdx.x;
    const int64_t b = r / rows_out;
    const int64_t i = r - b * rows_out;
    const u16* xr = x + (b * src_rows_per_batch + src_row_offset + i) * ldx;
    u16* yr = y + r * ldy;
    const int nvec = D >> 3;
    float v[ROW_MAXV][8];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < ROW_MAXV; ++j) {
        const int c = threadIdx.x + j * ROW_THREADS;
        if (c < nvec) {
            uint4 u = *reinterpret_cast<const uint4*>(xr + (int64_t)c * 8);
            unpack8(u, v[j]);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += v[j][e];
        }
    }
    const float mean = block_sum_256(s, red) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < ROW_MAXV; ++j) {
        const int c = threadIdx.x + j * ROW_THREADS;
        if (c < nvec) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = v[j][e] - mean;
                q += d * d;
            }
        }
    }
    const float var = block_sum_256(q, red) / (float)D;
    const float rstd = rsqrtf(var + eps);
    const float* a0 = (MODE == 0) ? p0 + b * mod_stride : p0;  // shift | weight
    const float* a1 = (MODE == 0) ? p1 + b * mod_stride : p1;  // scale | bias
#pragma unroll
    for (int j = 0; j < ROW_MAXV; ++j) {
        const int c = threadIdx.x + j * ROW_THREADS;
        if (c < nvec) {
            float o[8];
            const float4 s0 = *reinterpret_cast<const float4*>(a0 + c * 8);
            const float4 s1 = *reinterpret_cast<const float4*>(a0 + c * 8 + 4);
            const float4 t0 = *reinterpret_cast<const float4*>(a1 + c * 8);
            const float4 t1 = *reinterpret_cast<const float4*>(a1 + c * 8 + 4);
            const float A0[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
            const float A1[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float n = (v[j][e] - mean) * rstd;
                o[e] = (MODE == 0) ? n * (1.0f + A1[e]) + A0[e] : n * A0[e] + A1[e];
            }
            *reinterpret_cast<uint4*>(yr + (int64_t)c * 8) = pack8(o);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// RMSNorm over D (+ optional interleaved RoPE with per-token pair tables)
// ------------------------------------------------------------------------------------------------
// Output layout: row-major (row stride ldy, slab_w == 0), or COLUMN SLABS (slab_w > 0): the D columns are cut into D / slab_w
// slabs, slab g holds a (rows, slab_w) matrix with row stride ldy (>= slab_w) at y + g * slab_stride -- the send layout of the Ulysses
// head <-> sequence all-to-all (scail_amd/parallel.py: one slab per destination rank; ldy = 3 * slab_w puts q | k | v side by side in
// ONE message per destination), written by the norm itself instead of a pack pass.
// w == nullptr: no normalisation / RoPE / scale, a plain copy into the chosen layout (the V third of the exchange).
__global__ __launch_bounds__(ROW_THREADS) void rmsnorm_rope_kernel(
    const u16* __restrict__ x, int64_t ldx, u16* __restrict__ y, int64_t ldy,
    const float* __restrict__ w, const float* __restrict__ cos_tab, const float* __restrict__ sin_tab,
    int64_t rows_per_batch, int D, int head_dim, float eps, float out_scale, int slab_w, int64_t slab_stride) {
    __shared__ float red[4];
    const int64_t r = blockIdx.x;
    const u16* xr = x + r * ldx;
    u16* yr = y + r * ldy;
    const int nvec = D >> 3;
    auto dst = [&](int c) -> u16* {                      // 16-byte chunk c of this row in the output layout
        if (slab_w == 0) return yr + (int64_t)c * 8;
        const int col = c * 8, gsl = col / slab_w;
        return y + (int64_t)gsl * slab_stride + r * ldy + (col - gsl * slab_w);
    };
    if (w == nullptr) {
        for (int c = threadIdx.x; c < nvec; c += ROW_THREADS)
            *reinterpret_cast<uint4*>(dst(c)) = *reinterpret_cast<const uint4*>(xr + (int64_t)c * 8);
        return;
    }
    float v[ROW_MAXV][8];
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < ROW_MAXV; ++j) {
        const int c = threadIdx.x + j * ROW_THREADS;
        if (c < nvec) {
            uint4 u = *reinterpret_cast<const uint4*>(xr + (int64_t)c * 8);
            unpack8(u, v[j]);
#pragma unroll
            for (int e = 0; e < 8; ++e) q += v[j][e] * v[j][e];
        }
    }
    const float var = block_sum_256(q, red) / (float)D;
    const float rstd = rsqrtf(var + eps);
    const int half = head_dim >> 1;
    const int64_t tok = r % rows_per_batch;
#pragma unroll
    for (int j = 0; j < ROW_MAXV; ++j) {
        const int c = threadIdx.x + j * ROW_THREADS;
        if (c < nvec) {
            float n[8], o[8];
            const float4 w0 = *reinterpret_cast<const float4*>(w + c * 8);
            const float4 w1 = *reinterpret_cast<const float4*>(w + c * 8 + 4);
            const float W[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) n[e] = W[e] * (v[j][e] * rstd);
            if (cos_tab != nullptr) {
                // columns c*8 .. c*8+7 lie in one head; pair index inside the head:
                const int p0 = ((c * 8) % head_dim) >> 1;
                const float4 cs = *reinterpret_cast<const float4*>(cos_tab + tok * half + p0);
                const float4 sn = *reinterpret_cast<const float4*>(sin_tab + tok * half + p0);
                const float C[4] = {cs.x, cs.y, cs.z, cs.w};
                const float S[4] = {sn.x, sn.y, sn.z, sn.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // out[2i] = x[2i] cos - x[2i+1] sin ; out[2i+1] = x[2i+1] cos + x[2i] sin
                    o[2 * e] = n[2 * e] * C[e] - n[2 * e + 1] * S[e];
                    o[2 * e + 1] = n[2 * e + 1] * C[e] + n[2 * e] * S[e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = n[e];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] *= out_scale;       // 1.0f (exact) unless the caller folds a scale into the row
            *reinterpret_cast<uint4*>(dst(c)) = pack8(o);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// ONE WAVE PER ROW forms of the two norm kernels (round 4): D = 512 * CPL columns, lane l holds the 16-byte chunks l, l + 64, ... of its
// row (each wave-instruction moves 1 KB of contiguous bytes), all CPL loads in flight before the first use, wave-level reductions only
// (no LDS, no barrier), four independent rows per 256-thread workgroup.  Same arithmetic as the block kernels above up to the order of
// the fp32 sums.  The block kernels had every thread wait at two (LayerNorm: four) barriers per row and left the third pass half empty
// at D = 5120 (640 chunks on 256 threads): 4.3 TB/s; see DESIGN.md section 4.3 for the measured A/B.
// ------------------------------------------------------------------------------------------------
template <int MODE, int CPL>
__global__ __launch_bounds__(256) void ln_wave_kernel(
    const u16* __restrict__ x, int64_t ldx, u16* __restrict__ y, int64_t ldy,
    const float* __restrict__ p0, const float* __restrict__ p1, int64_t mod_stride,
    int64_t rows_out, int64_t src_rows_per_batch, int64_t src_row_offset, int wgs_per_batch, float eps) {
    constexpr int D = 512 * CPL;
    // the row parameters of this workgroup's batch element in LDS: [D] multiplier (1 + scale | weight), [D] addend (shift | bias).  From
    // global memory they are 8 bytes per element against the 2 + 2 of x and y (40 KB per row through L2 at D = 5120).
    extern __shared__ __attribute__((aligned(16))) float prm[];
    const int64_t b = blockIdx.x / wgs_per_batch;
    const int g = blockIdx.x - (int)b * wgs_per_batch;
    {
        const float* a0 = (MODE == 0) ? p0 + b * mod_stride : p0;  // shift | weight
        const float* a1 = (MODE == 0) ? p1 + b * mod_stride : p1;  // scale | bias
        for (int i4 = threadIdx.x; i4 < D / 4; i4 += 256) {
            float4 m = *reinterpret_cast<const float4*>((MODE == 0 ? a1 : a0) + i4 * 4);
            const float4 ad = *reinterpret_cast<const float4*>((MODE == 0 ? a0 : a1) + i4 * 4);
            if (MODE == 0) { m.x += 1.0f; m.y += 1.0f; m.z += 1.0f; m.w += 1.0f; }
            *reinterpret_cast<float4*>(prm + i4 * 4) = m;
            *reinterpret_cast<float4*>(prm + D + i4 * 4) = ad;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)g * 4 + (threadIdx.x >> 6); i < rows_out; i += (int64_t)wgs_per_batch * 4) {
        const u16* xr = x + (b * src_rows_per_batch + src_row_offset + i) * ldx;
        u16* yr = y + (b * rows_out + i) * ldy;
        uint4 u[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) u[j] = *reinterpret_cast<const uint4*>(xr + (j * 64 + lane) * 8);
        float v[CPL][8];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            unpack8(u[j], v[j]);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += v[j][e];
        }
        const float mean = wave_sum(s) * (1.0f / (float)D);
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < CPL; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = v[j][e] - mean;
                q += d * d;
            }
        const float rstd = rsqrtf(wave_sum(q) * (1.0f / (float)D) + eps);
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int c = j * 64 + lane;
            const float4 m0 = *reinterpret_cast<const float4*>(prm + c * 8);
            const float4 m1 = *reinterpret_cast<const float4*>(prm + c * 8 + 4);
            const float4 t0 = *reinterpret_cast<const float4*>(prm + D + c * 8);
            const float4 t1 = *reinterpret_cast<const float4*>(prm + D + c * 8 + 4);
            const float Mu[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
            const float Ad[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (v[j][e] - mean) * rstd * Mu[e] + Ad[e];
            *reinterpret_cast<uint4*>(yr + c * 8) = pack8(o);
        }
    }
}

template <int CPL, bool HD128>
__global__ __launch_bounds__(256) void rmsnorm_rope_wave_kernel(
    const u16* __restrict__ x, int64_t ldx, u16* __restrict__ y, int64_t ldy,
    const float* __restrict__ w, const float* __restrict__ cos_tab, const float* __restrict__ sin_tab,
    int64_t rows, int64_t rows_per_batch, int head_dim, float eps, float out_scale, int slab_w, int64_t slab_stride) {
    constexpr int D = 512 * CPL;
    extern __shared__ __attribute__((aligned(16))) float prm[];       // the norm weight as given: [D] (out_scale multiplies each result element below)
    for (int i4 = threadIdx.x; i4 < D / 4; i4 += 256) *reinterpret_cast<float4*>(prm + i4 * 4) = *reinterpret_cast<const float4*>(w + i4 * 4);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int half = head_dim >> 1;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
        const u16* xr = x + r * ldx;
        u16* yr = y + r * ldy;
        uint4 u[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) u[j] = *reinterpret_cast<const uint4*>(xr + (j * 64 + lane) * 8);
        // head_dim == 128: chunk j * 64 + lane starts at column (lane % 16) * 8 of its head for every j, so the lane's four (cos, sin)
        // pairs are the same for all its chunks: two 16-byte loads per row, requested with the row itself (the block kernel asks for them
        // per chunk, after the reduction: 20 loads per lane at D = 5120)
        const int64_t tok = r % rows_per_batch;
        float4 cs1 = make_float4(0.f, 0.f, 0.f, 0.f), sn1 = cs1;
        if (HD128 && cos_tab != nullptr) {
            cs1 = *reinterpret_cast<const float4*>(cos_tab + tok * 64 + (lane & 15) * 4);
            sn1 = *reinterpret_cast<const float4*>(sin_tab + tok * 64 + (lane & 15) * 4);
        }
        float v[CPL][8];
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            unpack8(u[j], v[j]);
#pragma unroll
            for (int e = 0; e < 8; ++e) q += v[j][e] * v[j][e];
        }
        const float rstd = rsqrtf(wave_sum(q) * (1.0f / (float)D) + eps);
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int c = j * 64 + lane;
            float n[8], o[8];
            const float4 w0 = *reinterpret_cast<const float4*>(prm + c * 8);
            const float4 w1 = *reinterpret_cast<const float4*>(prm + c * 8 + 4);
            const float W[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) n[e] = W[e] * (v[j][e] * rstd);
            if (cos_tab != nullptr) {
                float4 cs = cs1, sn = sn1;
                if (!HD128) {
                    const int p0 = ((c * 8) % head_dim) >> 1;
                    cs = *reinterpret_cast<const float4*>(cos_tab + tok * half + p0);
                    sn = *reinterpret_cast<const float4*>(sin_tab + tok * half + p0);
                }
                const float C[4] = {cs.x, cs.y, cs.z, cs.w};
                const float S[4] = {sn.x, sn.y, sn.z, sn.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[2 * e] = n[2 * e] * C[e] - n[2 * e + 1] * S[e];
                    o[2 * e + 1] = n[2 * e + 1] * C[e] + n[2 * e] * S[e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = n[e];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] *= out_scale;
            u16* dst;
            if (slab_w == 0) {
                dst = yr + c * 8;
            } else {
                const int col = c * 8, gsl = col / slab_w;
                dst = y + (int64_t)gsl * slab_stride + r * ldy + (col - gsl * slab_w);
            }
            *reinterpret_cast<uint4*>(dst) = pack8(o);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// V -> V^T staging (64 keys x head_dim tile through LDS)
// ------------------------------------------------------------------------------------------------
#define TV_KEYS 64
__global__ __launch_bounds__(256) void transpose_v_kernel(
    const u16* __restrict__ v, int64_t ldv, int64_t v_bs, u16* __restrict__ vt, int heads,
    int head_dim, int64_t Lk, int64_t Lkp) {
    extern __shared__ __attribute__((aligned(16))) u16 tile[];  // [64][head_dim + 8]
    const int ldt = head_dim + 8;
    const int64_t key0 = (int64_t)blockIdx.x * TV_KEYS;
    const int h = blockIdx.y;
    const int64_t b = blockIdx.z;
    const int cpr = head_dim >> 3;  // 16-byte chunks per row
    const u16* src = v + b * v_bs + (int64_t)h * head_dim;
    for (int c = threadIdx.x; c < TV_KEYS * cpr; c += 256) {
        const int kr = c / cpr, cc = c - kr * cpr;
        uint4 u = make_uint4(0, 0, 0, 0);
        if (key0 + kr < Lk) u = *reinterpret_cast<const uint4*>(src + (key0 + kr) * ldv + cc * 8);
        *reinterpret_cast<uint4*>(tile + kr * ldt + cc * 8) = u;
    }
    __syncthreads();
    u16* dst = vt + ((b * heads + h) * (int64_t)head_dim) * Lkp + key0;
    for (int o = threadIdx.x; o < head_dim * (TV_KEYS / 8); o += 256) {
        const int d = o >> 3, ch = o & 7;
        u16 e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int p = ch * 8 + j;  // position inside the 64-key tile
            const int key = (p & ~12) | (((p >> 3) & 1) << 2) | (((p >> 2) & 1) << 3);  // swap bits 2,3
            e[j] = tile[key * ldt + d];
        }
        uint4 u;
        u.x = e[0] | ((uint32_t)e[1] << 16);
        u.y = e[2] | ((uint32_t)e[3] << 16);
        u.z = e[4] | ((uint32_t)e[5] << 16);
        u.w = e[6] | ((uint32_t)e[7] << 16);
        *reinterpret_cast<uint4*>(dst + (int64_t)d * Lkp + ch * 8) = u;
    }
}

// ------------------------------------------------------------------------------------------------
// small stuff
// ------------------------------------------------------------------------------------------------
__global__ void timestep_embedding_kernel(const float* __restrict__ t, float* __restrict__ out, int dim) {
    const int b = blockIdx.x;
    const int half = dim >> 1;
    for (int j = threadIdx.x; j < half; j += blockDim.x) {
        const double f = exp(-log(10000.0) * (double)j / (double)half);
        const double a = (double)t[b] * f;
        out[(int64_t)b * dim + j] = (float)cos(a);
        out[(int64_t)b * dim + half + j] = (float)sin(a);
    }
    if ((dim & 1) && threadIdx.x == 0) out[(int64_t)b * dim + dim - 1] = 0.f;
}

__device__ __forceinline__ float act_f(float x, int a) {
    return a == 1 ? silu_f(x) : (a == 2 ? gelu_tanh_f(x) : x);
}

#define SL_MAXM 8
// one wave per output column n; lanes stride over K in 8-element chunks
__global__ __launch_bounds__(256) void small_linear_kernel(
    const float* __restrict__ x, const u16* __restrict__ w, const float* __restrict__ bias,
    float* __restrict__ y, int M, int N, int K, int act_in, int act_out) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (n >= N) return;
    float acc[SL_MAXM];
#pragma unroll
    for (int m = 0; m < SL_MAXM; ++m) acc[m] = 0.f;
    const u16* wr = w + (int64_t)n * K;
    for (int k = lane * 8; k < K; k += 64 * 8) {
        float wf[8];
        unpack8(*reinterpret_cast<const uint4*>(wr + k), wf);
#pragma unroll
        for (int m = 0; m < SL_MAXM; ++m) {
            if (m < M) {
                const float4 x0 = *reinterpret_cast<const float4*>(x + (int64_t)m * K + k);
                const float4 x1 = *reinterpret_cast<const float4*>(x + (int64_t)m * K + k + 4);
                const float X[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[m] += act_f(X[e], act_in) * wf[e];
            }
        }
    }
#pragma unroll
    for (int m = 0; m < SL_MAXM; ++m) {
        if (m < M) {
            const float s = wave_sum(acc[m]);
            if (lane == 0) y[(int64_t)m * N + n] = act_f(s + (bias ? bias[n] : 0.f), act_out);
        }
    }
}

__global__ void adaln_table_kernel(const float* __restrict__ emb, const float* __restrict__ table,
                                   float* __restrict__ out, int64_t n_batch, int64_t width, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t j = i % width;
    const int64_t b = (i / width) % n_batch;
    const int64_t l = i / (width * n_batch);
    out[i] = emb[b * width + j] + table[l * width + j];
}

// one thread per (token, 8-column chunk) of the im2col matrix
__global__ void patchify_kernel(const float* __restrict__ x, const u16* __restrict__ ref,
                                const u16* __restrict__ pose, u16* __restrict__ tok, int64_t n_batch,
                                int64_t n_ref, int64_t n_pose, int T, int H, int W, int kpad, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cpr = kpad >> 3;
    const int ch = (int)(i % cpr);
    const int64_t row = i / cpr;
    const int h2 = H >> 1, w2 = W >> 1, h4 = H >> 2, w4 = W >> 2;
    const int64_t Lref = (int64_t)h2 * w2, Lnoise = (int64_t)T * h2 * w2, Lpose = (int64_t)T * h4 * w4;
    const int64_t L = Lref + Lnoise + Lpose;
    const int64_t b = row / L;
    int64_t l = row - b * L;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = ch * 8 + e;
        float val = 0.f;
        if (k < 80) {
            const int c = k >> 2, p = (k >> 1) & 1, q = k & 1;
            if (l < Lref) {
                const int hh = (int)(l / w2), ww = (int)(l % w2);
                if (c >= 16) val = 1.f;
                else {
                    const int64_t bb = (n_ref == 1) ? 0 : b;
                    val = bf2f(ref[((bb * 16 + c) * H + (2 * hh + p)) * W + 2 * ww + q]);
                }
            } else if (l < Lref + Lnoise) {
                const int64_t ll = l - Lref;
                const int t = (int)(ll / (h2 * w2));
                const int rem = (int)(ll % (h2 * w2));
                const int hh = rem / w2, ww = rem % w2;
                if (c >= 16) val = 0.f;
                else val = bf2f(f2bf(x[(((b * T + t) * 16 + c) * H + (2 * hh + p)) * W + 2 * ww + q]));
            } else {
                const int64_t ll = l - Lref - Lnoise;
                const int t = (int)(ll / (h4 * w4));
                const int rem = (int)(ll % (h4 * w4));
                const int hh = rem / w4, ww = rem % w4;
                if (c >= 16) val = 1.f;
                else {
                    const int64_t bb = (n_pose == 1) ? 0 : b;
                    val = bf2f(pose[(((bb * T + t) * 16 + c) * h2 + (2 * hh + p)) * w2 + 2 * ww + q]);
                }
            }
        }
        o[e] = val;
    }
    *reinterpret_cast<uint4*>(tok + row * kpad + ch * 8) = pack8(o);
}

// Multi-character token assembly: the whole im2col matrix [ref_0..ref_{C-1} | noise | pose_0..pose_{C-1}] in one launch.
// One thread per (token, 8-column chunk), chunks of a token on consecutive lanes: a wave stores 1 KiB of contiguous destination rows
// (16 bytes per lane), the larger of the two streams.  A chunk is two channels x the 2x2 patch; its four (channel, patch row) pairs
// are contiguous in the source and are read as one 4-byte (bf16) / 8-byte (fp32) access each, lanes 16 apart (the next token of a
// character's plane) continuing the same source line.  Chunks 8 and 9 are the constant mask channels, the rest of kpad is zero:
// neither reads anything.  Every source element is read once; with n_char == 1 the result is patchify_kernel's.
__global__ void patchify_chars_kernel(const float* __restrict__ x, const u16* __restrict__ ref, const u16* __restrict__ pose,
                                      u16* __restrict__ tok, int64_t n_ref, int64_t n_pose, int n_char, int T, int H, int W, int kpad,
                                      int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cpr = kpad >> 3;
    const int ch = (int)(i % cpr);
    const int64_t row = i / cpr;
    const int h2 = H >> 1, w2 = W >> 1, h4 = H >> 2, w4 = W >> 2;
    const int64_t Lref1 = (int64_t)h2 * w2, Lnoise = (int64_t)T * h2 * w2, Lpose1 = (int64_t)T * h4 * w4;
    const int64_t Lref = n_char * Lref1, L = Lref + Lnoise + n_char * Lpose1;
    const int64_t b = row / L;
    const int64_t l = row - b * L;
    const bool noise = l >= Lref && l < Lref + Lnoise;
    float o[8];
    if (ch >= 8) {                  // mask channels 16..19 (1 on ref / pose tokens, 0 on noise tokens), then the zero padding
        const float m = (ch < 10 && !noise) ? 1.f : 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = m;
    } else if (noise) {
        const int64_t ll = l - Lref;
        const int t = (int)(ll / Lref1), rem = (int)(ll % Lref1);
        const int hh = rem / w2, ww = rem % w2;
        const float* src = x + (((b * T + t) * 16 + 2 * ch) * H + 2 * hh) * W + 2 * ww;
#pragma unroll
        for (int e = 0; e < 4; ++e) {       // e = (channel, patch row)
            const float2 v = *reinterpret_cast<const float2*>(src + ((int64_t)(e >> 1) * H + (e & 1)) * W);
            o[2 * e] = v.x;
            o[2 * e + 1] = v.y;
        }
    } else {
        const u16* src;
        int64_t plane, line;                // elements between two channels / two patch rows
        if (l < Lref) {
            const int k = (int)(l / Lref1), rem = (int)(l % Lref1);
            const int hh = rem / w2, ww = rem % w2;
            const int64_t bb = (n_ref == 1) ? 0 : b;
            plane = (int64_t)H * W, line = W;
            src = ref + (((bb * n_char + k) * 16 + 2 * ch) * H + 2 * hh) * W + 2 * ww;
        } else {
            const int64_t ll = l - Lref - Lnoise;
            const int k = (int)(ll / Lpose1);
            const int64_t rem1 = ll % Lpose1;
            const int t = (int)(rem1 / (h4 * w4)), rem = (int)(rem1 % (h4 * w4));
            const int hh = rem / w4, ww = rem % w4;
            const int64_t bb = (n_pose == 1) ? 0 : b;
            plane = (int64_t)h2 * w2, line = w2;
            src = pose + ((((bb * n_char + k) * T + t) * 16 + 2 * ch) * h2 + 2 * hh) * w2 + 2 * ww;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(src + (e >> 1) * plane + (e & 1) * line);
            o[2 * e] = bf_lo(v);
            o[2 * e + 1] = bf_hi(v);
        }
    }
    *reinterpret_cast<uint4*>(tok + row * kpad + ch * 8) = pack8(o);
}

// out[b][t][c][2h+p][2w+q] = tok[b][(t,h,w)][p*32 + q*16 + c]
__global__ void unpatchify_kernel(const u16* __restrict__ tok, float* __restrict__ out, int T, int H,
                                  int W, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ww = (int)(i % W);
    const int hh = (int)((i / W) % H);
    const int c = (int)((i / ((int64_t)W * H)) % 16);
    const int t = (int)((i / ((int64_t)W * H * 16)) % T);
    const int64_t b = i / ((int64_t)W * H * 16 * T);
    const int h2 = H >> 1, w2 = W >> 1;
    const int64_t row = (b * T + t) * (int64_t)(h2 * w2) + (int64_t)(hh >> 1) * w2 + (ww >> 1);
    out[i] = bf2f(tok[row * 64 + (hh & 1) * 32 + (ww & 1) * 16 + c]);
}

__global__ void cfg_euler_kernel(float* __restrict__ x, const float* __restrict__ v, int64_t n,
                                 float cfg, float dsigma) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float vu = v[i], vc = v[n + i];
    x[i] = x[i] + dsigma * (vu + cfg * (vc - vu));
}

// ---- temporal tiling (RFSamplerLong, sampling.py:986-1085; include/scail_hip.h scail_tile_*) ----
// A latent frame is F = 16 * H * W floats.  The frame indices / weights of one tile travel BY VALUE in the kernel arguments (no
// host-to-device copy, no synchronisation: the launches stay capturable); blockIdx.y is the tile frame, so the index is wave-uniform.
// Every operation is rounded on its own (contraction off): each kernel gives the bits of the torch expression it replaces, unlike
// cfg_euler_kernel above, whose multiply-adds contract.
#define TILE_MAX 64
struct TileArgs {
    int32_t f[TILE_MAX];   // frame index of tile frame j (gather / blend); unused by the finish kernel
    float w[TILE_MAX];     // blend: m_k * tile_weight[j];  finish: 1 / weight_sum of frame f0 + j
};

// xin[j, :] = xin[Tt + j, :] = x[f_j, :]   (torch.cat([x[:, idx]] * 2): the CFG batch)
__global__ void tile_gather_kernel(const float* __restrict__ x, float* __restrict__ xin, TileArgs a, int64_t Tt, int64_t F) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= F) return;
    const int64_t j = blockIdx.y;
    const float v = x[(int64_t)a.f[j] * F + e];
    xin[j * F + e] = v;
    xin[(Tt + j) * F + e] = v;
}

// den[f_j, e] += wk_j * (vu + cfg * (vc - vu)),  v = [v_u; v_c] fp32 [2, Tt, F]; the f_j of one tile are distinct (checked on the host)
__global__ void tile_blend_acc_kernel(float* __restrict__ den, const float* __restrict__ v, TileArgs a, int64_t Tt, int64_t F, float cfg) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= F) return;
    const int64_t j = blockIdx.y;
    const float vu = v[j * F + e], vc = v[(Tt + j) * F + e];
    const float d = vu + cfg * (vc - vu);
    const int64_t o = (int64_t)a.f[j] * F + e;
    den[o] = den[o] + a.w[j] * d;
}

// x[f0 + j, e] += dsigma * (den[f0 + j, e] * inv_j);  den[f0 + j, e] = 0 (ready for the next step's accumulation)
__global__ void tile_finish_kernel(float* __restrict__ x, float* __restrict__ den, TileArgs a, int64_t f0, int64_t F, float dsigma) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= F) return;
    const int64_t j = blockIdx.y;
    const int64_t o = (f0 + j) * F + e;
    x[o] = x[o] + dsigma * (den[o] * a.w[j]);
    den[o] = 0.0f;
}

// ---- guidance plan (include/scail_dit.h "guidance plan"; include/scail_hip.h scail_cfg_delta_*) ----
// Every operation is rounded on its own (contraction off), like the tile kernels above: each kernel gives the bits of the torch fp32
// expression it stands for.
// delta[i] = v_c[i] - v_u[i],  v = [v_u; v_c] fp32 [2, n]
__global__ void cfg_delta_store_kernel(const float* __restrict__ v, float* __restrict__ delta, int64_t n) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    delta[i] = v[n + i] - v[i];
}
// x[i] = x[i] + dsigma * (v_c[i] + g * delta[i])   (delta == nullptr: x[i] = x[i] + dsigma * v_c[i])
__global__ void cfg_euler_delta_kernel(float* __restrict__ x, const float* __restrict__ vc, const float* __restrict__ delta, int64_t n, float g,
                                       float dsigma) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float d = vc[i];
    if (delta != nullptr) {
        const float gd = g * delta[i];
        d = d + gd;
    }
    const float step = dsigma * d;
    x[i] = x[i] + step;
}

// ---- solver plan (include/scail_dit.h "solver plan"; include/scail_hip.h scail_cfg_multistep / scail_tile_finish_multistep) ----
// One element of a multistep update x <- a x + b D + c D_prev around the data prediction D = x - sigma d, every operation rounded on
// its own.  use_prev == 0: `hist` is not read (the caller has not loaded it either); it leaves as D.
__device__ __forceinline__ void multistep_elem(float& x, float& hist, float d, float sigma, float a, float b, float c, int use_prev) {
#pragma clang fp contract(off)
    const float sd = sigma * d;
    const float D = x - sd;
    const float ax = a * x;
    const float bD = b * D;
    float y = ax + bD;
    if (use_prev) {
        const float ch = c * hist;
        y = y + ch;
    }
    x = y;
    hist = D;
}
__device__ __forceinline__ float cfg_combine(float vu, float vc, float cfg) {
#pragma clang fp contract(off)
    const float diff = vc - vu;
    const float g = cfg * diff;
    return vu + g;
}
// v = [v_u; v_c] fp32 [2, n].  vec: x, v and hist are 16-byte aligned -- thread t takes elements 4t .. 4t + 3 of the first n & ~3 with
// 16-byte accesses (v_c = v + n is 16-byte aligned only where n % 4 == 0; elsewhere its four values are loaded one by one), and the
// first n & 3 threads take one element of the tail each.  Not vec: one element per thread.
__global__ void cfg_multistep_kernel(float* __restrict__ x, const float* __restrict__ v, float* __restrict__ hist, int64_t n, float cfg,
                                     float sigma, float a, float b, float c, int use_prev, int vec) {
#pragma clang fp contract(off)
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n4 = vec ? n >> 2 : 0;
    if (t < n4) {
        const int64_t i = 4 * t;
        float4 xv = *reinterpret_cast<const float4*>(x + i);
        const float4 vu = *reinterpret_cast<const float4*>(v + i);
        float4 vc;
        if ((n & 3) == 0) {
            vc = *reinterpret_cast<const float4*>(v + n + i);
        } else {
            vc = make_float4(v[n + i], v[n + i + 1], v[n + i + 2], v[n + i + 3]);
        }
        float4 hv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (use_prev) hv = *reinterpret_cast<const float4*>(hist + i);
        multistep_elem(xv.x, hv.x, cfg_combine(vu.x, vc.x, cfg), sigma, a, b, c, use_prev);
        multistep_elem(xv.y, hv.y, cfg_combine(vu.y, vc.y, cfg), sigma, a, b, c, use_prev);
        multistep_elem(xv.z, hv.z, cfg_combine(vu.z, vc.z, cfg), sigma, a, b, c, use_prev);
        multistep_elem(xv.w, hv.w, cfg_combine(vu.w, vc.w, cfg), sigma, a, b, c, use_prev);
        *reinterpret_cast<float4*>(x + i) = xv;
        *reinterpret_cast<float4*>(hist + i) = hv;
    }
    const int64_t i = 4 * n4 + t;      // the tail (vec), or every element
    if (i < n) {
        float xs = x[i], hs = 0.0f;
        if (use_prev) hs = hist[i];
        multistep_elem(xs, hs, cfg_combine(v[i], v[n + i], cfg), sigma, a, b, c, use_prev);
        x[i] = xs;
        hist[i] = hs;
    }
}
// The tiled loop's finishing pass under a solver plan: tile_finish_kernel's d = den * inv_j, then the multistep update; den is left
// zeroed.  vec: F % 4 == 0 and x, den and hist are 16-byte aligned, so every frame is -- thread e takes elements 4e .. 4e + 3 of frame
// f0 + j; a frame size that is no multiple of 4 takes the scalar form throughout (its frames do not start on 16 bytes).
__global__ void tile_finish_multistep_kernel(float* __restrict__ x, float* __restrict__ den, float* __restrict__ hist, TileArgs w, int64_t f0,
                                             int64_t F, float sigma, float a, float b, float c, int use_prev, int vec) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t j = blockIdx.y;
    const float inv = w.w[j];
    if (vec) {
        if (4 * e >= F) return;
        const int64_t o = (f0 + j) * F + 4 * e;
        float4 xv = *reinterpret_cast<const float4*>(x + o);
        const float4 dn = *reinterpret_cast<const float4*>(den + o);
        float4 hv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (use_prev) hv = *reinterpret_cast<const float4*>(hist + o);
        multistep_elem(xv.x, hv.x, dn.x * inv, sigma, a, b, c, use_prev);
        multistep_elem(xv.y, hv.y, dn.y * inv, sigma, a, b, c, use_prev);
        multistep_elem(xv.z, hv.z, dn.z * inv, sigma, a, b, c, use_prev);
        multistep_elem(xv.w, hv.w, dn.w * inv, sigma, a, b, c, use_prev);
        *reinterpret_cast<float4*>(x + o) = xv;
        *reinterpret_cast<float4*>(hist + o) = hv;
        *reinterpret_cast<float4*>(den + o) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    if (e >= F) return;
    const int64_t o = (f0 + j) * F + e;
    float xs = x[o], hs = 0.0f;
    if (use_prev) hs = hist[o];
    multistep_elem(xs, hs, den[o] * inv, sigma, a, b, c, use_prev);
    x[o] = xs;
    hist[o] = hs;
    den[o] = 0.0f;
}

__global__ void zero_f32_kernel(float* __restrict__ y, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = 0.0f;
}

__global__ void f32_to_bf16_kernel(const float* __restrict__ x, u16* __restrict__ y, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = f2bf(x[i]);
}
__global__ void bf16_to_f32_kernel(const u16* __restrict__ x, float* __restrict__ y, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = bf2f(x[i]);
}

// ================================================================================================
// C ABI
// ================================================================================================
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// option "row_wave" (scail_set_option): 1 (default) = the one-wave-per-row norm kernels where D is 1536 / 2048 / 4096 / 5120 / 6144,
// 0 = the block-per-row kernels for every D (same-process A/B; the results agree up to the order of the fp32 sums)
static std::atomic<int> g_row_wave{1};   // option state: atomic (set by one thread, read by every launching thread)
int scail_row_wave_enable(int on) { g_row_wave = on != 0; return 0; }

// ------------------------------------------------------------------------------------------------
// Which kernel a LayerNorm / RMSNorm (+ RoPE) call runs.  row_choose is the ONE statement of it: ln_launch and rmsnorm_rope_launch launch
// what it says, and the host-side query scail_row_kernel_name_for is a projection of the same answer.  Nothing else reads option "row_wave".
// ------------------------------------------------------------------------------------------------
struct RowChoice {
    bool wave = false;           // one wave per row (ln_wave_kernel / rmsnorm_rope_wave_kernel) instead of one workgroup per row
    int cpl = 0;                 // wave form: 16-byte chunks per lane, D = 512 * cpl
    bool hd128 = false;          // RMSNorm + RoPE wave form: head_dim == 128, the lane's (cos, sin) pairs loaded once per row
    int64_t wgs_per_batch = 0;   // LayerNorm wave form: workgroups dealt to one batch element
    int64_t grid = 0;            // workgroups; -1: the wave form's grid was asked for and the device's CU count is not available
};

// form: SCAIL_ROW_*; rows = n_batch * rows_out (the RMSNorm forms have no batch split: only the product counts).  want_grid == false
// answers the kernel alone, which needs no device; the grid of a wave form is sized by the device's compute units.
static RowChoice row_choose(int form, int64_t n_batch, int64_t rows_out, int64_t D, int64_t head_dim, bool want_grid) {
    RowChoice c;
    const int64_t rows = n_batch * rows_out;
    c.grid = rows;                                     // the block kernels: one workgroup per row
    const bool ln = form == SCAIL_ROW_LN_MODULATE || form == SCAIL_ROW_LN_AFFINE;
    // LayerNorm: the wave form wherever it covers D.  RMSNorm: with RoPE the wave form wins (0.455 -> 0.41 ms at config 2: the (cos, sin) pairs
    // once per row instead of per chunk); without, the block kernel is already at the pass's plateau (0.367 against 0.383 ms;
    // profiles/r04_row_pass_probe.log)
    if (!g_row_wave || D % 512 != 0 || rows <= 0 || !(ln || form == SCAIL_ROW_RMSNORM_ROPE)) return c;
    const int cpl = (int)(D / 512);
    if (cpl != 3 && cpl != 4 && cpl != 8 && cpl != 10 && cpl != 12) return c;       // the instantiations
    c.wave = true;
    c.cpl = cpl;
    c.hd128 = !ln && head_dim == 128;
    c.grid = 0;
    if (!want_grid) return c;
    const int cus = scail_device_cus();
    if (cus <= 0) { c.grid = -1; return c; }
    if (ln) {
        // persistent workgroups: about three per compute unit (157 VGPRs, 40 KB of LDS), dealt evenly to the batch elements
        c.wgs_per_batch = std::max<int64_t>(1, std::min<int64_t>((rows_out + 3) / 4, (3 * cus + n_batch - 1) / n_batch));
        c.grid = n_batch * c.wgs_per_batch;
    } else {
        c.grid = std::max<int64_t>(1, std::min<int64_t>((rows + 3) / 4, 3 * (int64_t)cus));
    }
    return c;
}

// The choice in words: the kernel's template name with the arguments of the instantiation
static std::string row_choice_name(int form, const RowChoice& c) {
    const bool ln = form == SCAIL_ROW_LN_MODULATE || form == SCAIL_ROW_LN_AFFINE;
    const std::string mode = form == SCAIL_ROW_LN_MODULATE ? "0" : "1";
    if (!c.wave) return ln ? "ln_kernel<" + mode + ">" : "rmsnorm_rope_kernel";
    if (ln) return "ln_wave_kernel<" + mode + ", " + std::to_string(c.cpl) + ">";
    return "rmsnorm_rope_wave_kernel<" + std::to_string(c.cpl) + (c.hd128 ? ", true>" : ", false>");
}

extern "C" int scail_row_kernel_name_for(int form, int64_t n_batch, int64_t rows_out, int64_t D, int64_t head_dim, char* buf, int64_t len,
                                         int64_t* workgroups) {
    SCAIL_REQUIRE(buf != nullptr, "null argument");
    SCAIL_REQUIRE(form >= SCAIL_ROW_LN_MODULATE && form <= SCAIL_ROW_COPY, "unknown form");
    SCAIL_REQUIRE(D > 0 && D % 8 == 0 && D <= ROW_THREADS * 8 * ROW_MAXV, "D must be a multiple of 8 and <= 6144");
    SCAIL_REQUIRE(n_batch >= 0 && rows_out >= 0, "negative row count");
    SCAIL_REQUIRE(form < SCAIL_ROW_RMSNORM || (head_dim > 0 && head_dim % 8 == 0 && D % head_dim == 0), "head_dim must be a multiple of 8 dividing D");
    const RowChoice c = row_choose(form, n_batch, rows_out, D, head_dim, workgroups != nullptr);
    if (c.grid < 0) return 2;                           // (scail_device_cus left the message)
    const std::string name = row_choice_name(form, c);
    SCAIL_REQUIRE((int64_t)name.size() < len, "buffer too small");
    std::memcpy(buf, name.c_str(), name.size() + 1);
    if (workgroups != nullptr) *workgroups = c.grid;
    return 0;
}

template <int MODE>
static int ln_launch(const scail_bf16* x, int64_t ldx, scail_bf16* y, int64_t ldy, const float* p0, const float* p1, int64_t mod_stride,
                     int64_t n_batch, int64_t rows_out, int64_t src_rows_per_batch, int64_t src_row_offset, int64_t D, float eps, void* stream) {
    const RowChoice c = row_choose(MODE == 0 ? SCAIL_ROW_LN_MODULATE : SCAIL_ROW_LN_AFFINE, n_batch, rows_out, D, 0, true);
    if (c.grid < 0) return 2;
    if (!c.wave) {
        hipLaunchKernelGGL(ln_kernel<MODE>, dim3((unsigned)c.grid), dim3(ROW_THREADS), 0, (hipStream_t)stream, x, ldx, y, ldy, p0, p1, mod_stride,
                           rows_out, src_rows_per_batch, src_row_offset, (int)D, eps);
        return scail_check_launch(MODE == 0 ? "ln_modulate" : "layernorm_affine");
    }
#define LN_WAVE(CPL_)                                                                                                                  \
    case CPL_:                                                                                                                         \
        return scail_launch_lds<ln_wave_kernel<MODE, CPL_>>("ln_wave", 2 * 512 * CPL_ * 4, dim3((unsigned)c.grid), dim3(256), 2 * 512 * CPL_ * 4, stream, \
                                                            x, ldx, y, ldy, p0, p1, mod_stride, rows_out, src_rows_per_batch, src_row_offset, (int)c.wgs_per_batch, eps);
    switch (c.cpl) {
        LN_WAVE(3) LN_WAVE(4) LN_WAVE(8) LN_WAVE(10) LN_WAVE(12)
        default: break;
    }
#undef LN_WAVE
    scail_set_error("layernorm: no wave kernel for the choice " + row_choice_name(MODE == 0 ? SCAIL_ROW_LN_MODULATE : SCAIL_ROW_LN_AFFINE, c));
    return 2;
}

extern "C" int scail_ln_modulate(const scail_bf16* x, int64_t ldx, scail_bf16* y, int64_t ldy,
                                 const float* shift, const float* scale, int64_t mod_stride,
                                 int64_t n_batch, int64_t rows_out, int64_t src_rows_per_batch,
                                 int64_t src_row_offset, int64_t D, float eps, void* stream) {
    SCAIL_REQUIRE(D % 8 == 0 && D <= ROW_THREADS * 8 * ROW_MAXV, "D must be a multiple of 8 and <= 6144");
    SCAIL_REQUIRE(ldx % 8 == 0 && ldy % 8 == 0 && mod_stride % 4 == 0, "strides must keep 16-byte alignment");
    SCAIL_REQUIRE(aligned16(x) && aligned16(y) && aligned16(shift) && aligned16(scale), "pointers must be 16-byte aligned");
    const int64_t rows = n_batch * rows_out;
    if (rows == 0) return 0;
    return ln_launch<0>(x, ldx, y, ldy, shift, scale, mod_stride, n_batch, rows_out, src_rows_per_batch, src_row_offset, D, eps, stream);
}

extern "C" int scail_layernorm_affine(const scail_bf16* x, int64_t ldx, scail_bf16* y, int64_t ldy,
                                      const float* w, const float* b, int64_t rows, int64_t D, float eps,
                                      void* stream) {
    SCAIL_REQUIRE(D % 8 == 0 && D <= ROW_THREADS * 8 * ROW_MAXV, "D must be a multiple of 8 and <= 6144");
    SCAIL_REQUIRE(ldx % 8 == 0 && ldy % 8 == 0, "strides must keep 16-byte alignment");
    SCAIL_REQUIRE(aligned16(x) && aligned16(y) && aligned16(w) && aligned16(b), "pointers must be 16-byte aligned");
    if (rows == 0) return 0;
    return ln_launch<1>(x, ldx, y, ldy, w, b, 0, 1, rows, rows, 0, D, eps, stream);
}

extern "C" int scail_rmsnorm_rope(const scail_bf16* x, int64_t ldx, scail_bf16* y, int64_t ldy,
                                  const float* w, const float* cos_tab, const float* sin_tab,
                                  int64_t rows, int64_t rows_per_batch, int64_t D, int64_t head_dim,
                                  float eps, void* stream) {
    return scail_rmsnorm_rope_scaled(x, ldx, y, ldy, w, cos_tab, sin_tab, rows, rows_per_batch, D, head_dim, eps, 1.0f, stream);
}

static int rmsnorm_rope_launch(const scail_bf16* x, int64_t ldx, scail_bf16* y, int64_t ldy, const float* w, const float* cos_tab,
                               const float* sin_tab, int64_t rows, int64_t rows_per_batch, int64_t D, int64_t head_dim, float eps,
                               float out_scale, int64_t slab_w, int64_t slab_stride, void* stream) {
    SCAIL_REQUIRE(D % 8 == 0 && D <= ROW_THREADS * 8 * ROW_MAXV, "D must be a multiple of 8 and <= 6144");
    SCAIL_REQUIRE(head_dim % 8 == 0 && D % head_dim == 0, "head_dim must be a multiple of 8 dividing D");
    SCAIL_REQUIRE(ldx % 8 == 0 && ldy % 8 == 0, "strides must keep 16-byte alignment");
    SCAIL_REQUIRE((cos_tab == nullptr) == (sin_tab == nullptr), "cos and sin tables go together");
    SCAIL_REQUIRE(aligned16(x) && aligned16(y) && aligned16(w) && aligned16(cos_tab) && aligned16(sin_tab),
                  "pointers must be 16-byte aligned");
    SCAIL_REQUIRE(rows_per_batch > 0, "rows_per_batch must be positive");
    SCAIL_REQUIRE(slab_w == 0 || (slab_w % 8 == 0 && D % slab_w == 0 && ldy >= slab_w && slab_stride % 8 == 0 && slab_stride >= (rows - 1) * ldy + slab_w),
                  "slab width must be a multiple of 8 dividing D, slab row stride >= slab width, slab stride a multiple of 8 that holds rows of that stride");
    if (rows == 0) return 0;
    const int form = w == nullptr ? SCAIL_ROW_COPY : cos_tab != nullptr ? SCAIL_ROW_RMSNORM_ROPE : SCAIL_ROW_RMSNORM;
    const RowChoice c = row_choose(form, 1, rows, D, head_dim, true);
    if (c.grid < 0) return 2;
    if (c.wave) {
#define RR_WAVE(CPL_)                                                                                                                \
    case CPL_: {                                                                                                                     \
        constexpr int lds_ = 512 * CPL_ * 4;                                                                                         \
        if (c.hd128)                                                                                                                 \
            hipLaunchKernelGGL((rmsnorm_rope_wave_kernel<CPL_, true>), dim3((unsigned)c.grid), dim3(256), lds_, (hipStream_t)stream, x, ldx, y,  \
                               ldy, w, cos_tab, sin_tab, rows, rows_per_batch, (int)head_dim, eps, out_scale, (int)slab_w, slab_stride); \
        else                                                                                                                         \
            hipLaunchKernelGGL((rmsnorm_rope_wave_kernel<CPL_, false>), dim3((unsigned)c.grid), dim3(256), lds_, (hipStream_t)stream, x, ldx, y, \
                               ldy, w, cos_tab, sin_tab, rows, rows_per_batch, (int)head_dim, eps, out_scale, (int)slab_w, slab_stride); \
        return scail_check_launch("rmsnorm_rope");                                                                                   \
    }
        switch (c.cpl) {
            RR_WAVE(3) RR_WAVE(4) RR_WAVE(8) RR_WAVE(10) RR_WAVE(12)
            default: break;
        }
#undef RR_WAVE
        scail_set_error("rmsnorm_rope: no wave kernel for the choice " + row_choice_name(form, c));
        return 2;
    }
    hipLaunchKernelGGL(rmsnorm_rope_kernel, dim3((unsigned)c.grid), dim3(ROW_THREADS), 0, (hipStream_t)stream,
                       x, ldx, y, ldy, w, cos_tab, sin_tab, rows_per_batch, (int)D, (int)head_dim, eps, out_scale, (int)slab_w, slab_stride);
    return scail_check_launch("rmsnorm_rope");
}

extern "C" int scail_rmsnorm_rope_scaled(const scail_bf16* x, int64_t ldx, scail_bf16* y, int64_t ldy,
                                         const float* w, const float* cos_tab, const float* sin_tab,
                                         int64_t rows, int64_t rows_per_batch, int64_t D, int64_t head_dim,
                                         float eps, float out_scale, void* stream) {
    SCAIL_REQUIRE(w != nullptr, "null weight");
    return rmsnorm_rope_launch(x, ldx, y, ldy, w, cos_tab, sin_tab, rows, rows_per_batch, D, head_dim, eps, out_scale, 0, 0, stream);
}

extern "C" int scail_rmsnorm_rope_slabs(const scail_bf16* x, int64_t ldx, scail_bf16* y, int64_t slab_w, int64_t slab_ld, int64_t slab_stride,
                                        const float* w, const float* cos_tab, const float* sin_tab,
                                        int64_t rows, int64_t rows_per_batch, int64_t D, int64_t head_dim,
                                        float eps, float out_scale, void* stream) {
    SCAIL_REQUIRE(slab_w > 0, "slab width must be positive");
    SCAIL_REQUIRE(w != nullptr || (cos_tab == nullptr && sin_tab == nullptr), "a plain slab copy (w == NULL) takes no RoPE tables");
    return rmsnorm_rope_launch(x, ldx, y, slab_ld, w, cos_tab, sin_tab, rows, rows_per_batch, D, head_dim, eps, out_scale, slab_w, slab_stride, stream);
}

// slabs -> rows: the way back of the Ulysses exchange (the inverse layout of scail_rmsnorm_rope_slabs): slab g is a dense [rows, slab_w]
// matrix at x + g * slab_stride; row r of y gets slab g's row r at columns [g * slab_w, (g + 1) * slab_w).  One 16-byte chunk per thread,
// chunk index fastest along the OUTPUT row (whole-line stores; the loads of a slab row are contiguous too).
__global__ void slabs_to_rows_kernel(const u16* __restrict__ x, int64_t slab_stride, int slab_chunks, u16* __restrict__ y, int64_t ldy,
                                     int row_chunks, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t r = i / row_chunks;
    const int c = (int)(i - r * row_chunks);
    const int g = c / slab_chunks, j = c - g * slab_chunks;
    const uint4 v = *reinterpret_cast<const uint4*>(x + g * slab_stride + (r * slab_chunks + j) * 8);
    *reinterpret_cast<uint4*>(y + r * ldy + (int64_t)c * 8) = v;
}

extern "C" int scail_slabs_to_rows(const scail_bf16* x, int64_t slab_w, int64_t slab_stride, scail_bf16* y, int64_t ldy,
                                   int64_t rows, int64_t D, void* stream) {
    SCAIL_REQUIRE(slab_w > 0 && slab_w % 8 == 0 && D % slab_w == 0, "slab width must be a multiple of 8 that divides D");
    SCAIL_REQUIRE(ldy % 8 == 0 && slab_stride % 8 == 0 && slab_stride >= rows * slab_w && aligned16(x) && aligned16(y), "16-byte alignment / slab stride");
    const int64_t total = rows * (D / 8);
    if (total == 0) return 0;
    SCAIL_REQUIRE(total / 256 + 1 < (1ll << 31), "too many rows");
    hipLaunchKernelGGL(slabs_to_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, slab_stride,
                       (int)(slab_w / 8), y, ldy, (int)(D / 8), total);
    return scail_check_launch("slabs_to_rows");
}

extern "C" int scail_transpose_v(const scail_bf16* v, int64_t ldv, int64_t v_batch_stride,
                                 scail_bf16* vt, int64_t n_batch, int64_t heads, int64_t head_dim,
                                 int64_t Lk, void* stream) {
    SCAIL_REQUIRE(head_dim % 8 == 0 && head_dim <= 512, "head_dim must be a multiple of 8, <= 512");
    SCAIL_REQUIRE(ldv % 8 == 0 && v_batch_stride % 8 == 0 && aligned16(v) && aligned16(vt), "16-byte alignment");
    if (Lk == 0 || n_batch == 0) return 0;
    const int64_t Lkp = (Lk + 63) / 64 * 64;
    const size_t lds = (size_t)TV_KEYS * (head_dim + 8) * sizeof(u16);
    hipLaunchKernelGGL(transpose_v_kernel, dim3((unsigned)(Lkp / 64), (unsigned)heads, (unsigned)n_batch),
                       dim3(256), lds, (hipStream_t)stream, v, ldv, v_batch_stride, vt, (int)heads,
                       (int)head_dim, Lk, Lkp);
    return scail_check_launch("transpose_v");
}

extern "C" int scail_timestep_embedding(const float* t, float* out, int64_t n, int64_t dim, void* stream) {
    SCAIL_REQUIRE(dim >= 1 && dim < (1ll << 31) && n >= 0 && n < (1ll << 31), "need dim >= 1 and 0 <= n < 2^31 (one workgroup per timestep)");
    if (n == 0) return 0;
    SCAIL_REQUIRE(t != nullptr && out != nullptr, "null pointer");
    hipLaunchKernelGGL(timestep_embedding_kernel, dim3((unsigned)n), dim3(128), 0, (hipStream_t)stream, t, out,
                       (int)dim);
    return scail_check_launch("timestep_embedding");
}

extern "C" int scail_small_linear(const float* x, const scail_bf16* w, const float* b, float* y, int64_t M,
                                  int64_t N, int64_t K, int act_in, int act_out, void* stream) {
    SCAIL_REQUIRE(M >= 0 && M <= SL_MAXM, "M must be <= 8");
    SCAIL_REQUIRE(K % 8 == 0, "K must be a multiple of 8");
    SCAIL_REQUIRE(aligned16(x) && aligned16(w), "16-byte alignment");
    if (M == 0 || N == 0) return 0;
    hipLaunchKernelGGL(small_linear_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x,
                       w, b, y, (int)M, (int)N, (int)K, act_in, act_out);
    return scail_check_launch("small_linear");
}

extern "C" int scail_adaln_table(const float* emb, const float* table, float* out, int64_t n_layers,
                                 int64_t n_batch, int64_t width, void* stream) {
    SCAIL_REQUIRE(n_layers >= 0 && n_batch >= 0 && width >= 0 && n_layers < (1 << 20) && n_batch < (1 << 20) && width < (1 << 20), "sizes must be 0 .. 2^20 - 1");
    const int64_t total = n_layers * n_batch * width;
    if (total == 0) return 0;
    SCAIL_REQUIRE(emb != nullptr && table != nullptr && out != nullptr, "null pointer");
    SCAIL_REQUIRE((total + 255) / 256 < (1ll << 31), "table too large for one launch");
    hipLaunchKernelGGL(adaln_table_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, emb, table, out, n_batch, width, total);
    return scail_check_launch("adaln_table");
}

extern "C" int scail_patchify(const float* x, const scail_bf16* ref, const scail_bf16* pose,
                              scail_bf16* tok, int64_t n_batch, int64_t n_ref, int64_t n_pose, int64_t T,
                              int64_t H, int64_t W, int64_t kpad, void* stream) {
    SCAIL_REQUIRE(n_batch >= 0 && T >= 0 && H >= 0 && W >= 0 && n_batch < (1 << 15) && H < (1 << 15) && W < (1 << 15) && T < (1 << 15), "bad shape");
    SCAIL_REQUIRE(H % 4 == 0 && W % 4 == 0, "latent H and W must be multiples of 4 (pose is half size, patch 2)");
    SCAIL_REQUIRE(kpad >= 80 && kpad % 8 == 0 && kpad < (1 << 15), "kpad must be >= 80 and a multiple of 8");
    SCAIL_REQUIRE((n_ref == 1 || n_ref == n_batch) && (n_pose == 1 || n_pose == n_batch), "cond batch must be 1 or n_batch");
    const int64_t L = (1 + T) * (H / 2) * (W / 2) + T * (H / 4) * (W / 4);
    const int64_t total = n_batch * L * (kpad / 8);
    if (total == 0) return 0;
    SCAIL_REQUIRE(x != nullptr && ref != nullptr && pose != nullptr && tok != nullptr, "null pointer");
    // the kernel reads single elements and stores 16 bytes per thread
    SCAIL_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(ref) & 1) == 0 &&
                      (reinterpret_cast<uintptr_t>(pose) & 1) == 0 && (reinterpret_cast<uintptr_t>(tok) & 15) == 0,
                  "pointer alignment (x 4, ref / pose 2, tok 16 bytes)");
    SCAIL_REQUIRE((total + 255) / 256 < (1ll << 31), "token matrix too large for one launch");
    hipLaunchKernelGGL(patchify_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, x, ref, pose, tok, n_batch, n_ref, n_pose, (int)T, (int)H, (int)W,
                       (int)kpad, total);
    return scail_check_launch("patchify");
}

extern "C" int scail_patchify_chars(const float* x, const scail_bf16* ref, const scail_bf16* pose, scail_bf16* tok, int64_t n_batch,
                                    int64_t n_ref, int64_t n_pose, int64_t n_char, int64_t T, int64_t H, int64_t W, int64_t kpad,
                                    void* stream) {
    if (n_char < 1 || n_char > 64) {
        scail_set_error("scail_patchify_chars: n_char must be 1..64, got " + std::to_string(n_char));
        return 1;
    }
    SCAIL_REQUIRE(n_batch >= 0 && T >= 0 && H >= 0 && W >= 0 && H < (1 << 15) && W < (1 << 15) && T < (1 << 15), "bad shape");
    SCAIL_REQUIRE(H % 4 == 0 && W % 4 == 0, "latent H and W must be multiples of 4 (pose is half size, patch 2)");
    SCAIL_REQUIRE(kpad >= 80 && kpad % 8 == 0, "kpad must be >= 80 and a multiple of 8");
    SCAIL_REQUIRE((n_ref == 1 || n_ref == n_batch) && (n_pose == 1 || n_pose == n_batch), "cond batch must be 1 or n_batch");
    // the kernel reads pairs of neighbouring elements in one access and stores 16 bytes per thread
    SCAIL_REQUIRE((reinterpret_cast<uintptr_t>(x) & 7) == 0 && (reinterpret_cast<uintptr_t>(ref) & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(pose) & 3) == 0 && (reinterpret_cast<uintptr_t>(tok) & 15) == 0,
                  "pointer alignment (x 8, ref / pose 4, tok 16 bytes)");
    const int64_t L = (n_char + T) * (H / 2) * (W / 2) + n_char * T * (H / 4) * (W / 4);
    const int64_t total = n_batch * L * (kpad / 8);
    if (total == 0) return 0;
    SCAIL_REQUIRE((total + 255) / 256 < (1ll << 31), "token matrix too large for one launch");
    hipLaunchKernelGGL(patchify_chars_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ref, pose, tok,
                       n_ref, n_pose, (int)n_char, (int)T, (int)H, (int)W, (int)kpad, total);
    return scail_check_launch("patchify_chars");
}

extern "C" int scail_unpatchify(const scail_bf16* tok, float* out, int64_t n_batch, int64_t T, int64_t H,
                                int64_t W, void* stream) {
    SCAIL_REQUIRE(n_batch >= 0 && T >= 0 && H >= 0 && W >= 0 && n_batch < (1 << 15) && H < (1 << 15) && W < (1 << 15) && T < (1 << 15), "bad shape");
    SCAIL_REQUIRE(H % 2 == 0 && W % 2 == 0, "latent H and W must be even (patch 2)");
    const int64_t total = n_batch * T * 16 * H * W;
    if (total == 0) return 0;
    SCAIL_REQUIRE(tok != nullptr && out != nullptr, "null pointer");
    SCAIL_REQUIRE((total + 255) / 256 < (1ll << 31), "latent too large for one launch");
    hipLaunchKernelGGL(unpatchify_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, tok, out, (int)T, (int)H, (int)W, total);
    return scail_check_launch("unpatchify");
}

extern "C" int scail_cfg_euler(float* x, const float* v, int64_t n, float cfg_scale, float dsigma,
                               void* stream) {
    SCAIL_REQUIRE(n >= 0 && (n + 255) / 256 < (1ll << 31), "n must be 0 .. 2^39 - 256 (one launch)");
    if (n == 0) return 0;
    SCAIL_REQUIRE(x != nullptr && v != nullptr, "null pointer");
    hipLaunchKernelGGL(cfg_euler_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       x, v, n, cfg_scale, dsigma);
    return scail_check_launch("cfg_euler");
}

// ---- guidance plan: host-side checks (the message names the value) + launches ----
static int cfg_delta_n_check(const char* who, int64_t n) {
    if (n < 0 || (n + 255) / 256 >= (1ll << 31)) {
        scail_set_error(std::string(who) + ": n must be 0 .. 2^39 - 256 (one launch), got " + std::to_string(n));
        return 1;
    }
    return 0;
}
extern "C" int scail_cfg_delta_store(const float* v, float* delta, int64_t n, void* stream) {
    if (int rc = cfg_delta_n_check("scail_cfg_delta_store", n)) return rc;
    if (v == nullptr || delta == nullptr) {
        scail_set_error(std::string("scail_cfg_delta_store: null pointer: ") + (v == nullptr ? "v" : "delta") + " (n = " + std::to_string(n) + ")");
        return 1;
    }
    if (n == 0) return 0;
    hipLaunchKernelGGL(cfg_delta_store_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, v, delta, n);
    return scail_check_launch("cfg_delta_store");
}
extern "C" int scail_cfg_euler_delta(float* x, const float* v_c, const float* delta, int64_t n, float cfg_scale, float dsigma, void* stream) {
    if (int rc = cfg_delta_n_check("scail_cfg_euler_delta", n)) return rc;
    if (x == nullptr || v_c == nullptr) {
        scail_set_error(std::string("scail_cfg_euler_delta: null pointer: ") + (x == nullptr ? "x" : "v_c") + " (n = " + std::to_string(n) + ")");
        return 1;
    }
    if (n == 0) return 0;
    const float g = cfg_scale - 1.0f;      // formed once, in fp32
    hipLaunchKernelGGL(cfg_euler_delta_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, v_c, delta, n, g, dsigma);
    return scail_check_launch("cfg_euler_delta");
}

// ---- solver plan: host-side checks (the message names the value) + launches ----
extern "C" int scail_cfg_multistep(float* x, const float* v, float* hist, int64_t n, float cfg_scale, float sigma, float a, float b, float c,
                                   int use_prev, void* stream) {
    if (int rc = cfg_delta_n_check("scail_cfg_multistep", n)) return rc;
    if (n == 0) return 0;
    if (x == nullptr || v == nullptr || hist == nullptr) {
        scail_set_error(std::string("scail_cfg_multistep: null pointer: ") + (x == nullptr ? "x" : v == nullptr ? "v" : "hist") +
                        " (n = " + std::to_string(n) + ")");
        return 1;
    }
    const int vec = aligned16(x) && aligned16(v) && aligned16(hist);
    const int64_t n4 = vec ? n >> 2 : 0, tail = n - 4 * n4, threads = n4 > tail ? n4 : tail;
    hipLaunchKernelGGL(cfg_multistep_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, v, hist, n, cfg_scale,
                       sigma, a, b, c, use_prev != 0, vec);
    return scail_check_launch("cfg_multistep");
}

// ---- temporal tiling: host-side checks (the message names the value) + launches ----
// Tt in 1..min(T, 64), every frame index in [0, T) and, `unique`, no index twice (two tile frames would accumulate into one latent frame
// concurrently).  Shared with the sampler entry point (dit_step.hip), which checks every tile before anything is enqueued.
int scail_tile_len_check(const char* who, int64_t Tt, int64_t T) {
    if (T >= 1 && Tt >= 1 && Tt <= TILE_MAX && Tt <= T) return 0;
    if (who != nullptr)
        scail_set_error(std::string(who) + ": the tile length Tt must be 1..min(T, 64), got Tt = " + std::to_string(Tt) + " with T = " + std::to_string(T));
    return 1;
}
int scail_tile_check(const char* who, const int32_t* frames, int64_t Tt, int64_t T, bool unique) {
    if (int rc = scail_tile_len_check(who, Tt, T)) return rc;
    if (frames == nullptr) {
        scail_set_error(std::string(who) + ": null pointer: frames");
        return 1;
    }
    for (int64_t j = 0; j < Tt; ++j) {
        if (frames[j] < 0 || frames[j] >= T) {
            scail_set_error(std::string(who) + ": frame index " + std::to_string(frames[j]) + " (tile frame " + std::to_string(j) + ") is outside [0, T = " +
                            std::to_string(T) + ")");
            return 1;
        }
        for (int64_t i = 0; unique && i < j; ++i)
            if (frames[i] == frames[j]) {
                scail_set_error(std::string(who) + ": frame index " + std::to_string(frames[j]) + " is repeated inside one tile (tile frames " +
                                std::to_string(i) + " and " + std::to_string(j) + ")");
                return 1;
            }
    }
    return 0;
}

static int tile_shape_check(const char* who, int64_t F) {
    if (F < 0 || (F + 255) / 256 >= (1ll << 31)) {
        scail_set_error(std::string(who) + ": bad frame size F = " + std::to_string(F));
        return 1;
    }
    return 0;
}

extern "C" int scail_tile_gather(const float* x, float* xin, const int32_t* frames, int64_t Tt, int64_t T, int64_t F, void* stream) {
    if (int rc = scail_tile_check("scail_tile_gather", frames, Tt, T, false)) return rc;
    if (int rc = tile_shape_check("scail_tile_gather", F)) return rc;
    SCAIL_REQUIRE(x != nullptr && xin != nullptr, "null pointer");
    if (F == 0) return 0;
    TileArgs a = {};
    for (int64_t j = 0; j < Tt; ++j) a.f[j] = frames[j];
    hipLaunchKernelGGL(tile_gather_kernel, dim3((unsigned)((F + 255) / 256), (unsigned)Tt), dim3(256), 0, (hipStream_t)stream, x, xin, a, Tt, F);
    return scail_check_launch("tile_gather");
}

extern "C" int scail_tile_blend_acc(float* den, const float* v, const int32_t* frames, const float* wk, int64_t Tt, int64_t T, int64_t F,
                                    float cfg_scale, void* stream) {
    if (int rc = scail_tile_check("scail_tile_blend_acc", frames, Tt, T, true)) return rc;
    if (int rc = tile_shape_check("scail_tile_blend_acc", F)) return rc;
    SCAIL_REQUIRE(den != nullptr && v != nullptr && wk != nullptr, "null pointer");
    if (F == 0) return 0;
    TileArgs a = {};
    for (int64_t j = 0; j < Tt; ++j) {
        a.f[j] = frames[j];
        a.w[j] = wk[j];
    }
    hipLaunchKernelGGL(tile_blend_acc_kernel, dim3((unsigned)((F + 255) / 256), (unsigned)Tt), dim3(256), 0, (hipStream_t)stream, den, v, a, Tt, F,
                       cfg_scale);
    return scail_check_launch("tile_blend_acc");
}

// y[0 .. n) = 0 as a kernel launch.  Observation, cause not established: with one hipMemsetAsync in this place, the captured
// scail_dit_sample_tiled gave wrong results from its second graph replay on (eager runs and the first replay were right); with this
// kernel every replay is right.
int scail_zero_f32(float* y, int64_t n, void* stream) {
    if (n <= 0) return 0;
    SCAIL_REQUIRE(y != nullptr && (n + 255) / 256 < (1ll << 31), "null pointer / too large");
    hipLaunchKernelGGL(zero_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, n);
    return scail_check_launch("zero_f32");
}

extern "C" int scail_tile_finish(float* x, float* den, const float* inv_wsum, int64_t T, int64_t F, float dsigma, void* stream) {
    if (int rc = tile_shape_check("scail_tile_finish", F)) return rc;
    SCAIL_REQUIRE(T >= 0 && T < (1ll << 31), "bad frame count");
    SCAIL_REQUIRE(x != nullptr && den != nullptr && inv_wsum != nullptr, "null pointer");
    if (F == 0) return 0;
    for (int64_t f0 = 0; f0 < T; f0 += TILE_MAX) {      // 64 frames' factors per launch
        const int64_t n = T - f0 < TILE_MAX ? T - f0 : TILE_MAX;
        TileArgs a = {};
        for (int64_t j = 0; j < n; ++j) a.w[j] = inv_wsum[f0 + j];
        hipLaunchKernelGGL(tile_finish_kernel, dim3((unsigned)((F + 255) / 256), (unsigned)n), dim3(256), 0, (hipStream_t)stream, x, den, a, f0, F,
                           dsigma);
        if (int rc = scail_check_launch("tile_finish")) return rc;
    }
    return 0;
}

// scail_tile_finish under a solver plan: the same checks, launches and treatment of den / inv_wsum, the multistep update in its place
extern "C" int scail_tile_finish_multistep(float* x, float* den, const float* inv_wsum, float* hist, int64_t T, int64_t F, float sigma, float a,
                                           float b, float c, int use_prev, void* stream) {
    if (int rc = tile_shape_check("scail_tile_finish_multistep", F)) return rc;
    SCAIL_REQUIRE(T >= 0 && T < (1ll << 31), "bad frame count");
    SCAIL_REQUIRE(x != nullptr && den != nullptr && inv_wsum != nullptr && hist != nullptr, "null pointer");
    if (F == 0) return 0;
    const int vec = (F & 3) == 0 && aligned16(x) && aligned16(den) && aligned16(hist);
    const int64_t per_frame = vec ? F >> 2 : F;
    for (int64_t f0 = 0; f0 < T; f0 += TILE_MAX) {      // 64 frames' factors per launch
        const int64_t n = T - f0 < TILE_MAX ? T - f0 : TILE_MAX;
        TileArgs w = {};
        for (int64_t j = 0; j < n; ++j) w.w[j] = inv_wsum[f0 + j];
        hipLaunchKernelGGL(tile_finish_multistep_kernel, dim3((unsigned)((per_frame + 255) / 256), (unsigned)n), dim3(256), 0, (hipStream_t)stream,
                           x, den, hist, w, f0, F, sigma, a, b, c, use_prev != 0, vec);
        if (int rc = scail_check_launch("tile_finish_multistep")) return rc;
    }
    return 0;
}

extern "C" int scail_f32_to_bf16(const float* x, scail_bf16* y, int64_t n, void* stream) {
    SCAIL_REQUIRE(n >= 0 && (n + 255) / 256 < (1ll << 31), "n must be 0 .. 2^39 - 256 (one launch)");
    if (n == 0) return 0;
    SCAIL_REQUIRE(x != nullptr && y != nullptr, "null pointer");
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, x, y, n);
    return scail_check_launch("f32_to_bf16");
}
extern "C" int scail_bf16_to_f32(const scail_bf16* x, float* y, int64_t n, void* stream) {
    SCAIL_REQUIRE(n >= 0 && (n + 255) / 256 < (1ll << 31), "n must be 0 .. 2^39 - 256 (one launch)");
    if (n == 0) return 0;
    SCAIL_REQUIRE(x != nullptr && y != nullptr, "null pointer");
    hipLaunchKernelGGL(bf16_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, x, y, n);
    return scail_check_launch("bf16_to_f32");
}

// ================================================================================================
// Step cache (include/scail_hip.h scail_resid_store / scail_resid_apply / scail_abs_diff_sums; the executor's SCAIL_DIT_CACHE_* modes).
// The two residual kernels are streaming passes: one 16-byte load / store (8 bf16) per lane and operand, a grid capped at
// RESID_MAX_WGS workgroups with a grid-stride loop over the 8-column chunks.  Rows are D apart in every operand, so the rows of one
// batch element are one contiguous run of rows * D elements and a chunk index needs no division by D.
// ================================================================================================
constexpr int RESID_MAX_WGS = 2048;     // 256 CUs x 8 workgroups

// r[b, c] = bf16(float(hout[b, c]) - float(hin[b, c])): chunk c of element b; hin's batch stride may be 0
__global__ __launch_bounds__(256) void resid_store_kernel(const u16* __restrict__ hout, int64_t out_bs, const u16* __restrict__ hin, int64_t in_bs,
                                                          u16* __restrict__ r, int64_t per_b8, int64_t total8) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total8; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / per_b8, c = i - b * per_b8;
        float fo[8], fi[8];
        unpack8(*reinterpret_cast<const uint4*>(hout + b * out_bs + c * 8), fo);
        unpack8(*reinterpret_cast<const uint4*>(hin + b * in_bs + c * 8), fi);
#pragma unroll
        for (int e = 0; e < 8; ++e) fo[e] = fo[e] - fi[e];
        *reinterpret_cast<uint4*>(r + i * 8) = pack8(fo);
    }
}

// h[b, c] = bf16(float(hin[b, c]) + float(r[b, c])).  ONE thread owns chunk c of EVERY element: it reads hin[b, c] before it writes
// h[b, c] (in_bs == 0: hin[c] once, before its first write), and no other thread touches chunk c of any element -- so h may be hin.
// (no __restrict__ on h / hin: they may alias)
__global__ __launch_bounds__(256) void resid_apply_kernel(const u16* hin, int64_t in_bs, const u16* __restrict__ r, u16* h, int64_t h_bs,
                                                          int64_t n_batch, int64_t per_b8) {
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < per_b8; c += (int64_t)gridDim.x * 256) {
        float fi[8], fr[8], fo[8];
        for (int64_t b = 0; b < n_batch; ++b) {
            if (b == 0 || in_bs != 0) unpack8(*reinterpret_cast<const uint4*>(hin + b * in_bs + c * 8), fi);
            unpack8(*reinterpret_cast<const uint4*>(r + (b * per_b8 + c) * 8), fr);
#pragma unroll
            for (int e = 0; e < 8; ++e) fo[e] = fi[e] + fr[e];
            *reinterpret_cast<uint4*>(h + b * h_bs + c * 8) = pack8(fo);
        }
    }
}

// out[0] = sum_j |a_j - b_j|, out[1] = sum_j |b_j|, every a_j and b_j widened to fp64 first.  ONE workgroup: thread t sums the terms
// j = t, t + 256, .. in ascending order, then a binary tree over the 256 partial sums in LDS -- an order fixed by n alone.
__global__ __launch_bounds__(256) void abs_diff_sums_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                                            double* __restrict__ out) {
    __shared__ double sd[256], sb[256];
    const int t = threadIdx.x;
    double d = 0.0, m = 0.0;
    for (int64_t j = t; j < n; j += 256) {
        const double bj = (double)b[j];
        d += fabs((double)a[j] - bj);
        m += fabs(bj);
    }
    sd[t] = d;
    sb[t] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            sd[t] += sd[t + s];
            sb[t] += sb[t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        out[0] = sd[0];
        out[1] = sb[0];
    }
}

// what the two residual calls share: shapes, strides, alignment (host only; the message names the value)
static int resid_check(const char* who, int64_t n_batch, int64_t rows, int64_t D, int64_t bs0, const char* bs0_name, int64_t bs1,
                       const char* bs1_name, const void* p0, const void* p1, const void* p2) {
    auto fail = [&](const std::string& msg) {
        scail_set_error(std::string(who) + ": " + msg);
        return 1;
    };
    if (n_batch < 0 || n_batch > 64) return fail("n_batch must be 0..64, got " + std::to_string(n_batch));
    if (rows < 0 || rows >= (1ll << 31)) return fail("rows must be 0 .. 2^31 - 1, got " + std::to_string(rows));
    if (D < 8 || D % 8 != 0 || D >= (1 << 20)) return fail("D must be a multiple of 8 in 8 .. 2^20 - 8 (16-byte loads), got " + std::to_string(D));
    if (bs0 < 0 || bs0 % 8 != 0) return fail(std::string(bs0_name) + " must be a non-negative multiple of 8 elements, got " + std::to_string(bs0));
    if (bs1 < 0 || bs1 % 8 != 0) return fail(std::string(bs1_name) + " must be a non-negative multiple of 8 elements, got " + std::to_string(bs1));
    if (n_batch == 0 || rows == 0) return 0;
    if (p0 == nullptr || p1 == nullptr || p2 == nullptr) return fail("null pointer");
    if (!aligned16(p0) || !aligned16(p1) || !aligned16(p2)) return fail("every base pointer must be 16-byte aligned");
    return 0;
}

extern "C" int scail_resid_store(const scail_bf16* h_out, int64_t out_bs, const scail_bf16* h_in, int64_t in_bs, scail_bf16* r,
                                 int64_t n_batch, int64_t rows, int64_t D, void* stream) {
    if (int rc = resid_check("scail_resid_store", n_batch, rows, D, out_bs, "out_bs", in_bs, "in_bs", h_out, h_in, r)) return rc;
    if (n_batch == 0 || rows == 0) return 0;
    const int64_t per_b8 = rows * (D / 8), total8 = n_batch * per_b8;
    const int64_t wgs = std::min<int64_t>((total8 + 255) / 256, RESID_MAX_WGS);
    hipLaunchKernelGGL(resid_store_kernel, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, h_out, out_bs, h_in, in_bs, r, per_b8, total8);
    return scail_check_launch("resid_store");
}

extern "C" int scail_resid_apply(const scail_bf16* h_in, int64_t in_bs, const scail_bf16* r, scail_bf16* h, int64_t h_bs,
                                 int64_t n_batch, int64_t rows, int64_t D, void* stream) {
    if (int rc = resid_check("scail_resid_apply", n_batch, rows, D, h_bs, "h_bs", in_bs, "in_bs", h_in, r, h)) return rc;
    if (n_batch == 0 || rows == 0) return 0;
    const int64_t span = rows * D, per_b8 = rows * (D / 8);
    if (n_batch > 1 && h_bs < span) {
        scail_set_error("scail_resid_apply: h_bs = " + std::to_string(h_bs) + " is smaller than one element's rows * D = " + std::to_string(span) +
                        " (the output elements would overlap)");
        return 1;
    }
    // h may BE h_in (element for element, or in_bs == 0 with h[0] == h_in); any other overlap of the two would let one thread's write
    // reach another thread's read
    const int64_t in_lo = (int64_t)reinterpret_cast<uintptr_t>(h_in), in_hi = in_lo + ((n_batch - 1) * in_bs + span) * 2;
    const int64_t h_lo = (int64_t)reinterpret_cast<uintptr_t>(h), h_hi = h_lo + ((n_batch - 1) * h_bs + span) * 2;
    if (in_lo < h_hi && h_lo < in_hi && !(h == h_in && (in_bs == 0 || in_bs == h_bs))) {
        scail_set_error("scail_resid_apply: h overlaps h_in without being h_in (h - h_in = " + std::to_string((h_lo - in_lo) / 2) + " elements, in_bs " +
                        std::to_string(in_bs) + ", h_bs " + std::to_string(h_bs) + "): in place means h == h_in with in_bs == 0 or in_bs == h_bs");
        return 1;
    }
    const int64_t wgs = std::min<int64_t>((per_b8 + 255) / 256, RESID_MAX_WGS);
    hipLaunchKernelGGL(resid_apply_kernel, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, h_in, in_bs, r, h, h_bs, n_batch, per_b8);
    return scail_check_launch("resid_apply");
}

extern "C" int scail_abs_diff_sums(const float* a, const float* b, int64_t n, double* out, void* stream) {
    if (n < 0 || n >= (1ll << 31)) {
        scail_set_error("scail_abs_diff_sums: n must be 0 .. 2^31 - 1, got " + std::to_string(n));
        return 1;
    }
    SCAIL_REQUIRE(out != nullptr && (reinterpret_cast<uintptr_t>(out) & 7) == 0, "out must be an 8-byte aligned device pointer");
    SCAIL_REQUIRE(n == 0 || (a != nullptr && b != nullptr), "null pointer");
    SCAIL_REQUIRE(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 3) == 0, "a and b must be 4-byte aligned");
    hipLaunchKernelGGL(abs_diff_sums_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a, b, n, out);
    return scail_check_launch("abs_diff_sums");
}

// ================================================================================================
// Small-sequence attention for the conditioning encoders (UMT5: 64 heads x 64, relative-position bias,
// key padding mask, no scaling -- umt5.py:72-123; CLIP ViT-H: 16 heads x 80, scale 1/sqrt(80) --
// clip.py:71-108).  Sequences are <= 512 tokens and the FLOPs are negligible (4 GFLOP per T5 layer), so
// this is a plain VALU kernel: K and V of one (batch, head) live in LDS, one wave per query row.
// ================================================================================================
#define SA_ROWS 32   // query rows per workgroup (8 per wave)
__global__ __launch_bounds__(256) void attn_small_kernel(
    const u16* __restrict__ q, const u16* __restrict__ k, const u16* __restrict__ v, u16* __restrict__ o,
    int64_t q_bs, int64_t q_rs, int64_t k_bs, int64_t k_rs, int64_t v_bs, int64_t v_rs, int64_t o_bs, int64_t o_rs,
    int Lq, int Lk, int hd, float scale, const int* __restrict__ bucket, const float* __restrict__ bias_tab, int n_heads_tab,
    const int* __restrict__ kmask, int64_t kmask_bs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_raw[];
    const int ldk = hd + 8;                                  // padded rows: conflict-free 16-byte reads
    u16* Ks = reinterpret_cast<u16*>(sm_raw);                // [Lk][ldk]
    u16* Vs = Ks + (size_t)Lk * ldk;                         // [Lk][hd]
    float* Ps = reinterpret_cast<float*>(Vs + (size_t)Lk * hd);   // [4 waves][Lk]
    float* Qs = Ps + 4 * Lk;                                 // [4 waves][hd]
    const int h = blockIdx.y;
    const int64_t b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cpr = hd >> 3;
    for (int c = tid; c < Lk * cpr; c += 256) {
        const int j = c / cpr, cc = c - j * cpr;
        *reinterpret_cast<uint4*>(Ks + j * ldk + cc * 8) = *reinterpret_cast<const uint4*>(k + b * k_bs + (int64_t)j * k_rs + h * hd + cc * 8);
        *reinterpret_cast<uint4*>(Vs + j * hd + cc * 8) = *reinterpret_cast<const uint4*>(v + b * v_bs + (int64_t)j * v_rs + h * hd + cc * 8);
    }
    __syncthreads();
    float* P = Ps + wave * Lk;
    float* Q = Qs + wave * hd;
    const int i0 = blockIdx.x * SA_ROWS;
    for (int ii = wave; ii < SA_ROWS; ii += 4) {
        const int i = i0 + ii;
        if (i >= Lq) break;                                   // wave-uniform
        for (int d = lane; d < hd; d += 64) Q[d] = bf2f(q[b * q_bs + (int64_t)i * q_rs + h * hd + d]) * scale;
        __builtin_amdgcn_s_waitcnt(0xC07F);                   // lgkmcnt(0): Q visible to the whole wave
        float mx = -INFINITY;
        for (int j = lane; j < Lk; j += 64) {
            float s = 0.f;
            for (int c = 0; c < cpr; ++c) {
                float kf[8];
                unpack8(*reinterpret_cast<const uint4*>(Ks + j * ldk + c * 8), kf);
#pragma unroll
                for (int e = 0; e < 8; ++e) s += Q[c * 8 + e] * kf[e];
            }
            if (bias_tab != nullptr) s += bias_tab[bucket[(int64_t)i * Lk + j] * n_heads_tab + h];
            if (kmask != nullptr && kmask[b * kmask_bs + j] == 0) s = -INFINITY;
            P[j] = s;
            mx = fmaxf(mx, s);
        }
#pragma unroll
        for (int of = 32; of > 0; of >>= 1) mx = fmaxf(mx, __shfl_xor(mx, of, 64));
        float sum = 0.f;
        for (int j = lane; j < Lk; j += 64) {
            const float pv = __expf(P[j] - mx);
            P[j] = pv;
            sum += pv;
        }
        sum = wave_sum(sum);
        __builtin_amdgcn_s_waitcnt(0xC07F);
        const float inv = 1.0f / sum;
        for (int d = lane; d < hd; d += 64) {
            float acc = 0.f;
            for (int j = 0; j < Lk; ++j) acc += P[j] * bf2f(Vs[j * hd + d]);
            o[b * o_bs + (int64_t)i * o_rs + h * hd + d] = f2bf(acc * inv);
        }
    }
}

__global__ void mul_bf16_kernel(const u16* __restrict__ a, const u16* __restrict__ b, u16* __restrict__ y, int64_t n8) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    float fa[8], fb[8], fo[8];
    unpack8(*reinterpret_cast<const uint4*>(a + i * 8), fa);
    unpack8(*reinterpret_cast<const uint4*>(b + i * 8), fb);
#pragma unroll
    for (int e = 0; e < 8; ++e) fo[e] = fa[e] * fb[e];
    *reinterpret_cast<uint4*>(y + i * 8) = pack8(fo);
}

// y[r, :] = x[r, :] * rowscale[r] + addrow[r % add_rows, :]   (either may be NULL)
__global__ void row_affine_kernel(const u16* __restrict__ x, u16* __restrict__ y, const float* __restrict__ rowscale,
                                  const u16* __restrict__ addrow, int64_t add_rows, int64_t rows, int D8) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * D8) return;
    const int64_t r = i / D8;
    const int c = (int)(i - r * D8);
    float f[8], a[8];
    unpack8(*reinterpret_cast<const uint4*>(x + i * 8), f);
    const float s = rowscale ? rowscale[r] : 1.f;
    if (addrow) unpack8(*reinterpret_cast<const uint4*>(addrow + ((r % add_rows) * D8 + c) * 8), a);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = f[e] * s + (addrow ? a[e] : 0.f);
    *reinterpret_cast<uint4*>(y + i * 8) = pack8(f);
}

extern "C" int scail_attn_small(const scail_bf16* q, const scail_bf16* k, const scail_bf16* v, scail_bf16* o,
                                const int64_t* strides, int64_t n_batch, int64_t heads, int64_t Lq, int64_t Lk, int64_t head_dim,
                                float scale, const int32_t* bucket, const float* bias_tab, const int32_t* key_mask,
                                int64_t key_mask_bs, void* stream) {
    SCAIL_REQUIRE(head_dim % 8 == 0 && head_dim <= 128, "head_dim must be a multiple of 8, <= 128");
    SCAIL_REQUIRE((bucket == nullptr) == (bias_tab == nullptr), "bucket and bias table go together");
    for (int i = 0; i < 8; ++i) SCAIL_REQUIRE(strides[i] % 8 == 0, "strides must keep 16-byte alignment");
    const size_t lds = (size_t)Lk * (head_dim + 8) * 2 + (size_t)Lk * head_dim * 2 + 4 * Lk * 4 + 4 * head_dim * 4;
    SCAIL_REQUIRE(lds <= 160 * 1024, "K and V of one head must fit in LDS (Lk * head_dim too large for this kernel)");
    if (Lq == 0 || n_batch == 0) return 0;
    dim3 grid((unsigned)((Lq + SA_ROWS - 1) / SA_ROWS), (unsigned)heads, (unsigned)n_batch);
    return scail_launch_lds<attn_small_kernel>("attn_small", 160 * 1024, grid, dim3(256), lds, stream, q, k, v, o, strides[0], strides[1], strides[2],       // (opt-in: the bound above)
                                               strides[3], strides[4], strides[5], strides[6], strides[7], (int)Lq, (int)Lk, (int)head_dim, scale, bucket, bias_tab,
                                               (int)heads, key_mask, key_mask_bs);
}

extern "C" int scail_mul_bf16(const scail_bf16* a, const scail_bf16* b, scail_bf16* y, int64_t n, void* stream) {
    SCAIL_REQUIRE(n % 8 == 0, "n must be a multiple of 8");
    if (n == 0) return 0;
    hipLaunchKernelGGL(mul_bf16_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, y, n / 8);
    return scail_check_launch("mul_bf16");
}

extern "C" int scail_row_affine(const scail_bf16* x, scail_bf16* y, const float* rowscale, const scail_bf16* addrow, int64_t add_rows,
                                int64_t rows, int64_t D, void* stream) {
    SCAIL_REQUIRE(D % 8 == 0, "D must be a multiple of 8");
    if (rows == 0) return 0;
    const int64_t total = rows * (D / 8);
    hipLaunchKernelGGL(row_affine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, rowscale,
                       addrow, add_rows > 0 ? add_rows : 1, rows, (int)(D / 8));
    return scail_check_launch("row_affine");
}

// ------------------------------------------------------------------------------------------------
// MEASUREMENT helper: a collective's CU occupancy on one GPU (include/scail_hip.h scail_comm_standin)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void comm_standin_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, int64_t n16, int64_t min_ticks) {
    const int64_t t0 = (int64_t)wall_clock64();                    // 100 MHz constant clock
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) dst[i] = src[i];
    while ((int64_t)wall_clock64() - t0 < min_ticks) __builtin_amdgcn_s_sleep(64);
}
extern "C" int scail_comm_standin(const void* src, void* dst, int64_t bytes, int32_t workgroups, int64_t min_ns, void* stream) {
    SCAIL_REQUIRE(bytes >= 0 && bytes % 16 == 0 && aligned16(src) && aligned16(dst), "bytes must be a multiple of 16, pointers 16-byte aligned");
    SCAIL_REQUIRE(workgroups >= 1 && workgroups <= 4096 && min_ns >= 0 && min_ns <= 1000000000ll, "workgroups in [1, 4096], min_ns in [0, 1e9]");
    hipLaunchKernelGGL(comm_standin_kernel, dim3((unsigned)workgroups), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst), bytes / 16, min_ns / 10);
    return scail_check_launch("comm_standin");
}
