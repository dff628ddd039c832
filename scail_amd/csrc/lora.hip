// LoRA adapters (include/scail_hip.h scail_lora_merge_bf16 / scail_add_scaled_bf16; scail_amd/lora.py): the one-off merge of a low-rank
// weight update, or of a full difference, into a bf16 weight window, in place.
//   merge:       acc = 0;  for j ascending: acc = acc + up[n, j] * down[j, k];   w[n, k] = bf16_rne(float(w[n, k]) + scale * acc)
//   add_scaled:  w[n, k] = bf16_rne(float(w[n, k]) + scale * d[n, k])
// EVERY operation is rounded on its own (contraction off), like the per-op-rounded passes of rowops.hip: the call gives the bits of the
// torch fp32 expression.  An fp32 MFMA is bitwise an fmaf chain, which is NOT this specification, so the product runs on the VALU.
//
// merge: a 256-thread workgroup owns a 64 x 128 tile of w; thread (ty, tx) of a 16 x 16 layout keeps a 4 x 8 micro-tile of acc in
// registers (its 8 columns are one 16-byte access to w).  The r loop is chunked: LORA_RC = 32 values of j at a time, the tile's up rows
// [64][32] and down columns [32][128] staged through LDS (25 KB), so r is unbounded by the kernel.
#include "common.h"
#include <cmath>

#define LORA_TN 64
#define LORA_TK 128
#define LORA_RC 32            // the LDS chunk of the r loop
#define LORA_UP_LD (LORA_RC + 4)   // 36 floats: rows stay 16-byte aligned; the four ty of a wave land 16 banks apart

// one element's last step, shared by the two kernels: three separately rounded operations
__device__ __forceinline__ float lora_axpy(float w, float scale, float a) {
#pragma clang fp contract(off)
    const float sa = scale * a;
    return w + sa;
}

__global__ __launch_bounds__(256) void lora_merge_kernel(u16* __restrict__ w, int64_t ldw, int64_t N, int64_t K, const float* __restrict__ up,
                                                         int64_t ld_up, const float* __restrict__ down, int64_t ld_down, int r, float scale,
                                                         int64_t tiles_k, int vec) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float up_s[LORA_TN][LORA_UP_LD];
    __shared__ __attribute__((aligned(16))) float dn_s[LORA_RC][LORA_TK];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t bn = (int64_t)blockIdx.x / tiles_k, bk = (int64_t)blockIdx.x - bn * tiles_k;
    const int64_t n0 = bn * LORA_TN, k0 = bk * LORA_TK;

    float acc[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[i][c] = 0.0f;

    for (int j0 = 0; j0 < r; j0 += LORA_RC) {
        const int jn = (r - j0 < LORA_RC) ? r - j0 : LORA_RC;
        // stage up[n0 .. n0 + 64, j0 .. j0 + jn) and down[j0 .. j0 + jn, k0 .. k0 + 128); what lies outside N, K or r is zero and never used
        for (int e = tid; e < LORA_TN * LORA_RC; e += 256) {
            const int row = e / LORA_RC, j = e - row * LORA_RC;
            const int64_t n = n0 + row;
            up_s[row][j] = (n < N && j < jn) ? up[n * ld_up + j0 + j] : 0.0f;
        }
        for (int e = tid; e < LORA_RC * LORA_TK; e += 256) {
            const int j = e / LORA_TK, c = e - j * LORA_TK;
            const int64_t k = k0 + c;
            dn_s[j][c] = (k < K && j < jn) ? down[(int64_t)(j0 + j) * ld_down + k] : 0.0f;
        }
        __syncthreads();
        int j = 0;
        for (; j + 4 <= jn; j += 4) {
            float a[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(&up_s[ty * 4 + i][j]);
                a[i][0] = v.x; a[i][1] = v.y; a[i][2] = v.z; a[i][3] = v.w;
            }
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {       // ascending j: the order is part of the contract
                const f32x4 b0 = *reinterpret_cast<const f32x4*>(&dn_s[j + jj][tx * 8]);
                const f32x4 b1 = *reinterpret_cast<const f32x4*>(&dn_s[j + jj][tx * 8 + 4]);
                const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        const float p = a[i][jj] * b[c];
                        acc[i][c] = acc[i][c] + p;
                    }
            }
        }
        for (; j < jn; ++j) {
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(&dn_s[j][tx * 8]);
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(&dn_s[j][tx * 8 + 4]);
            const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float a = up_s[ty * 4 + i][j];
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float p = a * b[c];
                    acc[i][c] = acc[i][c] + p;
                }
            }
        }
        __syncthreads();
    }

    const int64_t kc = k0 + tx * 8;
    if (kc >= K) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t n = n0 + ty * 4 + i;
        if (n >= N) break;
        u16* wr = w + n * ldw + kc;
        if (vec && kc + 8 <= K) {
            float f[8];
            unpack8(*reinterpret_cast<const uint4*>(wr), f);
#pragma unroll
            for (int c = 0; c < 8; ++c) f[c] = lora_axpy(f[c], scale, acc[i][c]);
            *reinterpret_cast<uint4*>(wr) = pack8(f);
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (kc + c < K) wr[c] = f2bf(lora_axpy(bf2f(wr[c]), scale, acc[i][c]));
        }
    }
}

// one thread per 8 columns of one row: idx -> (n, group of 8 columns)
__global__ __launch_bounds__(256) void add_scaled_kernel(u16* __restrict__ w, int64_t ldw, int64_t N, int64_t K, const float* __restrict__ d,
                                                         int64_t ldd, float scale, int64_t groups, int vec_w, int vec_d) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = idx / groups;
    if (n >= N) return;
    const int64_t kc = (idx - n * groups) * 8;
    u16* wr = w + n * ldw + kc;
    const float* dr = d + n * ldd + kc;
    if (kc + 8 <= K) {
        float f[8], g[8];
        if (vec_d) {
            const f32x4 d0 = *reinterpret_cast<const f32x4*>(dr), d1 = *reinterpret_cast<const f32x4*>(dr + 4);
            g[0] = d0.x; g[1] = d0.y; g[2] = d0.z; g[3] = d0.w; g[4] = d1.x; g[5] = d1.y; g[6] = d1.z; g[7] = d1.w;
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) g[c] = dr[c];
        }
        if (vec_w) {
            unpack8(*reinterpret_cast<const uint4*>(wr), f);
#pragma unroll
            for (int c = 0; c < 8; ++c) f[c] = lora_axpy(f[c], scale, g[c]);
            *reinterpret_cast<uint4*>(wr) = pack8(f);
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) wr[c] = f2bf(lora_axpy(bf2f(wr[c]), scale, g[c]));
        }
    } else {
        for (int c = 0; kc + c < K; ++c) wr[c] = f2bf(lora_axpy(bf2f(wr[c]), scale, dr[c]));
    }
}

// ---- host-side checks (the message names the value) + launches ----
static int lora_fail(const char* who, const std::string& msg) {
    scail_set_error(std::string(who) + ": " + msg);
    return 1;
}
static int lora_window_check(const char* who, int64_t ldw, int64_t N, int64_t K, float scale) {
    if (N < 0) return lora_fail(who, "N must be >= 0, got " + std::to_string(N));
    if (K < 0) return lora_fail(who, "K must be >= 0, got " + std::to_string(K));
    if (ldw < K) return lora_fail(who, "ldw = " + std::to_string(ldw) + " is smaller than K = " + std::to_string(K));
    if (!std::isfinite(scale)) return lora_fail(who, "scale must be finite, got " + std::to_string(scale));
    return 0;
}
static bool lora_aligned(const void* p, int64_t ld, int64_t elems) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % elems == 0; }
static const int64_t LORA_MAX_GRID = (1ll << 31) - 1;

extern "C" int scail_lora_merge_bf16(scail_bf16* w, int64_t ldw, int64_t N, int64_t K, const float* up, int64_t ld_up, const float* down,
                                     int64_t ld_down, int64_t r, float scale, void* stream) {
    const char* who = "scail_lora_merge_bf16";
    if (int rc = lora_window_check(who, ldw, N, K, scale)) return rc;
    if (r < 0) return lora_fail(who, "r must be >= 0, got " + std::to_string(r));
    if (r >= (1ll << 15)) return lora_fail(who, "r must be below 2^15 = 32768, got " + std::to_string(r));
    if (ld_up < r) return lora_fail(who, "ld_up = " + std::to_string(ld_up) + " is smaller than r = " + std::to_string(r));
    if (ld_down < K) return lora_fail(who, "ld_down = " + std::to_string(ld_down) + " is smaller than K = " + std::to_string(K));
    if (N == 0 || K == 0 || r == 0) return 0;
    if (w == nullptr || up == nullptr || down == nullptr)
        return lora_fail(who, std::string("null pointer: ") + (w == nullptr ? "w" : up == nullptr ? "up" : "down") + " (N = " + std::to_string(N) +
                                  ", K = " + std::to_string(K) + ", r = " + std::to_string(r) + ")");
    const int64_t tiles_n = N / LORA_TN + (N % LORA_TN != 0), tiles_k = K / LORA_TK + (K % LORA_TK != 0);
    if (tiles_n > LORA_MAX_GRID / tiles_k)
        return lora_fail(who, "the grid must stay below 2^31 workgroups, got " + std::to_string(tiles_n) + " x " + std::to_string(tiles_k) +
                                  " tiles of 64 x 128 (N = " + std::to_string(N) + ", K = " + std::to_string(K) + ")");
    hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)(tiles_n * tiles_k)), dim3(256), 0, (hipStream_t)stream, w, ldw, N, K, up, ld_up, down,
                       ld_down, (int)r, scale, tiles_k, lora_aligned(w, ldw, 8) ? 1 : 0);
    return scail_check_launch("lora_merge");
}

extern "C" int scail_add_scaled_bf16(scail_bf16* w, int64_t ldw, int64_t N, int64_t K, const float* d, int64_t ldd, float scale, void* stream) {
    const char* who = "scail_add_scaled_bf16";
    if (int rc = lora_window_check(who, ldw, N, K, scale)) return rc;
    if (ldd < K) return lora_fail(who, "ldd = " + std::to_string(ldd) + " is smaller than K = " + std::to_string(K));
    if (N == 0 || K == 0) return 0;
    if (w == nullptr || d == nullptr)
        return lora_fail(who, std::string("null pointer: ") + (w == nullptr ? "w" : "d") + " (N = " + std::to_string(N) + ", K = " +
                                  std::to_string(K) + ")");
    const int64_t groups = K / 8 + (K % 8 != 0);
    if (N > (LORA_MAX_GRID * 256) / groups)
        return lora_fail(who, "the grid must stay below 2^31 workgroups, got N = " + std::to_string(N) + " rows of " + std::to_string(groups) +
                                  " 8-column groups (K = " + std::to_string(K) + ")");
    const int64_t threads = N * groups;
    hipLaunchKernelGGL(add_scaled_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, ldw, N, K, d, ldd, scale,
                       groups, lora_aligned(w, ldw, 8) ? 1 : 0, lora_aligned(d, ldd, 4) ? 1 : 0);
    return scail_check_launch("add_scaled");
}
