// FP8 (OCP e4m3fn) path of the per-token GEMMs (include/scail_hip.h "fp8 per-token GEMMs"):
//   scail_quant_fp8_rows  bf16 [R, C] -> e4m3 [R, C] + one fp32 scale per row (activations per token, weights per output channel)
//   scail_rel_err_rows    sum of squared differences / sum of squares of two bf16 matrices into a device fp64 accumulator (the fp8 probe)
//   scail_gemm_fp8        y = epi(acc[m, n] * sx[m] * sw[n] + bias[n]), acc = the e4m3 product on the block-scaled MFMA
//                         v_mfma_scale_f32_32x32x64_f8f6f4 (twice the bf16 matrix rate per clock), bf16 out.
// The E8M0 block scales of the MFMA are held at the unit value (127): the per-row fp32 scales are applied in the epilogue, so every
// output row still depends on its own input row alone (what keeps the executor's CFG-pair and last-layer prunings exact).
//   scail_quant_mxfp8_rows  bf16 [R, C] -> e4m3 [R, C] + one E8M0 byte per aligned block of 32 columns (the OCP MX layout)
//   scail_gemm_mxfp8        the same GEMM kernel with the block scales in the MFMA's scale operands and no fp32 scales in the epilogue;
//                           a block lies inside a row, so the row independence above holds here too.
//   scail_quant_mxfp6_rows  bf16 [R, C] -> packed OCP e2m3 codes [R, 3 C / 4 bytes] + one E8M0 byte per aligned block of 32 columns
//   scail_gemm_mxfp6        the MX GEMM on 6-bit operands (cbsz = blgp = 2: half the MFMA cycles, 3/4 of the operand bytes); a sibling
//                           kernel at the end of this file.
#include "common.h"
#include "gemm_epi.h"

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef uint8_t u8;

// ---- quantization ------------------------------------------------------------------------------------------------------------
// One 256-thread block per row, 16-byte loads (8 bf16) per lane: pass 1 takes amax = max |x| over the row, pass 2 re-reads the row
// (an L2 hit: a row is at most a few tens of KB) and writes 8 codes per lane.  Numerics (bit-exact, tests/test_fp8_gpu.py):
//   amax == 0: s = 1, q = 0;  else s = amax / 448, r = 448 / amax, q = e4m3_rne(clamp(x r, -448, 448)) (clamped first: e4m3fn has no
//   infinity, v_cvt_pk_fp8_f32 would turn an overflow into NaN).
#define QF8_THREADS 256
__global__ __launch_bounds__(QF8_THREADS) void scail_quant_fp8_rows_kernel(const u16* __restrict__ x, int64_t ldx, u8* __restrict__ q,
                                                                           int64_t ldq, float* __restrict__ s, int cols) {
    __shared__ float red[QF8_THREADS / 64];
    const int64_t r = blockIdx.x;
    const u16* xr = x + r * ldx;
    u8* qr = q + r * ldq;
    float amax = 0.f;
    for (int c = threadIdx.x * 8; c < cols; c += QF8_THREADS * 8) {
        float f[8];
        unpack8(*reinterpret_cast<const uint4*>(xr + c), f);
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(f[e]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const bool zero = amax == 0.f;
    const float rs = zero ? 0.f : 448.0f / amax;
    if (threadIdx.x == 0) s[r] = zero ? 1.0f : amax / 448.0f;
    for (int c = threadIdx.x * 8; c < cols; c += QF8_THREADS * 8) {
        float f[8];
        unpack8(*reinterpret_cast<const uint4*>(xr + c), f);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = fminf(fmaxf(f[e] * rs, -448.0f), 448.0f);
        int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
        int hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
        *reinterpret_cast<uint2*>(qr + c) = zero ? make_uint2(0u, 0u) : make_uint2((uint32_t)lo, (uint32_t)hi);
    }
}

extern "C" int scail_quant_fp8_rows(const scail_bf16* x, int64_t ldx, uint8_t* q, int64_t ldq, float* s, int64_t rows, int64_t cols,
                                    void* stream) {
    SCAIL_REQUIRE(x != nullptr && q != nullptr && s != nullptr, "null pointer");
    SCAIL_REQUIRE(rows >= 0 && cols > 0 && cols % 8 == 0 && cols < (1ll << 30), "cols must be a positive multiple of 8");
    SCAIL_REQUIRE(ldx >= cols && ldq >= cols && ldx % 8 == 0 && ldq % 8 == 0, "ldx / ldq must be >= cols and multiples of 8");
    SCAIL_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(q) & 7) == 0 &&
                      (reinterpret_cast<uintptr_t>(s) & 3) == 0,
                  "pointer alignment (x 16 B, q 8 B, s 4 B)");
    SCAIL_REQUIRE(rows < (1ll << 31), "too many rows");
    if (rows == 0) return 0;
    hipLaunchKernelGGL(scail_quant_fp8_rows_kernel, dim3((unsigned)rows), dim3(QF8_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const u16*>(x), ldx, q, ldq, s, (int)cols);
    return scail_check_launch("scail_quant_fp8_rows");
}

// ---- MX block quantization (include/scail_hip.h scail_quant_mxfp8_rows) ------------------------------------------------------------
// One lane per 8 columns (a 16-byte load), the 4 lanes of an aligned quad hold one block of 32: the block's amax is two xor shuffles away
// and the row is read once.  The lanes are laid over the [rows, cols / 8] chunks linearly, so every shape fills its workgroups; cols % 32
// == 0 keeps a quad inside one row and makes the tail of the last workgroup whole quads.  Numerics (bit-exact, tests/test_mxfp8_gpu.py):
//   amax == 0: byte 127, codes 0;  else amax = m 2^E (1 <= m < 2), s = E - 8 + (m > 1.75) clamped to >= -127 (the smallest s with
//   amax 2^-s <= 448), byte s + 127, q = e4m3_rne(clamp(x 2^-s, -448, 448)).  E and m are read from amax's fp32 bits; a subnormal amax
//   (biased exponent 0) lands below the clamp either way.  2^-s has the biased exponent 127 - s in [7, 254]: a normal fp32.
#define QMX_THREADS 256
__global__ __launch_bounds__(QMX_THREADS) void scail_quant_mxfp8_rows_kernel(const u16* __restrict__ x, int64_t ldx, u8* __restrict__ q,
                                                                             int64_t ldq, u8* __restrict__ e, int64_t lde, int64_t chunks,
                                                                             int cpr) {
    const int64_t i = (int64_t)blockIdx.x * QMX_THREADS + threadIdx.x;
    if (i >= chunks) return;          // whole quads leave together
    const int64_t r = i / cpr;
    const int c = (int)(i - r * cpr) * 8;
    float f[8];
    unpack8(*reinterpret_cast<const uint4*>(x + r * ldx + c), f);
    float amax = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) amax = fmaxf(amax, fabsf(f[k]));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    const bool zero = amax == 0.f;
    const uint32_t bits = __float_as_uint(amax);
    int s = (int)(bits >> 23) - 127 - 8 + ((bits & 0x7fffffu) > 0x600000u ? 1 : 0);
    s = zero ? 0 : max(s, -127);
    const float rs = __uint_as_float((uint32_t)(127 - s) << 23);
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = fminf(fmaxf(f[k] * rs, -448.0f), 448.0f);
    int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
    int hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
    *reinterpret_cast<uint2*>(q + r * ldq + c) = zero ? make_uint2(0u, 0u) : make_uint2((uint32_t)lo, (uint32_t)hi);
    if ((threadIdx.x & 3) == 0) e[r * lde + (c >> 5)] = (u8)(s + 127);
}

extern "C" int scail_quant_mxfp8_rows(const scail_bf16* x, int64_t ldx, uint8_t* q, int64_t ldq, uint8_t* e, int64_t lde, int64_t rows,
                                      int64_t cols, void* stream) {
    SCAIL_REQUIRE(x != nullptr && q != nullptr && e != nullptr, "null pointer");
    SCAIL_REQUIRE(rows >= 0 && cols > 0 && cols % 32 == 0 && cols < (1ll << 30), "cols must be a positive multiple of 32");
    SCAIL_REQUIRE(ldx >= cols && ldq >= cols && ldx % 8 == 0 && ldq % 8 == 0, "ldx / ldq must be >= cols and multiples of 8");
    SCAIL_REQUIRE(lde >= cols / 32, "lde must be >= cols / 32");
    SCAIL_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(q) & 7) == 0, "pointer alignment (x 16 B, q 8 B)");
    SCAIL_REQUIRE(rows < (1ll << 31), "too many rows");
    const int64_t cpr = cols / 8, chunks = rows * cpr, wgs = (chunks + QMX_THREADS - 1) / QMX_THREADS;
    SCAIL_REQUIRE(wgs < (1ll << 31), "too many elements (rows * cols / 2048 must stay below 2^31)");
    if (rows == 0) return 0;
    hipLaunchKernelGGL(scail_quant_mxfp8_rows_kernel, dim3((unsigned)wgs), dim3(QMX_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const u16*>(x), ldx, q, ldq, e, lde, chunks, (int)cpr);
    return scail_check_launch("scail_quant_mxfp8_rows");
}

// ---- MXFP6 block quantization (include/scail_hip.h scail_quant_mxfp6_rows) ---------------------------------------------------------
// One lane per 16 columns (two 16-byte loads), the 2 lanes of an aligned pair hold one block of 32: the block's amax is one xor shuffle
// away and the row is read once.  A lane's 16 codes are 96 bits = 3 dwords, written with one 12-byte store at byte 12 * (c / 16) of the
// row: consecutive lanes write consecutive bytes.  (A lane's piece of the packed row is 12 bytes at a 12-byte pitch, so 16-byte stores
// would need a 4-lane exchange; the pass moves 2 bytes in and 0.78 out per element.)  Plain integer code, no convert instruction.
// Numerics (bit-exact, tests/test_mxfp6_gpu.py):
//   amax == 0: byte 127, codes 0;  else amax = m 2^E (1 <= m < 2), s = E - 2 + (m > 1.875) clamped to >= -127 (the smallest s with
//   amax 2^-s <= 7.5), byte s + 127, q = e2m3_rne(clamp(x 2^-s, -7.5, 7.5)).  e2m3_rne: |v| < 2 has the step 1/8 (subnormals and the first
//   binade), [2, 4) 1/4, [4, 7.5] 1/2; n = rint(|v| / step) (ties to even) and the code magnitude is n, n + 8, n + 16: n and the code have
//   the same parity, so the tie rule carries over, and n = 16 is the next binade's first code.  The sign bit of v is kept (-0 too).
//   A NaN is skipped by the amax and becomes code 0; an infinity counts as 2^128 (byte 253) and becomes +-7.5.
#define QF6_THREADS 256
__device__ __forceinline__ uint32_t e2m3_code(float v) {
    const float a = fabsf(v);
    const float inv = a < 2.f ? 8.f : a < 4.f ? 4.f : 2.f;
    const uint32_t base = a < 2.f ? 0u : a < 4.f ? 8u : 16u;
    return ((uint32_t)__builtin_rintf(a * inv) + base) | ((__float_as_uint(v) >> 31) << 5);
}
__global__ __launch_bounds__(QF6_THREADS) void scail_quant_mxfp6_rows_kernel(const u16* __restrict__ x, int64_t ldx, u8* __restrict__ q,
                                                                             int64_t ldq, u8* __restrict__ e, int64_t lde, int64_t chunks,
                                                                             int cpr) {
    const int64_t i = (int64_t)blockIdx.x * QF6_THREADS + threadIdx.x;
    if (i >= chunks) return;          // whole pairs leave together
    const int64_t r = i / cpr;
    const int c16 = (int)(i - r * cpr);
    float f[16];
    unpack8(*reinterpret_cast<const uint4*>(x + r * ldx + c16 * 16), f);
    unpack8(*reinterpret_cast<const uint4*>(x + r * ldx + c16 * 16 + 8), f + 8);
    float amax = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) amax = fmaxf(amax, fabsf(f[k]));      // fmaxf skips a NaN
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    const bool zero = amax == 0.f;
    const uint32_t bits = __float_as_uint(amax);
    int s = (int)(bits >> 23) - 127 - 2 + ((bits & 0x7fffffu) > 0x700000u ? 1 : 0);
    s = zero ? 0 : max(s, -127);
    const float rs = __uint_as_float((uint32_t)(127 - s) << 23);
    uint32_t cd[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        float v = f[k] * rs;
        v = v != v ? 0.f : fminf(fmaxf(v, -7.5f), 7.5f);
        cd[k] = zero ? 0u : e2m3_code(v);
    }
    uint32_t* out = reinterpret_cast<uint32_t*>(q + r * ldq + c16 * 12);
    out[0] = cd[0] | cd[1] << 6 | cd[2] << 12 | cd[3] << 18 | cd[4] << 24 | cd[5] << 30;
    out[1] = cd[5] >> 2 | cd[6] << 4 | cd[7] << 10 | cd[8] << 16 | cd[9] << 22 | cd[10] << 28;
    out[2] = cd[10] >> 4 | cd[11] << 2 | cd[12] << 8 | cd[13] << 14 | cd[14] << 20 | cd[15] << 26;
    if ((threadIdx.x & 1) == 0) e[r * lde + (c16 >> 1)] = (u8)(s + 127);
}

extern "C" int scail_quant_mxfp6_rows(const scail_bf16* x, int64_t ldx, uint8_t* q, int64_t ldq, uint8_t* e, int64_t lde, int64_t rows,
                                      int64_t cols, void* stream) {
    SCAIL_REQUIRE(x != nullptr && q != nullptr && e != nullptr, "null pointer");
    SCAIL_REQUIRE(rows >= 0 && cols > 0 && cols % 32 == 0 && cols < (1ll << 30), "cols must be a positive multiple of 32");
    SCAIL_REQUIRE(ldx >= cols && ldx % 8 == 0, "ldx must be >= cols and a multiple of 8");
    SCAIL_REQUIRE(ldq >= cols / 4 * 3 && ldq % 4 == 0, "ldq (bytes) must be >= 3 * cols / 4 and a multiple of 4");
    SCAIL_REQUIRE(lde >= cols / 32, "lde must be >= cols / 32");
    SCAIL_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(q) & 3) == 0, "pointer alignment (x 16 B, q 4 B)");
    SCAIL_REQUIRE(rows < (1ll << 31), "too many rows");
    const int64_t cpr = cols / 16, chunks = rows * cpr, wgs = (chunks + QF6_THREADS - 1) / QF6_THREADS;
    SCAIL_REQUIRE(wgs < (1ll << 31), "too many elements (rows * cols / 4096 must stay below 2^31)");
    if (rows == 0) return 0;
    hipLaunchKernelGGL(scail_quant_mxfp6_rows_kernel, dim3((unsigned)wgs), dim3(QF6_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const u16*>(x), ldx, q, ldq, e, lde, chunks, (int)cpr);
    return scail_check_launch("scail_quant_mxfp6_rows");
}

// ---- relative error of two bf16 matrices (the executor's fp8 probe, include/scail_hip.h scail_rel_err_rows) -------------------------
// Stage 1: workgroup k walks the rows [k rpb, (k + 1) rpb) in ascending order, 256 threads and 16-byte loads per row as above.  A lane
// adds its elements in ascending column order, d = b - a, err = err + d d, pow = pow + a a in fp32 with every operation rounded on its own
// (contraction off); the lanes of a wave are combined by the xor butterfly 32, 16, .., 1 and the four waves as (w0 + w1) + (w2 + w3): the
// same bits in every thread.  Thread 0 widens the row's two sums to fp64, adds them to the workgroup's and keeps the largest row ratio.
// Stage 2 (one workgroup, after stage 1 in stream order): thread 0 adds the workgroups' partial sums in ascending order and updates acc.
// No floating-point atomics and no inter-workgroup hand-off inside a launch: rpb and the grid depend on `rows` alone, so the same inputs
// give the same bits.  The partial sums live in static device memory (one copy per device): calls on one device must be stream-ordered
// among themselves, as the executor's are.
#define RE_THREADS 256
#define RE_MAX_WGS 1024
static __device__ double g_rel_err_part[RE_MAX_WGS][2];
static __device__ float g_rel_err_max[RE_MAX_WGS];

// max that keeps a NaN (a row with a non-finite element must not look clean)
__device__ __forceinline__ float re_max(float m, float r) { return (r > m || r != r) ? r : m; }

__global__ __launch_bounds__(RE_THREADS) void scail_rel_err_rows_kernel(const u16* __restrict__ a, int64_t lda, const u16* __restrict__ b,
                                                                        int64_t ldb, int64_t rows, int64_t rpb, int cols) {
#pragma clang fp contract(off)
    __shared__ float red[2][RE_THREADS / 64];
    const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = r0 + rpb < rows ? r0 + rpb : rows;
    double se = 0.0, sp = 0.0;
    float mx = 0.f;
    for (int64_t r = r0; r < r1; ++r) {
        const u16* ar = a + r * lda;
        const u16* br = b + r * ldb;
        float err = 0.f, pw = 0.f;
        for (int c = threadIdx.x * 8; c < cols; c += RE_THREADS * 8) {
            float fa[8], fb[8];
            unpack8(*reinterpret_cast<const uint4*>(ar + c), fa);
            unpack8(*reinterpret_cast<const uint4*>(br + c), fb);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = fb[e] - fa[e];
                err = err + d * d;
                pw = pw + fa[e] * fa[e];
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            err = err + __shfl_xor(err, o, 64);
            pw = pw + __shfl_xor(pw, o, 64);
        }
        __syncthreads();     // the previous row's reads of red are done
        if ((threadIdx.x & 63) == 0) {
            red[0][threadIdx.x >> 6] = err;
            red[1][threadIdx.x >> 6] = pw;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const float err_r = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
            const float pow_r = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
            const float ratio = pow_r == 0.f ? (err_r == 0.f ? 0.f : __builtin_inff()) : __fdiv_rn(err_r, pow_r);
            se = se + (double)err_r;
            sp = sp + (double)pow_r;
            mx = re_max(mx, ratio);
        }
    }
    if (threadIdx.x == 0) {
        g_rel_err_part[blockIdx.x][0] = se;
        g_rel_err_part[blockIdx.x][1] = sp;
        g_rel_err_max[blockIdx.x] = mx;
    }
}

__global__ __launch_bounds__(64) void scail_rel_err_finish_kernel(double* __restrict__ acc, int wgs, double rows) {
    if (threadIdx.x != 0) return;
    double se = 0.0, sp = 0.0;
    float mx = 0.f;
    for (int k = 0; k < wgs; ++k) {
        se = se + g_rel_err_part[k][0];
        sp = sp + g_rel_err_part[k][1];
        mx = re_max(mx, g_rel_err_max[k]);
    }
    acc[0] = acc[0] + se;
    acc[1] = acc[1] + sp;
    const double m = (double)mx;
    acc[2] = (m > acc[2] || m != m) ? m : acc[2];
    acc[3] = acc[3] + rows;
}

extern "C" int scail_rel_err_rows(const scail_bf16* a, int64_t lda, const scail_bf16* b, int64_t ldb, double* acc, int64_t rows,
                                  int64_t cols, void* stream) {
    SCAIL_REQUIRE(a != nullptr && b != nullptr && acc != nullptr, "null pointer");
    SCAIL_REQUIRE(rows >= 0 && cols > 0 && cols % 8 == 0 && cols < (1ll << 30), "cols must be a positive multiple of 8");
    SCAIL_REQUIRE(lda >= cols && ldb >= cols && lda % 8 == 0 && ldb % 8 == 0, "lda / ldb must be >= cols and multiples of 8");
    SCAIL_REQUIRE((reinterpret_cast<uintptr_t>(a) & 15) == 0 && (reinterpret_cast<uintptr_t>(b) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(acc) & 7) == 0,
                  "pointer alignment (a, b 16 B; acc 8 B)");
    SCAIL_REQUIRE(rows < (1ll << 31), "too many rows");
    if (rows == 0) return 0;
    const int64_t rpb = (rows + RE_MAX_WGS - 1) / RE_MAX_WGS, wgs = (rows + rpb - 1) / rpb;
    hipLaunchKernelGGL(scail_rel_err_rows_kernel, dim3((unsigned)wgs), dim3(RE_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const u16*>(a), lda, reinterpret_cast<const u16*>(b), ldb, rows, rpb, (int)cols);
    if (int rc = scail_check_launch("scail_rel_err_rows")) return rc;
    hipLaunchKernelGGL(scail_rel_err_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, acc, (int)wgs, (double)rows);
    return scail_check_launch("scail_rel_err_rows (finish)");
}

// ---- GEMM --------------------------------------------------------------------------------------------------------------------
// 256 x 256 tile, k-tile 128 (= 128 bytes of a row, as the bf16 kernels' 64), 8 waves (2 x 4), wave tile 128(m) x 64(n) as
// 4 x 2 fragments of v_mfma_scale_f32_32x32x64_f8f6f4.  Both operands arrive by LDS-DMA (global_load_lds_dwordx4, 8 rows x 128 B per
// wave-instruction, lane-linear unpadded 128-B rows) two k-tiles deep, all LDS in ONE dynamic __shared__ array; bank conflicts are
// removed by XOR-ing the 16-byte chunk index with (row >> 1) & 7 on the per-lane SOURCE address and on the fragment reads (the layout
// of gemm.hip's LDS-DMA kernel).  One barrier per k-tile: the DMA of tile t + 1 is issued before the MFMAs of tile t and retired
// (vmcnt(0) + barrier) after them.
// Fragments: the MFMA is issued "transposed" (A = W rows, B = x rows) so that a lane's accumulators run along n (gemm_epi.h).  Lane
// (r = l & 31, g = l >> 5) of a 32x32x64 step feeds the 32 bytes k = 32 g .. 32 g + 31 of row r of each operand.  A and B take the same
// k subset per lane, so the dot product is right whatever order the hardware gives those 32 k inside the step (the block scales are
// all 1); the exact-integer test with an asymmetric W proves the row / column map.
// MX instantiation (scail_gemm_mxfp8): lane (r, g) passes the E8M0 byte of block g of the step as its scale operand; the hardware applies
// it to the first (g = 0) or second (g = 1) 16 bytes of both lanes of row r, so this instantiation deals the bytes accordingly (foff below).
// The 4 blocks of a row's k-tile are one aligned dword of the row-major scale matrix.  The scale dwords are staged with the tile: 4 KB of
// LDS behind the tiles, [2][512] dwords = x rows 0 .. 255 then W rows 0 .. 255 of the tile, filled by ONE global_load_lds_dword per wave
// and k-tile (lane -> row 64 wave + lane) next to the tile's own DMA and retired by the same vmcnt(0) + barrier: still one barrier per
// k-tile.  A lane reads the dword of each of its 2 + 4 fragment rows (ds_read_b32, consecutive rows: no bank conflict) and extracts byte
// 2 ks + g with a bit-field extract (the index depends on the lane, so it cannot be the instruction's op_sel).  The epilogue then applies
// no scales.  (First form: every lane loaded its six dwords from global memory, 6 scattered loads of 32 cache lines each per wave and
// k-tile; it ran at 1.36 - 1.46 x the per-row kernel's time, profiles/fp8_mx_ab_global_scale_loads.log.)  The per-row instantiation takes
// none of this: it compiles to the instructions it had before.
#define F8_BK 128
#define F8_GROUP_M 4

struct GemmFp8Params {
    GemmParams e;                  // epilogue part (x / w unused)
    const u8* x; const u8* w;      // e4m3 [M, lda], [N, K]
    const float* sx; const float* sw;   // per-row instantiation: fp32 scales [M], [N]
    const u8* ex; const u8* ew;         // MX instantiation: E8M0 block scales [M, ldex], [N, K / 32]
    int64_t ldex;
};

template <int EPI, bool MX>
__global__ __launch_bounds__(512) void scail_gemm_fp8_kernel(GemmFp8Params P) {
    constexpr int BM = 256, BN = 256, WN = 4, NT = 512;
    constexpr int WTM = 128, WTN = 64, MI = WTM / 32, NI = WTN / 32;
    extern __shared__ __attribute__((aligned(16))) u8 smem8[];
    u8* Xs = smem8;                   // [2][BM][F8_BK]
    u8* Ws = smem8 + 2 * BM * F8_BK;  // [2][BN][F8_BK]
    uint32_t* Ss = reinterpret_cast<uint32_t*>(smem8 + 2 * (BM + BN) * F8_BK);   // MX only: [2][BM + BN] scale dwords of the k-tile
    const GemmParams& p = P.e;

    // ---- tile mapping: XCD-aware bijective remap, then groups of F8_GROUP_M m-tiles sweeping n ----
    const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
    const int nb = tiles_m * tiles_n;
    int wg;
    {
        const int id = blockIdx.x;
        const int q = nb >> 3, r = nb & 7, xcd = id & 7, loc = id >> 3;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    const int in_group = F8_GROUP_M * tiles_n;
    const int gid = wg / in_group;
    const int first_m = gid * F8_GROUP_M;
    const int gsz = min(tiles_m - first_m, F8_GROUP_M);
    const int pid_m = first_m + (wg % in_group) % gsz;
    const int pid_n = (wg % in_group) / gsz;
    const int m0 = pid_m * BM, n0 = pid_n * BN;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, g = lane >> 5;

    // LDS-DMA pieces: piece j of an operand = tile rows 8j .. 8j + 7; lane -> row 8j + (l >> 3), chunk l & 7.  Rows past M / N read
    // the last row (their outputs are not stored).
    constexpr int PA = BM / 8 / (NT / 64), PB = BN / 8 / (NT / 64);
    const int d_row = lane >> 3, d_c = lane & 7;
    const u8* srcx[PA];
    const u8* srcw[PB];
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        const int r = 8 * (wave * PA + i) + d_row;
        srcx[i] = P.x + (int64_t)min(m0 + r, p.M - 1) * p.lda + ((d_c ^ ((r >> 1) & 7)) << 4);
    }
#pragma unroll
    for (int i = 0; i < PB; ++i) {
        const int r = 8 * (wave * PB + i) + d_row;
        srcw[i] = P.w + (int64_t)min(n0 + r, p.N - 1) * p.K + ((d_c ^ ((r >> 1) & 7)) << 4);
    }
#define F8_DMA(k0_, buf_)                                                                                                 \
    {                                                                                                                     \
        _Pragma("unroll") for (int i_ = 0; i_ < PA; ++i_)                                                                 \
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(srcx[i_] + (k0_)),          \
                (__attribute__((address_space(3))) void*)(Xs + ((buf_) * BM + 8 * (wave * PA + i_)) * F8_BK), 16, 0, 0);  \
        _Pragma("unroll") for (int i_ = 0; i_ < PB; ++i_)                                                                 \
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(srcw[i_] + (k0_)),          \
                (__attribute__((address_space(3))) void*)(Ws + ((buf_) * BN + 8 * (wave * PB + i_)) * F8_BK), 16, 0, 0);  \
    }
    // fragment-read byte offsets in this lane's row: k-step ks, 16-byte half hf -> chunk 4 ks + 2 g + hf, swizzled.
    // MX: chunk 4 ks + 2 hf + g instead.  The hardware takes the scale that lane (r, h) supplies for the register half h (registers
    // 4 h .. 4 h + 3) of BOTH lanes (r, 0) and (r, 1) -- a step is two K = 32 halves, a lane holds 16 bytes of each --, so the block
    // k = 32 h .. 32 h + 31 of a step has to sit in half h of the two lanes: lane (r, g) takes bytes 16 g .. 16 g + 15 of either block.
    // (Found on the device: with contiguous 32 bytes per lane, one raised scale byte still moves the right row by the right amount,
    // but it scales bytes {0..15, 32..47} or {16..31, 48..63} of the step.)
    int foff[2][2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) foff[ks][hf] = ((4 * ks + (MX ? 2 * hf + g : 2 * g + hf)) ^ ((l31 >> 1) & 7)) << 4;

    f32x16 acc[NI][MI];
#pragma unroll
    for (int a = 0; a < NI; ++a)
#pragma unroll
        for (int b = 0; b < MI; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

    const int nk = p.K / F8_BK;
    // MX: this lane's row of the scale stage, 64 wave + lane: waves 0 .. 3 the x rows, 4 .. 7 the W rows (rows past M / N read the last
    // row's scales, as they read its codes)
    static_assert(BM == 256 && BN == 256 && NT == 512, "one scale row per thread");
    const u8* srcs = nullptr;
    if constexpr (MX) {
        const int r = (wave & 3) * 64 + lane;
        srcs = wave < 4 ? P.ex + (int64_t)min(m0 + r, p.M - 1) * P.ldex : P.ew + (int64_t)min(n0 + r, p.N - 1) * (p.K / 32);
    }
#define F8_SCALE_DMA(k0_, buf_)                                                                                            \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(srcs + ((k0_) >> 5)),                \
        (__attribute__((address_space(3))) void*)(Ss + (buf_) * (BM + BN) + 64 * wave), 4, 0, 0);
    if constexpr (MX) F8_SCALE_DMA(0, 0)
    F8_DMA(0, 0)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
        const int cur = t & 1;
        if (t + 1 < nk) {
            F8_DMA((t + 1) * F8_BK, cur ^ 1)
            if constexpr (MX) F8_SCALE_DMA((t + 1) * F8_BK, cur ^ 1)
        }
        uint32_t sc[NI + MI];          // MX: the scale dwords of this lane's fragment rows, W then x
        if constexpr (MX) {
#pragma unroll
            for (int i = 0; i < NI; ++i) sc[i] = Ss[cur * (BM + BN) + BM + wn * WTN + i * 32 + l31];
#pragma unroll
            for (int i = 0; i < MI; ++i) sc[NI + i] = Ss[cur * (BM + BN) + wm * WTM + i * 32 + l31];
        }
        const u8* xs = Xs + (cur * BM + wm * WTM + l31) * F8_BK;
        const u8* ws = Ws + (cur * BN + wn * WTN + l31) * F8_BK;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            i32x8 wf[NI], xf[MI];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const uint4 lo = *reinterpret_cast<const uint4*>(ws + i * 32 * F8_BK + foff[ks][0]);
                const uint4 hi = *reinterpret_cast<const uint4*>(ws + i * 32 * F8_BK + foff[ks][1]);
                wf[i] = i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
            }
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const uint4 lo = *reinterpret_cast<const uint4*>(xs + i * 32 * F8_BK + foff[ks][0]);
                const uint4 hi = *reinterpret_cast<const uint4*>(xs + i * 32 * F8_BK + foff[ks][1]);
                xf[i] = i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
            }
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    if constexpr (MX)
                        acc[ni][mi] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[ni], xf[mi], acc[ni][mi], 0, 0, 0,
                                                                                     (int)((sc[ni] >> (16 * ks + 8 * g)) & 0xffu), 0,
                                                                                     (int)((sc[NI + mi] >> (16 * ks + 8 * g)) & 0xffu));
                    else
                        acc[ni][mi] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[ni], xf[mi], acc[ni][mi], 0, 0, 0, 127, 0, 127);
                }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
#undef F8_DMA
#undef F8_SCALE_DMA

    // per-token x per-channel scales: acc[ni][mi][4 rr + e] is (m = .. + l31, n = .. + 8 rr + 4 g + e); v = (acc * sx[m]) * sw[n]
    if constexpr (!MX) {
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int n = n0 + wn * WTN + ni * 32 + 8 * rr + 4 * g;
                const float4 swn = n < p.N ? *reinterpret_cast<const float4*>(P.sw + n) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    const float sxm = P.sx[min(m0 + wm * WTM + mi * 32 + l31, p.M - 1)];
                    acc[ni][mi][4 * rr + 0] = acc[ni][mi][4 * rr + 0] * sxm * swn.x;
                    acc[ni][mi][4 * rr + 1] = acc[ni][mi][4 * rr + 1] * sxm * swn.y;
                    acc[ni][mi][4 * rr + 2] = acc[ni][mi][4 * rr + 2] * sxm * swn.z;
                    acc[ni][mi][4 * rr + 3] = acc[ni][mi][4 * rr + 3] * sxm * swn.w;
                }
            }
    }
    gemm_epilogue<EPI, MI, NI, WTM, WTN>(acc, p, m0, n0, wm, wn, l31, g);
}

template <int EPI, bool MX>
static int launch_gemm_fp8(const GemmFp8Params& P, hipStream_t stream) {
    constexpr int lds = 2 * (256 + 256) * F8_BK + (MX ? 2 * (256 + 256) * 4 : 0);   // 128 KB (+ 4 KB of staged block scales)
    const int tiles = ((P.e.M + 255) / 256) * ((P.e.N + 255) / 256);
    return scail_launch_lds<scail_gemm_fp8_kernel<EPI, MX>>(MX ? "scail_gemm_mxfp8" : "scail_gemm_fp8", lds, dim3((unsigned)tiles), dim3(512),
                                                            lds, stream, P);
}

extern "C" int scail_gemm_fp8(const uint8_t* x, int64_t lda, const float* sx, const uint8_t* w, const float* sw, const float* bias,
                              scail_bf16* y, int64_t ldc, int64_t M, int64_t N, int64_t K, int epilogue,
                              const scail_bf16* resid, int64_t ldr, const float* gate, int64_t gate_stride,
                              int64_t rows_per_batch, void* stream) {
    SCAIL_REQUIRE(x != nullptr && sx != nullptr && w != nullptr && sw != nullptr && y != nullptr, "null pointer");
    SCAIL_REQUIRE(M >= 1 && M < (1ll << 31), "M must be >= 1");
    SCAIL_REQUIRE(N > 0 && N % 128 == 0 && N < (1ll << 31), "N must be a positive multiple of 128");
    SCAIL_REQUIRE(K > 0 && K % 128 == 0 && K < (1ll << 31), "K must be a positive multiple of 128");
    SCAIL_REQUIRE(lda >= K && lda % 16 == 0 && ldc >= N && ldc % 4 == 0, "lda must be >= K and a multiple of 16, ldc >= N and a multiple of 4");
    SCAIL_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(sw) & 15) == 0 && (reinterpret_cast<uintptr_t>(sx) & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(y) & 7) == 0 && (reinterpret_cast<uintptr_t>(bias) & 15) == 0,
                  "pointer alignment (x, w, sw, bias 16 B; y 8 B; sx 4 B)");
    if (epilogue == SCAIL_EPI_RESID) {
        SCAIL_REQUIRE(resid != nullptr && ldr % 4 == 0 && (reinterpret_cast<uintptr_t>(resid) & 7) == 0, "RESID epilogue needs resid with ldr % 4 == 0");
        SCAIL_REQUIRE(gate == nullptr || (rows_per_batch > 0 && gate_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(gate) & 15) == 0),
                      "gate needs rows_per_batch > 0, gate_stride % 4 == 0");
    }
    GemmFp8Params P;
    GemmParams& p = P.e;
    p.x = nullptr; p.lda = lda; p.w = nullptr; p.bias = bias;
    p.y = reinterpret_cast<u16*>(y); p.ldc = ldc;
    p.M = (int)M; p.N = (int)N; p.K = (int)K;
    p.resid = reinterpret_cast<const u16*>(resid); p.ldr = ldr; p.gate = gate; p.gate_stride = gate_stride; p.rows_per_batch = rows_per_batch;
    p.group_m = F8_GROUP_M;
    P.x = x; P.w = w; P.sx = sx; P.sw = sw;
    P.ex = nullptr; P.ew = nullptr; P.ldex = 0;
    hipStream_t s = (hipStream_t)stream;
    switch (epilogue) {
        case SCAIL_EPI_BIAS: return launch_gemm_fp8<SCAIL_EPI_BIAS, false>(P, s);
        case SCAIL_EPI_GELU_TANH: return launch_gemm_fp8<SCAIL_EPI_GELU_TANH, false>(P, s);
        case SCAIL_EPI_RESID: return launch_gemm_fp8<SCAIL_EPI_RESID, false>(P, s);
        default:
            scail_set_error("scail_gemm_fp8: epilogue must be SCAIL_EPI_BIAS, SCAIL_EPI_GELU_TANH or SCAIL_EPI_RESID");
            return 1;
    }
}

extern "C" int scail_gemm_mxfp8(const uint8_t* x, int64_t lda, const uint8_t* ex, int64_t ldex, const uint8_t* w, const uint8_t* ew,
                                const float* bias, scail_bf16* y, int64_t ldc, int64_t M, int64_t N, int64_t K, int epilogue,
                                const scail_bf16* resid, int64_t ldr, const float* gate, int64_t gate_stride, int64_t rows_per_batch,
                                void* stream) {
    SCAIL_REQUIRE(x != nullptr && ex != nullptr && w != nullptr && ew != nullptr && y != nullptr, "null pointer");
    SCAIL_REQUIRE(M >= 1 && M < (1ll << 31), "M must be >= 1");
    SCAIL_REQUIRE(N > 0 && N % 128 == 0 && N < (1ll << 31), "N must be a positive multiple of 128");
    SCAIL_REQUIRE(K > 0 && K % 128 == 0 && K < (1ll << 31), "K must be a positive multiple of 128");
    SCAIL_REQUIRE(lda >= K && lda % 16 == 0 && ldc >= N && ldc % 4 == 0, "lda must be >= K and a multiple of 16, ldc >= N and a multiple of 4");
    SCAIL_REQUIRE(ldex >= K / 32 && ldex % 4 == 0, "ldex must be >= K / 32 and a multiple of 4");
    SCAIL_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(ex) & 3) == 0 && (reinterpret_cast<uintptr_t>(ew) & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(y) & 7) == 0 && (reinterpret_cast<uintptr_t>(bias) & 15) == 0,
                  "pointer alignment (x, w, bias 16 B; y 8 B; ex, ew 4 B)");
    if (epilogue == SCAIL_EPI_RESID) {
        SCAIL_REQUIRE(resid != nullptr && ldr % 4 == 0 && (reinterpret_cast<uintptr_t>(resid) & 7) == 0, "RESID epilogue needs resid with ldr % 4 == 0");
        SCAIL_REQUIRE(gate == nullptr || (rows_per_batch > 0 && gate_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(gate) & 15) == 0),
                      "gate needs rows_per_batch > 0, gate_stride % 4 == 0");
    }
    GemmFp8Params P;
    GemmParams& p = P.e;
    p.x = nullptr; p.lda = lda; p.w = nullptr; p.bias = bias;
    p.y = reinterpret_cast<u16*>(y); p.ldc = ldc;
    p.M = (int)M; p.N = (int)N; p.K = (int)K;
    p.resid = reinterpret_cast<const u16*>(resid); p.ldr = ldr; p.gate = gate; p.gate_stride = gate_stride; p.rows_per_batch = rows_per_batch;
    p.group_m = F8_GROUP_M;
    P.x = x; P.w = w; P.sx = nullptr; P.sw = nullptr;
    P.ex = ex; P.ew = ew; P.ldex = ldex;
    hipStream_t s = (hipStream_t)stream;
    switch (epilogue) {
        case SCAIL_EPI_BIAS: return launch_gemm_fp8<SCAIL_EPI_BIAS, true>(P, s);
        case SCAIL_EPI_GELU_TANH: return launch_gemm_fp8<SCAIL_EPI_GELU_TANH, true>(P, s);
        case SCAIL_EPI_RESID: return launch_gemm_fp8<SCAIL_EPI_RESID, true>(P, s);
        default:
            scail_set_error("scail_gemm_mxfp8: epilogue must be SCAIL_EPI_BIAS, SCAIL_EPI_GELU_TANH or SCAIL_EPI_RESID");
            return 1;
    }
}

// ---- MXFP6 GEMM (include/scail_hip.h scail_gemm_mxfp6) ---------------------------------------------------------------------------------
// The MX kernel above on packed e2m3 operands (cbsz = blgp = 2: the MFMA reads 6 registers per operand and takes half the e4m3 form's
// cycles).  Same 256 x 256 tile, 8 waves, wave tile 128(m) x 64(n), LDS-DMA two k-tiles deep, one barrier per k-tile, the same scale
// stage (a k-tile of 128 elements is still one aligned scale dword per row) and the same epilogue.  What differs:
//   Rows of a k-tile are 96 bytes = 6 chunks of 16.  A tile is 24 KB = 24 DMA pieces of 1 KB (3 per wave and operand): lane l of piece p
//   fills the 16-byte slot 64 p + l of the tile = chunk slot % 6 of row slot / 6 (the LDS image stays lane-linear; rows are 96 bytes
//   apart, unpadded).  LDS: 2 x 2 x 24 KB of tiles + 4 KB of scale dwords = 100 KB.
//   Operand layout, found on the device (one code and one raised scale byte at a time): code j of a lane's 32 sits in bits [6 j, 6 j + 6)
//   of its 6 registers, lane (r, g) holds 32 consecutive k of row r, A and B alike, and its scale operand applies to exactly those 32
//   codes.  So a lane's fragment is one whole block, the 24 bytes at 24 b of the row's 96, and its scale is that block's byte: no
//   dealing of halves as in the e4m3 form.
//   24 bytes at a 24-byte pitch are not 16-byte aligned for odd b.  Step ks of lane half g takes block b = ks + 2 g (not 2 ks + g): the
//   parity of b is then the same in every lane of an instruction, even blocks are read as ds_read_b128 (chunk 3 g) + ds_read_b64 (first
//   half of chunk 3 g + 1), odd blocks as ds_read_b64 (second half of chunk 3 g + 1) + ds_read_b128 (chunk 3 g + 2): every read is
//   naturally aligned and the register order is fixed at compile time.  A and B use the same assignment, and each block meets its own
//   scale byte.
//   Bank conflicts: 16-byte slot 6 r + c of the tile, so the rows of a ds_read_b128 lane group ({0-3, 12-15, 20-27} or {4-11, 16-19,
//   28-31}) fall on the 8 even or the 8 odd slots of the 256-byte bank row twice over.  Storing chunk c of row r at c ^ ((r >> 4) & 1)
//   (on the DMA's per-lane source address and on the reads) moves the rows 16 .. 31 to the other parity: conflict-free.  The 8-byte
//   reads stay 2-way (rows r and r + 8 share a bank and 16-byte granularity leaves the half fixed): 4 LDS cycles like a b128, 8 per
//   fragment, what the e4m3 form spends on its 32 bytes.
//   The k-tile is 128 elements.  A 256-element k-tile (the MFMA cycles per barrier of the e4m3 kernel) was not built or measured.
#define F6_BKB 96      // bytes of a row's k-tile
template <int EPI>
__global__ __launch_bounds__(512) void scail_gemm_fp6_kernel(GemmFp8Params P) {
    constexpr int BM = 256, BN = 256, WN = 4, NT = 512;
    constexpr int WTM = 128, WTN = 64, MI = WTM / 32, NI = WTN / 32;
    extern __shared__ __attribute__((aligned(16))) u8 smem8[];
    u8* Xs = smem8;                    // [2][BM][F6_BKB]
    u8* Ws = smem8 + 2 * BM * F6_BKB;  // [2][BN][F6_BKB]
    uint32_t* Ss = reinterpret_cast<uint32_t*>(smem8 + 2 * (BM + BN) * F6_BKB);   // [2][BM + BN] scale dwords of the k-tile
    const GemmParams& p = P.e;

    // ---- tile mapping: as scail_gemm_fp8_kernel ----
    const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
    const int nb = tiles_m * tiles_n;
    int wg;
    {
        const int id = blockIdx.x;
        const int q = nb >> 3, r = nb & 7, xcd = id & 7, loc = id >> 3;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    const int in_group = F8_GROUP_M * tiles_n;
    const int gid = wg / in_group;
    const int first_m = gid * F8_GROUP_M;
    const int gsz = min(tiles_m - first_m, F8_GROUP_M);
    const int pid_m = first_m + (wg % in_group) % gsz;
    const int pid_n = (wg % in_group) / gsz;
    const int m0 = pid_m * BM, n0 = pid_n * BN;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, g = lane >> 5;

    // LDS-DMA pieces: piece j of an operand = slots 64 j .. 64 j + 63 of the tile.  Rows past M / N read the last row.
    static_assert(BM * F6_BKB % (1024 * (NT / 64)) == 0 && BM == BN, "whole pieces per wave");
    constexpr int PC = BM * F6_BKB / 1024 / (NT / 64);     // 3
    const int64_t ldw = (int64_t)p.K / 4 * 3;
    const u8* srcx[PC];
    const u8* srcw[PC];
#pragma unroll
    for (int i = 0; i < PC; ++i) {
        const int slot = 64 * (wave * PC + i) + lane, r = slot / 6, c = (slot - 6 * r) ^ ((r >> 4) & 1);
        srcx[i] = P.x + (int64_t)min(m0 + r, p.M - 1) * p.lda + (c << 4);
        srcw[i] = P.w + (int64_t)min(n0 + r, p.N - 1) * ldw + (c << 4);
    }
#define F6_DMA(kb_, buf_)                                                                                                     \
    {                                                                                                                         \
        _Pragma("unroll") for (int i_ = 0; i_ < PC; ++i_) {                                                                   \
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(srcx[i_] + (kb_)),              \
                (__attribute__((address_space(3))) void*)(Xs + (buf_) * BM * F6_BKB + 1024 * (wave * PC + i_)), 16, 0, 0);     \
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(srcw[i_] + (kb_)),              \
                (__attribute__((address_space(3))) void*)(Ws + (buf_) * BN * F6_BKB + 1024 * (wave * PC + i_)), 16, 0, 0);     \
        }                                                                                                                     \
    }
    // fragment-read byte offsets in this lane's row: step 0 reads block 2 g as chunk 3 g + the first half of chunk 3 g + 1, step 1
    // block 2 g + 1 as the second half of chunk 3 g + 1 + chunk 3 g + 2; chunks swizzled by the row's bit 4 (= l31's: fragment rows
    // start at multiples of 32)
    const int fsw = (l31 >> 4) & 1;
    const int off_q0 = ((3 * g) ^ fsw) << 4, off_d = ((3 * g + 1) ^ fsw) << 4, off_q1 = ((3 * g + 2) ^ fsw) << 4;

    f32x16 acc[NI][MI];
#pragma unroll
    for (int a = 0; a < NI; ++a)
#pragma unroll
        for (int b = 0; b < MI; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

    const int nk = p.K / F8_BK;
    static_assert(BM == 256 && BN == 256 && NT == 512, "one scale row per thread");
    const u8* srcs;
    {
        const int r = (wave & 3) * 64 + lane;
        srcs = wave < 4 ? P.ex + (int64_t)min(m0 + r, p.M - 1) * P.ldex : P.ew + (int64_t)min(n0 + r, p.N - 1) * (p.K / 32);
    }
#define F6_SCALE_DMA(t_, buf_)                                                                                             \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(srcs + 4 * (t_)),                    \
        (__attribute__((address_space(3))) void*)(Ss + (buf_) * (BM + BN) + 64 * wave), 4, 0, 0);
    F6_SCALE_DMA(0, 0)
    F6_DMA(0, 0)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
        const int cur = t & 1;
        if (t + 1 < nk) {
            F6_DMA((t + 1) * F6_BKB, cur ^ 1)
            F6_SCALE_DMA(t + 1, cur ^ 1)
        }
        uint32_t sc[NI + MI];          // the scale dwords of this lane's fragment rows, W then x
#pragma unroll
        for (int i = 0; i < NI; ++i) sc[i] = Ss[cur * (BM + BN) + BM + wn * WTN + i * 32 + l31];
#pragma unroll
        for (int i = 0; i < MI; ++i) sc[NI + i] = Ss[cur * (BM + BN) + wm * WTM + i * 32 + l31];
        const u8* xs = Xs + (cur * BM + wm * WTM + l31) * F6_BKB;
        const u8* ws = Ws + (cur * BN + wn * WTN + l31) * F6_BKB;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            i32x8 wf[NI], xf[MI];
#pragma unroll
            for (int i = 0; i < NI + MI; ++i) {
                const u8* row = i < NI ? ws + i * 32 * F6_BKB : xs + (i - NI) * 32 * F6_BKB;
                const uint4 q4 = *reinterpret_cast<const uint4*>(row + (ks == 0 ? off_q0 : off_q1));
                const uint2 d2 = *reinterpret_cast<const uint2*>(row + off_d + 8 * ks);
                const i32x8 fr = ks == 0 ? i32x8{(int)q4.x, (int)q4.y, (int)q4.z, (int)q4.w, (int)d2.x, (int)d2.y, 0, 0}
                                         : i32x8{(int)d2.x, (int)d2.y, (int)q4.x, (int)q4.y, (int)q4.z, (int)q4.w, 0, 0};
                if (i < NI) wf[i] = fr; else xf[i - NI] = fr;
            }
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
                    acc[ni][mi] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[ni], xf[mi], acc[ni][mi], 2, 2, 0,
                                                                                 (int)((sc[ni] >> (8 * ks + 16 * g)) & 0xffu), 0,
                                                                                 (int)((sc[NI + mi] >> (8 * ks + 16 * g)) & 0xffu));
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
#undef F6_DMA
#undef F6_SCALE_DMA
    gemm_epilogue<EPI, MI, NI, WTM, WTN>(acc, p, m0, n0, wm, wn, l31, g);
}

template <int EPI>
static int launch_gemm_fp6(const GemmFp8Params& P, hipStream_t stream) {
    constexpr int lds = 2 * (256 + 256) * F6_BKB + 2 * (256 + 256) * 4;   // 96 KB + 4 KB of staged block scales
    const int tiles = ((P.e.M + 255) / 256) * ((P.e.N + 255) / 256);
    return scail_launch_lds<scail_gemm_fp6_kernel<EPI>>("scail_gemm_mxfp6", lds, dim3((unsigned)tiles), dim3(512), lds, stream, P);
}

extern "C" int scail_gemm_mxfp6(const uint8_t* x, int64_t lda, const uint8_t* ex, int64_t ldex, const uint8_t* w, const uint8_t* ew,
                                const float* bias, scail_bf16* y, int64_t ldc, int64_t M, int64_t N, int64_t K, int epilogue,
                                const scail_bf16* resid, int64_t ldr, const float* gate, int64_t gate_stride, int64_t rows_per_batch,
                                void* stream) {
    SCAIL_REQUIRE(x != nullptr && ex != nullptr && w != nullptr && ew != nullptr && y != nullptr, "null pointer");
    SCAIL_REQUIRE(M >= 1 && M < (1ll << 31), "M must be >= 1");
    SCAIL_REQUIRE(N > 0 && N % 128 == 0 && N < (1ll << 31), "N must be a positive multiple of 128");
    SCAIL_REQUIRE(K > 0 && K % 128 == 0 && K < (1ll << 31), "K must be a positive multiple of 128");
    SCAIL_REQUIRE(lda >= K / 4 * 3 && lda % 16 == 0 && ldc >= N && ldc % 4 == 0,
                  "lda (bytes) must be >= 3 * K / 4 and a multiple of 16, ldc >= N and a multiple of 4");
    SCAIL_REQUIRE(ldex >= K / 32 && ldex % 4 == 0, "ldex must be >= K / 32 and a multiple of 4");
    SCAIL_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(ex) & 3) == 0 && (reinterpret_cast<uintptr_t>(ew) & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(y) & 7) == 0 && (reinterpret_cast<uintptr_t>(bias) & 15) == 0,
                  "pointer alignment (x, w, bias 16 B; y 8 B; ex, ew 4 B)");
    if (epilogue == SCAIL_EPI_RESID) {
        SCAIL_REQUIRE(resid != nullptr && ldr % 4 == 0 && (reinterpret_cast<uintptr_t>(resid) & 7) == 0, "RESID epilogue needs resid with ldr % 4 == 0");
        SCAIL_REQUIRE(gate == nullptr || (rows_per_batch > 0 && gate_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(gate) & 15) == 0),
                      "gate needs rows_per_batch > 0, gate_stride % 4 == 0");
    }
    GemmFp8Params P;
    GemmParams& p = P.e;
    p.x = nullptr; p.lda = lda; p.w = nullptr; p.bias = bias;
    p.y = reinterpret_cast<u16*>(y); p.ldc = ldc;
    p.M = (int)M; p.N = (int)N; p.K = (int)K;
    p.resid = reinterpret_cast<const u16*>(resid); p.ldr = ldr; p.gate = gate; p.gate_stride = gate_stride; p.rows_per_batch = rows_per_batch;
    p.group_m = F8_GROUP_M;
    P.x = x; P.w = w; P.sx = nullptr; P.sw = nullptr;
    P.ex = ex; P.ew = ew; P.ldex = ldex;
    hipStream_t s = (hipStream_t)stream;
    switch (epilogue) {
        case SCAIL_EPI_BIAS: return launch_gemm_fp6<SCAIL_EPI_BIAS>(P, s);
        case SCAIL_EPI_GELU_TANH: return launch_gemm_fp6<SCAIL_EPI_GELU_TANH>(P, s);
        case SCAIL_EPI_RESID: return launch_gemm_fp6<SCAIL_EPI_RESID>(P, s);
        default:
            scail_set_error("scail_gemm_mxfp6: epilogue must be SCAIL_EPI_BIAS, SCAIL_EPI_GELU_TANH or SCAIL_EPI_RESID");
            return 1;
    }
}
