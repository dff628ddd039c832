// Request preprocessing (include/scail_hip.h scail_resize_crop_aa / scail_pose_half; scail_amd/preprocess.py *_hip): the antialiased
// bicubic resize + centre crop of the driving video and the reference image (data_video.py:141-170), and the [-1, 1] normalisation +
// 0.5x bilinear of the pose frames (sample_video.py:340-351).
#include "common.h"

#include <math.h>

// ---- separable antialiased bicubic resize, fused with the crop window ----
// One workgroup = RS_TW threads = an RS_TH x RS_TW tile of the output window, every channel.  Thread t owns output column t of the tile:
// it walks the input rows the tile's output rows touch, reduces each row horizontally with its column's weights (fp32, the
// intermediate of the two 1-D passes) and adds the result into the accumulators of the output rows whose vertical support holds that
// input row -- in ascending input row, so every output is the plain left-to-right sum of its taps.  No intermediate image exists in
// memory.  The weights are evaluated HERE, in fp64, once per workgroup (columns: one thread each; rows: the first RS_TH threads), and
// rounded to fp32 after the normalisation: the coordinates of a 1920- or 2160-pixel axis do not survive fp32.
#define RS_TW 64
#define RS_TH 8

struct ResizeArgs {
    double sh, sw;              // in / out per axis
    int64_t src_frame, dst_frame;   // elements per frame: Hin * Win * C, C * Hout * Wout
    int Hin, Win, Hout, Wout, top, left;
    int kh, kw;                 // tap budget per axis: floor(4 * max(s, 1)) + 1, at most `in`
    int row_tiles, col_tiles;
};

// Keys' cubic, a = -0.5
__device__ __forceinline__ double cubic_aa(double x) {
    x = fabs(x);
    if (x < 1.0) return (1.5 * x - 2.5) * x * x + 1.0;
    if (x < 2.0) return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0;
    return 0.0;
}

// taps [j0, j0 + cnt) and normalised weights w[k * stride] of output index i (in the resized image) of an axis with `in` samples
__device__ __forceinline__ void axis_weights(int i, double s, int in, int kmax, int& j0, int& cnt, float* w, int stride) {
    const double sc = s > 1.0 ? s : 1.0, sup = 2.0 * sc, c = s * ((double)i + 0.5);
    int lo = (int)floor(c - sup + 0.5), hi = (int)floor(c + sup + 0.5);
    lo = lo < 0 ? 0 : lo;
    hi = hi > in ? in : hi;
    j0 = lo;
    cnt = hi - lo;
    cnt = cnt > kmax ? kmax : cnt;          // (the host's budget already covers it; the table is never overrun)
    double tot = 0.0;
    for (int k = 0; k < cnt; ++k) tot += cubic_aa(((double)(lo + k) - c + 0.5) / sc);
    for (int k = 0; k < cnt; ++k) w[k * stride] = (float)(cubic_aa(((double)(lo + k) - c + 0.5) / sc) / tot);
}

// SrcT = uint8_t: channels-last (n, Hin, Win, C), result rounded half-to-even and clamped to [0, 255];  float: planar (n, C, Hin, Win)
template <typename SrcT, int C>
__global__ void __launch_bounds__(RS_TW) resize_crop_aa_kernel(const SrcT* __restrict__ src, float* __restrict__ dst, ResizeArgs a) {
    extern __shared__ float rs_lds[];
    float* ww = rs_lds;                           // [kw][RS_TW]: tap k of column t at ww[k * RS_TW + t]
    float* wv = ww + a.kw * RS_TW;                // [RS_TH][kh]
    int* yinfo = (int*)(wv + RS_TH * a.kh);       // first tap, tap count of each output row of the tile
    const int tid = threadIdx.x;
    int64_t b = blockIdx.x;
    const int ct = (int)(b % a.col_tiles);
    b /= a.col_tiles;
    const int rt = (int)(b % a.row_tiles);
    const int64_t n = b / a.row_tiles;

    const int ox = ct * RS_TW + tid;
    int x0 = 0, xc = 0;
    if (ox < a.Wout) axis_weights(ox + a.left, a.sw, a.Win, a.kw, x0, xc, ww + tid, RS_TW);
    if (tid < RS_TH) {
        const int oy = rt * RS_TH + tid;
        int y0 = 0, yc = 0;
        if (oy < a.Hout) axis_weights(oy + a.top, a.sh, a.Hin, a.kh, y0, yc, wv + tid * a.kh, 1);
        yinfo[tid] = y0;
        yinfo[RS_TH + tid] = yc;
    }
    __syncthreads();

    int y0r[RS_TH], ycr[RS_TH];
    int ylo = 0, yhi = 0;
#pragma unroll
    for (int r = 0; r < RS_TH; ++r) {             // workgroup-uniform: kept in scalar registers
        y0r[r] = __builtin_amdgcn_readfirstlane(yinfo[r]);
        ycr[r] = __builtin_amdgcn_readfirstlane(yinfo[RS_TH + r]);
        if (r == 0) ylo = y0r[0];
        if (ycr[r] > 0 && y0r[r] + ycr[r] > yhi) yhi = y0r[r] + ycr[r];
    }

    float acc[RS_TH][C];
#pragma unroll
    for (int r = 0; r < RS_TH; ++r)
#pragma unroll
        for (int ch = 0; ch < C; ++ch) acc[r][ch] = 0.0f;

    const SrcT* frame = src + n * a.src_frame;
    const int64_t plane = (int64_t)a.Hin * a.Win;
    for (int y = ylo; y < yhi; ++y) {
        float h[C];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) h[ch] = 0.0f;
        if constexpr (sizeof(SrcT) == 1) {
            const SrcT* p = frame + ((int64_t)y * a.Win + x0) * C;
            for (int k = 0; k < xc; ++k) {
                const float w = ww[k * RS_TW + tid];
#pragma unroll
                for (int ch = 0; ch < C; ++ch) h[ch] = fmaf(w, (float)p[k * C + ch], h[ch]);
            }
        } else {
            const SrcT* p = frame + (int64_t)y * a.Win + x0;
            for (int k = 0; k < xc; ++k) {
                const float w = ww[k * RS_TW + tid];
#pragma unroll
                for (int ch = 0; ch < C; ++ch) h[ch] = fmaf(w, (float)p[ch * plane + k], h[ch]);
            }
        }
#pragma unroll
        for (int r = 0; r < RS_TH; ++r) {
            const int k = y - y0r[r];
            if (k >= 0 && k < ycr[r]) {
                const float w = wv[r * a.kh + k];
#pragma unroll
                for (int ch = 0; ch < C; ++ch) acc[r][ch] = fmaf(w, h[ch], acc[r][ch]);
            }
        }
    }

    if (ox >= a.Wout) return;
    float* out = dst + n * a.dst_frame;
#pragma unroll
    for (int r = 0; r < RS_TH; ++r) {
        const int oy = rt * RS_TH + r;
        if (oy >= a.Hout) break;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            float v = acc[r][ch];
            if constexpr (sizeof(SrcT) == 1) v = fminf(fmaxf(rintf(v), 0.0f), 255.0f);     // the uint8 round trip of the reference's resize
            out[((int64_t)ch * a.Hout + oy) * a.Wout + ox] = v;
        }
    }
}

template <typename SrcT>
static void resize_launch(const void* src, float* dst, const ResizeArgs& a, int C, unsigned grid, size_t lds, hipStream_t st) {
    const SrcT* s = (const SrcT*)src;
    switch (C) {
        case 1: hipLaunchKernelGGL((resize_crop_aa_kernel<SrcT, 1>), dim3(grid), dim3(RS_TW), lds, st, s, dst, a); break;
        case 2: hipLaunchKernelGGL((resize_crop_aa_kernel<SrcT, 2>), dim3(grid), dim3(RS_TW), lds, st, s, dst, a); break;
        case 3: hipLaunchKernelGGL((resize_crop_aa_kernel<SrcT, 3>), dim3(grid), dim3(RS_TW), lds, st, s, dst, a); break;
        default: hipLaunchKernelGGL((resize_crop_aa_kernel<SrcT, 4>), dim3(grid), dim3(RS_TW), lds, st, s, dst, a); break;
    }
}

static std::string i2s(int64_t v) { return std::to_string(v); }

extern "C" int scail_resize_crop_aa(const void* src, int src_kind, float* dst, int64_t n, int64_t C, int64_t Hin, int64_t Win,
                                    int64_t Hr, int64_t Wr, int64_t top, int64_t left, int64_t Hout, int64_t Wout, void* stream) {
    SCAIL_REQUIRE(src != nullptr && dst != nullptr, "null pointer");
    SCAIL_REQUIRE(src_kind == SCAIL_SRC_U8_NHWC || src_kind == SCAIL_SRC_F32_NCHW, "unknown source kind " + i2s(src_kind));
    SCAIL_REQUIRE(C >= 1 && C <= 4, "C must be 1..4, got " + i2s(C));
    SCAIL_REQUIRE(n >= 0, "negative image count n = " + i2s(n));
    SCAIL_REQUIRE(Hin >= 1 && Win >= 1 && Hr >= 1 && Wr >= 1 && Hout >= 1 && Wout >= 1,
                  "sizes must be positive, got source " + i2s(Hin) + " x " + i2s(Win) + ", resized " + i2s(Hr) + " x " + i2s(Wr) + ", window " +
                      i2s(Hout) + " x " + i2s(Wout));
    SCAIL_REQUIRE(top >= 0 && left >= 0 && Hout <= Hr - top && Wout <= Wr - left,
                  "the window [" + i2s(top) + ", " + i2s(top) + " + " + i2s(Hout) + ") x [" + i2s(left) + ", " + i2s(left) + " + " + i2s(Wout) +
                      ") is outside the resized image " + i2s(Hr) + " x " + i2s(Wr));
    SCAIL_REQUIRE(Hin <= SCAIL_RESIZE_MAX_SCALE * Hr, "the vertical scale " + i2s(Hin) + " / " + i2s(Hr) + " is above the cap of " +
                                                          i2s(SCAIL_RESIZE_MAX_SCALE) + " (the kernel's tap budget)");
    SCAIL_REQUIRE(Win <= SCAIL_RESIZE_MAX_SCALE * Wr, "the horizontal scale " + i2s(Win) + " / " + i2s(Wr) + " is above the cap of " +
                                                          i2s(SCAIL_RESIZE_MAX_SCALE) + " (the kernel's tap budget)");
    SCAIL_REQUIRE(Hin < (1ll << 24) && Win < (1ll << 24) && Hr < (1ll << 24) && Wr < (1ll << 24) && Hin * Win * C < (1ll << 31) &&
                      C * Hout * Wout < (1ll << 31),
                  "a frame must hold fewer than 2^31 samples, got source " + i2s(Hin) + " x " + i2s(Win) + " x " + i2s(C));
    const int64_t row_tiles = (Hout + RS_TH - 1) / RS_TH, col_tiles = (Wout + RS_TW - 1) / RS_TW;
    SCAIL_REQUIRE(n == 0 || row_tiles * col_tiles < (1ll << 31) / n, "too many tiles for one launch, n = " + i2s(n));
    if (n == 0) return 0;
    ResizeArgs a;
    a.sh = (double)Hin / (double)Hr;
    a.sw = (double)Win / (double)Wr;
    a.src_frame = Hin * Win * C;
    a.dst_frame = C * Hout * Wout;
    a.Hin = (int)Hin; a.Win = (int)Win; a.Hout = (int)Hout; a.Wout = (int)Wout; a.top = (int)top; a.left = (int)left;
    const int64_t kh = (int64_t)floor(4.0 * (a.sh > 1.0 ? a.sh : 1.0)) + 1, kw = (int64_t)floor(4.0 * (a.sw > 1.0 ? a.sw : 1.0)) + 1;
    a.kh = (int)(kh < Hin ? kh : Hin);
    a.kw = (int)(kw < Win ? kw : Win);
    a.row_tiles = (int)row_tiles;
    a.col_tiles = (int)col_tiles;
    const size_t lds = ((size_t)a.kw * RS_TW + (size_t)RS_TH * a.kh + 2 * RS_TH) * 4;      // at most 65 taps per axis: 18.8 KB
    const unsigned grid = (unsigned)(n * row_tiles * col_tiles);
    if (src_kind == SCAIL_SRC_U8_NHWC)
        resize_launch<uint8_t>(src, dst, a, (int)C, grid, lds, (hipStream_t)stream);
    else
        resize_launch<float>(src, dst, a, (int)C, grid, lds, (hipStream_t)stream);
    return scail_check_launch("resize_crop_aa");
}

// ---- pose frames: (x - 127.5) / 127.5 and its 0.5x bilinear, one pass ----
// One thread per half-resolution pixel: the 2 x 2 block as two 8-byte loads.  Every operation is rounded on its own (contraction off,
// as in the tile kernels of rowops.hip), so the normalisation gives the bits of the torch expression it replaces.
__global__ void pose_half_kernel(const float* __restrict__ x, float* __restrict__ half, float* __restrict__ full, int64_t hfs, int64_t hcs,
                                 int C, int H, int W, int64_t total) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int Hh = H >> 1, Wh = W >> 1;
    const int xo = (int)(i % Wh);
    int64_t t = i / Wh;
    const int yo = (int)(t % Hh);
    t /= Hh;
    const int c = (int)(t % C);
    const int64_t f = t / C;
    const int64_t o = ((f * C + c) * H + 2 * yo) * (int64_t)W + 2 * xo;
    const float2 r0 = *reinterpret_cast<const float2*>(x + o), r1 = *reinterpret_cast<const float2*>(x + o + W);
    const float a = (r0.x - 127.5f) / 127.5f, b = (r0.y - 127.5f) / 127.5f;
    const float cc = (r1.x - 127.5f) / 127.5f, d = (r1.y - 127.5f) / 127.5f;
    if (full != nullptr) {
        *reinterpret_cast<float2*>(full + o) = make_float2(a, b);
        *reinterpret_cast<float2*>(full + o + W) = make_float2(cc, d);
    }
    half[f * hfs + c * hcs + (int64_t)yo * Wh + xo] = ((a + b) + (cc + d)) * 0.25f;
}

extern "C" int scail_pose_half(const float* x, float* half, int64_t half_frame_stride, int64_t half_chan_stride, float* full, int64_t n,
                               int64_t C, int64_t H, int64_t W, void* stream) {
    SCAIL_REQUIRE(x != nullptr && half != nullptr, "null pointer");
    SCAIL_REQUIRE(n >= 0 && n < (1ll << 31) && C >= 1 && C < (1ll << 24), "bad counts n = " + i2s(n) + ", C = " + i2s(C));
    SCAIL_REQUIRE(H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "H and W must be even (whole 2 x 2 blocks), got " + i2s(H) + " x " + i2s(W));
    SCAIL_REQUIRE(H < (1ll << 24) && W < (1ll << 24) && C * H * W < (1ll << 31),
                  "a frame must hold fewer than 2^31 samples, got " + i2s(C) + " x " + i2s(H) + " x " + i2s(W));
    const int64_t hw = (H / 2) * (W / 2);
    SCAIL_REQUIRE(half_frame_stride >= hw && half_chan_stride >= hw,
                  "the half-size strides must hold a plane of " + i2s(hw) + " pixels, got frame stride " + i2s(half_frame_stride) +
                      ", channel stride " + i2s(half_chan_stride));
    SCAIL_REQUIRE((uintptr_t)x % 8 == 0 && (uintptr_t)full % 8 == 0, "x and full must be 8-byte aligned (paired loads and stores)");
    const int64_t total = n * C * hw;
    SCAIL_REQUIRE((total + 255) / 256 < (1ll << 31), "too many pixels for one launch, n = " + i2s(n));
    if (total == 0) return 0;
    hipLaunchKernelGGL(pose_half_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, half, full,
                       half_frame_stride, half_chan_stride, (int)C, (int)H, (int)W, total);
    return scail_check_launch("pose_half");
}
