// k_pyramid.hip -- cv2.pyrDown of 8-bit BGR frames (the one documented use of CaptureReaderBase.downsample,
// core/vmanager.py:484-498), alone and fused behind the I420 conversion of the file reader.
//
//   dst[y, x] = (sum_{i,j in -2..2} k[i] k[j] src[r(2y+i), r(2x+j)] + 128) >> 8,  k = 1 4 6 4 1,  r = BORDER_REFLECT_101
//
// Integer only and exact (largest sum 255 * 256: no clamp).  HBM-bound: the BGR kernel reads 3 B and writes 0.75 B per
// source pixel; the fused kernel reads 1.5 B (I420) and writes 0.75 B, the full-size BGR frame never exists.
//
// One workgroup = PT_W x PT_H output pixels (64 x 16).  Three steps with a barrier between them:
//   1. stage   the source tile plus its halo as BGR bytes in LDS.  The staged window starts at source column
//              2*x0 - 4 and row 2*y0 - 2: two columns more than the filter needs on the left, so that the window starts
//              on a dword of the row (and, for I420, on a chroma sample).  An INTERIOR tile of the dword form loads
//              dwords with no reflect arithmetic; a rim tile, and every tile of the narrow form, loads bytes through
//              reflect_101.
//   2. rows    1 4 6 4 1 along x, decimated: one item = 4 output pixels of one staged row (nine LDS dwords in, twelve
//              16-bit sums out, at most 4080).
//   3. columns 1 4 6 4 1 along y, decimated, + 128 >> 8: one item = 4 output bytes of one output row, packed into a
//              dword store (dword form) or written byte by byte with bounds checks (narrow form).
// The dword form needs w % 8 == 0 (then both the source rows and the destination rows start on dwords, and so does every
// frame of a batch) and dword-aligned pointers; everything else -- odd widths, batches with h*w*3 odd, offset pointers --
// takes the narrow form.
#include "ck_common.h"
#include "ck_i420.h"

namespace {

constexpr int PT_W = 64, PT_H = 16;                 // output tile
constexpr int PS_ROWS = 2 * PT_H + 4;               // staged source rows (2*PT_H + 3 used; even for the 2x2 chroma blocks)
constexpr int PS_COLS = 2 * PT_W + 8;               // staged source columns (2*PT_W + 5 used; a multiple of 4)
constexpr int PS_ROWB = PS_COLS * 3;                // 408 staged bytes = 102 dwords per row
constexpr int PS_PITCH = PS_ROWB + 4;               // 103 dwords: rows_pass reads 16 lanes per row 6 dwords apart (the even banks);
                                                    // an odd pitch puts the next row's 16 lanes on the odd ones
constexpr int PH_ROWS = 2 * PT_H + 3;               // rows of horizontal sums
constexpr int PH_PITCH = PT_W * 3;                  // 192 ushorts
static_assert(PS_ROWB % 4 == 0 && PS_PITCH % 4 == 0 && (PT_W * 3) % 4 == 0 && PT_W % 4 == 0, "tile rows are whole dwords");

// BORDER_REFLECT_101 for the indices a 5-tap filter at stride 2 reaches (-2 .. n + 1), n >= 2; for n == 2 the index -2
// folds twice (-2 -> 2 -> 0), as cv::borderInterpolate does.  Indices beyond that (staged, but only read for outputs
// that are not stored) are clamped into the image.
__device__ __forceinline__ int reflect_101(int i, int n)
{
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// the staged window of tile (x0, y0) lies inside the h x w source with room for its last, partly unused dword
__device__ __forceinline__ bool tile_is_interior(int x0, int y0, int h, int w)
{
    return 2 * x0 - 4 >= 0 && 2 * x0 - 4 + PS_COLS <= w && 2 * y0 - 2 >= 0 && 2 * y0 - 2 + PS_ROWS <= h;
}

// step 2
__device__ __forceinline__ void rows_pass(const uint8_t* __restrict__ s, uint16_t* __restrict__ hs)
{
    for (int it = threadIdx.x; it < PH_ROWS * (PT_W / 4); it += blockDim.x) {
        const int r = it / (PT_W / 4), q = it - r * (PT_W / 4);
        // output pixel 4q + p, tap j (0..4), channel c reads staged column 8q + 2p + 2 + j: byte 24q + 6 + 6p + 3j + c
        const uint32_t* d4 = reinterpret_cast<const uint32_t*>(s + r * PS_PITCH + 24 * q + 4);
        uint32_t d[9];
#pragma unroll
        for (int k = 0; k < 9; k++) d[k] = d4[k];
        auto B = [&](int i) { return (d[i >> 2] >> (8 * (i & 3))) & 255u; };
        uint32_t o[6];
#pragma unroll
        for (int e = 0; e < 12; e++) {
            const int b = 2 + 6 * (e / 3) + (e % 3);
            const uint32_t v = B(b) + 4 * B(b + 3) + 6 * B(b + 6) + 4 * B(b + 9) + B(b + 12);
            if (e & 1) o[e >> 1] |= v << 16; else o[e >> 1] = v;
        }
        uint32_t* o4 = reinterpret_cast<uint32_t*>(hs + r * PH_PITCH + 12 * q);
#pragma unroll
        for (int k = 0; k < 6; k++) o4[k] = o[k];
    }
}

// step 3.  dst: the frame's output, oh x ow x 3
template <bool WIDE>
__device__ __forceinline__ void cols_pass(const uint16_t* __restrict__ hs, uint8_t* __restrict__ dst, int x0, int y0,
                                          int oh, int ow, bool interior)
{
    for (int it = threadIdx.x; it < PT_H * (PT_W * 3 / 4); it += blockDim.x) {
        const int y = it / (PT_W * 3 / 4), d = it - y * (PT_W * 3 / 4);
        uint32_t acc[4] = {128, 128, 128, 128};
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const uint2 v = *reinterpret_cast<const uint2*>(hs + (2 * y + k) * PH_PITCH + 4 * d);
            const uint32_t wgt = k == 0 || k == 4 ? 1 : (k == 2 ? 6 : 4);
            acc[0] += wgt * (v.x & 0xffffu); acc[1] += wgt * (v.x >> 16);
            acc[2] += wgt * (v.y & 0xffffu); acc[3] += wgt * (v.y >> 16);
        }
        const int oy = y0 + y;
        const size_t row = ((size_t)oy * ow + x0) * 3;
        if constexpr (WIDE) {
            // ow % 4 == 0 and x0 % 4 == 0: a dword of the tile row lies wholly inside the output row or wholly outside
            if (interior || (oy < oh && x0 * 3 + 4 * d < ow * 3))
                *reinterpret_cast<uint32_t*>(dst + row + 4 * d) =
                    (acc[0] >> 8) | ((acc[1] >> 8) << 8) | ((acc[2] >> 8) << 16) | ((acc[3] >> 8) << 24);
        } else {
            if (oy < oh) {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (x0 * 3 + 4 * d + k < ow * 3) dst[row + 4 * d + k] = (uint8_t)(acc[k] >> 8);
            }
        }
    }
}

template <bool WIDE>
__global__ __launch_bounds__(256) void pyr_down_kernel(const uint8_t* __restrict__ src, int h, int w,
                                                       uint8_t* __restrict__ dst, int oh, int ow)
{
    __shared__ __attribute__((aligned(16))) uint8_t s[PS_ROWS * PS_PITCH];
    __shared__ __attribute__((aligned(16))) uint16_t hs[PH_ROWS * PH_PITCH];
    const int x0 = blockIdx.x * PT_W, y0 = blockIdx.y * PT_H;
    const uint8_t* f = src + (size_t)blockIdx.z * h * w * 3;
    const int sx = 2 * x0 - 4, sy = 2 * y0 - 2;
    const bool interior = WIDE && tile_is_interior(x0, y0, h, w);
    if (interior) {
        for (int it = threadIdx.x; it < PH_ROWS * (PS_ROWB / 4); it += blockDim.x) {
            const int r = it / (PS_ROWB / 4), d = it - r * (PS_ROWB / 4);
            reinterpret_cast<uint32_t*>(s + r * PS_PITCH)[d] =
                reinterpret_cast<const uint32_t*>(f + ((size_t)(sy + r) * w + sx) * 3)[d];
        }
    } else {
        for (int it = threadIdx.x; it < PH_ROWS * PS_ROWB; it += blockDim.x) {
            const int r = it / PS_ROWB, b = it - r * PS_ROWB;
            const int c = b / 3;
            s[r * PS_PITCH + b] = f[((size_t)reflect_101(sy + r, h) * w + reflect_101(sx + c, w)) * 3 + (b - 3 * c)];
        }
    }
    __syncthreads();
    rows_pass(s, hs);
    __syncthreads();
    cols_pass<WIDE>(hs, dst + (size_t)blockIdx.z * oh * ow * 3, x0, y0, oh, ow, interior);
}

// n I420 frames -> the first pyramid level of their BGR conversion; h and w even
template <bool WIDE>
__global__ __launch_bounds__(256) void i420_pyr_down_kernel(const uint8_t* __restrict__ src, int h, int w,
                                                            uint8_t* __restrict__ dst, int oh, int ow)
{
    using namespace ck_i420;
    __shared__ __attribute__((aligned(16))) uint8_t s[PS_ROWS * PS_PITCH];
    __shared__ __attribute__((aligned(16))) uint16_t hs[PH_ROWS * PH_PITCH];
    const int x0 = blockIdx.x * PT_W, y0 = blockIdx.y * PT_H;
    const uint8_t* Y = src + (size_t)blockIdx.z * (h * w * 3 / 2);
    const uint8_t* U = Y + (size_t)h * w;
    const uint8_t* V = U + (size_t)(h / 2) * (w / 2);
    const int sx = 2 * x0 - 4, sy = 2 * y0 - 2;            // both even: the window starts on a chroma sample
    const bool interior = WIDE && tile_is_interior(x0, y0, h, w);
    if (interior) {
        // one item = 4 x 2 pixels: two Y dwords, one U and one V ushort in, two times three LDS dwords out
        for (int it = threadIdx.x; it < (PS_ROWS / 2) * (PS_COLS / 4); it += blockDim.x) {
            const int r = it / (PS_COLS / 4), g = it - r * (PS_COLS / 4);
            const int y = sy + 2 * r, x = sx + 4 * g;
            const uint32_t ya[2] = {*reinterpret_cast<const uint32_t*>(Y + (size_t)y * w + x),
                                    *reinterpret_cast<const uint32_t*>(Y + (size_t)(y + 1) * w + x)};
            const uint16_t u2 = *reinterpret_cast<const uint16_t*>(U + (size_t)(y / 2) * (w / 2) + x / 2);
            const uint16_t v2 = *reinterpret_cast<const uint16_t*>(V + (size_t)(y / 2) * (w / 2) + x / 2);
            const Chroma ch[2] = {i420_chroma((uint8_t)u2, (uint8_t)v2), i420_chroma((uint8_t)(u2 >> 8), (uint8_t)(v2 >> 8))};
#pragma unroll
            for (int rr = 0; rr < 2; rr++) {
                uint8_t o[12];
#pragma unroll
                for (int k = 0; k < 4; k++) i420_pixel((uint8_t)(ya[rr] >> (8 * k)), ch[k / 2], o + 3 * k);
                uint32_t* d4 = reinterpret_cast<uint32_t*>(s + (2 * r + rr) * PS_PITCH + 12 * g);
                d4[0] = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24);
                d4[1] = (uint32_t)o[4] | ((uint32_t)o[5] << 8) | ((uint32_t)o[6] << 16) | ((uint32_t)o[7] << 24);
                d4[2] = (uint32_t)o[8] | ((uint32_t)o[9] << 8) | ((uint32_t)o[10] << 16) | ((uint32_t)o[11] << 24);
            }
        }
    } else {
        for (int it = threadIdx.x; it < PH_ROWS * PS_COLS; it += blockDim.x) {
            const int r = it / PS_COLS, c = it - r * PS_COLS;
            const int y = reflect_101(sy + r, h), x = reflect_101(sx + c, w);
            const size_t uv = (size_t)(y / 2) * (w / 2) + x / 2;
            i420_pixel(Y[(size_t)y * w + x], i420_chroma(U[uv], V[uv]), s + r * PS_PITCH + 3 * c);
        }
    }
    __syncthreads();
    rows_pass(s, hs);
    __syncthreads();
    cols_pass<WIDE>(hs, dst + (size_t)blockIdx.z * oh * ow * 3, x0, y0, oh, ow, interior);
}

bool dword_form(const void* a, const void* b, int w)
{
    return (w % 8) == 0 && (((uintptr_t)a | (uintptr_t)b) & 3) == 0;
}

}  // namespace

int k_pyr_down(ck_ctx* ctx, const uint8_t* d_bgr, int n, int h, int w, uint8_t* d_out)
{
    TimeScope ts(ctx, "pyr_down");
    const int oh = (h + 1) / 2, ow = (w + 1) / 2;
    const dim3 grid((ow + PT_W - 1) / PT_W, (oh + PT_H - 1) / PT_H, n);
    if (dword_form(d_bgr, d_out, w))
        hipLaunchKernelGGL(pyr_down_kernel<true>, grid, dim3(256), 0, ctx->stream, d_bgr, h, w, d_out, oh, ow);
    else
        hipLaunchKernelGGL(pyr_down_kernel<false>, grid, dim3(256), 0, ctx->stream, d_bgr, h, w, d_out, oh, ow);
    CK_HIP(ctx, hipGetLastError());
    return CK_OK;
}

int k_i420_pyr_down(ck_ctx* ctx, const uint8_t* d_i420, int n, int h, int w, uint8_t* d_out)
{
    TimeScope ts(ctx, "i420_pyr_down");
    const int oh = h / 2, ow = w / 2;
    const dim3 grid((ow + PT_W - 1) / PT_W, (oh + PT_H - 1) / PT_H, n);
    if (dword_form(d_i420, d_out, w))
        hipLaunchKernelGGL(i420_pyr_down_kernel<true>, grid, dim3(256), 0, ctx->stream, d_i420, h, w, d_out, oh, ow);
    else
        hipLaunchKernelGGL(i420_pyr_down_kernel<false>, grid, dim3(256), 0, ctx->stream, d_i420, h, w, d_out, oh, ow);
    CK_HIP(ctx, hipGetLastError());
    return CK_OK;
}
