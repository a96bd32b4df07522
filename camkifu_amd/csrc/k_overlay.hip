// k_overlay.hip -- overlays: the finders' debug drawing (lines, circles, discs, rectangles, text) rasterised in place on
// images that already lie in HBM, on their way to the JPEG encoder (include/camkifu_amd.h, "overlays").
//
// Pixels own the work.  Every primitive is a per-pixel membership test in integer arithmetic, so a thread walks the
// primitives of its bin in list order with the colour of its own pixels in registers: painter's order needs no atomics
// and no second pass, and a pixel nothing covers is neither read nor written.
//
// One workgroup of 256 threads = one non-empty bin of CK_OV_BIN x CK_OV_BIN pixels of one frame (the launch is built from
// the plan of ck_overlay.cpp: empty bins are not launched).  A thread has 4 pixels side by side; a wave has 8 full rows of
// the bin, so the test of a primitive's bounding box against a wave's pixels is wave-uniform and made a scalar branch
// (the record's fields go through readfirstlane).  The bin's records are staged in LDS, OV_CHUNK at a time.
// The destination is loaded only in bins whose list holds a primitive with alpha < 255 (uniform per workgroup).
// A frame row is w * c bytes with no alignment promise (frames of 17 x 33 x 3 start off a dword): pixels are stored
// byte by byte, only those that were covered.  HBM traffic: the bytes of the covered pixels, once more where blending
// is asked for, plus 48 bytes per (bin, primitive) pair.
#include "ck_common.h"
#include "ck_overlay.h"

#define CK_FONT_QUAL static __constant__ const
#include "ck_font5x7.h"

namespace {

constexpr int OV_CHUNK = 64;       // records staged in LDS at a time (3 KiB)
constexpr int OV_PX = 4;           // pixels per thread, side by side
static_assert(CK_OV_BIN == 32 && 256 * OV_PX == CK_OV_BIN * CK_OV_BIN, "a workgroup of 256 threads is one bin");

__device__ __forceinline__ int sgpr(int v) { return __builtin_amdgcn_readfirstlane(v); }

// minor offset of the Bresenham path at major position i (0 <= i <= D, D > 0): floor((2 d i + D - 1) / (2 D)).
// 2 d i reaches 8.6e9 at the coordinate limit: 64-bit there, 32-bit where D keeps the numerator below 2^31.
__device__ __forceinline__ int seg_minor(int i, int d, int D)
{
    if (D <= 32767) return (int)((2u * (uint32_t)d * (uint32_t)i + (uint32_t)D - 1u) / (2u * (uint32_t)D));
    return (int)((2ull * (uint64_t)d * (uint64_t)i + (uint64_t)D - 1ull) / (2ull * (uint64_t)D));
}

__device__ __forceinline__ bool in_disc(int dx, int dy, int r)      // |dx|, |dy| <= 4102: 32 bits hold the squares
{
    return dx * dx + dy * dy <= r * r + r;
}

// does the primitive cover pixel (x, y)?  r0 .. r7: the record's fields, wave-uniform
__device__ __forceinline__ bool covers(int kind, int x0, int y0, int x1, int y1, int size, int aux, const uint8_t* __restrict__ text,
                                       int x, int y)
{
    switch (kind) {
    case CK_OV_SEGMENT: {
        const int dx = x1 - x0, dy = y1 - y0;                   // dx >= 0: the endpoints come ordered
        const int ady = dy < 0 ? -dy : dy, hh = (size - 1) >> 1;
        const bool xmajor = dx >= ady;
        const int D = xmajor ? dx : ady, d = xmajor ? ady : dx;
        const int sy = dy < 0 ? y0 - y : y - y0;                // the pixel's offset along the path's y direction
        const int i = xmajor ? x - x0 : sy, q = xmajor ? sy : x - x0;
        const int a = i - hh < 0 ? 0 : i - hh, b = i + hh > D ? D : i + hh;
        if (a > b || q + hh < 0 || q - hh > d) return false;
        if (D == 0) return true;                                // a point: its offset is 0, and |q| <= hh was just seen
        // the path's offsets over i = a .. b are every integer from m(a) to m(b): steps are 0 or 1
        return seg_minor(a, d, D) <= q + hh && seg_minor(b, d, D) >= q - hh;
    }
    case CK_OV_DISC:
    case CK_OV_CIRCLE: {
        const int dx = x - x0, dy = y - y0;
        if (dx < -size || dx > size || dy < -size || dy > size) return false;
        if (!in_disc(dx, dy, size)) return false;
        return kind == CK_OV_DISC || x1 < 0 || !in_disc(dx, dy, x1);
    }
    case CK_OV_RECT: {
        if (x < x0 || x > x1 || y < y0 || y > y1) return false;
        return size == 0 || x - x0 < size || x1 - x < size || y - y0 < size || y1 - y < size;
    }
    case CK_OV_TEXT: {
        const int rx = x - x0, ry = y - y0;
        if (rx < 0 || ry < 0 || ry >= 8 * size) return false;
        const int cell = rx / (6 * size);
        if (cell >= x1) return false;
        const int gx = (rx - cell * 6 * size) / size, gy = ry / size;
        if (gx >= 5 || gy >= 7) return false;
        int ch = text[aux + cell];
        if (ch < 32 || ch > 126) ch = '?';
        return (ck_font5x7[ch - 32][gy] >> (4 - gx)) & 1;
    }
    }
    return false;
}

// work: per launched bin {frame, bin column, bin row, first entry in refs, entries, 1 when a primitive blends, 0, 0}
template <int C>
__global__ __launch_bounds__(256) void overlay_kernel(uint8_t* __restrict__ img, int h, int w, const int32_t* __restrict__ work,
                                                      const int32_t* __restrict__ refs, const int32_t* __restrict__ recs,
                                                      const uint8_t* __restrict__ text)
{
    __shared__ int32_t s_rec[OV_CHUNK * CK_OV_REC];
    const int32_t* wk = work + (size_t)blockIdx.x * 8;
    const int frame = wk[0], bx = wk[1], by = wk[2], first = wk[3], count = wk[4], blends = wk[5];
    const int wave = sgpr((int)threadIdx.x >> 6);
    // the wave's pixels: all 32 columns of the bin, 8 rows; clipped to the image
    const int wx0 = bx * CK_OV_BIN, wy0 = by * CK_OV_BIN + wave * 8;
    const int wx1 = min(wx0 + CK_OV_BIN - 1, w - 1), wy1 = min(wy0 + 7, h - 1);
    const int x = wx0 + ((int)threadIdx.x & 7) * OV_PX, y = by * CK_OV_BIN + ((int)threadIdx.x >> 3);
    const bool row_ok = y < h;
    uint8_t* const px = img + (((size_t)frame * h + (row_ok ? y : 0)) * w + (x < w ? x : 0)) * C;

    uint32_t pix[OV_PX];           // b | g << 8 | r << 16 as it stands now
    uint32_t valid = 0, covered = 0;
#pragma unroll
    for (int k = 0; k < OV_PX; k++) {
        pix[k] = 0;
        if (row_ok && x + k < w) valid |= 1u << k;
    }
    if (blends) {
#pragma unroll
        for (int k = 0; k < OV_PX; k++)
            if (valid >> k & 1) {
                uint32_t v = px[k * C];
                if (C == 3) v |= (uint32_t)px[k * C + 1] << 8 | (uint32_t)px[k * C + 2] << 16;
                pix[k] = v;
            }
    }

    for (int c0 = 0; c0 < count; c0 += OV_CHUNK) {
        const int m = min(OV_CHUNK, count - c0);
        __syncthreads();                                        // the chunk before has been walked by every wave
        for (int j = threadIdx.x; j < m * CK_OV_REC; j += 256) {
            const int i = j / CK_OV_REC;
            s_rec[j] = recs[(size_t)refs[first + c0 + i] * CK_OV_REC + (j - i * CK_OV_REC)];
        }
        __syncthreads();
        for (int i = 0; i < m; i++) {
            const int32_t* r = s_rec + i * CK_OV_REC;
            if (sgpr(r[8]) > wx1 || sgpr(r[10]) < wx0 || sgpr(r[9]) > wy1 || sgpr(r[11]) < wy0) continue;     // scalar branch
            const int kind = sgpr(r[0]), x0 = sgpr(r[1]), y0 = sgpr(r[2]), x1 = sgpr(r[3]), y1 = sgpr(r[4]), size = sgpr(r[5]);
            const uint32_t colour = (uint32_t)sgpr(r[6]);
            const int aux = sgpr(r[7]);
            const uint32_t alpha = colour >> 24;
#pragma unroll
            for (int k = 0; k < OV_PX; k++) {
                if (!(valid >> k & 1) || !covers(kind, x0, y0, x1, y1, size, aux, text, x + k, y)) continue;
                covered |= 1u << k;
                if (alpha == 255) {
                    pix[k] = colour & 0xffffffu;
                } else {
                    uint32_t out = 0;
#pragma unroll
                    for (int ch = 0; ch < C; ch++) {
                        const uint32_t cv = colour >> (8 * ch) & 255u, pv = pix[k] >> (8 * ch) & 255u;
                        out |= ((cv * alpha + pv * (255u - alpha) + 127u) / 255u) << (8 * ch);
                    }
                    pix[k] = out;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < OV_PX; k++)
        if (covered >> k & 1) {                                 // (covered is a subset of valid)
#pragma unroll
            for (int ch = 0; ch < C; ch++) px[k * C + ch] = (uint8_t)(pix[k] >> (8 * ch));
        }
}

}  // namespace

int k_overlay(ck_ctx* ctx, uint8_t* d_img, int h, int w, int c, const int32_t* d_work, int n_work, const int32_t* d_refs,
              const int32_t* d_recs, const uint8_t* d_text)
{
    if (n_work <= 0) return CK_OK;
    TimeScope ts(ctx, "overlay_draw");
    if (c == 3)
        hipLaunchKernelGGL(overlay_kernel<3>, dim3(n_work), dim3(256), 0, ctx->stream, d_img, h, w, d_work, d_refs, d_recs, d_text);
    else
        hipLaunchKernelGGL(overlay_kernel<1>, dim3(n_work), dim3(256), 0, ctx->stream, d_img, h, w, d_work, d_refs, d_recs, d_text);
    CK_HIP(ctx, hipGetLastError());
    return CK_OK;
}
