// ck_i420.h -- the I420 -> BGR arithmetic, shared by k_color.hip (ck_i420_to_bgr) and k_pyramid.hip (the fused
// conversion + pyrDown): BT.601 studio range, 20-bit fixed point (cv2.cvtColor COLOR_YUV2BGR_I420 constants),
// saturated to 8 bits.  One chroma sample serves a 2x2 block of pixels: i420_chroma() once, i420_pixel() per pixel.
#pragma once
#include <stdint.h>

namespace ck_i420 {

constexpr int CY = 1220542, CUB = 2116026, CUG = -409993, CVG = -852492, CVR = 1673527, SHIFT = 20;

__device__ __forceinline__ uint32_t sat8(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

struct Chroma {
    int ruv, guv, buv;
};

__device__ __forceinline__ Chroma i420_chroma(uint8_t ub, uint8_t vb)
{
    const int u = (int)ub - 128, v = (int)vb - 128;
    Chroma c;
    c.ruv = (1 << (SHIFT - 1)) + CVR * v;
    c.guv = (1 << (SHIFT - 1)) + CVG * v + CUG * u;
    c.buv = (1 << (SHIFT - 1)) + CUB * u;
    return c;
}

// o[0..2] = B, G, R
__device__ __forceinline__ void i420_pixel(uint8_t yb, const Chroma& c, uint8_t* o)
{
    int yy = (int)yb - 16;
    yy = (yy < 0 ? 0 : yy) * CY;
    o[0] = (uint8_t)sat8((yy + c.buv) >> SHIFT);
    o[1] = (uint8_t)sat8((yy + c.guv) >> SHIFT);
    o[2] = (uint8_t)sat8((yy + c.ruv) >> SHIFT);
}

}  // namespace ck_i420
