// k_jpeg.hip -- everything of a baseline JPEG decode that comes after the Huffman decoder, in one kernel: dequantise,
// inverse DCT, chroma upsampling, YCbCr -> BGR.  The numbers are libjpeg's default path (jidctint's slow-integer IDCT,
// "fancy" triangle upsampling, the 16-bit fixed-point colour conversion) -- what cv2.imread gives -- bit for bit, in int32.
//
// Reads the int16 coefficients once and writes interleaved BGR once: 6 * W * H bytes per 4:2:0 frame.
//
// One workgroup = JT_W x JT_H output pixels (64 x 32: a whole number of MCUs for every sampling).  It owns the 8 x 4 luma
// blocks of its tile and, per chroma component, the blocks that cover the tile's chroma samples plus one sample of halo all
// round where the upsampling filter needs it -- 6 x 4 blocks for 4:2:0 (halo left/right and above/below) and for 4:2:2
// (left/right only), 8 x 4 for 4:4:4.  Blocks outside the component's grid are skipped; the filter never reads them because
// its taps are clamped to the REAL chroma size ceil(w/2) x ceil(h/2), not to the MCU-padded one.  Steps, a barrier between:
//   1. load      one item = one row of one block: 8 coefficients (one 16-byte load) times 8 quant entries -> int32 in LDS
//   2. columns   one item = one column of one block: the 8-point pass, (x + 2^10) >> 11, in place
//   3. rows      one item = one row of one block: the same pass, (x + 2^17) >> 18, range-limited to a byte -> the
//                component's sample plane of the tile in LDS (8 bytes, two dword stores)
//   4. pixels    one item = 4 output pixels of one row: upsample + convert from the planes, 12 bytes out -- three dwords
//                when rows start on dwords (w % 4 == 0), bounds-checked bytes otherwise.
// A block's int32 workspace has a pitch of 72 dwords: step 2 reads with 8 lanes per block at consecutive dwords, and 72
// puts the four blocks of a 32-lane group on banks 0-7, 8-15, 16-23, 24-31.
#include "ck_common.h"
#include "ck_jpeg.h"

namespace {

constexpr int JT_W = 64, JT_H = 32;
constexpr int JB_LUMA = (JT_W / 8) * (JT_H / 8);         // 32 luma blocks
constexpr int JWS_PITCH = 72;

template <int S> struct Geo;                             // chroma block columns of a tile, halo blocks left / above, log2 subsampling
template <> struct Geo<CK_JPEG_GREY> { static constexpr int ncx = 0, hx = 0, hy = 0, sx = 0, sy = 0; };
template <> struct Geo<CK_JPEG_444>  { static constexpr int ncx = 8, hx = 0, hy = 0, sx = 0, sy = 0; };
template <> struct Geo<CK_JPEG_422>  { static constexpr int ncx = 6, hx = 1, hy = 0, sx = 1, sy = 0; };
template <> struct Geo<CK_JPEG_420>  { static constexpr int ncx = 6, hx = 1, hy = 1, sx = 1, sy = 1; };

// jidctint's 8-point pass (CONST_BITS 13).  Unsigned arithmetic: the same bits as int32, and a value that wraps (only
// coefficients no encoder writes get there) wraps instead of being undefined.
template <int SHIFT>
__device__ __forceinline__ void idct8(const uint32_t in[8], int out[8])
{
    uint32_t z1 = (in[2] + in[6]) * 4433u;
    const uint32_t t2 = z1 + in[6] * (uint32_t)-15137;
    const uint32_t t3 = z1 + in[2] * 6270u;
    const uint32_t t0 = (in[0] + in[4]) << 13, t1 = (in[0] - in[4]) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t o0 = in[7], o1 = in[5], o2 = in[3], o3 = in[1];
    z1 = o0 + o3;
    uint32_t z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    o0 *= 2446u; o1 *= 16819u; o2 *= 25172u; o3 *= 12299u;
    z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995; z3 *= (uint32_t)-16069; z4 *= (uint32_t)-3196;
    z3 += z5; z4 += z5;
    o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
    constexpr uint32_t R = 1u << (SHIFT - 1);
    out[0] = (int)(t10 + o3 + R) >> SHIFT; out[7] = (int)(t10 - o3 + R) >> SHIFT;
    out[1] = (int)(t11 + o2 + R) >> SHIFT; out[6] = (int)(t11 - o2 + R) >> SHIFT;
    out[2] = (int)(t12 + o1 + R) >> SHIFT; out[5] = (int)(t12 - o1 + R) >> SHIFT;
    out[3] = (int)(t13 + o0 + R) >> SHIFT; out[4] = (int)(t13 - o0 + R) >> SHIFT;
}

// libjpeg's range table read at v & 1023 (128..255, 384 x 255, 384 x 0, 0..127): the low 10 bits as a signed number, plus
// 128, clamped to a byte
__device__ __forceinline__ uint32_t range_limit(int v)
{
    const int s = ((int)((uint32_t)v << 22) >> 22) + 128;
    return (uint32_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
}

struct BlockAt {
    int comp, lx, ly;      // component, block position inside the component's tile
    long long at;          // block index in the frame's coefficient array, -1: outside the component's grid
};

template <int S>
__device__ __forceinline__ BlockAt locate(int blk, int tx, int ty, int lw, int lh, int cgw, int cgh)
{
    using G = Geo<S>;
    BlockAt b;
    if (blk < JB_LUMA) {
        b.comp = 0; b.lx = blk & 7; b.ly = blk >> 3;
        const int gx = tx * 8 + b.lx, gy = ty * 4 + b.ly;
        b.at = (gx < lw && gy < lh) ? (long long)gy * lw + gx : -1;
        return b;
    }
    constexpr int per = (G::ncx ? G::ncx : 1) * 4;
    const int cb = blk - JB_LUMA;
    b.comp = 1 + cb / per;
    const int l = cb - (b.comp - 1) * per;
    b.ly = l / (G::ncx ? G::ncx : 1); b.lx = l - b.ly * (G::ncx ? G::ncx : 1);
    const int gx = ((tx * 8) >> G::sx) - G::hx + b.lx, gy = ((ty * 4) >> G::sy) - G::hy + b.ly;
    b.at = (gx >= 0 && gy >= 0 && gx < cgw && gy < cgh)
               ? (long long)lw * lh + (long long)(b.comp - 1) * cgw * cgh + (long long)gy * cgw + gx : -1;
    return b;
}

template <int S, bool WIDE>
__global__ __launch_bounds__(256) void jpeg_reconstruct_kernel(const int16_t* __restrict__ coef, const uint16_t* __restrict__ quant,
                                                               int h, int w, long long blocks, uint8_t* __restrict__ bgr)
{
    using G = Geo<S>;
    constexpr int NB = JB_LUMA + 2 * G::ncx * 4;
    constexpr int CP = (G::ncx ? G::ncx : 1) * 8;            // pitch of a chroma plane
    __shared__ __attribute__((aligned(16))) int ws[NB * JWS_PITCH];
    __shared__ __attribute__((aligned(16))) uint8_t yp[JT_H * JT_W];
    __shared__ __attribute__((aligned(16))) uint8_t cp[2][32 * CP];

    const int tx = blockIdx.x, ty = blockIdx.y;
    const int hs = S >= CK_JPEG_422 ? 2 : 1, vs = S == CK_JPEG_420 ? 2 : 1;
    const int mcux = (w + 8 * hs - 1) / (8 * hs), mcuy = (h + 8 * vs - 1) / (8 * vs);
    const int lw = mcux * hs, lh = mcuy * vs;                // luma grid; the chroma grids are mcux x mcuy
    const int16_t* fc = coef + (size_t)blockIdx.z * (size_t)blocks * 64;
    const uint16_t* fq = quant + (size_t)blockIdx.z * 192;

    // 1. load and dequantise
    for (int it = threadIdx.x; it < NB * 8; it += blockDim.x) {
        const int blk = it >> 3, r = it & 7;
        const BlockAt b = locate<S>(blk, tx, ty, lw, lh, mcux, mcuy);
        if (b.at < 0) continue;
        const uint4 c4 = *reinterpret_cast<const uint4*>(fc + (size_t)b.at * 64 + r * 8);
        const uint4 q4 = *reinterpret_cast<const uint4*>(fq + b.comp * 64 + r * 8);
        const uint32_t cw[4] = {c4.x, c4.y, c4.z, c4.w}, qw[4] = {q4.x, q4.y, q4.z, q4.w};
        int v[8];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            v[2 * k] = (int)(int16_t)(cw[k] & 0xffffu) * (int)(qw[k] & 0xffffu);
            v[2 * k + 1] = (int)(int16_t)(cw[k] >> 16) * (int)(qw[k] >> 16);
        }
        int4* d = reinterpret_cast<int4*>(ws + blk * JWS_PITCH + r * 8);
        d[0] = make_int4(v[0], v[1], v[2], v[3]);
        d[1] = make_int4(v[4], v[5], v[6], v[7]);
    }
    __syncthreads();
    // 2. columns
    for (int it = threadIdx.x; it < NB * 8; it += blockDim.x) {
        const int blk = it >> 3, c = it & 7;
        if (locate<S>(blk, tx, ty, lw, lh, mcux, mcuy).at < 0) continue;
        int* p = ws + blk * JWS_PITCH + c;
        uint32_t in[8];
        int out[8];
#pragma unroll
        for (int k = 0; k < 8; k++) in[k] = (uint32_t)p[k * 8];
        idct8<11>(in, out);
#pragma unroll
        for (int k = 0; k < 8; k++) p[k * 8] = out[k];
    }
    __syncthreads();
    // 3. rows -> sample planes
    for (int it = threadIdx.x; it < NB * 8; it += blockDim.x) {
        const int blk = it >> 3, r = it & 7;
        const BlockAt b = locate<S>(blk, tx, ty, lw, lh, mcux, mcuy);
        if (b.at < 0) continue;
        const int4* s4 = reinterpret_cast<const int4*>(ws + blk * JWS_PITCH + r * 8);
        const int4 a = s4[0], e = s4[1];
        const uint32_t in[8] = {(uint32_t)a.x, (uint32_t)a.y, (uint32_t)a.z, (uint32_t)a.w,
                                (uint32_t)e.x, (uint32_t)e.y, (uint32_t)e.z, (uint32_t)e.w};
        int out[8];
        idct8<18>(in, out);
        const uint32_t lo = range_limit(out[0]) | (range_limit(out[1]) << 8) | (range_limit(out[2]) << 16) | (range_limit(out[3]) << 24);
        const uint32_t hi = range_limit(out[4]) | (range_limit(out[5]) << 8) | (range_limit(out[6]) << 16) | (range_limit(out[7]) << 24);
        uint8_t* plane = b.comp == 0 ? yp : cp[b.comp - 1];
        const int pitch = b.comp == 0 ? JT_W : CP;
        uint32_t* d = reinterpret_cast<uint32_t*>(plane + (b.ly * 8 + r) * pitch + b.lx * 8);
        d[0] = lo; d[1] = hi;
    }
    __syncthreads();
    // 4. pixels
    uint8_t* fo = bgr + (size_t)blockIdx.z * (size_t)h * w * 3;
    const int cw_real = (w + G::sx) >> G::sx, ch_real = (h + G::sy) >> G::sy;       // the real chroma size
    // libjpeg upsamples with the triangle filter only where the chroma plane is more than 2 samples wide (jdsample.c) and
    // replicates samples otherwise: with both taps on the sample itself the filters below give exactly that
    const bool replicate = cw_real <= 2;
    const int cx0 = ((tx * JT_W) >> G::sx) - 8 * G::hx, cy0 = ((ty * JT_H) >> G::sy) - 8 * G::hy;    // chroma sample at plane (0, 0)
    for (int it = threadIdx.x; it < JT_H * (JT_W / 4); it += blockDim.x) {
        const int ly = it / (JT_W / 4), q = it - ly * (JT_W / 4);
        const int gy = ty * JT_H + ly, gx = tx * JT_W + 4 * q;
        if (gy >= h || gx >= w) continue;
        const uint32_t y4 = *reinterpret_cast<const uint32_t*>(yp + ly * JT_W + 4 * q);
        uint8_t o[12];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int Y = (int)((y4 >> (8 * k)) & 255u);
            const int x = gx + k < w ? gx + k : w - 1;              // (a pixel beyond the row is computed, not stored)
            int B = Y, Gn = Y, R = Y;
            if constexpr (S != CK_JPEG_GREY) {
                int cbv, crv;
                if constexpr (S == CK_JPEG_444) {
                    cbv = cp[0][ly * CP + (x - tx * JT_W)];
                    crv = cp[1][ly * CP + (x - tx * JT_W)];
                } else {
                    const int c = x >> 1;
                    int nb = (x & 1) ? c + 1 : c - 1;
                    nb = nb < 0 ? 0 : (nb >= cw_real ? cw_real - 1 : nb);
                    if (replicate) nb = c;
                    const int ic = c - cx0, in = nb - cx0;
                    if constexpr (S == CK_JPEG_422) {
                        const int row = (gy - cy0) * CP;
                        const int rnd = (x & 1) ? 2 : 1;
                        cbv = (3 * cp[0][row + ic] + cp[0][row + in] + rnd) >> 2;
                        crv = (3 * cp[1][row + ic] + cp[1][row + in] + rnd) >> 2;
                    } else {
                        const int r = gy >> 1;
                        int fr = (gy & 1) ? r + 1 : r - 1;
                        fr = fr < 0 ? 0 : (fr >= ch_real ? ch_real - 1 : fr);
                        if (replicate) fr = r;
                        const int rn = (r - cy0) * CP, rf = (fr - cy0) * CP;
                        const int rnd = (x & 1) ? 7 : 8;
                        const int sb = 3 * cp[0][rn + ic] + cp[0][rf + ic], sbn = 3 * cp[0][rn + in] + cp[0][rf + in];
                        const int sr = 3 * cp[1][rn + ic] + cp[1][rf + ic], srn = 3 * cp[1][rn + in] + cp[1][rf + in];
                        cbv = (3 * sb + sbn + rnd) >> 4;
                        crv = (3 * sr + srn + rnd) >> 4;
                    }
                }
                cbv -= 128; crv -= 128;
                R = Y + ((91881 * crv + 32768) >> 16);
                B = Y + ((116130 * cbv + 32768) >> 16);
                Gn = Y + ((-22554 * cbv - 46802 * crv + 32768) >> 16);
            }
            o[3 * k] = (uint8_t)(B < 0 ? 0 : (B > 255 ? 255 : B));
            o[3 * k + 1] = (uint8_t)(Gn < 0 ? 0 : (Gn > 255 ? 255 : Gn));
            o[3 * k + 2] = (uint8_t)(R < 0 ? 0 : (R > 255 ? 255 : R));
        }
        uint8_t* d = fo + ((size_t)gy * w + gx) * 3;
        if constexpr (WIDE) {
            // w % 4 == 0: the four pixels lie inside the row, and d is on a dword
            uint32_t* d4 = reinterpret_cast<uint32_t*>(d);
            d4[0] = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24);
            d4[1] = (uint32_t)o[4] | ((uint32_t)o[5] << 8) | ((uint32_t)o[6] << 16) | ((uint32_t)o[7] << 24);
            d4[2] = (uint32_t)o[8] | ((uint32_t)o[9] << 8) | ((uint32_t)o[10] << 16) | ((uint32_t)o[11] << 24);
        } else {
            const int npx = w - gx < 4 ? w - gx : 4;
            for (int k = 0; k < npx * 3; k++) d[k] = o[k];
        }
    }
}

template <int S>
int launch(ck_ctx* ctx, const int16_t* d_coef, const uint16_t* d_quant, int n, int h, int w, uint8_t* d_bgr)
{
    const long long blocks = ck_jpeg_blocks(h, w, S);
    const bool wide = (w % 4) == 0 && ((uintptr_t)d_bgr & 3) == 0;          // (then every frame of the batch starts on a dword)
    for (int f0 = 0; f0 < n; f0 += 65535) {                                  // a grid holds 65535 frames
        const dim3 grid((w + JT_W - 1) / JT_W, (h + JT_H - 1) / JT_H, n - f0 < 65535 ? n - f0 : 65535);
        const int16_t* c = d_coef + (size_t)f0 * (size_t)blocks * 64;
        const uint16_t* q = d_quant + (size_t)f0 * 192;
        uint8_t* o = d_bgr + (size_t)f0 * (size_t)h * w * 3;
        if (wide)
            hipLaunchKernelGGL((jpeg_reconstruct_kernel<S, true>), grid, dim3(256), 0, ctx->stream, c, q, h, w, blocks, o);
        else
            hipLaunchKernelGGL((jpeg_reconstruct_kernel<S, false>), grid, dim3(256), 0, ctx->stream, c, q, h, w, blocks, o);
        CK_HIP(ctx, hipGetLastError());
    }
    return CK_OK;
}

}  // namespace

// d_coef (16-byte aligned) and d_quant as ck_jpeg_coefficients writes them, on the device
int k_jpeg_reconstruct(ck_ctx* ctx, const int16_t* d_coef, const uint16_t* d_quant, int n, int h, int w, int sampling, uint8_t* d_bgr)
{
    TimeScope ts(ctx, "jpeg");
    switch (sampling) {
    case CK_JPEG_GREY: return launch<CK_JPEG_GREY>(ctx, d_coef, d_quant, n, h, w, d_bgr);
    case CK_JPEG_444: return launch<CK_JPEG_444>(ctx, d_coef, d_quant, n, h, w, d_bgr);
    case CK_JPEG_422: return launch<CK_JPEG_422>(ctx, d_coef, d_quant, n, h, w, d_bgr);
    case CK_JPEG_420: return launch<CK_JPEG_420>(ctx, d_coef, d_quant, n, h, w, d_bgr);
    }
    return ck_fail(ctx, CK_ERR_ARG, "bad JPEG sampling %d", sampling);
}
