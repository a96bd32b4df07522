// k_jpeg_enc.hip -- everything of a baseline JPEG encode that comes before the Huffman coder, in one kernel: BGR -> YCbCr,
// edge replication, chroma downsampling, forward DCT, quantisation.  The mirror of k_jpeg.hip.  The numbers are libjpeg's
// default compressor (jccolor's 16-bit fixed point, jcsample's box filter without smoothing, jfdctint's slow-integer DCT,
// jcdctmgr's truncating division) -- what PIL.Image.save(.., "JPEG") gives -- bit for bit, in int32.
//
// Reads the interleaved BGR once and writes the int16 coefficients once: 6 * W * H bytes per 4:2:0 frame.
//
// One workgroup = JT_W x JT_H input pixels (64 x 32: a whole number of MCUs for every sampling).  It owns the 8 x 4 luma
// blocks of its tile and, per chroma component, the 8 x 4 (4:4:4), 4 x 4 (4:2:2) or 4 x 2 (4:2:0) blocks its pixels reduce
// to; no halo: a box filter reads no neighbour.  Steps, a barrier between:
//   1. pixels    one item = 4 pixels of one row, coordinates clamped to the image (that IS libjpeg's replication of the last
//                column and row at full size): 12 bytes in -- three dwords when rows start on dwords -- Y, Cb, Cr to the
//                tile's three full-size sample planes in LDS
//   2. rows      one item = one row of one REAL block: 8 samples (chroma: reduced here from the full-size planes) minus
//                128, the 8-point pass, -> the block's int32 workspace in LDS
//   3. columns   one item = one column of one block: the same pass with the second descale, then the quantiser, in place
//   4. store     one item = one row of one block of the MCU-padded grid: 8 int16, one 16-byte store.  A dummy block (luma
//                at 4:2:2 / 4:2:0 beyond the real blocks) stores zeros and the quantised DC of the block it copies, which
//                always lies in the same MCU, so in this tile.
// The one place where clamped coordinates are NOT libjpeg's edge rule: at 4:2:0 full-size rows are replicated only up to an
// even count, and below that the REDUCED rows are: step 2 reads reduced row min(r, ceil(h/2) - 1), not r.
#include "ck_common.h"
#include "ck_jpeg.h"

namespace {

constexpr int JT_W = 64, JT_H = 32;
constexpr int JB_LUMA = (JT_W / 8) * (JT_H / 8);         // 32 luma blocks
constexpr int JWS_PITCH = 72;                            // as in k_jpeg.hip: four blocks of a 32-lane group on banks 0-7 .. 24-31

template <int S> struct Geo;                             // log2 of the vertical chroma reduction; chroma blocks of a tile across and down
template <> struct Geo<CK_JPEG_GREY> { static constexpr int sy = 0, cbx = 0, cby = 0; };
template <> struct Geo<CK_JPEG_444>  { static constexpr int sy = 0, cbx = 8, cby = 4; };
template <> struct Geo<CK_JPEG_422>  { static constexpr int sy = 0, cbx = 4, cby = 4; };
template <> struct Geo<CK_JPEG_420>  { static constexpr int sy = 1, cbx = 4, cby = 2; };

// jfdctint's 8-point pass (CONST_BITS 13, PASS1_BITS 2).  FIRST: the row pass (even DC terms << 2, the rest descaled by 11);
// else the column pass (2 and 15).  int32 holds every intermediate: samples are within +-128, so the row pass gives at most
// 5793 in magnitude and the largest sum of the column pass stays below 1.6e9.
template <bool FIRST>
__device__ __forceinline__ void fdct8(const int d[8], int out[8])
{
    constexpr int N = FIRST ? 11 : 15, R = 1 << (N - 1);
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if constexpr (FIRST) {
        out[0] = (t10 + t11) * 4; out[4] = (t10 - t11) * 4;
    } else {
        out[0] = (t10 + t11 + 2) >> 2; out[4] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * 4433;
    out[2] = (z1 + t13 * 6270 + R) >> N;
    out[6] = (z1 - t12 * 15137 + R) >> N;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int o4 = t4 * 2446, o5 = t5 * 16819, o6 = t6 * 25172, o7 = t7 * 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    out[7] = (o4 + z1 + z3 + R) >> N;
    out[5] = (o5 + z2 + z4 + R) >> N;
    out[3] = (o6 + z2 + z3 + R) >> N;
    out[1] = (o7 + z1 + z4 + R) >> N;
}

struct BlockAt {
    int comp, lx, ly;      // component, block position inside the component's tile
    int gx, gy;            // block position in the component's MCU-padded grid
    long long at;          // block index in the frame's coefficient array, -1: outside the component's grid
};

template <int S>
__device__ __forceinline__ BlockAt locate(int blk, int tx, int ty, int lw, int lh, int cgw, int cgh)
{
    using G = Geo<S>;
    BlockAt b;
    if (blk < JB_LUMA) {
        b.comp = 0; b.lx = blk & 7; b.ly = blk >> 3;
        b.gx = tx * 8 + b.lx; b.gy = ty * 4 + b.ly;
        b.at = (b.gx < lw && b.gy < lh) ? (long long)b.gy * lw + b.gx : -1;
        return b;
    }
    constexpr int cbx = G::cbx ? G::cbx : 1, per = cbx * (G::cby ? G::cby : 1);
    const int cb = blk - JB_LUMA;
    b.comp = 1 + cb / per;
    const int l = cb - (b.comp - 1) * per;
    b.ly = l / cbx; b.lx = l - b.ly * cbx;
    b.gx = tx * G::cbx + b.lx; b.gy = ty * G::cby + b.ly;
    b.at = (b.gx < cgw && b.gy < cgh) ? (long long)lw * lh + (long long)(b.comp - 1) * cgw * cgh + (long long)b.gy * cgw + b.gx : -1;
    return b;
}

template <int S, bool WIDE>
__global__ __launch_bounds__(256) void jpeg_forward_kernel(const uint8_t* __restrict__ bgr, const uint16_t* __restrict__ quant,
                                                           int h, int w, long long blocks, int16_t* __restrict__ coef)
{
    using G = Geo<S>;
    constexpr int NB = JB_LUMA + 2 * G::cbx * G::cby;
    constexpr int NP = S == CK_JPEG_GREY ? 1 : 3;
    __shared__ __attribute__((aligned(16))) int ws[NB * JWS_PITCH];
    __shared__ __attribute__((aligned(16))) uint8_t pl[NP][JT_H * JT_W];          // Y, Cb, Cr at full size

    const int tx = blockIdx.x, ty = blockIdx.y;
    const int hs = S >= CK_JPEG_422 ? 2 : 1, vs = S == CK_JPEG_420 ? 2 : 1;
    const int mcux = (w + 8 * hs - 1) / (8 * hs), mcuy = (h + 8 * vs - 1) / (8 * vs);
    const int lw = mcux * hs, lh = mcuy * vs;                // luma grid; the chroma grids are mcux x mcuy
    const int wbl = (w + 7) >> 3, hbl = (h + 7) >> 3;        // REAL luma blocks (every chroma block of the grid is real)
    const uint8_t* fi = bgr + (size_t)blockIdx.z * (size_t)h * w * 3;
    int16_t* fo = coef + (size_t)blockIdx.z * (size_t)blocks * 64;

    // 1. pixels
    for (int it = threadIdx.x; it < JT_H * (JT_W / 4); it += blockDim.x) {
        const int ly = it / (JT_W / 4), q = it - ly * (JT_W / 4);
        const int gy = ty * JT_H + ly, gx = tx * JT_W + 4 * q;
        const int sy = gy < h ? gy : h - 1;
        uint8_t px[12];
        bool whole = false;
        if constexpr (WIDE) whole = gx + 3 < w;             // w % 4 == 0: then the four pixels lie inside the row, on a dword
        if (whole) {
            const uint32_t* s4 = reinterpret_cast<const uint32_t*>(fi + ((size_t)sy * w + gx) * 3);
            const uint32_t a = s4[0], b = s4[1], c = s4[2];
#pragma unroll
            for (int k = 0; k < 4; k++) { px[k] = (uint8_t)(a >> (8 * k)); px[4 + k] = (uint8_t)(b >> (8 * k)); px[8 + k] = (uint8_t)(c >> (8 * k)); }
        } else {
            const uint8_t* row = fi + (size_t)sy * w * 3;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int x = gx + k < w ? gx + k : w - 1;
                px[3 * k] = row[3 * x]; px[3 * k + 1] = row[3 * x + 1]; px[3 * k + 2] = row[3 * x + 2];
            }
        }
        uint32_t y4 = 0, cb4 = 0, cr4 = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int B = px[3 * k], Gn = px[3 * k + 1], R = px[3 * k + 2];
            y4 |= (uint32_t)((19595 * R + 38470 * Gn + 7471 * B + 32768) >> 16) << (8 * k);
            if constexpr (S != CK_JPEG_GREY) {
                cb4 |= (uint32_t)((-11059 * R - 21709 * Gn + 32768 * B + (128 << 16) + 32767) >> 16) << (8 * k);
                cr4 |= (uint32_t)((32768 * R - 27439 * Gn - 5329 * B + (128 << 16) + 32767) >> 16) << (8 * k);
            }
        }
        *reinterpret_cast<uint32_t*>(pl[0] + ly * JT_W + 4 * q) = y4;
        if constexpr (S != CK_JPEG_GREY) {
            *reinterpret_cast<uint32_t*>(pl[1] + ly * JT_W + 4 * q) = cb4;
            *reinterpret_cast<uint32_t*>(pl[2] + ly * JT_W + 4 * q) = cr4;
        }
    }
    __syncthreads();
    // 2. rows
    const int ch_real = (h + G::sy) >> G::sy;                // the real chroma height
    for (int it = threadIdx.x; it < NB * 8; it += blockDim.x) {
        const int blk = it >> 3, r = it & 7;
        const BlockAt b = locate<S>(blk, tx, ty, lw, lh, mcux, mcuy);
        if (b.at < 0 || (b.comp == 0 && (b.gx >= wbl || b.gy >= hbl))) continue;
        int d[8];
        if (b.comp == 0 || S == CK_JPEG_444) {
            const uint32_t* s = reinterpret_cast<const uint32_t*>(pl[b.comp] + (b.ly * 8 + r) * JT_W + b.lx * 8);
            const uint32_t lo = s[0], hi = s[1];
#pragma unroll
            for (int k = 0; k < 4; k++) { d[k] = (int)((lo >> (8 * k)) & 255u) - 128; d[4 + k] = (int)((hi >> (8 * k)) & 255u) - 128; }
        } else if constexpr (S == CK_JPEG_422) {
            const uint8_t* s = pl[b.comp] + (b.ly * 8 + r) * JT_W + b.lx * 16;
#pragma unroll
            for (int k = 0; k < 8; k++) d[k] = ((s[2 * k] + s[2 * k + 1] + (k & 1)) >> 1) - 128;
        } else if constexpr (S == CK_JPEG_420) {
            int rr = ty * (JT_H / 2) + b.ly * 8 + r;         // the reduced row, in the frame
            rr = (rr < ch_real ? rr : ch_real - 1) - ty * (JT_H / 2);
            const uint8_t* s = pl[b.comp] + 2 * rr * JT_W + b.lx * 16;
#pragma unroll
            for (int k = 0; k < 8; k++) d[k] = ((s[2 * k] + s[2 * k + 1] + s[JT_W + 2 * k] + s[JT_W + 2 * k + 1] + 1 + (k & 1)) >> 2) - 128;
        }
        int out[8];
        fdct8<true>(d, out);
        int4* o = reinterpret_cast<int4*>(ws + blk * JWS_PITCH + r * 8);
        o[0] = make_int4(out[0], out[1], out[2], out[3]);
        o[1] = make_int4(out[4], out[5], out[6], out[7]);
    }
    __syncthreads();
    // 3. columns, quantised
    for (int it = threadIdx.x; it < NB * 8; it += blockDim.x) {
        const int blk = it >> 3, c = it & 7;
        const BlockAt b = locate<S>(blk, tx, ty, lw, lh, mcux, mcuy);
        if (b.at < 0 || (b.comp == 0 && (b.gx >= wbl || b.gy >= hbl))) continue;
        int* p = ws + blk * JWS_PITCH + c;
        int d[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; k++) d[k] = p[k * 8];
        fdct8<false>(d, out);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t qv = (uint32_t)quant[b.comp * 64 + k * 8 + c] << 3;
            const uint32_t a = (uint32_t)(out[k] < 0 ? -out[k] : out[k]) + (qv >> 1);
            const int m = (int)(a / qv);
            p[k * 8] = out[k] < 0 ? -m : m;
        }
    }
    __syncthreads();
    // 4. store
    for (int it = threadIdx.x; it < NB * 8; it += blockDim.x) {
        const int blk = it >> 3, r = it & 7;
        const BlockAt b = locate<S>(blk, tx, ty, lw, lh, mcux, mcuy);
        if (b.at < 0) continue;
        int v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (b.comp == 0 && (b.gx >= wbl || b.gy >= hbl)) {
            // a dummy block: at the bottom it copies the last block of the row above in its MCU, and that one (or the block
            // itself, at the right edge) the block to its left when it is a dummy too
            int sx = b.lx, sy = b.ly;
            if (b.gy >= hbl) { sy -= 1; sx |= hs - 1; }
            if (tx * 8 + sx >= wbl) sx -= 1;
            if (r == 0) v[0] = ws[(sy * 8 + sx) * JWS_PITCH];
        } else {
            const int4* s4 = reinterpret_cast<const int4*>(ws + blk * JWS_PITCH + r * 8);
            const int4 a = s4[0], e = s4[1];
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = e.x; v[5] = e.y; v[6] = e.z; v[7] = e.w;
        }
        uint4 o;
        o.x = (uint32_t)(v[0] & 0xffff) | ((uint32_t)v[1] << 16);
        o.y = (uint32_t)(v[2] & 0xffff) | ((uint32_t)v[3] << 16);
        o.z = (uint32_t)(v[4] & 0xffff) | ((uint32_t)v[5] << 16);
        o.w = (uint32_t)(v[6] & 0xffff) | ((uint32_t)v[7] << 16);
        *reinterpret_cast<uint4*>(fo + (size_t)b.at * 64 + r * 8) = o;
    }
}

template <int S>
int launch(ck_ctx* ctx, const uint8_t* d_bgr, const uint16_t* d_quant, int n, int h, int w, int16_t* d_coef)
{
    const long long blocks = ck_jpeg_blocks(h, w, S);
    const bool wide = (w % 4) == 0 && ((uintptr_t)d_bgr & 3) == 0;          // (then every row of every frame starts on a dword)
    for (int f0 = 0; f0 < n; f0 += 65535) {                                  // a grid holds 65535 frames
        const dim3 grid((w + JT_W - 1) / JT_W, (h + JT_H - 1) / JT_H, n - f0 < 65535 ? n - f0 : 65535);
        const uint8_t* i = d_bgr + (size_t)f0 * (size_t)h * w * 3;
        int16_t* o = d_coef + (size_t)f0 * (size_t)blocks * 64;
        if (wide)
            hipLaunchKernelGGL((jpeg_forward_kernel<S, true>), grid, dim3(256), 0, ctx->stream, i, d_quant, h, w, blocks, o);
        else
            hipLaunchKernelGGL((jpeg_forward_kernel<S, false>), grid, dim3(256), 0, ctx->stream, i, d_quant, h, w, blocks, o);
        CK_HIP(ctx, hipGetLastError());
    }
    return CK_OK;
}

}  // namespace

// d_quant: one set of tables (3 x 64 uint16, natural order, by component) and d_coef (16-byte aligned), on the device
int k_jpeg_forward(ck_ctx* ctx, const uint8_t* d_bgr, const uint16_t* d_quant, int n, int h, int w, int sampling, int16_t* d_coef)
{
    TimeScope ts(ctx, "jpeg_enc");
    switch (sampling) {
    case CK_JPEG_GREY: return launch<CK_JPEG_GREY>(ctx, d_bgr, d_quant, n, h, w, d_coef);
    case CK_JPEG_444: return launch<CK_JPEG_444>(ctx, d_bgr, d_quant, n, h, w, d_coef);
    case CK_JPEG_422: return launch<CK_JPEG_422>(ctx, d_bgr, d_quant, n, h, w, d_coef);
    case CK_JPEG_420: return launch<CK_JPEG_420>(ctx, d_bgr, d_quant, n, h, w, d_coef);
    }
    return ck_fail(ctx, CK_ERR_ARG, "bad JPEG sampling %d", sampling);
}
