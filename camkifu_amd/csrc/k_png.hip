// k_png.hip -- PNG on the device.
//
// Reading: png_unfilter_kernel undoes the row filters of inflated images in place and writes BGR.  Byte i of a row needs
// the same row's byte i - bpp and the row above's bytes i and i - bpp, so the work runs along anti-diagonals: a workgroup
// takes an image, lane r the rows r, r + 256, r + 512 .., a chunk of CK_PNG_CHUNK bytes per step.  With C chunks in a row and
// D = max(C, 256), chunk c of row 256 k + r runs at step k D + r + c: one step behind the chunk above it (lane r - 1, or for
// r = 0 the last lane's previous row, which finished D - 255 steps earlier), and a lane's rows follow one another without
// overlap.  The left context and the tail of the chunk above-left stay in registers; the chunk above is read from the
// rows themselves, which hold reconstructed bytes by then.  A barrier ends every step: no lane waits on a flag.
// About rows + (rows / 256) * max(0, C - 256) + C steps for an image, not rows * rowbytes.
//
// Writing: the steps of ck_png_stage.h, a launch each -- filter (a workgroup per row), count (per band), build (per band),
// size (per tile), scan (per band, then per frame; then the frames' places), put (the bands' headers; the tiles' literals, assembled in
// LDS and written out whole dwords, the two a tile shares with its neighbours by OR).  The mode (literals only, or runs of
// equal bytes as matches of distance 1) is a compile-time parameter of count, build, size, scan and put; the runs mode has
// two launches more behind filter -- edges (per tile) and join (per band) -- from which every tile knows how far the runs
// at its two ends reach beyond it.
#include "ck_common.h"

constexpr int PNG_TB = 256;
static_assert(CK_PNG_GROUP_ROWS == PNG_TB, "a lane per row");
static_assert(CK_PNG_TILE_BYTES == 4 * PNG_TB, "four literals a lane");

// ---- reading ---------------------------------------------------------------------------------------------------
template <int BPP>
__device__ __forceinline__ void png_unfilter_chunk(uint8_t (&cur)[CK_PNG_CHUNK], const uint8_t (&up)[CK_PNG_CHUNK], const uint8_t (&pa)[8],
                                                   const uint8_t (&pc)[8], int ft)
{
#pragma unroll
    for (int i = 0; i < CK_PNG_CHUNK; i++) {
        const int a = i >= BPP ? cur[i >= BPP ? i - BPP : 0] : pa[i >= BPP ? 0 : 8 + i - BPP];
        const int c = i >= BPP ? up[i >= BPP ? i - BPP : 0] : pc[i >= BPP ? 0 : 8 + i - BPP];
        cur[i] = (uint8_t)(cur[i] + ck_png_predict(ft, a, up[i], c));
    }
}

// the pixels of chunk c of a row (its reconstructed bytes at s) -> BGR at orow
__device__ void png_expand(const uint8_t* s, const CkPngDesc& d, const uint8_t* __restrict__ pal, long long c, int w, uint8_t* __restrict__ orow)
{
    const int ct = d.color_type, depth = d.depth;
    const int channels = ct == 0 ? 1 : ct == 2 ? 3 : ct == 3 ? 1 : ct == 4 ? 2 : 4;
    const int bpx = depth * channels, ppc = CK_PNG_CHUNK * 8 / bpx;
    if (ct == 2 && depth == 8 && (c + 1) * ppc <= w) {           // the common case, a full chunk of 8-bit RGB: 24 bytes out in whole words
        uint8_t o[CK_PNG_CHUNK];
#pragma unroll
        for (int q = 0; q < CK_PNG_CHUNK / 3; q++) { o[3 * q] = s[3 * q + 2]; o[3 * q + 1] = s[3 * q + 1]; o[3 * q + 2] = s[3 * q]; }
        __builtin_memcpy(orow + c * CK_PNG_CHUNK, o, CK_PNG_CHUNK);
        return;
    }
    for (int q = 0; q < ppc; q++) {
        const long long px = c * ppc + q;
        if (px >= w) break;
        const int bit = q * bpx, by = bit >> 3;
        int R, G, B, idx = 0;
        if (depth < 8) {
            const int v = (s[by] >> (8 - depth - (bit & 7))) & ((1 << depth) - 1);
            idx = v;
            R = G = B = v * (255 / ((1 << depth) - 1));
        } else {
            const int sb = depth >> 3;                           // 16-bit samples: the high byte comes first
            idx = s[by];
            if (ct == 2 || ct == 6) { R = s[by]; G = s[by + sb]; B = s[by + 2 * sb]; }
            else R = G = B = s[by];
        }
        if (ct == 3) {
            if (idx < d.palette_n) { R = pal[3 * idx]; G = pal[3 * idx + 1]; B = pal[3 * idx + 2]; }
            else R = G = B = 0;
        }
        uint8_t* o = orow + px * 3;
        o[0] = (uint8_t)B; o[1] = (uint8_t)G; o[2] = (uint8_t)R;
    }
}

template <int BPP>
__device__ void png_unfilter_image(uint8_t* img, const CkPngDesc& d, const uint8_t* __restrict__ pal, int h, int w, uint8_t* __restrict__ out,
                                   uint8_t* slot)
{
    const int r = threadIdx.x;
    const long long rb = d.rowbytes, pitch = rb + 1;
    const long long C = (rb + CK_PNG_CHUNK - 1) / CK_PNG_CHUNK, D = C > PNG_TB ? C : PNG_TB, K = (h + PNG_TB - 1) / PNG_TB;
    const long long steps = (K - 1) * D + (h - (K - 1) * PNG_TB) + C - 1;
    uint8_t pa[8], pc[8];
    long long y = r, c = 0;                                      // the lane's row and its next chunk (c >= C: idle until c == D)
    int ft = 0;
    for (long long s = 0; s < steps; s++) {
        if (s >= r && y < h) {
            if (c < C) {
                uint8_t* rowp = img + y * pitch;
                if (c == 0) {
                    ft = rowp[0];
#pragma unroll
                    for (int i = 0; i < 8; i++) pa[i] = pc[i] = 0;
                }
                const long long at = 1 + c * CK_PNG_CHUNK;
                const int nb = rb - c * CK_PNG_CHUNK < CK_PNG_CHUNK ? (int)(rb - c * CK_PNG_CHUNK) : CK_PNG_CHUNK;
                // a lane's rows lie a row apart, so every access of a wave touches 64 lines: a full chunk moves as whole words
                // (rows start at odd addresses: the copies are unaligned ones), only a row's last, short chunk byte by byte
                uint8_t cur[CK_PNG_CHUNK], up[CK_PNG_CHUNK];
                if (nb == CK_PNG_CHUNK) {
                    __builtin_memcpy(cur, rowp + at, CK_PNG_CHUNK);
                    if (y > 0) __builtin_memcpy(up, rowp + at - pitch, CK_PNG_CHUNK);
                    else __builtin_memset(up, 0, CK_PNG_CHUNK);
                } else {
#pragma unroll
                    for (int i = 0; i < CK_PNG_CHUNK; i++) {
                        cur[i] = i < nb ? rowp[at + i] : 0;
                        up[i] = (y > 0 && i < nb) ? rowp[at + i - pitch] : 0;
                    }
                }
                png_unfilter_chunk<BPP>(cur, up, pa, pc, ft);
                if (nb == CK_PNG_CHUNK) {
                    __builtin_memcpy(rowp + at, cur, CK_PNG_CHUNK);
                } else {
#pragma unroll
                    for (int i = 0; i < CK_PNG_CHUNK; i++)
                        if (i < nb) rowp[at + i] = cur[i];
                }
                __builtin_memcpy(slot, cur, CK_PNG_CHUNK);
#pragma unroll
                for (int i = 0; i < 8; i++) { pa[i] = cur[CK_PNG_CHUNK - 8 + i]; pc[i] = up[CK_PNG_CHUNK - 8 + i]; }
                png_expand(slot, d, pal, c, w, out + (size_t)y * w * 3);
            }
            if (++c == D) { c = 0; y += PNG_TB; }
        }
        __syncthreads();                                         // the chunk is in memory before the row below reads it
    }
}

__global__ __launch_bounds__(PNG_TB) void png_unfilter_kernel(uint8_t* rows, const CkPngDesc* __restrict__ desc, const uint8_t* __restrict__ palettes,
                                                              int h, int w, uint8_t* __restrict__ out)
{
    __shared__ uint8_t slots[PNG_TB * CK_PNG_CHUNK];
    const CkPngDesc d = desc[blockIdx.x];
    uint8_t* img = rows + d.off;
    const uint8_t* pal = palettes + (size_t)blockIdx.x * 768;
    uint8_t* o = out + (size_t)blockIdx.x * h * w * 3;
    uint8_t* slot = slots + threadIdx.x * CK_PNG_CHUNK;
    switch (d.bpp) {
    case 1: png_unfilter_image<1>(img, d, pal, h, w, o, slot); break;
    case 2: png_unfilter_image<2>(img, d, pal, h, w, o, slot); break;
    case 3: png_unfilter_image<3>(img, d, pal, h, w, o, slot); break;
    case 4: png_unfilter_image<4>(img, d, pal, h, w, o, slot); break;
    case 6: png_unfilter_image<6>(img, d, pal, h, w, o, slot); break;
    case 8: png_unfilter_image<8>(img, d, pal, h, w, o, slot); break;
    default: break;
    }
}

int k_png_unfilter(ck_ctx* ctx, uint8_t* d_rows, const CkPngDesc* d_desc, const uint8_t* d_palettes, int n, int h, int w, uint8_t* d_bgr)
{
    TimeScope ts(ctx, "png_unfilter");
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)n), dim3(PNG_TB), 0, ctx->stream, d_rows, d_desc, d_palettes, h, w, d_bgr);
    CK_HIP(ctx, hipGetLastError());
    return CK_OK;
}

// ---- writing ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PNG_TB) void png_filter_kernel(const uint8_t* __restrict__ bgr, CkPngGeom g, int filter, uint8_t* __restrict__ filt)
{
    __shared__ uint32_t sum[5];
    const long long f = blockIdx.x / g.h, y = blockIdx.x % g.h;
    const uint8_t* img = bgr + (size_t)f * g.h * g.w * 3;
    const long long nb = g.row - 1;
    int ft = filter;
    if (filter < 0) {
        if (threadIdx.x < 5) sum[threadIdx.x] = 0;
        __syncthreads();
        uint32_t s[5] = {0, 0, 0, 0, 0};
        for (long long i = threadIdx.x; i < nb; i += PNG_TB) {
            int x, a, b, c;
            ck_png_context(img, g.w, y, i, &x, &a, &b, &c);
#pragma unroll
            for (int t = 0; t < 5; t++) s[t] += ck_png_cost((uint8_t)(x - ck_png_predict(t, a, b, c)));
        }
#pragma unroll
        for (int t = 0; t < 5; t++) atomicAdd(&sum[t], s[t]);
        __syncthreads();
        ft = ck_png_choose(sum);
    }
    uint8_t* dst = filt + (size_t)f * g.fbytes + y * g.row;
    if (threadIdx.x == 0) dst[0] = (uint8_t)ft;
    for (long long i = threadIdx.x; i < nb; i += PNG_TB) dst[1 + i] = ck_png_residual(img, g.w, y, i, ft);
}

// ---- the runs mode: where the runs of equal bytes start and end ----
// edges, a tile alone: lane i looks at its four bytes
__global__ __launch_bounds__(PNG_TB) void png_edges_kernel(const uint8_t* __restrict__ filt, CkPngGeom g, CkPngEdge* __restrict__ edge)
{
    __shared__ int lo, hi;                                       // the first position that differs from the first byte, the last that differs from the last
    const long long f = blockIdx.x / g.tiles, k = blockIdx.x % g.tiles, band = k / g.band_tiles, t = k % g.band_tiles;
    const int L = ck_png_tile_len(g, band, t);
    if (threadIdx.x == 0) { lo = L; hi = -1; }
    __syncthreads();
    const uint8_t* p = filt + (size_t)f * g.fbytes + ck_png_tile_at(g, band, t);
    uint32_t first = 0, last = 0;
    if (L > 0) {
        first = p[0]; last = p[L - 1];
        int mn = L, mx = -1;
        for (int j = 0; j < 4; j++) {
            const int i = 4 * threadIdx.x + j;
            if (i < L) {
                const uint32_t x = p[i];
                if (x != first && i < mn) mn = i;
                if (x != last) mx = i;
            }
        }
        if (mn < L) atomicMin(&lo, mn);
        if (mx >= 0) atomicMax(&hi, mx);
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                      // what ck_png_edge gives
        CkPngEdge e;
        e.first = (uint8_t)first; e.last = (uint8_t)last;
        e.head = (uint16_t)(L > 0 ? lo : 0); e.tail = (uint16_t)(L > 0 ? L - 1 - hi : 0);
        edge[blockIdx.x] = e;
    }
}

// join, a lane per band
__global__ __launch_bounds__(64) void png_join_kernel(CkPngGeom g, CkPngWork wk, long long n_bands)
{
    const long long gb = (long long)blockIdx.x * 64 + threadIdx.x;
    if (gb >= n_bands) return;
    const size_t k = (size_t)gb * g.band_tiles;
    ck_png_join_band(g, gb % g.bands, wk.edge + k, wk.before + k, wk.after + k);
}

// The runs of a lane's four positions 4 lane + j of a tile of L bytes at p: x[j] the bytes, s[j] and e[j] where the run of
// each starts and ends, counted from the tile's start (s down to -before, e up to L + after).  A position starts a run
// inside the tile where it is the tile's first or differs from the byte before it; the last start at or before a position
// and the first start behind it come from two scans over the lanes (lo, hi: PNG_TB words of LDS each).  Every lane of the
// workgroup calls it, with L > 0.
__device__ __forceinline__ void png_tile_runs(const uint8_t* __restrict__ p, int L, int before, int after, int* lo, int* hi,
                                              uint32_t (&x)[4], int (&s)[4], int (&e)[4])
{
    constexpr int NONE = 1 << 30;
    const int lane = threadIdx.x, i0 = 4 * lane;
    uint32_t prev = i0 > 0 && i0 <= L ? p[i0 - 1] : 0;
    bool st[4];
    int last = -1, first = NONE;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int i = i0 + j;
        x[j] = 0; st[j] = false;
        if (i < L) {
            x[j] = p[i];
            st[j] = i == 0 || x[j] != prev;
            prev = x[j];
            if (st[j]) { last = i; if (first == NONE) first = i; }
        }
    }
    __syncthreads();                                             // (the arrays may still be read by a call before this one)
    lo[lane] = last; hi[lane] = first;
    __syncthreads();
    for (int d = 1; d < PNG_TB; d <<= 1) {
        const int a = lane >= d ? lo[lane - d] : -1, b = lane + d < PNG_TB ? hi[lane + d] : NONE;
        __syncthreads();
        if (a > lo[lane]) lo[lane] = a;
        if (b < hi[lane]) hi[lane] = b;
        __syncthreads();
    }
    int cur = lane > 0 ? lo[lane - 1] : -1, nxt = lane + 1 < PNG_TB ? hi[lane + 1] : NONE;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (st[j]) cur = i0 + j;
        s[j] = cur <= 0 ? -before : cur;
    }
#pragma unroll
    for (int j = 3; j >= 0; j--) {
        e[j] = nxt == NONE ? L + after : nxt;
        if (st[j]) nxt = i0 + j;
    }
}

// count.  RUNS: over the tokens of the band's tiles, tile after tile
template <int RUNS>
__global__ __launch_bounds__(PNG_TB) void png_count_kernel(const uint8_t* __restrict__ filt, CkPngGeom g, uint32_t* __restrict__ count,
                                                           const uint32_t* __restrict__ before, const uint32_t* __restrict__ after)
{
    __shared__ uint32_t hist[RUNS ? CK_PNG_RUN_SYMS : 256];
    const long long f = blockIdx.x / g.bands, band = blockIdx.x % g.bands;
    const uint8_t* p = filt + (size_t)f * g.fbytes + ck_png_tile_at(g, band, 0);
    uint32_t* out = count + (size_t)blockIdx.x * ck_png_pitch(RUNS);
    if constexpr (!RUNS) {
        hist[threadIdx.x] = 0;
        __syncthreads();
        for (long long i = threadIdx.x, e = ck_png_band_bytes(g, band); i < e; i += PNG_TB) atomicAdd(&hist[p[i]], 1u);
        __syncthreads();
        out[threadIdx.x] = hist[threadIdx.x];
        if (threadIdx.x == 0) out[256] = 1;
    } else {
        __shared__ int lo[PNG_TB], hi[PNG_TB];
        for (int i = threadIdx.x; i < CK_PNG_RUN_SYMS; i += PNG_TB) hist[i] = 0;
        __syncthreads();
        for (long long t = 0; t < g.band_tiles; t++) {
            const int L = ck_png_tile_len(g, band, t);
            if (L == 0) break;
            const size_t k = (size_t)blockIdx.x * g.band_tiles + t;
            uint32_t x[4];
            int s[4], e[4];
            png_tile_runs(p + t * CK_PNG_TILE_BYTES, L, (int)before[k], (int)after[k], lo, hi, x, s, e);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int i = 4 * threadIdx.x + j;
                if (i < L) {
                    int tb;
                    uint32_t tail;
                    const int sym = ck_png_token(x[j], i - s[j] - 1, e[j] - s[j] - 1, &tb, &tail);
                    if (sym >= 0) atomicAdd(&hist[sym], 1u);
                }
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < CK_PNG_RUN_SYMS; i += PNG_TB) out[i] = i == 256 ? 1u : hist[i];
    }
}

constexpr int PNG_BUILD_TB = 320;
static_assert(PNG_BUILD_TB >= CK_PNG_HDR_FIELDS + 2 && PNG_BUILD_TB >= CK_PNG_RUN_HDR_FIELDS + 2,
              "a lane per header field, one for the end-of-block code, one for the zlib wrapper");
template <int RUNS>
__global__ __launch_bounds__(PNG_BUILD_TB) void png_build_kernel(const uint32_t* __restrict__ count, uint8_t* __restrict__ lens, uint16_t* __restrict__ codes)
{
    constexpr int NS = ck_png_syms(RUNS), PITCH = ck_png_pitch(RUNS);
    __shared__ uint32_t cnt[NS], work[NS];
    __shared__ uint16_t order[NS];
    __shared__ int m;
    const int s = threadIdx.x;
    if (s == 0) m = 0;
    if (s < NS) cnt[s] = count[(size_t)blockIdx.x * PITCH + s];
    __syncthreads();
    if (s < NS && cnt[s]) {
        order[ck_png_rank<NS>(cnt, s)] = (uint16_t)s;
        atomicAdd(&m, 1);
    }
    __syncthreads();
    if (s == 0) ck_png_lengths<NS>(cnt, order, m, work, lens + (size_t)blockIdx.x * PITCH, codes + (size_t)blockIdx.x * PITCH);
}

// size.  RUNS: the bits of the tokens that start in the tile
template <int RUNS>
__global__ __launch_bounds__(PNG_TB) void png_size_kernel(const uint8_t* __restrict__ filt, CkPngGeom g, const uint8_t* __restrict__ lens,
                                                          uint32_t* __restrict__ tile_bits, uint32_t* __restrict__ tile_a, uint32_t* __restrict__ tile_b,
                                                          const uint32_t* __restrict__ before, const uint32_t* __restrict__ after)
{
    __shared__ uint32_t acc[3];
    const long long f = blockIdx.x / g.tiles, k = blockIdx.x % g.tiles, band = k / g.band_tiles, t = k % g.band_tiles;
    const int L = ck_png_tile_len(g, band, t);
    if (threadIdx.x < 3) acc[threadIdx.x] = 0;
    __syncthreads();
    const uint8_t* p = filt + (size_t)f * g.fbytes + ck_png_tile_at(g, band, t);
    const uint8_t* bl = lens + (size_t)(f * g.bands + band) * ck_png_pitch(RUNS);
    uint32_t bits = 0, a = 0, b = 0;
    if constexpr (!RUNS) {
        for (int j = 0; j < 4; j++) {
            const int i = 4 * threadIdx.x + j;
            if (i < L) { const uint32_t x = p[i]; bits += bl[x]; a += x; b += (uint32_t)(L - i) * x; }
        }
    } else if (L > 0) {
        __shared__ int lo[PNG_TB], hi[PNG_TB];
        uint32_t x[4];
        int s[4], e[4];
        png_tile_runs(p, L, (int)before[blockIdx.x], (int)after[blockIdx.x], lo, hi, x, s, e);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = 4 * threadIdx.x + j;
            if (i < L) {
                int tb;
                uint32_t tail;
                const int sym = ck_png_token(x[j], i - s[j] - 1, e[j] - s[j] - 1, &tb, &tail);
                if (sym >= 0) bits += (uint32_t)(bl[sym] + tb);
                a += x[j]; b += (uint32_t)(L - i) * x[j];
            }
        }
    }
    atomicAdd(&acc[0], bits); atomicAdd(&acc[1], a); atomicAdd(&acc[2], b);
    __syncthreads();
    if (threadIdx.x == 0) { tile_bits[blockIdx.x] = acc[0]; tile_a[blockIdx.x] = acc[1]; tile_b[blockIdx.x] = acc[2]; }
}

// a lane per band, then a lane per frame over its bands
template <int RUNS>
__global__ __launch_bounds__(64) void png_scan_band_kernel(CkPngGeom g, CkPngWork wk, long long n_bands)
{
    const long long gb = (long long)blockIdx.x * 64 + threadIdx.x;
    if (gb >= n_bands) return;
    const size_t k = (size_t)gb * g.band_tiles;
    ck_png_scan_band(g, gb % g.bands, wk.tile_bits + k, wk.tile_a + k, wk.tile_b + k, wk.lens[(size_t)gb * ck_png_pitch(RUNS) + 256], wk.tile_off + k,
                     wk.band_bits + gb, wk.band_a + gb, wk.band_b + gb, ck_png_hdr_bits(RUNS));
}

__global__ void png_scan_kernel(CkPngGeom g, CkPngWork wk)
{
    const size_t f = blockIdx.x;
    if (threadIdx.x != 0) return;
    uint64_t bits;
    ck_png_scan_frame(g, wk.band_bits + f * g.bands, wk.band_a + f * g.bands, wk.band_b + f * g.bands, wk.band_off + f * g.bands, &bits, wk.adler + f);
    wk.frame_bits[f] = bits;
    wk.head[1 + f] = ck_png_zlib_bytes(bits);
}

// the frames' streams one behind the other, each on 16 bytes: head[0] the bytes of all of them
__global__ void png_frames_kernel(int m, CkPngWork wk)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint64_t at = 0;
    for (int f = 0; f < m; f++) { wk.out_off[f] = at; at += (wk.head[1 + f] + 15) & ~(uint64_t)15; }
    wk.out_off[m] = at;
    wk.head[0] = at;
}

__device__ __forceinline__ void png_or_bits(uint32_t* buf, uint64_t pos, uint32_t v, int nbits)
{
    const int s = (int)(pos & 31);
    if (!nbits) return;
    atomicOr(&buf[pos >> 5], v << s);
    if (s + nbits > 32) atomicOr(&buf[(pos >> 5) + 1], v >> (32 - s));
}

template <int RUNS>
__global__ __launch_bounds__(PNG_BUILD_TB) void png_put_header_kernel(CkPngGeom g, CkPngWork wk, uint32_t* __restrict__ pack)
{
    constexpr int FIELDS = ck_png_hdr_fields(RUNS), PITCH = ck_png_pitch(RUNS);
    const size_t gb = blockIdx.x, f = gb / g.bands, band = gb % g.bands;
    const uint8_t* bl = wk.lens + gb * PITCH;
    const uint64_t frame = wk.out_off[f] * 8;
    const int i = threadIdx.x;
    if (i < FIELDS) {
        uint32_t v;
        int nb, off;
        if constexpr (RUNS) ck_png_run_hdr_field(i, bl, band == (size_t)g.bands - 1, &v, &nb, &off);
        else ck_png_hdr_field(i, bl, band == (size_t)g.bands - 1, &v, &nb, &off);
        png_or_bits(pack, frame + 16 + wk.band_off[gb] + (uint64_t)off, v, nb);
    } else if (i == FIELDS) {                                    // the end-of-block code, behind the band's last tile
        const size_t last = f * g.tiles + band * g.band_tiles + g.band_tiles - 1;
        png_or_bits(pack, frame + 16 + wk.band_off[gb] + wk.tile_off[last] + wk.tile_bits[last], wk.codes[gb * PITCH + 256], bl[256]);
    } else if (i == FIELDS + 1 && band == 0) {                   // the zlib wrapper: 78 01 in front, the Adler-32 behind, high byte first
        png_or_bits(pack, frame, 0x0178u, 16);
        const uint32_t ad = wk.adler[f];
        const uint32_t sw = ad >> 24 | (ad >> 8 & 0xff00u) | (ad << 8 & 0xff0000u) | ad << 24;
        png_or_bits(pack, frame + (2 + (wk.frame_bits[f] + 7) / 8) * 8, sw, 32);
    }
}

// The bits of a tile's tokens.  RUNS: a match of up to 21 bits belongs to the tile that holds its first byte; the bytes it
// covers there hold no token, so only a match at the tile's last byte adds more than that byte's 15 bits: a tile has at
// most 1024 * 15 + 6 bits, which the words below hold beside the 31 bits of the tile's place in its first word.
constexpr int PNG_TILE_WORDS = (CK_PNG_TILE_BYTES * CK_PNG_MAX_BITS + 31 + 31) / 32 + 3;
template <int RUNS>
__global__ __launch_bounds__(PNG_TB) void png_put_kernel(CkPngGeom g, CkPngWork wk, uint32_t* __restrict__ pack)
{
    __shared__ uint32_t words[PNG_TILE_WORDS];
    __shared__ uint32_t scan[PNG_TB];
    const size_t gt = blockIdx.x, f = gt / g.tiles, k = gt % g.tiles, band = k / g.band_tiles, t = k % g.band_tiles;
    const int L = ck_png_tile_len(g, band, t);
    if (L == 0) return;
    const uint64_t P = wk.out_off[f] * 8 + 16 + wk.band_off[f * g.bands + band] + wk.tile_off[gt];
    const int sh = (int)(P & 31);
    for (int i = threadIdx.x; i < PNG_TILE_WORDS; i += PNG_TB) words[i] = 0;
    const uint8_t* p = wk.filt + f * g.fbytes + ck_png_tile_at(g, band, t);
    const uint8_t* bl = wk.lens + (f * g.bands + band) * ck_png_pitch(RUNS);
    const uint16_t* bc = wk.codes + (f * g.bands + band) * ck_png_pitch(RUNS);
    uint64_t acc = 0;
    uint32_t nb = 0;
    // RUNS: a lane's four positions can hold three literals and a match, 66 bits: the tokens are kept apart (their symbols,
    // -1: none, and what follows the symbol's code) and go to the words one by one
    int sym[4] = {-1, -1, -1, -1}, tb[4] = {0, 0, 0, 0};
    uint32_t tail[4] = {0, 0, 0, 0};
    if constexpr (!RUNS) {
        for (int j = 0; j < 4; j++) {
            const int i = 4 * threadIdx.x + j;
            if (i < L) { const uint32_t x = p[i]; acc |= (uint64_t)bc[x] << nb; nb += bl[x]; }
        }
    } else {
        __shared__ int lo[PNG_TB], hi[PNG_TB];
        uint32_t x[4];
        int s[4], e[4];
        png_tile_runs(p, L, (int)wk.before[gt], (int)wk.after[gt], lo, hi, x, s, e);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = 4 * threadIdx.x + j;
            if (i < L) {
                sym[j] = ck_png_token(x[j], i - s[j] - 1, e[j] - s[j] - 1, &tb[j], &tail[j]);
                if (sym[j] >= 0) nb += (uint32_t)(bl[sym[j]] + tb[j]);
            }
        }
    }
    scan[threadIdx.x] = nb;
    __syncthreads();
    for (int d = 1; d < PNG_TB; d <<= 1) {                       // inclusive prefix sums of the lanes' bits
        const uint32_t v = threadIdx.x >= (unsigned)d ? scan[threadIdx.x - d] : 0;
        __syncthreads();
        scan[threadIdx.x] += v;
        __syncthreads();
    }
    if constexpr (!RUNS) {
        if (nb) {
            const uint32_t q = (uint32_t)sh + scan[threadIdx.x] - nb;
            const int s = (int)(q & 31);
            const uint64_t hi = s ? acc >> (32 - s) : acc >> 32;
            atomicOr(&words[q >> 5], (uint32_t)acc << s);
            if ((uint32_t)hi) atomicOr(&words[(q >> 5) + 1], (uint32_t)hi);
            if (hi >> 32) atomicOr(&words[(q >> 5) + 2], (uint32_t)(hi >> 32));
        }
    } else {
        uint32_t q = (uint32_t)sh + scan[threadIdx.x] - nb;
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (sym[j] >= 0) {
                png_or_bits(words, q, bc[sym[j]], bl[sym[j]]);
                q += bl[sym[j]];
                png_or_bits(words, q, tail[j], tb[j]);
                q += (uint32_t)tb[j];
            }
    }
    __syncthreads();
    const int nw = (int)(((uint32_t)sh + scan[PNG_TB - 1] + 31) >> 5);
    uint32_t* dst = pack + (P >> 5);
    for (int i = threadIdx.x; i < nw; i += PNG_TB) {
        if (i == 0 || i == nw - 1) atomicOr(&dst[i], words[i]);
        else dst[i] = words[i];
    }
}

template <int RUNS>
static int png_enc_measure(ck_ctx* ctx, const uint8_t* d_bgr, int m, const CkPngGeom& g, int filter, const CkPngWork& wk)
{
    const unsigned bands = (unsigned)(m * g.bands), tiles = (unsigned)(m * g.tiles);
    {
        TimeScope ts(ctx, "png_filter");
        hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)m * g.h), dim3(PNG_TB), 0, ctx->stream, d_bgr, g, filter, wk.filt);
        CK_HIP(ctx, hipGetLastError());
    }
    if constexpr (RUNS) {
        {
            TimeScope ts(ctx, "png_edges");
            hipLaunchKernelGGL(png_edges_kernel, dim3(tiles), dim3(PNG_TB), 0, ctx->stream, (const uint8_t*)wk.filt, g, wk.edge);
            CK_HIP(ctx, hipGetLastError());
        }
        TimeScope ts(ctx, "png_join");
        hipLaunchKernelGGL(png_join_kernel, dim3((bands + 63) / 64), dim3(64), 0, ctx->stream, g, wk, (long long)bands);
        CK_HIP(ctx, hipGetLastError());
    }
    {
        TimeScope ts(ctx, "png_count");
        hipLaunchKernelGGL(png_count_kernel<RUNS>, dim3(bands), dim3(PNG_TB), 0, ctx->stream, (const uint8_t*)wk.filt, g, wk.count,
                           (const uint32_t*)wk.before, (const uint32_t*)wk.after);
        CK_HIP(ctx, hipGetLastError());
    }
    {
        TimeScope ts(ctx, "png_build");
        hipLaunchKernelGGL(png_build_kernel<RUNS>, dim3(bands), dim3(PNG_BUILD_TB), 0, ctx->stream, (const uint32_t*)wk.count, wk.lens, wk.codes);
        CK_HIP(ctx, hipGetLastError());
    }
    {
        TimeScope ts(ctx, "png_size");
        hipLaunchKernelGGL(png_size_kernel<RUNS>, dim3(tiles), dim3(PNG_TB), 0, ctx->stream, (const uint8_t*)wk.filt, g, (const uint8_t*)wk.lens, wk.tile_bits,
                           wk.tile_a, wk.tile_b, (const uint32_t*)wk.before, (const uint32_t*)wk.after);
        CK_HIP(ctx, hipGetLastError());
    }
    TimeScope ts(ctx, "png_scan");
    hipLaunchKernelGGL(png_scan_band_kernel<RUNS>, dim3((bands + 63) / 64), dim3(64), 0, ctx->stream, g, wk, (long long)bands);
    CK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(png_scan_kernel, dim3((unsigned)m), dim3(64), 0, ctx->stream, g, wk);
    CK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(png_frames_kernel, dim3(1), dim3(64), 0, ctx->stream, m, wk);
    CK_HIP(ctx, hipGetLastError());
    return CK_OK;
}

int k_png_enc_measure(ck_ctx* ctx, const uint8_t* d_bgr, int m, const CkPngGeom& g, int filter, const CkPngWork& wk, int runs)
{
    return runs ? png_enc_measure<1>(ctx, d_bgr, m, g, filter, wk) : png_enc_measure<0>(ctx, d_bgr, m, g, filter, wk);
}

template <int RUNS>
static int png_enc_put(ck_ctx* ctx, int m, const CkPngGeom& g, const CkPngWork& wk, uint32_t* d_pack, uint64_t pack_bytes)
{
    CK_HIP(ctx, hipMemsetAsync(d_pack, 0, pack_bytes, ctx->stream));
    TimeScope ts(ctx, "png_put");
    hipLaunchKernelGGL(png_put_header_kernel<RUNS>, dim3((unsigned)(m * g.bands)), dim3(PNG_BUILD_TB), 0, ctx->stream, g, wk, d_pack);
    CK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(png_put_kernel<RUNS>, dim3((unsigned)(m * g.tiles)), dim3(PNG_TB), 0, ctx->stream, g, wk, d_pack);
    CK_HIP(ctx, hipGetLastError());
    return CK_OK;
}

int k_png_enc_put(ck_ctx* ctx, int m, const CkPngGeom& g, const CkPngWork& wk, uint32_t* d_pack, uint64_t pack_bytes, int runs)
{
    return runs ? png_enc_put<1>(ctx, m, g, wk, d_pack, pack_bytes) : png_enc_put<0>(ctx, m, g, wk, d_pack, pack_bytes);
}
