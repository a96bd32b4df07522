// k_jpeg_enc_huff.hip -- the Huffman stage of a baseline JPEG encode on the GPU: the steps of ck_jpeg_enc_stage.h (size, scan,
// put, stuff), each a launch of its own on the context's stream.  No kernel waits for another workgroup: whatever crosses
// workgroups is the next launch, so a wrong offset could give wrong bytes but never a hang.
//
//   jpeg_enc_size   one wave per block tile, a lane per block in scan order.  The tile's blocks are staged in LDS with 16-byte
//                   loads (rows of 33 dwords: the lanes' zigzag reads fall on different banks), the tables and the zigzag
//                   order beside them.  bits[block], the tile's sum, and an atomicMin of (frame << 32 | block) for a
//                   block the tables cannot code.
//   jpeg_enc_scan   tile sums -> tile offsets and B per segment (a wave per segment); U per segment -> segment offsets per
//                   frame (a workgroup per frame); frames -> their places in the bit buffer (one workgroup).
//   jpeg_enc_put    one wave per block tile again: the lanes OR their codes into the tile's words in LDS (many short blocks
//                   share a word), the lane of a segment's last block adds the pad ones, then whole dwords go out
//                   byte-swapped: the first and the last by atomicOr into the zeroed buffer, the others by plain stores.
//   jpeg_enc_histo, jpeg_enc_tables   with optimised tables only, in front of the others: the symbols of every block tile counted
//                   in LDS and added to the frame's 4 x 256 counters; then a wave per (frame, table) runs libjpeg's
//                   jpeg_gen_optimal_table -- each merge two wave-wide arg-min reductions, one lane the code sizes (from the
//                   list of merges, backwards) and the length limiting, every loop bounded by a constant -- and a workgroup per frame puts the frame's header
//                   together.  size, put and stuff then read the tables and the header of their tile's frame.
//   jpeg_enc_stuff  FF bytes per byte tile; their sums before each tile of a frame and the stream lengths (a workgroup per
//                   frame); the frames' places in the packed buffer (one workgroup); then every unstuffed byte to its
//                   place with its 00, its RSTn or EOI behind it, and the header in front of each frame.
//
// Bounds: a tile index comes from the grid and is checked against the count; a block index from ck_enc_tile_blocks, inside
// the frame; the LDS sink drops a code that would leave the tile's words; every store into the bit buffer and the packed
// buffer is checked against the buffer's size, so offsets that were wrong could not write outside them.
#include "ck_common.h"
#include "ck_jpeg_enc_stage.h"

namespace {

constexpr int TB = CK_ENC_TILE_BLOCKS;
constexpr int TY = CK_ENC_TILE_BYTES;
constexpr int ROW = 33;                                      // dwords of a staged block: 32 and one to spread the banks
static_assert(TB == 64, "a block tile is one wave");
static_assert(TY == 1024, "a byte tile is a dword for each of 256 lanes");
constexpr int TAB_DWORDS = (int)(sizeof(CkEncTables) / 4);

__device__ inline uint32_t wave_incl_scan(uint32_t v)
{
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}
__device__ inline uint32_t wave_sum(uint32_t v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    return __shfl(v, 0);
}
// inclusive scan over the 256 lanes of a workgroup; s: 256 words of LDS
__device__ inline uint64_t wg_incl_scan(uint64_t v, uint64_t* s)
{
    const int i = threadIdx.x;
    s[i] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint64_t o = i >= d ? s[i - d] : 0;
        __syncthreads();
        s[i] += o;
        __syncthreads();
    }
    const uint64_t r = s[i];
    __syncthreads();
    return r;
}

// the tile's blocks into LDS; s_place: the places of the tile's blocks
__device__ inline void stage_blocks(const int16_t* __restrict__ fc, const CkEncGeom& g, int64_t b0, int cnt, uint32_t* s_blk, int64_t* s_place)
{
    const int lane = threadIdx.x;
    if (lane < cnt) s_place[lane] = ck_enc_place(g, b0 + lane);
    __syncthreads();
    for (int it = 0; it < 8; it++) {
        const int idx = it * TB + lane, bl = idx >> 3, part = idx & 7;
        if (bl < cnt) {
            const uint4 v = *(const uint4*)(fc + s_place[bl] * 64 + part * 8);
            uint32_t* d = s_blk + bl * ROW + part * 4;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
    }
    __syncthreads();
}
// the tables (the standard ones, or those of the tile's frame), the zigzag order and the tile's blocks into LDS
__device__ inline void stage_tile(const uint8_t* __restrict__ tables, const uint8_t* __restrict__ zz, const int16_t* __restrict__ fc,
                                  const CkEncGeom& g, int64_t b0, int cnt, uint32_t* s_tab, uint8_t* s_zz, uint32_t* s_blk, int64_t* s_place)
{
    const int lane = threadIdx.x;
    const uint32_t* tab = (const uint32_t*)tables;
    for (int i = lane; i < TAB_DWORDS; i += TB) s_tab[i] = tab[i];
    s_zz[lane] = zz[lane];
    stage_blocks(fc, g, b0, cnt, s_blk, s_place);
}

__device__ inline int pred_of(const int16_t* __restrict__ fc, const CkEncGeom& g, int64_t b)
{
    const int64_t pb = ck_enc_pred_block(g, b);
    return pb < 0 ? 0 : (int)fc[ck_enc_place(g, pb) * 64];
}

// OWN: every frame has a CkEncTables of its own at tables + f * sizeof(CkEncTables); otherwise one set for all
template <bool OWN>
__global__ __launch_bounds__(TB) void enc_size_kernel(const int16_t* __restrict__ coef, const uint8_t* __restrict__ tables,
                                                      const uint8_t* __restrict__ zz, CkEncGeom g,
                                                      long long n_tiles, uint32_t* __restrict__ bits, uint32_t* __restrict__ tile_bits,
                                                      unsigned long long* __restrict__ fail)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[TAB_DWORDS];
    __shared__ uint8_t s_zz[64];
    __shared__ uint32_t s_blk[TB * ROW];
    __shared__ int64_t s_place[TB];
    const long long tile = blockIdx.x;
    if (tile >= n_tiles) return;
    const int64_t ftiles = g.nseg * g.seg_tiles, f = tile / ftiles, r = tile % ftiles;
    int64_t b0;
    int cnt;
    ck_enc_tile_blocks(g, r / g.seg_tiles, r % g.seg_tiles, &b0, &cnt);
    const int16_t* fc = coef + f * g.blocks * 64;
    stage_tile(OWN ? tables + f * sizeof(CkEncTables) : tables, zz, fc, g, b0, cnt, s_tab, s_zz, s_blk, s_place);
    const int lane = threadIdx.x;
    uint32_t v = 0;
    if (lane < cnt) {
        const int64_t b = b0 + lane;
        v = ck_enc_block_bits((const int16_t*)(s_blk + lane * ROW), pred_of(fc, g, b), ck_enc_is_chroma(g, b), (const CkEncTables*)s_tab, s_zz);
        bits[f * g.blocks + b] = v;
        if (v & CK_ENC_FAIL) {
            atomicMin(fail, ((unsigned long long)f << 32) | (unsigned long long)b);
            v = 0;
        }
    }
    const uint32_t sum = wave_sum(v);
    if (lane == 0) tile_bits[tile] = sum;
}

// a wave per segment: offsets of its tiles in it, its bits
__global__ __launch_bounds__(256) void enc_scan_seg_kernel(const uint32_t* __restrict__ tile_bits, long long n_segs, long long seg_tiles,
                                                           uint64_t* __restrict__ tile_off, uint64_t* __restrict__ seg_bits)
{
    const long long seg = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (seg >= n_segs) return;
    uint64_t carry = 0;
    for (long long t0 = 0; t0 < seg_tiles; t0 += 64) {
        const long long t = t0 + lane;
        const uint32_t v = t < seg_tiles ? tile_bits[seg * seg_tiles + t] : 0;
        const uint32_t inc = wave_incl_scan(v);                  // (64 tiles hold less than 2^23 bits)
        if (t < seg_tiles) tile_off[seg * seg_tiles + t] = carry + inc - v;
        carry += __shfl(inc, 63);
    }
    if (lane == 0) seg_bits[seg] = carry;
}

// a workgroup per frame: byte offsets of its segments, nseg + 1 of them
__global__ __launch_bounds__(256) void enc_scan_frame_kernel(const uint64_t* __restrict__ seg_bits, long long nseg, uint64_t* __restrict__ seg_u0)
{
    __shared__ uint64_t s[256];
    const long long f = blockIdx.x;
    uint64_t carry = 0;
    for (long long k0 = 0; k0 < nseg; k0 += 256) {
        const long long k = k0 + threadIdx.x;
        const uint64_t u = k < nseg ? ck_enc_seg_bytes(seg_bits[f * nseg + k]) : 0;
        const uint64_t inc = wg_incl_scan(u, s);
        if (k < nseg) seg_u0[f * (nseg + 1) + k] = carry + inc - u;
        s[threadIdx.x] = inc;
        __syncthreads();
        carry += s[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) seg_u0[f * (nseg + 1) + nseg] = carry;
}

// one workgroup: v[f * stride], each rounded up to `align`, end to end -> off[0 .. m], the sum to *total as well (nullable)
__global__ __launch_bounds__(256) void enc_scan_aligned_kernel(const uint64_t* __restrict__ v, long long stride, long long m, uint64_t align,
                                                               uint64_t* __restrict__ off, uint64_t* __restrict__ total)
{
    __shared__ uint64_t s[256];
    uint64_t carry = 0;
    for (long long f0 = 0; f0 < m; f0 += 256) {
        const long long f = f0 + threadIdx.x;
        const uint64_t u = f < m ? ck_enc_up(v[f * stride], align) : 0;
        const uint64_t inc = wg_incl_scan(u, s);
        if (f < m) off[f] = carry + inc - u;
        s[threadIdx.x] = inc;
        __syncthreads();
        carry += s[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        off[m] = carry;
        if (total) *total = carry;
    }
}

// the host's CkEncWordSink over LDS: atomics, and a code that would leave the tile's words is dropped
struct LdsSink {
    uint32_t* words;
    uint32_t pos, limit;
    __device__ inline void put(uint32_t v, int len)
    {
        if (pos + (uint32_t)len > limit) return;
        const uint64_t x = (uint64_t)v << (64 - (int)(pos & 31) - len);
        atomicOr(words + (pos >> 5), (uint32_t)(x >> 32));
        if ((uint32_t)x) atomicOr(words + (pos >> 5) + 1, (uint32_t)x);
        pos += (uint32_t)len;
    }
};

// OWN: as in enc_size_kernel; a tile then has CK_ENC_OPT_TILE_WORDS words
template <bool OWN>
__global__ __launch_bounds__(TB) void enc_put_kernel(const int16_t* __restrict__ coef, const uint8_t* __restrict__ tables,
                                                     const uint8_t* __restrict__ zz, CkEncGeom g, long long n_tiles, const uint32_t* __restrict__ bits, const uint32_t* __restrict__ tile_bits,
                                                     const uint64_t* __restrict__ tile_off, const uint64_t* __restrict__ seg_bits,
                                                     const uint64_t* __restrict__ seg_u0, const uint64_t* __restrict__ frame_u0,
                                                     uint32_t* __restrict__ buf, unsigned long long buf_words)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[TAB_DWORDS];
    __shared__ uint8_t s_zz[64];
    __shared__ uint32_t s_blk[TB * ROW];
    __shared__ int64_t s_place[TB];
    constexpr int WORDS = OWN ? CK_ENC_OPT_TILE_WORDS : CK_ENC_TILE_WORDS;
    __shared__ uint32_t s_words[WORDS];
    const long long tile = blockIdx.x;
    if (tile >= n_tiles) return;
    const int64_t ftiles = g.nseg * g.seg_tiles, f = tile / ftiles, r = tile % ftiles, k = r / g.seg_tiles;
    int64_t b0;
    int cnt;
    ck_enc_tile_blocks(g, k, r % g.seg_tiles, &b0, &cnt);
    if (!cnt) return;
    const uint64_t sbits = seg_bits[f * g.nseg + k], toff = tile_off[tile];
    const uint32_t tb = tile_bits[tile];
    const uint64_t p0 = 8 * (frame_u0[f] + seg_u0[f * (g.nseg + 1) + k]) + toff;
    const int pad = toff + tb == sbits ? ck_enc_seg_pad(sbits) : 0;
    const uint32_t first = (uint32_t)(p0 & 31), nbits = tb + (uint32_t)pad;
    const uint32_t nw = (first + nbits + 31) / 32;
    if (nw > (uint32_t)WORDS) return;
    const int lane = threadIdx.x;
    for (uint32_t i = lane; i < nw; i += TB) s_words[i] = 0;
    const int16_t* fc = coef + f * g.blocks * 64;
    stage_tile(OWN ? tables + f * sizeof(CkEncTables) : tables, zz, fc, g, b0, cnt, s_tab, s_zz, s_blk, s_place);
    const uint32_t mine = lane < cnt ? bits[f * g.blocks + b0 + lane] : 0;
    const uint32_t inc = wave_incl_scan(mine);
    if (lane < cnt) {
        const int64_t b = b0 + lane;
        LdsSink sink{s_words, first + inc - mine, first + nbits};
        ck_enc_block_put((const int16_t*)(s_blk + lane * ROW), pred_of(fc, g, b), ck_enc_is_chroma(g, b), (const CkEncTables*)s_tab, s_zz, sink);
        if (lane == cnt - 1 && pad) sink.put((1u << pad) - 1, pad);
    }
    __syncthreads();
    const unsigned long long w0 = p0 >> 5;
    for (uint32_t i = lane; i < nw; i += TB) {
        if (w0 + i >= buf_words) break;
        const uint32_t v = ck_enc_bswap(s_words[i]);
        if (ck_enc_flush_how((int)i, (int)nw)) atomicOr(buf + w0 + i, v); else buf[w0 + i] = v;
    }
}

__device__ inline uint32_t ff_bytes(uint32_t w, int valid)
{
    uint32_t c = 0;
    for (int j = 0; j < valid; j++) c += ((w >> (8 * j)) & 255u) == 255u;
    return c;
}

// FF bytes of every byte tile (the slack behind a frame's bytes is zero)
__global__ __launch_bounds__(256) void enc_ff_count_kernel(const uint32_t* __restrict__ buf, uint32_t* __restrict__ ff_cnt)
{
    __shared__ uint32_t s_w[4];
    const uint32_t c = wave_sum(ff_bytes(buf[(size_t)blockIdx.x * 256 + threadIdx.x], 4));
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) ff_cnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// a workgroup per frame: FF bytes before each of its byte tiles, and the length of its stream
__global__ __launch_bounds__(256) void enc_scan_ff_kernel(const uint32_t* __restrict__ ff_cnt, const uint64_t* __restrict__ frame_u0,
                                                          const uint64_t* __restrict__ seg_u0, long long nseg, uint64_t header,
                                                          const uint32_t* __restrict__ hlen, uint32_t* __restrict__ ff_off, uint64_t* __restrict__ len)
{
    __shared__ uint64_t s[256];
    const long long f = blockIdx.x;
    const long long t_begin = (long long)(frame_u0[f] / TY), t_end = (long long)(frame_u0[f + 1] / TY);
    uint64_t carry = 0;
    for (long long t0 = t_begin; t0 < t_end; t0 += 256) {
        const long long t = t0 + threadIdx.x;
        const uint64_t c = t < t_end ? ff_cnt[t] : 0;
        const uint64_t inc = wg_incl_scan(c, s);
        if (t < t_end) ff_off[t] = (uint32_t)(carry + inc - c);
        s[threadIdx.x] = inc;
        __syncthreads();
        carry += s[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) len[f] = ck_enc_stream_len(hlen ? hlen[f] : header, seg_u0[f * (nseg + 1) + nseg], carry, nseg);
}

// a workgroup per byte tile, a dword per lane: every byte to its place in the packed streams.  hlen (nullable): the frames have
// headers of their own, hlen[f] bytes at headers + f * CK_ENC_HEADER_SLOT
__global__ __launch_bounds__(256) void enc_stuff_kernel(const uint32_t* __restrict__ buf, const uint32_t* __restrict__ ff_off,
                                                        const uint64_t* __restrict__ frame_u0, const uint64_t* __restrict__ seg_u0,
                                                        const uint64_t* __restrict__ out_off, long long m, long long nseg,
                                                        const uint8_t* __restrict__ headers, uint32_t one_hl, const uint32_t* __restrict__ hlen,
                                                        uint8_t* __restrict__ pack, unsigned long long pack_bytes)
{
    __shared__ uint32_t s_w[4];
    const uint64_t byte0 = (uint64_t)blockIdx.x * TY;
    long long lo = 0, hi = m - 1;                                // the frame of this tile: the last one that starts at or before it
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (frame_u0[mid] <= byte0) lo = mid; else hi = mid - 1;
    }
    const long long f = lo;
    const uint8_t* header = hlen ? headers + f * CK_ENC_HEADER_SLOT : headers;
    const uint32_t hl = hlen ? (hlen[f] <= (uint32_t)CK_ENC_HEADER_SLOT ? hlen[f] : 0) : one_hl;
    const uint64_t* su = seg_u0 + f * (nseg + 1);
    const uint64_t u = su[nseg], i0 = byte0 - frame_u0[f] + (uint64_t)threadIdx.x * 4;
    const uint32_t w = buf[(size_t)blockIdx.x * 256 + threadIdx.x];
    const int valid = i0 >= u ? 0 : (u - i0 < 4 ? (int)(u - i0) : 4);
    const uint32_t mine = ff_bytes(w, valid);
    const uint32_t inc = wave_incl_scan(mine);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) s_w[wave] = inc;
    __syncthreads();
    uint64_t ff = (uint64_t)ff_off[blockIdx.x] + inc - mine;
    for (int j = 0; j < wave; j++) ff += s_w[j];
    const uint64_t at = out_off[f];
    if (at + hl > pack_bytes) return;
    if (byte0 == frame_u0[f])
        for (uint32_t i = threadIdx.x; i < hl; i += 256)
            if (at + i < pack_bytes) pack[at + i] = header[i];
    for (int j = 0; j < valid; j++) {
        const unsigned c = (w >> (8 * j)) & 255u;
        const uint64_t i = i0 + (uint64_t)j;
        ck_enc_emit(pack + at + hl, pack + pack_bytes, su, nseg, i, c, ff);
        ff += c == 255u;
    }
}

// ---- optimised tables: histo, tables ----
// one wave per block tile, a lane per block, staged as enc_size_kernel stages its blocks: the symbols of the tile into a
// histogram in LDS, its non-zero counters into the frame's 4 x 256 by integer atomics.  A symbol is below 256 whatever the
// coefficients are, so no counter outside the tables is touched.
struct LdsInc {
    __device__ inline void operator()(uint32_t* c) const { atomicAdd(c, 1u); }
};
__global__ __launch_bounds__(TB) void enc_histo_kernel(const int16_t* __restrict__ coef, const uint8_t* __restrict__ zz, CkEncGeom g, long long n_tiles,
                                                       uint32_t* __restrict__ freq)
{
    __shared__ uint8_t s_zz[64];
    __shared__ uint32_t s_blk[TB * ROW];
    __shared__ int64_t s_place[TB];
    __shared__ uint32_t s_hist[4 * 256];
    const long long tile = blockIdx.x;
    if (tile >= n_tiles) return;
    const int64_t ftiles = g.nseg * g.seg_tiles, f = tile / ftiles, r = tile % ftiles;
    int64_t b0;
    int cnt;
    ck_enc_tile_blocks(g, r / g.seg_tiles, r % g.seg_tiles, &b0, &cnt);
    if (!cnt) return;
    const int lane = threadIdx.x;
    const int16_t* fc = coef + f * g.blocks * 64;
    s_zz[lane] = zz[lane];
    for (int i = lane; i < 4 * 256; i += TB) s_hist[i] = 0;
    stage_blocks(fc, g, b0, cnt, s_blk, s_place);
    if (lane < cnt) {
        const int64_t b = b0 + lane;
        ck_enc_block_histo<LdsInc>((const int16_t*)(s_blk + lane * ROW), pred_of(fc, g, b), ck_enc_is_chroma(g, b), s_hist, s_zz);
    }
    __syncthreads();
    for (int i = lane; i < 4 * 256; i += TB) {
        const uint32_t c = s_hist[i];
        if (c) atomicAdd(freq + f * (4 * 256) + i, c);
    }
}

// ck_enc_optimal_table run by one wave: the least entry by a reduction over a 64-bit key -- the sum, then 256 - index, so the
// larger index wins among equals (a sum stays below 2^55: CK_ENC_OPT_MAX_BLOCKS) -- and lane 0 for the rest
struct WaveExec {
    int lane;
    __device__ inline int least(const uint64_t* freq, int skip) const
    {
        unsigned long long best = ~0ull;
        for (int i = lane; i <= 256; i += TB) {
            const unsigned long long v = freq[i];
            if (i != skip && v) {
                const unsigned long long key = (v << 9) | (unsigned long long)(256 - i);
                best = key < best ? key : best;
            }
        }
        for (int d = 32; d > 0; d >>= 1) {
            const unsigned long long o = __shfl_xor(best, d);
            best = o < best ? o : best;
        }
        return best == ~0ull ? -1 : 256 - (int)(best & 511ull);
    }
    __device__ inline bool one() const { return lane == 0; }
    __device__ inline void sync() const { __syncthreads(); }
};

// a wave per (frame, table): the table's counters -> its CkEncHuff in the frame's CkEncTables, its DHT segment and its length
__global__ __launch_bounds__(TB) void enc_tables_kernel(const uint32_t* __restrict__ freq, int ntab, uint8_t* __restrict__ tables,
                                                        uint8_t* __restrict__ dht, uint32_t* __restrict__ dht_len)
{
    __shared__ CkEncTreeWork s_w;
    __shared__ __attribute__((aligned(16))) CkEncHuff s_huff;
    __shared__ __attribute__((aligned(16))) uint8_t s_dht[CK_ENC_DHT_SLOT];
    __shared__ uint8_t s_bits[16], s_vals[256];
    __shared__ int32_t s_count;
    __shared__ uint32_t s_len;
    const long long ft = blockIdx.x, f = ft >> 2;
    const int t = (int)(ft & 3), lane = threadIdx.x;
    if (t >= ntab) return;
    for (int i = lane; i < 256; i += TB) { s_w.freq[i] = freq[ft * 256 + i]; s_vals[i] = 0; }
    for (int i = lane; i < CK_ENC_DHT_SLOT; i += TB) s_dht[i] = 0;
    __syncthreads();
    ck_enc_optimal_table(&s_w, s_bits, s_vals, &s_count, WaveExec{lane});
    if (lane == 0) {
        ck_enc_fill(&s_huff, s_bits, s_vals);
        s_len = ck_enc_dht(s_dht, t, s_bits, s_vals, s_count);
    }
    __syncthreads();
    const int slot = (t & 1) * 2 + (t >> 1);                     // CkEncTables: dc[0], dc[1], ac[0], ac[1]
    uint32_t* dst = (uint32_t*)(tables + f * sizeof(CkEncTables) + slot * sizeof(CkEncHuff));
    for (int i = lane; i < (int)(sizeof(CkEncHuff) / 4); i += TB) dst[i] = ((const uint32_t*)&s_huff)[i];
    uint32_t* dd = (uint32_t*)(dht + ft * CK_ENC_DHT_SLOT);
    for (int i = lane; i < CK_ENC_DHT_SLOT / 4; i += TB) dd[i] = ((const uint32_t*)s_dht)[i];
    if (lane == 0) dht_len[ft] = s_len;
}

// a workgroup per frame: its header and the header's length (0, and nothing written, if it would not fit its slot)
__global__ __launch_bounds__(256) void enc_header_kernel(const uint8_t* __restrict__ pre, uint32_t pre_len, const uint8_t* __restrict__ post,
                                                         uint32_t post_len, const uint8_t* __restrict__ dht, const uint32_t* __restrict__ dht_len,
                                                         int ntab, uint8_t* __restrict__ headers, uint32_t* __restrict__ hlen)
{
    const long long f = blockIdx.x;
    uint32_t dl[4] = {0, 0, 0, 0};
    for (int t = 0; t < ntab && t < 4; t++) dl[t] = dht_len[f * 4 + t] <= (uint32_t)CK_ENC_DHT_SLOT ? dht_len[f * 4 + t] : 0;
    const uint32_t total = ck_enc_header_len(pre_len, dl, ntab, post_len);
    const bool fits = total <= (uint32_t)CK_ENC_HEADER_SLOT;
    if (fits)
        for (uint32_t i = threadIdx.x; i < total; i += 256)
            headers[f * CK_ENC_HEADER_SLOT + i] = ck_enc_header_byte(i, pre, pre_len, dht + f * 4 * CK_ENC_DHT_SLOT, dl, ntab, post);
    if (threadIdx.x == 0) hlen[f] = fits ? total : 0;
}

}  // namespace

int k_jpeg_enc_measure(ck_ctx* ctx, const int16_t* d_coef, int m, const CkEncGeom& g, const CkEncWork& w)
{
    if (m <= 0) return ck_fail(ctx, CK_ERR_ARG, "k_jpeg_enc_measure: nothing to code");
    const long long n_tiles = (long long)m * g.nseg * g.seg_tiles, n_segs = (long long)m * g.nseg;
    if (n_tiles > 0x7fffffffLL) return ck_fail(ctx, CK_ERR_ARG, "%lld block tiles in one pass", n_tiles);
    CK_HIP(ctx, hipMemsetAsync(w.head, 0xFF, sizeof(uint64_t), ctx->stream));
    const uint8_t* zz = w.consts + sizeof(CkEncTables);
    if (w.freq) {
        // optimised tables: count, then a table per (frame, table) and a header per frame, before anything is sized
        const int ntab = g.mcu_blocks == 1 ? 2 : 4;
        CK_HIP(ctx, hipMemsetAsync(w.freq, 0, (size_t)m * 4 * 256 * sizeof(uint32_t), ctx->stream));
        CK_HIP(ctx, hipMemsetAsync(w.tables, 0, (size_t)m * sizeof(CkEncTables), ctx->stream));
        {
            TimeScope ts(ctx, "jpeg_enc_histo");
            hipLaunchKernelGGL(enc_histo_kernel, dim3((unsigned)n_tiles), dim3(TB), 0, ctx->stream, d_coef, zz, g, n_tiles, w.freq);
            CK_HIP(ctx, hipGetLastError());
        }
        TimeScope ts(ctx, "jpeg_enc_tables");
        hipLaunchKernelGGL(enc_tables_kernel, dim3((unsigned)m * 4), dim3(TB), 0, ctx->stream, (const uint32_t*)w.freq, ntab, w.tables, w.dht, w.dht_len);
        CK_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(enc_header_kernel, dim3((unsigned)m), dim3(256), 0, ctx->stream, w.pre, w.pre_len, w.post, w.post_len, (const uint8_t*)w.dht,
                           (const uint32_t*)w.dht_len, ntab, w.headers, w.hlen);
        CK_HIP(ctx, hipGetLastError());
    }
    {
        TimeScope ts(ctx, "jpeg_enc_size");
        if (w.freq)
            hipLaunchKernelGGL(enc_size_kernel<true>, dim3((unsigned)n_tiles), dim3(TB), 0, ctx->stream, d_coef, (const uint8_t*)w.tables, zz, g, n_tiles,
                               w.bits, w.tile_bits, (unsigned long long*)w.head);
        else
            hipLaunchKernelGGL(enc_size_kernel<false>, dim3((unsigned)n_tiles), dim3(TB), 0, ctx->stream, d_coef, w.consts, zz, g, n_tiles, w.bits,
                               w.tile_bits, (unsigned long long*)w.head);
        CK_HIP(ctx, hipGetLastError());
    }
    TimeScope ts(ctx, "jpeg_enc_scan");
    hipLaunchKernelGGL(enc_scan_seg_kernel, dim3((unsigned)((n_segs + 3) / 4)), dim3(256), 0, ctx->stream, w.tile_bits, n_segs,
                       (long long)g.seg_tiles, w.tile_off, w.seg_bits);
    CK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(enc_scan_frame_kernel, dim3((unsigned)m), dim3(256), 0, ctx->stream, w.seg_bits, (long long)g.nseg, w.seg_u0);
    CK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(enc_scan_aligned_kernel, dim3(1), dim3(256), 0, ctx->stream, w.seg_u0 + g.nseg, (long long)(g.nseg + 1), (long long)m,
                       (uint64_t)TY, w.frame_u0, w.head + 1);
    CK_HIP(ctx, hipGetLastError());
    return CK_OK;
}

int k_jpeg_enc_put(ck_ctx* ctx, const int16_t* d_coef, int m, const CkEncGeom& g, const CkEncWork& w, uint32_t* d_buf, uint64_t total_u,
                   uint32_t* d_ff_cnt, uint32_t* d_ff_off, uint32_t hl)
{
    const long long n_tiles = (long long)m * g.nseg * g.seg_tiles;
    if (m <= 0 || !total_u || total_u % TY || total_u / TY > 0x7fffffffULL) return ck_fail(ctx, CK_ERR_ARG, "k_jpeg_enc_put: a bit buffer of %llu bytes", (unsigned long long)total_u);
    CK_HIP(ctx, hipMemsetAsync(d_buf, 0, total_u, ctx->stream));
    {
        TimeScope ts(ctx, "jpeg_enc_put");
        const uint8_t* zz = w.consts + sizeof(CkEncTables);
        if (w.freq)
            hipLaunchKernelGGL(enc_put_kernel<true>, dim3((unsigned)n_tiles), dim3(TB), 0, ctx->stream, d_coef, (const uint8_t*)w.tables, zz, g, n_tiles, w.bits, w.tile_bits, w.tile_off, w.seg_bits, w.seg_u0,
                               w.frame_u0, d_buf, (unsigned long long)(total_u / 4));
        else
            hipLaunchKernelGGL(enc_put_kernel<false>, dim3((unsigned)n_tiles), dim3(TB), 0, ctx->stream, d_coef, w.consts, zz, g,
                               n_tiles, w.bits, w.tile_bits, w.tile_off, w.seg_bits, w.seg_u0, w.frame_u0, d_buf, (unsigned long long)(total_u / 4));
        CK_HIP(ctx, hipGetLastError());
    }
    TimeScope ts(ctx, "jpeg_enc_stuff");
    hipLaunchKernelGGL(enc_ff_count_kernel, dim3((unsigned)(total_u / TY)), dim3(256), 0, ctx->stream, d_buf, d_ff_cnt);
    CK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(enc_scan_ff_kernel, dim3((unsigned)m), dim3(256), 0, ctx->stream, d_ff_cnt, w.frame_u0, w.seg_u0, (long long)g.nseg,
                       (uint64_t)hl, w.freq ? (const uint32_t*)w.hlen : (const uint32_t*)nullptr, d_ff_off, w.len);
    CK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(enc_scan_aligned_kernel, dim3(1), dim3(256), 0, ctx->stream, w.len, 1LL, (long long)m, (uint64_t)16, w.out_off,
                       (uint64_t*)nullptr);
    CK_HIP(ctx, hipGetLastError());
    return CK_OK;
}

int k_jpeg_enc_stuff(ck_ctx* ctx, int m, const CkEncGeom& g, const CkEncWork& w, const uint32_t* d_buf, uint64_t total_u,
                     const uint32_t* d_ff_off, uint32_t hl, uint8_t* d_pack, uint64_t pack_bytes)
{
    TimeScope ts(ctx, "jpeg_enc_stuff");
    hipLaunchKernelGGL(enc_stuff_kernel, dim3((unsigned)(total_u / TY)), dim3(256), 0, ctx->stream, d_buf, d_ff_off, w.frame_u0, w.seg_u0,
                       w.out_off, (long long)m, (long long)g.nseg, w.freq ? (const uint8_t*)w.headers : w.consts + sizeof(CkEncTables) + 64, hl,
                       w.freq ? (const uint32_t*)w.hlen : (const uint32_t*)nullptr, d_pack, (unsigned long long)pack_bytes);
    CK_HIP(ctx, hipGetLastError());
    return CK_OK;
}
