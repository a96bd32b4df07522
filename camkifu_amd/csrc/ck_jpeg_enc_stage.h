// ck_jpeg_enc_stage.h -- the Huffman stage of the JPEG encoder cut into steps that do not depend on one another, written once:
// plain C++ for the host (ck_jpeg_enc.cpp, tools/sanitize/jpeg_enc_stage_fuzz.cpp) and device code for k_jpeg_enc_huff.hip.
// No HIP call in here; host and device differ in the sink that receives the codes and in who runs the loops.
//
// Terms.  A SEGMENT is one restart interval of one frame: MCUs [k * ri, min((k + 1) * ri, total)), the whole scan when ri
// is 0.  SCAN ORDER is the order ck_jpeg_enc_entropy walks: MCU by MCU, inside an MCU Y (vs rows of hs blocks), Cb, Cr.
// Block b of a frame is its index in that order; its PLACE is its index in the component-planar coefficient layout.
//
// The steps:
//   size   every block alone: the bits of its code (ck_enc_block_bits).  The DC predictor is the DC value of the block
//          ck_enc_pred_block names, a closed form, so no block waits for another.
//   scan   a block TILE is CK_ENC_TILE_BLOCKS consecutive blocks of one segment (a segment has seg_tiles of them, the last
//          ones of a frame's last segment may be empty).  Bits of a tile -> offsets of the tiles in their segment ->
//          B bits, U = ceil(B / 8) bytes and 8U - B pad bits (ones) per segment -> byte offsets of the segments in their
//          frame -> frames one after another in one bit buffer, each starting on CK_ENC_TILE_BYTES.
//   put    a tile assembles its bits in CK_ENC_TILE_WORDS words of its own (big-endian dwords, the first one starting at
//          the bit where the tile starts in the buffer) and writes them out byte-swapped: the first and the last dword, which
//          the neighbours share, by OR into the zeroed buffer, the others by plain stores (ck_enc_flush_how).
//   stuff  a byte TILE is CK_ENC_TILE_BYTES unstuffed bytes.  FF bytes of a tile -> FF bytes before a tile in its frame ->
//          byte i of a frame goes to header + i + (FF before i) + 2 * (segments before i) with 00 behind an FF, the marker
//          FF D0+(k & 7) behind the last byte of segment k, FF D9 behind the last of all (ck_enc_emit).
// The padded last byte of a segment is stuffed like any other when it comes out FF, as the host coder's pad() does.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef CK_HD
#ifdef __HIPCC__
#define CK_HD __host__ __device__
#else
#define CK_HD
#endif
#endif

constexpr int CK_ENC_TILE_BLOCKS = 64;                       // one wave: a lane per block
constexpr int CK_ENC_TILE_BYTES = 1024;                      // 256 lanes, a dword each
constexpr int CK_ENC_BLOCK_BITS = 20 + 63 * 26;              // DC: 9 + 11, AC: 16 + 10
// the bits of a full tile, 7 pad bits, up to 31 bits in front of it in its first dword
constexpr int CK_ENC_TILE_WORDS = (CK_ENC_TILE_BLOCKS * CK_ENC_BLOCK_BITS + 7 + 31 + 31) / 32;

// symbol -> code and length (0: the table has no such symbol)
struct CkEncHuff {
    uint16_t code[256];
    uint8_t len[256];
};
struct CkEncTables {
    CkEncHuff dc[2], ac[2];                                  // [0] luma, [1] chroma
};
static_assert(sizeof(CkEncTables) == 4 * 768, "four tables of 768 bytes");

struct CkEncGeom {
    int32_t hs, vs, mcux, mcuy, lw;                          // luma blocks per MCU across / down, MCUs, luma blocks across
    int32_t luma_blocks, mcu_blocks;                         // per MCU
    int64_t mcus, blocks, base_cb, base_cr;                  // of a frame; places of the first Cb / Cr block
    int64_t seg_mcus, nseg, seg_tiles;                       // MCUs of a segment, segments of a frame, block tiles of a segment
};

// h, w in 1 .. 65535, sampling 0 (grey) .. 3 (4:2:0), ri in 0 .. 65535: the callers check
CK_HD inline CkEncGeom ck_enc_geom(int h, int w, int sampling, int ri)
{
    CkEncGeom g;
    g.hs = sampling >= 2 ? 2 : 1;
    g.vs = sampling == 3 ? 2 : 1;
    g.mcux = (w + 8 * g.hs - 1) / (8 * g.hs);
    g.mcuy = (h + 8 * g.vs - 1) / (8 * g.vs);
    g.lw = g.mcux * g.hs;
    g.luma_blocks = g.hs * g.vs;
    g.mcu_blocks = g.luma_blocks + (sampling == 0 ? 0 : 2);
    g.mcus = (int64_t)g.mcux * g.mcuy;
    g.blocks = g.mcus * g.mcu_blocks;
    g.base_cb = g.mcus * g.luma_blocks;
    g.base_cr = g.base_cb + g.mcus;
    g.seg_mcus = ri > 0 && ri < g.mcus ? ri : g.mcus;
    g.nseg = (g.mcus + g.seg_mcus - 1) / g.seg_mcus;
    g.seg_tiles = (g.seg_mcus * g.mcu_blocks + CK_ENC_TILE_BLOCKS - 1) / CK_ENC_TILE_BLOCKS;
    return g;
}

// scan order -> place in the coefficient layout
CK_HD inline int64_t ck_enc_place(const CkEncGeom& g, int64_t b)
{
    const int64_t mcu = b / g.mcu_blocks;
    const int j = (int)(b % g.mcu_blocks);
    if (j >= g.luma_blocks) return (j == g.luma_blocks ? g.base_cb : g.base_cr) + mcu;
    const int64_t my = mcu / g.mcux, mx = mcu % g.mcux;
    return (my * g.vs + j / g.hs) * g.lw + mx * g.hs + j % g.hs;
}
// and back
CK_HD inline int64_t ck_enc_block_of(const CkEncGeom& g, int64_t place)
{
    if (place >= g.base_cr) return (place - g.base_cr) * g.mcu_blocks + g.luma_blocks + 1;
    if (place >= g.base_cb) return (place - g.base_cb) * g.mcu_blocks + g.luma_blocks;
    const int64_t row = place / g.lw, col = place % g.lw;
    return ((row / g.vs) * g.mcux + col / g.hs) * g.mcu_blocks + (row % g.vs) * g.hs + col % g.hs;
}
CK_HD inline int ck_enc_is_chroma(const CkEncGeom& g, int64_t b) { return (int)(b % g.mcu_blocks) >= g.luma_blocks; }
// the block whose DC value is b's predictor: the previous block of the same component inside the segment, -1 for none
CK_HD inline int64_t ck_enc_pred_block(const CkEncGeom& g, int64_t b)
{
    const int64_t mcu = b / g.mcu_blocks;
    const int j = (int)(b % g.mcu_blocks);
    const bool first = mcu % g.seg_mcus == 0;
    if (j >= g.luma_blocks) return first ? -1 : b - g.mcu_blocks;
    if (j > 0) return b - 1;
    return first ? -1 : b - (g.mcu_blocks - g.luma_blocks) - 1;
}
// tile t of segment k: its first block and how many it has (0 .. CK_ENC_TILE_BLOCKS)
CK_HD inline void ck_enc_tile_blocks(const CkEncGeom& g, int64_t k, int64_t t, int64_t* b0, int* count)
{
    const int64_t m1 = (k + 1) * g.seg_mcus < g.mcus ? (k + 1) * g.seg_mcus : g.mcus;
    const int64_t first = k * g.seg_mcus * g.mcu_blocks + t * CK_ENC_TILE_BLOCKS, end = m1 * g.mcu_blocks;
    *b0 = first;
    *count = end <= first ? 0 : (end - first < CK_ENC_TILE_BLOCKS ? (int)(end - first) : CK_ENC_TILE_BLOCKS);
}

// ---- one block ----
// what the size step says of a block: its bits, or CK_ENC_FAIL | kind << 8 | the bit count the tables have no code for
enum { CK_ENC_DC = 1, CK_ENC_AC = 2 };
constexpr uint32_t CK_ENC_FAIL = 0x80000000u;
CK_HD inline uint32_t ck_enc_status(int kind, int size) { return CK_ENC_FAIL | ((uint32_t)kind << 8) | (uint32_t)size; }

CK_HD inline int ck_enc_bit_size(int v)
{
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}

// the codes of a block as (value, length) pairs of at most 27 bits -- a code and the value bits behind it in one -- in the
// host coder's order, with its refusals; 0 or a status word
template <class Sink>
CK_HD inline uint32_t ck_enc_block_put(const int16_t* blk, int pred, int is_chroma, const CkEncTables* T, const uint8_t* zigzag, Sink& sink)
{
    const CkEncHuff& dc = T->dc[is_chroma];
    const CkEncHuff& ac = T->ac[is_chroma];
    const int diff = (int)blk[0] - pred;
    int s = ck_enc_bit_size(diff);
    if (s > 11) return ck_enc_status(CK_ENC_DC, s);
    sink.put(((uint32_t)dc.code[s] << s) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1)), dc.len[s] + s);
    int run = 0;
    for (int k = 1; k < 64; k++) {
        const int val = blk[zigzag[k]];
        if (val == 0) { run++; continue; }
        for (; run > 15; run -= 16) sink.put(ac.code[0xF0], ac.len[0xF0]);
        s = ck_enc_bit_size(val);
        if (s > 10) return ck_enc_status(CK_ENC_AC, s);
        const int sym = (run << 4) | s;
        sink.put(((uint32_t)ac.code[sym] << s) | ((uint32_t)(val < 0 ? val - 1 : val) & ((1u << s) - 1)), ac.len[sym] + s);
        run = 0;
    }
    if (run) sink.put(ac.code[0], ac.len[0]);
    return 0;
}

struct CkEncCount {
    uint32_t bits = 0;
    CK_HD inline void put(uint32_t, int len) { bits += (uint32_t)len; }
};
CK_HD inline uint32_t ck_enc_block_bits(const int16_t* blk, int pred, int is_chroma, const CkEncTables* T, const uint8_t* zigzag)
{
    CkEncCount c;
    const uint32_t st = ck_enc_block_put(blk, pred, is_chroma, T, zigzag, c);
    return st ? st : c.bits;
}

// bits into big-endian dwords at bit `pos` of `words`; Or()(word, bits) is `|=` on the host and an atomic in LDS
struct CkEncPlainOr {
    CK_HD inline void operator()(uint32_t* w, uint32_t x) const { *w |= x; }
};
template <class Or>
struct CkEncWordSink {
    uint32_t* words;
    uint32_t pos;
    CK_HD inline void put(uint32_t v, int len)               // 1 <= len <= 32, v below 2^len
    {
        const uint64_t x = (uint64_t)v << (64 - (int)(pos & 31) - len);
        Or()(words + (pos >> 5), (uint32_t)(x >> 32));
        if ((uint32_t)x) Or()(words + (pos >> 5) + 1, (uint32_t)x);
        pos += (uint32_t)len;
    }
};

// ---- segments, tiles, bytes ----
CK_HD inline uint64_t ck_enc_seg_bytes(uint64_t bits) { return (bits + 7) >> 3; }
CK_HD inline int ck_enc_seg_pad(uint64_t bits) { return (int)(8 * ck_enc_seg_bytes(bits) - bits); }
CK_HD inline uint64_t ck_enc_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }
CK_HD inline uint32_t ck_enc_bswap(uint32_t v) { return __builtin_bswap32(v); }

// word i of the n a tile assembled -> the bit buffer; how: 0 plain store, 1 OR (the dwords the neighbours share)
CK_HD inline int ck_enc_flush_how(int i, int n) { return i == 0 || i == n - 1; }

// segment of byte i of a frame: the largest k with seg_u0[k] <= i (seg_u0: nseg + 1 offsets, the last one the frame's bytes)
CK_HD inline int64_t ck_enc_seg_of(const uint64_t* seg_u0, int64_t nseg, uint64_t i)
{
    int64_t lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (seg_u0[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// unstuffed byte i of a frame, value c, with `ff` FF bytes before it in the frame -> the stream behind its header at dst;
// nothing is written at or beyond `end` (offsets that are right never get there)
CK_HD inline void ck_enc_emit(uint8_t* dst, const uint8_t* end, const uint64_t* seg_u0, int64_t nseg, uint64_t i, unsigned c, uint64_t ff)
{
    const int64_t k = nseg > 1 ? ck_enc_seg_of(seg_u0, nseg, i) : 0;
    const bool last = i + 1 == seg_u0[k + 1];
    uint8_t* p = dst + i + ff + 2 * (uint64_t)k;
    if (p + 1 + (c == 0xFF) + 2 * last > end) return;
    *p++ = (uint8_t)c;
    if (c == 0xFF) *p++ = 0;
    if (last) {
        *p++ = 0xFF;
        *p++ = (uint8_t)(k + 1 < nseg ? 0xD0 + (k & 7) : 0xD9);
    }
}
// the length of a frame's stream
CK_HD inline uint64_t ck_enc_stream_len(uint64_t header, uint64_t bytes, uint64_t ff, int64_t nseg) { return header + bytes + ff + 2 * (uint64_t)nseg; }
