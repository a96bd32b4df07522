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
//
// With OPTIMISED tables (libjpeg's optimize_coding) two steps come first, and the code tables and the header belong to a frame:
//   histo  every block alone: the symbols ck_enc_block_walk names, counted into the frame's four tables of 256 counters --
//          DC luma, AC luma, DC chroma, AC chroma, the order of the DHT segments.
//   tables a table alone: libjpeg's jpeg_gen_optimal_table over its counters (ck_enc_optimal_table) -> the 16 counts and the
//          values of a DHT segment, the CkEncHuff derived from them (ck_enc_fill), the segment's bytes (ck_enc_dht); then
//          the frame's header: what stands in front of the DHT segments, the segments, what stands behind (ck_enc_header_byte).
// A DC code can be 16 bits long then, so a block has up to CK_ENC_OPT_BLOCK_BITS bits and a tile CK_ENC_OPT_TILE_WORDS words.
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
// optimised tables: any code can have 16 bits
constexpr int CK_ENC_OPT_BLOCK_BITS = 27 + 63 * 26;          // DC: 16 + 11, AC: 16 + 10
constexpr int CK_ENC_OPT_TILE_WORDS = (CK_ENC_TILE_BLOCKS * CK_ENC_OPT_BLOCK_BITS + 7 + 31 + 31) / 32;
constexpr int64_t CK_ENC_OPT_MAX_BLOCKS = (int64_t)1 << 25;  // of a frame: 64 symbols a block, so a counter stays below 2^32
constexpr int CK_ENC_DHT_SLOT = 288;                         // room for a DHT segment of one table: 21 + 256 bytes, rounded up
constexpr int CK_ENC_HEADER_SLOT = 1024;                     // room for a frame's header (CK_JPEG_ENC_HEADER_BOUND)

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

// the symbols of a block in the host coder's order, with its refusals: v.sym(ac, symbol, size, value) for the DC difference
// (ac 0: the symbol is its size) and for every AC symbol (ZRL and EOB have size 0); 0 or a status word
template <class Visit>
CK_HD inline uint32_t ck_enc_block_walk(const int16_t* blk, int pred, const uint8_t* zigzag, Visit& v)
{
    const int diff = (int)blk[0] - pred;
    int s = ck_enc_bit_size(diff);
    if (s > 11) return ck_enc_status(CK_ENC_DC, s);
    v.sym(0, s, s, diff);
    int run = 0;
    for (int k = 1; k < 64; k++) {
        const int val = blk[zigzag[k]];
        if (val == 0) { run++; continue; }
        for (; run > 15; run -= 16) v.sym(1, 0xF0, 0, 0);
        s = ck_enc_bit_size(val);
        if (s > 10) return ck_enc_status(CK_ENC_AC, s);
        v.sym(1, (run << 4) | s, s, val);
        run = 0;
    }
    if (run) v.sym(1, 0, 0, 0);
    return 0;
}

// the codes of a block as (value, length) pairs of at most 27 bits -- a code and the value bits behind it in one -- in the
// host coder's order, with its refusals; 0 or a status word
template <class Sink>
struct CkEncCoder {
    const CkEncHuff& dc;
    const CkEncHuff& ac;
    Sink& sink;
    CK_HD inline void sym(int is_ac, int symbol, int s, int val)
    {
        const CkEncHuff& t = is_ac ? ac : dc;
        sink.put(((uint32_t)t.code[symbol] << s) | ((uint32_t)(val < 0 ? val - 1 : val) & ((1u << s) - 1)), t.len[symbol] + s);
    }
};
template <class Sink>
CK_HD inline uint32_t ck_enc_block_put(const int16_t* blk, int pred, int is_chroma, const CkEncTables* T, const uint8_t* zigzag, Sink& sink)
{
    CkEncCoder<Sink> coder{T->dc[is_chroma], T->ac[is_chroma], sink};
    return ck_enc_block_walk(blk, pred, zigzag, coder);
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

// ---- optimised tables: histo and tables ----
// table t of a frame's four: t = 2 * chroma + ac, the order of the DHT segments (DC0, AC0, DC1, AC1)
CK_HD inline int ck_enc_table_index(int is_chroma, int is_ac) { return 2 * is_chroma + is_ac; }

// histo on the host: the symbols of a block into the frame's counters (4 x 256); Add()(counter) is `++` here and an atomic
// in LDS on the device
struct CkEncPlainInc {
    CK_HD inline void operator()(uint32_t* c) const { ++*c; }
};
template <class Add>
struct CkEncHisto {
    uint32_t* dc;                                            // the 256 counters of the block's DC table
    uint32_t* ac;                                            // and of its AC table
    CK_HD inline void sym(int is_ac, int symbol, int, int) { Add()((is_ac ? ac : dc) + symbol); }
};
template <class Add>
CK_HD inline uint32_t ck_enc_block_histo(const int16_t* blk, int pred, int is_chroma, uint32_t* freq, const uint8_t* zigzag)
{
    CkEncHisto<Add> h{freq + 256 * ck_enc_table_index(is_chroma, 0), freq + 256 * ck_enc_table_index(is_chroma, 1)};
    return ck_enc_block_walk(blk, pred, zigzag, h);
}

// jpeg_gen_optimal_table.  Sums in 64 bits; the caller puts the counters into freq[0 .. 255].  Who runs it is X: on the host
// one thread (CkEncSerial); on the device a wave, whose lanes find the least entry together (x.least), lane 0 doing the
// rest (x.one) with a barrier between the two (x.sync).  Every loop has a bound the counters cannot move.
constexpr int CK_ENC_MAX_CLEN = 256;                         // 257 leaves: no code is longer before the lengths are limited
struct CkEncTreeWork {
    uint64_t freq[257];
    int32_t codesize[257], others[257];                      // others: the merges (c1 | c2 << 16), then the sort's offsets
    uint32_t nbits[CK_ENC_MAX_CLEN + 2];
};
struct CkEncSerial {
    // the entry with the least non-zero freq other than `skip`, the largest index among equals; -1: none
    CK_HD inline int least(const uint64_t* freq, int skip) const
    {
        uint64_t v = ~(uint64_t)0;
        int c = -1;
        for (int i = 0; i <= 256; i++)
            if (i != skip && freq[i] && freq[i] <= v) { v = freq[i]; c = i; }
        return c;
    }
    CK_HD inline bool one() const { return true; }
    CK_HD inline void sync() const {}
};
// -> bits[16] (codes of length 1 .. 16), vals[256] (the first *count are used), as a DHT segment lists them
template <class X>
CK_HD inline void ck_enc_optimal_table(CkEncTreeWork* w, uint8_t* bits, uint8_t* vals, int32_t* count, const X& x)
{
    if (x.one()) {
        w->freq[256] = 1;                                    // the pseudo-symbol: no real symbol gets the code of all ones
        for (int i = 0; i <= 256; i++) { w->codesize[i] = 0; w->others[i] = 0; }
        for (int i = 0; i < CK_ENC_MAX_CLEN + 2; i++) w->nbits[i] = 0;
    }
    x.sync();
    int merges = 0;
    for (; merges < 256; merges++) {
        const int c1 = x.least(w->freq, -1);
        const int c2 = c1 < 0 ? -1 : x.least(w->freq, c1);
        if (c2 < 0) break;
        x.sync();
        if (x.one()) {
            w->freq[c1] += w->freq[c2];
            w->freq[c2] = 0;
            w->others[merges] = c1 | (c2 << 16);
        }
        x.sync();
    }
    if (x.one()) {
        // libjpeg adds 1 to the code size of every leaf of both trees at each merge, walking two chains of leaves.  The
        // same sizes without the chains: from the last merge back, the tree that was absorbed (c2) gets what the absorbing
        // one (c1, which stands for the merged tree from then on) collected later, and both get this merge.
        for (int k = merges - 1; k >= 0; k--) {
            const int c1 = w->others[k] & 0xffff, c2 = w->others[k] >> 16;
            w->codesize[c2] = w->codesize[c1] + 1;
            w->codesize[c1] += 1;
        }
        int top = 0;
        for (int i = 0; i <= 256; i++) {
            const int l = w->codesize[i] > CK_ENC_MAX_CLEN ? CK_ENC_MAX_CLEN : w->codesize[i];
            if (l) { w->nbits[l]++; if (l > top) top = l; }
        }
        // no code above 16 bits: a pair of the longest codes goes one up beside a shorter code that goes one down.
        // (libjpeg starts at 32 and gives up on a longer code; from `top` on the rule is the same where it has one)
        int guard = 257 * CK_ENC_MAX_CLEN;
        for (int i = top; i > 16; i--)
            while (w->nbits[i] > 1 && guard-- > 0) {
                int j = i - 2;
                while (j > 0 && w->nbits[j] == 0) j--;
                if (j == 0) { guard = 0; break; }
                w->nbits[i] -= 2;
                w->nbits[i - 1]++;
                w->nbits[j + 1] += 2;
                w->nbits[j]--;
            }
        int i = 16;
        while (i > 0 && w->nbits[i] == 0) i--;
        if (i) w->nbits[i]--;                                // the pseudo-symbol leaves
        for (int l = 1; l <= 16; l++) bits[l - 1] = (uint8_t)w->nbits[l];
        // the values by code length, by value inside a length: a counting sort over the lengths before they were limited
        int32_t* start = w->others;
        for (int l = 0; l <= CK_ENC_MAX_CLEN; l++) start[l] = 0;
        for (int s = 0; s < 256; s++) {
            const int l = w->codesize[s] > CK_ENC_MAX_CLEN ? CK_ENC_MAX_CLEN : w->codesize[s];
            if (l) start[l]++;
        }
        int32_t at = 0;
        for (int l = 1; l <= top; l++) { const int32_t c = start[l]; start[l] = at; at += c; }
        for (int s = 0; s < 256; s++) {
            const int l = w->codesize[s] > CK_ENC_MAX_CLEN ? CK_ENC_MAX_CLEN : w->codesize[s];
            if (l) vals[start[l]++] = (uint8_t)s;
        }
        *count = at;
    }
    x.sync();
}

// bits[16] and vals of a DHT segment -> symbol to code and length
CK_HD inline void ck_enc_fill(CkEncHuff* t, const uint8_t* bits, const uint8_t* vals)
{
    for (int i = 0; i < 256; i++) { t->code[i] = 0; t->len[i] = 0; }
    int c = 0, k = 0;
    for (int l = 1; l <= 16; l++) {
        for (int i = 0; i < bits[l - 1] && k < 256; i++, c++, k++) { t->code[vals[k]] = (uint16_t)c; t->len[vals[k]] = (uint8_t)l; }
        c <<= 1;
    }
}
// the DHT segment of table t (count values) -> out (CK_ENC_DHT_SLOT bytes of room); its length
CK_HD inline uint32_t ck_enc_dht(uint8_t* out, int t, const uint8_t* bits, const uint8_t* vals, int count)
{
    const int n = count < 0 ? 0 : (count > 256 ? 256 : count);
    out[0] = 0xFF; out[1] = 0xC4;
    out[2] = (uint8_t)((19 + n) >> 8); out[3] = (uint8_t)((19 + n) & 255);
    out[4] = (uint8_t)(((t & 1) << 4) | (t >> 1));           // Tc << 4 | Th
    for (int i = 0; i < 16; i++) out[5 + i] = bits[i];
    for (int i = 0; i < n; i++) out[21 + i] = vals[i];
    return (uint32_t)(21 + n);
}
// byte i of a frame's header: `pre` (SOI .. SOF0), the ntab DHT segments (slots of CK_ENC_DHT_SLOT bytes), `post` (DRI, SOS)
CK_HD inline uint32_t ck_enc_header_len(uint32_t pre_len, const uint32_t* dht_len, int ntab, uint32_t post_len)
{
    uint32_t n = pre_len + post_len;
    for (int t = 0; t < ntab; t++) n += dht_len[t];
    return n;
}
CK_HD inline uint8_t ck_enc_header_byte(uint32_t i, const uint8_t* pre, uint32_t pre_len, const uint8_t* dht, const uint32_t* dht_len, int ntab,
                                        const uint8_t* post)
{
    if (i < pre_len) return pre[i];
    i -= pre_len;
    for (int t = 0; t < ntab; t++) {
        if (i < dht_len[t]) return dht[(size_t)t * CK_ENC_DHT_SLOT + i];
        i -= dht_len[t];
    }
    return post[i];
}
