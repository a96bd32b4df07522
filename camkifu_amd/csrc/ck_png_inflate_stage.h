// ck_png_inflate_stage.h -- an inflate cut into pieces that a GPU lane and a host loop run as the same text: plain C++ for
// the host (ck_png.cpp: ck_png_unzip_staged, tools/sanitize/png_inflate_fuzz.cpp) and device code for k_png_inflate.hip.
// No HIP call in here.  The yardstick for every verdict is ck_png_unzip / ck_png_rows (ck_png.cpp), which stay as they are.
//
// Terms.  A TOKEN is what one literal/length code stands for: a literal byte, a length / distance pair with both extra
// fields (at most 15 + 5 + 15 + 13 = 48 bits), or end-of-block.  A WINDOW is CK_INF_WINDOW consecutive bit offsets
// p .. p + W - 1 of a block's data; a STEP decodes, for every offset of the window, the token that would start there
// (ck_inf_token: most of them garbage, at offsets where no token starts), then walks the chain from offset 0
// (next = offset + bits consumed) to pick the real ones and sum their output lengths (ck_inf_walk), then applies them.
//
// The pieces:
//   tables  code lengths -> a primary table of PB bits and second-level tables behind it (ck_inf_build): a look-up costs
//           the same for every code length (ck_inf_look), because a lane at a wrong offset meets long codes often and a
//           step lasts as long as its slowest lane.  The verdicts are huff_build's.
//   block   the three header bits, a stored block's lengths, a dynamic block's HLIT / HDIST / HCLEN, code-length code
//           and lengths with the repeats 16 / 17 / 18 (ck_inf_block): serial, once per block, every refusal of
//           ck_png_unzip in its order.
//   token   ck_inf_token.  Bits past the end of the data read as zeros; a token that needs them is refused.
//   walk    ck_inf_walk: the chain through the window.  It carries the running sum of the output lengths, which is the
//           exclusive prefix sum that places every token, and stops in front of the first token that carries a cause or
//           whose distance reaches before byte 0, behind an end-of-block, or in front of a token with which the step would
//           write more than CK_INF_STEP_BYTES.  The first token of a window is always taken (it writes at most 258 bytes),
//           so every step advances or ends the stream.  A token may begin inside the window and end outside it.
//   apply   into a ring of the last CK_INF_RING bytes (position mod 32768).  The order in which a step's bytes reach the
//           ring: (1) all literals of the step at once, (2) the matches one after the other in chain order, the bytes of one
//           match at once, byte i from source byte i mod d (a match of distance d shorter than its length repeats with
//           period d; every source byte lies before the match).  Why no byte is lost: the step writes the ring slots of
//           positions [n, n + S), which held [n - 32768, n + S - 32768).  A match at position q reads positions >= q - d;
//           if for every match of the step q - d >= n + S - 32768, none reads a slot the step overwrites, so (1) destroys
//           nothing, and in (2) a match finds old bytes, literals of (1) and earlier matches in place.  If one match reaches
//           further back (ck_inf_walk reports it: `far`), (1) is skipped and literals and matches are applied one after the
//           other in chain order: a token at q then overwrites only [q - 32768, ..), and nothing at or behind q reads
//           before q - 32768.  Inside one match the slot of byte i is read (source q + i - d) before any lane writes: all
//           reads of a pass of 64 bytes come before its writes, and later passes read slots ahead of those written.
//   flush   whenever CK_INF_FLUSH bytes are pending, that half of the ring goes out: the Adler-32 over it
//           (ck_inf_adler_chunk), the positions below `cap` to the output, the filter bytes of the rows that start in it
//           looked at (ck_inf_row_check).  S <= CK_INF_STEP_BYTES = CK_INF_FLUSH keeps pending bytes below the ring's size.
//   adler   per tile of CK_PNG_TILE_BYTES the pair (a, b) of the encoder's size step; tiles are joined by ck_png_scan_band,
//           the rule ck_png_stage.h has -- the running pair goes in as tile 0, whose length the rule never uses.
//   verdict CkInfRecord {cause, arg0, arg1, produced}; ck_png_inflate_message (ck_png.cpp) turns it into ck_png_unzip's text.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "ck_png_stage.h"

#ifndef CK_PNG_INFLATE_OPL
#define CK_PNG_INFLATE_OPL 1                                 // bit offsets a lane decodes per step (docs/lab_notes.md has the others)
#endif
constexpr int CK_INF_OPL = CK_PNG_INFLATE_OPL;
constexpr int CK_INF_WINDOW = 64 * CK_INF_OPL;
constexpr int CK_INF_RING = 32768;
constexpr int CK_INF_FLUSH = CK_INF_RING / 2;
constexpr int CK_INF_STEP_BYTES = CK_INF_FLUSH;              // (below 64 * 258)
constexpr int CK_INF_FLUSH_TILES = CK_INF_FLUSH / CK_PNG_TILE_BYTES;
static_assert(CK_INF_OPL == 1 || CK_INF_OPL == 2 || CK_INF_OPL == 4, "1, 2 or 4 offsets a lane");
static_assert(CK_INF_STEP_BYTES + CK_INF_FLUSH <= CK_INF_RING && CK_INF_STEP_BYTES <= 64 * 258, "pending bytes fit the ring");
// Table sizes.  A second-level table of 2^k entries holds a complete code tree of depth k, which has at least k + 1 leaves.
// Literal/length, PB 10: at most 286 long codes, k <= 5 -> at most 47 tables of 32 and one of 8 (1512 entries).  Distance,
// PB 8: 30 codes, k <= 7 -> three of 128 and one of 32 (416).  ck_inf_build checks the room all the same.
constexpr int CK_INF_LIT_BITS = 10, CK_INF_LIT_CAP = 1024 + 1536;
constexpr int CK_INF_DIST_BITS = 8, CK_INF_DIST_CAP = 256 + 448;
constexpr int CK_INF_CL_BITS = 7, CK_INF_CL_CAP = 128;

enum { CK_INF_KIND_CODES = 0, CK_INF_KIND_LENS = 1, CK_INF_KIND_DISTS = 2 };
enum { CK_INF_BUILD_OK = 0, CK_INF_BUILD_NONE = 1, CK_INF_BUILD_OVER = 2, CK_INF_BUILD_INCOMPLETE = 3, CK_INF_BUILD_ROOM = 4 };

// every cause of refusal, in the order ck_png_unzip and ck_png_rows meet them
enum {
    CK_INF_OK = 0,
    CK_INF_ZLIB_SHORT,                                       // arg0: the bytes
    CK_INF_ZLIB_CHECK, CK_INF_ZLIB_METHOD, CK_INF_ZLIB_WINDOW, CK_INF_ZLIB_DICT,      // arg0: the method, the window code
    CK_INF_BLOCK_ENDS, CK_INF_BLOCK_TYPE3,
    CK_INF_STORED_LENS_END, CK_INF_STORED_LENS,              // arg0, arg1: LEN, NLEN
    CK_INF_STORED_ENDS,
    CK_INF_DYN_ENDS, CK_INF_DYN_COUNTS,                      // arg0, arg1: literal/length codes, distance codes
    CK_INF_CL_ENDS, CK_INF_CL_NONE, CK_INF_CL_OVER, CK_INF_CL_INCOMPLETE, CK_INF_CL_ROOM,
    CK_INF_CLSYM, CK_INF_REPEAT_FIRST, CK_INF_REPEAT_ENDS, CK_INF_REPEAT_PAST, CK_INF_NO_EOB,
    CK_INF_LIT_NONE, CK_INF_LIT_OVER, CK_INF_LIT_INCOMPLETE, CK_INF_LIT_ROOM,
    CK_INF_DIST_NONE, CK_INF_DIST_OVER, CK_INF_DIST_INCOMPLETE, CK_INF_DIST_ROOM,
    // inflate_codes's, one value each; with "(after %zu bytes)": produced
    CK_INF_TOK_LITLEN, CK_INF_TOK_LITLEN_SYMBOL, CK_INF_TOK_LENGTH_ENDS, CK_INF_TOK_DIST, CK_INF_TOK_DIST_SYMBOL, CK_INF_TOK_DIST_ENDS,
    CK_INF_TOK_FAR,
    CK_INF_ADLER_ENDS, CK_INF_ADLER,                         // arg0, arg1: the stream's, the data's
    // ck_png_rows's two
    CK_INF_ROWS_SHORT, CK_INF_ROW_FILTER,                    // arg0, arg1: the row, its filter type
    CK_INF_CAUSES
};

struct CkInfRecord {
    int32_t cause;
    uint32_t arg0, arg1, reserved;
    int64_t produced;                                        // bytes applied: all of them for CK_INF_OK, else those before the refused token
    int64_t steps, tokens;                                   // window steps; literals and matches applied
};
static_assert(sizeof(CkInfRecord) == 40, "a verdict record is 40 bytes");
// what k_png_inflate is told of a stream (ck_common.h): offsets into the staged block, in bytes
struct CkInfJob {
    int64_t z_off, zlen, out_off, cap, need, pitch;
};

struct CkInfIn {
    const uint8_t* z;
    uint64_t bytes;
};
CK_HD inline uint64_t ck_inf_bits(const CkInfIn& in) { return in.bytes * 8; }
// at least 57 bits of the stream from bit p on (p <= the stream's bits), zeros behind its end
CK_HD inline uint64_t ck_inf_peek(const CkInfIn& in, uint64_t p)
{
    const uint64_t at = p >> 3;
    uint64_t v = 0;
    if (at + 8 <= in.bytes) {
        memcpy(&v, in.z + at, 8);
    } else {
        for (int i = 0; i < 8 && at + (uint64_t)i < in.bytes; i++) v |= (uint64_t)in.z[at + (uint64_t)i] << (8 * i);
    }
    return v >> (p & 7);
}
// n <= 16 bits at *pos, which moves on; false where the stream has fewer
CK_HD inline bool ck_inf_take(const CkInfIn& in, uint64_t* pos, int n, uint32_t* v)
{
    if (ck_inf_bits(in) - *pos < (uint64_t)n) return false;
    *v = (uint32_t)ck_inf_peek(in, *pos) & ((1u << n) - 1);
    *pos += (uint64_t)n;
    return true;
}

// ---- tables ----
// An entry: 0 no code; symbol << 4 | length of the code; or, in the primary table, 0x8000 | where << 3 | k: the codes with
// these PB bits in front are longer, look at the next k bits in the table of 2^k entries at `where`.
CK_HD inline int ck_inf_build(uint16_t* t, int PB, int cap, const uint8_t* lens, int n, int kind)
{
    uint32_t count[16], next[16];
    for (int l = 0; l < 16; l++) count[l] = 0;
    for (int i = 0; i < n; i++) count[lens[i]]++;
    count[0] = 0;
    int max = 15;
    while (max > 0 && !count[max]) max--;
    const uint32_t P = 1u << PB;
    for (uint32_t x = 0; x < P; x++) t[x] = 0;                // (no code at all: every look-up finds none)
    if (max == 0) return kind == CK_INF_KIND_CODES ? CK_INF_BUILD_NONE : CK_INF_BUILD_OK;
    int left = 1;
    for (int l = 1; l <= 15; l++) {
        left = (left << 1) - (int)count[l];
        if (left < 0) return CK_INF_BUILD_OVER;
    }
    if (left > 0 && (kind == CK_INF_KIND_CODES || max != 1)) return CK_INF_BUILD_INCOMPLETE;
    for (int pass = max > PB ? 0 : 1; pass < 2; pass++) {
        uint32_t code = 0;
        for (int l = 1; l <= 15; l++) { next[l] = code; code = (code + count[l]) << 1; }
        for (int i = 0; i < n; i++) {
            const int l = lens[i];
            if (!l) continue;
            const uint32_t r = ck_png_reverse(next[l]++, l);
            if (pass == 0) {                                 // how deep the tree behind every primary entry goes
                if (l > PB && t[r & (P - 1)] < (uint32_t)(l - PB)) t[r & (P - 1)] = (uint16_t)(l - PB);
                continue;
            }
            const uint16_t e = (uint16_t)(i << 4 | l);
            if (l <= PB) {
                for (uint32_t x = r; x < P; x += 1u << l) t[x] = e;
            } else {
                const uint32_t link = t[r & (P - 1)], at = (link >> 3) & 0xfffu, k = link & 7u;
                for (uint32_t x = r >> PB; x < (1u << k); x += 1u << (l - PB)) t[at + x] = e;
            }
        }
        if (pass == 0) {                                     // room for the second-level tables, none of their codes yet
            uint32_t at = P;
            for (uint32_t x = 0; x < P; x++) {
                const uint32_t k = t[x];
                if (!k) continue;
                if (at + (1u << k) > (uint32_t)cap) return CK_INF_BUILD_ROOM;
                for (uint32_t y = 0; y < (1u << k); y++) t[at + y] = 0;
                t[x] = (uint16_t)(0x8000u | at << 3 | k);
                at += 1u << k;
            }
        }
    }
    return CK_INF_BUILD_OK;
}
CK_HD inline uint32_t ck_inf_look(const uint16_t* t, int PB, uint64_t bits)
{
    uint32_t e = t[(uint32_t)bits & ((1u << PB) - 1)];
    if (e & 0x8000u) e = t[((e >> 3) & 0xfffu) + ((uint32_t)(bits >> PB) & ((1u << (e & 7u)) - 1))];
    return e;
}
// the fixed code of RFC 1951, 3.2.6.  lens: room for 320
CK_HD inline void ck_inf_fixed(uint16_t* lit, uint16_t* dist, uint8_t* lens)
{
    for (int i = 0; i < 288; i++) lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    ck_inf_build(lit, CK_INF_LIT_BITS, CK_INF_LIT_CAP, lens, 288, CK_INF_KIND_LENS);
    for (int i = 0; i < 32; i++) lens[i] = 5;
    ck_inf_build(dist, CK_INF_DIST_BITS, CK_INF_DIST_CAP, lens, 32, CK_INF_KIND_DISTS);
}

// ---- block ----
struct CkInfBlock {
    int32_t cause;
    uint32_t arg0, arg1;
    int32_t last, type;
    uint32_t stored;                                         // bytes of a stored block
    uint64_t pos;                                            // where the block's data starts (a stored block's: a whole byte)
};
// the header of the block at bit `pos`; for type 1 and 2 the tables are built.  cl: CK_INF_CL_CAP entries, lens: 320 bytes
CK_HD inline void ck_inf_block(const CkInfIn& in, uint64_t pos, uint16_t* lit, uint16_t* dist, uint16_t* cl, uint8_t* lens, CkInfBlock* b)
{
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t last = 0, type = 0;
    b->cause = CK_INF_OK; b->arg0 = b->arg1 = 0; b->stored = 0;
    const bool have = ck_inf_take(in, &pos, 1, &last) && ck_inf_take(in, &pos, 2, &type);
    b->last = (int32_t)last; b->type = (int32_t)type; b->pos = pos;
    if (!have) { b->cause = CK_INF_BLOCK_ENDS; return; }
    if (type == 3) { b->cause = CK_INF_BLOCK_TYPE3; return; }
    if (type == 0) {
        uint32_t len, nlen;
        pos = (pos + 7) & ~(uint64_t)7;
        if (!ck_inf_take(in, &pos, 16, &len) || !ck_inf_take(in, &pos, 16, &nlen)) { b->cause = CK_INF_STORED_LENS_END; return; }
        if ((len ^ 0xffffu) != nlen) { b->cause = CK_INF_STORED_LENS; b->arg0 = len; b->arg1 = nlen; return; }
        if (in.bytes - (pos >> 3) < len) { b->cause = CK_INF_STORED_ENDS; return; }
        b->stored = len; b->pos = pos;
        return;
    }
    if (type == 1) { ck_inf_fixed(lit, dist, lens); return; }
    uint32_t nlen, ndist, ncode;
    if (!ck_inf_take(in, &pos, 5, &nlen) || !ck_inf_take(in, &pos, 5, &ndist) || !ck_inf_take(in, &pos, 4, &ncode)) { b->cause = CK_INF_DYN_ENDS; return; }
    nlen += 257; ndist += 1; ncode += 4;
    if (nlen > 286 || ndist > 30) { b->cause = CK_INF_DYN_COUNTS; b->arg0 = nlen; b->arg1 = ndist; return; }
    for (int i = 0; i < 320; i++) lens[i] = 0;
    for (uint32_t i = 0; i < ncode; i++) {
        uint32_t v;
        if (!ck_inf_take(in, &pos, 3, &v)) { b->cause = CK_INF_CL_ENDS; return; }
        lens[order[i]] = (uint8_t)v;
    }
    int rc = ck_inf_build(cl, CK_INF_CL_BITS, CK_INF_CL_CAP, lens, 19, CK_INF_KIND_CODES);
    if (rc) { b->cause = CK_INF_CL_NONE + rc - 1; return; }
    for (int i = 0; i < 320; i++) lens[i] = 0;
    for (uint32_t have_n = 0; have_n < nlen + ndist;) {
        const uint32_t e = ck_inf_look(cl, CK_INF_CL_BITS, ck_inf_peek(in, pos));
        if (!e || (uint64_t)(e & 15u) > ck_inf_bits(in) - pos) { b->cause = CK_INF_CLSYM; return; }
        pos += e & 15u;
        const uint32_t sym = e >> 4;
        if (sym < 16) { lens[have_n++] = (uint8_t)sym; continue; }
        uint32_t rep = 0;
        uint8_t prev = 0;
        if (sym == 16) {
            if (have_n == 0) { b->cause = CK_INF_REPEAT_FIRST; return; }
            prev = lens[have_n - 1];
            if (!ck_inf_take(in, &pos, 2, &rep)) { b->cause = CK_INF_REPEAT_ENDS; return; }
            rep += 3;
        } else if (sym == 17) {
            if (!ck_inf_take(in, &pos, 3, &rep)) { b->cause = CK_INF_REPEAT_ENDS; return; }
            rep += 3;
        } else {
            if (!ck_inf_take(in, &pos, 7, &rep)) { b->cause = CK_INF_REPEAT_ENDS; return; }
            rep += 11;
        }
        if (have_n + rep > nlen + ndist) { b->cause = CK_INF_REPEAT_PAST; return; }
        while (rep--) lens[have_n++] = prev;
    }
    if (lens[256] == 0) { b->cause = CK_INF_NO_EOB; return; }
    rc = ck_inf_build(lit, CK_INF_LIT_BITS, CK_INF_LIT_CAP, lens, (int)nlen, CK_INF_KIND_LENS);
    if (rc) { b->cause = CK_INF_LIT_NONE + rc - 1; return; }
    rc = ck_inf_build(dist, CK_INF_DIST_BITS, CK_INF_DIST_CAP, lens + nlen, (int)ndist, CK_INF_KIND_DISTS);
    if (rc) { b->cause = CK_INF_DIST_NONE + rc - 1; return; }
    b->pos = pos;
}
// the two bytes in front of the deflate data
CK_HD inline int ck_inf_wrapper(const CkInfIn& in, uint32_t* arg0)
{
    *arg0 = (uint32_t)in.bytes;
    if (!in.z || in.bytes < 2) return CK_INF_ZLIB_SHORT;
    if (((uint32_t)in.z[0] << 8 | in.z[1]) % 31) return CK_INF_ZLIB_CHECK;
    *arg0 = in.z[0] & 15u;
    if ((in.z[0] & 15) != 8) return CK_INF_ZLIB_METHOD;
    *arg0 = in.z[0] >> 4;
    if ((in.z[0] >> 4) > 7) return CK_INF_ZLIB_WINDOW;
    if (in.z[1] & 0x20) return CK_INF_ZLIB_DICT;
    return CK_INF_OK;
}

// ---- token ----
enum { CK_INF_LITERAL = 0, CK_INF_MATCH = 1, CK_INF_EOB = 2, CK_INF_REFUSED = 3 };
// a token in two words.  pk: the bits it consumed (0 .. 48) | the bytes it writes << 6 | its kind << 15; val: the literal, the
// distance or the cause
CK_HD inline uint64_t ck_inf_pack(uint32_t kind, uint32_t bits, uint32_t len, uint32_t val) { return (uint64_t)val << 32 | kind << 15 | len << 6 | bits; }
CK_HD inline uint32_t ck_inf_kind(uint64_t t) { return ((uint32_t)t >> 15) & 3u; }
CK_HD inline uint32_t ck_inf_nbits(uint64_t t) { return (uint32_t)t & 63u; }
CK_HD inline uint32_t ck_inf_len(uint64_t t) { return ((uint32_t)t >> 6) & 511u; }
CK_HD inline uint32_t ck_inf_val(uint64_t t) { return (uint32_t)(t >> 32); }
// length symbol s - 257 (0 .. 28) and distance symbol (0 .. 29) -> base and extra bits (RFC 1951, 3.2.5)
CK_HD inline void ck_inf_length(uint32_t s, uint32_t* base, uint32_t* eb)
{
    if (s < 8) { *base = 3 + s; *eb = 0; }
    else if (s == 28) { *base = 258; *eb = 0; }
    else { *eb = (s - 4) >> 2; *base = 3 + ((4 + (s & 3u)) << *eb); }
}
CK_HD inline void ck_inf_distance(uint32_t s, uint32_t* base, uint32_t* eb)
{
    if (s < 4) { *base = 1 + s; *eb = 0; }
    else { *eb = (s - 2) >> 1; *base = 1 + ((2 + (s & 1u)) << *eb); }
}
// the token that starts where `b` starts (ck_inf_peek), `left` bits of the stream from there on (<= 0: none)
CK_HD inline uint64_t ck_inf_token(uint64_t b, int64_t left, const uint16_t* lit, const uint16_t* dist)
{
    uint32_t e = ck_inf_look(lit, CK_INF_LIT_BITS, b);
    if (!e || (int64_t)(e & 15u) > left) return ck_inf_pack(CK_INF_REFUSED, 0, 0, CK_INF_TOK_LITLEN);
    uint32_t n = e & 15u, sym = e >> 4;
    if (sym < 256) return ck_inf_pack(CK_INF_LITERAL, n, 1, sym);
    if (sym == 256) return ck_inf_pack(CK_INF_EOB, n, 0, 0);
    sym -= 257;
    if (sym >= 29) return ck_inf_pack(CK_INF_REFUSED, 0, 0, CK_INF_TOK_LITLEN_SYMBOL);
    uint32_t base, eb;
    ck_inf_length(sym, &base, &eb);
    if ((int64_t)(n + eb) > left) return ck_inf_pack(CK_INF_REFUSED, 0, 0, CK_INF_TOK_LENGTH_ENDS);
    const uint32_t len = base + ((uint32_t)(b >> n) & ((1u << eb) - 1));
    n += eb;
    e = ck_inf_look(dist, CK_INF_DIST_BITS, b >> n);
    if (!e || (int64_t)(n + (e & 15u)) > left) return ck_inf_pack(CK_INF_REFUSED, 0, 0, CK_INF_TOK_DIST);
    n += e & 15u;
    sym = e >> 4;
    if (sym >= 30) return ck_inf_pack(CK_INF_REFUSED, 0, 0, CK_INF_TOK_DIST_SYMBOL);
    ck_inf_distance(sym, &base, &eb);
    if ((int64_t)(n + eb) > left) return ck_inf_pack(CK_INF_REFUSED, 0, 0, CK_INF_TOK_DIST_ENDS);
    const uint32_t d = base + ((uint32_t)(b >> n) & ((1u << eb) - 1));
    return ck_inf_pack(CK_INF_MATCH, n + eb, len, d);
}

// ---- walk ----
struct CkInfWalk {
    uint32_t advance;                                        // bits the step consumed
    uint32_t tokens, bytes;                                  // literals and matches taken; what they write
    uint32_t end, cause;                                     // CK_INF_EOB: the block ends behind the step; CK_INF_REFUSED: the stream, with `cause`
    uint32_t far;                                            // a match reads a ring slot the step overwrites: apply in chain order
    uint64_t taken[CK_INF_OPL];                              // bit l of word j: the token at offset 64 j + l is real
};
// get(o): the token at offset o of the window; place(o, q): the token at o is real and writes from byte q of the step on.
// produced: the bytes in front of the step; limit: the most tokens to take (CK_INF_WINDOW: as many as the window holds)
template <class Get, class Place>
CK_HD inline void ck_inf_walk(Get get, Place place, uint64_t produced, uint32_t limit, CkInfWalk* w)
{
    w->advance = w->tokens = w->bytes = w->end = w->cause = w->far = 0;
    for (int j = 0; j < CK_INF_OPL; j++) w->taken[j] = 0;
    int64_t reach = 0;                                       // the least q - d of the step's matches (0: none before the step's start)
    uint32_t o = 0;
    while (o < (uint32_t)CK_INF_WINDOW && w->tokens < limit) {
        const uint64_t t = get(o);
        const uint32_t kind = ck_inf_kind(t), len = ck_inf_len(t);
        if (kind == CK_INF_REFUSED) { w->end = CK_INF_REFUSED; w->cause = ck_inf_val(t); break; }
        if (kind == CK_INF_EOB) { o += ck_inf_nbits(t); w->end = CK_INF_EOB; break; }
        if (w->bytes + len > (uint32_t)CK_INF_STEP_BYTES) break;
        if (kind == CK_INF_MATCH) {
            const uint64_t d = ck_inf_val(t);
            if (d > produced + w->bytes) { w->end = CK_INF_REFUSED; w->cause = CK_INF_TOK_FAR; break; }
            if ((int64_t)w->bytes - (int64_t)d < reach) reach = (int64_t)w->bytes - (int64_t)d;
        }
        place(o, w->bytes);
        w->taken[o >> 6] |= 1ull << (o & 63);
        w->bytes += len; w->tokens++;
        o += ck_inf_nbits(t);
    }
    w->advance = o;
    w->far = reach < (int64_t)w->bytes - CK_INF_RING;
}

// ---- adler, rows ----
// the encoder's size step on ring bytes: positions [from, from + L), L <= CK_PNG_TILE_BYTES
CK_HD inline void ck_inf_tile_pair(const uint8_t* ring, uint64_t from, int L, uint32_t* a, uint32_t* b)
{
    uint32_t A = 0, B = 0;
    for (int i = 0; i < L; i++) {
        const uint32_t x = ring[(from + (uint64_t)i) & (CK_INF_RING - 1)];
        A += x; B += (uint32_t)(L - i) * x;
    }
    *a = A; *b = B;
}
// what ck_inf_adler_chunk works on: entry 0 is the running pair, 1 .. the tiles of the chunk
struct CkInfAdlerWork {
    uint32_t bits[CK_INF_FLUSH_TILES + 1], a[CK_INF_FLUSH_TILES + 1], b[CK_INF_FLUSH_TILES + 1];
    uint64_t off[CK_INF_FLUSH_TILES + 1];
};
CK_HD inline int ck_inf_chunk_tiles(int L) { return (L + CK_PNG_TILE_BYTES - 1) / CK_PNG_TILE_BYTES; }
// the running pair (*A, *B) and the pairs of a chunk of L bytes (wk->a, wk->b from entry 1 on) -> the pair behind the chunk:
// ck_png_scan_band over a band of one row whose tile 0 stands for everything before
CK_HD inline void ck_inf_adler_chunk(CkInfAdlerWork* wk, int L, uint32_t* A, uint32_t* B)
{
    CkPngGeom g;
    g.h = 1; g.w = 0;
    g.row = CK_PNG_TILE_BYTES + (int64_t)L; g.fbytes = g.row;
    g.bands = 1; g.band_tiles = 1 + ck_inf_chunk_tiles(L); g.tiles = g.band_tiles;
    for (int t = 0; t < g.band_tiles; t++) wk->bits[t] = 0;
    wk->a[0] = *A; wk->b[0] = *B;
    uint64_t bits;
    ck_png_scan_band(g, 0, wk->bits, wk->a, wk->b, 0, wk->off, &bits, A, B, 0);
}
// the rows (of `pitch` bytes, below position `need`) that start in [from, to): the first whose filter byte is above 4
// among rows first, first + stride, ..; -1: none
CK_HD inline int64_t ck_inf_row_check(const uint8_t* ring, uint64_t from, uint64_t to, uint64_t need, uint64_t pitch, uint64_t first, uint64_t stride, uint32_t* type)
{
    if (to > need) to = need;
    for (uint64_t y = (from + pitch - 1) / pitch + first; y * pitch < to; y += stride) {
        const uint8_t ft = ring[(y * pitch) & (CK_INF_RING - 1)];
        if (ft > 4) { *type = ft; return (int64_t)y; }
    }
    return -1;
}
