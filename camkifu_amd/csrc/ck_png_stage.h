// ck_png_stage.h -- the PNG encoder cut into steps that do not depend on one another, written once: plain C++ for the host
// (ck_png.cpp, tools/sanitize/png_fuzz.cpp) and device code for k_png.hip.  No HIP call in here; host and device differ in
// who runs the loops and in the sink that receives the bits.
//
// Terms.  A frame is h rows of ROW = 1 + 3w bytes: the filter type, then the residuals of the RGB bytes.  A BAND is
// CK_PNG_BAND_ROWS consecutive rows (the last band of a frame has what is left); a band is one deflate block with a dynamic
// Huffman code of its own, literals only.  A TILE is CK_PNG_TILE_BYTES consecutive bytes of one band (the last tile of a
// band is short, and the last band of a frame has empty tiles where it has fewer rows): every band has band_tiles of them.
//
// The steps:
//   filter  a row alone: the residuals of the five filter types read raw pixels only; the type with the least sum of
//           |residual as int8| wins, the lowest number among equals (libpng's heuristic), unless one type is forced.
//   count   a band alone: how often each byte value occurs, and one end-of-block symbol.
//   build   a band alone: the symbols in ascending (count, symbol) order (ck_png_rank) -> code lengths of a Huffman code
//           limited to 15 bits that satisfies Kraft with equality, or one code of one bit (ck_png_lengths), and the codes,
//           bit-reversed as deflate packs them.
//   size    a tile alone: the bits of its literals, and its Adler-32 pair (a: the sum of its bytes, b: sum of (L - i) x_i).
//   scan    a band alone: bit offsets of its tiles in its block, the bits of the block, its Adler pair (ck_png_scan_band);
//           then a frame alone: bit offsets of the bands, the bits of the frame, the Adler-32 (ck_png_scan_frame).
//   put     a band's header fields (ck_png_hdr_field) and end-of-block code, and a tile's literals, by OR into zeroed memory:
//           deflate packs bits LSB first, so bit p of the stream is bit p & 31 of little-endian dword p >> 5.
// The block header: BFINAL, BTYPE = 2, HLIT = 0 (257 codes), HDIST = 0 (one distance code), HCLEN = 15 (all 19 code-length
// codes); the code-length alphabet gives its symbols 0 .. 15 four bits each and 16 .. 18 none, a complete set, so a code
// length l is sent as the four bits of l; one distance code of length 0 follows.  CK_PNG_HDR_BITS bits in all.
//
// The runs mode (CK_PNG_MATCH_RUNS; `RUNS` below, a compile-time parameter of every step).  A RUN is a maximal interval
// [s, e) of equal bytes inside one band: runs cross rows and tiles, never a band's edge.  Byte s is a literal; the
// r = e - s - 1 bytes behind it are r = 258 k + t: k matches of length 258 and distance 1, then one match of length t
// where t >= 3, or t literals where t is 1 or 2.  So every position is a literal, the head of a match or covered by one
// (no token), by o = i - s - 1 and r alone: ck_png_run_role.  A token belongs to the tile that holds its first byte.
//   edges   a tile alone: its first and last byte and the lengths of the runs that touch its first and last position,
//           capped at the tile.
//   join    a band alone, its tiles in order (ck_png_join_band): how many bytes just before a tile equal its first byte,
//           how many just behind it equal its last.  With these and the starts of runs inside the tile every position
//           knows s and e.
//   count   over tokens: literals, the end-of-block symbol once, the length symbols 257 .. 285.
//   build   over CK_PNG_RUN_SYMS symbols; size: the bits of the tokens that start in the tile; scan: as above.
//   put     a match is the length symbol's code, its extra bits (LSB first), and the distance code, one bit 0.
// Its block header: HLIT = 29 (286 codes), HDIST = 1: two distance codes of length 1, a complete set in which distance 1 is
// the code 0 (a single code of length 1 is the incomplete set zlib never writes).  CK_PNG_RUN_HDR_BITS bits in all.
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

constexpr int CK_PNG_BAND_ROWS = 16;
constexpr int CK_PNG_TILE_BYTES = 1024;                      // 256 lanes, four literals each
constexpr int CK_PNG_SYMS = 257;                             // 256 literals and the end-of-block symbol
constexpr int CK_PNG_SYM_PITCH = 272;                        // of the per-band length and code arrays
constexpr int CK_PNG_MAX_BITS = 15;
constexpr int CK_PNG_HDR_FIELDS = 3 + CK_PNG_SYMS + 1;
constexpr int CK_PNG_HDR_BITS = 17 + 19 * 3 + CK_PNG_SYMS * 4 + 4;
constexpr uint32_t CK_PNG_ADLER = 65521;
// the runs mode: 29 length symbols behind the end-of-block symbol, arrays of a pitch of their own, two distance codes
constexpr int CK_PNG_RUN_SYMS = 286;
constexpr int CK_PNG_RUN_PITCH = 288;
constexpr int CK_PNG_RUN_HDR_FIELDS = 3 + CK_PNG_RUN_SYMS + 2;
constexpr int CK_PNG_RUN_HDR_BITS = 17 + 19 * 3 + CK_PNG_RUN_SYMS * 4 + 2 * 4;
constexpr int CK_PNG_MAX_MATCH = 258;
// what the arrays and the header of a mode need (runs: 0 the literal-only mode, 1 the runs mode)
CK_HD constexpr int ck_png_syms(int runs) { return runs ? CK_PNG_RUN_SYMS : CK_PNG_SYMS; }
CK_HD constexpr int ck_png_pitch(int runs) { return runs ? CK_PNG_RUN_PITCH : CK_PNG_SYM_PITCH; }
CK_HD constexpr int ck_png_hdr_fields(int runs) { return runs ? CK_PNG_RUN_HDR_FIELDS : CK_PNG_HDR_FIELDS; }
CK_HD constexpr int ck_png_hdr_bits(int runs) { return runs ? CK_PNG_RUN_HDR_BITS : CK_PNG_HDR_BITS; }

struct CkPngGeom {
    int32_t h, w;
    int64_t row, fbytes;                                     // bytes of a filtered row and of a filtered frame
    int64_t bands, band_tiles, tiles;                        // bands of a frame, tiles of a band, tiles of a frame
};

// h, w in 1 .. 65535: the callers check
CK_HD inline CkPngGeom ck_png_geom(int h, int w)
{
    CkPngGeom g;
    g.h = h; g.w = w;
    g.row = 1 + 3 * (int64_t)w;
    g.fbytes = g.row * h;
    g.bands = (h + CK_PNG_BAND_ROWS - 1) / CK_PNG_BAND_ROWS;
    g.band_tiles = (g.row * CK_PNG_BAND_ROWS + CK_PNG_TILE_BYTES - 1) / CK_PNG_TILE_BYTES;
    g.tiles = g.bands * g.band_tiles;
    return g;
}

CK_HD inline int64_t ck_png_band_bytes(const CkPngGeom& g, int64_t band)
{
    const int64_t rows = g.h - band * CK_PNG_BAND_ROWS < CK_PNG_BAND_ROWS ? g.h - band * CK_PNG_BAND_ROWS : CK_PNG_BAND_ROWS;
    return rows * g.row;
}
// where tile t of a band starts in the filtered frame, and its bytes (0 .. CK_PNG_TILE_BYTES)
CK_HD inline int64_t ck_png_tile_at(const CkPngGeom& g, int64_t band, int64_t t) { return band * CK_PNG_BAND_ROWS * g.row + t * CK_PNG_TILE_BYTES; }
CK_HD inline int ck_png_tile_len(const CkPngGeom& g, int64_t band, int64_t t)
{
    const int64_t left = ck_png_band_bytes(g, band) - t * CK_PNG_TILE_BYTES;
    return left <= 0 ? 0 : left < CK_PNG_TILE_BYTES ? (int)left : CK_PNG_TILE_BYTES;
}

// reading (k_png_unfilter): where the inflated rows of an image lie in the staged block, and how to expand them
struct CkPngDesc {
    int64_t off, rowbytes;
    int32_t color_type, depth, bpp, palette_n;
};
static_assert(sizeof(CkPngDesc) == 32, "a descriptor row is 32 bytes");

// ---- filter ----
// (a frame holds B, G, R; the PNG holds R, G, B: byte i of a row is channel 2 - i % 3 of pixel i / 3)
CK_HD inline int ck_png_paeth(int a, int b, int c)
{
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}
// the predictor of filter type ft from the left (a), upper (b) and upper-left (c) bytes
CK_HD inline int ck_png_predict(int ft, int a, int b, int c)
{
    return ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : ck_png_paeth(a, b, c);
}
// byte i of row y with its left (a), upper (b) and upper-left (c) neighbours, found with one division: the pixel to the
// left is three bytes back in the frame, the row above w pixels back
CK_HD inline void ck_png_context(const uint8_t* bgr, int w, int64_t y, int64_t i, int* x, int* a, int* b, int* c)
{
    const int64_t px = i / 3;
    const uint8_t* p = bgr + (y * w + px) * 3 + 2 - (i - 3 * px);
    *x = p[0];
    *a = px > 0 ? p[-3] : 0;
    *b = y > 0 ? p[-3 * (int64_t)w] : 0;
    *c = px > 0 && y > 0 ? p[-3 * (int64_t)w - 3] : 0;
}
CK_HD inline uint8_t ck_png_residual(const uint8_t* bgr, int w, int64_t y, int64_t i, int ft)
{
    int x, a, b, c;
    ck_png_context(bgr, w, y, i, &x, &a, &b, &c);
    return (uint8_t)(x - ck_png_predict(ft, a, b, c));
}
CK_HD inline uint32_t ck_png_cost(uint8_t v) { return v < 128 ? v : 256u - v; }
CK_HD inline int ck_png_choose(const uint32_t* sum)
{
    int best = 0;
    for (int ft = 1; ft < 5; ft++)
        if (sum[ft] < sum[best]) best = ft;
    return best;
}

// ---- build ----
// the place of symbol s among the symbols that occur, in ascending (count, symbol) order; symbols: how many occur
template <int NS = CK_PNG_SYMS>
CK_HD inline int ck_png_rank(const uint32_t* count, int s)
{
    int r = 0;
    for (int j = 0; j < NS; j++)
        r += count[j] != 0 && (count[j] < count[s] || (count[j] == count[s] && j < s));
    return r;
}
CK_HD inline uint32_t ck_png_reverse(uint32_t code, int bits)
{
    uint32_t r = 0;
    for (int i = 0; i < bits; i++) r |= ((code >> i) & 1u) << (bits - 1 - i);
    return r;
}
// order[0 .. m): the symbols that occur, by ck_png_rank; A: m words of work.  -> len[NS] (0: the symbol does not
// occur) and the codes, reversed.  The lengths are those of a Huffman tree over the counts (Moffat and Katajainen's in-place
// computation over the sorted counts); where the tree is deeper than 15, codes above 15 bits are cut to 15 and, for every
// unit of 2^-15 the Kraft sum is above 1 then, one 15-bit code is taken away and the longest shorter code is split in two
// one bit longer -- the sum falls by exactly that unit, the number of codes stays -- and the lengths are handed out again,
// the longest to the rarest.  m = 1: one code of one bit (the set zlib accepts although it is incomplete).
template <int NS = CK_PNG_SYMS>
CK_HD inline void ck_png_lengths(const uint32_t* count, const uint16_t* order, int m, uint32_t* A, uint8_t* len, uint16_t* code)
{
    for (int s = 0; s < NS; s++) { len[s] = 0; code[s] = 0; }
    if (m <= 0) return;
    uint32_t bl[CK_PNG_MAX_BITS + 2];
    for (int l = 0; l <= CK_PNG_MAX_BITS + 1; l++) bl[l] = 0;
    if (m == 1) {
        bl[1] = 1;
    } else {
        for (int i = 0; i < m; i++) A[i] = count[order[i]];
        A[0] += A[1];
        int root = 0, leaf = 2;
        for (int next = 1; next < m - 1; next++) {
            if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; } else A[next] = A[leaf++];
            if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; } else A[next] += A[leaf++];
        }
        A[m - 2] = 0;
        for (int next = m - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
        int avail = 1, used = 0, depth = 0, next = m - 1;
        root = m - 2;
        while (avail > 0) {
            while (root >= 0 && (int)A[root] == depth) { used++; root--; }
            while (avail > used) { A[next--] = (uint32_t)depth; avail--; }
            avail = 2 * used; depth++; used = 0;
        }
        bool cut = false;
        for (int i = 0; i < m; i++) {
            if (A[i] > (uint32_t)CK_PNG_MAX_BITS) cut = true;
            bl[A[i] > (uint32_t)CK_PNG_MAX_BITS ? CK_PNG_MAX_BITS : A[i]]++;
        }
        if (cut) {
            uint32_t total = 0;
            for (int l = 1; l <= CK_PNG_MAX_BITS; l++) total += bl[l] << (CK_PNG_MAX_BITS - l);
            while (total > (1u << CK_PNG_MAX_BITS)) {
                bl[CK_PNG_MAX_BITS]--;
                for (int l = CK_PNG_MAX_BITS - 1; l > 0; l--)
                    if (bl[l]) { bl[l]--; bl[l + 1] += 2; break; }
                total--;
            }
        }
    }
    int at = 0;
    for (int l = CK_PNG_MAX_BITS; l >= 1; l--)
        for (uint32_t k = 0; k < bl[l]; k++) len[order[at++]] = (uint8_t)l;
    uint32_t next_code[CK_PNG_MAX_BITS + 2], c = 0;
    bl[0] = 0;
    for (int l = 1; l <= CK_PNG_MAX_BITS; l++) { c = (c + bl[l - 1]) << 1; next_code[l] = c; }
    for (int s = 0; s < NS; s++)
        if (len[s]) code[s] = (uint16_t)ck_png_reverse(next_code[len[s]]++, len[s]);
}

// ---- runs ----
enum { CK_PNG_ROLE_LITERAL = 0, CK_PNG_ROLE_HEAD = 1, CK_PNG_ROLE_COVERED = 2 };
// position i of the run [s, e): o = i - s - 1 (-1: the run's first byte), r = e - s - 1 -> its role, and for the head of a
// match the match's length
CK_HD inline int ck_png_run_role(int o, int r, int* len)
{
    *len = 0;
    if (o < 0) return CK_PNG_ROLE_LITERAL;
    const int full = r - r % CK_PNG_MAX_MATCH, t = r - full;
    if (o < full) {
        if (o % CK_PNG_MAX_MATCH) return CK_PNG_ROLE_COVERED;
        *len = CK_PNG_MAX_MATCH;
        return CK_PNG_ROLE_HEAD;
    }
    if (t < 3) return CK_PNG_ROLE_LITERAL;
    if (o > full) return CK_PNG_ROLE_COVERED;
    *len = t;
    return CK_PNG_ROLE_HEAD;
}
// a match length 3 .. 258 -> its symbol 257 .. 285, the number of its extra bits and their value (RFC 1951, 3.2.5): eight
// symbols without extra bits, then four symbols for every number of extra bits 1 .. 5, and 258 on its own
CK_HD inline int ck_png_len_symbol(int len, int* extra_bits, uint32_t* extra)
{
    *extra_bits = 0; *extra = 0;
    if (len == CK_PNG_MAX_MATCH) return 285;
    const int x = len - 3;
    if (x < 8) return 257 + x;
    int eb = 1;
    while (x >> (eb + 3)) eb++;
    *extra_bits = eb;
    *extra = (uint32_t)x & ((1u << eb) - 1);
    return 261 + 4 * eb + ((x >> eb) & 3);
}
// the token that starts at a position: the byte x there, o and r as for ck_png_run_role -> its symbol (-1: covered, no
// token), and what follows the symbol's code: `tail_bits` bits of value `tail` (a match's extra bits, then the distance code 0)
CK_HD inline int ck_png_token(uint32_t x, int o, int r, int* tail_bits, uint32_t* tail)
{
    int len;
    *tail_bits = 0; *tail = 0;
    const int role = ck_png_run_role(o, r, &len);
    if (role == CK_PNG_ROLE_COVERED) return -1;
    if (role == CK_PNG_ROLE_LITERAL) return (int)x;
    int eb;
    const int sym = ck_png_len_symbol(len, &eb, tail);
    *tail_bits = eb + 1;
    return sym;
}
// what the edges step gives for a tile
struct CkPngEdge {
    uint8_t first, last;                                     // its first and last byte
    uint16_t head, tail;                                     // bytes at its start equal to the first, at its end equal to the last
};
CK_HD inline CkPngEdge ck_png_edge(const uint8_t* p, int L)
{
    CkPngEdge e;
    e.first = e.last = 0; e.head = e.tail = 0;
    if (L <= 0) return e;
    e.first = p[0]; e.last = p[L - 1];
    int n = 1;
    while (n < L && p[n] == e.first) n++;
    e.head = (uint16_t)n;
    n = 1;
    while (n < L && p[L - 1 - n] == e.last) n++;
    e.tail = (uint16_t)n;
    return e;
}
// a band's tiles in order -> before[t]: how many bytes just before tile t equal its first byte, after[t]: how many just
// behind it equal its last byte (both inside the band; 0 for an empty tile)
CK_HD inline void ck_png_join_band(const CkPngGeom& g, int64_t band, const CkPngEdge* edge, uint32_t* before, uint32_t* after)
{
    uint32_t run = 0;                                        // the bytes at the end of the tiles so far that equal `v`
    int v = -1;
    for (int64_t t = 0; t < g.band_tiles; t++) {
        const int L = ck_png_tile_len(g, band, t);
        before[t] = L > 0 && v == edge[t].first ? run : 0;
        if (L <= 0) continue;
        if (edge[t].tail == L && v == edge[t].last) run += (uint32_t)L;
        else { v = edge[t].last; run = edge[t].tail; }
    }
    run = 0; v = -1;
    for (int64_t t = g.band_tiles - 1; t >= 0; t--) {
        const int L = ck_png_tile_len(g, band, t);
        after[t] = L > 0 && v == edge[t].last ? run : 0;
        if (L <= 0) continue;
        if (edge[t].head == L && v == edge[t].first) run += (uint32_t)L;
        else { v = edge[t].first; run = edge[t].head; }
    }
}

// ---- size, scan ----
// a band's tiles in order (tile_bits, tile_a, tile_b: band_tiles each) and the length of its end-of-block code -> where each
// tile starts, in bits from the start of the band's block (its header comes first), the bits of the whole block, and the
// band's Adler pair: a the sum of its bytes, b the sum of (bytes of the band - i) x_i, both mod 65521
CK_HD inline void ck_png_scan_band(const CkPngGeom& g, int64_t band, const uint32_t* tile_bits, const uint32_t* tile_a, const uint32_t* tile_b,
                                   int eob_len, uint64_t* tile_off, uint64_t* band_bits, uint32_t* band_a, uint32_t* band_b,
                                   int hdr_bits = CK_PNG_HDR_BITS)
{
    uint64_t pos = (uint64_t)hdr_bits, A = 0, B = 0;
    for (int64_t t = 0; t < g.band_tiles; t++) {
        tile_off[t] = pos;
        pos += tile_bits[t];
        B = (B + (uint64_t)ck_png_tile_len(g, band, t) * A + tile_b[t]) % CK_PNG_ADLER;
        A = (A + tile_a[t]) % CK_PNG_ADLER;
    }
    *band_bits = pos + (uint64_t)eob_len;
    *band_a = (uint32_t)A;
    *band_b = (uint32_t)B;
}
// the frame's bands in order -> where each band's block starts, in bits from the start of the frame's deflate data, the
// bits of all of it, and the Adler-32 of the filtered frame
CK_HD inline void ck_png_scan_frame(const CkPngGeom& g, const uint64_t* band_bits, const uint32_t* band_a, const uint32_t* band_b,
                                    uint64_t* band_off, uint64_t* frame_bits, uint32_t* adler)
{
    uint64_t pos = 0, A = 1, B = 0;
    for (int64_t band = 0; band < g.bands; band++) {
        band_off[band] = pos;
        pos += band_bits[band];
        B = (B + (uint64_t)ck_png_band_bytes(g, band) % CK_PNG_ADLER * A + band_b[band]) % CK_PNG_ADLER;
        A = (A + band_a[band]) % CK_PNG_ADLER;
    }
    *frame_bits = pos;
    *adler = (uint32_t)(B << 16 | A);
}
// a zlib stream: two bytes of header, the deflate data, the Adler-32
CK_HD inline uint64_t ck_png_zlib_bytes(uint64_t frame_bits) { return 2 + (frame_bits + 7) / 8 + 4; }

// ---- put ----
// field i (0 .. CK_PNG_HDR_FIELDS) of a band's block header -> its value, its bits and where it starts in the header
CK_HD inline void ck_png_hdr_field(int i, const uint8_t* len, int bfinal, uint32_t* value, int* nbits, int* offset)
{
    if (i == 0) {                                            // BFINAL, BTYPE 2, HLIT 0, HDIST 0, HCLEN 15
        *value = (uint32_t)(bfinal & 1) | 2u << 1 | 15u << 13; *nbits = 17; *offset = 0;
    } else if (i == 1) {                                     // code-length code lengths of 16, 17, 18 (none), 0, 8, 7, 9, 6, 10, 5 (four bits)
        uint32_t v = 0;
        for (int k = 3; k < 10; k++) v |= 4u << (3 * k);
        *value = v; *nbits = 30; *offset = 17;
    } else if (i == 2) {                                     // of 11, 4, 12, 3, 13, 2, 14, 1, 15
        uint32_t v = 0;
        for (int k = 0; k < 9; k++) v |= 4u << (3 * k);
        *value = v; *nbits = 27; *offset = 47;
    } else if (i < 3 + CK_PNG_SYMS) {                        // a literal/length code length: the code of symbol l is l in four bits
        *value = ck_png_reverse(len[i - 3], 4); *nbits = 4; *offset = 74 + 4 * (i - 3);
    } else {                                                 // the one distance code: length 0
        *value = 0; *nbits = 4; *offset = 74 + 4 * CK_PNG_SYMS;
    }
}
// the same for the runs mode's header, field i (0 .. CK_PNG_RUN_HDR_FIELDS); len: CK_PNG_RUN_SYMS code lengths
CK_HD inline void ck_png_run_hdr_field(int i, const uint8_t* len, int bfinal, uint32_t* value, int* nbits, int* offset)
{
    if (i == 0) {                                            // BFINAL, BTYPE 2, HLIT 29, HDIST 1, HCLEN 15
        *value = (uint32_t)(bfinal & 1) | 2u << 1 | 29u << 3 | 1u << 8 | 15u << 13; *nbits = 17; *offset = 0;
    } else if (i < 3) {                                      // the code-length code is the same
        ck_png_hdr_field(i, len, bfinal, value, nbits, offset);
    } else if (i < 3 + CK_PNG_RUN_SYMS) {
        *value = ck_png_reverse(len[i - 3], 4); *nbits = 4; *offset = 74 + 4 * (i - 3);
    } else {                                                 // two distance codes of length 1: distance 1 is the code 0
        *value = ck_png_reverse(1, 4); *nbits = 4; *offset = 74 + 4 * (i - 3);
    }
}
// host sink: OR `nbits` (up to 32) bits of v into zeroed bytes at bit `pos`
inline void ck_png_or_bits(uint8_t* buf, uint64_t pos, uint32_t v, int nbits)
{
    uint64_t x = (uint64_t)v << (pos & 7);
    for (uint64_t at = pos >> 3, end = (pos + (uint64_t)nbits + 7) >> 3; at < end; at++, x >>= 8) buf[at] |= (uint8_t)x;
}
