// ck_jpeg_enc.cpp -- quant tables, JFIF headers and the Huffman coder of baseline JPEG (see ck_jpeg_enc.h), in libjpeg's
// order and with its choices, so that the stream equals what its default compressor writes.  Plain C++: no HIP, no context.
#include "ck_jpeg_enc.h"
#include "ck_jpeg_tables.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

namespace {

// Annex K.1 and K.2, natural order
const uint8_t BASE_LUMA[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                               69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55, 64,
                               81, 104, 113, 92, 49, 64, 78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
const uint8_t BASE_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                 99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

constexpr size_t HEADER_BOUND = CK_JPEG_ENC_HEADER_BOUND;   // SOI, APP0, 2 DQT, SOF0, 4 DHT, DRI, SOS, EOI: 629 bytes
constexpr size_t BLOCK_BOUND = 64 * 26 / 8 * 2;

int refuse(char* msg, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, CK_JPEG_MSG, fmt, ap);
    va_end(ap);
    return CK_ERR_ARG;
}

void fill(CkEncHuff& t, const uint8_t* bits, const uint8_t* vals)
{
    memset(&t, 0, sizeof t);
    int c = 0, k = 0;
    for (int l = 1; l <= 16; l++) {
        for (int i = 0; i < bits[l - 1]; i++, c++, k++) { t.code[vals[k]] = (uint16_t)c; t.len[vals[k]] = (uint8_t)l; }
        c <<= 1;
    }
}

// bytes appended to a buffer of known end; the callers leave room before they write
struct Out {
    uint8_t* p;
    void byte(unsigned b) { *p++ = (uint8_t)b; }
    void be16(unsigned v) { byte(v >> 8); byte(v & 255); }
    void segment(unsigned marker, size_t body) { byte(0xFF); byte(marker); be16((unsigned)body + 2); }
};

// the entropy-coded segment: bits collected in a 64-bit word, whole bytes flushed with a 00 behind every FF.  At most 32
// bits are put at once, and fewer than 8 are ever left behind, so the word does not overflow.
struct BitWriter {
    uint8_t* p;
    uint64_t acc = 0;
    int n = 0;
    inline void put(uint32_t v, int len)
    {
        acc = (acc << len) | (v & ((1u << len) - 1));
        n += len;
        while (n >= 8) {
            const unsigned b = (unsigned)(acc >> (n - 8)) & 255u;
            *p++ = (uint8_t)b;
            if (b == 0xFF) *p++ = 0;
            n -= 8;
        }
    }
    void pad() { if (n) put((1u << (8 - n)) - 1, 8 - n); }
};

// what both coders refuse before they read a coefficient, in one order
int check_args(const int16_t* coef, const uint16_t* quant, int h, int w, int sampling, int restart_interval, const uint8_t* out,
               const size_t* len, char* msg)
{
    if (!coef || !quant || !out || !len) return refuse(msg, "NULL pointer");
    if (h < 1 || w < 1 || h > 65535 || w > 65535) return refuse(msg, "bad JPEG frame size %dx%d: sides of 1 .. 65535", w, h);
    if (sampling < CK_JPEG_GREY || sampling > CK_JPEG_420) return refuse(msg, "bad JPEG sampling %d", sampling);
    if (restart_interval < 0 || restart_interval > 65535) return refuse(msg, "restart interval %d: 0 .. 65535 MCUs", restart_interval);
    const bool grey = sampling == CK_JPEG_GREY;
    for (int i = 0; i < (grey ? 64 : 192); i++)
        if (quant[i] < 1 || quant[i] > 255) return refuse(msg, "quant entry %d is %d: baseline tables hold 1 .. 255", i, quant[i]);
    if (!grey && memcmp(quant + 64, quant + 128, 64 * sizeof(uint16_t)) != 0) return refuse(msg, "Cb and Cr share one quant table");
    return CK_OK;
}

}  // namespace

int ck_jpeg_enc_check(const uint16_t* quant, int h, int w, int sampling, int restart_interval, char* msg)
{
    static const int16_t some = 0;
    static const size_t one = 0;
    static const uint8_t byte = 0;
    msg[0] = 0;
    return check_args(&some, quant, h, w, sampling, restart_interval, &byte, &one, msg);
}

const CkEncTables& ck_jpeg_enc_tables()
{
    static const CkEncTables t = [] {
        CkEncTables x;
        fill(x.dc[0], STD_DC_LUMA_BITS, STD_DC_VALS);
        fill(x.dc[1], STD_DC_CHROMA_BITS, STD_DC_VALS);
        fill(x.ac[0], STD_AC_LUMA_BITS, STD_AC_LUMA_VALS);
        fill(x.ac[1], STD_AC_CHROMA_BITS, STD_AC_CHROMA_VALS);
        return x;
    }();
    return t;
}

const uint8_t* ck_jpeg_enc_zigzag() { return ZIGZAG; }

void ck_jpeg_enc_quant(int quality, uint16_t* quant)
{
    const int q = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
    const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int c = 0; c < 3; c++)
        for (int i = 0; i < 64; i++) {
            const int v = ((c ? BASE_CHROMA[i] : BASE_LUMA[i]) * scale + 50) / 100;
            quant[c * 64 + i] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
}

size_t ck_jpeg_enc_bound(int h, int w, int sampling)
{
    if (h < 1 || w < 1 || h > 65535 || w > 65535 || sampling < CK_JPEG_GREY || sampling > CK_JPEG_420) return 0;
    const int hs = ck_jpeg_luma_h(sampling), vs = ck_jpeg_luma_v(sampling);
    const size_t mcus = (size_t)((w + 8 * hs - 1) / (8 * hs)) * (size_t)((h + 8 * vs - 1) / (8 * vs));
    return HEADER_BOUND + (size_t)ck_jpeg_blocks(h, w, sampling) * BLOCK_BOUND + mcus * 4;
}

// in libjpeg's order: what stands in front of the DHT segments, ...
static void header_front(Out& o, const uint16_t* quant, int h, int w, int sampling)
{
    const bool grey = sampling == CK_JPEG_GREY;
    const int ncomp = grey ? 1 : 3;
    o.byte(0xFF); o.byte(0xD8);
    static const uint8_t JFIF[14] = {0x4A, 0x46, 0x49, 0x46, 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00};
    o.segment(0xE0, sizeof JFIF);
    for (uint8_t b : JFIF) o.byte(b);
    for (int t = 0; t < (grey ? 1 : 2); t++) {
        o.segment(0xDB, 65);
        o.byte((unsigned)t);
        for (int i = 0; i < 64; i++) o.byte(quant[t * 64 + ZIGZAG[i]]);
    }
    const int hs = ck_jpeg_luma_h(sampling), vs = ck_jpeg_luma_v(sampling);
    o.segment(0xC0, 6 + 3 * (size_t)ncomp);
    o.byte(8); o.be16((unsigned)h); o.be16((unsigned)w); o.byte((unsigned)ncomp);
    for (int c = 0; c < ncomp; c++) { o.byte((unsigned)c + 1); o.byte(c == 0 ? (unsigned)(hs * 16 + vs) : 0x11u); o.byte(c ? 1u : 0u); }
}
// ... and what stands behind them
static void header_back(Out& o, int sampling, int restart_interval)
{
    const int ncomp = sampling == CK_JPEG_GREY ? 1 : 3;
    if (restart_interval) { o.segment(0xDD, 2); o.be16((unsigned)restart_interval); }
    o.segment(0xDA, 4 + 2 * (size_t)ncomp);
    o.byte((unsigned)ncomp);
    for (int c = 0; c < ncomp; c++) { o.byte((unsigned)c + 1); o.byte(c ? 0x11u : 0x00u); }
    o.byte(0); o.byte(63); o.byte(0);
}

size_t ck_jpeg_enc_headers(const uint16_t* quant, int h, int w, int sampling, int restart_interval, uint8_t* out)
{
    const bool grey = sampling == CK_JPEG_GREY;
    Out o{out};
    header_front(o, quant, h, w, sampling);
    const struct { unsigned id; const uint8_t* bits; const uint8_t* vals; } dht[4] = {
        {0x00, STD_DC_LUMA_BITS, STD_DC_VALS}, {0x10, STD_AC_LUMA_BITS, STD_AC_LUMA_VALS},
        {0x01, STD_DC_CHROMA_BITS, STD_DC_VALS}, {0x11, STD_AC_CHROMA_BITS, STD_AC_CHROMA_VALS}};
    for (int t = 0; t < (grey ? 2 : 4); t++) {
        int total = 0;
        for (int i = 0; i < 16; i++) total += dht[t].bits[i];
        o.segment(0xC4, 17 + (size_t)total);
        o.byte(dht[t].id);
        for (int i = 0; i < 16; i++) o.byte(dht[t].bits[i]);
        for (int i = 0; i < total; i++) o.byte(dht[t].vals[i]);
    }
    header_back(o, sampling, restart_interval);
    return (size_t)(o.p - out);
}

void ck_jpeg_enc_header_parts(const uint16_t* quant, int h, int w, int sampling, int restart_interval, uint8_t* pre, uint32_t* pre_len,
                              uint8_t* post, uint32_t* post_len)
{
    Out a{pre}, b{post};
    header_front(a, quant, h, w, sampling);
    header_back(b, sampling, restart_interval);
    *pre_len = (uint32_t)(a.p - pre);
    *post_len = (uint32_t)(b.p - post);
}

int ck_jpeg_enc_entropy(const int16_t* coef, const uint16_t* quant, int h, int w, int sampling, int restart_interval,
                        uint8_t* out, size_t cap, size_t* len, char* msg)
{
    msg[0] = 0;
    if (len) *len = 0;
    if (const int rc = check_args(coef, quant, h, w, sampling, restart_interval, out, len, msg)) return rc;
    if (cap < HEADER_BOUND) return refuse(msg, "output buffer of %zu bytes: too small for the headers", cap);
    const bool grey = sampling == CK_JPEG_GREY;
    const int ncomp = grey ? 1 : 3;
    const int hs = ck_jpeg_luma_h(sampling), vs = ck_jpeg_luma_v(sampling);
    uint8_t* const scan = out + ck_jpeg_enc_headers(quant, h, w, sampling, restart_interval, out);

    // ---- the scan ----
    const CkEncTables& T = ck_jpeg_enc_tables();
    const int mcux = (w + 8 * hs - 1) / (8 * hs), mcuy = (h + 8 * vs - 1) / (8 * vs);
    const int lw = mcux * hs, lh = mcuy * vs;
    const size_t base[3] = {0, (size_t)lw * lh, (size_t)lw * lh + (size_t)mcux * mcuy};
    const uint8_t* const end = out + cap;
    BitWriter bw{scan};
    int pred[3] = {0, 0, 0};
    int since = 0, nrst = 0;
    const long long total = (long long)mcux * mcuy;
    const size_t mcu_blocks = grey ? 1 : (size_t)(hs * vs + 2);
    for (long long mcu = 0; mcu < total; mcu++) {
        // room for this MCU at its worst (its blocks; padding, its stuffing and a marker in front) and for the end of the
        // stream, before a byte of it is written: a buffer of ck_jpeg_enc_bound bytes always has it
        if ((size_t)(end - bw.p) < mcu_blocks * BLOCK_BOUND + 8)
            return refuse(msg, "output buffer of %zu bytes: too small (MCU %lld of %lld)", cap, mcu, total);
        if (restart_interval && since == restart_interval) {
            bw.pad();
            *bw.p++ = 0xFF; *bw.p++ = (uint8_t)(0xD0 + (nrst++ & 7));
            since = 0;
            pred[0] = pred[1] = pred[2] = 0;
        }
        since++;
        const int my = (int)(mcu / mcux), mx = (int)(mcu % mcux);
        for (int c = 0; c < ncomp; c++) {
            const int bh = (c == 0 && !grey) ? hs : 1, bv = (c == 0 && !grey) ? vs : 1;
            const int gw = c == 0 ? lw : mcux;
            const CkEncHuff& dc = T.dc[c ? 1 : 0];
            const CkEncHuff& ac = T.ac[c ? 1 : 0];
            for (int v = 0; v < bv; v++)
                for (int u = 0; u < bh; u++) {
                    const int16_t* blk = coef + (base[c] + (size_t)(my * bv + v) * gw + (size_t)(mx * bh + u)) * 64;
                    const int diff = (int)blk[0] - pred[c];
                    pred[c] = blk[0];
                    int s = ck_enc_bit_size(diff);
                    if (s > 11) return refuse(msg, "DC difference of %d bits (MCU %lld): baseline JPEG has 11", s, mcu);
                    bw.put(dc.code[s], dc.len[s]);
                    if (s) bw.put((uint32_t)(diff < 0 ? diff - 1 : diff), s);
                    int run = 0;
                    for (int k = 1; k < 64; k++) {
                        const int val = blk[ZIGZAG[k]];
                        if (val == 0) { run++; continue; }
                        for (; run > 15; run -= 16) bw.put(ac.code[0xF0], ac.len[0xF0]);
                        s = ck_enc_bit_size(val);
                        if (s > 10) return refuse(msg, "AC value of %d bits (MCU %lld): baseline JPEG has 10", s, mcu);
                        const int sym = (run << 4) | s;
                        bw.put(ac.code[sym], ac.len[sym]);
                        bw.put((uint32_t)(val < 0 ? val - 1 : val), s);
                        run = 0;
                    }
                    if (run) bw.put(ac.code[0], ac.len[0]);
                }
        }
    }
    if ((size_t)(end - bw.p) < 4) return refuse(msg, "output buffer of %zu bytes: too small", cap);
    bw.pad();
    *bw.p++ = 0xFF; *bw.p++ = 0xD9;
    *len = (size_t)(bw.p - out);
    return CK_OK;
}

void ck_jpeg_enc_status_message(uint32_t status, long long mcu, char* msg)
{
    const int size = (int)(status & 255);
    if (((status >> 8) & 255) == CK_ENC_DC) snprintf(msg, CK_JPEG_MSG, "DC difference of %d bits (MCU %lld): baseline JPEG has 11", size, mcu);
    else snprintf(msg, CK_JPEG_MSG, "AC value of %d bits (MCU %lld): baseline JPEG has 10", size, mcu);
}

// The steps of ck_jpeg_enc_stage.h in plain loops, tile by tile as the kernels of k_jpeg_enc_huff.hip run them; with
// `optimise` the histo and tables steps first, and the tables and the header of each frame its own.
static int staged(const int16_t* coef, const uint16_t* quant, int n, int h, int w, int sampling, int restart_interval,
                  uint8_t* out, size_t stride, size_t* len, int* bad, char* msg, bool optimise)
{
    msg[0] = 0;
    *bad = -1;
    if (len) for (int f = 0; f < n; f++) len[f] = 0;
    if (const int rc = check_args(coef, quant, h, w, sampling, restart_interval, out, len, msg)) { *bad = 0; return rc; }
    if (stride < ck_jpeg_enc_bound(h, w, sampling)) { *bad = 0; return refuse(msg, "output buffer of %zu bytes: too small for the headers", stride); }
    const CkEncGeom g = ck_enc_geom(h, w, sampling, restart_interval);
    if (optimise && g.blocks > CK_ENC_OPT_MAX_BLOCKS) { *bad = 0; return refuse(msg, "%lld blocks in a frame: optimised tables take 2^25", (long long)g.blocks); }
    const size_t cframe = (size_t)g.blocks * 64;
    const int64_t ftiles = g.nseg * g.seg_tiles;

    // histo and tables: the counters of every frame (a block that cannot be coded stops its walk there: size names it),
    // its four tables, its header
    const int ntab = sampling == CK_JPEG_GREY ? 2 : 4;
    std::vector<CkEncTables> own(optimise ? (size_t)n : 0);
    std::vector<uint8_t> headers((size_t)n * CK_ENC_HEADER_SLOT, 0);
    std::vector<uint32_t> hlen((size_t)n, 0);
    if (optimise) {
        uint8_t pre[CK_ENC_HEADER_SLOT], post[64], dht[4 * CK_ENC_DHT_SLOT];
        uint32_t pre_len, post_len, dht_len[4];
        ck_jpeg_enc_header_parts(quant, h, w, sampling, restart_interval, pre, &pre_len, post, &post_len);
        std::vector<uint32_t> freq(4 * 256);
        auto work = std::make_unique<CkEncTreeWork>();
        for (int f = 0; f < n; f++) {
            const int16_t* fc = coef + (size_t)f * cframe;
            std::fill(freq.begin(), freq.end(), 0u);
            for (int64_t k = 0; k < g.nseg; k++)
                for (int64_t t = 0; t < g.seg_tiles; t++) {
                    int64_t b0;
                    int cnt;
                    ck_enc_tile_blocks(g, k, t, &b0, &cnt);
                    for (int i = 0; i < cnt; i++) {
                        const int64_t b = b0 + i, pb = ck_enc_pred_block(g, b);
                        ck_enc_block_histo<CkEncPlainInc>(fc + ck_enc_place(g, b) * 64, pb < 0 ? 0 : fc[ck_enc_place(g, pb) * 64],
                                                          ck_enc_is_chroma(g, b), freq.data(), ZIGZAG);
                    }
                }
            memset(&own[f], 0, sizeof(CkEncTables));
            for (int t = 0; t < ntab; t++) {
                uint8_t bits[16], vals[256];
                int32_t count;
                for (int i = 0; i < 256; i++) work->freq[i] = freq[(size_t)t * 256 + i];
                ck_enc_optimal_table(work.get(), bits, vals, &count, CkEncSerial());
                ck_enc_fill(t & 1 ? &own[f].ac[t >> 1] : &own[f].dc[t >> 1], bits, vals);
                dht_len[t] = ck_enc_dht(dht + (size_t)t * CK_ENC_DHT_SLOT, t, bits, vals, count);
            }
            hlen[f] = ck_enc_header_len(pre_len, dht_len, ntab, post_len);
            if (hlen[f] > (uint32_t)CK_ENC_HEADER_SLOT) { *bad = f; return refuse(msg, "a header of %u bytes", hlen[f]); }
            for (uint32_t i = 0; i < hlen[f]; i++)
                headers[(size_t)f * CK_ENC_HEADER_SLOT + i] = ck_enc_header_byte(i, pre, pre_len, dht, dht_len, ntab, post);
        }
    } else {
        const uint32_t hl = (uint32_t)ck_jpeg_enc_headers(quant, h, w, sampling, restart_interval, headers.data());
        for (int f = 0; f < n; f++) {
            hlen[f] = hl;
            if (f) memcpy(headers.data() + (size_t)f * CK_ENC_HEADER_SLOT, headers.data(), hl);
        }
    }
    auto tables_of = [&](int f) -> const CkEncTables& { return optimise ? own[f] : ck_jpeg_enc_tables(); };

    // size: every block, the bit sums of the tiles, the lowest (frame, block) that cannot be coded
    std::vector<uint32_t> bits((size_t)n * g.blocks), tile_bits((size_t)n * ftiles, 0);
    uint64_t fail = ~(uint64_t)0;
    for (int f = 0; f < n; f++)
        for (int64_t k = 0; k < g.nseg; k++)
            for (int64_t t = 0; t < g.seg_tiles; t++) {
                int64_t b0;
                int cnt;
                ck_enc_tile_blocks(g, k, t, &b0, &cnt);
                for (int i = 0; i < cnt; i++) {
                    const int64_t b = b0 + i, pb = ck_enc_pred_block(g, b);
                    const int16_t* fc = coef + (size_t)f * cframe;
                    const int pred = pb < 0 ? 0 : fc[ck_enc_place(g, pb) * 64];
                    const uint32_t r = ck_enc_block_bits(fc + ck_enc_place(g, b) * 64, pred, ck_enc_is_chroma(g, b), &tables_of(f), ZIGZAG);
                    bits[(size_t)f * g.blocks + b] = r;
                    if (r & CK_ENC_FAIL) { const uint64_t key = ((uint64_t)f << 32) | (uint64_t)b; if (key < fail) fail = key; }
                    else tile_bits[((size_t)f * g.nseg + k) * g.seg_tiles + t] += r;
                }
            }
    if (fail != ~(uint64_t)0) {
        *bad = (int)(fail >> 32);
        const int64_t b = (int64_t)(fail & 0xffffffffu);
        ck_jpeg_enc_status_message(bits[(size_t)*bad * g.blocks + b], b / g.mcu_blocks, msg);
        return CK_ERR_ARG;
    }

    // scan: tiles in their segment, segments in their frame, frames in the bit buffer
    std::vector<uint64_t> tile_off((size_t)n * ftiles), seg_u0((size_t)n * (g.nseg + 1)), seg_bits((size_t)n * g.nseg), frame_u0((size_t)n + 1);
    uint64_t at = 0;
    for (int f = 0; f < n; f++) {
        uint64_t u = 0;
        for (int64_t k = 0; k < g.nseg; k++) {
            uint64_t sum = 0;
            for (int64_t t = 0; t < g.seg_tiles; t++) {
                const size_t ti = ((size_t)f * g.nseg + k) * g.seg_tiles + t;
                tile_off[ti] = sum;
                sum += tile_bits[ti];
            }
            seg_bits[(size_t)f * g.nseg + k] = sum;
            seg_u0[(size_t)f * (g.nseg + 1) + k] = u;
            u += ck_enc_seg_bytes(sum);
        }
        seg_u0[(size_t)f * (g.nseg + 1) + g.nseg] = u;
        frame_u0[f] = at;
        at += ck_enc_up(u, CK_ENC_TILE_BYTES);
    }
    frame_u0[n] = at;

    // put: every tile into words of its own, then into the zeroed buffer
    std::vector<uint32_t> buf(at / 4, 0), words(optimise ? CK_ENC_OPT_TILE_WORDS : CK_ENC_TILE_WORDS);
    for (int f = 0; f < n; f++)
        for (int64_t k = 0; k < g.nseg; k++)
            for (int64_t t = 0; t < g.seg_tiles; t++) {
                int64_t b0;
                int cnt;
                ck_enc_tile_blocks(g, k, t, &b0, &cnt);
                if (!cnt) continue;
                const size_t ti = ((size_t)f * g.nseg + k) * g.seg_tiles + t;
                const uint64_t sbits = seg_bits[(size_t)f * g.nseg + k];
                const uint64_t p0 = 8 * (frame_u0[f] + seg_u0[(size_t)f * (g.nseg + 1) + k]) + tile_off[ti];
                const bool last = tile_off[ti] + tile_bits[ti] == sbits;        // (a tile with blocks has bits)
                const uint32_t nbits = tile_bits[ti] + (last ? (uint32_t)ck_enc_seg_pad(sbits) : 0);
                const int nw = (int)(((p0 & 31) + nbits + 31) / 32);
                memset(words.data(), 0, (size_t)nw * sizeof(uint32_t));
                CkEncWordSink<CkEncPlainOr> sink{words.data(), (uint32_t)(p0 & 31)};
                for (int i = 0; i < cnt; i++) {
                    const int64_t b = b0 + i, pb = ck_enc_pred_block(g, b);
                    const int16_t* fc = coef + (size_t)f * cframe;
                    const int pred = pb < 0 ? 0 : fc[ck_enc_place(g, pb) * 64];
                    ck_enc_block_put(fc + ck_enc_place(g, b) * 64, pred, ck_enc_is_chroma(g, b), &tables_of(f), ZIGZAG, sink);
                }
                if (last && ck_enc_seg_pad(sbits)) sink.put((1u << ck_enc_seg_pad(sbits)) - 1, ck_enc_seg_pad(sbits));
                for (int i = 0; i < nw; i++) {
                    uint32_t* dst = buf.data() + (p0 >> 5) + i;
                    if (ck_enc_flush_how(i, nw)) *dst |= ck_enc_bswap(words[i]); else *dst = ck_enc_bswap(words[i]);
                }
            }

    // stuff: FF bytes of the byte tiles, their sums before a tile in its frame, then every byte to its place
    const uint8_t* bytes = (const uint8_t*)buf.data();
    for (int f = 0; f < n; f++) {
        const uint8_t* header = headers.data() + (size_t)f * CK_ENC_HEADER_SLOT;
        const size_t hl = hlen[f];
        const uint64_t* su = seg_u0.data() + (size_t)f * (g.nseg + 1);
        const uint64_t u = su[g.nseg];
        uint8_t* o = out + (size_t)f * stride;
        memcpy(o, header, hl);
        uint64_t ff = 0;
        for (uint64_t t0 = 0; t0 < u; t0 += CK_ENC_TILE_BYTES) {
            const uint64_t t1 = t0 + CK_ENC_TILE_BYTES < u ? t0 + CK_ENC_TILE_BYTES : u;
            uint64_t in_tile = 0;
            for (uint64_t i = t0; i < t1; i++) {
                const unsigned c = bytes[frame_u0[f] + i];
                ck_enc_emit(o + hl, o + stride, su, g.nseg, i, c, ff + in_tile);
                in_tile += c == 0xFF;
            }
            ff += in_tile;
        }
        len[f] = (size_t)ck_enc_stream_len(hl, u, ff, g.nseg);
    }
    return CK_OK;
}

int ck_jpeg_enc_staged(const int16_t* coef, const uint16_t* quant, int n, int h, int w, int sampling, int restart_interval,
                       uint8_t* out, size_t stride, size_t* len, int* bad, char* msg)
{
    return staged(coef, quant, n, h, w, sampling, restart_interval, out, stride, len, bad, msg, false);
}

int ck_jpeg_enc_staged_opt(const int16_t* coef, const uint16_t* quant, int n, int h, int w, int sampling, int restart_interval,
                           uint8_t* out, size_t stride, size_t* len, int* bad, char* msg)
{
    return staged(coef, quant, n, h, w, sampling, restart_interval, out, stride, len, bad, msg, true);
}

// ---- optimised tables on the host: one pass counts, one pass codes ----
int ck_jpeg_enc_histogram(const int16_t* coef, int h, int w, int sampling, int restart_interval, uint32_t* freq, char* msg)
{
    msg[0] = 0;
    if (!coef || !freq) return refuse(msg, "NULL pointer");
    if (h < 1 || w < 1 || h > 65535 || w > 65535) return refuse(msg, "bad JPEG frame size %dx%d: sides of 1 .. 65535", w, h);
    if (sampling < CK_JPEG_GREY || sampling > CK_JPEG_420) return refuse(msg, "bad JPEG sampling %d", sampling);
    if (restart_interval < 0 || restart_interval > 65535) return refuse(msg, "restart interval %d: 0 .. 65535 MCUs", restart_interval);
    const CkEncGeom g = ck_enc_geom(h, w, sampling, restart_interval);
    if (g.blocks > CK_ENC_OPT_MAX_BLOCKS) return refuse(msg, "%lld blocks in a frame: optimised tables take 2^25", (long long)g.blocks);
    memset(freq, 0, 4 * 256 * sizeof(uint32_t));
    for (int64_t b = 0; b < g.blocks; b++) {
        const int64_t pb = ck_enc_pred_block(g, b);
        const uint32_t st = ck_enc_block_histo<CkEncPlainInc>(coef + ck_enc_place(g, b) * 64, pb < 0 ? 0 : coef[ck_enc_place(g, pb) * 64],
                                                              ck_enc_is_chroma(g, b), freq, ZIGZAG);
        if (st) { ck_jpeg_enc_status_message(st, (long long)(b / g.mcu_blocks), msg); return CK_ERR_ARG; }
    }
    return CK_OK;
}

void ck_jpeg_enc_optimal_table(const uint32_t* freq, uint8_t* bits, uint8_t* vals, int32_t* count)
{
    auto work = std::make_unique<CkEncTreeWork>();
    for (int i = 0; i < 256; i++) work->freq[i] = freq[i];
    memset(vals, 0, 256);
    ck_enc_optimal_table(work.get(), bits, vals, count, CkEncSerial());
}

int ck_jpeg_enc_entropy_opt(const int16_t* coef, const uint16_t* quant, int h, int w, int sampling, int restart_interval,
                            uint8_t* out, size_t cap, size_t* len, char* msg)
{
    msg[0] = 0;
    if (len) *len = 0;
    if (const int rc = check_args(coef, quant, h, w, sampling, restart_interval, out, len, msg)) return rc;
    if (cap < HEADER_BOUND) return refuse(msg, "output buffer of %zu bytes: too small for the headers", cap);
    // the first pass: what is refused is refused before any table is made
    uint32_t freq[4 * 256];
    if (const int rc = ck_jpeg_enc_histogram(coef, h, w, sampling, restart_interval, freq, msg)) return rc;
    const CkEncGeom g = ck_enc_geom(h, w, sampling, restart_interval);
    const int ntab = sampling == CK_JPEG_GREY ? 2 : 4;
    auto T = std::make_unique<CkEncTables>();
    memset(T.get(), 0, sizeof(CkEncTables));
    Out o{out};
    header_front(o, quant, h, w, sampling);
    for (int t = 0; t < ntab; t++) {
        uint8_t bits[16], vals[256], dht[CK_ENC_DHT_SLOT];
        int32_t count;
        ck_jpeg_enc_optimal_table(freq + 256 * t, bits, vals, &count);
        ck_enc_fill(t & 1 ? &T->ac[t >> 1] : &T->dc[t >> 1], bits, vals);
        const uint32_t n = ck_enc_dht(dht, t, bits, vals, count);
        if ((size_t)(o.p - out) + n + 64 > HEADER_BOUND) return refuse(msg, "a header above %zu bytes", HEADER_BOUND);
        memcpy(o.p, dht, n);
        o.p += n;
    }
    header_back(o, sampling, restart_interval);

    // the second pass: the scan, with room for an MCU whose every code has 16 bits
    constexpr size_t OPT_BLOCK_BOUND = (size_t)(CK_ENC_OPT_BLOCK_BITS + 7) / 8 * 2;
    const uint8_t* const end = out + cap;
    BitWriter bw{o.p};
    for (int64_t mcu = 0; mcu < g.mcus; mcu++) {
        if ((size_t)(end - bw.p) < (size_t)g.mcu_blocks * OPT_BLOCK_BOUND + 8)
            return refuse(msg, "output buffer of %zu bytes: too small (MCU %lld of %lld)", cap, (long long)mcu, (long long)g.mcus);
        if (mcu && mcu % g.seg_mcus == 0) {
            bw.pad();
            *bw.p++ = 0xFF; *bw.p++ = (uint8_t)(0xD0 + ((mcu / g.seg_mcus - 1) & 7));
        }
        for (int j = 0; j < g.mcu_blocks; j++) {
            const int64_t b = mcu * g.mcu_blocks + j, pb = ck_enc_pred_block(g, b);
            ck_enc_block_put(coef + ck_enc_place(g, b) * 64, pb < 0 ? 0 : coef[ck_enc_place(g, pb) * 64], ck_enc_is_chroma(g, b), T.get(), ZIGZAG, bw);
        }
    }
    if ((size_t)(end - bw.p) < 4) return refuse(msg, "output buffer of %zu bytes: too small", cap);
    bw.pad();
    *bw.p++ = 0xFF; *bw.p++ = 0xD9;
    *len = (size_t)(bw.p - out);
    return CK_OK;
}
