// ck_jpeg_enc.cpp -- quant tables, JFIF headers and the Huffman coder of baseline JPEG (see ck_jpeg_enc.h), in libjpeg's
// order and with its choices, so that the stream equals what its default compressor writes.  Plain C++: no HIP, no context.
#include "ck_jpeg_enc.h"
#include "ck_jpeg_tables.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

namespace {

// Annex K.1 and K.2, natural order
const uint8_t BASE_LUMA[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                               69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55, 64,
                               81, 104, 113, 92, 49, 64, 78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
const uint8_t BASE_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                 99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

constexpr size_t HEADER_BOUND = 1024;        // SOI, APP0, 2 DQT, SOF0, 4 DHT, DRI, SOS, EOI: 629 bytes
constexpr size_t BLOCK_BOUND = 64 * 26 / 8 * 2;

int refuse(char* msg, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, CK_JPEG_MSG, fmt, ap);
    va_end(ap);
    return CK_ERR_ARG;
}

// symbol -> code and length (0: the table has no such symbol)
struct EncHuff {
    uint16_t code[256];
    uint8_t len[256];
    EncHuff(const uint8_t* bits, const uint8_t* vals)
    {
        memset(code, 0, sizeof code);
        memset(len, 0, sizeof len);
        int c = 0, k = 0;
        for (int l = 1; l <= 16; l++) {
            for (int i = 0; i < bits[l - 1]; i++, c++, k++) { code[vals[k]] = (uint16_t)c; len[vals[k]] = (uint8_t)l; }
            c <<= 1;
        }
    }
};

struct Tables {
    EncHuff dc[2] = {EncHuff(STD_DC_LUMA_BITS, STD_DC_VALS), EncHuff(STD_DC_CHROMA_BITS, STD_DC_VALS)};
    EncHuff ac[2] = {EncHuff(STD_AC_LUMA_BITS, STD_AC_LUMA_VALS), EncHuff(STD_AC_CHROMA_BITS, STD_AC_CHROMA_VALS)};
};
const Tables& tables()
{
    static const Tables t;
    return t;
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

inline int bit_size(int v)
{
    unsigned a = (unsigned)(v < 0 ? -v : v);
    int s = 0;
    while (a) { s++; a >>= 1; }
    return s;
}

}  // namespace

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

int ck_jpeg_enc_entropy(const int16_t* coef, const uint16_t* quant, int h, int w, int sampling, int restart_interval,
                        uint8_t* out, size_t cap, size_t* len, char* msg)
{
    msg[0] = 0;
    if (len) *len = 0;
    if (!coef || !quant || !out || !len) return refuse(msg, "NULL pointer");
    if (h < 1 || w < 1 || h > 65535 || w > 65535) return refuse(msg, "bad JPEG frame size %dx%d: sides of 1 .. 65535", w, h);
    if (sampling < CK_JPEG_GREY || sampling > CK_JPEG_420) return refuse(msg, "bad JPEG sampling %d", sampling);
    if (restart_interval < 0 || restart_interval > 65535) return refuse(msg, "restart interval %d: 0 .. 65535 MCUs", restart_interval);
    const bool grey = sampling == CK_JPEG_GREY;
    const int ncomp = grey ? 1 : 3;
    for (int i = 0; i < (grey ? 64 : 192); i++)
        if (quant[i] < 1 || quant[i] > 255) return refuse(msg, "quant entry %d is %d: baseline tables hold 1 .. 255", i, quant[i]);
    if (!grey && memcmp(quant + 64, quant + 128, 64 * sizeof(uint16_t)) != 0) return refuse(msg, "Cb and Cr share one quant table");
    if (cap < HEADER_BOUND) return refuse(msg, "output buffer of %zu bytes: too small for the headers", cap);

    // ---- headers, in libjpeg's order ----
    Out o{out};
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
    if (restart_interval) { o.segment(0xDD, 2); o.be16((unsigned)restart_interval); }
    o.segment(0xDA, 4 + 2 * (size_t)ncomp);
    o.byte((unsigned)ncomp);
    for (int c = 0; c < ncomp; c++) { o.byte((unsigned)c + 1); o.byte(c ? 0x11u : 0x00u); }
    o.byte(0); o.byte(63); o.byte(0);

    // ---- the scan ----
    const Tables& T = tables();
    const int mcux = (w + 8 * hs - 1) / (8 * hs), mcuy = (h + 8 * vs - 1) / (8 * vs);
    const int lw = mcux * hs, lh = mcuy * vs;
    const size_t base[3] = {0, (size_t)lw * lh, (size_t)lw * lh + (size_t)mcux * mcuy};
    const uint8_t* const end = out + cap;
    BitWriter bw{o.p};
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
            const EncHuff& dc = T.dc[c ? 1 : 0];
            const EncHuff& ac = T.ac[c ? 1 : 0];
            for (int v = 0; v < bv; v++)
                for (int u = 0; u < bh; u++) {
                    const int16_t* blk = coef + (base[c] + (size_t)(my * bv + v) * gw + (size_t)(mx * bh + u)) * 64;
                    const int diff = (int)blk[0] - pred[c];
                    pred[c] = blk[0];
                    int s = bit_size(diff);
                    if (s > 11) return refuse(msg, "DC difference of %d bits (MCU %lld): baseline JPEG has 11", s, mcu);
                    bw.put(dc.code[s], dc.len[s]);
                    if (s) bw.put((uint32_t)(diff < 0 ? diff - 1 : diff), s);
                    int run = 0;
                    for (int k = 1; k < 64; k++) {
                        const int val = blk[ZIGZAG[k]];
                        if (val == 0) { run++; continue; }
                        for (; run > 15; run -= 16) bw.put(ac.code[0xF0], ac.len[0xF0]);
                        s = bit_size(val);
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
