// ck_jpeg.cpp -- marker parser and Huffman decoder of baseline JPEG (see ck_jpeg.h).  Plain C++: no HIP, no context.
#include "ck_jpeg.h"
#include "ck_jpeg_tables.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <new>

namespace {

int refuse(char* msg, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, CK_JPEG_MSG, fmt, ap);
    va_end(ap);
    return CK_ERR_DATA;
}

// bits[16] code counts per length, vals the symbols in code order (nvals of them available)
bool build_huff(CkHuff& t, const uint8_t* bits, const uint8_t* vals, int nvals)
{
    int total = 0;
    for (int l = 0; l < 16; l++) total += bits[l];
    if (total > 256 || total > nvals) return false;
    memset(t.look, 0, sizeof t.look);
    memset(t.vals, 0, sizeof t.vals);
    memcpy(t.vals, vals, (size_t)total);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; l++) {
        const int cnt = bits[l - 1];
        t.valoff[l] = k - code;
        if (code + cnt > (1 << l)) return false;                 // more codes than the length has
        for (int i = 0; i < cnt; i++, code++, k++) {
            if (l <= 9) {
                const int first = code << (9 - l);
                for (int j = 0; j < (1 << (9 - l)); j++) t.look[first + j] = (uint16_t)((l << 8) | vals[k]);
            }
        }
        t.maxcode[l] = cnt ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    t.present = true;
    return true;
}

inline unsigned be16(const uint8_t* p) { return ((unsigned)p[0] << 8) | p[1]; }

// the entropy-coded segment as a bit stream: byte unstuffing here, nothing is read at or beyond a marker or the end --
// zero bits come instead, and `fake` counts them, so a decoder that has used one of them knows it ran past the end
struct BitReader {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc = 0;
    int n = 0;             // bits in acc
    int fake = 0;          // how many of them (the lowest) are invented zeros

    void fill()
    {
        while (n <= 56) {
            unsigned b = 0;
            bool real = false;
            if (p < end) {
                if (*p != 0xFF) { b = *p++; real = true; }
                else if (p + 1 < end && p[1] == 0) { b = 0xFF; p += 2; real = true; }
            }
            acc = (acc << 8) | b;
            n += 8;
            if (!real || fake) fake += 8;
        }
    }
    inline unsigned peek(int k) { return (unsigned)((acc >> (n - k)) & ((1u << k) - 1)); }
    inline void drop(int k) { n -= k; }
    bool overrun() const { return n < fake; }
};

inline int decode_symbol(BitReader& br, const CkHuff& t)
{
    if (br.n < 16) br.fill();
    const unsigned e = t.look[br.peek(9)];
    if (e) { br.drop(e >> 8); return e & 255; }
    int l = 10;
    int code = (int)br.peek(10);
    while (l <= 16 && code > t.maxcode[l]) { l++; code = (int)br.peek(l <= 16 ? l : 16); }
    if (l > 16) return -1;
    br.drop(l);
    const int idx = code + t.valoff[l];
    return (idx < 0 || idx > 255) ? -1 : t.vals[idx];
}

inline int receive_extend(BitReader& br, int s)
{
    if (br.n < s) br.fill();
    const int v = (int)br.peek(s);
    br.drop(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

}  // namespace

int ck_jpeg_parse(const uint8_t* data, size_t len, CkJpegFrame* f, char* msg)
{
    msg[0] = 0;
    if (!data || !f) { snprintf(msg, CK_JPEG_MSG, "JPEG data is NULL"); return CK_ERR_ARG; }
    if (len < 4 || data[0] != 0xFF || data[1] != 0xD8) return refuse(msg, "not a JPEG stream: no SOI marker");
    uint16_t qt[4][64];
    bool have_qt[4] = {false, false, false, false};
    CkHuff* huff = new (std::nothrow) CkHuff[8];                 // [class * 4 + id]
    if (!huff) return refuse(msg, "out of memory");
    struct Free { CkHuff* p; ~Free() { delete[] p; } } free_huff{huff};
    bool any_dht = false, have_sof = false;
    int adobe_transform = -1, restart = 0;
    int comp_id[3] = {0, 0, 0}, comp_h[3] = {1, 1, 1}, comp_v[3] = {1, 1, 1}, comp_tq[3] = {0, 0, 0};
    int ncomp = 0, h = 0, w = 0;
    size_t p = 2;
    for (;;) {
        if (p + 4 > len) return refuse(msg, "the headers run past the end of the data");
        if (data[p] != 0xFF) return refuse(msg, "marker expected at byte %zu", p);
        const unsigned m = data[p + 1];
        if (m == 0xFF) { p++; continue; }                          // fill byte
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) { p += 2; continue; }      // stand-alone markers
        if (m == 0xD9) return refuse(msg, "EOI before any scan");
        const size_t ln = be16(data + p + 2);
        if (ln < 2 || p + 2 + ln > len) return refuse(msg, "segment 0x%02X runs past the end of the data", m);
        const uint8_t* s = data + p + 4;
        const size_t n = ln - 2;
        if (m == 0xDB) {
            size_t q = 0;
            while (q < n) {
                const int pq = s[q] >> 4, tq = s[q] & 15;
                if (pq > 1 || tq > 3) return refuse(msg, "bad quantisation table header");
                const size_t need = pq ? 128 : 64;
                if (q + 1 + need > n) return refuse(msg, "quantisation table runs past its segment");
                for (int i = 0; i < 64; i++) qt[tq][ZIGZAG[i]] = pq ? (uint16_t)be16(s + q + 1 + 2 * i) : s[q + 1 + i];
                have_qt[tq] = true;
                q += 1 + need;
            }
        } else if (m == 0xC0) {
            if (have_sof) return refuse(msg, "more than one frame header");
            if (n < 6) return refuse(msg, "frame header too short");
            if (s[0] != 8) return refuse(msg, "sample precision %d: only 8 bits", s[0]);
            h = (int)be16(s + 1); w = (int)be16(s + 3); ncomp = s[5];
            if (h == 0 || w == 0) return refuse(msg, "frame of %dx%d", w, h);
            if (ncomp != 1 && ncomp != 3) return refuse(msg, "%d components: only grey (1) and YCbCr (3)", ncomp);
            if (n < (size_t)(6 + 3 * ncomp)) return refuse(msg, "frame header too short");
            for (int c = 0; c < ncomp; c++) {
                comp_id[c] = s[6 + 3 * c]; comp_h[c] = s[7 + 3 * c] >> 4; comp_v[c] = s[7 + 3 * c] & 15; comp_tq[c] = s[8 + 3 * c];
                if (comp_tq[c] > 3) return refuse(msg, "bad quantisation table selector");
                if (comp_h[c] < 1 || comp_h[c] > 4 || comp_v[c] < 1 || comp_v[c] > 4) return refuse(msg, "bad sampling factors");
            }
            have_sof = true;
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            return refuse(msg, "frame type SOF%d (extended, progressive, lossless or arithmetic): only baseline SOF0", (int)m - 0xC0);
        } else if (m == 0xCC) {
            return refuse(msg, "arithmetic coding conditioning: only Huffman-coded baseline");
        } else if (m == 0xC4) {
            size_t q = 0;
            while (q < n) {
                if (q + 17 > n) return refuse(msg, "Huffman table runs past its segment");
                const int tc = s[q] >> 4, th = s[q] & 15;
                if (tc > 1 || th > 3) return refuse(msg, "bad Huffman table header");
                int total = 0;
                for (int i = 0; i < 16; i++) total += s[q + 1 + i];
                if (q + 17 + (size_t)total > n) return refuse(msg, "Huffman table runs past its segment");
                if (!build_huff(huff[tc * 4 + th], s + q + 1, s + q + 17, total)) return refuse(msg, "bad Huffman table");
                any_dht = true;
                q += 17 + (size_t)total;
            }
        } else if (m == 0xDD) {
            if (n < 2) return refuse(msg, "restart interval segment too short");
            restart = (int)be16(s);
        } else if (m == 0xEE) {
            if (n >= 12 && memcmp(s, "Adobe", 5) == 0) adobe_transform = s[11];
        } else if (m == 0xDA) {
            if (!have_sof) return refuse(msg, "scan before the frame header");
            if (n < 1 || n < (size_t)(4 + 2 * s[0])) return refuse(msg, "scan header too short");
            if (s[0] != ncomp) return refuse(msg, "a scan of %d of the %d components: only one interleaved scan", s[0], ncomp);
            if (ncomp == 3 && adobe_transform == 0) return refuse(msg, "Adobe APP14 transform 0 (RGB, not YCbCr)");
            if (ncomp == 3) {
                const bool chroma11 = comp_h[1] == 1 && comp_v[1] == 1 && comp_h[2] == 1 && comp_v[2] == 1;
                const int hv = comp_h[0] * 16 + comp_v[0];
                if (!chroma11 || (hv != 0x11 && hv != 0x21 && hv != 0x22))
                    return refuse(msg, "sampling %dx%d %dx%d %dx%d: only luma 1x1, 2x1, 2x2 with chroma 1x1", comp_h[0], comp_v[0],
                                  comp_h[1], comp_v[1], comp_h[2], comp_v[2]);
                f->info.sampling = hv == 0x11 ? CK_JPEG_444 : (hv == 0x21 ? CK_JPEG_422 : CK_JPEG_420);
            } else {
                f->info.sampling = CK_JPEG_GREY;
            }
            if (!any_dht) {
                build_huff(huff[0], STD_DC_LUMA_BITS, STD_DC_VALS, 12);
                build_huff(huff[1], STD_DC_CHROMA_BITS, STD_DC_VALS, 12);
                build_huff(huff[4], STD_AC_LUMA_BITS, STD_AC_LUMA_VALS, 162);
                build_huff(huff[5], STD_AC_CHROMA_BITS, STD_AC_CHROMA_VALS, 162);
            }
            for (int c = 0; c < ncomp; c++) {
                if (s[1 + 2 * c] != comp_id[c]) return refuse(msg, "scan components are not the frame's, in order");
                const int td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
                if (td > 3 || ta > 3 || !huff[td].present || !huff[4 + ta].present) return refuse(msg, "missing Huffman table");
                if (!have_qt[comp_tq[c]]) return refuse(msg, "missing quantisation table");
                f->dc[c] = huff[td];
                f->ac[c] = huff[4 + ta];
                memcpy(f->quant[c], qt[comp_tq[c]], sizeof qt[0]);
            }
            for (int c = ncomp; c < 3; c++) memset(f->quant[c], 0, sizeof f->quant[c]);
            const uint8_t* tail = s + 1 + 2 * ncomp;
            if (tail[0] != 0 || tail[1] != 63 || tail[2] != 0) return refuse(msg, "spectral selection / approximation: only sequential scans");
            f->ncomp = ncomp;
            f->hs = ck_jpeg_luma_h(f->info.sampling);
            f->vs = ck_jpeg_luma_v(f->info.sampling);
            f->mcux = (w + 8 * f->hs - 1) / (8 * f->hs);
            f->mcuy = (h + 8 * f->vs - 1) / (8 * f->vs);
            f->info.h = h; f->info.w = w; f->info.restart_interval = restart;
            const long long blocks = ck_jpeg_blocks(h, w, f->info.sampling);
            if (blocks > 0x7fffffffLL / 64) return refuse(msg, "frame too large");
            f->info.blocks = (int32_t)blocks;
            f->scan = p + 2 + ln;
            return CK_OK;
        }
        p += 2 + ln;
    }
}

int ck_jpeg_entropy(const uint8_t* data, size_t len, const CkJpegFrame& f, int16_t* coef, char* msg)
{
    msg[0] = 0;
    if (f.scan > len) return refuse(msg, "the scan starts past the end of the data");
    memset(coef, 0, (size_t)f.info.blocks * 64 * sizeof(int16_t));
    // where each component's blocks start, and how wide its grid is
    const int lw = f.mcux * f.hs, lh = f.mcuy * f.vs;
    size_t base[3] = {0, (size_t)lw * lh, (size_t)lw * lh + (size_t)f.mcux * f.mcuy};
    BitReader br{data + f.scan, data + len};
    const long long total = (long long)f.mcux * f.mcuy;
    const int ri = f.info.restart_interval;
    int pred[3] = {0, 0, 0};
    int expect = 0, since = 0;
    for (long long mcu = 0; mcu < total; mcu++) {
        if (ri && since == ri) {
            // the rest of the buffered bits is padding; the marker must be the next thing in the data
            if (br.overrun()) return refuse(msg, "the entropy-coded data ran past its end (MCU %lld)", mcu);
            br.acc = 0; br.n = 0; br.fake = 0;
            while (br.p + 1 < br.end && br.p[0] == 0xFF && br.p[1] == 0xFF) br.p++;
            if (br.p + 2 > br.end || br.p[0] != 0xFF || br.p[1] != 0xD0 + expect)
                return refuse(msg, "restart marker RST%d missing or out of order before MCU %lld", expect, mcu);
            br.p += 2;
            expect = (expect + 1) & 7;
            since = 0;
            pred[0] = pred[1] = pred[2] = 0;
        }
        since++;
        const int my = (int)(mcu / f.mcux), mx = (int)(mcu % f.mcux);
        for (int c = 0; c < f.ncomp; c++) {
            const int bh = (c == 0 && f.ncomp == 3) ? f.hs : 1, bv = (c == 0 && f.ncomp == 3) ? f.vs : 1;
            const int gw = (c == 0) ? lw : f.mcux;
            for (int v = 0; v < bv; v++)
                for (int u = 0; u < bh; u++) {
                    int16_t* blk = coef + (base[c] + (size_t)(my * bv + v) * gw + (size_t)(mx * bh + u)) * 64;
                    int s = decode_symbol(br, f.dc[c]);
                    if (s < 0) return refuse(msg, br.overrun() ? "the entropy-coded data ran past its end (MCU %lld)" : "unknown Huffman code (MCU %lld)", mcu);
                    if (s > 11) return refuse(msg, "DC difference of %d bits (MCU %lld)", s, mcu);
                    if (s) pred[c] += receive_extend(br, s);
                    if (pred[c] < -32768 || pred[c] > 32767) return refuse(msg, "DC value out of range (MCU %lld)", mcu);
                    blk[0] = (int16_t)pred[c];
                    for (int k = 1; k < 64;) {
                        const int rs = decode_symbol(br, f.ac[c]);
                        if (rs < 0) return refuse(msg, br.overrun() ? "the entropy-coded data ran past its end (MCU %lld)" : "unknown Huffman code (MCU %lld)", mcu);
                        const int r = rs >> 4;
                        s = rs & 15;
                        if (s == 0) {
                            if (r != 15) break;
                            k += 16;
                            continue;
                        }
                        k += r;
                        if (k > 63) return refuse(msg, "coefficient index above 63 (MCU %lld)", mcu);
                        blk[ZIGZAG[k]] = (int16_t)receive_extend(br, s);
                        k++;
                    }
                    if (br.overrun()) return refuse(msg, "the entropy-coded data ran past its end (MCU %lld)", mcu);
                }
        }
    }
    return CK_OK;
}
