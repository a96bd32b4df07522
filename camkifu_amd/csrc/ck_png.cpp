// ck_png.cpp -- the host half of the PNG reader and writer: see ck_png.h.  Plain C++ (tools/sanitize/png_fuzz.cpp links it alone).
#include "ck_png.h"
#include "ck_png_stage.h"
#include "ck_png_inflate_stage.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

namespace {

int refuse(char* msg, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, CK_PNG_MSG, fmt, ap);
    va_end(ap);
    return CK_ERR_DATA;
}

uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
void put_be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

struct CrcTables {
    uint32_t t[8][256];
    CrcTables()
    {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
            t[0][i] = c;
        }
        for (int k = 1; k < 8; k++)
            for (int i = 0; i < 256; i++) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 255];
    }
};

// ---- inflate ----
constexpr int FAST = 10;                                     // codes up to this many bits decode in one look-up
struct Huff {
    uint16_t fast[1 << FAST];                                // symbol << 4 | bits; 0: a longer code, or none
    uint16_t count[16];                                      // codes of each length
    uint16_t symbol[288];                                    // symbols by (length, symbol)
};
enum { KIND_CODES = 0, KIND_LENS = 1, KIND_DISTS = 2 };

// zlib's inflate_table verdict: an over-subscribed set is an error; so is an incomplete one, except a literal/length or
// distance set of one code of one bit; no code at all is an error for the code-length code and a table without symbols else
const char* huff_build(Huff& h, const uint8_t* lens, int n, int kind)
{
    memset(&h, 0, sizeof h);
    for (int i = 0; i < n; i++) h.count[lens[i]]++;
    h.count[0] = 0;
    int max = 15;
    while (max > 0 && !h.count[max]) max--;
    if (max == 0) return kind == KIND_CODES ? "no code-length code" : nullptr;
    int left = 1;
    for (int l = 1; l <= 15; l++) {
        left = (left << 1) - h.count[l];
        if (left < 0) return "over-subscribed code set";
    }
    if (left > 0 && (kind == KIND_CODES || max != 1)) return "incomplete code set";
    uint16_t offs[16];
    offs[1] = 0;
    for (int l = 1; l < 15; l++) offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
    for (int i = 0; i < n; i++)
        if (lens[i]) h.symbol[offs[lens[i]]++] = (uint16_t)i;
    uint32_t code = 0;
    int at = 0;
    for (int l = 1; l <= FAST; l++) {
        for (int k = 0; k < h.count[l]; k++, code++, at++) {
            const uint32_t rev = ck_png_reverse(code, l);
            for (uint32_t x = rev; x < (1u << FAST); x += 1u << l) h.fast[x] = (uint16_t)(h.symbol[at] << 4 | l);
        }
        code <<= 1;
    }
    return nullptr;
}

struct BitIn {
    const uint8_t *p, *end;
    uint64_t acc = 0;
    int cnt = 0;
    void refill()
    {
        while (cnt <= 56 && p < end) { acc |= (uint64_t)*p++ << cnt; cnt += 8; }
    }
    bool take(int n, uint32_t* v)                            // n <= 16
    {
        if (cnt < n) { refill(); if (cnt < n) return false; }
        *v = (uint32_t)acc & ((1u << n) - 1);
        acc >>= n; cnt -= n;
        return true;
    }
    // the next symbol, -1 for bits that are no code or a code the input ends in (bits past the end read as zeros: a code
    // that needs more than there are is never one of the shorter ones, a prefix code has no such pair)
    int decode(const Huff& h)
    {
        refill();
        const uint32_t e = h.fast[acc & ((1u << FAST) - 1)];
        if (e) {
            const int l = (int)(e & 15);
            if (l > cnt) return -1;
            acc >>= l; cnt -= l;
            return (int)(e >> 4);
        }
        int code = 0, first = 0, index = 0;
        uint64_t a = acc;
        for (int l = 1; l <= 15; l++) {
            if (l > cnt) return -1;
            code |= (int)(a & 1);
            a >>= 1;
            const int c = h.count[l];
            if (code - c < first) { acc >>= l; cnt -= l; return h.symbol[index + (code - first)]; }
            index += c; first += c; first <<= 1; code <<= 1;
        }
        return -1;
    }
};

struct FixedTables {
    Huff lit, dist;
    FixedTables()
    {
        uint8_t l[288];
        for (int i = 0; i < 288; i++) l[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
        huff_build(lit, l, 288, KIND_LENS);
        for (int i = 0; i < 32; i++) l[i] = 5;
        huff_build(dist, l, 32, KIND_DISTS);
    }
};

const uint16_t LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
const uint8_t LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
const uint16_t DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
const uint8_t DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
const uint8_t CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// what inflate writes: the first cap bytes are kept, the rest only as far back as a distance can reach
struct Sink {
    uint8_t* out;
    size_t cap, n = 0;
    std::vector<uint8_t> ring;                               // bytes from cap on, at their position mod 32768
    uint32_t ta = 0, tb = 0;                                 // the Adler-32 state once bytes are dropped
    void byte(uint8_t b)
    {
        if (n < cap) { out[n++] = b; return; }
        if (ring.empty()) {
            ring.assign(32768, 0);
            const uint32_t ad = ck_png_adler32(out, cap);
            ta = ad & 0xffff; tb = ad >> 16;
        }
        ring[n++ & 32767] = b;
        ta = (ta + b) % CK_PNG_ADLER; tb = (tb + ta) % CK_PNG_ADLER;
    }
    uint8_t at(size_t pos) const { return pos < cap ? out[pos] : ring[pos & 32767]; }
    void copy(size_t dist, int len)
    {
        if (n + (size_t)len <= cap) {
            uint8_t* d = out + n;
            const uint8_t* s = d - dist;
            for (int i = 0; i < len; i++) d[i] = s[i];
            n += (size_t)len;
            return;
        }
        for (int i = 0; i < len; i++) byte(at(n - dist));
    }
    uint32_t adler() const { return ring.empty() ? ck_png_adler32(out, n) : tb << 16 | ta; }
};

const char* inflate_codes(BitIn& in, Sink& o, const Huff& lit, const Huff& dist)
{
    for (;;) {
        int sym = in.decode(lit);                            // (one refill holds a whole length / distance pair: 15 + 5 + 15 + 13 bits)
        if (sym < 0) return "invalid literal/length code or the data ends inside one";
        if (sym < 256) { o.byte((uint8_t)sym); continue; }
        if (sym == 256) return nullptr;
        sym -= 257;
        if (sym >= 29) return "invalid literal/length code";
        uint32_t extra = 0;
        if (!in.take(LEN_EXTRA[sym], &extra)) return "the data ends inside a length";
        const int len = LEN_BASE[sym] + (int)extra;
        const int ds = in.decode(dist);
        if (ds < 0) return "invalid distance code or the data ends inside one";
        if (ds >= 30) return "invalid distance code";
        if (!in.take(DIST_EXTRA[ds], &extra)) return "the data ends inside a distance";
        const size_t d = DIST_BASE[ds] + (size_t)extra;
        if (d > o.n) return "a distance beyond the bytes produced so far";
        o.copy(d, len);
    }
}

}  // namespace

uint32_t ck_png_crc32(const uint8_t* p, size_t n, uint32_t crc)
{
    static const CrcTables T;
    uint32_t c = ~crc;
    for (; n >= 8; n -= 8, p += 8) {
        uint32_t lo, hi;
        memcpy(&lo, p, 4);
        memcpy(&hi, p + 4, 4);
        lo ^= c;
        c = T.t[7][lo & 255] ^ T.t[6][(lo >> 8) & 255] ^ T.t[5][(lo >> 16) & 255] ^ T.t[4][lo >> 24] ^
            T.t[3][hi & 255] ^ T.t[2][(hi >> 8) & 255] ^ T.t[1][(hi >> 16) & 255] ^ T.t[0][hi >> 24];
    }
    for (; n; n--, p++) c = T.t[0][(c ^ *p) & 255] ^ (c >> 8);
    return ~c;
}

uint32_t ck_png_adler32(const uint8_t* p, size_t n, uint32_t adler)
{
    uint32_t a = adler & 0xffff, b = adler >> 16;
    while (n) {
        const size_t k = n < 5552 ? n : 5552;                // the most bytes before b can pass 2^32
        for (size_t i = 0; i < k; i++) { a += p[i]; b += a; }
        a %= CK_PNG_ADLER; b %= CK_PNG_ADLER;
        p += k; n -= k;
    }
    return b << 16 | a;
}

int ck_png_unzip(const uint8_t* z, size_t zlen, uint8_t* out, size_t cap, size_t* total, char* msg)
{
    *total = 0;
    if (!z || zlen < 2) return refuse(msg, "zlib stream of %zu bytes", zlen);
    if (((uint32_t)z[0] << 8 | z[1]) % 31) return refuse(msg, "zlib header: the check bits do not hold");
    if ((z[0] & 15) != 8) return refuse(msg, "zlib header: compression method %d, not deflate", z[0] & 15);
    if ((z[0] >> 4) > 7) return refuse(msg, "zlib header: window size code %d", z[0] >> 4);
    if (z[1] & 0x20) return refuse(msg, "zlib header: a preset dictionary");
    static const FixedTables fixed;
    BitIn in;
    in.p = z + 2; in.end = z + zlen;
    Sink o;
    o.out = out; o.cap = out ? cap : 0;
    Huff cl, lit, dist;
    for (uint32_t last = 0; !last;) {
        uint32_t type = 0;
        if (!in.take(1, &last) || !in.take(2, &type)) return refuse(msg, "the deflate data ends before a block header");
        if (type == 3) return refuse(msg, "deflate block type 3");
        if (type == 0) {
            uint32_t drop, len, nlen;
            in.take(in.cnt & 7, &drop);
            if (!in.take(16, &len) || !in.take(16, &nlen)) return refuse(msg, "the data ends inside a stored block's lengths");
            if ((len ^ 0xffffu) != nlen) return refuse(msg, "stored block: LEN %u and NLEN %u do not agree", len, nlen);
            in.p -= in.cnt / 8;                              // whole bytes read ahead go back
            in.acc = 0; in.cnt = 0;
            if ((size_t)(in.end - in.p) < len) return refuse(msg, "the data ends inside a stored block");
            if (o.n + len <= o.cap) { if (len) memcpy(o.out + o.n, in.p, len); o.n += len; }
            else for (uint32_t i = 0; i < len; i++) o.byte(in.p[i]);
            in.p += len;
            continue;
        }
        const char* why;
        if (type == 1) {
            why = inflate_codes(in, o, fixed.lit, fixed.dist);
        } else {
            uint32_t nlen, ndist, ncode;
            if (!in.take(5, &nlen) || !in.take(5, &ndist) || !in.take(4, &ncode)) return refuse(msg, "the data ends inside a dynamic block's header");
            nlen += 257; ndist += 1; ncode += 4;
            if (nlen > 286 || ndist > 30) return refuse(msg, "dynamic block: %u literal/length codes, %u distance codes", nlen, ndist);
            uint8_t lens[320];
            memset(lens, 0, sizeof lens);
            for (uint32_t i = 0; i < ncode; i++) {
                uint32_t v;
                if (!in.take(3, &v)) return refuse(msg, "the data ends inside the code-length code");
                lens[CL_ORDER[i]] = (uint8_t)v;
            }
            if ((why = huff_build(cl, lens, 19, KIND_CODES)) != nullptr) return refuse(msg, "code-length code: %s", why);
            memset(lens, 0, sizeof lens);
            for (uint32_t have = 0; have < nlen + ndist;) {
                const int sym = in.decode(cl);
                if (sym < 0) return refuse(msg, "invalid code-length code or the data ends inside one");
                if (sym < 16) { lens[have++] = (uint8_t)sym; continue; }
                uint32_t rep = 0;
                uint8_t prev = 0;
                if (sym == 16) {
                    if (have == 0) return refuse(msg, "code-length repeat with nothing before it");
                    prev = lens[have - 1];
                    if (!in.take(2, &rep)) return refuse(msg, "the data ends inside a code-length repeat");
                    rep += 3;
                } else if (sym == 17) {
                    if (!in.take(3, &rep)) return refuse(msg, "the data ends inside a code-length repeat");
                    rep += 3;
                } else {
                    if (!in.take(7, &rep)) return refuse(msg, "the data ends inside a code-length repeat");
                    rep += 11;
                }
                if (have + rep > nlen + ndist) return refuse(msg, "code-length repeat past the last code");
                while (rep--) lens[have++] = prev;
            }
            if (lens[256] == 0) return refuse(msg, "dynamic block without an end-of-block code");
            if ((why = huff_build(lit, lens, (int)nlen, KIND_LENS)) != nullptr) return refuse(msg, "literal/length code: %s", why);
            if ((why = huff_build(dist, lens + nlen, (int)ndist, KIND_DISTS)) != nullptr) return refuse(msg, "distance code: %s", why);
            why = inflate_codes(in, o, lit, dist);
        }
        if (why) return refuse(msg, "%s (after %zu bytes)", why, o.n);
    }
    in.cnt -= in.cnt & 7;
    const uint8_t* tail = in.p - in.cnt / 8;
    if (in.end - tail < 4) return refuse(msg, "the zlib stream ends before its Adler-32");
    const uint32_t want = be32(tail), got = o.adler();
    if (want != got) return refuse(msg, "Adler-32 %08x where the data has %08x", want, got);
    *total = o.n;
    return CK_OK;
}

int ck_png_walk(const uint8_t* data, size_t len, CkPngHead* hd, char* msg)
{
    static const uint8_t SIG[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    if (!data || !hd) { snprintf(msg, CK_PNG_MSG, "NULL pointer"); return CK_ERR_ARG; }
    if (len < 8 || memcmp(data, SIG, 8) != 0) return refuse(msg, "not a PNG file: bad signature");
    *hd = CkPngHead();
    size_t at = 8, idat_chunks = 0, idat_bytes = 0;
    const uint8_t* first_idat = nullptr;
    bool have_ihdr = false, ended = false, idat_closed = false, seen_plte = false;
    // pass 1: every chunk's bounds and CRC, IHDR, PLTE; pass 2 (below) joins the IDAT chunks when there are several
    while (!ended) {
        if (len - at < 12) return refuse(msg, "%s", at == len ? "the file ends without IEND" : "the file ends inside a chunk header");
        const uint32_t clen = be32(data + at);
        const uint8_t* type = data + at + 4;
        char name[5] = {0, 0, 0, 0, 0};
        for (int i = 0; i < 4; i++) name[i] = type[i] >= 32 && type[i] < 127 ? (char)type[i] : '?';
        if (clen > 0x7fffffffu || (size_t)clen > len - at - 12) return refuse(msg, "chunk %s of %u bytes runs past the end of the file", name, clen);
        const uint8_t* body = type + 4;
        if (ck_png_crc32(type, 4 + (size_t)clen) != be32(body + clen)) return refuse(msg, "chunk %s: bad CRC", name);
        const bool is = memcmp(type, "IHDR", 4) == 0;
        if (!have_ihdr && !is) return refuse(msg, "IHDR is missing: the first chunk is %s", name);
        if (is) {
            if (have_ihdr) return refuse(msg, "a second IHDR");
            if (clen != 13) return refuse(msg, "IHDR of %u bytes", clen);
            const uint32_t w = be32(body), h = be32(body + 4);
            const int depth = body[8], ct = body[9];
            if (w == 0 || h == 0) return refuse(msg, "zero %s", w == 0 ? "width" : "height");
            if (w > (uint32_t)CK_PNG_MAX_SIDE || h > (uint32_t)CK_PNG_MAX_SIDE || (long long)w * h > CK_PNG_MAX_PIXELS)
                return refuse(msg, "%ux%u: above %d a side or 2^28 pixels", w, h, CK_PNG_MAX_SIDE);
            const int channels = ct == 0 ? 1 : ct == 2 ? 3 : ct == 3 ? 1 : ct == 4 ? 2 : ct == 6 ? 4 : 0;
            if (!channels) return refuse(msg, "colour type %d", ct);
            const bool depth_ok = ct == 0 ? (depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16)
                                : ct == 3 ? (depth == 1 || depth == 2 || depth == 4 || depth == 8) : (depth == 8 || depth == 16);
            if (!depth_ok) return refuse(msg, "bit depth %d with colour type %d", depth, ct);
            if (body[10] != 0) return refuse(msg, "compression method %d", body[10]);
            if (body[11] != 0) return refuse(msg, "filter method %d", body[11]);
            if (body[12] == 1) return refuse(msg, "Adam7 interlace is not read");
            if (body[12] != 0) return refuse(msg, "interlace method %d", body[12]);
            hd->w = (int32_t)w; hd->h = (int32_t)h; hd->bit_depth = depth; hd->color_type = ct; hd->channels = channels;
            hd->bpp = channels * depth >= 8 ? channels * depth / 8 : 1;
            hd->rowbytes = ((int64_t)w * channels * depth + 7) / 8;
            have_ihdr = true;
        } else if (memcmp(type, "PLTE", 4) == 0) {
            // libpng's rules: one PLTE, in front of IDAT; in a grey image it is passed over; entries beyond 2^depth are dropped
            if (clen == 0 || clen % 3 || clen > 768) return refuse(msg, "PLTE of %u bytes", clen);
            if (idat_chunks) return refuse(msg, "PLTE behind IDAT");
            if (seen_plte) return refuse(msg, "a second PLTE");
            seen_plte = true;
            if (hd->color_type != 0 && hd->color_type != 4) {
                const uint32_t most = hd->color_type == 3 ? 1u << hd->bit_depth : 256u;
                hd->palette_n = (int32_t)(clen / 3 < most ? clen / 3 : most);
                memcpy(hd->palette, body, (size_t)hd->palette_n * 3);
            }
        } else if (memcmp(type, "IDAT", 4) == 0) {
            if (idat_closed) return refuse(msg, "IDAT chunks are not consecutive");
            if (!idat_chunks) first_idat = body;
            idat_chunks++;
            idat_bytes += clen;
        } else if (memcmp(type, "IEND", 4) == 0) {
            ended = true;
        } else if (!(type[0] & 0x20)) {
            return refuse(msg, "unknown critical chunk %s", name);
        }
        if (idat_chunks && memcmp(type, "IDAT", 4) != 0) idat_closed = true;
        at += 12 + (size_t)clen;
    }
    if (!idat_chunks) return refuse(msg, "no IDAT chunk");
    if (hd->color_type == 3 && !hd->palette_n) return refuse(msg, "colour type 3 without PLTE");
    if (idat_chunks == 1) {
        hd->z = first_idat; hd->zlen = idat_bytes;
        return CK_OK;
    }
    hd->joined.reserve(idat_bytes);
    for (at = 8; at + 12 <= len;) {
        const uint32_t clen = be32(data + at);
        if (memcmp(data + at + 4, "IDAT", 4) == 0) hd->joined.insert(hd->joined.end(), data + at + 8, data + at + 8 + clen);
        if (memcmp(data + at + 4, "IEND", 4) == 0) break;
        at += 12 + (size_t)clen;
    }
    hd->z = hd->joined.data(); hd->zlen = hd->joined.size();
    return CK_OK;
}

int ck_png_rows(const CkPngHead& hd, uint8_t* rows, char* msg)
{
    const size_t need = hd.inflated(), pitch = (size_t)(1 + hd.rowbytes);
    size_t total = 0;
    const int rc = ck_png_unzip(hd.z, hd.zlen, rows, need, &total, msg);
    if (rc != CK_OK) return rc;
    if (total < need) return refuse(msg, "IDAT data too short: %zu bytes where %d rows of 1 + %lld need %zu", total, hd.h, (long long)hd.rowbytes, need);
    for (int y = 0; y < hd.h; y++)
        if (rows[(size_t)y * pitch] > 4) return refuse(msg, "row %d: filter type %d", y, rows[(size_t)y * pitch]);
    return CK_OK;
}

// ---- the staged inflate: the steps of ck_png_inflate_stage.h in plain loops, in the kernel's order ----
void ck_png_inflate_message(const CkInfRecord& r, int h, long long rowbytes, char* msg)
{
    static const char* const TOKEN[] = {"invalid literal/length code or the data ends inside one", "invalid literal/length code",
                                        "the data ends inside a length", "invalid distance code or the data ends inside one",
                                        "invalid distance code", "the data ends inside a distance", "a distance beyond the bytes produced so far"};
    static const char* const BUILD[] = {"no code-length code", "over-subscribed code set", "incomplete code set", "a code table without room"};
    const size_t need = (size_t)(h > 0 ? h : 0) * (size_t)(1 + rowbytes);
    msg[0] = 0;
    switch (r.cause) {
    case CK_INF_OK: break;
    case CK_INF_ZLIB_SHORT: refuse(msg, "zlib stream of %zu bytes", (size_t)r.arg0); break;
    case CK_INF_ZLIB_CHECK: refuse(msg, "zlib header: the check bits do not hold"); break;
    case CK_INF_ZLIB_METHOD: refuse(msg, "zlib header: compression method %d, not deflate", (int)r.arg0); break;
    case CK_INF_ZLIB_WINDOW: refuse(msg, "zlib header: window size code %d", (int)r.arg0); break;
    case CK_INF_ZLIB_DICT: refuse(msg, "zlib header: a preset dictionary"); break;
    case CK_INF_BLOCK_ENDS: refuse(msg, "the deflate data ends before a block header"); break;
    case CK_INF_BLOCK_TYPE3: refuse(msg, "deflate block type 3"); break;
    case CK_INF_STORED_LENS_END: refuse(msg, "the data ends inside a stored block's lengths"); break;
    case CK_INF_STORED_LENS: refuse(msg, "stored block: LEN %u and NLEN %u do not agree", r.arg0, r.arg1); break;
    case CK_INF_STORED_ENDS: refuse(msg, "the data ends inside a stored block"); break;
    case CK_INF_DYN_ENDS: refuse(msg, "the data ends inside a dynamic block's header"); break;
    case CK_INF_DYN_COUNTS: refuse(msg, "dynamic block: %u literal/length codes, %u distance codes", r.arg0, r.arg1); break;
    case CK_INF_CL_ENDS: refuse(msg, "the data ends inside the code-length code"); break;
    case CK_INF_CL_NONE: case CK_INF_CL_OVER: case CK_INF_CL_INCOMPLETE: case CK_INF_CL_ROOM:
        refuse(msg, "code-length code: %s", BUILD[r.cause - CK_INF_CL_NONE]); break;
    case CK_INF_CLSYM: refuse(msg, "invalid code-length code or the data ends inside one"); break;
    case CK_INF_REPEAT_FIRST: refuse(msg, "code-length repeat with nothing before it"); break;
    case CK_INF_REPEAT_ENDS: refuse(msg, "the data ends inside a code-length repeat"); break;
    case CK_INF_REPEAT_PAST: refuse(msg, "code-length repeat past the last code"); break;
    case CK_INF_NO_EOB: refuse(msg, "dynamic block without an end-of-block code"); break;
    case CK_INF_LIT_NONE: case CK_INF_LIT_OVER: case CK_INF_LIT_INCOMPLETE: case CK_INF_LIT_ROOM:
        refuse(msg, "literal/length code: %s", BUILD[r.cause - CK_INF_LIT_NONE]); break;
    case CK_INF_DIST_NONE: case CK_INF_DIST_OVER: case CK_INF_DIST_INCOMPLETE: case CK_INF_DIST_ROOM:
        refuse(msg, "distance code: %s", BUILD[r.cause - CK_INF_DIST_NONE]); break;
    case CK_INF_TOK_LITLEN: case CK_INF_TOK_LITLEN_SYMBOL: case CK_INF_TOK_LENGTH_ENDS: case CK_INF_TOK_DIST: case CK_INF_TOK_DIST_SYMBOL:
    case CK_INF_TOK_DIST_ENDS: case CK_INF_TOK_FAR:
        refuse(msg, "%s (after %zu bytes)", TOKEN[r.cause - CK_INF_TOK_LITLEN], (size_t)r.produced); break;
    case CK_INF_ADLER_ENDS: refuse(msg, "the zlib stream ends before its Adler-32"); break;
    case CK_INF_ADLER: refuse(msg, "Adler-32 %08x where the data has %08x", r.arg0, r.arg1); break;
    case CK_INF_ROWS_SHORT:
        refuse(msg, "IDAT data too short: %zu bytes where %d rows of 1 + %lld need %zu", (size_t)r.produced, h, rowbytes, need); break;
    case CK_INF_ROW_FILTER: refuse(msg, "row %d: filter type %d", (int)r.arg0, (int)r.arg1); break;
    default: refuse(msg, "inflate cause %d", r.cause); break;
    }
}

namespace {

// what a wave of the kernel keeps in LDS and in registers
struct Staged {
    uint8_t ring[CK_INF_RING];
    uint16_t lit[CK_INF_LIT_CAP], dist[CK_INF_DIST_CAP], cl[CK_INF_CL_CAP];
    uint8_t lens[320];
    CkInfAdlerWork aw;
    uint64_t tok[CK_INF_WINDOW];
    uint32_t q[CK_INF_WINDOW];
    uint8_t* out = nullptr;
    uint64_t cap = 0, need = 0, pitch = 0;
    uint64_t produced = 0, flushed = 0;
    uint32_t A = 1, B = 0;
    int64_t bad_row = -1;
    uint32_t bad_type = 0;

    // positions [flushed, to), at most CK_INF_FLUSH of them, leave the ring
    void flush(uint64_t to)
    {
        const int L = (int)(to - flushed);
        for (int t = 0; t < ck_inf_chunk_tiles(L); t++) {
            const int left = L - t * CK_PNG_TILE_BYTES;
            ck_inf_tile_pair(ring, flushed + (uint64_t)t * CK_PNG_TILE_BYTES, left < CK_PNG_TILE_BYTES ? left : CK_PNG_TILE_BYTES, &aw.a[1 + t], &aw.b[1 + t]);
        }
        ck_inf_adler_chunk(&aw, L, &A, &B);
        for (uint64_t p = flushed; p < to && p < cap; p++) out[p] = ring[p & (CK_INF_RING - 1)];
        if (pitch && bad_row < 0) bad_row = ck_inf_row_check(ring, flushed, to, need, pitch, 0, 1, &bad_type);
        flushed = to;
    }
    void drain()
    {
        while (produced - flushed >= (uint64_t)CK_INF_FLUSH) flush(flushed + CK_INF_FLUSH);
    }
};

void staged_run(const CkInfIn& in, Staged& s, CkInfRecord* rec)
{
    *rec = CkInfRecord();
    rec->cause = ck_inf_wrapper(in, &rec->arg0);
    if (rec->cause) return;
    rec->arg0 = 0;
    const uint64_t bits = ck_inf_bits(in);
    uint64_t pos = 16;
    for (int last = 0; !last;) {
        CkInfBlock b;
        ck_inf_block(in, pos, s.lit, s.dist, s.cl, s.lens, &b);
        if (b.cause) { rec->cause = b.cause; rec->arg0 = b.arg0; rec->arg1 = b.arg1; rec->produced = (int64_t)s.produced; return; }
        last = b.last;
        pos = b.pos;
        if (b.type == 0) {                                   // a stored block, a piece of the ring at a time
            for (uint32_t done = 0; done < b.stored;) {
                const uint32_t m = b.stored - done < (uint32_t)CK_INF_STEP_BYTES ? b.stored - done : (uint32_t)CK_INF_STEP_BYTES;
                for (uint32_t i = 0; i < m; i++) s.ring[(s.produced + i) & (CK_INF_RING - 1)] = in.z[(pos >> 3) + done + i];
                s.produced += m; done += m;
                s.drain();
            }
            pos += (uint64_t)b.stored * 8;
            continue;
        }
        for (;;) {                                           // window steps
            for (int o = 0; o < CK_INF_WINDOW; o++)
                s.tok[o] = ck_inf_token(ck_inf_peek(in, pos + (uint64_t)o), (int64_t)(bits - pos) - o, s.lit, s.dist);
            CkInfWalk w;
            ck_inf_walk([&](uint32_t o) { return s.tok[o]; }, [&](uint32_t o, uint32_t at) { s.q[o] = at; }, s.produced, CK_INF_WINDOW, &w);
            const uint64_t n = s.produced;
            if (!w.far)
                for (int o = 0; o < CK_INF_WINDOW; o++)
                    if ((w.taken[o >> 6] >> (o & 63) & 1) && ck_inf_kind(s.tok[o]) == CK_INF_LITERAL)
                        s.ring[(n + s.q[o]) & (CK_INF_RING - 1)] = (uint8_t)ck_inf_val(s.tok[o]);
            for (int o = 0; o < CK_INF_WINDOW; o++) {
                if (!(w.taken[o >> 6] >> (o & 63) & 1)) continue;
                const uint64_t at = n + s.q[o], v = ck_inf_val(s.tok[o]);
                if (ck_inf_kind(s.tok[o]) == CK_INF_LITERAL) {
                    if (w.far) s.ring[at & (CK_INF_RING - 1)] = (uint8_t)v;
                    continue;
                }
                for (uint32_t i = 0, len = ck_inf_len(s.tok[o]); i < len; i++)
                    s.ring[(at + i) & (CK_INF_RING - 1)] = s.ring[(at - v + i % v) & (CK_INF_RING - 1)];
            }
            s.produced += w.bytes; pos += w.advance;
            rec->steps++; rec->tokens += w.tokens;
            s.drain();
            if (w.end == CK_INF_REFUSED) { rec->cause = (int32_t)w.cause; rec->produced = (int64_t)s.produced; return; }
            if (w.end == CK_INF_EOB) break;
        }
    }
    if (s.produced > s.flushed) s.flush(s.produced);
    rec->produced = (int64_t)s.produced;
    const uint64_t tail = (pos + 7) >> 3;
    if (in.bytes - tail < 4) { rec->cause = CK_INF_ADLER_ENDS; return; }
    const uint32_t want = be32(in.z + tail), got = s.B << 16 | s.A;
    if (want != got) { rec->cause = CK_INF_ADLER; rec->arg0 = want; rec->arg1 = got; return; }
    if (!s.pitch) return;
    if (s.produced < s.need) { rec->cause = CK_INF_ROWS_SHORT; return; }
    if (s.bad_row >= 0) { rec->cause = CK_INF_ROW_FILTER; rec->arg0 = (uint32_t)s.bad_row; rec->arg1 = s.bad_type; }
}

}  // namespace

int ck_png_unzip_staged_rows(const uint8_t* z, size_t zlen, uint8_t* out, size_t cap, size_t* total, CkInfRecord* record, char* msg, int h, long long rowbytes)
{
    *total = 0;
    std::vector<Staged> st(1);
    Staged& s = st[0];
    s.out = out; s.cap = out ? cap : 0;
    if (h > 0) { s.pitch = (uint64_t)(1 + rowbytes); s.need = (uint64_t)h * s.pitch; }
    CkInfIn in;
    in.z = z; in.bytes = z ? zlen : 0;
    CkInfRecord rec;
    staged_run(in, s, &rec);
    if (!z) rec.arg0 = (uint32_t)zlen;
    if (record) *record = rec;
    ck_png_inflate_message(rec, h, rowbytes, msg);
    if (rec.cause) return CK_ERR_DATA;
    *total = (size_t)rec.produced;
    return CK_OK;
}

int ck_png_unzip_staged(const uint8_t* z, size_t zlen, uint8_t* out, size_t cap, size_t* total, CkInfRecord* record, char* msg)
{
    return ck_png_unzip_staged_rows(z, zlen, out, cap, total, record, msg, 0, 0);
}

// ---- writing ----
size_t ck_png_wrap(const uint8_t* z, size_t zlen, int h, int w, uint8_t* out)
{
    static const uint8_t SIG[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    uint8_t* p = out;
    memcpy(p, SIG, 8); p += 8;
    put_be32(p, 13); memcpy(p + 4, "IHDR", 4);
    put_be32(p + 8, (uint32_t)w); put_be32(p + 12, (uint32_t)h);
    p[16] = 8; p[17] = 2; p[18] = 0; p[19] = 0; p[20] = 0;   // 8 bits, RGB, deflate, the five filters, not interlaced
    put_be32(p + 21, ck_png_crc32(p + 4, 17)); p += 25;
    put_be32(p, (uint32_t)zlen); memcpy(p + 4, "IDAT", 4);
    if (p + 8 != z) memmove(p + 8, z, zlen);
    put_be32(p + 8 + zlen, ck_png_crc32(p + 4, 4 + zlen)); p += 12 + zlen;
    put_be32(p, 0); memcpy(p + 4, "IEND", 4);
    put_be32(p + 8, ck_png_crc32(p + 4, 4)); p += 12;
    return (size_t)(p - out);
}

size_t ck_png_bound(int h, int w)
{
    const CkPngGeom g = ck_png_geom(h, w);
    const uint64_t bits = (uint64_t)g.bands * (CK_PNG_HDR_BITS + CK_PNG_MAX_BITS) + (uint64_t)g.fbytes * CK_PNG_MAX_BITS;
    return CK_PNG_CONTAINER + (size_t)ck_png_zlib_bytes(bits) + 16;
}

namespace {

// where the run of every position of a tile starts and ends, from the tile's start (s may be negative, e beyond L)
void tile_runs(const uint8_t* p, int L, uint32_t before, uint32_t after, int* s, int* e)
{
    for (int i = 0; i < L; i++) s[i] = i == 0 ? -(int)before : p[i] == p[i - 1] ? s[i - 1] : i;
    for (int i = L - 1; i >= 0; i--) e[i] = i == L - 1 ? L + (int)after : p[i + 1] == p[i] ? e[i + 1] : i + 1;
}

template <int NS>
void build_band(const uint32_t* count, uint8_t* len, uint16_t* code)
{
    uint32_t work[NS];
    uint16_t order[NS];
    int m = 0;
    for (int s = 0; s < NS; s++)
        if (count[s]) { order[ck_png_rank<NS>(count, s)] = (uint16_t)s; m++; }
    ck_png_lengths<NS>(count, order, m, work, len, code);
}

}  // namespace

int ck_png_stage_encode(const uint8_t* bgr, int n, int h, int w, int filter, uint8_t* out, size_t stride, size_t* len, char* msg, int runs)
{
    const CkPngGeom g = ck_png_geom(h, w);
    const int PITCH = ck_png_pitch(runs);
    std::vector<uint8_t> filt((size_t)g.fbytes), lens((size_t)g.bands * PITCH), z;
    std::vector<uint16_t> codes((size_t)g.bands * PITCH);
    std::vector<uint32_t> tile_bits((size_t)g.tiles), tile_a((size_t)g.tiles), tile_b((size_t)g.tiles);
    std::vector<uint64_t> tile_off((size_t)g.tiles), band_off((size_t)g.bands), band_bits((size_t)g.bands);
    std::vector<uint32_t> band_a((size_t)g.bands), band_b((size_t)g.bands);
    std::vector<CkPngEdge> edge(runs ? (size_t)g.tiles : 0);
    std::vector<uint32_t> before(edge.size()), after(edge.size());
    int rs[CK_PNG_TILE_BYTES], re[CK_PNG_TILE_BYTES];
    for (int f = 0; f < n; f++) {
        const uint8_t* img = bgr + (size_t)f * h * w * 3;
        // filter
        for (int64_t y = 0; y < h; y++) {
            int ft = filter;
            if (ft < 0) {
                uint32_t sum[5] = {0, 0, 0, 0, 0};
                for (int64_t i = 0; i < 3 * (int64_t)w; i++) {
                    int x, a, b, c;
                    ck_png_context(img, w, y, i, &x, &a, &b, &c);
                    for (int t = 0; t < 5; t++) sum[t] += ck_png_cost((uint8_t)(x - ck_png_predict(t, a, b, c)));
                }
                ft = ck_png_choose(sum);
            }
            uint8_t* row = filt.data() + y * g.row;
            row[0] = (uint8_t)ft;
            for (int64_t i = 0; i < 3 * (int64_t)w; i++) row[1 + i] = ck_png_residual(img, w, y, i, ft);
        }
        // edges, join (the runs mode)
        if (runs)
            for (int64_t band = 0; band < g.bands; band++) {
                const size_t k = (size_t)(band * g.band_tiles);
                for (int64_t t = 0; t < g.band_tiles; t++) edge[k + t] = ck_png_edge(filt.data() + ck_png_tile_at(g, band, t), ck_png_tile_len(g, band, t));
                ck_png_join_band(g, band, edge.data() + k, before.data() + k, after.data() + k);
            }
        // count, build
        for (int64_t band = 0; band < g.bands; band++) {
            uint32_t count[CK_PNG_RUN_SYMS];
            memset(count, 0, sizeof count);
            const uint8_t* p = filt.data() + ck_png_tile_at(g, band, 0);
            if (!runs) {
                for (int64_t i = 0, e = ck_png_band_bytes(g, band); i < e; i++) count[p[i]]++;
            } else {
                for (int64_t t = 0; t < g.band_tiles; t++) {
                    const size_t k = (size_t)(band * g.band_tiles + t);
                    const uint8_t* q = p + t * CK_PNG_TILE_BYTES;
                    const int L = ck_png_tile_len(g, band, t);
                    tile_runs(q, L, before[k], after[k], rs, re);
                    for (int i = 0; i < L; i++) {
                        int tb;
                        uint32_t tail;
                        const int sym = ck_png_token(q[i], i - rs[i] - 1, re[i] - rs[i] - 1, &tb, &tail);
                        if (sym >= 0) count[sym]++;
                    }
                }
            }
            count[256] = 1;
            if (runs) build_band<CK_PNG_RUN_SYMS>(count, lens.data() + band * PITCH, codes.data() + band * PITCH);
            else build_band<CK_PNG_SYMS>(count, lens.data() + band * PITCH, codes.data() + band * PITCH);
        }
        // size
        for (int64_t band = 0; band < g.bands; band++)
            for (int64_t t = 0; t < g.band_tiles; t++) {
                const uint8_t* p = filt.data() + ck_png_tile_at(g, band, t);
                const uint8_t* bl = lens.data() + band * PITCH;
                const int L = ck_png_tile_len(g, band, t);
                const size_t k = (size_t)(band * g.band_tiles + t);
                uint32_t bits = 0, a = 0, b = 0;
                for (int i = 0; i < L; i++) { a += p[i]; b += (uint32_t)(L - i) * p[i]; }
                if (!runs) {
                    for (int i = 0; i < L; i++) bits += bl[p[i]];
                } else {
                    tile_runs(p, L, before[k], after[k], rs, re);
                    for (int i = 0; i < L; i++) {
                        int tb;
                        uint32_t tail;
                        const int sym = ck_png_token(p[i], i - rs[i] - 1, re[i] - rs[i] - 1, &tb, &tail);
                        if (sym >= 0) bits += (uint32_t)(bl[sym] + tb);
                    }
                }
                tile_bits[k] = bits; tile_a[k] = a; tile_b[k] = b;
            }
        // scan
        uint64_t frame_bits = 0;
        uint32_t adler = 0;
        for (int64_t band = 0; band < g.bands; band++) {
            const size_t k = (size_t)(band * g.band_tiles);
            ck_png_scan_band(g, band, tile_bits.data() + k, tile_a.data() + k, tile_b.data() + k, lens[(size_t)band * PITCH + 256],
                             tile_off.data() + k, &band_bits[(size_t)band], &band_a[(size_t)band], &band_b[(size_t)band], ck_png_hdr_bits(runs));
        }
        ck_png_scan_frame(g, band_bits.data(), band_a.data(), band_b.data(), band_off.data(), &frame_bits, &adler);
        const size_t zlen = (size_t)ck_png_zlib_bytes(frame_bits);
        if (CK_PNG_CONTAINER + zlen > stride) {
            snprintf(msg, CK_PNG_MSG, "frame %d: a file of %zu bytes, above the stride of %zu", f, CK_PNG_CONTAINER + zlen, stride);
            return CK_ERR_ARG;
        }
        // put
        z.assign(zlen + 8, 0);
        z[0] = 0x78; z[1] = 0x01;
        for (int64_t band = 0; band < g.bands; band++) {
            const uint8_t* bl = lens.data() + band * PITCH;
            const uint16_t* bc = codes.data() + band * PITCH;
            for (int i = 0; i < ck_png_hdr_fields(runs); i++) {
                uint32_t v;
                int nb, off;
                if (runs) ck_png_run_hdr_field(i, bl, band == g.bands - 1, &v, &nb, &off);
                else ck_png_hdr_field(i, bl, band == g.bands - 1, &v, &nb, &off);
                ck_png_or_bits(z.data(), 16 + band_off[(size_t)band] + (uint64_t)off, v, nb);
            }
            uint64_t pos = 0;
            for (int64_t t = 0; t < g.band_tiles; t++) {
                const uint8_t* p = filt.data() + ck_png_tile_at(g, band, t);
                const size_t k = (size_t)(band * g.band_tiles + t);
                const int L = ck_png_tile_len(g, band, t);
                pos = 16 + band_off[(size_t)band] + tile_off[k];
                if (!runs) {
                    for (int i = 0; i < L; i++) { ck_png_or_bits(z.data(), pos, bc[p[i]], bl[p[i]]); pos += bl[p[i]]; }
                    continue;
                }
                tile_runs(p, L, before[k], after[k], rs, re);
                for (int i = 0; i < L; i++) {
                    int tb;
                    uint32_t tail;
                    const int sym = ck_png_token(p[i], i - rs[i] - 1, re[i] - rs[i] - 1, &tb, &tail);
                    if (sym < 0) continue;
                    ck_png_or_bits(z.data(), pos, bc[sym], bl[sym]); pos += bl[sym];
                    ck_png_or_bits(z.data(), pos, tail, tb); pos += (uint64_t)tb;
                }
            }
            ck_png_or_bits(z.data(), pos, bc[256], bl[256]);
        }
        put_be32(z.data() + 2 + (frame_bits + 7) / 8, adler);
        len[f] = ck_png_wrap(z.data(), zlen, h, w, out + (size_t)f * stride);
    }
    return CK_OK;
}
