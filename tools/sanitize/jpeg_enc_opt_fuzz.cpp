// jpeg_enc_opt_fuzz.cpp -- optimised Huffman tables on the host under AddressSanitizer + UBSan: the histo and tables steps of
// camkifu_amd/csrc/ck_jpeg_enc_stage.h and the two coders built on them in ck_jpeg_enc.cpp (linked with ck_jpeg.cpp and nothing
// else).  Every batch goes through ck_jpeg_enc_entropy_opt frame by frame and through ck_jpeg_enc_staged_opt, and the status,
// the lowest refused frame, its message, the lengths and the bytes must agree; an accepted stream is parsed and decoded by
// ck_jpeg.cpp, which must give the coefficients back.  Inputs: all-zero frames, frames whose every coefficient is at the end
// of the baseline range, seeded random coefficients, dense and sparse, those the coder refuses included, over a few
// geometries and restart intervals.  Tables: counters that are random, equal, single, Fibonacci, of 32 bits throughout and
// one chain as deep as 256 leaves allow; each result is a prefix code of at most 16 bits without the code of all ones that
// covers exactly the counted symbols.  Coefficients, streams, counters and lengths live in heap blocks of exactly their size.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I include tools/sanitize/jpeg_enc_opt_fuzz.cpp \
//       camkifu_amd/csrc/ck_jpeg_enc.cpp camkifu_amd/csrc/ck_jpeg.cpp
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../camkifu_amd/csrc/ck_jpeg_enc.h"
#include "../../camkifu_amd/csrc/ck_jpeg_tables.h"

static long g_ok = 0, g_refused = 0, g_tables = 0;

static void die(const char* what) { fprintf(stderr, "%s\n", what); exit(2); }

// counters -> a table; what every table must be
static void table(const uint32_t* counts)
{
    std::unique_ptr<uint32_t[]> freq(new uint32_t[256]);
    memcpy(freq.get(), counts, 256 * sizeof(uint32_t));
    std::unique_ptr<uint8_t[]> bits(new uint8_t[16]), vals(new uint8_t[256]);
    int32_t count = -1;
    ck_jpeg_enc_optimal_table(freq.get(), bits.get(), vals.get(), &count);
    int symbols = 0, total = 0;
    for (int i = 0; i < 256; i++) symbols += counts[i] != 0;
    uint64_t kraft = 0;
    for (int l = 1; l <= 16; l++) { total += bits[l - 1]; kraft += (uint64_t)bits[l - 1] << (16 - l); }
    if (count != symbols || total != symbols) die("the table does not hold the counted symbols");
    if (symbols && kraft > 65535) die("Kraft's sum leaves no room for the code of all ones");
    char seen[256] = {0};
    for (int i = 0; i < count; i++) {
        if (!counts[vals[i]] || seen[vals[i]]++) die("a value that was not counted, or twice");
    }
    auto huff = std::make_unique<CkEncHuff>();
    ck_enc_fill(huff.get(), bits.get(), vals.get());
    for (int s = 0; s < 256; s++) {
        if ((huff->len[s] != 0) != (counts[s] != 0)) die("a counted symbol without a code, or a code without a count");
        if (huff->len[s] > 16 || (huff->len[s] && huff->code[s] == (1u << huff->len[s]) - 1)) die("a code above 16 bits or of all ones");
    }
    std::unique_ptr<uint8_t[]> dht(new uint8_t[CK_ENC_DHT_SLOT]);
    if (ck_enc_dht(dht.get(), 3, bits.get(), vals.get(), count) != (uint32_t)(21 + count) || dht[4] != 0x11) die("the DHT segment is wrong");
    g_tables++;
}

// n frames through both coders, every buffer of exactly its size; an accepted stream must decode to the coefficients
static int both(const int16_t* frames, int n, size_t ncoef, const uint16_t* quant, int h, int w, int s, int ri)
{
    const size_t stride = ck_jpeg_enc_bound(h, w, s);
    std::unique_ptr<int16_t[]> coef(new int16_t[(size_t)n * ncoef]);
    memcpy(coef.get(), frames, (size_t)n * ncoef * sizeof(int16_t));
    std::unique_ptr<uint8_t[]> plain(new uint8_t[(size_t)n * stride]), staged(new uint8_t[(size_t)n * stride]);
    std::unique_ptr<size_t[]> plen(new size_t[n]), slen(new size_t[n]);
    std::unique_ptr<uint32_t[]> freq(new uint32_t[4 * 256]);
    int prc = CK_OK, pbad = -1;
    char pmsg[CK_JPEG_MSG] = {0}, smsg[CK_JPEG_MSG] = {0};
    for (int f = 0; f < n; f++) {
        char msg[CK_JPEG_MSG], hmsg[CK_JPEG_MSG], std_msg[CK_JPEG_MSG];
        const int rc = ck_jpeg_enc_entropy_opt(coef.get() + (size_t)f * ncoef, quant, h, w, s, ri, plain.get() + (size_t)f * stride, stride, &plen[f], msg);
        // the histogram alone and the standard coder refuse what it refuses, in its words
        const int hrc = ck_jpeg_enc_histogram(coef.get() + (size_t)f * ncoef, h, w, s, ri, freq.get(), hmsg);
        size_t std_len;
        std::unique_ptr<uint8_t[]> std_out(new uint8_t[stride]);
        const int std_rc = ck_jpeg_enc_entropy(coef.get() + (size_t)f * ncoef, quant, h, w, s, ri, std_out.get(), stride, &std_len, std_msg);
        if (hrc != rc || std_rc != rc || (rc != CK_OK && (strcmp(hmsg, msg) != 0 || strcmp(std_msg, msg) != 0))) {
            fprintf(stderr, "optimised: %d '%s'\nhistogram: %d '%s'\nstandard: %d '%s'\n", rc, msg, hrc, hmsg, std_rc, std_msg);
            die("the optimised coder refuses otherwise than the standard one");
        }
        if (rc == CK_OK) for (int t = 0; t < (s == CK_JPEG_GREY ? 2 : 4); t++) table(freq.get() + 256 * t);
        if (rc != CK_OK && prc == CK_OK) { prc = rc; pbad = f; memcpy(pmsg, msg, sizeof pmsg); }
    }
    int sbad = -1;
    const int src = ck_jpeg_enc_staged_opt(coef.get(), quant, n, h, w, s, ri, staged.get(), stride, slen.get(), &sbad, smsg);
    if (src != prc || sbad != pbad || strcmp(smsg, pmsg) != 0) {
        fprintf(stderr, "plain: %d frame %d '%s'\nstaged: %d frame %d '%s'\n", prc, pbad, pmsg, src, sbad, smsg);
        die("the staged coder decides otherwise than the plain one");
    }
    if (src != CK_OK) { g_refused++; return src; }
    for (int f = 0; f < n; f++) {
        if (slen[f] != plen[f] || memcmp(staged.get() + (size_t)f * stride, plain.get() + (size_t)f * stride, plen[f]) != 0) {
            fprintf(stderr, "%dx%d sampling %d interval %d frame %d of %d: %zu bytes, the plain coder %zu\n", w, h, s, ri, f, n, slen[f], plen[f]);
            die("the staged coder writes other bytes than the plain one");
        }
        std::unique_ptr<uint8_t[]> stream(new uint8_t[plen[f]]);
        memcpy(stream.get(), plain.get() + (size_t)f * stride, plen[f]);
        auto fr = std::make_unique<CkJpegFrame>();
        char msg[CK_JPEG_MSG];
        if (ck_jpeg_parse(stream.get(), plen[f], fr.get(), msg) != CK_OK) { fprintf(stderr, "%s\n", msg); die("the stream does not parse"); }
        if (fr->info.h != h || fr->info.w != w || fr->info.sampling != s) die("the stream has another geometry");
        std::unique_ptr<int16_t[]> back(new int16_t[ncoef]);
        if (ck_jpeg_entropy(stream.get(), plen[f], *fr, back.get(), msg) != CK_OK) { fprintf(stderr, "%s\n", msg); die("the stream does not decode"); }
        if (memcmp(back.get(), coef.get() + (size_t)f * ncoef, ncoef * sizeof(int16_t)) != 0) die("the stream decodes to other coefficients");
    }
    g_ok++;
    return CK_OK;
}

int main()
{
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };

    // ---- tables ----
    std::vector<uint32_t> c(256);
    auto clear = [&]() { for (auto& v : c) v = 0; };
    clear(); table(c.data());                                                        // nothing counted: an empty table
    for (int s : {0, 7, 255}) { clear(); c[s] = 1; table(c.data()); c[s] = 0xFFFFFFFFu; table(c.data()); }
    for (uint32_t v : {1u, 3u, 0xFFFFFFFFu}) { for (auto& x : c) x = v; table(c.data()); }    // all equal; sums of 40 bits
    clear();
    { uint32_t a = 1, b = 2; for (int i = 0; i < 45; i++) { c[(i * 37 + 5) & 255] = a; const uint32_t n = a + b; a = b; b = n; } }
    table(c.data());                                                                 // one chain: code sizes up to 45
    // as deep as 256 symbols allow without leaving 64 bits: a chain of 60, the others equal
    clear();
    for (int i = 0; i < 256; i++) c[i] = i < 32 ? 1u << i : 0xFFFFFFFFu;
    table(c.data());
    for (int round = 0; round < 400; round++) {
        for (auto& v : c) {
            const uint64_t r = next();
            v = round % 4 == 0 ? (uint32_t)r : round % 4 == 1 ? (uint32_t)(r % 3 ? 0 : r >> 40) : round % 4 == 2 ? (uint32_t)(r % 7 == 0) : (uint32_t)(1u << (r % 32));
        }
        table(c.data());
    }

    // ---- a frame of more than 2^25 blocks: refused before a coefficient is read ----
    {
        std::unique_ptr<int16_t[]> one(new int16_t[64]());
        std::unique_ptr<uint32_t[]> freq(new uint32_t[4 * 256]);
        char msg[CK_JPEG_MSG];
        if (ck_jpeg_enc_histogram(one.get(), 65535, 65535, CK_JPEG_GREY, 0, freq.get(), msg) != CK_ERR_ARG || !strstr(msg, "2^25")) die("2^26 blocks are counted");
        uint16_t q[192];
        ck_jpeg_enc_quant(50, q);
        std::unique_ptr<uint8_t[]> out(new uint8_t[2048]);
        size_t len = 1;
        if (ck_jpeg_enc_entropy_opt(one.get(), q, 65535, 65535, CK_JPEG_GREY, 0, out.get(), 2048, &len, msg) != CK_ERR_ARG || len != 0) die("2^26 blocks are coded");
    }

    // ---- coders ----
    static const int GEOM[][3] = {{8, 8, CK_JPEG_GREY}, {16, 16, CK_JPEG_420}, {17, 23, CK_JPEG_GREY}, {17, 23, CK_JPEG_444}, {17, 23, CK_JPEG_422},
                                  {17, 23, CK_JPEG_420}, {1, 1, CK_JPEG_420}, {64, 96, CK_JPEG_420}, {8, 600, CK_JPEG_444}};
    uint16_t quant[192];
    ck_jpeg_enc_quant(90, quant);
    for (const auto& gm : GEOM) {
        const int h = gm[0], w = gm[1], s = gm[2];
        const size_t ncoef = (size_t)ck_jpeg_blocks(h, w, s) * 64;
        for (int ri : {0, 1, 2, 65535}) {
            std::vector<int16_t> x(3 * ncoef);
            for (int kind = 0; kind < 3; kind++) {
                // all zero: one-symbol tables; the ends of the range everywhere: no EOB, stuffed bytes; a lone last coefficient: ZRL
                for (size_t i = 0; i < x.size(); i++) {
                    const size_t k = i % 64, b = i / 64;
                    x[i] = kind == 0 ? 0
                         : kind == 1 ? (int16_t)(k == 0 ? (b & 1 ? 1023 : -1023) : (k & 1 ? -1023 : 1023))
                                     : (int16_t)(k == 63 ? 1 + (int)(b % 5) : (k == 0 ? (int)(b % 9) * 100 : 0));
                }
                if (both(x.data(), 3, ncoef, quant, h, w, s, ri) != CK_OK) die("a synthetic case is refused");
            }
            for (int round = 0; round < 6; round++) {
                for (auto& v : x) {
                    const uint64_t r = next();
                    v = round == 0 ? (int16_t)((int)(r % 2047) - 1023)
                      : round == 1 ? (int16_t)(r % 9 ? 0 : (int)((r >> 8) % 2047) - 1023)
                      : round == 2 ? (int16_t)(r % 40 ? 0 : (int)((r >> 8) % 7) - 3)
                      : round == 3 ? (int16_t)(r % 3 ? 0 : ((r >> 8) & 1 ? 1023 : -1023))
                      : round == 4 ? (int16_t)(r % 5000 ? (int)((r >> 8) % 63) - 31 : 1024)
                                   : (int16_t)r;
                }
                if (round < 4) for (size_t b = 0; b < x.size() / 64; b++) x[b * 64] = (int16_t)(x[b * 64] / 2);       // DC differences inside 11 bits
                const int rc = both(x.data(), 3, ncoef, quant, h, w, s, ri);
                if (round < 4 && rc != CK_OK) die("coefficients inside the baseline range are refused");
            }
        }
    }
    printf("jpeg optimised tables: %ld tables valid, %ld batches equal in both coders (%ld accepted and decoded back, %ld refused)\n", g_tables,
           g_ok + g_refused, g_ok, g_refused);
    return 0;
}
