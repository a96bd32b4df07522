// jpeg_enc_stage_fuzz.cpp -- the steps of the GPU's JPEG entropy coder run on the host (ck_jpeg_enc_staged over
// camkifu_amd/csrc/ck_jpeg_enc_stage.h, in ck_jpeg_enc.cpp; linked with ck_jpeg.cpp and nothing else) under AddressSanitizer +
// UBSan, every result held to the plain coder ck_jpeg_enc_entropy: the status, the lowest frame that is refused and its
// message, the lengths and the bytes.  Inputs: the coefficients of every JPEG file given on the command line (which must give
// the file's bytes back), alone and as a batch of three; the synthetic extremes of tests/jpeg_enc_stage_cases.py (all zero;
// codes that end in stuffed bytes; no EOB and 11-bit DC differences) over a few geometries and restart intervals; seeded
// random coefficients, sparse and dense, those the baseline tables cannot code included.  Coefficients, streams and lengths
// live in heap blocks of exactly their size, so a read or write one byte outside them is caught.  The closed forms that map
// scan order to the coefficient layout and back are walked over every block on the way.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I include tools/sanitize/jpeg_enc_stage_fuzz.cpp \
//       camkifu_amd/csrc/ck_jpeg_enc.cpp camkifu_amd/csrc/ck_jpeg.cpp
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../camkifu_amd/csrc/ck_jpeg_enc.h"
#include "../../camkifu_amd/csrc/ck_jpeg_tables.h"

static long g_ok = 0, g_refused = 0;

static void die(const char* what) { fprintf(stderr, "%s\n", what); exit(2); }

static void walk_geometry(int h, int w, int s, int ri)
{
    const CkEncGeom g = ck_enc_geom(h, w, s, ri);
    if (g.blocks != ck_jpeg_blocks(h, w, s)) die("the geometry counts other blocks");
    std::vector<char> seen((size_t)g.blocks, 0);
    for (int64_t b = 0; b < g.blocks; b++) {
        const int64_t p = ck_enc_place(g, b);
        if (p < 0 || p >= g.blocks || seen[(size_t)p]++) die("scan order does not map onto the layout one to one");
        if (ck_enc_block_of(g, p) != b) die("the way back from the layout is another block");
        const int64_t pb = ck_enc_pred_block(g, b);
        if (pb >= b || (pb >= 0 && ck_enc_is_chroma(g, pb) != ck_enc_is_chroma(g, b))) die("a predecessor that is none");
    }
    int64_t covered = 0;
    for (int64_t k = 0; k < g.nseg; k++)
        for (int64_t t = 0; t < g.seg_tiles; t++) {
            int64_t b0;
            int cnt;
            ck_enc_tile_blocks(g, k, t, &b0, &cnt);
            if (cnt && b0 != covered) die("the tiles do not follow one another");
            covered += cnt;
        }
    if (covered != g.blocks) die("the tiles do not cover the frame");
}

// n frames through both coders, every buffer of exactly its size
static int both(const int16_t* frames, int n, size_t ncoef, const uint16_t* quant, int h, int w, int s, int ri, std::vector<uint8_t>* first = nullptr)
{
    const size_t stride = ck_jpeg_enc_bound(h, w, s);
    std::unique_ptr<int16_t[]> coef(new int16_t[(size_t)n * ncoef]);
    memcpy(coef.get(), frames, (size_t)n * ncoef * sizeof(int16_t));
    std::unique_ptr<uint8_t[]> plain(new uint8_t[(size_t)n * stride]), staged(new uint8_t[(size_t)n * stride]);
    std::unique_ptr<size_t[]> plen(new size_t[n]), slen(new size_t[n]);
    int prc = CK_OK, pbad = -1;
    char pmsg[CK_JPEG_MSG] = {0}, smsg[CK_JPEG_MSG] = {0};
    for (int f = 0; f < n; f++) {
        char msg[CK_JPEG_MSG];
        const int rc = ck_jpeg_enc_entropy(coef.get() + (size_t)f * ncoef, quant, h, w, s, ri, plain.get() + (size_t)f * stride, stride, &plen[f], msg);
        if (rc != CK_OK && prc == CK_OK) { prc = rc; pbad = f; memcpy(pmsg, msg, sizeof pmsg); }
    }
    int sbad = -1;
    const int src = ck_jpeg_enc_staged(coef.get(), quant, n, h, w, s, ri, staged.get(), stride, slen.get(), &sbad, smsg);
    if (src != prc || sbad != pbad || strcmp(smsg, pmsg) != 0) {
        fprintf(stderr, "plain: %d frame %d '%s'\nstaged: %d frame %d '%s'\n", prc, pbad, pmsg, src, sbad, smsg);
        die("the staged coder decides otherwise than the plain one");
    }
    if (src != CK_OK) { g_refused++; return src; }
    for (int f = 0; f < n; f++)
        if (slen[f] != plen[f] || memcmp(staged.get() + (size_t)f * stride, plain.get() + (size_t)f * stride, plen[f]) != 0) {
            fprintf(stderr, "%dx%d sampling %d interval %d frame %d of %d: %zu bytes, the plain coder %zu\n", w, h, s, ri, f, n, slen[f], plen[f]);
            die("the staged coder writes other bytes than the plain one");
        }
    if (first) first->assign(staged.get(), staged.get() + slen[0]);
    g_ok++;
    return CK_OK;
}

static void synthetic(int kind, std::vector<int16_t>& c)
{
    const size_t nb = c.size() / 64;
    for (auto& v : c) v = 0;
    for (size_t b = 0; b < nb; b++) {
        int16_t* blk = c.data() + b * 64;
        if (kind == 1) {
            blk[ZIGZAG[16]] = blk[ZIGZAG[32]] = blk[ZIGZAG[48]] = 1023;
            blk[0] = (int16_t)(b & 1 ? 1000 : 0);
        } else if (kind == 2) {
            for (int i = 1; i < 64; i++) blk[i] = (int16_t)(i & 1 ? -1023 : 1023);
            blk[0] = (int16_t)(b & 1 ? 1023 : -1023);
        }
    }
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: jpeg_enc_stage_fuzz case.jpg ...\n"); return 2; }
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    uint16_t quant[192];
    // the committed streams
    for (int a = 1; a < argc; a++) {
        FILE* fp = fopen(argv[a], "rb");
        if (!fp) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> buf;
        uint8_t chunk[4096];
        for (size_t k; (k = fread(chunk, 1, sizeof chunk, fp)) > 0;) buf.insert(buf.end(), chunk, chunk + k);
        fclose(fp);
        auto f = std::make_unique<CkJpegFrame>();
        char msg[CK_JPEG_MSG];
        if (ck_jpeg_parse(buf.data(), buf.size(), f.get(), msg) != CK_OK) { fprintf(stderr, "%s: %s\n", argv[a], msg); return 2; }
        const int h = f->info.h, w = f->info.w, s = f->info.sampling, ri = f->info.restart_interval;
        const size_t ncoef = (size_t)f->info.blocks * 64;
        std::vector<int16_t> coef(3 * ncoef);
        if (ck_jpeg_entropy(buf.data(), buf.size(), *f, coef.data(), msg) != CK_OK) { fprintf(stderr, "%s: %s\n", argv[a], msg); return 2; }
        memcpy(quant, f->quant, sizeof quant);
        if (s == CK_JPEG_GREY) for (int i = 64; i < 192; i++) quant[i] = quant[i - 64];
        walk_geometry(h, w, s, ri);
        std::vector<uint8_t> again;
        if (both(coef.data(), 1, ncoef, quant, h, w, s, ri, &again) != CK_OK) { fprintf(stderr, "%s is refused\n", argv[a]); return 2; }
        if (again != buf) { fprintf(stderr, "%s: other bytes than the file's\n", argv[a]); return 2; }
        // a batch of three: the case, the case with a few coefficients moved, the case again; other restart intervals
        memcpy(coef.data() + ncoef, coef.data(), ncoef * sizeof(int16_t));
        memcpy(coef.data() + 2 * ncoef, coef.data(), ncoef * sizeof(int16_t));
        for (int k = 0; k < 16; k++) coef[ncoef + next() % ncoef] = (int16_t)((int)(next() % 31) - 15);
        for (int r : {ri, 0, 1, 2}) both(coef.data(), 3, ncoef, quant, h, w, s, r);
        // an uncodable value in the last frame, then also in the middle one: the lowest frame is named
        coef[2 * ncoef + 64 * (next() % (ncoef / 64)) + 1 + next() % 63] = 2000;
        if (both(coef.data(), 3, ncoef, quant, h, w, s, ri) == CK_OK) die("a value of 11 bits is accepted");
        coef[ncoef + 64 * (next() % (ncoef / 64))] = -32768;
        if (both(coef.data(), 3, ncoef, quant, h, w, s, ri) == CK_OK) die("a DC value of 16 bits is accepted");
        // bad tables and arguments are refused in the plain coder's words
        uint16_t zq[192];
        memcpy(zq, quant, sizeof zq);
        zq[5] = 0;
        if (both(coef.data(), 1, ncoef, zq, h, w, s, ri) == CK_OK) die("a zero quant entry is accepted");
        if (both(coef.data(), 1, ncoef, quant, h, w, s, 65536) == CK_OK) die("a restart interval of 65536 is accepted");
    }
    // the synthetic extremes and random coefficients
    static const int GEOM[][3] = {{64, 96, CK_JPEG_GREY}, {64, 96, CK_JPEG_444}, {64, 96, CK_JPEG_422}, {64, 96, CK_JPEG_420},
                                  {1, 1, CK_JPEG_GREY}, {1, 1, CK_JPEG_420}, {17, 33, CK_JPEG_422}, {17, 33, CK_JPEG_420}, {8, 200, CK_JPEG_444}};
    ck_jpeg_enc_quant(90, quant);
    for (const auto& gm : GEOM) {
        const int h = gm[0], w = gm[1], s = gm[2];
        const size_t ncoef = (size_t)ck_jpeg_blocks(h, w, s) * 64;
        const int row = (w + 8 * ck_jpeg_luma_h(s) - 1) / (8 * ck_jpeg_luma_h(s));
        for (int ri : {0, 1, 5, row, 65535}) {
            walk_geometry(h, w, s, ri);
            std::vector<int16_t> c(2 * ncoef);
            for (int kind = 0; kind < 3; kind++) {
                std::vector<int16_t> one(ncoef);
                synthetic(kind, one);
                memcpy(c.data(), one.data(), ncoef * sizeof(int16_t));
                synthetic((kind + 1) % 3, one);
                memcpy(c.data() + ncoef, one.data(), ncoef * sizeof(int16_t));
                if (both(c.data(), 2, ncoef, quant, h, w, s, ri) != CK_OK) die("a synthetic case is refused");
            }
            for (int round = 0; round < 6; round++) {
                for (auto& v : c) {
                    const uint64_t r = next();
                    v = round == 0 ? (int16_t)((int)(r % 2047) - 1023)                                   // dense, inside the range
                      : round == 1 ? (int16_t)(r % 9 ? 0 : (int)((r >> 8) % 2047) - 1023)               // sparse: runs and ZRL
                      : round == 2 ? (int16_t)(r % 40 ? 0 : (int)((r >> 8) % 7) - 3)                    // very sparse: many blocks to a dword
                      : round == 3 ? (int16_t)(r % 3 ? 0 : ((r >> 8) & 1 ? 1023 : -1023))               // stuffed bytes
                      : round == 4 ? (int16_t)(r % 5000 ? (int)((r >> 8) % 63) - 31 : 1024)             // a few uncodable ones
                                   : (int16_t)r;                                                         // anything
                }
                const int rc = both(c.data(), 2, ncoef, quant, h, w, s, ri);
                if (round < 4 && rc != CK_OK) die("coefficients inside the baseline range are refused");
            }
        }
    }
    printf("jpeg staged encoder: %d cases, %ld batches equal to the plain coder (%ld accepted, %ld refused)\n", argc - 1, g_ok + g_refused, g_ok, g_refused);
    return 0;
}
