// jpeg_enc_fuzz.cpp -- the host half of the JPEG encoder (camkifu_amd/csrc/ck_jpeg_enc.cpp, linked with ck_jpeg.cpp and
// nothing else) under AddressSanitizer + UBSan.  Every case file given on the command line is a JPEG stream: it is decoded
// to coefficients, encoded again with its own tables and restart interval (must give the file's bytes back), and every
// stream the encoder writes is parsed and decoded again and the coefficients compared.  Then hostile coefficients over
// the case's geometry: +-32767 everywhere, random int16, random values inside the baseline range, at qualities 1 .. 100
// and restart intervals 0, 1 and 7 -- each must be refused with CK_ERR_ARG and a message, or encoded within the bound and
// decode back to itself.  The output lives in a heap block of exactly the bound, and in smaller ones (every size up to the
// headers', then some larger): a write one byte past it is caught, and a block below the bound must never be overrun.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I include tools/sanitize/jpeg_enc_fuzz.cpp \
//       camkifu_amd/csrc/ck_jpeg_enc.cpp camkifu_amd/csrc/ck_jpeg.cpp
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../camkifu_amd/csrc/ck_jpeg_enc.h"

static long g_ok = 0, g_refused = 0;

static void die(const char* what) { fprintf(stderr, "%s\n", what); exit(2); }

// encode into a block of exactly `cap` bytes; an accepted stream is decoded again and must give the coefficients back
static int run(const int16_t* coef, size_t ncoef, const uint16_t* quant, int h, int w, int sampling, int ri, size_t cap,
               std::vector<uint8_t>* keep = nullptr)
{
    std::unique_ptr<uint8_t[]> out(new uint8_t[cap ? cap : 1]);
    size_t len = 0;
    char msg[CK_JPEG_MSG];
    const int rc = ck_jpeg_enc_entropy(coef, quant, h, w, sampling, ri, out.get(), cap, &len, msg);
    if (rc != CK_OK && rc != CK_ERR_ARG) die("a status other than CK_OK / CK_ERR_ARG");
    if (rc != CK_OK) {
        if (!msg[0]) die("a refusal without a message");
        g_refused++;
        return rc;
    }
    if (len > cap || len > ck_jpeg_enc_bound(h, w, sampling)) die("a stream longer than its buffer or the bound");
    auto f = std::make_unique<CkJpegFrame>();
    std::unique_ptr<uint8_t[]> exact(new uint8_t[len]);
    memcpy(exact.get(), out.get(), len);
    if (ck_jpeg_parse(exact.get(), len, f.get(), msg) != CK_OK) die("the decoder refuses the encoder's headers");
    if (f->info.h != h || f->info.w != w || f->info.sampling != sampling || f->info.restart_interval != ri ||
        (size_t)f->info.blocks * 64 != ncoef)
        die("the headers say another geometry");
    for (int c = 0; c < f->ncomp; c++)
        if (memcmp(f->quant[c], quant + 64 * c, 64 * sizeof(uint16_t)) != 0) die("the headers hold other quant tables");
    std::unique_ptr<int16_t[]> back(new int16_t[ncoef]);
    if (ck_jpeg_entropy(exact.get(), len, *f, back.get(), msg) != CK_OK) die("the decoder refuses the encoder's scan");
    if (memcmp(back.get(), coef, ncoef * sizeof(int16_t)) != 0) die("the coefficients do not come back");
    if (keep) keep->assign(exact.get(), exact.get() + len);
    g_ok++;
    return rc;
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: jpeg_enc_fuzz case.jpg ...\n"); return 2; }
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
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
        const size_t ncoef = (size_t)f->info.blocks * 64, bound = ck_jpeg_enc_bound(h, w, s);
        std::vector<int16_t> coef(ncoef);
        if (ck_jpeg_entropy(buf.data(), buf.size(), *f, coef.data(), msg) != CK_OK) { fprintf(stderr, "%s: %s\n", argv[a], msg); return 2; }
        uint16_t quant[192];
        memcpy(quant, f->quant, sizeof quant);
        if (s == CK_JPEG_GREY) for (int i = 64; i < 192; i++) quant[i] = quant[i - 64];
        // the case itself: the file's bytes come back
        std::vector<uint8_t> again;
        if (run(coef.data(), ncoef, quant, h, w, s, ri, bound, &again) != CK_OK) { fprintf(stderr, "%s is refused\n", argv[a]); return 2; }
        if (again != buf) { fprintf(stderr, "%s: other bytes than the file's\n", argv[a]); return 2; }
        // buffers below the bound: refused or written inside them, never overrun
        for (size_t cap = 0; cap < 1100; cap++) run(coef.data(), ncoef, quant, h, w, s, ri, cap);
        for (size_t cap = 1100; cap < bound; cap += 1 + cap / 16) run(coef.data(), ncoef, quant, h, w, s, ri, cap);
        // bad arguments
        if (run(coef.data(), ncoef, quant, 0, w, s, ri, bound) == CK_OK || run(coef.data(), ncoef, quant, h, 65536, s, ri, bound) == CK_OK ||
            run(coef.data(), ncoef, quant, h, w, 4, ri, bound) == CK_OK || run(coef.data(), ncoef, quant, h, w, s, 65536, bound) == CK_OK)
            die("a bad argument is accepted");
        uint16_t zq[192];
        memcpy(zq, quant, sizeof zq);
        zq[5] = 0;
        if (run(coef.data(), ncoef, zq, h, w, s, ri, bound) == CK_OK) die("a zero quant entry is accepted");
        // hostile coefficients
        std::vector<int16_t> hostile(ncoef);
        for (int sign = -1; sign <= 1; sign += 2) {
            for (auto& v : hostile) v = (int16_t)(sign * 32767);
            if (run(hostile.data(), ncoef, quant, h, w, s, 0, bound) == CK_OK) die("+-32767 everywhere is accepted");
        }
        for (int round = 0; round < 40; round++) {
            ck_jpeg_enc_quant((int)(next() % 100) + 1, quant);
            const int r = round % 3 == 0 ? 0 : (round % 3 == 1 ? 1 : 7);
            for (auto& v : hostile) v = (int16_t)next();
            run(hostile.data(), ncoef, quant, h, w, s, r, bound);
            // inside the range of the baseline tables: AC within +-1023, DC within +-1023 so that differences have 11 bits
            for (auto& v : hostile) v = (int16_t)((int)(next() % 2047) - 1023);
            if (run(hostile.data(), ncoef, quant, h, w, s, r, bound) != CK_OK) die("coefficients inside the baseline range are refused");
            // the worst case of the bound: every AC value of 10 bits behind the longest codes, alternating signs
            for (size_t i = 0; i < ncoef; i++) hostile[i] = (int16_t)((i & 1) ? 1023 : -1023);
            if (run(hostile.data(), ncoef, quant, h, w, s, r, bound) != CK_OK) die("the worst case is refused");
        }
    }
    printf("jpeg host encoder: %d cases, %ld encodes clean (%ld accepted, %ld refused)\n", argc - 1, g_ok + g_refused, g_ok, g_refused);
    return 0;
}
