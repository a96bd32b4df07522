// jpeg_fuzz.cpp -- the host half of the JPEG decoder (camkifu_amd/csrc/ck_jpeg.cpp, linked on its own) under
// AddressSanitizer + UBSan: every case file given on the command line is decoded whole (must be CK_OK), truncated at
// every offset, and with a few thousand seeded single-byte mutations.  Each input lives in a heap block of exactly its
// size and the coefficients in one of exactly info.blocks * 64 values, so a read or write one byte outside either is
// caught; every status must be CK_OK or CK_ERR_DATA.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I include tools/sanitize/jpeg_fuzz.cpp camkifu_amd/csrc/ck_jpeg.cpp
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../camkifu_amd/csrc/ck_jpeg.h"

static long g_ok = 0, g_refused = 0;

// -> status of the whole decode; aborts the program on a status that must not occur
static int run(const uint8_t* src, size_t len)
{
    std::unique_ptr<uint8_t[]> data(new uint8_t[len ? len : 1]);
    memcpy(data.get(), src, len);
    auto f = std::make_unique<CkJpegFrame>();
    char msg[CK_JPEG_MSG];
    int rc = ck_jpeg_parse(data.get(), len, f.get(), msg);
    if (rc == CK_OK) {
        if (f->info.blocks > (1 << 16)) { g_refused++; return CK_ERR_DATA; }      // (a mutated size: the caller's geometry check refuses it)
        std::unique_ptr<int16_t[]> coef(new int16_t[(size_t)f->info.blocks * 64]);
        rc = ck_jpeg_entropy(data.get(), len, *f, coef.get(), msg);
    }
    if (rc != CK_OK && rc != CK_ERR_DATA) { fprintf(stderr, "status %d (%s)\n", rc, msg); exit(2); }
    if (rc != CK_OK && !msg[0]) { fprintf(stderr, "a refusal without a message\n"); exit(2); }
    (rc == CK_OK ? g_ok : g_refused)++;
    return rc;
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: jpeg_fuzz case.jpg ...\n"); return 2; }
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    for (int a = 1; a < argc; a++) {
        FILE* fp = fopen(argv[a], "rb");
        if (!fp) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> buf;
        uint8_t chunk[4096];
        for (size_t k; (k = fread(chunk, 1, sizeof chunk, fp)) > 0;) buf.insert(buf.end(), chunk, chunk + k);
        fclose(fp);
        if (run(buf.data(), buf.size()) != CK_OK) { fprintf(stderr, "%s does not decode\n", argv[a]); return 2; }
        for (size_t cut = 0; cut < buf.size(); cut++) run(buf.data(), cut);
        std::vector<uint8_t> m(buf);
        for (int k = 0; k < 3000; k++) {
            const size_t at = (size_t)(next() % buf.size());
            const uint8_t old = m[at];
            m[at] = (uint8_t)(next() >> 11);
            run(m.data(), m.size());
            m[at] = old;
        }
    }
    printf("jpeg host decoder: %d cases, %ld decodes clean (%ld accepted, %ld refused)\n", argc - 1, g_ok + g_refused, g_ok, g_refused);
    return 0;
}
