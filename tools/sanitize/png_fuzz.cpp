// png_fuzz.cpp -- the host half of the PNG reader and writer under AddressSanitizer and UBSan: a stand-alone program that
// links csrc/ck_png.cpp alone (tests/test_png_sanitize_cpu.py builds and runs it).
//   png_fuzz FILE...     *.z: a zlib stream, *.png: a PNG file
// Every file goes through the reader whole, cut at every length and with three single-byte changes at every offset (xor 01,
// 80, FF); a zlib stream is inflated into no room, little room and all the room it needs, and what comes out must not
// depend on the room.  Then the staged encoder writes frames of sizes around its band and tile seams with every filter,
// and the reader must give the pixels back.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../camkifu_amd/csrc/ck_png.h"
#include "../../camkifu_amd/csrc/ck_png_stage.h"

static std::vector<uint8_t> slurp(const char* path)
{
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    uint8_t buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

static long long g_runs = 0, g_refused = 0;

// a heap copy of exactly n bytes, so that a read past the end is seen
static void one_zlib(const uint8_t* p, size_t n)
{
    std::vector<uint8_t> in(p, p + n);
    char msg[CK_PNG_MSG];
    size_t total = 0;
    const int rc0 = ck_png_unzip(in.data(), n, nullptr, 0, &total, msg);
    g_runs++;
    if (rc0 != CK_OK) g_refused++;
    const size_t caps[3] = {7, total / 2, total};
    for (size_t cap : caps) {
        std::vector<uint8_t> out(cap);
        size_t t2 = 0;
        const int rc = ck_png_unzip(in.data(), n, out.data(), cap, &t2, msg);
        if (rc != rc0 || (rc == CK_OK && t2 != total)) { fprintf(stderr, "the verdict depends on the room: %d / %d, %zu / %zu\n", rc0, rc, total, t2); exit(1); }
    }
}

static void one_png(const uint8_t* p, size_t n)
{
    std::vector<uint8_t> in(p, p + n);
    char msg[CK_PNG_MSG];
    CkPngHead hd;
    g_runs++;
    if (ck_png_walk(in.data(), n, &hd, msg) != CK_OK) { g_refused++; return; }
    std::vector<uint8_t> rows(hd.inflated());
    if (ck_png_rows(hd, rows.data(), msg) != CK_OK) g_refused++;
}

static void every_damage(const std::vector<uint8_t>& v, void (*one)(const uint8_t*, size_t))
{
    one(v.data(), v.size());
    const size_t step = v.size() > 4096 ? v.size() / 512 : 1;      // (a long file: 512 offsets spread over it)
    for (size_t cut = 0; cut < v.size(); cut += step) one(v.data(), cut);
    std::vector<uint8_t> m = v;
    for (size_t at = 0; at < v.size(); at += step)
        for (uint8_t x : {(uint8_t)0x01, (uint8_t)0x80, (uint8_t)0xFF}) {
            m[at] = v[at] ^ x;
            one(m.data(), m.size());
            m[at] = v[at];
        }
}

static int encoder_round_trips()
{
    const int shapes[][2] = {{1, 1}, {1, 17}, {17, 1}, {15, 6}, {16, 6}, {17, 6}, {33, 5}, {5, 341}, {5, 342}, {40, 90}};
    int files = 0;
    uint32_t seed = 12345;
    for (const auto& s : shapes) {
        const int h = s[0], w = s[1], n = 2;
        std::vector<uint8_t> bgr((size_t)n * h * w * 3);
        for (size_t i = 0; i < bgr.size(); i++) {
            seed = seed * 1664525u + 1013904223u;
            bgr[i] = (uint8_t)((seed >> 24) % 7 ? (i / 3) * 3 + (seed >> 29) : seed >> 16);       // smooth runs with noise in them
        }
        const size_t stride = ck_png_bound(h, w);
        std::vector<uint8_t> out((size_t)n * stride);          // exactly the bound: a write past it is seen
        for (int filter = -1; filter <= 4; filter++) {
            size_t len[2] = {0, 0};
            char msg[CK_PNG_MSG];
            if (ck_png_stage_encode(bgr.data(), n, h, w, filter, out.data(), stride, len, msg) != CK_OK) { fprintf(stderr, "encode %dx%d: %s\n", w, h, msg); return 1; }
            for (int f = 0; f < n; f++) {
                CkPngHead hd;
                if (ck_png_walk(out.data() + f * stride, len[f], &hd, msg) != CK_OK) { fprintf(stderr, "walk %dx%d: %s\n", w, h, msg); return 1; }
                std::vector<uint8_t> rows(hd.inflated());
                if (hd.h != h || hd.w != w || hd.color_type != 2 || hd.bit_depth != 8 || ck_png_rows(hd, rows.data(), msg) != CK_OK) {
                    fprintf(stderr, "rows %dx%d filter %d: %s\n", w, h, filter, msg);
                    return 1;
                }
                // undo the filters byte by byte and compare with the frame
                const size_t rb = 3 * (size_t)w;
                std::vector<uint8_t> prev(rb, 0), cur(rb, 0);
                for (int y = 0; y < h; y++) {
                    const uint8_t* r = rows.data() + (size_t)y * (rb + 1);
                    if (filter >= 0 && r[0] != filter) { fprintf(stderr, "row %d has filter %d, not %d\n", y, r[0], filter); return 1; }
                    for (size_t i = 0; i < rb; i++) {
                        const int a = i >= 3 ? cur[i - 3] : 0, c = i >= 3 ? prev[i - 3] : 0;
                        cur[i] = (uint8_t)(r[1 + i] + ck_png_predict(r[0], a, prev[i], c));
                        if (cur[i] != bgr[((size_t)f * h + y) * rb + (i / 3) * 3 + 2 - i % 3]) { fprintf(stderr, "pixel byte %zu of row %d differs\n", i, y); return 1; }
                    }
                    prev = cur;
                }
                files++;
            }
        }
    }
    printf("png encoder: %d files round trip\n", files);
    return 0;
}

int main(int argc, char** argv)
{
    int cases = 0;
    for (int i = 1; i < argc; i++) {
        const std::string path = argv[i];
        const std::vector<uint8_t> v = slurp(argv[i]);
        const bool z = path.size() > 2 && path.compare(path.size() - 2, 2, ".z") == 0;
        every_damage(v, z ? one_zlib : one_png);
        cases++;
    }
    printf("png reader: %d cases, %lld runs, %lld refused, clean\n", cases, g_runs, g_refused);
    return encoder_round_trips();
}
