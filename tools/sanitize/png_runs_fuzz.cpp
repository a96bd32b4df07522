// png_runs_fuzz.cpp -- the staged PNG encoder in its runs mode under AddressSanitizer and UBSan: a stand-alone program that
// links csrc/ck_png.cpp alone (tests/test_png_runs_sanitize_cpu.py builds and runs it).
//   png_runs_fuzz
// Frames of sizes around the band and tile seams -- smooth ones with noise in them, all-zero ones, and rows that hold one run
// of every length around the limits of a match (3, 258 and their multiples) -- go through ck_png_stage_encode with runs on
// and every filter, into a buffer of exactly the bound; the reader inflates every file, and undoing the filters must give
// the frame back.  The literal-only mode must write what it writes without the parameter.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../camkifu_amd/csrc/ck_png.h"
#include "../../camkifu_amd/csrc/ck_png_stage.h"

static int g_files = 0;

// the frame (BGR) through the runs mode with `filter`, then back: 0 when the pixels return
static int round_trip(const std::vector<uint8_t>& bgr, int n, int h, int w, int filter)
{
    const size_t stride = ck_png_bound(h, w);
    std::vector<uint8_t> out((size_t)n * stride), plain((size_t)n * stride), same((size_t)n * stride);      // exactly the bound: a write past it is seen
    std::vector<size_t> len((size_t)n), len0((size_t)n), len1((size_t)n);
    char msg[CK_PNG_MSG];
    if (ck_png_stage_encode(bgr.data(), n, h, w, filter, out.data(), stride, len.data(), msg, 1) != CK_OK) { fprintf(stderr, "encode %dx%d: %s\n", w, h, msg); return 1; }
    if (ck_png_stage_encode(bgr.data(), n, h, w, filter, plain.data(), stride, len0.data(), msg) != CK_OK ||
        ck_png_stage_encode(bgr.data(), n, h, w, filter, same.data(), stride, len1.data(), msg, 0) != CK_OK) { fprintf(stderr, "encode %dx%d: %s\n", w, h, msg); return 1; }
    for (int f = 0; f < n; f++) {
        if (len0[f] != len1[f] || memcmp(plain.data() + f * stride, same.data() + f * stride, len0[f]) != 0) { fprintf(stderr, "%dx%d: the default mode moved\n", w, h); return 1; }
        CkPngHead hd;
        if (ck_png_walk(out.data() + f * stride, len[f], &hd, msg) != CK_OK) { fprintf(stderr, "walk %dx%d: %s\n", w, h, msg); return 1; }
        // the library's inflate on the zlib stream alone, into exactly the room the rows need
        std::vector<uint8_t> rows(hd.inflated());
        size_t total = 0;
        if (ck_png_unzip(hd.z, hd.zlen, rows.data(), rows.size(), &total, msg) != CK_OK || total != rows.size()) {
            fprintf(stderr, "inflate %dx%d filter %d: %s (%zu of %zu bytes)\n", w, h, filter, msg, total, rows.size());
            return 1;
        }
        if (hd.h != h || hd.w != w || hd.color_type != 2 || hd.bit_depth != 8 || ck_png_rows(hd, rows.data(), msg) != CK_OK) { fprintf(stderr, "rows %dx%d: %s\n", w, h, msg); return 1; }
        const size_t rb = 3 * (size_t)w;
        std::vector<uint8_t> prev(rb, 0), cur(rb, 0);
        for (int y = 0; y < h; y++) {
            const uint8_t* r = rows.data() + (size_t)y * (rb + 1);
            if (filter >= 0 && r[0] != filter) { fprintf(stderr, "row %d has filter %d, not %d\n", y, r[0], filter); return 1; }
            for (size_t i = 0; i < rb; i++) {
                const int a = i >= 3 ? cur[i - 3] : 0, c = i >= 3 ? prev[i - 3] : 0;
                cur[i] = (uint8_t)(r[1 + i] + ck_png_predict(r[0], a, prev[i], c));
                if (cur[i] != bgr[((size_t)f * h + y) * rb + (i / 3) * 3 + 2 - i % 3]) { fprintf(stderr, "%dx%d filter %d: pixel byte %zu of row %d differs\n", w, h, filter, i, y); return 1; }
            }
            prev = cur;
        }
        g_files++;
    }
    return 0;
}

int main()
{
    const int shapes[][2] = {{1, 1}, {1, 17}, {17, 1}, {15, 6}, {16, 6}, {17, 6}, {33, 5}, {5, 341}, {5, 342}, {20, 40}, {35, 50}, {64, 64}};
    uint32_t seed = 12345;
    for (const auto& s : shapes) {
        const int h = s[0], w = s[1], n = 2;
        std::vector<uint8_t> bgr((size_t)n * h * w * 3);
        for (size_t i = 0; i < bgr.size() / 2; i++) {          // frame 0: smooth runs with noise in them; frame 1: zeros
            seed = seed * 1664525u + 1013904223u;
            bgr[i] = (uint8_t)((seed >> 24) % 7 ? (i / 96) * 3 : seed >> 16);
        }
        for (int filter = -1; filter <= 4; filter++)
            if (round_trip(bgr, n, h, w, filter)) return 1;
    }
    // one row of 342 pixels, 1026 bytes without equal neighbours, and in it a run of sevens of every length in turn
    const int lengths[] = {1, 2, 3, 4, 5, 258, 259, 260, 261, 262, 263, 516, 517, 518, 519, 520};
    for (int run : lengths) {
        std::vector<uint8_t> rgb(1026), bgr(1026);
        for (size_t i = 0; i < rgb.size(); i++) rgb[i] = (uint8_t)(8 + (i * 37) % 241 + (i % 2));
        for (int i = 0; i < run; i++) rgb[100 + i] = 7;
        for (size_t i = 0; i < rgb.size(); i++) bgr[(i / 3) * 3 + 2 - i % 3] = rgb[i];
        for (int filter : {-1, 0, 4})
            if (round_trip(bgr, 1, 1, 342, filter)) return 1;
    }
    printf("png runs encoder: %d files round trip, clean\n", g_files);
    return 0;
}
