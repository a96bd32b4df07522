// png_inflate_fuzz.cpp -- the staged inflate (the text the GPU kernel of k_png_inflate.hip runs) under AddressSanitizer and
// UBSan: a stand-alone program that links csrc/ck_png.cpp alone (tests/test_png_inflate_sanitize_cpu.py builds and runs it).
//   png_inflate_fuzz [stride]
// ck_png_unzip_staged and ck_png_unzip must agree in status, bytes and message on
//   - the zlib streams of files the staged encoder writes in both of its modes: frames whose filtered bytes count just
//     below, at and above half a ring and a whole ring (16384 and 32768), inflated into exactly their room, into one byte
//     less and into none;
//   - every truncation and every single-byte change (^0x01, ^0x80, ^0xFF) of those streams.  `stride` thins that for the
//     streams of 2000 bytes and more (the 18 that cross half a ring and a ring) to every stride-th position, from a
//     phase that differs from stream to stream: the test runs the build under the sanitizers with stride 8 (every position
//     would take most of an hour there) and a second, plain -O2 build of this file with stride 1, which leaves nothing out.
//     The positions of a stream are dealt to up to 16 threads;
//   - random byte strings behind a valid wrapper, from a fixed seed, steered to every block type.
// A write outside the ring, the tables or the room given, or a loop that does not end, shows here before a GPU runs the text.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../../camkifu_amd/csrc/ck_png.h"
#include "../../camkifu_amd/csrc/ck_png_inflate_stage.h"

static std::atomic<long> g_streams{0}, g_refused{0};
static std::atomic<int> g_failed{0};

// both inflates on one stream with room for `cap` bytes: 0 when they agree
static int compare(const uint8_t* z, size_t zlen, size_t cap, const char* what)
{
    std::vector<uint8_t> a(cap), b(cap);                     // exactly the room: a write past it is seen
    size_t ta = 0, tb = 0;
    char ma[CK_PNG_MSG] = "", mb[CK_PNG_MSG] = "";
    CkInfRecord rec;
    const int ra = ck_png_unzip(z, zlen, cap ? a.data() : nullptr, cap, &ta, ma);
    const int rb = ck_png_unzip_staged(z, zlen, cap ? b.data() : nullptr, cap, &tb, &rec, mb);
    g_streams++;
    g_refused += ra != CK_OK;
    if (ra != rb || ta != tb || (ra != CK_OK && strcmp(ma, mb) != 0) || (ra == CK_OK && (rec.cause != CK_INF_OK || (size_t)rec.produced != ta))) {
        fprintf(stderr, "%s (%zu bytes, room %zu): host %d '%s' %zu, staged %d '%s' %zu\n", what, zlen, cap, ra, ma, ta, rb, mb, tb);
        return 1;
    }
    if (ra == CK_OK && cap && ta && memcmp(a.data(), b.data(), ta < cap ? ta : cap) != 0) { fprintf(stderr, "%s: the bytes differ\n", what); return 1; }
    return 0;
}

// truncations at, and the three changes of, the positions phase, phase + every, .. of z, dealt to the threads
static int damage(const std::vector<uint8_t>& z, size_t cap, size_t every, size_t phase)
{
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : nt > 16 ? 16 : nt;
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; t++)
        pool.emplace_back([&, t] {
            std::vector<uint8_t> m(z);
            for (size_t at = phase % every + t * every; at < z.size() && !g_failed; at += nt * every) {
                if (compare(z.data(), at, cap, "truncation")) g_failed = 1;
                for (uint8_t x : {0x01, 0x80, 0xFF}) {
                    m[at] ^= x;
                    if (compare(m.data(), m.size(), cap, "byte change")) g_failed = 1;
                    m[at] ^= x;
                }
            }
        });
    for (auto& th : pool) th.join();
    return g_failed;
}

int main(int argc, char** argv)
{
    const size_t every = argc > 1 && atoi(argv[1]) > 0 ? (size_t)atoi(argv[1]) : 1;     // (the stride of the large streams)
    size_t large = 0;
    // rows of 1 + 3 w bytes: 1024 for w = 341; 16 and 32 of them are half a ring and a ring
    const int shapes[][2] = {{1, 1}, {3, 5}, {4, 20}, {15, 341}, {16, 341}, {17, 341}, {16, 340}, {16, 342}, {31, 341}, {32, 341}, {33, 341}, {32, 342}};
    uint32_t seed = 2024;
    for (const auto& s : shapes) {
        const int h = s[0], w = s[1];
        std::vector<uint8_t> bgr((size_t)h * w * 3);
        for (size_t i = 0; i < bgr.size(); i++) {              // smooth runs with noise in them
            seed = seed * 1664525u + 1013904223u;
            bgr[i] = (uint8_t)((seed >> 24) % 5 ? (i / 60) * 3 : seed >> 16);
        }
        for (int runs = 0; runs < 2; runs++) {
            const size_t stride = ck_png_bound(h, w);
            std::vector<uint8_t> file(stride);
            size_t len = 0;
            char msg[CK_PNG_MSG];
            if (ck_png_stage_encode(bgr.data(), 1, h, w, -1, file.data(), stride, &len, msg, runs) != CK_OK) { fprintf(stderr, "encode %dx%d: %s\n", w, h, msg); return 1; }
            CkPngHead hd;
            if (ck_png_walk(file.data(), len, &hd, msg) != CK_OK) { fprintf(stderr, "walk %dx%d: %s\n", w, h, msg); return 1; }
            const std::vector<uint8_t> z(hd.z, hd.z + hd.zlen);
            const size_t need = hd.inflated();
            for (size_t cap : {need, need - 1, (size_t)0, need + 5})
                if (compare(z.data(), z.size(), cap, "round trip")) return 1;
            // the checks of the rows behind the inflate: the staged form with rows against ck_png_rows
            std::vector<uint8_t> rows(need), rows2(need);
            size_t total = 0;
            char m1[CK_PNG_MSG] = "", m2[CK_PNG_MSG] = "";
            const int r1 = ck_png_rows(hd, rows.data(), m1);
            const int r2 = ck_png_unzip_staged_rows(z.data(), z.size(), rows2.data(), need, &total, nullptr, m2, hd.h, (long long)hd.rowbytes);
            if (r1 != r2 || r1 != CK_OK || rows != rows2) { fprintf(stderr, "rows %dx%d: %d '%s', %d '%s'\n", w, h, r1, m1, r2, m2); return 1; }
            if (z.size() >= 2000) large++;
            if (damage(z, need, z.size() < 2000 ? 1 : every, 3 * large)) return 1;
        }
    }
    // random strings behind a valid wrapper: the first byte's low bits choose BFINAL and the block type
    for (int it = 0; it < 30000; it++) {
        seed = seed * 1664525u + 1013904223u;
        const size_t n = 2 + (seed >> 20) % 90;
        std::vector<uint8_t> z(n);
        z[0] = 0x78; z[1] = 0x9c;
        for (size_t i = 2; i < n; i++) { seed = seed * 1664525u + 1013904223u; z[i] = (uint8_t)(seed >> 24); }
        if (n > 2) z[2] = (uint8_t)((z[2] & ~7u) | (uint32_t)(it % 8));
        if (it % 8 < 2 && n > 7) { z[5] = (uint8_t)~z[3]; z[6] = (uint8_t)~z[4]; }      // a stored block whose LEN and NLEN agree
        if (compare(z.data(), z.size(), it % 3 ? 300 : 0, "random string")) return 1;
    }
    printf("png inflate: %ld streams (%ld refused) agree, %zu large streams at stride %zu, clean\n", g_streams.load(), g_refused.load(), large, every);
    return 0;
}
