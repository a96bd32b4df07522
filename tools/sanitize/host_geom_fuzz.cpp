// CPU sanitizer harness for the host-side geometry of libck_hip.so (ck_host_geom.cpp: convex hull + float32
// rotating calipers, perspective transform, 3x3 inverse; the host decisions of k_board_lines: exact-area rounds, ranking
// and gate, Hough slab, peaks to lines).  Built with -fsanitize=address,undefined and fed
// degenerate and random point sets; GPU sanitizers are not available on the pool, so this is where the
// product's host C++ gets its memory / UB check.   tools/sanitize/run.sh builds and runs it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../camkifu_amd/csrc/ck_host_geom.h"      // (with camkifu_amd.h: ck_get_perspective_transform)

int main()
{
    std::mt19937 rng(20161001);
    long checks = 0;
    for (int trial = 0; trial < 20000; trial++) {
        const int kind = trial % 8;
        int n = 1 + (int)(rng() % (kind == 7 ? 4000 : 40));
        std::vector<int32_t> p((size_t)n * 2);
        for (int i = 0; i < n; i++) {
            int x = (int)(rng() % 2000), y = (int)(rng() % 1200);
            if (kind == 0) y = 7;                        // all on one horizontal line
            if (kind == 1) x = 13;                       // vertical line
            if (kind == 2) { x = 100; y = 100; }         // one repeated point
            if (kind == 3) y = x;                        // diagonal
            if (kind == 4) { x = (i % 2) * 50; y = (i / 2 % 2) * 30; }   // the 4 corners of a rectangle, repeated
            p[2 * i] = x; p[2 * i + 1] = y;
        }
        float wh[2] = {-1.f, -1.f};
        ck_min_area_rect(p.data(), n, wh);
        if (!(wh[0] >= 0.f && wh[1] >= 0.f) || std::isnan(wh[0]) || std::isnan(wh[1])) {
            fprintf(stderr, "bad rect %g x %g (kind %d, n %d)\n", wh[0], wh[1], kind, n);
            return 1;
        }
        checks++;
    }
    for (int trial = 0; trial < 20000; trial++) {
        float src[8], dst[8] = {0, 0, 380, 0, 380, 380, 0, 380};
        for (int i = 0; i < 8; i++) src[i] = (float)(rng() % 2000) / (trial % 3 == 0 ? 1.f : 7.f);
        if (trial % 5 == 0) { src[2] = src[0]; src[3] = src[1]; }       // two equal corners: degenerate
        double M[9], Mi[9];
        const int rc = ck_get_perspective_transform(src, dst, M);
        if (rc == 0) ck_invert3x3(M, Mi);
        checks++;
    }
    // component tables: random, empty frames, all-equal areas, nothing known, everything known; exactly sized arrays
    for (int trial = 0; trial < 20000; trial++) {
        const int kind = trial % 5;
        const int nc = kind == 0 ? 0 : 1 + (int)(rng() % (trial % 50 == 7 ? 3000 : 40));
        std::vector<int32_t> root((size_t)nc);
        std::vector<double> ub((size_t)nc), area((size_t)nc);
        std::vector<uint8_t> known((size_t)nc), want((size_t)nc);
        for (int s = 0; s < nc; s++) {
            root[s] = (int32_t)(rng() % 2000000);
            ub[s] = kind == 1 ? 4096. : (double)(rng() % 5000);
            area[s] = kind == 1 ? 2048. : (double)(rng() % 5000) * 0.5;
            known[s] = kind == 2 ? 0 : kind == 3 ? 1 : (uint8_t)(rng() & 1);
        }
        for (int round = 0; round < 3; round++) {
            std::fill(want.begin(), want.end(), 0);
            const int got = ck_board_round_want(round, nc, ub.data(), area.data(), known.data(), want.data());
            int marked = 0;
            for (int s = 0; s < nc; s++) {
                if (want[s] && known[s]) { fprintf(stderr, "round %d wants a known component\n", round); return 1; }
                marked += want[s];
                if (want[s]) known[s] = 1;
            }
            if (got != marked || (round == 0 && got > 16)) { fprintf(stderr, "round %d: %d wanted, %d marked\n", round, got, marked); return 1; }
        }
        int32_t sel[4];
        ck_board_result res = {CK_BOARD_LINES, nc, 0, 0, 0.};
        const int go = ck_board_rank(nc, root.data(), area.data(), known.data(), 40, 60, sel, &res);
        for (int i = 0; i < 3; i++)
            if (sel[i] < -1 || sel[i] >= nc || (!go && sel[i] != -1)) { fprintf(stderr, "bad selection %d (nc %d)\n", sel[i], nc); return 1; }
        if (go != sel[3] || (go && !(800. < res.biggest_area))) { fprintf(stderr, "bad gate\n"); return 1; }
        checks += 4;
    }
    // Hough slab: sides from 1 to beyond what fits; the slab never exceeds its LDS budget
    for (int trial = 0; trial < 20000; trial++) {
        const int n = 1 + (int)(rng() % 200), h = 1 + (int)(rng() % (trial % 4 ? 3000 : 70000)), w = 1 + (int)(rng() % (trial % 4 ? 5000 : 70000));
        size_t row_bytes = 0;
        int rb = 0, threads = 0;
        const int rc = ck_hough_slab(n, h, w, 32, 1024, &row_bytes, &rb, &threads);
        if (rc == 0 && (rb < 1 || rb > 10 || (rb + 2) * row_bytes > 144 * 1024 || (threads != 512 && threads != 1024))) {
            fprintf(stderr, "bad slab %d rows of %zu bytes, %d threads (%d x %d x %d)\n", rb, row_bytes, threads, n, h, w);
            return 1;
        }
        checks++;
    }
    // peaks: none, ties in count, cap below, at and above the peak count; the line buffer holds min(np, cap) lines exactly
    for (int trial = 0; trial < 20000; trial++) {
        const int h = 3 + (int)(rng() % 1200), w = 3 + (int)(rng() % 2000), numrho = 2 * (w + h) + 1;
        const int np = trial % 7 == 0 ? 0 : (int)(rng() % 300);
        const int cap = trial % 3 == 0 ? (int)(rng() % (np + 1)) : trial % 3 == 1 ? np : np + (int)(rng() % 50);
        std::vector<int32_t> pk((size_t)np * 2);
        for (int i = 0; i < np; i++) {
            pk[2 * i] = (1 + (int)(rng() % 180)) * (numrho + 2) + 1 + (int)(rng() % numrho);
            pk[2 * i + 1] = trial % 5 == 0 ? 40 : 1 + (int)(rng() % 20);
        }
        std::vector<float> lines((size_t)std::min(np, cap) * 2, -1.f);
        ck_peaks_to_lines(pk.data(), np, numrho, cap, lines.data());
        for (size_t i = 0; i < lines.size(); i += 2)
            if (!(std::fabs(lines[i]) <= (float)(w + h)) || !(lines[i + 1] >= 0.f && lines[i + 1] < 3.15f)) {
                fprintf(stderr, "bad line (%g, %g)\n", lines[i], lines[i + 1]);
                return 1;
            }
        checks++;
    }
    printf("host geometry: %ld calls clean under ASan/UBSan\n", checks);
    return 0;
}
