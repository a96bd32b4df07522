// overlay_fuzz.cpp -- hostile display lists through ck_overlay_plan under AddressSanitizer + UBSan.  A stand-alone program:
// it links camkifu_amd/csrc/ck_overlay.cpp alone (tests/test_overlay_sanitize_cpu.py builds and runs it).
//   - every field of a primitive pushed to and past its limits, INT32_MIN / INT32_MAX included
//   - text offsets and lengths out of range, frame_start going backwards, not starting at 0, pointing past the list
//   - cap of 0 and of one short: CK_ERR_CAPACITY with the size needed, nothing written
//   - random lists: whatever the plan accepts is planned into exactly sized buffers, and every entry is checked
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "camkifu_amd.h"

static int failures = 0;
#define EXPECT(cond)                                                           \
    do {                                                                       \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static uint32_t rng_state = 20161001u;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state;
}

static const int32_t EDGES[] = {INT32_MIN, INT32_MIN + 1, -65536, -32768, -32767, -4096, -16, -1, 0, 1, 2, 7, 8, 9, 15, 16, 17, 255,
                                4095, 4096, 32767, 32768, 65535, 65536, INT32_MAX - 1, INT32_MAX};
static const int N_EDGES = sizeof EDGES / sizeof EDGES[0];

// plans a list into buffers of exactly the size the plan asks for (ASan watches both ends) -> the status
static int plan_exact(int n, int h, int w, const std::vector<int32_t>& prims, const std::vector<int32_t>& start, int text_len, long* refs_out)
{
    int32_t bin = 0, refs = -1;
    int rc = ck_overlay_plan(n, h, w, prims.data(), start.data(), text_len, &bin, nullptr, nullptr, 0, &refs);
    if (rc != CK_OK) return rc;
    EXPECT(bin > 0 && refs >= 0);
    const long bins = n == 0 ? 0 : (long)n * ((h + bin - 1) / bin) * ((w + bin - 1) / bin);
    std::vector<int32_t> bin_start((size_t)bins + 1, -1);
    int32_t* bin_prims = (int32_t*)malloc(refs > 0 ? (size_t)refs * sizeof(int32_t) : 1);
    int32_t refs2 = -1;
    rc = ck_overlay_plan(n, h, w, prims.data(), start.data(), text_len, &bin, bin_start.data(), bin_prims, refs, &refs2);
    EXPECT(rc == CK_OK && refs2 == refs && bin_start[0] == 0 && bin_start[(size_t)bins] == refs);
    for (long b = 0; b < bins && n > 0; b++) {
        const int f = (int)(b / (bins / n));
        EXPECT(bin_start[b] <= bin_start[b + 1]);
        for (int32_t j = bin_start[b]; j < bin_start[b + 1]; j++) {
            EXPECT(bin_prims[j] >= start[f] && bin_prims[j] < start[f + 1]);
            EXPECT(j == bin_start[b] || bin_prims[j - 1] < bin_prims[j]);
        }
    }
    if (refs > 0) {                                           // cap of 0 and of one short: the size needed, nothing written
        const int caps[2] = {0, refs - 1};
        for (int cap : caps) {
            int32_t* small_buf = (int32_t*)malloc(cap > 0 ? (size_t)cap * sizeof(int32_t) : 1);
            int32_t need = -1;
            EXPECT(ck_overlay_plan(n, h, w, prims.data(), start.data(), text_len, &bin, bin_start.data(), small_buf, cap, &need) == CK_ERR_CAPACITY);
            EXPECT(need == refs);
            free(small_buf);
        }
        int32_t need = -1;
        EXPECT(ck_overlay_plan(n, h, w, prims.data(), start.data(), text_len, &bin, bin_start.data(), bin_prims, -1, &need) == CK_ERR_ARG);
    }
    free(bin_prims);
    if (refs_out) *refs_out += refs;
    return CK_OK;
}

int main()
{
    long planned = 0, refused = 0, refs = 0;
    // one field at a time at every edge value, for every kind (and the kinds around the valid ones)
    for (int kind = -1; kind <= 7; kind++)
        for (int field = 1; field < 8; field++)
            for (int e = 0; e < N_EDGES; e++) {
                std::vector<int32_t> prims = {kind, 5, 6, 9, 3, 1, (int32_t)0xff102030u, 0};
                if (kind == CK_OV_CIRCLE) prims[3] = 3;
                prims[(size_t)field] = EDGES[e];
                const int rc = plan_exact(1, 40, 70, prims, {0, 1}, 12, &refs);
                EXPECT(rc == CK_OK || rc == CK_ERR_ARG);
                (rc == CK_OK ? planned : refused)++;
            }
    // frame_start: backwards, not from 0, negative, past the list (the list is as long as frame_start says: a liar's list
    // is the caller's fault, a non-monotone one is refused)
    {
        std::vector<int32_t> prims;
        for (int i = 0; i < 4; i++) { const int32_t p[8] = {CK_OV_DISC, 10 * i, 10, 0, 0, 4, -1, 0}; prims.insert(prims.end(), p, p + 8); }
        EXPECT(plan_exact(3, 40, 70, prims, {0, 2, 2, 4}, 0, &refs) == CK_OK);
        EXPECT(plan_exact(3, 40, 70, prims, {0, 3, 2, 4}, 0, nullptr) == CK_ERR_ARG);
        EXPECT(plan_exact(3, 40, 70, prims, {1, 2, 3, 4}, 0, nullptr) == CK_ERR_ARG);
        EXPECT(plan_exact(3, 40, 70, prims, {0, -1, 2, 4}, 0, nullptr) == CK_ERR_ARG);
        EXPECT(plan_exact(3, 40, 70, prims, {0, 4, 4, INT32_MIN}, 0, nullptr) == CK_ERR_ARG);
        EXPECT(plan_exact(-1, 40, 70, prims, {0}, 0, nullptr) == CK_ERR_ARG);
        EXPECT(plan_exact(1, 0, 70, prims, {0, 1}, 0, nullptr) == CK_ERR_ARG);
        EXPECT(plan_exact(1, 40, -3, prims, {0, 1}, 0, nullptr) == CK_ERR_ARG);
        EXPECT(plan_exact(1, 1 << 20, 1 << 20, prims, {0, 1}, 0, nullptr) == CK_ERR_ARG);
        EXPECT(plan_exact(1, 40, 70, prims, {0, 1}, -1, nullptr) == CK_ERR_ARG);
        EXPECT(plan_exact(0, 0, 0, {}, {0}, 0, &refs) == CK_OK);
        int32_t bin = 0, n_refs = 0;
        EXPECT(ck_overlay_plan(1, 40, 70, nullptr, nullptr, 0, &bin, nullptr, nullptr, 0, &n_refs) == CK_ERR_ARG);
        const int32_t one[2] = {0, 1};
        EXPECT(ck_overlay_plan(1, 40, 70, nullptr, one, 0, &bin, nullptr, nullptr, 0, &n_refs) == CK_ERR_ARG);
        EXPECT(ck_overlay_plan(1, 40, 70, prims.data(), one, 0, nullptr, nullptr, nullptr, 0, &n_refs) == CK_ERR_ARG);
        EXPECT(ck_overlay_plan(1, 40, 70, prims.data(), one, 0, &bin, nullptr, nullptr, 0, nullptr) == CK_ERR_ARG);
    }
    // text ranges around the end of the byte string
    for (int len = -1; len <= 13; len++)
        for (int off = -1; off <= 13; off++) {
            const int rc = plan_exact(1, 40, 70, {CK_OV_TEXT, -3, 2, len, 0, 2, -1, off}, {0, 1}, 12, &refs);
            EXPECT(rc == ((len >= 0 && off >= 0 && len + off <= 12) ? CK_OK : CK_ERR_ARG));
        }
    EXPECT(plan_exact(1, 40, 70, {CK_OV_TEXT, 0, 0, INT32_MAX, 0, 8, -1, 0}, {0, 1}, INT32_MAX, &refs) == CK_OK);
    EXPECT(plan_exact(1, 40, 70, {CK_OV_TEXT, 0, 0, INT32_MAX, 0, 8, -1, 1}, {0, 1}, INT32_MAX, nullptr) == CK_ERR_ARG);
    // random lists over several frames and shapes, valid fields mixed with edge values
    for (int round = 0; round < 400; round++) {
        const int n = 1 + (int)(rnd() % 3), h = 1 + (int)(rnd() % 90), w = 1 + (int)(rnd() % 130);
        std::vector<int32_t> prims, start = {0};
        for (int f = 0; f < n; f++) {
            const int count = (int)(rnd() % 12);
            for (int i = 0; i < count; i++) {
                const int kind = 1 + (int)(rnd() % 5);
                int32_t p[8] = {kind, (int32_t)(rnd() % 300) - 100, (int32_t)(rnd() % 300) - 100, (int32_t)(rnd() % 300) - 100,
                                (int32_t)(rnd() % 300) - 100, 1 + 2 * (int32_t)(rnd() % 8), (int32_t)(rnd() | 0x01000000u), 0};
                if (kind == CK_OV_CIRCLE) p[3] = 1 + 2 * (int32_t)(rnd() % 8);
                if (kind == CK_OV_TEXT) { p[3] = (int32_t)(rnd() % 9); p[5] = 1 + (int32_t)(rnd() % 8); p[7] = (int32_t)(rnd() % 4); }
                if (rnd() % 16 == 0) p[1 + rnd() % 7] = EDGES[rnd() % N_EDGES];
                prims.insert(prims.end(), p, p + 8);
            }
            start.push_back((int32_t)(prims.size() / 8));
        }
        const int rc = plan_exact(n, h, w, prims, start, 12, &refs);
        EXPECT(rc == CK_OK || rc == CK_ERR_ARG);
        (rc == CK_OK ? planned : refused)++;
    }
    // the glyphs: every byte, and the ones without a glyph
    uint8_t rows[7], question[7];
    EXPECT(ck_overlay_glyph('?', question) == CK_OK);
    for (int ch = -300; ch <= 300; ch++) {
        EXPECT(ck_overlay_glyph(ch, rows) == CK_OK);
        bool same = true;
        for (int k = 0; k < 7; k++) same = same && rows[k] == question[k];
        EXPECT(same == (ch < 32 || ch > 126 || ch == '?'));
    }
    EXPECT(ck_overlay_glyph('A', nullptr) == CK_ERR_ARG);
    EXPECT(planned > 300 && refused > 300 && refs > 1000);
    if (failures) { printf("overlay plan: %d FAILURES\n", failures); return 1; }
    printf("overlay plan: %ld lists planned (%ld bin entries), %ld refused: clean\n", planned, refs, refused);
    return 0;
}
