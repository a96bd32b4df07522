// ck_overlay.cpp -- the host half of the overlay rasteriser: the limits of a display list, the per-primitive record, and
// the plan (which primitives can touch which bin of which frame, in list order).  ck_overlay_draw (ck_api.hip) runs
// exactly this plan; k_overlay.hip then tests pixels, never primitives, so a bounding box only has to be no smaller
// than the primitive.  Host only, free of HIP.
#include "ck_overlay.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/camkifu_amd.h"
#include "ck_font5x7.h"

// the library's error sink (ck_api.hip).  Weak: a program that links this file alone (tools/sanitize/overlay_fuzz.cpp)
// has none, and the status code is then all a refusal leaves.
int ck_fail(ck_ctx* ctx, int code, const char* fmt, ...) __attribute__((weak));

namespace {

int refuse(char* msg, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, CK_OV_MSG, fmt, ap);
    va_end(ap);
    return CK_ERR_ARG;
}

// the status goes back; the text goes to the library's error sink where there is one
int report(int code, const char* fmt, ...)
{
    char text[CK_OV_MSG + 32];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    return ck_fail ? ck_fail(nullptr, code, "%s", text) : code;
}

bool coord_ok(int32_t v) { return v >= -32767 && v <= 32767; }
bool thick_ok(int32_t t) { return t >= 1 && t <= 15 && (t & 1); }

int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

}  // namespace

int ck_overlay_check(int n, int h, int w, const int32_t* prims, const int32_t* frame_start, int text_len, char* msg)
{
    msg[0] = 0;
    if (n < 0 || text_len < 0) return refuse(msg, "n = %d, text_len = %d: negative", n, text_len);
    if (n == 0) return CK_OK;
    if (h <= 0 || w <= 0 || (long long)h * w > (1LL << 28)) return refuse(msg, "bad image shape h=%d w=%d", h, w);
    if (!frame_start) return refuse(msg, "frame_start is NULL");
    if (frame_start[0] != 0) return refuse(msg, "frame_start[0] is %d, not 0", frame_start[0]);
    for (int f = 0; f < n; f++)
        if (frame_start[f + 1] < frame_start[f])
            return refuse(msg, "frame_start goes backwards at frame %d: %d after %d", f, frame_start[f + 1], frame_start[f]);
    const int total = frame_start[n];
    if (total > 0 && !prims) return refuse(msg, "prims is NULL");
    for (int i = 0; i < total; i++) {
        const int32_t* p = prims + (size_t)i * CK_OV_PRIM;
        const int32_t kind = p[0], size = p[5];
        if (kind < CK_OV_SEGMENT || kind > CK_OV_TEXT) return refuse(msg, "primitive %d: unknown kind %d", i, kind);
        if (!coord_ok(p[1]) || !coord_ok(p[2])) return refuse(msg, "primitive %d: coordinate beyond +-32767", i);
        if (((uint32_t)p[6] >> 24) == 0) return refuse(msg, "primitive %d: alpha 0", i);
        switch (kind) {
        case CK_OV_SEGMENT:
            if (!coord_ok(p[3]) || !coord_ok(p[4])) return refuse(msg, "primitive %d: coordinate beyond +-32767", i);
            if (!thick_ok(size)) return refuse(msg, "primitive %d: thickness %d is not odd in 1 .. 15", i, size);
            break;
        case CK_OV_RECT:
            if (!coord_ok(p[3]) || !coord_ok(p[4])) return refuse(msg, "primitive %d: coordinate beyond +-32767", i);
            if (size < 0 || size > 65535) return refuse(msg, "primitive %d: rectangle thickness %d outside 0 .. 65535", i, size);
            break;
        case CK_OV_CIRCLE:
            if (!thick_ok(p[3])) return refuse(msg, "primitive %d: thickness %d is not odd in 1 .. 15", i, p[3]);
            [[fallthrough]];
        case CK_OV_DISC:
            if (size < 0 || size > 4095) return refuse(msg, "primitive %d: radius %d outside 0 .. 4095", i, size);
            break;
        case CK_OV_TEXT:
            if (size < 1 || size > 8) return refuse(msg, "primitive %d: text scale %d outside 1 .. 8", i, size);
            if (p[3] < 0 || p[7] < 0 || (long long)p[7] + p[3] > text_len)
                return refuse(msg, "primitive %d: text bytes %d + %d outside the %d given", i, p[7], p[3], text_len);
            break;
        }
    }
    return CK_OK;
}

void ck_overlay_record(const int32_t* p, int32_t* rec)
{
    memcpy(rec, p, CK_OV_PRIM * sizeof(int32_t));
    int64_t bx0 = p[1], by0 = p[2], bx1 = p[1], by1 = p[2];
    switch (p[0]) {
    case CK_OV_SEGMENT: {
        if (p[3] < p[1] || (p[3] == p[1] && p[4] < p[2])) { rec[1] = p[3]; rec[2] = p[4]; rec[3] = p[1]; rec[4] = p[2]; }
        const int hh = (p[5] - 1) / 2;
        bx0 = rec[1] - hh; bx1 = rec[3] + hh;
        by0 = (rec[2] < rec[4] ? rec[2] : rec[4]) - hh; by1 = (rec[2] < rec[4] ? rec[4] : rec[2]) + hh;
        break;
    }
    case CK_OV_RECT:
        if (p[3] < p[1]) { rec[1] = p[3]; rec[3] = p[1]; }
        if (p[4] < p[2]) { rec[2] = p[4]; rec[4] = p[2]; }
        bx0 = rec[1]; bx1 = rec[3]; by0 = rec[2]; by1 = rec[4];
        break;
    case CK_OV_CIRCLE: {
        const int outer = p[5] + (p[3] - 1) / 2, inner = p[5] - (p[3] + 1) / 2;
        rec[5] = outer; rec[3] = inner < 0 ? -1 : inner;
        bx0 -= outer; bx1 += outer; by0 -= outer; by1 += outer;
        break;
    }
    case CK_OV_DISC:
        bx0 -= p[5]; bx1 += p[5]; by0 -= p[5]; by1 += p[5];
        break;
    case CK_OV_TEXT:
        bx1 = bx0 + (int64_t)6 * p[5] * p[3] - 1;              // (no text: bx1 < bx0, the empty box)
        by1 = by0 + 8 * p[5] - 1;
        break;
    }
    const int64_t far = 1 << 30;
    rec[8] = (int32_t)clamp64(bx0, -far, far); rec[9] = (int32_t)clamp64(by0, -far, far);
    rec[10] = (int32_t)clamp64(bx1, -far, far); rec[11] = (int32_t)clamp64(by1, -far, far);
}

extern "C" {

int ck_overlay_plan(int n, int h, int w, const int32_t* prims, const int32_t* frame_start, int text_len,
                    int32_t* bin_size, int32_t* bin_start, int32_t* bin_prims, int cap, int32_t* n_refs)
{
    char msg[CK_OV_MSG];
    int rc = CK_OK;
    if (!bin_size || !n_refs) rc = refuse(msg, "bin_size or n_refs is NULL");
    else if (bin_prims && cap < 0) rc = refuse(msg, "cap = %d: negative", cap);
    else rc = ck_overlay_check(n, h, w, prims, frame_start, text_len, msg);
    if (rc != CK_OK) return report(rc, "ck_overlay_plan: %s", msg);
    *bin_size = CK_OV_BIN;
    *n_refs = 0;
    if (n == 0) {
        if (bin_start) bin_start[0] = 0;
        return CK_OK;
    }
    const int nbx = (w + CK_OV_BIN - 1) / CK_OV_BIN, nby = (h + CK_OV_BIN - 1) / CK_OV_BIN;
    const long long bins = (long long)n * nbx * nby;
    // two passes over the primitives, in list order: count per bin, then fill; so every bin's list ascends
    for (int pass = 0; pass < 2; pass++) {
        long long total = 0;
        int32_t* fill = nullptr;                    // pass 1: next free slot per bin
        if (pass == 1) {
            if (!bin_prims) return CK_OK;
            fill = (int32_t*)malloc((size_t)bins * sizeof(int32_t));
            if (!fill) return report(CK_ERR_STATE, "ck_overlay_plan: out of memory");
            memcpy(fill, bin_start, (size_t)bins * sizeof(int32_t));
        } else if (bin_start) {
            memset(bin_start, 0, ((size_t)bins + 1) * sizeof(int32_t));
        }
        for (int f = 0; f < n; f++) {
            const long long base = (long long)f * nbx * nby;
            for (int i = frame_start[f]; i < frame_start[f + 1]; i++) {
                int32_t rec[CK_OV_REC];
                ck_overlay_record(prims + (size_t)i * CK_OV_PRIM, rec);
                const int x0 = rec[8] < 0 ? 0 : rec[8], y0 = rec[9] < 0 ? 0 : rec[9];
                const int x1 = rec[10] > w - 1 ? w - 1 : rec[10], y1 = rec[11] > h - 1 ? h - 1 : rec[11];
                if (x0 > x1 || y0 > y1) continue;
                for (int by = y0 / CK_OV_BIN; by <= y1 / CK_OV_BIN; by++)
                    for (int bx = x0 / CK_OV_BIN; bx <= x1 / CK_OV_BIN; bx++) {
                        const long long b = base + (long long)by * nbx + bx;
                        if (pass == 0) { total++; if (bin_start) bin_start[b + 1]++; }
                        else bin_prims[fill[b]++] = i;
                    }
            }
        }
        if (pass == 1) { free(fill); break; }
        if (total > 0x7fffffffLL) return report(CK_ERR_ARG, "ck_overlay_plan: %lld bin entries: too many", total);
        *n_refs = (int32_t)total;
        if (bin_start)
            for (long long b = 0; b < bins; b++) bin_start[b + 1] += bin_start[b];
        if (!bin_start) return CK_OK;                           // sizes only
        if (bin_prims && cap < total)
            return report(CK_ERR_CAPACITY, "ck_overlay_plan: %lld bin entries, room for %d", total, cap);
    }
    return CK_OK;
}

int ck_overlay_glyph(int ch, uint8_t rows[7])
{
    if (!rows) return report(CK_ERR_ARG, "ck_overlay_glyph: rows is NULL");
    if (ch < 32 || ch > 126) ch = '?';
    memcpy(rows, ck_font5x7[ch - 32], 7);
    return CK_OK;
}

}  // extern "C"
