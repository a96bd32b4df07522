// ck_jpeg_span.cpp -- the steps of ck_jpeg_span.h on the host, in the order and on the staged layout the GPU runs them
// (jpeg_huff_pass in ck_api_jpeg.hip, k_jpeg_span.hip): one loop where the device has one launch.  Plain C++: no HIP, no context;
// tools/sanitize/jpeg_span_fuzz.cpp links it with ck_jpeg.cpp and ck_jpeg_plan.cpp on its own.
#include "ck_jpeg_span.h"
#include "ck_jpeg_tables.h"

#include <stdio.h>
#include <string.h>

#include <memory>

void ck_jpeg_span_host_wording(const uint8_t* data, size_t len, const ck_jpeg_info& geom, char* msg)
{
    auto fr = std::make_unique<CkJpegFrame>();
    char why[CK_JPEG_MSG] = {0};
    int rc = ck_jpeg_parse(data, len, fr.get(), why);
    if (rc == CK_OK && (fr->info.h != geom.h || fr->info.w != geom.w || fr->info.sampling != geom.sampling)) return;   // (the planner's wording is the host's)
    if (rc == CK_OK) {
        std::vector<int16_t> coef((size_t)fr->info.blocks * 64);
        rc = ck_jpeg_entropy(data, len, *fr, coef.data(), why);
    }
    if (rc != CK_OK) memcpy(msg, why, CK_JPEG_MSG);
}

int ck_jpeg_spans_host(const uint8_t* const* data, const size_t* len, int n, const ck_jpeg_info& geom, int span_bytes, int16_t* coef,
                       uint16_t* quant, int* bad, char* msg, long long* stats)
{
    for (int i = 0; i < CK_SPAN_STATS; i++) stats[i] = 0;
    CkJpegPlan plan;
    const int prc = ck_jpeg_plan_build(data, len, n, geom, &plan);
    if (prc != CK_OK && prc != CK_ERR_DATA) { *bad = plan.frames; memcpy(msg, plan.msg, CK_JPEG_MSG); return prc; }
    const size_t cframe = (size_t)geom.blocks * 64;
    const size_t ns = plan.strands.size();
    memset(coef, 0, (size_t)plan.frames * cframe * sizeof(int16_t));
    std::vector<uint32_t> status(ns, 0);
    if (ns) {
        // the staged block: every frame's entropy-coded segment, one behind the other
        std::vector<size_t> seg((size_t)plan.frames);
        size_t at = 0;
        for (int f = 0; f < plan.frames; f++) { seg[f] = at; at += len[f] - plan.scan[f]; }
        std::vector<uint8_t> bytes(at ? at : 1, 0);               // (no slack behind: a read past the last byte is one past the block)
        for (int f = 0; f < plan.frames; f++) memcpy(bytes.data() + seg[f], data[f] + plan.scan[f], len[f] - plan.scan[f]);
        std::vector<CkStrand> rows(plan.strands);
        std::vector<int32_t> span0(ns + 1, 0);
        for (size_t s = 0; s < ns; s++) {
            const int64_t shift = (int64_t)seg[(size_t)rows[s].frame] - (int64_t)plan.scan[(size_t)rows[s].frame];
            rows[s].begin += shift;
            rows[s].end += shift;
            span0[s + 1] = span0[s] + (int32_t)ck_span_count(rows[s].end - rows[s].begin, span_bytes);
        }
        const size_t spans = (size_t)span0[ns];
        CkSpanJob J{};
        J.bytes = bytes.data(); J.n_bytes = (long long)at;
        J.rows = rows.data(); J.n_strands = (int)ns;
        J.span0 = span0.data();
        J.sets = plan.sets.data(); J.n_sets = (int)plan.sets.size();
        J.g = plan.g; J.cframe = (long long)cframe; J.n_frames = plan.frames; J.span_bytes = span_bytes; J.bpm = ck_span_bpm(plan.g);
        std::vector<uint64_t> cand_a(spans * J.bpm), cand_x(spans * J.bpm), entry(spans);
        std::vector<uint32_t> cand_c(spans * J.bpm), flags(ns), unresolved(ns), verdict(ns);
        std::vector<int32_t> ord(spans);
        J.cand_a = cand_a.data(); J.cand_x = cand_x.data(); J.cand_c = cand_c.data();
        J.entry = entry.data(); J.ord = ord.data();
        J.flags = flags.data(); J.unresolved = unresolved.data(); J.verdict = verdict.data();
        J.coef = coef;
        for (size_t i = 0; i < spans; i++)
            for (int q = 0; q < J.bpm; q++) ck_span_speculate(J, (long long)i, q, nullptr, -1);
        for (size_t s = 0; s < ns; s++) ck_span_resolve(J, (int)s, nullptr, -1);
        for (size_t i = 0; i < spans; i++) ck_span_write(J, (long long)i, ZIGZAG, nullptr, -1);
        for (size_t s = 0; s < ns; s++) {
            if (!ck_span_row_ok(J, rows[s])) continue;
            int16_t* fc = coef + (size_t)rows[s].frame * cframe;
            for (int c = 0; c < plan.g.ncomp; c++)
                if (ck_span_dc_apply(fc, plan.g, rows[s].first_mcu, c, 0, ck_span_dc_count(plan.g, rows[s].n_mcu, c), 0))
                    flags[s] |= CK_SPANF_DC_RANGE;
        }
        for (size_t s = 0; s < ns; s++) ck_span_verdict(J, (int)s);
        // the suspect frames again, by the one-lane decoder: its status words decide
        std::vector<uint8_t> again((size_t)plan.frames, 0);
        stats[0] = (long long)spans;
        for (size_t s = 0; s < ns; s++) {
            stats[1] += verdict[s] >> 1;
            if (verdict[s] & 1) { stats[2]++; again[(size_t)rows[s].frame] = 1; }
        }
        for (int f = 0; f < plan.frames; f++)
            if (again[f]) { stats[3]++; memset(coef + (size_t)f * cframe, 0, cframe * sizeof(int16_t)); }
        for (size_t s = 0; s < ns; s++) {
            const CkStrand& r = rows[s];
            if (!again[(size_t)r.frame]) continue;
            status[s] = ck_strand_decode(J.bytes + r.begin, J.bytes + r.end, plan.g, r.first_mcu, r.n_mcu, &plan.sets[(size_t)r.table_set], ZIGZAG,
                                         coef + (size_t)r.frame * cframe);
        }
    }
    for (size_t s = 0; s < ns; s++)
        if (status[s]) {
            *bad = (int)plan.strands[s].frame;
            ck_strand_message(status[s], plan.ri[(size_t)plan.strands[s].frame], msg);
            ck_jpeg_span_host_wording(data[*bad], len[*bad], geom, msg);
            return CK_ERR_DATA;
        }
    if (prc != CK_OK) {
        *bad = plan.frames;
        memcpy(msg, plan.msg, CK_JPEG_MSG);
        ck_jpeg_span_host_wording(data[*bad], len[*bad], geom, msg);
        return prc;
    }
    memcpy(quant, plan.quant.data(), plan.quant.size() * sizeof(uint16_t));
    return CK_OK;
}
