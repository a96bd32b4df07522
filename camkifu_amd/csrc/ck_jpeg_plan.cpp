// ck_jpeg_plan.cpp -- the planner of the strand decoder (ck_jpeg_strand.h): headers through ck_jpeg_parse, then a walk of
// the entropy-coded segment by bytes that finds the restart markers -- no Huffman work.  Plain C++: no HIP, no context;
// tools/sanitize/jpeg_strand_fuzz.cpp links it with ck_jpeg.cpp on its own.
#include "ck_jpeg_strand.h"
#include "ck_jpeg_tables.h"

#include <stdio.h>
#include <string.h>

#include <memory>

namespace {

void to_tab(const CkHuff& h, CkHuffTab& t)
{
    memset(&t, 0, sizeof t);                                     // (build_huff leaves entry 0 of maxcode and valoff alone)
    memcpy(t.look, h.look, sizeof t.look);
    for (int l = 1; l < 18; l++) t.maxcode[l] = h.maxcode[l];
    for (int l = 1; l < 17; l++) t.valoff[l] = h.valoff[l];
    memcpy(t.vals, h.vals, sizeof t.vals);
}

// the first byte at or behind `from` where the bit reader stops: an FF that no 00 follows, or the end of the data
size_t strand_end(const uint8_t* data, size_t len, size_t from)
{
    size_t q = from;
    while (q < len) {
        const void* ff = memchr(data + q, 0xFF, len - q);
        if (!ff) return len;
        q = (size_t)((const uint8_t*)ff - data);
        if (q + 1 < len && data[q + 1] == 0) { q += 2; continue; }
        return q;
    }
    return len;
}

}  // namespace

int ck_jpeg_plan_build(const uint8_t* const* data, const size_t* len, int n, const ck_jpeg_info& geom, CkJpegPlan* plan)
{
    plan->strands.clear(); plan->ri.clear(); plan->scan.clear(); plan->sets.clear(); plan->quant.clear();
    plan->frames = 0;
    plan->msg[0] = 0;
    auto fr = std::make_unique<CkJpegFrame>();
    auto set = std::make_unique<CkHuffSet>();
    for (int f = 0; f < n; f++) {
        plan->frames = f;
        int rc = ck_jpeg_parse(data[f], len[f], fr.get(), plan->msg);
        if (rc != CK_OK) return rc;
        if (fr->info.h != geom.h || fr->info.w != geom.w || fr->info.sampling != geom.sampling) {
            snprintf(plan->msg, sizeof plan->msg, "%dx%d sampling %d where the batch is %dx%d sampling %d", fr->info.w, fr->info.h,
                     fr->info.sampling, geom.w, geom.h, geom.sampling);
            return CK_ERR_DATA;
        }
        plan->g = CkStrandGeom{fr->ncomp, fr->hs, fr->vs, fr->mcux, fr->mcuy};
        // the frame's table set
        for (int c = 0; c < 3; c++) {
            const int from = c < fr->ncomp ? c : 0;
            to_tab(fr->dc[from], set->t[2 * c + CK_SET_DC]);
            to_tab(fr->ac[from], set->t[2 * c + CK_SET_AC]);
        }
        size_t si = 0;
        while (si < plan->sets.size() && memcmp(&plan->sets[si], set.get(), sizeof(CkHuffSet))) si++;
        if (si == plan->sets.size()) plan->sets.push_back(*set);
        // the strands: the first ceil(mcus / ri) of them; what follows the last MCU is not looked at
        const long long total = (long long)fr->mcux * fr->mcuy;
        const long long ri = fr->info.restart_interval ? fr->info.restart_interval : total;
        const long long needed = (total + ri - 1) / ri;
        const uint8_t* d = data[f];
        const size_t ln = len[f];
        const size_t first_row = plan->strands.size();
        size_t begin = fr->scan;
        for (long long k = 0; k < needed; k++) {
            const size_t end = strand_end(d, ln, begin);
            const long long first = k * ri;
            plan->strands.push_back(CkStrand{f, (int64_t)begin, (int64_t)end, first, total - first < ri ? total - first : ri, (int64_t)si});
            if (k + 1 == needed) break;
            size_t m = end;
            while (m + 1 < ln && d[m] == 0xFF && d[m + 1] == 0xFF) m++;              // fill bytes
            const int expect = (int)(k & 7);
            if (m + 2 > ln || d[m] != 0xFF || d[m + 1] != 0xD0 + expect) {
                plan->strands.resize(first_row);
                snprintf(plan->msg, sizeof plan->msg, "restart marker RST%d missing or out of order before MCU %lld", expect, first + ri);
                return CK_ERR_DATA;
            }
            begin = m + 2;
        }
        plan->ri.push_back(fr->info.restart_interval);
        plan->scan.push_back(fr->scan);
        plan->quant.insert(plan->quant.end(), &fr->quant[0][0], &fr->quant[0][0] + 192);
    }
    plan->frames = n;
    return CK_OK;
}

void ck_strand_message(uint32_t status, int restart_interval, char* msg)
{
    const long long mcu = status & 0x0fffffffu;
    switch (status >> 28) {
    case CK_STRAND_OVERRUN: snprintf(msg, CK_JPEG_MSG, "the entropy-coded data ran past its end (MCU %lld)", mcu); break;
    case CK_STRAND_CODE: snprintf(msg, CK_JPEG_MSG, "unknown Huffman code (MCU %lld)", mcu); break;
    case CK_STRAND_DC_BITS: snprintf(msg, CK_JPEG_MSG, "DC difference of more than 11 bits (MCU %lld)", mcu); break;
    case CK_STRAND_DC_RANGE: snprintf(msg, CK_JPEG_MSG, "DC value out of range (MCU %lld)", mcu); break;
    case CK_STRAND_INDEX: snprintf(msg, CK_JPEG_MSG, "coefficient index above 63 (MCU %lld)", mcu); break;
    case CK_STRAND_MARKER:
        snprintf(msg, CK_JPEG_MSG, "restart marker RST%d missing or out of order before MCU %lld",
                 restart_interval > 0 ? (int)((mcu / restart_interval - 1) & 7) : 0, mcu);
        break;
    default: snprintf(msg, CK_JPEG_MSG, "a strand outside its frame"); break;
    }
}

int ck_jpeg_strands_host(const uint8_t* const* data, const size_t* len, int n, const ck_jpeg_info& geom, int16_t* coef,
                         uint16_t* quant, bool reverse, int* bad, char* msg)
{
    CkJpegPlan plan;
    const int prc = ck_jpeg_plan_build(data, len, n, geom, &plan);
    if (prc != CK_OK && prc != CK_ERR_DATA) { *bad = plan.frames; memcpy(msg, plan.msg, CK_JPEG_MSG); return prc; }
    const size_t cframe = (size_t)geom.blocks * 64;
    memset(coef, 0, (size_t)plan.frames * cframe * sizeof(int16_t));
    const size_t ns = plan.strands.size();
    std::vector<uint32_t> status(ns, 0);
    for (size_t i = 0; i < ns; i++) {
        const size_t s = reverse ? ns - 1 - i : i;
        const CkStrand& r = plan.strands[s];
        const uint8_t* d = data[r.frame];
        status[s] = ck_strand_decode(d + r.begin, d + r.end, plan.g, r.first_mcu, r.n_mcu, &plan.sets[(size_t)r.table_set], ZIGZAG,
                                     coef + (size_t)r.frame * cframe);
    }
    for (size_t s = 0; s < ns; s++)
        if (status[s]) {
            *bad = (int)plan.strands[s].frame;
            ck_strand_message(status[s], plan.ri[(size_t)plan.strands[s].frame], msg);
            return CK_ERR_DATA;
        }
    if (prc != CK_OK) { *bad = plan.frames; memcpy(msg, plan.msg, CK_JPEG_MSG); return prc; }
    memcpy(quant, plan.quant.data(), plan.quant.size() * sizeof(uint16_t));
    return CK_OK;
}
