// ck_jpeg_strand.h -- the Huffman decoder of one strand, written once: plain C++ for the host (ck_jpeg_plan.cpp,
// tools/sanitize/jpeg_strand_fuzz.cpp) and device code for k_jpeg_huff.hip.  A strand is one restart interval of one frame
// (its whole scan where the frame has none): it starts byte-aligned with the DC predictors at zero and decodes without
// knowing anything of the others.
//
// The rules are those of the reader in ck_jpeg.cpp, to the bit, because which damaged streams are still accepted depends on
// them: FF 00 is the byte FF; nothing is read at or beyond `end` (zero bits come instead, `fake` counts them); the refill
// points are n < 16 before a symbol, n < s before s extra bits, fill while n <= 56; the refusals are an unknown code, a DC
// category above 11, a DC value outside int16, a coefficient index above 63 and an overrun, checked after every block.  A
// strand that a restart marker follows is also refused when its reader has not arrived at `end` once its MCUs are done
// (the host's "the marker must be the next thing in the data").
//
// Bounds: at most 16 steps per symbol, 64 coefficients per block, n_mcu MCUs; every table index is masked or checked; a
// store lands inside the frame's blocks * 64 coefficients because first_mcu + n_mcu <= mcux * mcuy is checked on entry.
// No input byte can cause an access outside a buffer or a loop without an end.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define CK_HD __host__ __device__
#else
#define CK_HD
#endif

// one decode table as the strand decoder reads it: CkHuff (ck_jpeg.h) without its `present` flag, 1420 bytes
struct CkHuffTab {
    uint16_t look[512];          // the next 9 bits -> (length << 8) | symbol, 0 where the code is longer
    int32_t maxcode[18];         // largest code of each length (-1: none), [17] a sentinel
    int32_t valoff[17];          // index of the first symbol of each length minus its first code
    uint8_t vals[256];
};
// the tables of a frame, selectors resolved: DC and AC of each component (a stream may name other tables for Cr than for
// Cb, and the host decoder takes that); a grey frame has its one pair three times
struct CkHuffSet {
    CkHuffTab t[6];
};
enum { CK_SET_DC = 0, CK_SET_AC = 1 };           // t[2 * component + CK_SET_DC / CK_SET_AC]

struct CkStrandGeom {
    int32_t ncomp, hs, vs, mcux, mcuy;
};

// one row of a plan: begin / end are byte offsets (into stream `frame` on the host, into the staged block on the device)
struct CkStrand {
    int64_t frame, begin, end, first_mcu, n_mcu, table_set;
};

// status word of a strand: 0, or cause << 28 | MCU (an MCU index is below 2^25: blocks * 64 fits int32)
enum {
    CK_STRAND_OVERRUN = 1,       // the entropy-coded data ran past its end
    CK_STRAND_CODE = 2,          // unknown Huffman code
    CK_STRAND_DC_BITS = 3,       // DC category above 11
    CK_STRAND_DC_RANGE = 4,      // DC value outside int16
    CK_STRAND_INDEX = 5,         // coefficient index above 63
    CK_STRAND_MARKER = 6,        // the reader has not arrived at the restart marker that follows
    CK_STRAND_ROW = 7            // a plan row outside the frame (never from ck_jpeg_plan)
};
CK_HD inline uint32_t ck_strand_status(int cause, long long mcu) { return ((uint32_t)cause << 28) | ((uint32_t)mcu & 0x0fffffffu); }

struct CkBitReader {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc;
    int n;                       // bits in acc
    int fake;                    // how many of them (the lowest) are invented zeros
};

CK_HD inline void ck_br_fill(CkBitReader& br)
{
    while (br.n <= 56) {
        unsigned b = 0;
        bool real = false;
        if (br.p < br.end) {
            const unsigned c = *br.p;
            if (c != 0xFF) { b = c; br.p++; real = true; }
            else if (br.p + 1 < br.end && br.p[1] == 0) { b = 0xFF; br.p += 2; real = true; }
        }
        br.acc = (br.acc << 8) | b;
        br.n += 8;
        if (!real || br.fake) br.fake += 8;
    }
}
CK_HD inline unsigned ck_br_peek(const CkBitReader& br, int k) { return (unsigned)((br.acc >> (br.n - k)) & ((1u << k) - 1)); }
CK_HD inline bool ck_br_overrun(const CkBitReader& br) { return br.n < br.fake; }

CK_HD inline int ck_decode_symbol(CkBitReader& br, const CkHuffTab* t)
{
    if (br.n < 16) ck_br_fill(br);
    const unsigned e = t->look[ck_br_peek(br, 9)];
    if (e) { br.n -= (int)(e >> 8); return (int)(e & 255); }
    int l = 10;
    int code = (int)ck_br_peek(br, 10);
    while (l <= 16 && code > t->maxcode[l]) { l++; code = (int)ck_br_peek(br, l <= 16 ? l : 16); }
    if (l > 16) return -1;
    br.n -= l;
    const int idx = code + t->valoff[l];
    return (idx < 0 || idx > 255) ? -1 : t->vals[idx];
}

CK_HD inline int ck_receive_extend(CkBitReader& br, int s)
{
    if (br.n < s) ck_br_fill(br);
    const int v = (int)ck_br_peek(br, s);
    br.n -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// one 8x8 block -> blk (64 values, zero on entry); pred is the component's DC predictor.  -> 0 or a cause
CK_HD inline int ck_decode_block(CkBitReader& br, const CkHuffTab* dc, const CkHuffTab* ac, const uint8_t* zigzag, int& pred,
                                 int16_t* blk)
{
    int s = ck_decode_symbol(br, dc);
    if (s < 0) return ck_br_overrun(br) ? CK_STRAND_OVERRUN : CK_STRAND_CODE;
    if (s > 11) return CK_STRAND_DC_BITS;
    if (s) pred += ck_receive_extend(br, s);
    if (pred < -32768 || pred > 32767) return CK_STRAND_DC_RANGE;
    blk[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {
        const int rs = ck_decode_symbol(br, ac);
        if (rs < 0) return ck_br_overrun(br) ? CK_STRAND_OVERRUN : CK_STRAND_CODE;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;
            k += 16;
            continue;
        }
        k += r;
        if (k > 63) return CK_STRAND_INDEX;
        blk[zigzag[k]] = (int16_t)ck_receive_extend(br, s);
        k++;
    }
    return ck_br_overrun(br) ? CK_STRAND_OVERRUN : 0;
}

// The strand [begin, end) of a frame of geometry g: MCUs first_mcu .. first_mcu + n_mcu - 1 -> coef, the frame's coefficient
// base (zeroed by the caller).  set: the frame's tables; zigzag: 64 entries.  -> status word
CK_HD inline uint32_t ck_strand_decode(const uint8_t* begin, const uint8_t* end, const CkStrandGeom& g, long long first_mcu,
                                       long long n_mcu, const CkHuffSet* set, const uint8_t* zigzag, int16_t* coef)
{
    const long long total = (long long)g.mcux * g.mcuy;
    if (first_mcu < 0 || n_mcu < 1 || first_mcu > total - n_mcu || end < begin) return ck_strand_status(CK_STRAND_ROW, 0);
    const bool colour = g.ncomp == 3;
    const int bh = colour ? g.hs : 1, bv = colour ? g.vs : 1;
    const int lw = g.mcux * bh;
    const size_t base1 = (size_t)lw * ((size_t)g.mcuy * bv), base2 = base1 + (size_t)total;
    const CkHuffTab *dc0 = &set->t[CK_SET_DC], *ac0 = &set->t[CK_SET_AC];
    const CkHuffTab *dc1 = &set->t[2 + CK_SET_DC], *ac1 = &set->t[2 + CK_SET_AC];
    const CkHuffTab *dc2 = &set->t[4 + CK_SET_DC], *ac2 = &set->t[4 + CK_SET_AC];
    CkBitReader br = {begin, end, 0, 0, 0};
    int pred0 = 0, pred1 = 0, pred2 = 0;
    int my = (int)(first_mcu / g.mcux), mx = (int)(first_mcu % g.mcux);
    for (long long i = 0; i < n_mcu; i++) {
        const long long mcu = first_mcu + i;
        for (int v = 0; v < bv; v++)
            for (int u = 0; u < bh; u++) {
                const int rc = ck_decode_block(br, dc0, ac0, zigzag, pred0, coef + ((size_t)(my * bv + v) * lw + (size_t)(mx * bh + u)) * 64);
                if (rc) return ck_strand_status(rc, mcu);
            }
        if (colour) {
            const size_t at = (size_t)my * g.mcux + (size_t)mx;
            int rc = ck_decode_block(br, dc1, ac1, zigzag, pred1, coef + (base1 + at) * 64);
            if (rc) return ck_strand_status(rc, mcu);
            rc = ck_decode_block(br, dc2, ac2, zigzag, pred2, coef + (base2 + at) * 64);
            if (rc) return ck_strand_status(rc, mcu);
        }
        if (++mx == g.mcux) { mx = 0; my++; }
    }
    // a restart marker follows every strand but the frame's last: the reader must stand on it
    if (first_mcu + n_mcu < total && br.p != end) return ck_strand_status(CK_STRAND_MARKER, first_mcu + n_mcu);
    return 0;
}

// ---- host side: the planner (ck_jpeg_plan.cpp) ----
#include <vector>

#include "ck_jpeg.h"

// what ck_jpeg_plan_build makes of n streams of one geometry (ck_jpeg_plan.cpp; host only, no HIP)
struct CkJpegPlan {
    CkStrandGeom g{};
    int frames = 0;                      // frames planned: n, or the index of the frame that was refused
    std::vector<CkStrand> strands;       // frame-major, MCUs ascending; begin / end are offsets into the frame's stream
    std::vector<int32_t> ri;             // restart interval by frame
    std::vector<size_t> scan;            // offset of the entropy-coded segment by frame
    std::vector<CkHuffSet> sets;         // de-duplicated by content across the call
    std::vector<uint16_t> quant;         // frames * 192
    char msg[CK_JPEG_MSG] = {0};         // why frame `frames` was refused
};
// CK_OK (frames == n), or the status of the first refused frame: the frames before it are planned all the same, so that
// a caller can still find an earlier frame whose entropy-coded data is damaged
int ck_jpeg_plan_build(const uint8_t* const* data, const size_t* len, int n, const ck_jpeg_info& geom, CkJpegPlan* plan);
// the message of a failed strand's status word, in the host decoder's wording
void ck_strand_message(uint32_t status, int restart_interval, char* msg);
// the plan, then every strand through ck_strand_decode on this thread (`reverse`: last strand first) -> what
// ck_jpeg_coefficients gives.  On failure *bad is the first frame that failed and msg (CK_JPEG_MSG) the cause.
int ck_jpeg_strands_host(const uint8_t* const* data, const size_t* len, int n, const ck_jpeg_info& geom, int16_t* coef,
                         uint16_t* quant, bool reverse, int* bad, char* msg);
