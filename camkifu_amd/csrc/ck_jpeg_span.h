// ck_jpeg_span.h -- parallel Huffman decoding INSIDE a strand, written once: plain C++ for the host (ck_jpeg_span.cpp,
// tools/sanitize/jpeg_span_fuzz.cpp) and device code for k_jpeg_span.hip.  A strand (ck_jpeg_strand.h) is cut into spans of
// S raw bytes.  Huffman streams fall into step with the true symbol boundaries a short run after a wrong start, so a lane
// can guess: it starts one span early, once per block slot of the MCU (the slot selects the tables and never falls into
// step on its own), and records where it stands when it crosses into its span.  A serial walk per strand then only
// compares states.  The steps, each one launch (one loop on the host), `i` a span of the pass, `s` a strand:
//
//   speculate (i, guess)  warm-up through span j - 1 from (guess, k = 0) with the recovery rule -> A, the candidate entry
//                         of span j; then strictly through span j -> X, the candidate exit, C, the blocks completed, and
//                         `bad` when that part met a refusal.  Span 0 is decoded once, from the strand's true start.
//   resolve   (s)         in span order: the true entry of span j is the exit of span j - 1; where a candidate's A equals it
//                         (and is not bad) X and C are taken, else the span is decoded here (an UNRESOLVED span).
//                         -> per span the true entry and the ordinal of the block it stands in
//   write     (i)         decodes span i from its true entry with the host's block-loop rules and stores the coefficients of
//                         the symbols that begin inside it, the DC DIFFERENCE in coefficient 0
//   dc        (s)         per component an inclusive sum of the differences in decode order
//   verdict   (s)         clean, or suspect: see ck_span_verdict
//
// A state at a symbol boundary is (position, block slot in the MCU, next zigzag index k; 0: the DC symbol comes next).  A
// position is (raw byte offset from the strand's begin, bit in byte) and never lies inside a stuffing 00: the reader steps
// over the pair FF 00 as one byte.  Behind the strand's end come zero bits, and the position goes on counting.
//
// Bounds, for every input byte:
//   - every decode loop consumes at least one bit per step (a code has a length of 1 .. 16; the recovery rule moves on
//     one bit) and ends at a bit limit the data cannot move: the end of the lane's span, so at most two spans plus one
//     symbol for speculate and one span plus one symbol for resolve and write;
//   - no load goes outside the staged block: a row is checked against it (ck_span_row_ok) and the reader loads nothing
//     at or behind the strand's end; table indices are masked or checked;
//   - no store goes outside the strand's frame: write stores only for a block whose ordinal is below n_mcu * bpm, and the
//     row check holds first_mcu + n_mcu inside the frame; dc walks the same blocks;
//   - the resolve walk has as many steps as the strand has spans.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>                     // (atomicOr: write and dc meet in a strand's flag word)
#endif
#include "ck_jpeg_strand.h"

enum { CK_SPAN_MIN = 8, CK_SPAN_MAX = 4096, CK_SPAN_DEFAULT = 512 };

// the flag word of a strand
enum {
    CK_SPANF_REFUSED = 1,        // the true chain met a symbol the strict decoder refuses
    CK_SPANF_DC_RANGE = 2,       // a running DC value outside int16
    CK_SPANF_DONE = 4,           // the true chain completed all the strand's blocks
    CK_SPANF_TAIL = 8,           // ... and fewer than 8 bits remained behind the last
    CK_SPANF_OVERRUN = 16,       // ... but consumed bits behind the end of the data
    CK_SPANF_ROW = 32            // a plan row outside the frame or the staged block (never from ck_jpeg_plan)
};
#define CK_SPAN_DEAD (~(uint64_t)0)              // the entry of a span the true chain never reaches
#define CK_SPAN_BAD 0x80000000u                   // in a candidate's block count: the strict part met a refusal

// what the steps of one pass read and write; every pointer is to host memory on the host and to HBM on the device
struct CkSpanJob {
    const uint8_t* bytes;        // the staged entropy-coded segments
    long long n_bytes;
    const CkStrand* rows;        // begin / end are offsets into bytes
    int n_strands;
    const int32_t* span0;        // n_strands + 1: the first span of each strand
    const CkHuffSet* sets;
    int n_sets;
    CkStrandGeom g;
    long long cframe;            // coefficients of a frame
    int n_frames, span_bytes, bpm;
    uint64_t *cand_a, *cand_x;   // spans * bpm candidates
    uint32_t* cand_c;
    uint64_t* entry;             // spans
    int32_t* ord;
    uint32_t *flags, *unresolved, *verdict;     // strands; verdict: suspect | unresolved spans << 1
    int16_t* coef;               // n_frames * cframe, zeroed before write
};

CK_HD inline int ck_span_bpm(const CkStrandGeom& g) { return g.ncomp == 3 ? g.hs * g.vs + 2 : 1; }
CK_HD inline long long ck_span_count(long long strand_bytes, int span_bytes)
{
    return strand_bytes <= 0 ? 1 : (strand_bytes + span_bytes - 1) / span_bytes;
}
CK_HD inline uint64_t ck_span_pack(long long pos, int slot, int k) { return ((uint64_t)pos << 16) | ((uint64_t)slot << 8) | (uint64_t)k; }

CK_HD inline bool ck_span_row_ok(const CkSpanJob& J, const CkStrand& r)
{
    const long long total = (long long)J.g.mcux * J.g.mcuy;
    return r.frame >= 0 && r.frame < J.n_frames && r.begin >= 0 && r.end >= r.begin && r.end <= J.n_bytes && r.table_set >= 0 &&
           r.table_set < J.n_sets && r.first_mcu >= 0 && r.n_mcu >= 1 && r.first_mcu <= total - r.n_mcu;
}

// the strand of span i: span0[s] <= i < span0[s + 1]
CK_HD inline int ck_span_strand(const CkSpanJob& J, long long i)
{
    int lo = 0, hi = J.n_strands - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (J.span0[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- the reader: a window of four data bytes from the current one on, and which of them had a stuffing 00 behind ----
struct CkSpanReader {
    const uint8_t* d;
    long long len, p, rp;        // p: raw offset of the current byte; rp: of the next byte to load
    int bit;                     // bits of the current byte that are consumed
    uint32_t w, fl;              // fl bit 3: the current byte is an FF with its 00
};
CK_HD inline void ck_sr_load(CkSpanReader& r)
{
    uint32_t b = 0, st = 0;
    if (r.rp < r.len) {
        b = r.d[r.rp];
        if (b == 0xFF && r.rp + 1 < r.len && r.d[r.rp + 1] == 0) { st = 1; r.rp += 2; }
        else r.rp += 1;
    } else {
        r.rp += 1;
    }
    r.w = (r.w << 8) | b;
    r.fl = ((r.fl << 1) | st) & 15u;
}
CK_HD inline void ck_sr_open(CkSpanReader& r, const uint8_t* d, long long len, long long p, int bit)
{
    r.d = d; r.len = len; r.p = p; r.rp = p; r.bit = bit; r.w = 0; r.fl = 0;
    for (int i = 0; i < 4; i++) ck_sr_load(r);
}
CK_HD inline long long ck_sr_pos(const CkSpanReader& r) { return r.p * 8 + r.bit; }
CK_HD inline uint32_t ck_sr_peek(const CkSpanReader& r, int n) { return (uint32_t)(r.w << r.bit) >> (32 - n); }      // n: 1 .. 16
CK_HD inline void ck_sr_skip(CkSpanReader& r, int n)
{
    r.bit += n;
    while (r.bit >= 8) {
        r.p += 1 + ((r.fl >> 3) & 1u);
        ck_sr_load(r);
        r.bit -= 8;
    }
}
CK_HD inline int ck_sr_symbol(CkSpanReader& r, const CkHuffTab* t)
{
    const uint32_t v = ck_sr_peek(r, 16);
    const unsigned e = t->look[v >> 7];
    if (e) { const int l = (int)(e >> 8); ck_sr_skip(r, l < 1 ? 1 : (l > 16 ? 16 : l)); return (int)(e & 255); }
    for (int l = 10; l <= 16; l++) {
        const int code = (int)(v >> (16 - l));
        if (code <= t->maxcode[l]) {
            const int idx = code + t->valoff[l];
            if (idx < 0 || idx > 255) return -1;
            ck_sr_skip(r, l);
            return t->vals[idx];
        }
    }
    return -1;
}
CK_HD inline int ck_sr_extend(CkSpanReader& r, int s)            // s: 1 .. 15
{
    const int v = (int)ck_sr_peek(r, s);
    ck_sr_skip(r, s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One symbol of the block in slot `slot` at zigzag index k.  -> -1: the strict decoder refuses it (unknown code, DC category
// above 11, index above 63; the reader may have moved), else bit 0: the block ended, bit 1: (idx, val) is a coefficient.
enum { CK_STEP_END = 1, CK_STEP_COEF = 2 };
CK_HD inline int ck_span_step(CkSpanReader& r, const CkHuffSet* set, const CkStrandGeom& g, int slot, int& k, int& idx, int& val)
{
    const int nl = g.hs * g.vs;
    const int c = g.ncomp == 3 ? (slot < nl ? 0 : slot - nl + 1) : 0;
    if (k == 0) {
        const int s = ck_sr_symbol(r, &set->t[2 * c + CK_SET_DC]);
        if (s < 0 || s > 11) return -1;
        idx = 0;
        val = s ? ck_sr_extend(r, s) : 0;
        k = 1;
        return CK_STEP_COEF;
    }
    const int rs = ck_sr_symbol(r, &set->t[2 * c + CK_SET_AC]);
    if (rs < 0) return -1;
    const int run = rs >> 4, s = rs & 15;
    if (s == 0) {
        if (run != 15) { k = 0; return CK_STEP_END; }
        k += 16;                                                 // a ZRL that runs past index 63 ends the block silently
        if (k > 63) { k = 0; return CK_STEP_END; }
        return 0;
    }
    k += run;
    if (k > 63) return -1;
    idx = k;
    val = ck_sr_extend(r, s);
    k++;
    if (k > 63) { k = 0; return CK_STEP_END | CK_STEP_COEF; }
    return CK_STEP_COEF;
}

// what a lane knows of its span once it has found its strand
struct CkSpanAt {
    int s;                       // strand
    long long j, lo, hi, len;    // span j of the strand covers raw bytes lo .. hi - 1 of its len
    long long nblocks;
    const uint8_t* d;
    const CkHuffSet* set;
};
// fast / fast_set: a copy of table set fast_set that is quicker to read (LDS on the device; nullptr, -1 on the host)
CK_HD inline bool ck_span_at(const CkSpanJob& J, long long i, const CkHuffSet* fast, long long fast_set, CkSpanAt& a, CkStrand& r)
{
    a.s = ck_span_strand(J, i);
    r = J.rows[a.s];
    if (!ck_span_row_ok(J, r)) return false;
    a.j = i - J.span0[a.s];
    a.len = r.end - r.begin;
    a.lo = a.j * J.span_bytes;
    a.hi = a.lo + J.span_bytes < a.len ? a.lo + J.span_bytes : a.len;
    a.nblocks = r.n_mcu * J.bpm;
    a.d = J.bytes + r.begin;
    a.set = r.table_set == fast_set ? fast : J.sets + r.table_set;
    return true;
}

CK_HD inline void ck_span_speculate(const CkSpanJob& J, long long i, int guess, const CkHuffSet* fast, long long fast_set)
{
    const size_t at = (size_t)i * J.bpm + guess;
    J.cand_a[at] = CK_SPAN_DEAD;
    J.cand_x[at] = CK_SPAN_DEAD;
    J.cand_c[at] = CK_SPAN_BAD;
    CkSpanAt a;
    CkStrand r;
    if (!ck_span_at(J, i, fast, fast_set, a, r)) return;
    if (a.j == 0 && guess > 0) return;
    CkSpanReader rd;
    int slot = guess, k = 0, idx, val;
    if (a.j == 0) {
        ck_sr_open(rd, a.d, a.len, 0, 0);
    } else {
        long long start = a.lo - J.span_bytes;                   // (start + 1 <= lo < len)
        if (a.d[start] == 0 && start > 0 && a.d[start - 1] == 0xFF) start++;
        ck_sr_open(rd, a.d, a.len, start, 0);
        while (ck_sr_pos(rd) < a.lo * 8) {
            const CkSpanReader keep = rd;
            const int rc = ck_span_step(rd, a.set, J.g, slot, k, idx, val);
            if (rc < 0) { rd = keep; ck_sr_skip(rd, 1); k = 0; }  // the recovery rule: the block ends, one bit further
            if (rc < 0 || (rc & CK_STEP_END)) slot = slot + 1 == J.bpm ? 0 : slot + 1;
        }
    }
    J.cand_a[at] = ck_span_pack(ck_sr_pos(rd), slot, k);
    const long long limit = a.j == 0 ? a.nblocks : 0x7fffffff;   // (span 0 knows its ordinal: it stops with the strand)
    uint32_t cnt = 0, bad = 0;
    while (ck_sr_pos(rd) < a.hi * 8 && (long long)cnt < limit) {
        const int rc = ck_span_step(rd, a.set, J.g, slot, k, idx, val);
        if (rc < 0) { bad = CK_SPAN_BAD; break; }
        if (rc & CK_STEP_END) { slot = slot + 1 == J.bpm ? 0 : slot + 1; cnt++; }
    }
    J.cand_x[at] = ck_span_pack(ck_sr_pos(rd), slot, k);
    J.cand_c[at] = cnt | bad;
}

CK_HD inline void ck_span_resolve(const CkSpanJob& J, int s, const CkHuffSet* fast, long long fast_set)
{
    const long long i0 = J.span0[s], nsp = J.span0[s + 1] - i0;
    CkSpanAt a;
    CkStrand r;
    uint32_t fl = 0, unres = 0;
    bool alive = ck_span_at(J, i0, fast, fast_set, a, r);
    if (!alive) fl = CK_SPANF_ROW;
    uint64_t state = ck_span_pack(0, 0, 0);
    long long ord = 0;
    for (long long j = 0; j < nsp; j++) {
        const long long i = i0 + j;
        if (!alive) { J.entry[i] = CK_SPAN_DEAD; J.ord[i] = 0; continue; }
        J.entry[i] = state;
        J.ord[i] = (int32_t)ord;
        // all the span's candidates are loaded before any is compared: the loads do not wait for one another, and the walk
        // is a chain of memory round trips otherwise (a guess of span 0 beyond the first is dead and matches nothing)
        uint64_t ca[6];
        uint32_t cc[6];
        for (int q = 0; q < 6; q++) {
            const size_t at = (size_t)i * J.bpm + (q < J.bpm ? q : 0);
            ca[q] = J.cand_a[at];
            cc[q] = J.cand_c[at];
        }
        int hit = -1;
        for (int q = 5; q >= 0; q--)
            if (q < J.bpm && ca[q] == state && !(cc[q] & CK_SPAN_BAD)) hit = q;
        if (hit >= 0) {
            state = J.cand_x[(size_t)i * J.bpm + hit];
            ord += cc[hit];
        } else {
            unres++;
            const long long lo = j * J.span_bytes, hi = lo + J.span_bytes < a.len ? lo + J.span_bytes : a.len;
            CkSpanReader rd;
            ck_sr_open(rd, a.d, a.len, (long long)(state >> 19), (int)((state >> 16) & 7));
            int slot = (int)((state >> 8) & 255), k = (int)(state & 255), idx, val;
            while (ck_sr_pos(rd) < hi * 8 && ord < a.nblocks) {
                const int rc = ck_span_step(rd, a.set, J.g, slot, k, idx, val);
                if (rc < 0) { fl |= CK_SPANF_REFUSED; alive = false; break; }
                if (rc & CK_STEP_END) { slot = slot + 1 == J.bpm ? 0 : slot + 1; ord++; }
            }
            state = ck_span_pack(ck_sr_pos(rd), slot, k);
        }
        if (ord >= a.nblocks) alive = false;
    }
    J.flags[s] = fl;
    J.unresolved[s] = unres;
}

#if defined(__HIP_DEVICE_COMPILE__)
#define CK_SPAN_OR(word, bits) atomicOr(&(word), (bits))
#else
#define CK_SPAN_OR(word, bits) ((word) |= (bits))
#endif

CK_HD inline void ck_span_write(const CkSpanJob& J, long long i, const uint8_t* zigzag, const CkHuffSet* fast, long long fast_set)
{
    CkSpanAt a;
    CkStrand r;
    if (!ck_span_at(J, i, fast, fast_set, a, r)) return;
    const uint64_t state = J.entry[i];
    if (state == CK_SPAN_DEAD) return;
    long long ord = J.ord[i];
    if (ord < 0 || ord >= a.nblocks) return;
    const CkStrandGeom& g = J.g;
    const bool colour = g.ncomp == 3;
    const int bh = colour ? g.hs : 1, bv = colour ? g.vs : 1, nl = bh * bv;
    const int lw = g.mcux * bh;
    const size_t base1 = (size_t)lw * ((size_t)g.mcuy * bv), base2 = base1 + (size_t)g.mcux * g.mcuy;
    const long long mcu = r.first_mcu + ord / J.bpm;
    int my = (int)(mcu / g.mcux), mx = (int)(mcu % g.mcux);
    int slot = (int)(ord % J.bpm), k = (int)(state & 255), idx = 0, val = 0;
    int16_t* coef = J.coef + r.frame * J.cframe;
    CkSpanReader rd;
    ck_sr_open(rd, a.d, a.len, (long long)(state >> 19), (int)((state >> 16) & 7));
    while (ck_sr_pos(rd) < a.hi * 8) {
        const int rc = ck_span_step(rd, a.set, g, slot, k, idx, val);
        if (rc < 0) { CK_SPAN_OR(J.flags[a.s], (uint32_t)CK_SPANF_REFUSED); return; }
        if (rc & CK_STEP_COEF) {
            const size_t blk = slot < nl ? (size_t)(my * bv + slot / bh) * lw + (size_t)(mx * bh + slot % bh)
                                         : (slot == nl ? base1 : base2) + (size_t)my * g.mcux + (size_t)mx;
            coef[blk * 64 + zigzag[idx & 63]] = (int16_t)val;
        }
        if (rc & CK_STEP_END) {
            if (++ord == a.nblocks) {
                uint32_t f = CK_SPANF_DONE;
                const long long next = rd.bit ? rd.p + 1 + ((rd.fl >> 3) & 1u) : rd.p;
                if (ck_sr_pos(rd) > a.len * 8) f |= CK_SPANF_OVERRUN;
                if (next == a.len) f |= CK_SPANF_TAIL;
                CK_SPAN_OR(J.flags[a.s], f);
                return;
            }
            if (++slot == J.bpm) { slot = 0; if (++mx == g.mcux) { mx = 0; my++; } }
        }
    }
}

// the blocks of component c of a strand in decode order: block t of them -> its index among the frame's blocks
CK_HD inline size_t ck_span_dc_block(const CkStrandGeom& g, long long first_mcu, int c, long long t)
{
    const bool colour = g.ncomp == 3;
    const int bh = colour ? g.hs : 1, bv = colour ? g.vs : 1;
    const int lw = g.mcux * bh;
    if (c == 0) {
        const long long mcu = first_mcu + t / (bh * bv);
        const int sub = (int)(t % (bh * bv));
        return (size_t)((mcu / g.mcux) * bv + sub / bh) * lw + (size_t)((mcu % g.mcux) * bh + sub % bh);
    }
    const size_t base1 = (size_t)lw * ((size_t)g.mcuy * bv);
    return base1 + (c == 2 ? (size_t)g.mcux * g.mcuy : 0) + (size_t)(first_mcu + t);
}
CK_HD inline long long ck_span_dc_count(const CkStrandGeom& g, long long n_mcu, int c) { return c == 0 && g.ncomp == 3 ? n_mcu * g.hs * g.vs : n_mcu; }
CK_HD inline long long ck_span_dc_sum(const int16_t* coef, const CkStrandGeom& g, long long first_mcu, int c, long long t0, long long t1)
{
    long long sum = 0;
    for (long long t = t0; t < t1; t++) sum += coef[ck_span_dc_block(g, first_mcu, c, t) * 64];
    return sum;
}
// differences -> values for blocks t0 .. t1 - 1, `run` the sum of the differences before t0.  -> a value left int16
CK_HD inline bool ck_span_dc_apply(int16_t* coef, const CkStrandGeom& g, long long first_mcu, int c, long long t0, long long t1, long long run)
{
    bool out = false;
    for (long long t = t0; t < t1; t++) {
        int16_t* at = coef + ck_span_dc_block(g, first_mcu, c, t) * 64;
        run += *at;
        if (run < -32768 || run > 32767) out = true;
        *at = (int16_t)run;
    }
    return out;
}

// A strand is clean when its true chain completed all its blocks with no refusal, consumed no bit behind the end of its
// data, its running DC stayed in range and, where a restart marker follows, fewer than 8 bits remained behind its last
// block.  The last is stricter than the host's "the marker must be the next thing" and implies it, so a clean strand is one
// the host accepts with the same coefficients.  Every other strand is suspect: no cause is named and nothing is refused --
// its frame is decoded again by the one-lane decoder (ck_strand_decode), whose status decides.
CK_HD inline void ck_span_verdict(const CkSpanJob& J, int s)
{
    const CkStrand r = J.rows[s];
    const uint32_t f = J.flags[s];
    bool clean = !(f & (CK_SPANF_REFUSED | CK_SPANF_DC_RANGE | CK_SPANF_OVERRUN | CK_SPANF_ROW)) && (f & CK_SPANF_DONE);
    if (clean && r.first_mcu + r.n_mcu < (long long)J.g.mcux * J.g.mcuy && !(f & CK_SPANF_TAIL)) clean = false;
    J.verdict[s] = (clean ? 0u : 1u) | (J.unresolved[s] << 1);
}

// ---- host side (ck_jpeg_span.cpp) ----
// The one-lane decoder's status decides that a frame is refused; its wording is not always the host decoder's (the planner
// refuses a frame with a missing marker before a block is decoded, the host reports what it met on the way there).  For the
// one frame a call refuses, this runs the host decoder on it and, where that refuses too, puts its message into msg.
void ck_jpeg_span_host_wording(const uint8_t* data, size_t len, const ck_jpeg_info& geom, char* msg);
// stats: spans, unresolved spans, suspect strands, frames handed to the one-lane decoder
enum { CK_SPAN_STATS = 4 };
// the plan, then the steps above in their order on this thread, the suspect frames through ck_strand_decode -> what
// ck_jpeg_coefficients gives.  On failure *bad is the first frame that failed and msg (CK_JPEG_MSG) the cause.
int ck_jpeg_spans_host(const uint8_t* const* data, const size_t* len, int n, const ck_jpeg_info& geom, int span_bytes, int16_t* coef,
                       uint16_t* quant, int* bad, char* msg, long long* stats);
