// ck_stage_layout.h -- where the parts of every staging and work block of the codec entry points lie (ck_api_jpeg.hip,
// ck_api_png.hip, ck_harvest_patches), and how many frames go into a pass.  Plain C++, no HIP and no context: the entry points
// turn these offsets into pointers and do no arithmetic of their own, and tools/stage_layouts.cpp prints them for
// tests/test_stage_layout_cpu.py, which holds them to tests/golden/stage_layouts.json.
//
// Every part starts on 16 bytes (ck_carve.h): the kernels read these blocks by offset with wide loads.  The offsets inside a
// block that is uploaded, or whose size a counter reports (ck_jpeg_uploaded_bytes, ck_png_uploaded_bytes), are pinned to the
// byte by the fixture; a block that exists on the device only is pinned as well, but free to move with a reason.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "ck_carve.h"
#include "ck_jpeg_strand.h"          // CkStrand, CkHuffSet
#include "ck_jpeg_enc.h"             // CkEncGeom, CkEncTables, CK_JPEG_ENC_HEADER_BOUND
#include "ck_png_stage.h"            // CkPngGeom, CkPngEdge, CkPngDesc
#include "ck_png_inflate_stage.h"    // CkInfJob, CkInfRecord

// ---- JPEG decode, the Huffman stage on the device (jpeg_huff_pass) ----
// The upload block: the entropy-coded segment of every frame, 16 zeroed bytes behind the last (a wide load at the last byte
// stays inside), the plan rows, the table sets, the quant tables, and with spans the first span of every strand and one
// more word.  seg[frames] is where the slack starts, n_bytes where it ends; the upload ends with its last word, not on 16.
struct CkHuffLayout {
    std::vector<size_t> seg;
    size_t n_bytes, rows, sets, quant, span0, total;
};
inline CkHuffLayout ck_huff_layout(const size_t* seg_len, int frames, size_t ns, size_t n_sets, bool spans)
{
    CkCarve c;
    CkHuffLayout L;
    for (int f = 0; f < frames; f++) L.seg.push_back(c.take(seg_len[f]));
    L.seg.push_back(c.take(16));
    L.n_bytes = c.size();
    L.rows = c.take(ns * sizeof(CkStrand));
    L.sets = c.take(n_sets * sizeof(CkHuffSet));
    L.quant = c.take((size_t)frames * 192 * sizeof(uint16_t));
    L.total = c.size();
    L.span0 = c.take(spans ? (ns + 1) * sizeof(int32_t) : 0);
    if (spans) L.total = L.span0 + (ns + 1) * sizeof(int32_t);
    return L;
}

// The work arrays of a pass with spans, in jspan: the 8-byte ones first.  cand = n_spans * bpm candidates.
struct CkSpanLayout {
    size_t cand_a, cand_x, entry, cand_c, ord, flags, unresolved, verdict, total;
};
inline CkSpanLayout ck_span_layout(size_t n_spans, size_t bpm, size_t ns)
{
    CkCarve c;
    CkSpanLayout L;
    const size_t cand = n_spans * bpm;
    L.cand_a = c.take(cand * 8); L.cand_x = c.take(cand * 8); L.entry = c.take(n_spans * 8);
    L.cand_c = c.take(cand * 4); L.ord = c.take(n_spans * 4);
    L.flags = c.take(ns * 4); L.unresolved = c.take(ns * 4); L.verdict = c.take(ns * 4);
    L.total = c.size();
    return L;
}

// ---- JPEG encode, the Huffman stage on the device (jpeg_enc_huff_pass) ----
// CkEncWork in jenc_work: 64-bit arrays first, then the 32-bit ones, then the constants -- the CkEncTables, the zigzag order
// and the stream header (consts_std bytes), with optimised tables the header in front of and behind the DHT segments as well
// -- and, optimised tables only, what belongs to a frame: counters, tables, DHT slots and header slots with their lengths.
// The pinned block: the constants going up, and at pin_words the size words coming down (16 bytes, then 8 a frame).
struct CkEncLayout {
    size_t head, tile_off, seg_bits, seg_u0, frame_u0, len, out_off, bits, tile_bits, consts;
    size_t freq, tables, dht, dht_len, headers, hlen, total;
    size_t consts_std, consts_bytes;
    size_t pin_words, pin_total;
};
inline CkEncLayout ck_enc_layout(const CkEncGeom& g, int m, bool optimise)
{
    CkCarve c, pin;
    CkEncLayout L;
    const size_t M = (size_t)m, blocks = M * g.blocks, tiles = M * g.nseg * g.seg_tiles, segs = M * g.nseg, om = optimise ? M : 0;
    L.consts_std = sizeof(CkEncTables) + 64 + CK_JPEG_ENC_HEADER_BOUND;
    L.consts_bytes = L.consts_std + (optimise ? (size_t)CK_ENC_HEADER_SLOT + 64 : 0);
    L.head = c.take(2 * 8); L.tile_off = c.take(tiles * 8); L.seg_bits = c.take(segs * 8); L.seg_u0 = c.take((segs + M) * 8);
    L.frame_u0 = c.take((M + 1) * 8); L.len = c.take(M * 8); L.out_off = c.take((M + 1) * 8);
    L.bits = c.take(blocks * 4); L.tile_bits = c.take(tiles * 4);
    L.consts = c.take(L.consts_bytes);
    L.freq = c.take(om * 4 * 256 * 4); L.tables = c.take(om * sizeof(CkEncTables)); L.dht = c.take(om * 4 * CK_ENC_DHT_SLOT);
    L.dht_len = c.take(om * 4 * 4); L.headers = c.take(om * CK_ENC_HEADER_SLOT); L.hlen = c.take(om * 4);
    L.total = c.size();
    pin.take(L.consts_bytes);
    L.pin_words = pin.take(16 + M * 8);
    L.pin_total = L.pin_words + 16 + M * 8;
    return L;
}

// ---- PNG ----
// ck_png_inflate_device, in png_inf: the jobs, the zlib streams (what goes up: the block as far as rec), the verdict records,
// and dstride bytes of output a stream (the longest room of the call, rounded up)
struct CkInflateLayout {
    std::vector<size_t> z;
    size_t jobs, rec, out, dstride, total;
};
inline CkInflateLayout ck_inflate_layout(const size_t* zlen, int n, size_t most)
{
    CkCarve c;
    CkInflateLayout L;
    L.dstride = ck_up16(most);
    L.jobs = c.take((size_t)n * sizeof(CkInfJob));
    for (int f = 0; f < n; f++) L.z.push_back(c.take(zlen[f]));
    L.rec = c.take((size_t)n * sizeof(CkInfRecord));
    L.out = c.take((size_t)n * L.dstride);
    L.total = c.size();
    return L;
}

// A pass of ck_png_decode over m frames, inflated[i] bytes of rows each.  The host inflates (zlen NULL): descriptors, palettes
// (768 bytes a frame) and the rows, all of it uploaded.  The device inflates (zlen[i]: the bytes of stream i): descriptors,
// palettes, jobs and streams go up (`upload` bytes); the records and the rows behind them exist on the device only.
struct CkPngDecodeLayout {
    std::vector<size_t> z, rows;
    size_t desc, pal, jobs, rec, upload, total;
};
inline CkPngDecodeLayout ck_png_decode_layout(const size_t* inflated, const size_t* zlen, int m)
{
    CkCarve c;
    CkPngDecodeLayout L;
    L.desc = c.take((size_t)m * sizeof(CkPngDesc));
    L.pal = c.take((size_t)m * 768);
    L.jobs = L.rec = 0;
    if (zlen) {
        L.jobs = c.take((size_t)m * sizeof(CkInfJob));
        for (int i = 0; i < m; i++) L.z.push_back(c.take(zlen[i]));
        L.rec = c.take((size_t)m * sizeof(CkInfRecord));
    }
    for (int i = 0; i < m; i++) L.rows.push_back(c.take(inflated[i]));
    L.total = c.size();
    L.upload = zlen ? L.rec : L.total;
    return L;
}

// CkPngWork in png_work, every array on 16 bytes.  The runs mode's three arrays come last: the literal-only mode's block is
// what it was before there were runs.
struct CkPngWorkLayout {
    size_t head, tile_off, band_off, frame_bits, out_off, count, tile_bits, tile_a, tile_b, adler, band_bits, band_a, band_b;
    size_t codes, lens, filt, before, after, edge, total;
};
inline CkPngWorkLayout ck_png_work_layout(const CkPngGeom& g, int m, int runs)
{
    CkCarve c;
    CkPngWorkLayout L;
    const size_t M = (size_t)m, P = (size_t)ck_png_pitch(runs), bands = M * g.bands, tiles = M * g.tiles;
    L.head = c.take((M + 1) * 8); L.tile_off = c.take(tiles * 8); L.band_off = c.take(bands * 8); L.frame_bits = c.take(M * 8);
    L.out_off = c.take((M + 1) * 8); L.count = c.take(bands * P * 4); L.tile_bits = c.take(tiles * 4);
    L.tile_a = c.take(tiles * 4); L.tile_b = c.take(tiles * 4); L.adler = c.take(M * 4);
    L.band_bits = c.take(bands * 8); L.band_a = c.take(bands * 4); L.band_b = c.take(bands * 4);
    L.codes = c.take(bands * P * 2); L.lens = c.take(bands * P); L.filt = c.take(M * (size_t)g.fbytes);
    L.before = L.after = L.edge = 0;
    if (runs) { L.before = c.take(tiles * 4); L.after = c.take(tiles * 4); L.edge = c.take(tiles * sizeof(CkPngEdge)); }
    L.total = c.size();
    return L;
}

// ---- ck_harvest_patches: state_of | positions (and one byte) | codes of the n * 100 candidates | block totals + the grand total
struct CkHarvestLayout {
    size_t state, pos, code, blocks, total;
};
inline CkHarvestLayout ck_harvest_layout(int n, int n_pos, int nb)
{
    CkCarve c;
    CkHarvestLayout L;
    L.state = c.take((size_t)n * 4); L.pos = c.take((size_t)n_pos * 361 + 1); L.code = c.take((size_t)n * 400);
    L.blocks = c.take(((size_t)nb + 1) * 4);
    L.total = c.size();
    return L;
}

// ---- frames per pass ----
// as many of n frames as `budget` bytes hold at frame_bytes each, one at least
inline int ck_pass_fit(int n, size_t frame_bytes, size_t budget)
{
    const size_t fit = budget / (frame_bytes ? frame_bytes : 1);
    return fit < 1 ? 1 : (fit < (size_t)n ? (int)fit : n);
}
// the same, with what a pass keeps in HBM (cframe bytes a frame) held to hbm_budget as well
inline int ck_pass_fit_hbm(int n, size_t frame_bytes, size_t budget, size_t cframe, size_t hbm_budget)
{
    return ck_pass_fit(ck_pass_fit(n, frame_bytes, budget), cframe, hbm_budget);
}
// a pass that stages compressed streams: a frame costs their mean length, its quant tables and the rounding
inline int ck_pass_fit_streams(int n, const size_t* len, size_t budget, size_t cframe, size_t hbm_budget)
{
    size_t sum = 0;
    for (int f = 0; f < n; f++) sum += len[f];
    return ck_pass_fit_hbm(n, sum / (size_t)n + 192 * sizeof(uint16_t) + 16, budget, cframe, hbm_budget);
}
// PNG frames differ in size: a pass takes frames from f0 on while their rows, each rounded up to 16, stay within `budget`
// (one frame at least).  -> how many; for who asks (nullable), the bytes of their rows and, with zlen, of their streams as
// ck_png_decode_layout will lay them out
inline int ck_png_pass_take(const size_t* inflated, const size_t* zlen, int f0, int n, size_t budget, size_t* rows_bytes, size_t* z_bytes)
{
    int m = 0;
    size_t rows = 0, zs = 0;
    while (f0 + m < n && (m == 0 || rows + ck_up16(inflated[f0 + m]) <= budget)) {
        if (zlen) zs += ck_up16(zlen[f0 + m]);
        rows += ck_up16(inflated[f0 + m++]);
    }
    if (rows_bytes) *rows_bytes = rows;
    if (z_bytes) *z_bytes = zs;
    return m;
}
