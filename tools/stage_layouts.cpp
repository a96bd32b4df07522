// stage_layouts.cpp -- prints every offset and total of every staging layout of the codec entry points (csrc/ck_stage_layout.h)
// and what the pass rules give, for a fixed list of small inputs: one JSON object a line.  tests/test_stage_layout_cpu.py
// builds it with the host compiler, holds the lines to tests/golden/stage_layouts.json and checks alignment, order and
// overlap of the parts.  Plain C++: it includes the two headers alone and links nothing of the library.
//
//     g++ -std=c++17 -I include tools/stage_layouts.cpp -o stage_layouts && ./stage_layouts
//
// A part is [name, offset, bytes, element size]; "first8" names the layouts whose comments promise the 8-byte arrays in front
// of the 4-byte ones (up to the part named there).
#include <stdio.h>

#include <string>
#include <vector>

#include "../camkifu_amd/csrc/ck_carve.h"
#include "../camkifu_amd/csrc/ck_stage_layout.h"

struct Part {
    std::string name;
    size_t off, bytes;
    int elem;
};

static std::string list_of(const std::vector<size_t>& v)
{
    std::string s = "[";
    for (size_t i = 0; i < v.size(); i++) s += (i ? ", " : "") + std::to_string(v[i]);
    return s + "]";
}

static void emit(const char* layout, const std::string& input, const std::vector<Part>& parts, size_t total, const char* extra = "")
{
    printf("{\"layout\": \"%s\", \"in\": {%s}, \"parts\": [", layout, input.c_str());
    for (size_t i = 0; i < parts.size(); i++)
        printf("%s[\"%s\", %zu, %zu, %d]", i ? ", " : "", parts[i].name.c_str(), parts[i].off, parts[i].bytes, parts[i].elem);
    printf("], \"total\": %zu%s}\n", total, extra);
}

static void huff(const std::vector<size_t>& seg_len, size_t ns, size_t n_sets, bool spans)
{
    const int frames = (int)seg_len.size();
    const CkHuffLayout L = ck_huff_layout(seg_len.data(), frames, ns, n_sets, spans);
    std::vector<Part> p;
    for (int f = 0; f < frames; f++) p.push_back({"seg" + std::to_string(f), L.seg[f], seg_len[f], 1});
    p.push_back({"slack", L.seg[frames], 16, 1});
    p.push_back({"rows", L.rows, ns * sizeof(CkStrand), 8});
    p.push_back({"sets", L.sets, n_sets * sizeof(CkHuffSet), 4});
    p.push_back({"quant", L.quant, (size_t)frames * 384, 2});
    if (spans) p.push_back({"span0", L.span0, (ns + 1) * 4, 4});
    const std::string extra = ", \"n_bytes\": " + std::to_string(L.n_bytes);
    emit("huff", "\"seg_len\": " + list_of(seg_len) + ", \"ns\": " + std::to_string(ns) + ", \"n_sets\": " + std::to_string(n_sets) +
                     ", \"spans\": " + std::to_string((int)spans), p, L.total, extra.c_str());
}

static void span(size_t n_spans, size_t bpm, size_t ns)
{
    const CkSpanLayout L = ck_span_layout(n_spans, bpm, ns);
    const size_t cand = n_spans * bpm;
    emit("jspan", "\"n_spans\": " + std::to_string(n_spans) + ", \"bpm\": " + std::to_string(bpm) + ", \"ns\": " + std::to_string(ns),
         {{"cand_a", L.cand_a, cand * 8, 8}, {"cand_x", L.cand_x, cand * 8, 8}, {"entry", L.entry, n_spans * 8, 8}, {"cand_c", L.cand_c, cand * 4, 4},
          {"ord", L.ord, n_spans * 4, 4}, {"flags", L.flags, ns * 4, 4}, {"unresolved", L.unresolved, ns * 4, 4}, {"verdict", L.verdict, ns * 4, 4}},
         L.total, ", \"first8\": \"verdict\"");
}

static void enc(int h, int w, int sampling, int ri, int m, bool optimise)
{
    const CkEncGeom g = ck_enc_geom(h, w, sampling, ri);
    const CkEncLayout L = ck_enc_layout(g, m, optimise);
    const size_t blocks = (size_t)m * g.blocks, tiles = (size_t)m * g.nseg * g.seg_tiles, segs = (size_t)m * g.nseg, M = (size_t)m;
    std::vector<Part> p = {{"head", L.head, 16, 8}, {"tile_off", L.tile_off, tiles * 8, 8}, {"seg_bits", L.seg_bits, segs * 8, 8},
                           {"seg_u0", L.seg_u0, (segs + M) * 8, 8}, {"frame_u0", L.frame_u0, (M + 1) * 8, 8}, {"len", L.len, M * 8, 8},
                           {"out_off", L.out_off, (M + 1) * 8, 8}, {"bits", L.bits, blocks * 4, 4}, {"tile_bits", L.tile_bits, tiles * 4, 4},
                           {"consts", L.consts, L.consts_bytes, 2}};
    if (optimise) {
        p.push_back({"freq", L.freq, M * 4 * 256 * 4, 4});
        p.push_back({"tables", L.tables, M * sizeof(CkEncTables), 2});
        p.push_back({"dht", L.dht, M * 4 * CK_ENC_DHT_SLOT, 1});
        p.push_back({"dht_len", L.dht_len, M * 4 * 4, 4});
        p.push_back({"headers", L.headers, M * CK_ENC_HEADER_SLOT, 1});
        p.push_back({"hlen", L.hlen, M * 4, 4});
    }
    const std::string extra = ", \"first8\": \"tile_bits\", \"consts_std\": " + std::to_string(L.consts_std) + ", \"consts_bytes\": " +
                              std::to_string(L.consts_bytes) + ", \"pin_words\": " + std::to_string(L.pin_words) + ", \"pin_total\": " +
                              std::to_string(L.pin_total);
    emit("jenc_work", "\"h\": " + std::to_string(h) + ", \"w\": " + std::to_string(w) + ", \"sampling\": " + std::to_string(sampling) + ", \"ri\": " +
                          std::to_string(ri) + ", \"m\": " + std::to_string(m) + ", \"optimise\": " + std::to_string((int)optimise), p, L.total, extra.c_str());
}

static void inflate(const std::vector<size_t>& zlen, size_t most)
{
    const int n = (int)zlen.size();
    const CkInflateLayout L = ck_inflate_layout(zlen.data(), n, most);
    std::vector<Part> p = {{"jobs", L.jobs, (size_t)n * sizeof(CkInfJob), 8}};
    for (int f = 0; f < n; f++) p.push_back({"z" + std::to_string(f), L.z[f], zlen[f], 1});
    p.push_back({"rec", L.rec, (size_t)n * sizeof(CkInfRecord), 8});
    p.push_back({"out", L.out, (size_t)n * L.dstride, 1});
    const std::string extra = ", \"dstride\": " + std::to_string(L.dstride);
    emit("png_inf", "\"zlen\": " + list_of(zlen) + ", \"most\": " + std::to_string(most), p, L.total, extra.c_str());
}

// inflated: h * (1 + rowbytes) of each frame; zlen empty: the host inflates
static void png_decode(const char* what, const std::vector<size_t>& inflated, const std::vector<size_t>& zlen)
{
    const int m = (int)inflated.size();
    const bool device = !zlen.empty();
    const CkPngDecodeLayout L = ck_png_decode_layout(inflated.data(), device ? zlen.data() : nullptr, m);
    std::vector<Part> p = {{"desc", L.desc, (size_t)m * sizeof(CkPngDesc), 8}, {"pal", L.pal, (size_t)m * 768, 1}};
    if (device) {
        p.push_back({"jobs", L.jobs, (size_t)m * sizeof(CkInfJob), 8});
        for (int i = 0; i < m; i++) p.push_back({"z" + std::to_string(i), L.z[i], zlen[i], 1});
        p.push_back({"rec", L.rec, (size_t)m * sizeof(CkInfRecord), 8});
    }
    for (int i = 0; i < m; i++) p.push_back({"rows" + std::to_string(i), L.rows[i], inflated[i], 1});
    const std::string extra = ", \"upload\": " + std::to_string(L.upload);
    emit(device ? "png_decode_device" : "png_decode_host",
         "\"what\": \"" + std::string(what) + "\", \"inflated\": " + list_of(inflated) + ", \"zlen\": " + list_of(zlen), p, L.total, extra.c_str());
}

static void png_work(int h, int w, int m, int runs)
{
    const CkPngGeom g = ck_png_geom(h, w);
    const CkPngWorkLayout L = ck_png_work_layout(g, m, runs);
    const size_t P = (size_t)ck_png_pitch(runs), bands = (size_t)m * g.bands, tiles = (size_t)m * g.tiles, M = (size_t)m;
    std::vector<Part> p = {{"head", L.head, (M + 1) * 8, 8}, {"tile_off", L.tile_off, tiles * 8, 8}, {"band_off", L.band_off, bands * 8, 8},
                           {"frame_bits", L.frame_bits, M * 8, 8}, {"out_off", L.out_off, (M + 1) * 8, 8}, {"count", L.count, bands * P * 4, 4},
                           {"tile_bits", L.tile_bits, tiles * 4, 4}, {"tile_a", L.tile_a, tiles * 4, 4}, {"tile_b", L.tile_b, tiles * 4, 4},
                           {"adler", L.adler, M * 4, 4}, {"band_bits", L.band_bits, bands * 8, 8}, {"band_a", L.band_a, bands * 4, 4},
                           {"band_b", L.band_b, bands * 4, 4}, {"codes", L.codes, bands * P * 2, 2}, {"lens", L.lens, bands * P, 1},
                           {"filt", L.filt, M * (size_t)g.fbytes, 1}};
    if (runs) {
        p.push_back({"before", L.before, tiles * 4, 4});
        p.push_back({"after", L.after, tiles * 4, 4});
        p.push_back({"edge", L.edge, tiles * sizeof(CkPngEdge), 2});
    }
    emit("png_work", "\"h\": " + std::to_string(h) + ", \"w\": " + std::to_string(w) + ", \"m\": " + std::to_string(m) + ", \"runs\": " + std::to_string(runs),
         p, L.total);
}

static void harvest(int n, int n_pos)
{
    const int nb = (int)(((long long)n * 100 + 1023) / 1024);        // ck_harvest_blocks
    const CkHarvestLayout L = ck_harvest_layout(n, n_pos, nb);
    emit("harvest", "\"n\": " + std::to_string(n) + ", \"n_pos\": " + std::to_string(n_pos) + ", \"nb\": " + std::to_string(nb),
         {{"state", L.state, (size_t)n * 4, 4}, {"pos", L.pos, (size_t)n_pos * 361 + 1, 1}, {"code", L.code, (size_t)n * 400, 4},
          {"blocks", L.blocks, ((size_t)nb + 1) * 4, 4}},
         L.total);
}

static void fit(int n, size_t frame_bytes, size_t budget)
{
    printf("{\"rule\": \"fit\", \"n\": %d, \"frame_bytes\": %zu, \"budget\": %zu, \"pass\": %d}\n", n, frame_bytes, budget, ck_pass_fit(n, frame_bytes, budget));
}
static void fit_hbm(int n, size_t frame_bytes, size_t budget, size_t cframe, size_t hbm)
{
    printf("{\"rule\": \"fit_hbm\", \"n\": %d, \"frame_bytes\": %zu, \"budget\": %zu, \"cframe\": %zu, \"hbm\": %zu, \"pass\": %d}\n", n, frame_bytes, budget,
           cframe, hbm, ck_pass_fit_hbm(n, frame_bytes, budget, cframe, hbm));
}
static void fit_streams(const std::vector<size_t>& len, size_t budget, size_t cframe, size_t hbm)
{
    printf("{\"rule\": \"fit_streams\", \"len\": %s, \"budget\": %zu, \"cframe\": %zu, \"hbm\": %zu, \"pass\": %d}\n", list_of(len).c_str(), budget, cframe, hbm,
           ck_pass_fit_streams((int)len.size(), len.data(), budget, cframe, hbm));
}
// every pass of a call over these frames: [first frame, frames, bytes of rows, bytes of streams]
static void take(const std::vector<size_t>& inflated, const std::vector<size_t>& zlen, size_t budget)
{
    const int n = (int)inflated.size();
    printf("{\"rule\": \"take\", \"inflated\": %s, \"zlen\": %s, \"budget\": %zu, \"passes\": [", list_of(inflated).c_str(), list_of(zlen).c_str(), budget);
    for (int f0 = 0, guard = 0; f0 < n && guard <= n; guard++) {
        size_t rows_bytes = 0, z_bytes = 0;
        const int m = ck_png_pass_take(inflated.data(), zlen.empty() ? nullptr : zlen.data(), f0, n, budget, &rows_bytes, &z_bytes);
        printf("%s[%d, %d, %zu, %zu]", f0 ? ", " : "", f0, m, rows_bytes, z_bytes);
        if (m <= 0) break;
        f0 += m;
    }
    printf("]}\n");
}

int main()
{
    for (int spans = 0; spans < 2; spans++) {
        for (size_t len : {0, 1, 15, 16, 17}) huff({len}, 1, 1, spans);
        huff({0, 1, 15}, 3, 1, spans);
        huff({16, 17, 1}, 4, 2, spans);
        huff({17, 17, 17}, 7, 3, spans);
    }
    span(1, 1, 1); span(3, 6, 3); span(5, 3, 2); span(4, 2, 4); span(7, 10, 5);
    for (int optimise = 0; optimise < 2; optimise++)
        for (int m : {1, 3}) {
            enc(8, 8, 0, 0, m, optimise);
            enc(17, 33, 3, 1, m, optimise);
            enc(64, 48, 1, 2, m, optimise);
        }
    inflate({0}, 0); inflate({1}, 5); inflate({15, 16}, 16); inflate({0, 17, 1}, 33); inflate({16, 0, 15}, 17);
    const std::vector<size_t> none;
    png_decode("one 1x1 rgb", {4}, none);            png_decode("one 1x1 rgb", {4}, {0});
    png_decode("one 5x3 palette, 4 bits", {12}, none);   png_decode("one 5x3 palette, 4 bits", {12}, {15});
    png_decode("two 5x3 rgb", {48, 48}, none);       png_decode("two 5x3 rgb", {48, 48}, {16, 17});
    png_decode("three, mixed types", {48, 12, 51}, none);   png_decode("three, mixed types", {48, 12, 51}, {1, 0, 33});
    for (int runs = 0; runs < 2; runs++)
        for (int m : {1, 3}) { png_work(1, 1, m, runs); png_work(17, 5, m, runs); png_work(33, 400, m, runs); }
    harvest(1, 0); harvest(3, 2); harvest(4, 3); harvest(11, 1);

    fit(5, 100, 99); fit(5, 100, 100); fit(5, 100, 499); fit(5, 100, 500); fit(5, 100, 501); fit(5, 100, 100000); fit(5, 0, 3); fit(1, 7, 0);
    fit_hbm(8, 10, 50, 1000, 3000); fit_hbm(8, 10, 50, 1000, 5000); fit_hbm(8, 10, 50, 1000, 999); fit_hbm(8, 10, 1000, 0, 4);
    fit_streams({100, 300, 200}, 1200, 64, 1000); fit_streams({100, 300, 200}, 1199, 64, 1000); fit_streams({100, 300, 200}, 10000, 64, 128);
    take({100, 10, 10}, none, 64);                                   // a first frame above the budget still goes
    take({16, 16, 32, 64}, none, 64);                                // frames that fill the budget exactly
    take({16, 16, 33, 64}, none, 64);                                // one byte over
    take({1, 15, 16, 17, 100, 0, 48, 48, 47, 49, 200, 3, 3, 3, 96, 1, 64, 32, 31, 33}, {5, 0, 17, 16, 1, 2, 3, 40, 15, 15, 0, 9, 9, 9, 30, 1, 2, 3, 4, 5}, 96);
    take({1, 15, 16, 17, 100, 0, 48, 48, 47, 49, 200, 3, 3, 3, 96, 1, 64, 32, 31, 33}, none, 1);
    take({1, 15, 16, 17, 100, 0, 48, 48, 47, 49, 200, 3, 3, 3, 96, 1, 64, 32, 31, 33}, none, 100000);
    return 0;
}
