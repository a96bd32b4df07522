// jpeg_strand_fuzz.cpp -- the planner and the strand decoder the GPU kernel runs (camkifu_amd/csrc/ck_jpeg_plan.cpp and
// ck_jpeg_strand.h, linked with ck_jpeg.cpp on their own) under AddressSanitizer + UBSan, on the host: every case file given
// on the command line is decoded whole (must be CK_OK), truncated at every offset, with a single-byte mutation at every
// offset of its scan and with a few thousand seeded mutations anywhere.  Each input lives in a heap block of exactly its
// size and the coefficients in one of exactly info.blocks * 64 values, so a read or write one byte outside either is
// caught.  Every input also goes through the host decoder (ck_jpeg_entropy): the two must take the same accept / refuse
// decision and, when they accept, give the same coefficients and quant tables -- in both strand orders.  Every refused
// variant whose headers are whole is also put into a batch of five (the first bad frame must be the host decoder's), and
// `--call a.jpg b.jpg ...` decodes the files as one call in both strand orders.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I include tools/sanitize/jpeg_strand_fuzz.cpp \
//       camkifu_amd/csrc/ck_jpeg.cpp camkifu_amd/csrc/ck_jpeg_plan.cpp
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../camkifu_amd/csrc/ck_jpeg_strand.h"

static long g_ok = 0, g_refused = 0, g_special = 0;

static void die(const char* what, const char* msg)
{
    fprintf(stderr, "%s (%s)\n", what, msg);
    exit(2);
}

// -> status of the strand decode; ends the program on anything that must not occur
static int run(const uint8_t* src, size_t len)
{
    std::unique_ptr<uint8_t[]> data(new uint8_t[len ? len : 1]);
    memcpy(data.get(), src, len);
    auto f = std::make_unique<CkJpegFrame>();
    char msg[CK_JPEG_MSG], smsg[CK_JPEG_MSG] = {0};
    int rc = ck_jpeg_parse(data.get(), len, f.get(), msg);
    if (rc != CK_OK) {
        if (rc != CK_ERR_DATA) die("status of the parser", msg);
        g_refused++;
        return rc;
    }
    if (f->info.blocks > (1 << 16)) { g_refused++; return CK_ERR_DATA; }      // (a mutated size: the caller's geometry check refuses it)
    const size_t nc = (size_t)f->info.blocks * 64;
    std::unique_ptr<int16_t[]> ref(new int16_t[nc]), got(new int16_t[nc]), rev(new int16_t[nc]);
    uint16_t quant[192], rquant[192];
    rc = ck_jpeg_entropy(data.get(), len, *f, ref.get(), msg);
    const uint8_t* one[1] = {data.get()};
    const size_t lens[1] = {len};
    int bad = -1;
    const int src_rc = ck_jpeg_strands_host(one, lens, 1, f->info, got.get(), quant, false, &bad, smsg);
    if (src_rc != CK_OK && src_rc != CK_ERR_DATA) die("status of the strand decoder", smsg);
    if (src_rc != CK_OK && (!smsg[0] || bad != 0)) die("a refusal without a message or a frame", smsg);
    if ((rc == CK_OK) != (src_rc == CK_OK)) { fprintf(stderr, "host: %d %s\nstrands: %d %s\n", rc, msg, src_rc, smsg); die("the decisions differ", ""); }
    if (rc == CK_OK) {
        if (memcmp(ref.get(), got.get(), nc * sizeof(int16_t))) die("the coefficients differ", "");
        if (memcmp(quant, f->quant, sizeof quant)) die("the quant tables differ", "");
    }
    if (src_rc == CK_OK && f->ncomp == 3 && (memcmp(f->dc[1].look, f->dc[2].look, sizeof f->dc[1].look) || memcmp(f->ac[1].look, f->ac[2].look, sizeof f->ac[1].look)))
        g_special++;                                                    // (accepted with other tables for Cr than for Cb)
    char rmsg[CK_JPEG_MSG] = {0};
    const int rev_rc = ck_jpeg_strands_host(one, lens, 1, f->info, rev.get(), rquant, true, &bad, rmsg);
    if (rev_rc != src_rc) die("the decision depends on the order of the strands", rmsg);
    if (rev_rc == CK_OK && memcmp(rev.get(), got.get(), nc * sizeof(int16_t))) die("the coefficients depend on the order of the strands", "");
    (src_rc == CK_OK ? g_ok : g_refused)++;
    return src_rc;
}

// one call of n streams: the strand decoder first strand first and last strand first, and the host decoder frame by frame.
// The three must agree on the status, on the first bad frame and, when all frames are accepted, on every byte.
static int run_call(const std::vector<std::vector<uint8_t>>& streams, const ck_jpeg_info& geom)
{
    const int n = (int)streams.size();
    std::vector<const uint8_t*> ptr;
    std::vector<size_t> len;
    for (auto& s : streams) { ptr.push_back(s.data()); len.push_back(s.size()); }
    const size_t nc = (size_t)geom.blocks * 64;
    std::vector<int16_t> fwd(nc * n), rev(nc * n), ref(nc * n);
    std::vector<uint16_t> q1(192 * n), q2(192 * n);
    char m1[CK_JPEG_MSG] = {0}, m2[CK_JPEG_MSG] = {0}, m3[CK_JPEG_MSG] = {0};
    int b1 = -1, b2 = -1, want = -1;
    const int r1 = ck_jpeg_strands_host(ptr.data(), len.data(), n, geom, fwd.data(), q1.data(), false, &b1, m1);
    const int r2 = ck_jpeg_strands_host(ptr.data(), len.data(), n, geom, rev.data(), q2.data(), true, &b2, m2);
    auto fr = std::make_unique<CkJpegFrame>();
    for (int f = 0; f < n && want < 0; f++) {
        int rc = ck_jpeg_parse(ptr[f], len[f], fr.get(), m3);
        if (rc == CK_OK && (fr->info.h != geom.h || fr->info.w != geom.w || fr->info.sampling != geom.sampling)) rc = CK_ERR_DATA;
        if (rc == CK_OK) rc = ck_jpeg_entropy(ptr[f], len[f], *fr, ref.data() + nc * f, m3);
        if (rc != CK_OK) want = f;
    }
    if (r1 != r2 || b1 != b2) die("the decision of a call depends on the order of the strands", m2);
    if ((r1 == CK_OK) != (want < 0) || (r1 != CK_OK && b1 != want)) {
        fprintf(stderr, "host: first bad frame %d; strands: status %d, frame %d (%s)\n", want, r1, b1, m1);
        die("the first bad frame of a call differs", "");
    }
    if (r1 == CK_OK && (memcmp(fwd.data(), rev.data(), nc * n * 2) || memcmp(fwd.data(), ref.data(), nc * n * 2) || q1 != q2))
        die("the bytes of a call depend on the order of the strands, or differ from the host decoder's", "");
    (r1 == CK_OK ? g_ok : g_refused)++;
    return r1;
}

static std::vector<uint8_t> read_file(const char* path)
{
    FILE* fp = fopen(path, "rb");
    if (!fp) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    std::vector<uint8_t> buf;
    uint8_t chunk[4096];
    for (size_t k; (k = fread(chunk, 1, sizeof chunk, fp)) > 0;) buf.insert(buf.end(), chunk, chunk + k);
    fclose(fp);
    return buf;
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: jpeg_strand_fuzz [--call] case.jpg ...\n"); return 2; }
    if (!strcmp(argv[1], "--call")) {
        // the files, all of one geometry, as ONE call: whole, and with each frame in turn cut in half
        std::vector<std::vector<uint8_t>> streams;
        for (int a = 2; a < argc; a++) streams.push_back(read_file(argv[a]));
        auto f = std::make_unique<CkJpegFrame>();
        char msg[CK_JPEG_MSG];
        if (streams.empty() || ck_jpeg_parse(streams[0].data(), streams[0].size(), f.get(), msg) != CK_OK) return 2;
        if (run_call(streams, f->info) != CK_OK) { fprintf(stderr, "the call does not decode\n"); return 2; }
        for (size_t k = 0; k < streams.size(); k++) {
            auto cut = streams;
            cut[k].resize(cut[k].size() - (cut[k].size() - f->scan) / 2);
            run_call(cut, f->info);
        }
        printf("jpeg strand decoder: one call of %zu frames, whole and with each frame cut: both strand orders give the host decoder's bytes and first bad frame\n",
               streams.size());
        return 0;
    }
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    for (int a = 1; a < argc; a++) {
        std::vector<uint8_t> buf = read_file(argv[a]);
        if (run(buf.data(), buf.size()) != CK_OK) { fprintf(stderr, "%s does not decode\n", argv[a]); return 2; }
        auto f = std::make_unique<CkJpegFrame>();
        char msg[CK_JPEG_MSG];
        if (ck_jpeg_parse(buf.data(), buf.size(), f.get(), msg) != CK_OK) return 2;
        // a refused variant whose headers are whole also goes into a batch of five good frames, at place 1 .. 4 in turn, with
        // the refused variant before it behind it: the first bad frame must be the host decoder's
        std::vector<uint8_t> before;
        long place = 0;
        auto in_batch = [&](const uint8_t* p, size_t n) {
            std::vector<std::vector<uint8_t>> five(5, buf);
            const int at = 1 + (int)(place++ % 4);
            five[at].assign(p, p + n);
            if (at < 4 && !before.empty()) five[4] = before;
            run_call(five, f->info);
            before.assign(p, p + n);
        };
        for (size_t cut = 0; cut < buf.size(); cut++)
            if (run(buf.data(), cut) != CK_OK && cut >= f->scan) in_batch(buf.data(), cut);
        std::vector<uint8_t> m(buf);
        for (size_t at = f->scan; at < buf.size(); at++) {              // the scan, byte by byte: to FF, to 00, a marker, a flipped bit
            const uint8_t old = m[at];
            const uint8_t vals[4] = {0xFF, 0x00, (uint8_t)(0xD0 + (at & 7)), (uint8_t)(old ^ (1u << (at & 7)))};
            for (int v = 0; v < 4; v++) {
                if (vals[v] == old) continue;
                m[at] = vals[v];
                if (run(m.data(), m.size()) != CK_OK) in_batch(m.data(), m.size());
            }
            m[at] = old;
        }
        for (int k = 0; k < 3000; k++) {
            const size_t at = (size_t)(next() % buf.size());
            const uint8_t old = m[at];
            m[at] = (uint8_t)(next() >> 11);
            run(m.data(), m.size());
            m[at] = old;
        }
    }
    printf("jpeg strand decoder: %d cases, %ld decodes clean and equal to the host decoder (%ld accepted, %ld refused; %ld accepted with tables of their own for Cr)\n",
           argc - 1, g_ok + g_refused, g_ok, g_refused, g_special);
    return 0;
}
