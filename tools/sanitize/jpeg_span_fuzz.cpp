// jpeg_span_fuzz.cpp -- the steps of the span decoder the GPU kernels run (camkifu_amd/csrc/ck_jpeg_span.h through
// ck_jpeg_span.cpp, linked with ck_jpeg.cpp and ck_jpeg_plan.cpp on their own) under AddressSanitizer + UBSan, on the host:
// every case file given on the command line is decoded whole (must be CK_OK, with no suspect strand), truncated at every
// offset, with single-byte mutations at every offset of its scan and with a few thousand seeded mutations anywhere, at span
// sizes of 8 and 64 bytes.  Each input lives in a heap block of exactly its size, the staged bytes in one of exactly
// their size and the coefficients in one of exactly info.blocks * 64 values, so a read or write one byte outside is caught.
// Every input also goes through the host decoder (ck_jpeg_entropy): the two must take the same accept / refuse decision
// with the same message and, when they accept, give the same coefficients and quant tables.  Every refused variant whose
// headers are whole is also put into a batch of five: the first bad frame and its message must be the host decoder's.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I include tools/sanitize/jpeg_span_fuzz.cpp \
//       camkifu_amd/csrc/ck_jpeg.cpp camkifu_amd/csrc/ck_jpeg_plan.cpp camkifu_amd/csrc/ck_jpeg_span.cpp
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../camkifu_amd/csrc/ck_jpeg_span.h"

static long g_ok = 0, g_refused = 0, g_unresolved = 0, g_suspect = 0, g_one_lane_ok = 0;
static const int SPANS[2] = {8, 64};

static void die(const char* what, const char* msg)
{
    fprintf(stderr, "%s (%s)\n", what, msg);
    exit(2);
}

// -> status of the span decode; ends the program on anything that must not occur
static int run(const uint8_t* src, size_t len, bool must_be_clean)
{
    std::unique_ptr<uint8_t[]> data(new uint8_t[len ? len : 1]);
    memcpy(data.get(), src, len);
    auto f = std::make_unique<CkJpegFrame>();
    char msg[CK_JPEG_MSG];
    int rc = ck_jpeg_parse(data.get(), len, f.get(), msg);
    if (rc != CK_OK) {
        if (rc != CK_ERR_DATA) die("status of the parser", msg);
        g_refused++;
        return rc;
    }
    if (f->info.blocks > (1 << 16)) { g_refused++; return CK_ERR_DATA; }      // (a mutated size: the caller's geometry check refuses it)
    const size_t nc = (size_t)f->info.blocks * 64;
    std::unique_ptr<int16_t[]> ref(new int16_t[nc]), got(new int16_t[nc]);
    rc = ck_jpeg_entropy(data.get(), len, *f, ref.get(), msg);
    const uint8_t* one[1] = {data.get()};
    const size_t lens[1] = {len};
    int last = CK_OK;
    for (int span : SPANS) {
        uint16_t quant[192];
        char smsg[CK_JPEG_MSG] = {0};
        long long st[CK_SPAN_STATS];
        int bad = -1;
        const int src_rc = ck_jpeg_spans_host(one, lens, 1, f->info, span, got.get(), quant, &bad, smsg, st);
        if (src_rc != CK_OK && src_rc != CK_ERR_DATA) die("status of the span decoder", smsg);
        if (src_rc != CK_OK && (!smsg[0] || bad != 0)) die("a refusal without a message or a frame", smsg);
        if ((rc == CK_OK) != (src_rc == CK_OK)) { fprintf(stderr, "host: %d %s\nspans: %d %s\n", rc, msg, src_rc, smsg); die("the decisions differ", ""); }
        if (rc != CK_OK && strcmp(msg, smsg)) { fprintf(stderr, "host: %s\nspans: %s\n", msg, smsg); die("the messages differ", ""); }
        if (rc == CK_OK) {
            if (memcmp(ref.get(), got.get(), nc * sizeof(int16_t))) die("the coefficients differ", "");
            if (memcmp(quant, f->quant, sizeof quant)) die("the quant tables differ", "");
            if (st[2]) g_one_lane_ok++;
        }
        if (must_be_clean && (st[2] || st[3])) die("a suspect strand in an undamaged stream", "");
        if (st[1] > st[0] || st[3] > 1) die("the statistics do not add up", "");
        g_unresolved += st[1];
        g_suspect += st[2];
        (src_rc == CK_OK ? g_ok : g_refused)++;
        last = src_rc;
    }
    return last;
}

// one call of n streams against the host decoder frame by frame: the status, the first bad frame, its message, every byte
static int run_call(const std::vector<std::vector<uint8_t>>& streams, const ck_jpeg_info& geom)
{
    const int n = (int)streams.size();
    std::vector<const uint8_t*> ptr;
    std::vector<size_t> len;
    for (auto& s : streams) { ptr.push_back(s.data()); len.push_back(s.size()); }
    const size_t nc = (size_t)geom.blocks * 64;
    std::vector<int16_t> got(nc * n), ref(nc * n);
    std::vector<uint16_t> q(192 * n);
    char m3[CK_JPEG_MSG] = {0};
    int want = -1;
    auto fr = std::make_unique<CkJpegFrame>();
    for (int f = 0; f < n && want < 0; f++) {
        int rc = ck_jpeg_parse(ptr[f], len[f], fr.get(), m3);
        if (rc == CK_OK && (fr->info.h != geom.h || fr->info.w != geom.w || fr->info.sampling != geom.sampling)) rc = CK_ERR_DATA;
        if (rc == CK_OK) rc = ck_jpeg_entropy(ptr[f], len[f], *fr, ref.data() + nc * f, m3);
        if (rc != CK_OK) want = f;
    }
    int r1 = CK_OK;
    for (int span : SPANS) {
        char m1[CK_JPEG_MSG] = {0};
        long long st[CK_SPAN_STATS];
        int b1 = -1;
        r1 = ck_jpeg_spans_host(ptr.data(), len.data(), n, geom, span, got.data(), q.data(), &b1, m1, st);
        if ((r1 == CK_OK) != (want < 0) || (r1 != CK_OK && (b1 != want || strcmp(m1, m3)))) {
            fprintf(stderr, "host: first bad frame %d (%s); spans: status %d, frame %d (%s)\n", want, m3, r1, b1, m1);
            die("the first bad frame of a call or its message differs", "");
        }
        if (r1 == CK_OK && memcmp(got.data(), ref.data(), nc * n * 2)) die("the bytes of a call differ from the host decoder's", "");
        (r1 == CK_OK ? g_ok : g_refused)++;
    }
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
    if (argc < 2) { fprintf(stderr, "usage: jpeg_span_fuzz case.jpg ...\n"); return 2; }
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    for (int a = 1; a < argc; a++) {
        std::vector<uint8_t> buf = read_file(argv[a]);
        if (run(buf.data(), buf.size(), true) != CK_OK) { fprintf(stderr, "%s does not decode\n", argv[a]); return 2; }
        auto f = std::make_unique<CkJpegFrame>();
        char msg[CK_JPEG_MSG];
        if (ck_jpeg_parse(buf.data(), buf.size(), f.get(), msg) != CK_OK) return 2;
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
            if (run(buf.data(), cut, false) != CK_OK && cut >= f->scan) in_batch(buf.data(), cut);
        std::vector<uint8_t> m(buf);
        for (size_t at = f->scan; at < buf.size(); at++) {              // the scan, byte by byte: to FF, to 00, a marker, a flipped bit
            const uint8_t old = m[at];
            const uint8_t vals[4] = {0xFF, 0x00, (uint8_t)(0xD0 + (at & 7)), (uint8_t)(old ^ (1u << (at & 7)))};
            for (int v = 0; v < 4; v++) {
                if (vals[v] == old) continue;
                m[at] = vals[v];
                if (run(m.data(), m.size(), false) != CK_OK) in_batch(m.data(), m.size());
            }
            m[at] = old;
        }
        for (int k = 0; k < 3000; k++) {
            const size_t at = (size_t)(next() % buf.size());
            const uint8_t old = m[at];
            m[at] = (uint8_t)(next() >> 11);
            run(m.data(), m.size(), false);
            m[at] = old;
        }
    }
    printf("jpeg span decoder: %d cases at spans of 8 and 64 bytes, %ld decodes clean and equal to the host decoder, message for message "
           "(%ld accepted, %ld refused; %ld unresolved spans, %ld suspect strands, %ld decodes accepted through the one-lane decoder)\n",
           argc - 1, g_ok + g_refused, g_ok, g_refused, g_unresolved, g_suspect, g_one_lane_ok);
    return 0;
}
