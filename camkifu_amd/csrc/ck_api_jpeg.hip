// ck_api_jpeg.hip -- the baseline JPEG entry points of libck_hip.so (see include/camkifu_amd.h): decode and encode, the
// Huffman stages on the host and on the device.  Host-side glue only, as ck_api.hip; where the parts of a staged block lie
// and how many frames go into a pass is ck_stage_layout.h's.
#include <stdlib.h>

#include <vector>

#include "ck_common.h"
#include "ck_api_util.h"
#include "ck_stage_layout.h"
#include "ck_jpeg.h"
#include "ck_jpeg_strand.h"
#include "ck_jpeg_span.h"
#include "ck_jpeg_enc.h"

extern "C" {

// ---- baseline JPEG: host half (ck_jpeg.cpp) behind the ABI, and the two calls that reach the GPU ----
int ck_jpeg_probe(const uint8_t* data, size_t len, ck_jpeg_info* info)
{
    if (!info) return ck_fail(nullptr, CK_ERR_ARG, "info is NULL");
    CK_HOST_BEGIN
    auto f = std::make_unique<CkJpegFrame>();
    char msg[CK_JPEG_MSG];
    const int rc = ck_jpeg_parse(data, len, f.get(), msg);
    if (rc != CK_OK) return ck_fail(nullptr, rc, "%s", msg);
    *info = f->info;
    return CK_OK;
    CK_HOST_END
}

// the Huffman stage of n frames, in parallel: coef n * geom.blocks * 64, quant n * 192.  On failure *bad is the first
// frame that failed and `why` its message.
static int jpeg_entropy_batch(const uint8_t* const* data, const size_t* len, int n, const ck_jpeg_info& geom, int16_t* coef,
                              uint16_t* quant, int* bad, std::string& why)
{
    std::vector<int> rcs((size_t)n, CK_OK);
    std::vector<std::string> msgs((size_t)n);
    ck_parallel_for(n, 16, [&](int f) {
        auto fr = std::make_unique<CkJpegFrame>();
        char msg[CK_JPEG_MSG];
        int rc = ck_jpeg_parse(data[f], len[f], fr.get(), msg);
        if (rc == CK_OK && (fr->info.h != geom.h || fr->info.w != geom.w || fr->info.sampling != geom.sampling)) {
            snprintf(msg, sizeof msg, "%dx%d sampling %d where the batch is %dx%d sampling %d", fr->info.w, fr->info.h,
                     fr->info.sampling, geom.w, geom.h, geom.sampling);
            rc = CK_ERR_DATA;
        }
        if (rc == CK_OK) rc = ck_jpeg_entropy(data[f], len[f], *fr, coef + (size_t)f * geom.blocks * 64, msg);
        if (rc == CK_OK) memcpy(quant + (size_t)f * 192, fr->quant, 192 * sizeof(uint16_t));
        rcs[f] = rc;
        if (rc != CK_OK) msgs[f] = msg;
    });
    for (int f = 0; f < n; f++)
        if (rcs[f] != CK_OK) { *bad = f; why = msgs[f]; return rcs[f]; }
    return CK_OK;
}

static int check_jpeg_geom(ck_ctx* ctx, int h, int w, int sampling, long long blocks)
{
    if (h <= 0 || w <= 0 || h > 65535 || w > 65535) return ck_fail(ctx, CK_ERR_ARG, "bad JPEG frame size %dx%d", w, h);
    if (sampling < CK_JPEG_GREY || sampling > CK_JPEG_420) return ck_fail(ctx, CK_ERR_ARG, "bad JPEG sampling %d", sampling);
    if (blocks >= 0 && blocks != ck_jpeg_blocks(h, w, sampling))
        return ck_fail(ctx, CK_ERR_ARG, "%lld blocks where a %dx%d frame of sampling %d has %lld", blocks, w, h, sampling,
                       ck_jpeg_blocks(h, w, sampling));
    if ((long long)h * w > (1LL << 28)) return ck_fail(ctx, CK_ERR_ARG, "image too large");
    return CK_OK;
}

int ck_jpeg_coefficients(const uint8_t* const* data, const size_t* len, int n, const ck_jpeg_info* geom,
                         int16_t* coef, uint16_t* quant, int32_t* bad_frame)
{
    if (bad_frame) *bad_frame = -1;
    if (!data || !len || !geom || !coef || !quant || n <= 0) return ck_fail(nullptr, CK_ERR_ARG, "NULL pointer or n <= 0");
    CK_TRY(check_jpeg_geom(nullptr, geom->h, geom->w, geom->sampling, geom->blocks));
    CK_HOST_BEGIN
    int bad = -1;
    std::string why;
    const int rc = jpeg_entropy_batch(data, len, n, *geom, coef, quant, &bad, why);
    if (rc != CK_OK) {
        if (bad_frame) *bad_frame = bad;
        return ck_fail(nullptr, rc, "frame %d: %s", bad, why.c_str());
    }
    return CK_OK;
    CK_HOST_END
}

int ck_jpeg_reconstruct(ck_ctx* ctx, const int16_t* coef, const uint16_t* quant, int n, int h, int w, int sampling,
                        int in_space, uint8_t* bgr, int out_space)
{
    CK_API_BEGIN(ctx)
    if (!coef || !quant || !bgr || n <= 0) return ck_fail(ctx, CK_ERR_ARG, "NULL pointer or n <= 0");
    CK_TRY(check_jpeg_geom(ctx, h, w, sampling, -1));
    const size_t cbytes = (size_t)n * (size_t)ck_jpeg_blocks(h, w, sampling) * 64 * sizeof(int16_t);
    const void *d_coef, *d_quant;
    CK_TRY(ck_to_device(ctx, coef, cbytes, in_space, ctx->in_stage, &d_coef));
    CK_TRY(ck_to_device(ctx, quant, (size_t)n * 192 * sizeof(uint16_t), in_space, ctx->in_stage2, &d_quant));
    CK_TRY(ck_coef_quant_on_16(ctx, d_coef, d_quant));
    OutStage<uint8_t> o;
    CK_TRY(o.open(ctx, bgr, (size_t)n * h * w * 3, out_space, ctx->out_stage));
    CK_TRY(k_jpeg_reconstruct(ctx, (const int16_t*)d_coef, (const uint16_t*)d_quant, n, h, w, sampling, o.dev));
    CK_TRY(o.deliver(ctx));
    return finish(ctx);
    CK_API_END(ctx)
}

// frames per pass of ck_jpeg_decode: the pinned block and its device twin hold the coefficients of one pass, not of the
// whole batch (a 1080p 4:2:0 frame is 6.2 MB of coefficients, a batch of 256 would pin 1.6 GB) -- 256 MB, or what
// CK_JPEG_PASS_BYTES says (a developer knob: the tests set it to a few KB to run several passes on small frames)
static size_t jpeg_pass_budget()
{
    if (const char* e = getenv("CK_JPEG_PASS_BYTES")) {
        const long long v = atoll(e);
        if (v > 0) return (size_t)v;
    }
    return (size_t)256 << 20;
}
static int jpeg_pass_frames(int n, size_t frame_bytes) { return ck_pass_fit(n, frame_bytes, jpeg_pass_budget()); }

// frames per pass in the device entropy mode: the same rule applied to what that mode stages.  Its pinned block and device
// twin hold the COMPRESSED bytes of a pass (plan rows, table sets and quant tables are small beside them), so the budget
// buys many more frames -- and the kernel needs them: one lane per strand, so a pass is as fast as its longest strand
// however many strands it has.  The coefficients of a pass exist in HBM only; they are held to 2 GiB.
static const size_t JPEG_PASS_HBM = (size_t)2 << 30;
static int jpeg_pass_frames_device(int n, const size_t* len, size_t cframe) { return ck_pass_fit_streams(n, len, jpeg_pass_budget(), cframe, JPEG_PASS_HBM); }
// and in the encoder's device mode: ck_jpeg_encode's rule, the coefficients of a pass held to the same 2 GiB of HBM
static int jpeg_enc_pass_frames_device(int n, size_t cframe) { return ck_pass_fit_hbm(n, cframe, jpeg_pass_budget(), cframe, JPEG_PASS_HBM); }

// The Huffman stage of m frames on the GPU (CK_JPEG_ENTROPY_DEVICE), one pass: the plan on the host, then the entropy-coded
// segments (each starting on 16 bytes, zeroed slack behind the last), the plan rows, the table sets and the quant tables in
// the context's pinned block -> one upload -> k_jpeg_huff -> the status words down.  d_coef: m * geom.blocks * 64 int16 on
// the device.  *d_quant: the m * 192 quant tables in HBM (inside in_stage2, 16-byte aligned), h_quant (nullable): the same
// on the host.  Returns with the stream idle.  On a refusal *bad is the lowest frame with a failed strand (or the frame
// the planner refused, when no frame before it failed) and `why` the cause at its lowest MCU; a failure that is no frame's
// fault (HIP, memory) leaves *bad at -1 and its message in the context.
// span_bytes > 0 (CK_JPEG_ENTROPY_DEVICE_SPANS): the first span of every strand goes up behind the quant tables, the five
// steps of k_jpeg_span.hip decode, the verdict words come down, and only the frames that hold a suspect strand go through
// k_jpeg_huff (k_jpeg_huff_frame), whose status words decide as above; every other strand's status is 0.
static int jpeg_huff_pass(ck_ctx* ctx, const uint8_t* const* data, const size_t* len, int m, const ck_jpeg_info& geom,
                          int16_t* d_coef, const uint16_t** d_quant, uint16_t* h_quant, int* bad, std::string& why, int span_bytes = 0)
{
    CkJpegPlan plan;
    const int prc = ck_jpeg_plan_build(data, len, m, geom, &plan);
    if (prc != CK_OK && prc != CK_ERR_DATA) { *bad = plan.frames; why = plan.msg; return prc; }
    const int frames = plan.frames;
    const size_t ns = plan.strands.size();
    if (ns > 0x7fffffff) return ck_fail(ctx, CK_ERR_ARG, "%zu strands in one pass", ns);
    if (ns) {
        std::vector<size_t> seg_len((size_t)frames);               // the entropy-coded segment of each frame
        for (int f = 0; f < frames; f++) seg_len[f] = len[f] - plan.scan[f];
        const CkHuffLayout L = ck_huff_layout(seg_len.data(), frames, ns, plan.sets.size(), span_bytes > 0);
        const std::vector<size_t>& seg = L.seg;
        const size_t n_bytes = L.n_bytes, total = L.total;
        CK_TRY(ck_ensure_pinned(ctx, ctx->host_pinned, total));
        uint8_t* hp = (uint8_t*)ctx->host_pinned.p;
        for (int f = 0; f < frames; f++) {                         // each segment, and zeros up to the next (behind the last: the slack)
            memcpy(hp + seg[f], data[f] + plan.scan[f], seg_len[f]);
            memset(hp + seg[f] + seg_len[f], 0, (f + 1 < frames ? seg[f + 1] : n_bytes) - seg[f] - seg_len[f]);
        }
        CkStrand* rows = (CkStrand*)(hp + L.rows);
        for (size_t s = 0; s < ns; s++) {
            rows[s] = plan.strands[s];
            const int64_t shift = (int64_t)seg[(size_t)rows[s].frame] - (int64_t)plan.scan[(size_t)rows[s].frame];
            rows[s].begin += shift;
            rows[s].end += shift;
        }
        memcpy(hp + L.sets, plan.sets.data(), plan.sets.size() * sizeof(CkHuffSet));
        memcpy(hp + L.quant, plan.quant.data(), (size_t)frames * 192 * sizeof(uint16_t));
        long long n_spans = 0;
        if (span_bytes > 0) {
            int32_t* span0 = (int32_t*)(hp + L.span0);
            for (size_t s = 0; s < ns; s++) {
                span0[s] = (int32_t)n_spans;
                n_spans += ck_span_count(rows[s].end - rows[s].begin, span_bytes);
                if (n_spans > 0x7fffffff / 8) return ck_fail(ctx, CK_ERR_ARG, "%lld spans in one pass", n_spans);
            }
            span0[ns] = (int32_t)n_spans;
        }
        const void* d_in;
        CK_TRY(ck_to_device(ctx, hp, total, CK_HOST, ctx->in_stage2, &d_in));
        ctx->jpeg_uploaded += (long long)total;
        const uint8_t* d = (const uint8_t*)d_in;
        CK_TRY(ck_ensure(ctx, ctx->misc, ns * sizeof(uint32_t)));
        CK_TRY(ck_ensure_pinned(ctx, ctx->host_pinned2, ns * sizeof(uint32_t)));
        uint32_t* status = (uint32_t*)ctx->host_pinned2.p;
        if (span_bytes > 0) {
            CkSpanJob J{};
            J.bytes = d; J.n_bytes = (long long)n_bytes;
            J.rows = (const CkStrand*)(d + L.rows); J.n_strands = (int)ns;
            J.span0 = (const int32_t*)(d + L.span0);
            J.sets = (const CkHuffSet*)(d + L.sets); J.n_sets = (int)plan.sets.size();
            J.g = plan.g; J.cframe = (long long)geom.blocks * 64; J.n_frames = frames; J.span_bytes = span_bytes; J.bpm = ck_span_bpm(plan.g);
            // the work arrays of the pass
            const CkSpanLayout W = ck_span_layout((size_t)n_spans, (size_t)J.bpm, ns);
            CK_TRY(ck_ensure(ctx, ctx->jspan, W.total));
            uint8_t* wk = (uint8_t*)ctx->jspan.p;
            J.cand_a = (uint64_t*)(wk + W.cand_a); J.cand_x = (uint64_t*)(wk + W.cand_x); J.entry = (uint64_t*)(wk + W.entry);
            J.cand_c = (uint32_t*)(wk + W.cand_c); J.ord = (int32_t*)(wk + W.ord);
            J.flags = (uint32_t*)(wk + W.flags); J.unresolved = (uint32_t*)(wk + W.unresolved); J.verdict = (uint32_t*)(wk + W.verdict);
            J.coef = d_coef;
            CK_TRY(k_jpeg_span(ctx, J, n_spans));
            CK_HIP(ctx, hipMemcpyAsync(status, J.verdict, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            CK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            // the frames that hold a suspect strand (their rows lie together: the plan is frame-major)
            std::vector<int> first_row((size_t)frames, -1), n_rows((size_t)frames, 0);
            std::vector<uint8_t> again((size_t)frames, 0);
            ctx->jpeg_span_stats[0] += n_spans;
            bool any = false;
            for (size_t s = 0; s < ns; s++) {
                const size_t f = (size_t)plan.strands[s].frame;
                if (first_row[f] < 0) first_row[f] = (int)s;
                n_rows[f]++;
                ctx->jpeg_span_stats[1] += status[s] >> 1;
                if (status[s] & 1) { ctx->jpeg_span_stats[2]++; again[f] = 1; any = true; }
            }
            memset(status, 0, ns * sizeof(uint32_t));
            if (any) {
                CK_HIP(ctx, hipMemsetAsync(ctx->misc.p, 0, ns * sizeof(uint32_t), ctx->stream));
                for (int f = 0; f < frames; f++)
                    if (again[f]) {
                        ctx->jpeg_span_stats[3]++;
                        CK_TRY(k_jpeg_huff_frame(ctx, d, (long long)n_bytes, J.rows, first_row[f], n_rows[f], J.sets, J.n_sets, plan.g, J.cframe,
                                                 frames, f, d_coef, (uint32_t*)ctx->misc.p));
                    }
                CK_HIP(ctx, hipMemcpyAsync(status, ctx->misc.p, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
                CK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            }
        } else {
            CK_TRY(k_jpeg_huff(ctx, d, (long long)n_bytes, (const CkStrand*)(d + L.rows), (int)ns, (const CkHuffSet*)(d + L.sets),
                               (int)plan.sets.size(), plan.g, (long long)geom.blocks * 64, frames, d_coef, (uint32_t*)ctx->misc.p));
            CK_HIP(ctx, hipMemcpyAsync(status, ctx->misc.p, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            CK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        for (size_t s = 0; s < ns; s++)
            if (status[s]) {
                char msg[CK_JPEG_MSG];
                *bad = (int)plan.strands[s].frame;
                ck_strand_message(status[s], plan.ri[(size_t)*bad], msg);
                why = msg;
                return CK_ERR_DATA;
            }
        *d_quant = (const uint16_t*)(d + L.quant);
        if (h_quant) memcpy(h_quant, plan.quant.data(), (size_t)frames * 192 * sizeof(uint16_t));
    }
    if (prc != CK_OK) { *bad = plan.frames; why = plan.msg; return prc; }
    return CK_OK;
}

int ck_jpeg_set_entropy(ck_ctx* ctx, int mode)
{
    CK_API_BEGIN(ctx)
    if (mode != CK_JPEG_ENTROPY_HOST && mode != CK_JPEG_ENTROPY_DEVICE && mode != CK_JPEG_ENTROPY_DEVICE_SPANS)
        return ck_fail(ctx, CK_ERR_ARG, "unknown JPEG entropy mode %d", mode);
    ctx->jpeg_entropy = mode;
    return CK_OK;
    CK_API_END(ctx)
}

int ck_jpeg_set_span_bytes(ck_ctx* ctx, int bytes)
{
    CK_API_BEGIN(ctx)
    if (bytes < CK_SPAN_MIN || bytes > CK_SPAN_MAX) return ck_fail(ctx, CK_ERR_ARG, "span size %d outside %d .. %d bytes", bytes, CK_SPAN_MIN, CK_SPAN_MAX);
    ctx->jpeg_span_bytes = bytes;
    return CK_OK;
    CK_API_END(ctx)
}

int ck_jpeg_span_bytes(int32_t* bytes)
{
    if (!bytes) return ck_fail(nullptr, CK_ERR_ARG, "bytes is NULL");
    *bytes = CK_SPAN_DEFAULT;
    return CK_OK;
}

int ck_jpeg_span_stats(ck_ctx* ctx, long long* stats)
{
    CK_API_BEGIN(ctx)
    if (!stats) return ck_fail(ctx, CK_ERR_ARG, "stats is NULL");
    for (int i = 0; i < CK_SPAN_STATS; i++) stats[i] = ctx->jpeg_span_stats[i];
    return CK_OK;
    CK_API_END(ctx)
}

// in that mode the frame a call refuses is named in the host decoder's words (ck_jpeg_span_host_wording)
static void jpeg_span_wording(const ck_ctx* ctx, const uint8_t* data, size_t len, const ck_jpeg_info& geom, std::string& why)
{
    if (ctx->jpeg_entropy != CK_JPEG_ENTROPY_DEVICE_SPANS) return;
    char msg[CK_JPEG_MSG] = {0};
    snprintf(msg, sizeof msg, "%s", why.c_str());
    ck_jpeg_span_host_wording(data, len, geom, msg);
    why = msg;
}
// the context's span size when its mode decodes inside strands, else 0 (jpeg_huff_pass)
static int jpeg_ctx_spans(const ck_ctx* ctx) { return ctx->jpeg_entropy == CK_JPEG_ENTROPY_DEVICE_SPANS ? ctx->jpeg_span_bytes : 0; }

// What a pass that began at frame f0 and came back with (rc, bad, why) means for the call.  CK_OK goes on; a failure that is
// no frame's fault (bad < 0: HIP, memory) has its message stored already; else frame f0 + bad is refused in `why`.
static int jpeg_pass_result(ck_ctx* ctx, int rc, int f0, int bad, const std::string& why)
{
    if (rc == CK_OK || bad < 0) return rc;
    return ck_fail(ctx, rc, "frame %d: %s", f0 + bad, why.c_str());
}
// The same for a pass of the decoder.  It names the frame in the host decoder's words where the mode decodes inside strands
// (jpeg_span_wording), leaves it in the context for ck_jpeg_bad_frame and at *bad_frame (nullable), and waits for the stream,
// which may still be working on the passes before.
static int jpeg_decode_pass_result(ck_ctx* ctx, int rc, int f0, int bad, std::string& why, const uint8_t* const* data, const size_t* len,
                                   const ck_jpeg_info& geom, int32_t* bad_frame)
{
    if (rc == CK_OK || bad < 0) return rc;
    const int f = f0 + bad;
    jpeg_span_wording(ctx, data[f], len[f], geom, why);
    if (bad_frame) *bad_frame = f;
    ctx->jpeg_bad_frame = f;
    (void)hipStreamSynchronize(ctx->stream);
    return jpeg_pass_result(ctx, rc, f0, bad, why);
}

int ck_jpeg_coefficients_device(ck_ctx* ctx, const uint8_t* const* data, const size_t* len, int n, const ck_jpeg_info* geom,
                                int16_t* coef, uint16_t* quant, int out_space, int32_t* bad_frame)
{
    CK_API_BEGIN(ctx)
    if (bad_frame) *bad_frame = -1;
    ctx->jpeg_bad_frame = -1;
    ctx->jpeg_uploaded = 0;
    for (long long& v : ctx->jpeg_span_stats) v = 0;
    if (!data || !len || !geom || !coef || !quant || n <= 0) return ck_fail(ctx, CK_ERR_ARG, "NULL pointer or n <= 0");
    CK_TRY(check_jpeg_geom(ctx, geom->h, geom->w, geom->sampling, geom->blocks));
    if (out_space != CK_HOST) CK_TRY(ck_coef_quant_on_16(ctx, coef, quant));
    const size_t cframe = (size_t)geom->blocks * 64 * sizeof(int16_t), qframe = 192 * sizeof(uint16_t);
    const int pass = jpeg_pass_frames_device(n, len, cframe);
    if (out_space == CK_HOST) CK_TRY(ck_ensure(ctx, ctx->in_stage, (size_t)pass * cframe));
    for (int f0 = 0; f0 < n; f0 += pass) {
        const int m = n - f0 < pass ? n - f0 : pass;
        int16_t* d_coef = out_space == CK_HOST ? (int16_t*)ctx->in_stage.p : coef + (size_t)f0 * (cframe / sizeof(int16_t));
        const uint16_t* d_quant = nullptr;
        int bad = -1;
        std::string why;
        const int rc = jpeg_huff_pass(ctx, data + f0, len + f0, m, *geom, d_coef, &d_quant, out_space == CK_HOST ? quant + (size_t)f0 * 192 : nullptr,
                                      &bad, why, jpeg_ctx_spans(ctx));
        CK_TRY(jpeg_decode_pass_result(ctx, rc, f0, bad, why, data, len, *geom, bad_frame));
        if (out_space == CK_HOST) {
            CK_TRY(ck_from_device(ctx, coef + (size_t)f0 * (cframe / sizeof(int16_t)), d_coef, (size_t)m * cframe, CK_HOST));
        } else {
            CK_TRY(ck_from_device(ctx, quant + (size_t)f0 * 192, d_quant, (size_t)m * qframe, CK_DEVICE));
        }
        CK_HIP(ctx, hipStreamSynchronize(ctx->stream));            // the next pass stages into the same blocks
    }
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_jpeg_plan(const uint8_t* const* data, const size_t* len, int n, const ck_jpeg_info* geom,
                 int64_t* strands, long long cap, long long* n_strands, int32_t* n_table_sets, int32_t* bad_frame)
{
    if (bad_frame) *bad_frame = -1;
    if (!data || !len || !geom || !n_strands || !n_table_sets || n <= 0 || cap < 0 || (cap > 0 && !strands))
        return ck_fail(nullptr, CK_ERR_ARG, "NULL pointer, n <= 0 or cap < 0");
    CK_TRY(check_jpeg_geom(nullptr, geom->h, geom->w, geom->sampling, geom->blocks));
    CK_HOST_BEGIN
    CkJpegPlan plan;
    const int rc = ck_jpeg_plan_build(data, len, n, *geom, &plan);
    if (rc != CK_OK) {
        if (bad_frame) *bad_frame = plan.frames;
        return ck_fail(nullptr, rc, "frame %d: %s", plan.frames, plan.msg);
    }
    *n_strands = (long long)plan.strands.size();
    *n_table_sets = (int32_t)plan.sets.size();
    if (*n_strands > cap) return ck_fail(nullptr, CK_ERR_CAPACITY, "%lld strands where the array holds %lld", *n_strands, cap);
    static_assert(sizeof(CkStrand) == 6 * sizeof(int64_t), "a plan row is 6 int64");
    if (*n_strands) memcpy(strands, plan.strands.data(), plan.strands.size() * sizeof(CkStrand));
    return CK_OK;
    CK_HOST_END
}

int ck_jpeg_coefficients_strands(const uint8_t* const* data, const size_t* len, int n, const ck_jpeg_info* geom,
                                 int16_t* coef, uint16_t* quant, int32_t* bad_frame)
{
    if (bad_frame) *bad_frame = -1;
    if (!data || !len || !geom || !coef || !quant || n <= 0) return ck_fail(nullptr, CK_ERR_ARG, "NULL pointer or n <= 0");
    CK_TRY(check_jpeg_geom(nullptr, geom->h, geom->w, geom->sampling, geom->blocks));
    CK_HOST_BEGIN
    int bad = -1;
    char msg[CK_JPEG_MSG] = {0};
    const int rc = ck_jpeg_strands_host(data, len, n, *geom, coef, quant, false, &bad, msg);
    if (rc != CK_OK) {
        if (bad_frame) *bad_frame = bad;
        return ck_fail(nullptr, rc, "frame %d: %s", bad, msg);
    }
    return CK_OK;
    CK_HOST_END
}

int ck_jpeg_coefficients_spans(const uint8_t* const* data, const size_t* len, int n, const ck_jpeg_info* geom, int span_bytes,
                               int16_t* coef, uint16_t* quant, int32_t* bad_frame, long long* stats)
{
    if (bad_frame) *bad_frame = -1;
    if (!data || !len || !geom || !coef || !quant || n <= 0) return ck_fail(nullptr, CK_ERR_ARG, "NULL pointer or n <= 0");
    if (span_bytes < CK_SPAN_MIN || span_bytes > CK_SPAN_MAX)
        return ck_fail(nullptr, CK_ERR_ARG, "span size %d outside %d .. %d bytes", span_bytes, CK_SPAN_MIN, CK_SPAN_MAX);
    CK_TRY(check_jpeg_geom(nullptr, geom->h, geom->w, geom->sampling, geom->blocks));
    CK_HOST_BEGIN
    int bad = -1;
    char msg[CK_JPEG_MSG] = {0};
    long long st[CK_SPAN_STATS];
    const int rc = ck_jpeg_spans_host(data, len, n, *geom, span_bytes, coef, quant, &bad, msg, st);
    if (stats) memcpy(stats, st, sizeof st);
    if (rc != CK_OK) {
        if (bad_frame) *bad_frame = bad;
        return ck_fail(nullptr, rc, "frame %d: %s", bad, msg);
    }
    return CK_OK;
    CK_HOST_END
}

// ck_jpeg_decode with the Huffman stage on the device.  Per pass: the compressed bytes up, the Huffman kernel, the
// reconstruct kernel: the coefficients stay in HBM.
static int jpeg_decode_device(ck_ctx* ctx, const uint8_t* const* data, const size_t* len, int n, const ck_jpeg_info& geom, uint8_t* d_bgr)
{
    const size_t cframe = (size_t)geom.blocks * 64 * sizeof(int16_t), oframe = (size_t)geom.h * geom.w * 3;
    const int pass = jpeg_pass_frames_device(n, len, cframe);
    CK_TRY(ck_ensure(ctx, ctx->in_stage, (size_t)pass * cframe));
    for (int f0 = 0; f0 < n; f0 += pass) {
        const int m = n - f0 < pass ? n - f0 : pass;
        const uint16_t* d_quant = nullptr;
        int bad = -1;
        std::string why;
        const int rc = jpeg_huff_pass(ctx, data + f0, len + f0, m, geom, (int16_t*)ctx->in_stage.p, &d_quant, nullptr, &bad, why, jpeg_ctx_spans(ctx));
        CK_TRY(jpeg_decode_pass_result(ctx, rc, f0, bad, why, data, len, geom, nullptr));
        CK_TRY(k_jpeg_reconstruct(ctx, (const int16_t*)ctx->in_stage.p, d_quant, m, geom.h, geom.w, geom.sampling, d_bgr + (size_t)f0 * oframe));
        if (f0 + pass < n) CK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return CK_OK;
}

// ck_jpeg_decode with the Huffman stage on the host's worker threads.  Per pass: coefficients, then quant tables, in one
// pinned block -> one upload -> the kernel.  The stream is waited for before the next pass decodes into the same block.
static int jpeg_decode_host(ck_ctx* ctx, const uint8_t* const* data, const size_t* len, int n, const ck_jpeg_info& geom, uint8_t* d_bgr)
{
    const size_t cframe = (size_t)geom.blocks * 64 * sizeof(int16_t), qframe = 192 * sizeof(uint16_t);
    const size_t oframe = (size_t)geom.h * geom.w * 3;
    const int pass = jpeg_pass_frames(n, cframe + qframe);
    CK_TRY(ck_ensure_pinned(ctx, ctx->host_pinned, (size_t)pass * (cframe + qframe)));
    for (int f0 = 0; f0 < n; f0 += pass) {
        const int m = n - f0 < pass ? n - f0 : pass;
        const size_t cbytes = (size_t)m * cframe, qbytes = (size_t)m * qframe;
        int16_t* coef = (int16_t*)ctx->host_pinned.p;
        uint16_t* quant = (uint16_t*)((uint8_t*)ctx->host_pinned.p + cbytes);
        int bad = -1;
        std::string why;
        const int rc = jpeg_entropy_batch(data + f0, len + f0, m, geom, coef, quant, &bad, why);
        CK_TRY(jpeg_decode_pass_result(ctx, rc, f0, bad, why, data, len, geom, nullptr));   // (the host mode: no rewording)
        const void* d_in;
        CK_TRY(ck_to_device(ctx, coef, cbytes + qbytes, CK_HOST, ctx->in_stage, &d_in));
        ctx->jpeg_uploaded += (long long)(cbytes + qbytes);
        CK_TRY(k_jpeg_reconstruct(ctx, (const int16_t*)d_in, (const uint16_t*)((const uint8_t*)d_in + cbytes), m, geom.h, geom.w,
                                  geom.sampling, d_bgr + (size_t)f0 * oframe));
        if (f0 + pass < n) CK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return CK_OK;
}

int ck_jpeg_decode(ck_ctx* ctx, const uint8_t* const* data, const size_t* len, int n, uint8_t* bgr, int out_space)
{
    CK_API_BEGIN(ctx)
    ctx->jpeg_bad_frame = -1;
    ctx->jpeg_uploaded = 0;
    for (long long& v : ctx->jpeg_span_stats) v = 0;
    if (!data || !len || !bgr || n <= 0) return ck_fail(ctx, CK_ERR_ARG, "NULL pointer or n <= 0");
    auto first = std::make_unique<CkJpegFrame>();
    char msg[CK_JPEG_MSG];
    const int rc0 = ck_jpeg_parse(data[0], len[0], first.get(), msg);
    if (rc0 != CK_OK) { ctx->jpeg_bad_frame = 0; return ck_fail(ctx, rc0, "frame 0: %s", msg); }
    const ck_jpeg_info geom = first->info;
    CK_TRY(check_jpeg_geom(ctx, geom.h, geom.w, geom.sampling, geom.blocks));
    OutStage<uint8_t> o;
    CK_TRY(o.open(ctx, bgr, (size_t)n * (size_t)geom.h * geom.w * 3, out_space, ctx->out_stage));
    CK_TRY((ctx->jpeg_entropy != CK_JPEG_ENTROPY_HOST ? jpeg_decode_device : jpeg_decode_host)(ctx, data, len, n, geom, o.dev));
    CK_TRY(o.deliver(ctx));
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_jpeg_uploaded_bytes(ck_ctx* ctx, long long* bytes)
{
    CK_API_BEGIN(ctx)
    if (!bytes) return ck_fail(ctx, CK_ERR_ARG, "bytes is NULL");
    *bytes = ctx->jpeg_uploaded;
    return CK_OK;
    CK_API_END(ctx)
}

int ck_jpeg_bad_frame(ck_ctx* ctx, int32_t* frame)
{
    CK_API_BEGIN(ctx)
    if (!frame) return ck_fail(ctx, CK_ERR_ARG, "frame is NULL");
    *frame = ctx->jpeg_bad_frame;
    return CK_OK;
    CK_API_END(ctx)
}

// ---- baseline JPEG encode: the forward kernel (k_jpeg_enc.hip) and the host half (ck_jpeg_enc.cpp) behind the ABI ----
int ck_jpeg_quant(int quality, uint16_t* quant)
{
    if (!quant) return ck_fail(nullptr, CK_ERR_ARG, "quant is NULL");
    ck_jpeg_enc_quant(quality, quant);
    return CK_OK;
}

int ck_jpeg_encode_bound(int h, int w, int sampling, size_t* bytes)
{
    if (!bytes) return ck_fail(nullptr, CK_ERR_ARG, "bytes is NULL");
    CK_TRY(check_jpeg_geom(nullptr, h, w, sampling, -1));
    *bytes = ck_jpeg_enc_bound(h, w, sampling);
    return CK_OK;
}

static int check_jpeg_quant(ck_ctx* ctx, const uint16_t* quant)
{
    for (int i = 0; i < 192; i++)
        if (quant[i] < 1 || quant[i] > 255) return ck_fail(ctx, CK_ERR_ARG, "quant entry %d is %d: baseline tables hold 1 .. 255", i, quant[i]);
    return CK_OK;
}

static int check_jpeg_out(ck_ctx* ctx, int h, int w, int sampling, int restart_interval, size_t stride)
{
    if (restart_interval < 0 || restart_interval > 65535) return ck_fail(ctx, CK_ERR_ARG, "restart interval %d: 0 .. 65535 MCUs", restart_interval);
    if (stride < ck_jpeg_enc_bound(h, w, sampling))
        return ck_fail(ctx, CK_ERR_ARG, "output buffer of %zu bytes per frame: smaller than the bound of %zu for a %dx%d frame", stride,
                       ck_jpeg_enc_bound(h, w, sampling), w, h);
    return CK_OK;
}

// the Huffman stage of n frames, in parallel; on failure *bad is the first frame that failed and `why` its message
static int jpeg_encode_batch(const int16_t* coef, const uint16_t* quant, int n, int h, int w, int sampling, int restart_interval,
                             uint8_t* out, size_t stride, size_t* len, int* bad, std::string& why, bool optimise = false)
{
    const size_t cframe = (size_t)ck_jpeg_blocks(h, w, sampling) * 64;
    std::vector<int> rcs((size_t)n, CK_OK);
    std::vector<std::string> msgs((size_t)n);
    ck_parallel_for(n, 16, [&](int f) {
        char msg[CK_JPEG_MSG];
        rcs[f] = (optimise ? ck_jpeg_enc_entropy_opt : ck_jpeg_enc_entropy)(coef + (size_t)f * cframe, quant, h, w, sampling, restart_interval,
                                                                            out + (size_t)f * stride, stride, len + f, msg);
        if (rcs[f] != CK_OK) msgs[f] = msg;
    });
    for (int f = 0; f < n; f++)
        if (rcs[f] != CK_OK) { *bad = f; why = msgs[f]; return rcs[f]; }
    return CK_OK;
}

int ck_jpeg_forward(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space, const uint16_t* quant, int sampling,
                    int16_t* coef, int out_space)
{
    CK_API_BEGIN(ctx)
    if (!bgr || !quant || !coef || n <= 0) return ck_fail(ctx, CK_ERR_ARG, "NULL pointer or n <= 0");
    CK_TRY(check_jpeg_geom(ctx, h, w, sampling, -1));
    CK_TRY(check_jpeg_quant(ctx, quant));
    const void *d_in, *d_quant;
    CK_TRY(ck_to_device(ctx, bgr, (size_t)n * h * w * 3, in_space, ctx->in_stage, &d_in));
    CK_TRY(ck_to_device(ctx, quant, 192 * sizeof(uint16_t), CK_HOST, ctx->in_stage2, &d_quant));
    OutStage<int16_t> o;
    CK_TRY(o.open(ctx, coef, (size_t)n * (size_t)ck_jpeg_blocks(h, w, sampling) * 64 * sizeof(int16_t), out_space, ctx->out_stage));
    CK_TRY(ck_coef_on_16(ctx, o.dev));
    CK_TRY(k_jpeg_forward(ctx, (const uint8_t*)d_in, (const uint16_t*)d_quant, n, h, w, sampling, o.dev));
    CK_TRY(o.deliver(ctx));
    return finish(ctx);           // (also: the quant tables were read from the caller's memory by the time this returns)
    CK_API_END(ctx)
}

// optimised tables count a frame's symbols in 32 bits
static int check_jpeg_opt_blocks(ck_ctx* ctx, int h, int w, int sampling)
{
    if ((long long)ck_jpeg_blocks(h, w, sampling) > (long long)CK_ENC_OPT_MAX_BLOCKS)
        return ck_fail(ctx, CK_ERR_ARG, "a %dx%d frame has %d blocks: optimised Huffman tables take 2^25", w, h, ck_jpeg_blocks(h, w, sampling));
    return CK_OK;
}

static int jpeg_entropy_encode_host(const int16_t* coef, const uint16_t* quant, int n, int h, int w, int sampling, int restart_interval,
                                    uint8_t* out, size_t stride, size_t* len, bool optimise)
{
    if (!coef || !quant || !out || !len || n <= 0) return ck_fail(nullptr, CK_ERR_ARG, "NULL pointer or n <= 0");
    CK_TRY(check_jpeg_geom(nullptr, h, w, sampling, -1));
    CK_TRY(check_jpeg_out(nullptr, h, w, sampling, restart_interval, stride));
    if (optimise) CK_TRY(check_jpeg_opt_blocks(nullptr, h, w, sampling));
    CK_HOST_BEGIN
    int bad = -1;
    std::string why;
    const int rc = jpeg_encode_batch(coef, quant, n, h, w, sampling, restart_interval, out, stride, len, &bad, why, optimise);
    if (rc != CK_OK) return ck_fail(nullptr, rc, "frame %d: %s", bad, why.c_str());
    return CK_OK;
    CK_HOST_END
}

int ck_jpeg_entropy_encode(const int16_t* coef, const uint16_t* quant, int n, int h, int w, int sampling, int restart_interval,
                           uint8_t* out, size_t stride, size_t* len)
{
    return jpeg_entropy_encode_host(coef, quant, n, h, w, sampling, restart_interval, out, stride, len, false);
}

int ck_jpeg_entropy_encode_opt(const int16_t* coef, const uint16_t* quant, int n, int h, int w, int sampling, int restart_interval,
                               uint8_t* out, size_t stride, size_t* len)
{
    return jpeg_entropy_encode_host(coef, quant, n, h, w, sampling, restart_interval, out, stride, len, true);
}

static int jpeg_entropy_encode_staged(const int16_t* coef, const uint16_t* quant, int n, int h, int w, int sampling, int restart_interval,
                                      uint8_t* out, size_t stride, size_t* len, bool optimise)
{
    if (!coef || !quant || !out || !len || n <= 0) return ck_fail(nullptr, CK_ERR_ARG, "NULL pointer or n <= 0");
    CK_TRY(check_jpeg_geom(nullptr, h, w, sampling, -1));
    CK_TRY(check_jpeg_out(nullptr, h, w, sampling, restart_interval, stride));
    if (optimise) CK_TRY(check_jpeg_opt_blocks(nullptr, h, w, sampling));
    CK_HOST_BEGIN
    int bad = -1;
    char msg[CK_JPEG_MSG] = {0};
    const int rc = (optimise ? ck_jpeg_enc_staged_opt : ck_jpeg_enc_staged)(coef, quant, n, h, w, sampling, restart_interval, out, stride, len, &bad, msg);
    if (rc != CK_OK) return ck_fail(nullptr, rc, "frame %d: %s", bad, msg);
    return CK_OK;
    CK_HOST_END
}

int ck_jpeg_entropy_encode_staged(const int16_t* coef, const uint16_t* quant, int n, int h, int w, int sampling, int restart_interval,
                                  uint8_t* out, size_t stride, size_t* len)
{
    return jpeg_entropy_encode_staged(coef, quant, n, h, w, sampling, restart_interval, out, stride, len, false);
}

int ck_jpeg_entropy_encode_opt_staged(const int16_t* coef, const uint16_t* quant, int n, int h, int w, int sampling, int restart_interval,
                                      uint8_t* out, size_t stride, size_t* len)
{
    return jpeg_entropy_encode_staged(coef, quant, n, h, w, sampling, restart_interval, out, stride, len, true);
}

int ck_jpeg_histogram(const int16_t* coef, int n, int h, int w, int sampling, int restart_interval, uint32_t* counts)
{
    if (!coef || !counts || n <= 0) return ck_fail(nullptr, CK_ERR_ARG, "NULL pointer or n <= 0");
    CK_TRY(check_jpeg_geom(nullptr, h, w, sampling, -1));
    CK_TRY(check_jpeg_opt_blocks(nullptr, h, w, sampling));
    const size_t cframe = (size_t)ck_jpeg_blocks(h, w, sampling) * 64;
    for (int f = 0; f < n; f++) {
        char msg[CK_JPEG_MSG];
        const int rc = ck_jpeg_enc_histogram(coef + (size_t)f * cframe, h, w, sampling, restart_interval, counts + (size_t)f * 4 * 256, msg);
        if (rc != CK_OK) return ck_fail(nullptr, rc, "frame %d: %s", f, msg);
    }
    return CK_OK;
}

int ck_jpeg_optimal_table(const uint32_t* counts, uint8_t* bits, uint8_t* vals, int32_t* count)
{
    if (!counts || !bits || !vals || !count) return ck_fail(nullptr, CK_ERR_ARG, "NULL pointer");
    CK_HOST_BEGIN
    ck_jpeg_enc_optimal_table(counts, bits, vals, count);
    return CK_OK;
    CK_HOST_END
}

int ck_jpeg_set_encode_tables(ck_ctx* ctx, int mode)
{
    CK_API_BEGIN(ctx)
    if (mode != CK_JPEG_TABLES_STANDARD && mode != CK_JPEG_TABLES_OPTIMISED) return ck_fail(ctx, CK_ERR_ARG, "unknown JPEG table mode %d", mode);
    ctx->jpeg_enc_tables = mode;
    return CK_OK;
    CK_API_END(ctx)
}

int ck_jpeg_encode_histograms(ck_ctx* ctx, int n, uint32_t* counts)
{
    CK_API_BEGIN(ctx)
    if (!counts) return ck_fail(ctx, CK_ERR_ARG, "counts is NULL");
    if (n <= 0 || n != ctx->jenc_freq_frames) return ck_fail(ctx, CK_ERR_STATE, "the last pass counted %d frames, not %d", ctx->jenc_freq_frames, n);
    CK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    CK_HIP(ctx, hipMemcpy(counts, (const uint8_t*)ctx->jenc_work.p + ctx->jenc_freq_at, (size_t)n * 4 * 256 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return CK_OK;
    CK_API_END(ctx)
}

int ck_jpeg_enc_tiles(int32_t* blocks_per_tile, int32_t* bytes_per_tile)
{
    if (!blocks_per_tile || !bytes_per_tile) return ck_fail(nullptr, CK_ERR_ARG, "NULL pointer");
    *blocks_per_tile = CK_ENC_TILE_BLOCKS;
    *bytes_per_tile = CK_ENC_TILE_BYTES;
    return CK_OK;
}

int ck_jpeg_set_encode_entropy(ck_ctx* ctx, int mode)
{
    CK_API_BEGIN(ctx)
    if (mode != CK_JPEG_ENTROPY_HOST && mode != CK_JPEG_ENTROPY_DEVICE) return ck_fail(ctx, CK_ERR_ARG, "unknown JPEG entropy mode %d", mode);
    ctx->jpeg_enc_entropy = mode;
    return CK_OK;
    CK_API_END(ctx)
}

int ck_jpeg_downloaded_bytes(ck_ctx* ctx, long long* bytes)
{
    CK_API_BEGIN(ctx)
    if (!bytes) return ck_fail(ctx, CK_ERR_ARG, "bytes is NULL");
    *bytes = ctx->jpeg_downloaded;
    return CK_OK;
    CK_API_END(ctx)
}

// The Huffman stage of m frames on the GPU (CK_JPEG_ENTROPY_DEVICE), one pass over coefficients that lie in HBM: size and
// scan -> 16 bytes down (the lowest block that cannot be coded, the bytes of the bit buffer) -> put, FF counts, lengths ->
// 8 bytes per frame down -> stuff into the packed buffer -> the streams down in one copy into the pinned block, scattered
// to out + f * stride from there.  Returns with the stream idle.  On a refusal *bad is the lowest frame that has one and
// `why` what the host coder says of it; a failure that is no frame's fault leaves *bad at -1, its message in the context.
// With `optimise` the counters, tables, DHT segments and headers of the frames lie in the work block as well, the header in
// front of and behind the DHT segments goes up with the constants, and nothing more comes down.
static int jpeg_enc_huff_pass(ck_ctx* ctx, const int16_t* d_coef, const uint16_t* quant, int m, int h, int w, int sampling,
                              int restart_interval, uint8_t* out, size_t stride, size_t* len, int* bad, std::string& why, bool optimise)
{
    const CkEncGeom g = ck_enc_geom(h, w, sampling, restart_interval);
    const CkEncLayout L = ck_enc_layout(g, m, optimise);
    const size_t consts_std = L.consts_std, consts_bytes = L.consts_bytes;
    CK_TRY(ck_ensure(ctx, ctx->jenc_work, L.total));
    uint8_t* wp = (uint8_t*)ctx->jenc_work.p;
    CkEncWork wk;
    wk.head = (uint64_t*)(wp + L.head); wk.tile_off = (uint64_t*)(wp + L.tile_off); wk.seg_bits = (uint64_t*)(wp + L.seg_bits);
    wk.seg_u0 = (uint64_t*)(wp + L.seg_u0); wk.frame_u0 = (uint64_t*)(wp + L.frame_u0); wk.len = (uint64_t*)(wp + L.len);
    wk.out_off = (uint64_t*)(wp + L.out_off); wk.bits = (uint32_t*)(wp + L.bits); wk.tile_bits = (uint32_t*)(wp + L.tile_bits);
    wk.consts = wp + L.consts;
    ctx->jenc_freq_at = L.freq;
    ctx->jenc_freq_frames = optimise ? m : 0;
    if (optimise) {
        wk.freq = (uint32_t*)(wp + L.freq); wk.tables = wp + L.tables; wk.dht = wp + L.dht; wk.dht_len = (uint32_t*)(wp + L.dht_len);
        wk.headers = wp + L.headers; wk.hlen = (uint32_t*)(wp + L.hlen);
        wk.pre = wk.consts + consts_std; wk.post = wk.pre + CK_ENC_HEADER_SLOT;
    }
    // pinned: the constants going up, the size words coming down
    CK_TRY(ck_ensure_pinned(ctx, ctx->host_pinned2, L.pin_total));
    uint8_t* hp = (uint8_t*)ctx->host_pinned2.p;
    memcpy(hp, &ck_jpeg_enc_tables(), sizeof(CkEncTables));
    memcpy(hp + sizeof(CkEncTables), ck_jpeg_enc_zigzag(), 64);
    memset(hp + sizeof(CkEncTables) + 64, 0, CK_JPEG_ENC_HEADER_BOUND);
    const uint32_t hl = (uint32_t)ck_jpeg_enc_headers(quant, h, w, sampling, restart_interval, hp + sizeof(CkEncTables) + 64);
    if (optimise) {
        memset(hp + consts_std, 0, (size_t)CK_ENC_HEADER_SLOT + 64);
        ck_jpeg_enc_header_parts(quant, h, w, sampling, restart_interval, hp + consts_std, &wk.pre_len, hp + consts_std + CK_ENC_HEADER_SLOT, &wk.post_len);
    }
    CK_HIP(ctx, hipMemcpyAsync(wp + L.consts, hp, consts_bytes, hipMemcpyHostToDevice, ctx->stream));
    uint64_t* words = (uint64_t*)(hp + L.pin_words);

    CK_TRY(k_jpeg_enc_measure(ctx, d_coef, m, g, wk));
    CK_HIP(ctx, hipMemcpyAsync(words, wk.head, 16, hipMemcpyDeviceToHost, ctx->stream));
    CK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->jpeg_downloaded += 16;
    if (words[0] != ~(uint64_t)0) {
        const uint64_t f = words[0] >> 32, b = words[0] & 0xffffffffu;
        if (f >= (uint64_t)m || b >= (uint64_t)g.blocks) return ck_fail(ctx, CK_ERR_STATE, "the size kernel names block %llu of frame %llu", (unsigned long long)b, (unsigned long long)f);
        CK_HIP(ctx, hipMemcpyAsync(words, wk.bits + f * (uint64_t)g.blocks + b, 4, hipMemcpyDeviceToHost, ctx->stream));
        CK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        char msg[CK_JPEG_MSG];
        ck_jpeg_enc_status_message(*(const uint32_t*)words, (long long)(b / (uint64_t)g.mcu_blocks), msg);
        *bad = (int)f;
        why = msg;
        return CK_ERR_ARG;
    }
    const uint64_t total_u = words[1];
    const size_t byte_tiles = (size_t)(total_u / CK_ENC_TILE_BYTES);
    if (!total_u || total_u % CK_ENC_TILE_BYTES) return ck_fail(ctx, CK_ERR_STATE, "a bit buffer of %llu bytes", (unsigned long long)total_u);
    CK_TRY(ck_ensure(ctx, ctx->jenc_bits, (size_t)total_u + byte_tiles * 8));
    uint32_t* d_buf = (uint32_t*)ctx->jenc_bits.p;
    uint32_t* d_ff_cnt = (uint32_t*)((uint8_t*)ctx->jenc_bits.p + total_u);
    uint32_t* d_ff_off = d_ff_cnt + byte_tiles;
    CK_TRY(k_jpeg_enc_put(ctx, d_coef, m, g, wk, d_buf, total_u, d_ff_cnt, d_ff_off, hl));
    CK_HIP(ctx, hipMemcpyAsync(words, wk.len, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream));
    CK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->jpeg_downloaded += (long long)m * 8;
    CkCarve pack;                                                  // the streams one behind the other, each on 16 bytes (out_off)
    std::vector<size_t> off((size_t)m);
    for (int f = 0; f < m; f++) {
        if (words[f] > stride) return ck_fail(ctx, CK_ERR_STATE, "frame %d: a stream of %llu bytes, above the bound", f, (unsigned long long)words[f]);
        len[f] = (size_t)words[f];
        off[f] = pack.take(len[f]);
    }
    const size_t total = pack.size();
    CK_TRY(ck_ensure(ctx, ctx->jenc_pack, total));
    CK_TRY(k_jpeg_enc_stuff(ctx, m, g, wk, d_buf, total_u, d_ff_off, hl, (uint8_t*)ctx->jenc_pack.p, total));
    CK_TRY(ck_ensure_pinned(ctx, ctx->host_pinned, total));
    CK_HIP(ctx, hipMemcpyAsync(ctx->host_pinned.p, ctx->jenc_pack.p, total, hipMemcpyDeviceToHost, ctx->stream));
    CK_TRY(finish(ctx));
    ctx->jpeg_downloaded += (long long)total;
    for (int f = 0; f < m; f++) memcpy(out + (size_t)f * stride, (const uint8_t*)ctx->host_pinned.p + off[f], len[f]);
    return CK_OK;
}

static int jpeg_entropy_encode_device(ck_ctx* ctx, const int16_t* coef, int in_space, const uint16_t* quant, int n, int h, int w,
                                      int sampling, int restart_interval, uint8_t* out, size_t stride, size_t* len, bool optimise)
{
    CK_API_BEGIN(ctx)
    ctx->jpeg_downloaded = 0;
    if (!coef || !quant || !out || !len || n <= 0) return ck_fail(ctx, CK_ERR_ARG, "NULL pointer or n <= 0");
    if (in_space != CK_HOST && in_space != CK_DEVICE) return ck_fail(ctx, CK_ERR_ARG, "bad memory space %d", in_space);
    CK_TRY(check_jpeg_geom(ctx, h, w, sampling, -1));
    CK_TRY(check_jpeg_out(ctx, h, w, sampling, restart_interval, stride));
    if (optimise) CK_TRY(check_jpeg_opt_blocks(ctx, h, w, sampling));
    if (in_space == CK_DEVICE) CK_TRY(ck_coef_on_16(ctx, coef));
    for (int f = 0; f < n; f++) len[f] = 0;
    char msg[CK_JPEG_MSG];
    if (ck_jpeg_enc_check(quant, h, w, sampling, restart_interval, msg) != CK_OK) return ck_fail(ctx, CK_ERR_ARG, "frame 0: %s", msg);
    const size_t cframe = (size_t)ck_jpeg_blocks(h, w, sampling) * 64 * sizeof(int16_t);
    const int pass = jpeg_enc_pass_frames_device(n, cframe);
    for (int f0 = 0; f0 < n; f0 += pass) {
        const int m = n - f0 < pass ? n - f0 : pass;
        const void* d_coef;
        CK_TRY(ck_to_device(ctx, coef + (size_t)f0 * (cframe / sizeof(int16_t)), (size_t)m * cframe, in_space, ctx->in_stage, &d_coef));
        int bad = -1;
        std::string why;
        const int rc = jpeg_enc_huff_pass(ctx, (const int16_t*)d_coef, quant, m, h, w, sampling, restart_interval, out + (size_t)f0 * stride,
                                          stride, len + f0, &bad, why, optimise);
        CK_TRY(jpeg_pass_result(ctx, rc, f0, bad, why));
    }
    return CK_OK;
    CK_API_END(ctx)
}

int ck_jpeg_entropy_encode_device(ck_ctx* ctx, const int16_t* coef, int in_space, const uint16_t* quant, int n, int h, int w,
                                  int sampling, int restart_interval, uint8_t* out, size_t stride, size_t* len)
{
    return jpeg_entropy_encode_device(ctx, coef, in_space, quant, n, h, w, sampling, restart_interval, out, stride, len, false);
}

int ck_jpeg_entropy_encode_opt_device(ck_ctx* ctx, const int16_t* coef, int in_space, const uint16_t* quant, int n, int h, int w,
                                      int sampling, int restart_interval, uint8_t* out, size_t stride, size_t* len)
{
    return jpeg_entropy_encode_device(ctx, coef, in_space, quant, n, h, w, sampling, restart_interval, out, stride, len, true);
}

int ck_jpeg_encode(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space, int quality, int sampling,
                   int restart_interval, uint8_t* out, size_t stride, size_t* len)
{
    CK_API_BEGIN(ctx)
    if (!bgr || !out || !len || n <= 0) return ck_fail(ctx, CK_ERR_ARG, "NULL pointer or n <= 0");
    CK_TRY(check_jpeg_geom(ctx, h, w, sampling, -1));
    CK_TRY(check_jpeg_out(ctx, h, w, sampling, restart_interval, stride));
    const bool optimise = ctx->jpeg_enc_tables == CK_JPEG_TABLES_OPTIMISED;
    if (optimise) CK_TRY(check_jpeg_opt_blocks(ctx, h, w, sampling));
    uint16_t quant[192];
    ck_jpeg_enc_quant(quality, quant);
    const size_t iframe = (size_t)h * w * 3, cframe = (size_t)ck_jpeg_blocks(h, w, sampling) * 64 * sizeof(int16_t);
    ctx->jpeg_downloaded = 0;
    if (ctx->jpeg_enc_entropy == CK_JPEG_ENTROPY_DEVICE) {
        // per pass: frames up (when they are the host's) -> the forward kernel -> the entropy kernels: the coefficients stay
        // in HBM, the streams come down
        const int pass = jpeg_enc_pass_frames_device(n, cframe);
        CK_TRY(ck_ensure_pinned(ctx, ctx->host_pinned2, sizeof quant));
        CK_TRY(ck_ensure(ctx, ctx->out_stage, (size_t)pass * cframe));
        memcpy(ctx->host_pinned2.p, quant, sizeof quant);
        const void* d_quant;
        CK_TRY(ck_to_device(ctx, ctx->host_pinned2.p, sizeof quant, CK_HOST, ctx->in_stage2, &d_quant));
        CK_HIP(ctx, hipStreamSynchronize(ctx->stream));          // (the pass stages its own words in that pinned block)
        for (int f0 = 0; f0 < n; f0 += pass) {
            const int m = n - f0 < pass ? n - f0 : pass;
            const void* d_in;
            CK_TRY(ck_to_device(ctx, bgr + (size_t)f0 * iframe, (size_t)m * iframe, in_space, ctx->in_stage, &d_in));
            CK_TRY(k_jpeg_forward(ctx, (const uint8_t*)d_in, (const uint16_t*)d_quant, m, h, w, sampling, (int16_t*)ctx->out_stage.p));
            int bad = -1;
            std::string why;
            const int rc = jpeg_enc_huff_pass(ctx, (const int16_t*)ctx->out_stage.p, quant, m, h, w, sampling, restart_interval,
                                              out + (size_t)f0 * stride, stride, len + f0, &bad, why, optimise);
            CK_TRY(jpeg_pass_result(ctx, rc, f0, bad, why));
        }
        return CK_OK;
    }
    const int pass = jpeg_pass_frames(n, cframe);
    // per pass: frames up (when they are the host's) -> the kernel -> the coefficients down in one copy into the pinned
    // block -> the Huffman coder on the worker threads.  The stream is idle while they code, as in ck_jpeg_decode.
    // The tables go up from the tail of the pinned block, not from this frame: the copy may outlive an early return.
    CK_TRY(ck_ensure_pinned(ctx, ctx->host_pinned, (size_t)pass * cframe + sizeof quant));
    CK_TRY(ck_ensure(ctx, ctx->out_stage, (size_t)pass * cframe));
    void* pinned_quant = (uint8_t*)ctx->host_pinned.p + (size_t)pass * cframe;
    memcpy(pinned_quant, quant, sizeof quant);
    const void* d_quant;
    CK_TRY(ck_to_device(ctx, pinned_quant, sizeof quant, CK_HOST, ctx->in_stage2, &d_quant));
    for (int f0 = 0; f0 < n; f0 += pass) {
        const int m = n - f0 < pass ? n - f0 : pass;
        const void* d_in;
        CK_TRY(ck_to_device(ctx, bgr + (size_t)f0 * iframe, (size_t)m * iframe, in_space, ctx->in_stage, &d_in));
        CK_TRY(k_jpeg_forward(ctx, (const uint8_t*)d_in, (const uint16_t*)d_quant, m, h, w, sampling, (int16_t*)ctx->out_stage.p));
        CK_TRY(ck_from_device(ctx, ctx->host_pinned.p, ctx->out_stage.p, (size_t)m * cframe, CK_HOST));
        CK_TRY(finish(ctx));
        ctx->jpeg_downloaded += (long long)((size_t)m * cframe);
        int bad = -1;
        std::string why;
        const int rc = jpeg_encode_batch((const int16_t*)ctx->host_pinned.p, quant, m, h, w, sampling, restart_interval,
                                         out + (size_t)f0 * stride, stride, len + f0, &bad, why, optimise);
        CK_TRY(jpeg_pass_result(ctx, rc, f0, bad, why));
    }
    return CK_OK;
    CK_API_END(ctx)
}

}  // extern "C"
