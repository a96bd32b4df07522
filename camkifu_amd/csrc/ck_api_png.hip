// ck_api_png.hip -- the PNG entry points of libck_hip.so (see include/camkifu_amd.h): reading (inflate on the host or on the
// device, unfilter on the device) and writing.  Host-side glue only, as ck_api.hip; where the parts of a staged block lie
// and how many frames go into a pass is ck_stage_layout.h's.
#include <vector>

#include "ck_common.h"
#include "ck_api_util.h"
#include "ck_stage_layout.h"
#include "ck_png.h"
#include "ck_png_inflate_stage.h"

extern "C" {

// ---- PNG: the host half (ck_png.cpp) behind the ABI, and the two calls that reach the GPU (k_png.hip) ----
static void png_info_of(const CkPngHead& hd, ck_png_info* info)
{
    info->h = hd.h; info->w = hd.w; info->color_type = hd.color_type; info->bit_depth = hd.bit_depth;
    info->palette_entries = hd.palette_n; info->reserved = 0; info->rowbytes = hd.rowbytes;
}

static int png_host_call(const uint8_t* data, size_t len, ck_png_info* info, bool deep)
{
    if (!data || !info) return ck_fail(nullptr, CK_ERR_ARG, "NULL pointer");
    CK_HOST_BEGIN
    CkPngHead hd;
    char msg[CK_PNG_MSG];
    int rc = ck_png_walk(data, len, &hd, msg);
    if (rc == CK_OK && deep) {
        std::vector<uint8_t> rows(hd.inflated());
        rc = ck_png_rows(hd, rows.data(), msg);
    }
    if (rc != CK_OK) return ck_fail(nullptr, rc, "%s", msg);
    png_info_of(hd, info);
    return CK_OK;
    CK_HOST_END
}

int ck_png_header(const uint8_t* data, size_t len, ck_png_info* info) { return png_host_call(data, len, info, false); }
int ck_png_probe(const uint8_t* data, size_t len, ck_png_info* info) { return png_host_call(data, len, info, true); }

int ck_png_inflate(const uint8_t* data, size_t len, uint8_t* out, size_t cap, size_t* total)
{
    if (!data || !total || (!out && cap)) return ck_fail(nullptr, CK_ERR_ARG, "NULL pointer");
    CK_HOST_BEGIN
    char msg[CK_PNG_MSG];
    const int rc = ck_png_unzip(data, len, out, cap, total, msg);
    return rc == CK_OK ? CK_OK : ck_fail(nullptr, rc, "%s", msg);
    CK_HOST_END
}

static int check_png_size(ck_ctx* ctx, int h, int w)
{
    if (h <= 0 || w <= 0 || h > CK_PNG_MAX_SIDE || w > CK_PNG_MAX_SIDE || (long long)h * w > CK_PNG_MAX_PIXELS)
        return ck_fail(ctx, CK_ERR_ARG, "bad PNG frame size %dx%d: 1 .. %d a side and up to 2^28 pixels", w, h, CK_PNG_MAX_SIDE);
    return CK_OK;
}

int ck_png_tiles(int32_t* band_rows, int32_t* tile_bytes, int32_t* chunk_bytes, int32_t* group_rows)
{
    if (!band_rows || !tile_bytes || !chunk_bytes || !group_rows) return ck_fail(nullptr, CK_ERR_ARG, "NULL pointer");
    *band_rows = CK_PNG_BAND_ROWS; *tile_bytes = CK_PNG_TILE_BYTES; *chunk_bytes = CK_PNG_CHUNK; *group_rows = CK_PNG_GROUP_ROWS;
    return CK_OK;
}

int ck_png_inflate_geometry(int32_t* window_bits, int32_t* flush_bytes)
{
    if (!window_bits || !flush_bytes) return ck_fail(nullptr, CK_ERR_ARG, "NULL pointer");
    *window_bits = CK_INF_WINDOW; *flush_bytes = CK_INF_FLUSH;
    return CK_OK;
}

int ck_png_inflate_staged(const uint8_t* data, size_t len, uint8_t* out, size_t cap, size_t* total, int h, long long rowbytes,
                          int32_t* cause, long long* produced)
{
    if (!data || !total || (!out && cap)) return ck_fail(nullptr, CK_ERR_ARG, "NULL pointer");
    if (h < 0 || rowbytes < 0 || (h > 0 && rowbytes == 0)) return ck_fail(nullptr, CK_ERR_ARG, "bad rows: %d of 1 + %lld bytes", h, rowbytes);
    CK_HOST_BEGIN
    char msg[CK_PNG_MSG];
    CkInfRecord rec;
    const int rc = ck_png_unzip_staged_rows(data, len, out, cap, total, &rec, msg, h, rowbytes);
    if (cause) *cause = rec.cause;
    if (produced) *produced = rec.produced;
    return rc == CK_OK ? CK_OK : ck_fail(nullptr, rc, "%s", msg);
    CK_HOST_END
}

int ck_png_set_inflate(ck_ctx* ctx, int mode)
{
    CK_API_BEGIN(ctx)
    if (mode != CK_PNG_INFLATE_HOST && mode != CK_PNG_INFLATE_DEVICE) return ck_fail(ctx, CK_ERR_ARG, "unknown PNG inflate mode %d", mode);
    ctx->png_inflate = mode;
    return CK_OK;
    CK_API_END(ctx)
}

int ck_png_uploaded_bytes(ck_ctx* ctx, long long* bytes)
{
    CK_API_BEGIN(ctx)
    if (!bytes) return ck_fail(ctx, CK_ERR_ARG, "bytes is NULL");
    *bytes = ctx->png_uploaded;
    return CK_OK;
    CK_API_END(ctx)
}

int ck_png_inflate_stats(ck_ctx* ctx, long long* stats)
{
    CK_API_BEGIN(ctx)
    if (!stats) return ck_fail(ctx, CK_ERR_ARG, "stats is NULL");
    for (int k = 0; k < 4; k++) stats[k] = ctx->png_inf_stats[k];
    return CK_OK;
    CK_API_END(ctx)
}

static void png_inflate_count(ck_ctx* ctx, const std::vector<CkInfRecord>& recs)
{
    for (const CkInfRecord& r : recs) {
        ctx->png_inf_stats[0] += 1; ctx->png_inf_stats[1] += r.steps; ctx->png_inf_stats[2] += r.tokens; ctx->png_inf_stats[3] += r.produced;
    }
}

int ck_png_inflate_device(ck_ctx* ctx, const uint8_t* const* z, const size_t* zlen, int n, uint8_t* out, const size_t* cap, size_t stride,
                          size_t* total, int32_t* cause, long long* produced)
{
    CK_API_BEGIN(ctx)
    if (!z || !zlen || !out || !cap || !total || !cause || !produced || n <= 0) return ck_fail(ctx, CK_ERR_ARG, "NULL pointer or n <= 0");
    size_t most = 0;
    for (int f = 0; f < n; f++) {
        if (!z[f] && zlen[f]) return ck_fail(ctx, CK_ERR_ARG, "stream %d is NULL", f);
        if (cap[f] > stride) return ck_fail(ctx, CK_ERR_ARG, "stream %d: room for %zu bytes, above the stride of %zu", f, cap[f], stride);
        most = cap[f] > most ? cap[f] : most;
    }
    const CkInflateLayout L = ck_inflate_layout(zlen, n, most);
    const size_t dstride = L.dstride;
    // pinned: jobs and streams going up, then the output of every stream coming down
    CK_TRY(ck_ensure_pinned(ctx, ctx->host_pinned, L.rec > (size_t)n * dstride ? L.rec : (size_t)n * dstride));
    CK_TRY(ck_ensure(ctx, ctx->png_inf, L.total));
    uint8_t* hp = (uint8_t*)ctx->host_pinned.p;
    CkInfJob* jobs = (CkInfJob*)(hp + L.jobs);
    for (int f = 0; f < n; f++) {
        jobs[f].z_off = (int64_t)L.z[f]; jobs[f].zlen = (int64_t)zlen[f]; jobs[f].out_off = (int64_t)(L.out + (size_t)f * dstride);
        jobs[f].cap = (int64_t)cap[f]; jobs[f].need = 0; jobs[f].pitch = 0;
        if (zlen[f]) memcpy(hp + L.z[f], z[f], zlen[f]);
    }
    uint8_t* dev = (uint8_t*)ctx->png_inf.p;
    CK_HIP(ctx, hipMemcpyAsync(dev, hp, L.rec, hipMemcpyHostToDevice, ctx->stream));
    CK_TRY(k_png_inflate(ctx, dev, dev, (const CkInfJob*)(dev + L.jobs), (CkInfRecord*)(dev + L.rec), n));
    std::vector<CkInfRecord> recs((size_t)n);
    CK_HIP(ctx, hipMemcpyAsync(recs.data(), dev + L.rec, (size_t)n * sizeof(CkInfRecord), hipMemcpyDeviceToHost, ctx->stream));
    if (dstride) CK_HIP(ctx, hipMemcpyAsync(hp, dev + L.out, (size_t)n * dstride, hipMemcpyDeviceToHost, ctx->stream));
    CK_TRY(finish(ctx));
    for (int k = 0; k < 4; k++) ctx->png_inf_stats[k] = 0;
    png_inflate_count(ctx, recs);
    for (int f = 0; f < n; f++) {
        const CkInfRecord& r = recs[(size_t)f];
        cause[f] = r.cause; produced[f] = r.produced; total[f] = r.cause == CK_INF_OK ? (size_t)r.produced : 0;
        const size_t have = r.cause != CK_INF_OK ? 0 : (size_t)r.produced < cap[f] ? (size_t)r.produced : cap[f];   // (a refused stream's pending bytes never left the ring)
        if (have) memcpy(out + (size_t)f * stride, hp + (size_t)f * dstride, have);
    }
    return CK_OK;
    CK_API_END(ctx)
}

// a pass of ck_png_decode takes frames while their rows stay within 256 MB (one frame at least), a pass of ck_png_encode
// frames whose filtered rows stay within 1 GiB: what the pinned block and its device twin hold.  There is no knob.
static const size_t PNG_DECODE_PASS_BYTES = (size_t)256 << 20, PNG_ENCODE_PASS_BYTES = (size_t)1 << 30;

// the descriptor and the palette of each of the m frames of a pass, into the block at hp
static void png_fill_descs(uint8_t* hp, const CkPngDecodeLayout& L, const CkPngHead* heads, int m)
{
    CkPngDesc* desc = (CkPngDesc*)(hp + L.desc);
    for (int i = 0; i < m; i++) {
        const CkPngHead& hd = heads[i];
        desc[i].off = (int64_t)L.rows[i]; desc[i].rowbytes = hd.rowbytes; desc[i].color_type = hd.color_type; desc[i].depth = hd.bit_depth;
        desc[i].bpp = hd.bpp; desc[i].palette_n = hd.palette_n;
        memcpy(hp + L.pal + (size_t)i * 768, hd.palette, 768);
    }
}

int ck_png_decode(ck_ctx* ctx, const uint8_t* const* data, const size_t* len, int n, uint8_t* bgr, int out_space, int32_t* bad_frame)
{
    if (bad_frame) *bad_frame = -1;
    CK_API_BEGIN(ctx)
    if (!data || !len || !bgr || n <= 0) return ck_fail(ctx, CK_ERR_ARG, "NULL pointer or n <= 0");
    std::vector<CkPngHead> heads((size_t)n);
    std::vector<int> rcs((size_t)n, CK_OK);
    std::vector<std::string> msgs((size_t)n);
    auto refused = [&](int f0) {
        for (size_t f = 0; f < rcs.size(); f++)
            if (rcs[f] != CK_OK) {
                if (bad_frame) *bad_frame = f0 + (int)f;
                (void)hipStreamSynchronize(ctx->stream);
                return ck_fail(ctx, rcs[f], "frame %d: %s", f0 + (int)f, msgs[f].c_str());
            }
        return (int)CK_OK;
    };
    ck_parallel_for(n, 16, [&](int f) {
        char msg[CK_PNG_MSG];
        rcs[f] = ck_png_walk(data[f], len[f], &heads[f], msg);          // (a NULL stream is refused there)
        if (rcs[f] != CK_OK) msgs[f] = msg;
    });
    CK_TRY(refused(0));
    const int h = heads[0].h, w = heads[0].w;
    for (int f = 1; f < n; f++)
        if (heads[f].h != h || heads[f].w != w) {
            if (bad_frame) *bad_frame = f;
            return ck_fail(ctx, CK_ERR_DATA, "frame %d: %dx%d where the batch is %dx%d", f, heads[f].w, heads[f].h, w, h);
        }
    const size_t oframe = (size_t)h * w * 3;
    OutStage<uint8_t> o;
    CK_TRY(o.open(ctx, bgr, (size_t)n * oframe, out_space, ctx->out_stage));
    std::vector<size_t> inflated((size_t)n), zlen((size_t)n);
    for (int f = 0; f < n; f++) { inflated[f] = heads[f].inflated(); zlen[f] = heads[f].zlen; }
    ctx->png_uploaded = 0;
    if (ctx->png_inflate == CK_PNG_INFLATE_DEVICE) {
        // per pass: descriptors, palettes, jobs and the zlib streams in one pinned block -> one upload -> the inflate kernel
        // writes the rows behind them -> the verdict records come down -> the unfilter kernel, unless a frame was refused
        for (int k = 0; k < 4; k++) ctx->png_inf_stats[k] = 0;
        for (int f0 = 0; f0 < n;) {
            const int m = ck_png_pass_take(inflated.data(), zlen.data(), f0, n, PNG_DECODE_PASS_BYTES, nullptr, nullptr);
            const CkPngDecodeLayout L = ck_png_decode_layout(inflated.data() + f0, zlen.data() + f0, m);
            CK_TRY(ck_ensure_pinned(ctx, ctx->host_pinned, L.upload));  // (the records and the rows exist on the device only)
            CK_TRY(ck_ensure(ctx, ctx->in_stage, L.total));
            uint8_t* hp = (uint8_t*)ctx->host_pinned.p;
            png_fill_descs(hp, L, &heads[f0], m);
            CkInfJob* jobs = (CkInfJob*)(hp + L.jobs);
            for (int i = 0; i < m; i++) {
                const CkPngHead& hd = heads[f0 + i];
                jobs[i].z_off = (int64_t)L.z[i]; jobs[i].zlen = (int64_t)hd.zlen; jobs[i].out_off = (int64_t)L.rows[i];
                jobs[i].cap = jobs[i].need = (int64_t)hd.inflated(); jobs[i].pitch = 1 + hd.rowbytes;
                if (hd.zlen) memcpy(hp + L.z[i], hd.z, hd.zlen);
            }
            uint8_t* dev = (uint8_t*)ctx->in_stage.p;
            CK_HIP(ctx, hipMemcpyAsync(dev, hp, L.upload, hipMemcpyHostToDevice, ctx->stream));
            ctx->png_uploaded += (long long)L.upload;
            CK_TRY(k_png_inflate(ctx, dev, dev, (const CkInfJob*)(dev + L.jobs), (CkInfRecord*)(dev + L.rec), m));
            std::vector<CkInfRecord> recs((size_t)m);
            CK_HIP(ctx, hipMemcpyAsync(recs.data(), dev + L.rec, (size_t)m * sizeof(CkInfRecord), hipMemcpyDeviceToHost, ctx->stream));
            CK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            png_inflate_count(ctx, recs);
            for (int i = 0; i < m; i++)
                if (recs[(size_t)i].cause != CK_INF_OK) {
                    char msg[CK_PNG_MSG];
                    ck_png_inflate_message(recs[(size_t)i], heads[f0 + i].h, (long long)heads[f0 + i].rowbytes, msg);
                    if (bad_frame) *bad_frame = f0 + i;
                    return ck_fail(ctx, CK_ERR_DATA, "frame %d: %s", f0 + i, msg);
                }
            CK_TRY(k_png_unfilter(ctx, dev, (const CkPngDesc*)(dev + L.desc), dev + L.pal, m, h, w, o.dev + (size_t)f0 * oframe));
            f0 += m;
            if (f0 < n) CK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the next pass uploads into the same block
        }
        CK_TRY(o.deliver(ctx));
        return finish(ctx);
    }
    // per pass: descriptors, palettes and the inflated rows of its frames in one pinned block -> one upload -> the kernel
    for (int f0 = 0; f0 < n;) {
        const int m = ck_png_pass_take(inflated.data(), nullptr, f0, n, PNG_DECODE_PASS_BYTES, nullptr, nullptr);
        const CkPngDecodeLayout L = ck_png_decode_layout(inflated.data() + f0, nullptr, m);
        CK_TRY(ck_ensure_pinned(ctx, ctx->host_pinned, L.total));
        uint8_t* hp = (uint8_t*)ctx->host_pinned.p;
        png_fill_descs(hp, L, &heads[f0], m);
        rcs.assign((size_t)m, CK_OK);
        msgs.assign((size_t)m, std::string());
        ck_parallel_for(m, 16, [&](int i) {
            char msg[CK_PNG_MSG];
            rcs[i] = ck_png_rows(heads[f0 + i], hp + L.rows[i], msg);
            if (rcs[i] != CK_OK) msgs[i] = msg;
        });
        CK_TRY(refused(f0));
        const void* d_in;
        CK_TRY(ck_to_device(ctx, hp, L.upload, CK_HOST, ctx->in_stage, &d_in));
        ctx->png_uploaded += (long long)L.upload;
        const uint8_t* d = (const uint8_t*)d_in;
        CK_TRY(k_png_unfilter(ctx, (uint8_t*)ctx->in_stage.p, (const CkPngDesc*)(d + L.desc), d + L.pal, m, h, w, o.dev + (size_t)f0 * oframe));
        f0 += m;
        if (f0 < n) CK_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the next pass inflates into the same block
    }
    CK_TRY(o.deliver(ctx));
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_png_encode_bound(int h, int w, size_t* bytes)
{
    if (!bytes) return ck_fail(nullptr, CK_ERR_ARG, "bytes is NULL");
    CK_TRY(check_png_size(nullptr, h, w));
    *bytes = ck_png_bound(h, w);
    return CK_OK;
}

int ck_png_encode_staged_mode(const uint8_t* bgr, int n, int h, int w, int filter, int matches, uint8_t* out, size_t stride, size_t* len)
{
    if (!bgr || !out || !len || n <= 0) return ck_fail(nullptr, CK_ERR_ARG, "NULL pointer or n <= 0");
    CK_TRY(check_png_size(nullptr, h, w));
    if (filter < -1 || filter > 4) return ck_fail(nullptr, CK_ERR_ARG, "filter %d: 0 .. 4, or -1 to choose per row", filter);
    if (matches != CK_PNG_MATCH_NONE && matches != CK_PNG_MATCH_RUNS) return ck_fail(nullptr, CK_ERR_ARG, "unknown PNG match mode %d", matches);
    CK_HOST_BEGIN
    char msg[CK_PNG_MSG];
    const int rc = ck_png_stage_encode(bgr, n, h, w, filter, out, stride, len, msg, matches == CK_PNG_MATCH_RUNS);
    return rc == CK_OK ? CK_OK : ck_fail(nullptr, rc, "%s", msg);
    CK_HOST_END
}

int ck_png_encode_staged(const uint8_t* bgr, int n, int h, int w, int filter, uint8_t* out, size_t stride, size_t* len)
{
    return ck_png_encode_staged_mode(bgr, n, h, w, filter, CK_PNG_MATCH_NONE, out, stride, len);
}

int ck_png_set_encode_matches(ck_ctx* ctx, int mode)
{
    CK_API_BEGIN(ctx)
    if (mode != CK_PNG_MATCH_NONE && mode != CK_PNG_MATCH_RUNS) return ck_fail(ctx, CK_ERR_ARG, "unknown PNG match mode %d", mode);
    ctx->png_matches = mode;
    return CK_OK;
    CK_API_END(ctx)
}

// the histograms the count step of the last pass left in png_work -> png_tokens, two numbers a frame.  known_literals >= 0
// (the literal-only mode between two passes of one call, where every byte of a frame is one literal token): that number
// for every frame, nothing is copied
static int png_read_counts(ck_ctx* ctx, long long known_literals = -1)
{
    const int m = ctx->png_count_frames;
    if (m <= 0) return CK_OK;
    if (known_literals >= 0 && !ctx->png_count_runs) {
        for (int f = 0; f < m; f++) { ctx->png_tokens.push_back(known_literals); ctx->png_tokens.push_back(0); }
        ctx->png_count_frames = 0;
        return CK_OK;
    }
    const size_t pitch = (size_t)ck_png_pitch(ctx->png_count_runs), per = (size_t)ctx->png_count_bands * pitch;
    std::vector<uint32_t> count((size_t)m * per);
    CK_HIP(ctx, hipMemcpyAsync(count.data(), (const uint8_t*)ctx->png_work.p + ctx->png_count_at, count.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int f = 0; f < m; f++) {
        long long lit = 0, match = 0;
        for (long long band = 0; band < ctx->png_count_bands; band++) {
            const uint32_t* c = count.data() + (size_t)f * per + (size_t)band * pitch;
            for (int s = 0; s < 256; s++) lit += c[s];
            if (ctx->png_count_runs)
                for (int s = 257; s < CK_PNG_RUN_SYMS; s++) match += c[s];
        }
        ctx->png_tokens.push_back(lit);
        ctx->png_tokens.push_back(match);
    }
    ctx->png_count_frames = 0;
    return CK_OK;
}

int ck_png_run_stats(ck_ctx* ctx, int n, long long* literals, long long* matches)
{
    CK_API_BEGIN(ctx)
    if (!literals || !matches) return ck_fail(ctx, CK_ERR_ARG, "NULL pointer");
    CK_TRY(png_read_counts(ctx));
    if (ctx->png_tokens.empty()) return ck_fail(ctx, CK_ERR_STATE, "no ck_png_encode of this context has completed: there are no tokens to report");
    if (n <= 0 || (size_t)n * 2 != ctx->png_tokens.size())
        return ck_fail(ctx, CK_ERR_STATE, "the last ck_png_encode took %zu frames, not %d", ctx->png_tokens.size() / 2, n);
    for (int f = 0; f < n; f++) { literals[f] = ctx->png_tokens[2 * (size_t)f]; matches[f] = ctx->png_tokens[2 * (size_t)f + 1]; }
    return CK_OK;
    CK_API_END(ctx)
}

int ck_png_encode(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space, int filter, uint8_t* out, size_t stride, size_t* len)
{
    CK_API_BEGIN(ctx)
    if (!bgr || !out || !len || n <= 0) return ck_fail(ctx, CK_ERR_ARG, "NULL pointer or n <= 0");
    CK_TRY(check_png_size(ctx, h, w));
    if (filter < -1 || filter > 4) return ck_fail(ctx, CK_ERR_ARG, "filter %d: 0 .. 4, or -1 to choose per row", filter);
    if (stride < ck_png_bound(h, w))
        return ck_fail(ctx, CK_ERR_ARG, "output buffer of %zu bytes per frame: smaller than the bound of %zu for a %dx%d frame", stride, ck_png_bound(h, w), w, h);
    const CkPngGeom g = ck_png_geom(h, w);
    const size_t iframe = (size_t)h * w * 3;
    const int runs = ctx->png_matches == CK_PNG_MATCH_RUNS;
    ctx->png_tokens.clear();
    ctx->png_count_frames = 0;
    const int pass = ck_pass_fit(n, (size_t)g.fbytes, PNG_ENCODE_PASS_BYTES);
    for (int f0 = 0; f0 < n; f0 += pass) {
        const int m = n - f0 < pass ? n - f0 : pass;
        // the histograms of the pass before this one are overwritten now: the runs mode reads them first (a copy and a wait
        // per further pass of a call above 1 GiB); the literal-only mode copies nothing, its tokens are the frame's bytes
        CK_TRY(png_read_counts(ctx, (long long)g.fbytes));
        const void* d_in;
        CK_TRY(ck_to_device(ctx, bgr + (size_t)f0 * iframe, (size_t)m * iframe, in_space, ctx->in_stage, &d_in));
        const CkPngWorkLayout L = ck_png_work_layout(g, m, runs);
        CK_TRY(ck_ensure(ctx, ctx->png_work, L.total));
        uint8_t* wp = (uint8_t*)ctx->png_work.p;
        CkPngWork wk;
        wk.head = (uint64_t*)(wp + L.head); wk.tile_off = (uint64_t*)(wp + L.tile_off); wk.band_off = (uint64_t*)(wp + L.band_off);
        wk.frame_bits = (uint64_t*)(wp + L.frame_bits); wk.out_off = (uint64_t*)(wp + L.out_off); wk.count = (uint32_t*)(wp + L.count);
        wk.tile_bits = (uint32_t*)(wp + L.tile_bits); wk.tile_a = (uint32_t*)(wp + L.tile_a); wk.tile_b = (uint32_t*)(wp + L.tile_b);
        wk.band_bits = (uint64_t*)(wp + L.band_bits); wk.band_a = (uint32_t*)(wp + L.band_a); wk.band_b = (uint32_t*)(wp + L.band_b);
        wk.adler = (uint32_t*)(wp + L.adler); wk.codes = (uint16_t*)(wp + L.codes); wk.lens = wp + L.lens; wk.filt = wp + L.filt;
        wk.before = runs ? (uint32_t*)(wp + L.before) : nullptr; wk.after = runs ? (uint32_t*)(wp + L.after) : nullptr;
        wk.edge = runs ? (CkPngEdge*)(wp + L.edge) : nullptr;
        CK_TRY(k_png_enc_measure(ctx, (const uint8_t*)d_in, m, g, filter, wk, runs));
        ctx->png_count_at = L.count; ctx->png_count_frames = m; ctx->png_count_runs = runs; ctx->png_count_bands = g.bands;
        CK_TRY(ck_ensure_pinned(ctx, ctx->host_pinned2, ((size_t)m + 1) * 8));
        uint64_t* words = (uint64_t*)ctx->host_pinned2.p;
        CK_HIP(ctx, hipMemcpyAsync(words, wk.head, ((size_t)m + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        CK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const size_t total = (size_t)words[0];
        CkCarve pack;                                              // the streams one behind the other, each on 16 bytes (out_off)
        std::vector<size_t> off((size_t)m);
        for (int f = 0; f < m; f++) {
            if (CK_PNG_CONTAINER + words[1 + f] > stride) return ck_fail(ctx, CK_ERR_STATE, "frame %d: a stream of %llu bytes, above the bound", f0 + f, (unsigned long long)words[1 + f]);
            off[f] = pack.take((size_t)words[1 + f]);
        }
        if (pack.size() != total) return ck_fail(ctx, CK_ERR_STATE, "the streams of a pass: %zu bytes where their sizes give %zu", total, pack.size());
        CK_TRY(ck_ensure(ctx, ctx->png_pack, total + 16));
        CK_TRY(k_png_enc_put(ctx, m, g, wk, (uint32_t*)ctx->png_pack.p, total + 16, runs));
        CK_TRY(ck_ensure_pinned(ctx, ctx->host_pinned, total));
        CK_HIP(ctx, hipMemcpyAsync(ctx->host_pinned.p, ctx->png_pack.p, total, hipMemcpyDeviceToHost, ctx->stream));
        CK_TRY(finish(ctx));
        // the container around every stream -- a copy and a CRC-32 over its bytes -- the frames on the worker threads
        ck_parallel_for(m, 16, [&](int f) {
            len[f0 + f] = ck_png_wrap((const uint8_t*)ctx->host_pinned.p + off[f], (size_t)words[1 + f], h, w, out + (size_t)(f0 + f) * stride);
        });
    }
    return CK_OK;
    CK_API_END(ctx)
}

}  // extern "C"
