// ck_api.hip -- C-ABI entry points of libck_hip.so (see include/camkifu_amd.h).
// Host-side glue only: argument checks, staging between host and HBM, and the order in
// which the stage kernels are launched on the context's stream.
#include <stdarg.h>
#include <stddef.h>
#include <stdlib.h>

#include <cfloat>
#include <cmath>
#include <algorithm>
#include <vector>
#include <thread>
#include <chrono>

#include "ck_common.h"
#include "ck_api_util.h"
#include "ck_stage_layout.h"
#include "ck_stonegeom.h"
#include "ck_overlay.h"

thread_local std::string g_ck_create_error;
static thread_local const ck_ctx* g_ck_busy_ctx = nullptr;     // the context that refused this thread's last call

unsigned long long ck_thread_token()
{
    static std::atomic<unsigned long long> next{1};
    static thread_local unsigned long long mine = 0;
    if (!mine) mine = next.fetch_add(1);
    return mine;
}
void ck_note_busy(const ck_ctx* ctx) { g_ck_busy_ctx = ctx; }

int ck_fail(ck_ctx* ctx, int code, const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf; else g_ck_create_error = buf;
    return code;
}

// the allocator under DevBuf and PinBuf (ck_buf.h): the only calls of it in the library
int ck_dev_alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
int ck_dev_free(void* p) { return (int)hipFree(p); }
int ck_pin_alloc(void** p, size_t bytes, unsigned flags) { return (int)hipHostMalloc(p, bytes, flags); }
int ck_pin_free(void* p) { return (int)hipHostFree(p); }
static_assert(CK_PIN_DEFAULT == hipHostMallocDefault && CK_PIN_MAPPED == hipHostMallocMapped, "ck_buf.h restates the flags");

int ck_ensure(ck_ctx* ctx, DevBuf& b, size_t bytes)
{
    if (bytes <= b.cap) return CK_OK;
    if (b.p) CK_HIP(ctx, hipStreamSynchronize(ctx->stream));      // queued work may still use the old block
    CK_HIP(ctx, (hipError_t)b.reserve(bytes, bytes + bytes / 8 + 256));
    return CK_OK;
}

int ck_ensure_pinned(ck_ctx* ctx, PinBuf& b, size_t bytes, size_t slack)
{
    // a little headroom: the survey's point count changes from batch to batch
    CK_HIP(ctx, (hipError_t)b.reserve(bytes, bytes + bytes / 4 + slack));
    return CK_OK;
}

int ck_to_device(ck_ctx* ctx, const void* src, size_t bytes, int space, DevBuf& stage, const void** dev)
{
    if (space == CK_DEVICE) { *dev = src; return CK_OK; }
    if (space != CK_HOST) return ck_fail(ctx, CK_ERR_ARG, "bad memory space %d", space);
    CK_TRY(ck_ensure(ctx, stage, bytes));
    CK_HIP(ctx, hipMemcpyAsync(stage.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    *dev = stage.p;
    return CK_OK;
}

int ck_from_device(ck_ctx* ctx, void* dst, const void* dev, size_t bytes, int space)
{
    if (!dst || dst == dev) return CK_OK;
    if (space == CK_DEVICE) {
        CK_HIP(ctx, hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        CK_HIP(ctx, hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    return CK_OK;
}

int ck_coef_on_16(ck_ctx* ctx, const void* coef)
{
    if ((uintptr_t)coef & 15) return ck_fail(ctx, CK_ERR_ARG, "coefficients must lie on 16 bytes");
    return CK_OK;
}
int ck_coef_quant_on_16(ck_ctx* ctx, const void* coef, const void* quant)
{
    if (((uintptr_t)coef | (uintptr_t)quant) & 15) return ck_fail(ctx, CK_ERR_ARG, "coefficients and quant tables must lie on 16 bytes");
    return CK_OK;
}

// ---- timing ---------------------------------------------------------------------------
TimeScope::TimeScope(ck_ctx* c, const char* name) : ctx(c)
{
    if (!ctx->timing) return;
    PendingEvent pe;
    auto get = [&](hipEvent_t* e) {
        if (!ctx->event_pool.empty()) { *e = ctx->event_pool.back(); ctx->event_pool.pop_back(); }
        else (void)hipEventCreate(e);
    };
    get(&pe.a); get(&pe.b);
    pe.name = name;
    (void)hipEventRecord(pe.a, ctx->stream);
    ctx->pending.push_back(pe);
    idx = (int)ctx->pending.size() - 1;
}
TimeScope::~TimeScope()
{
    if (idx >= 0) (void)hipEventRecord(ctx->pending[idx].b, ctx->stream);
}

int ck_timing_collect(ck_ctx* ctx)
{
    for (auto& pe : ctx->pending) {
        float ms = 0;
        if (hipEventSynchronize(pe.b) == hipSuccess && hipEventElapsedTime(&ms, pe.a, pe.b) == hipSuccess) {
            auto& s = ctx->slots[pe.name];
            s.ms += ms; s.launches += 1;
        }
        ctx->event_pool.push_back(pe.a);
        ctx->event_pool.push_back(pe.b);
    }
    ctx->pending.clear();
    return CK_OK;
}

// OpenCV's getThreshVal_Otsu_8u restated (double arithmetic, the FLT_EPSILON guards, first maximum wins)
double ck_otsu_level(const int* hist, size_t npx)
{
    double mu = 0, scale = 1. / (double)npx;
    for (int i = 0; i < 256; i++) mu += i * (double)hist[i];
    mu *= scale;
    double mu1 = 0, q1 = 0, max_sigma = 0, max_val = 0;
    for (int i = 0; i < 256; i++) {
        const double p_i = hist[i] * scale;
        mu1 *= q1;
        q1 += p_i;
        const double q2 = 1. - q1;
        if (std::min(q1, q2) < FLT_EPSILON || std::max(q1, q2) > 1. - FLT_EPSILON) continue;
        mu1 = (mu1 + i * p_i) / q1;
        const double mu2 = (mu - q1 * mu1) / q2;
        const double sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2);
        if (sigma > max_sigma) { max_sigma = sigma; max_val = i; }
    }
    return max_val;
}

// the device half of ck_goban_canny: interleaved BGR on the device -> edge maps on the device (one host round trip
// for the Otsu levels of the batch).  Scratch: planes, out_stage, misc, map, labels, mats.
int ck_goban_canny_dev(ck_ctx* ctx, const uint8_t* d_in, int n, int h, int w, uint8_t* d_edges, double* otsu_out)
{
    const size_t npx1 = (size_t)h * w, npx = (size_t)n * npx1;
    const int pitch = ck_pitch(w);
    CK_TRY(ck_ensure(ctx, ctx->planes, (size_t)n * 3 * h * pitch));
    CK_TRY(ck_ensure(ctx, ctx->out_stage, npx * 3));
    // medianBlur 13, then 7 (the kernel reads interleaved BGR and writes planes)
    CK_TRY(k_median_planar(ctx, d_in, n, h, w, 13, (uint8_t*)ctx->planes.p, pitch));
    CK_TRY(k_planar_to_interleaved(ctx, (const uint8_t*)ctx->planes.p, n, h, w, pitch, (uint8_t*)ctx->out_stage.p));
    CK_TRY(ck_ensure(ctx, ctx->trange, ck_range_bytes(n, h, w)));
    CK_TRY(k_median_planar(ctx, (const uint8_t*)ctx->out_stage.p, n, h, w, 7, (uint8_t*)ctx->planes.p, pitch, (uint8_t*)ctx->trange.p));
    // grey histogram per frame -> Otsu level on the host (256 bins, double arithmetic as the library does it)
    CK_TRY(ck_ensure(ctx, ctx->misc, (size_t)n * 256 * 4 + (size_t)n * 64 + 4096));
    int* d_hist = (int*)ctx->misc.p;
    CK_TRY(k_gray_hist(ctx, (const uint8_t*)ctx->planes.p, n, h, w, pitch, d_hist));
    std::vector<int> hist((size_t)n * 256);
    CK_HIP(ctx, hipMemcpyAsync(hist.data(), d_hist, hist.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    CK_TRY(ck_ensure(ctx, ctx->map, npx));
    CK_TRY(ck_ensure(ctx, ctx->labels, npx * 4));
    // cv2.Canny(median, otsu / 2, otsu): thresholds are floored (L1 gradient); one pair per frame, one batched call
    std::vector<int> thr((size_t)n * 2);
    for (int f = 0; f < n; f++) {
        const double otsu = ck_otsu_level(&hist[(size_t)f * 256], npx1);
        if (otsu_out) otsu_out[f] = otsu;
        thr[2 * f] = (int)std::floor(otsu / 2);
        thr[2 * f + 1] = (int)std::floor(otsu);
    }
    CK_TRY(ck_ensure(ctx, ctx->mats, (size_t)n * 8 + 1024));
    int* d_thr = (int*)ctx->mats.p;
    CK_HIP(ctx, hipMemcpyAsync(d_thr, thr.data(), thr.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    CK_HIP(ctx, hipStreamSynchronize(ctx->stream));           // thr is a local: the copy must be done before it goes
    return k_canny_planar(ctx, (const uint8_t*)ctx->planes.p, n, h, w, pitch, 0, 0, (uint8_t*)ctx->map.p,
                          (int32_t*)ctx->labels.p, d_edges, nullptr, nullptr, d_thr, (const uint8_t*)ctx->trange.p);
}

// ---- handles: an index into the context's models / trainers, valid while that slot is alive ----
static int mog2_of(ck_ctx* ctx, int handle, Mog2State** st)
{
    if (handle < 0 || handle >= (int)ctx->mog2.size() || !ctx->mog2[handle].alive)
        return ck_fail(ctx, CK_ERR_ARG, "bad mog2 handle %d", handle);
    *st = &ctx->mog2[handle];
    return CK_OK;
}

static int trainer_of(ck_ctx* ctx, int handle, CkTrainer** tr)
{
    if (handle < 0 || handle >= (int)ctx->trainers.size() || !ctx->trainers[handle].alive)
        return ck_fail(ctx, CK_ERR_ARG, "bad trainer handle %d", handle);
    *tr = &ctx->trainers[handle];
    return CK_OK;
}

// the first slot that is not alive (a dead model keeps its memory for the next one), else a new one at the end
template <class T>
static int free_slot(std::vector<T>& slots)
{
    for (size_t i = 0; i < slots.size(); i++) if (!slots[i].alive) return (int)i;
    slots.emplace_back();
    return (int)slots.size() - 1;
}

extern "C" {

int ck_version(void) { return 100; }

int ck_ctx_create(int device, ck_ctx** out) { return ck_ctx_create_prio(device, 0, out); }

int ck_ctx_create_prio(int device, int priority, ck_ctx** out)
{
    if (!out) return ck_fail(nullptr, CK_ERR_ARG, "out is NULL");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return ck_fail(nullptr, CK_ERR_HIP, "no HIP device available (%s)", hipGetErrorString(e));
    if (device < 0 || device >= count) return ck_fail(nullptr, CK_ERR_ARG, "device %d out of range [0,%d)", device, count);
    e = hipSetDevice(device);
    if (e != hipSuccess) return ck_fail(nullptr, CK_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    ck_ctx* ctx = new ck_ctx();
    ctx->device = device;
    if (priority == 0)
        e = hipStreamCreateWithFlags(&ctx->stream.s, hipStreamNonBlocking);
    else {
        int least = 0, greatest = 0;                     // (numerically: greatest priority = the smaller number)
        e = hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&ctx->stream.s, hipStreamNonBlocking, priority > 0 ? greatest : least);
    }
    if (e != hipSuccess) { delete ctx; return ck_fail(nullptr, CK_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    *out = ctx;
    return CK_OK;
}

void ck_ctx_destroy(ck_ctx* ctx)
{
    if (ck_ctx_destroy2(ctx) == CK_ERR_STATE)
        fprintf(stderr, "ck_ctx_destroy: context %p is still in use by another thread after 5 s; not freed\n", (void*)ctx);
}

int ck_stream_wait(ck_ctx* ctx, void* stream)
{
    CK_API_BEGIN(ctx)
    if (!ctx->handover) CK_HIP(ctx, hipEventCreateWithFlags(&ctx->handover, hipEventDisableTiming));
    CK_HIP(ctx, hipEventRecord(ctx->handover, (hipStream_t)stream));
    CK_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->handover, 0));
    return CK_OK;
    CK_API_END(ctx)
}

int ck_ctx_destroy2(ck_ctx* ctx)
{
    if (!ctx) return CK_OK;
    // A thread still inside an entry point owns the stream and the scratch buffers: freeing them under it would be a
    // use-after-free.  Wait for it to leave (a call is milliseconds); a context that stays busy is leaked, and said so.
    unsigned long long nobody = 0;
    const unsigned long long me = ck_thread_token();
    for (int spin = 0; !ctx->owner.compare_exchange_strong(nobody, me, std::memory_order_acq_rel); spin++) {
        if (nobody == me) break;                     // destroyed from inside one of its own calls: nothing to wait for
        if (spin >= 5000) return CK_ERR_STATE;          // still busy: not freed, the handle stays valid
        nobody = 0;
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    delete ctx;
    return CK_OK;
}

}  // extern "C"

// after ck_ctx_destroy2 has synchronised the stream: the events go here, every buffer frees itself, the stream goes last
ck_ctx::~ck_ctx()
{
    for (auto& m : mog2) if (m.rates_done) (void)hipEventDestroy(m.rates_done);
    for (auto& pe : pending) { (void)hipEventDestroy(pe.a); (void)hipEventDestroy(pe.b); }
    for (auto e : event_pool) (void)hipEventDestroy(e);
    if (handover) (void)hipEventDestroy(handover);
}

extern "C" {

const char* ck_last_error(const ck_ctx* ctx)
{
    if (!ctx) return g_ck_create_error.c_str();
    if (g_ck_busy_ctx == ctx) {              // this thread's call was refused: ctx->err belongs to the thread inside
        g_ck_busy_ctx = nullptr;
        return "the context is in use by another thread (a ck_ctx is single-threaded: one context per finder / thread)";
    }
    return ctx->err.c_str();
}
int ck_backend(const ck_ctx*) { return CK_BACKEND_HIP; }
void* ck_stream(ck_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int ck_timing_enable(ck_ctx* ctx, int on)
{
    CK_API_BEGIN(ctx)
    ctx->timing = on != 0;
    return CK_OK;
    CK_API_END(ctx)
}
int ck_timing_reset(ck_ctx* ctx)
{
    CK_API_BEGIN(ctx)
    ck_timing_collect(ctx);
    ctx->slots.clear();
    return CK_OK;
    CK_API_END(ctx)
}
int ck_timing_get(ck_ctx* ctx, const char* name, double* total_ms, int* launches)
{
    CK_API_BEGIN(ctx)
    if (!name) return CK_ERR_ARG;
    ck_timing_collect(ctx);
    auto it = ctx->slots.find(name);
    if (total_ms) *total_ms = it == ctx->slots.end() ? 0.0 : it->second.ms;
    if (launches) *launches = it == ctx->slots.end() ? 0 : it->second.launches;
    return CK_OK;
    CK_API_END(ctx)
}

// Overwrite whatever a call may find in scratch memory (include/camkifu_amd.h).  The weight packs, the MOG2 models (their
// rate staging included: it belongs to the model) and a trainer's w, m, v are state and are not touched; cnn_flag is a
// flag the split-precision kernels only ever raise, cleared by the host before each batch, and is no scratch either.
int ck_debug_scratch_fill(ck_ctx* ctx, int byte, long long* bytes_filled, int* buffers_filled)
{
    CK_API_BEGIN(ctx)
    if (byte < 0 || byte > 255) return ck_fail(ctx, CK_ERR_ARG, "fill byte %d: 0 .. 255", byte);
    CK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    long long bytes = 0;
    int buffers = 0;
    hipError_t bad = hipSuccess;
    auto fill = [&](DevBuf& b) {
        if (!b.p || !b.cap || bad != hipSuccess) return;
        bad = hipMemsetAsync(b.p, byte, b.cap, ctx->stream);
        bytes += (long long)b.cap; buffers++;
    };
    ck_for_each_scratch(*ctx, fill);
    // A trainer: what a call writes before it reads it.  g is among them: ck_train_grads / ck_train_step write all twelve
    // arrays of it (tr_reduce with accumulate = 0 for the first chunk) and ck_train_apply copies all twelve in before
    // tr_adam reads them; no entry point reads the gradients of an earlier call.
    for (CkTrainer& tr : ctx->trainers) {
        if (!tr.alive) continue;
        DevBuf* const per_call[] = { &tr.g, &tr.lab, &tr.a1, &tr.a2, &tr.p1, &tr.a3, &tr.a4, &tr.p2, &tr.h1, &tr.lg, &tr.dlg, &tr.dh1,
                                     &tr.dp2, &tr.dz4, &tr.dz3, &tr.dp1, &tr.dz2, &tr.dz1, &tr.part, &tr.lossv, &tr.mask1, &tr.mask2,
                                     &tr.mask3 };
        for (DevBuf* b : per_call) fill(*b);
    }
    if (bad != hipSuccess) return ck_fail(ctx, CK_ERR_HIP, "hipMemsetAsync failed: %s", hipGetErrorString(bad));
    for (PinBuf* b : { &ctx->host_pinned, &ctx->host_pinned2, &ctx->rec_host }) {
        if (!b->p || !b->cap) continue;
        memset(b->p, byte, b->cap);
        bytes += (long long)b->cap; buffers++;
    }
    // the two results that lie in scratch between calls: gone with it
    ctx->jenc_freq_frames = 0;
    ctx->jenc_freq_at = 0;
    ctx->png_tokens.clear();
    ctx->png_count_frames = 0;
    CK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bytes_filled) *bytes_filled = bytes;
    if (buffers_filled) *buffers_filled = buffers;
    return CK_OK;
    CK_API_END(ctx)
}

static int check_img(ck_ctx* ctx, const void* p, int n, int h, int w)
{
    if (!p) return ck_fail(ctx, CK_ERR_ARG, "image pointer is NULL");
    if (n <= 0 || h <= 0 || w <= 0) return ck_fail(ctx, CK_ERR_ARG, "bad shape n=%d h=%d w=%d", n, h, w);
    if ((long long)h * w > (1LL << 28)) return ck_fail(ctx, CK_ERR_ARG, "image too large");
    return CK_OK;
}

int ck_median15(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space, uint8_t* out, int out_space)
{
    return ck_median(ctx, bgr, n, h, w, 15, in_space, out, out_space);
}

int ck_median(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int ksize, int in_space, uint8_t* out, int out_space)
{
    CK_API_BEGIN(ctx)
    CK_TRY(check_img(ctx, bgr, n, h, w));
    if (!out) return ck_fail(ctx, CK_ERR_ARG, "out is NULL");
    if (ksize < 3 || ksize > 17 || !(ksize & 1)) return ck_fail(ctx, CK_ERR_ARG, "median window %d: odd sizes 3..17 only", ksize);
    const size_t bytes = (size_t)n * h * w * 3;
    const int pitch = ck_pitch(w);
    const void* d_in;
    CK_TRY(ck_to_device(ctx, bgr, bytes, in_space, ctx->in_stage, &d_in));
    CK_TRY(ck_ensure(ctx, ctx->planes, (size_t)n * 3 * h * pitch));
    CK_TRY(k_median_planar(ctx, (const uint8_t*)d_in, n, h, w, ksize, (uint8_t*)ctx->planes.p, pitch));
    OutStage<uint8_t> o;
    CK_TRY(o.open(ctx, out, bytes, out_space, ctx->out_stage));
    CK_TRY(k_planar_to_interleaved(ctx, (const uint8_t*)ctx->planes.p, n, h, w, pitch, o.dev));
    CK_TRY(o.deliver(ctx));
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_canny(ck_ctx* ctx, const uint8_t* img3, int n, int h, int w, int in_space,
             int low, int high, uint8_t* edges, uint8_t* map_out, int out_space)
{
    CK_API_BEGIN(ctx)
    CK_TRY(check_img(ctx, img3, n, h, w));
    if (!edges) return ck_fail(ctx, CK_ERR_ARG, "edges is NULL");
    const size_t npx = (size_t)n * h * w;
    const int pitch = ck_pitch(w);
    const void* d_in;
    CK_TRY(ck_to_device(ctx, img3, npx * 3, in_space, ctx->in_stage, &d_in));
    CK_TRY(ck_ensure(ctx, ctx->planes, (size_t)n * 3 * h * pitch));
    CK_TRY(k_interleaved_to_planar(ctx, (const uint8_t*)d_in, n, h, w, pitch, (uint8_t*)ctx->planes.p));
    CK_TRY(ck_ensure(ctx, ctx->map, npx));
    CK_TRY(ck_ensure(ctx, ctx->labels, npx * 4));
    OutStage<uint8_t> oe, om;
    CK_TRY(oe.open(ctx, edges, npx, out_space, ctx->edges));
    CK_TRY(om.open(ctx, map_out, npx, out_space, ctx->out_stage));
    CK_TRY(k_canny_planar(ctx, (const uint8_t*)ctx->planes.p, n, h, w, pitch, low, high,
                          (uint8_t*)ctx->map.p, (int32_t*)ctx->labels.p, oe.dev, om.dev));
    CK_TRY(oe.deliver(ctx));
    CK_TRY(om.deliver(ctx));
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_goban_canny(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space, uint8_t* edges, int out_space,
                   double* otsu_out)
{
    CK_API_BEGIN(ctx)
    CK_TRY(check_img(ctx, bgr, n, h, w));
    if (!edges) return ck_fail(ctx, CK_ERR_ARG, "edges is NULL");
    const size_t npx = (size_t)n * h * w;
    const void* d_in;
    CK_TRY(ck_to_device(ctx, bgr, npx * 3, in_space, ctx->in_stage, &d_in));
    OutStage<uint8_t> o;
    CK_TRY(o.open(ctx, edges, npx, out_space, ctx->edges));
    CK_TRY(ck_goban_canny_dev(ctx, (const uint8_t*)d_in, n, h, w, o.dev, otsu_out));
    CK_TRY(o.deliver(ctx));
    return finish(ctx);
    CK_API_END(ctx)
}

static int board_edges_dev(ck_ctx* ctx, const uint8_t* d_bgr, int n, int h, int w, uint8_t* d_edges,
                           int* d_border_flag = nullptr)
{
    const size_t npx = (size_t)n * h * w;
    const int pitch = ck_pitch(w);
    CK_TRY(ck_ensure(ctx, ctx->planes, (size_t)n * 3 * h * pitch));
    CK_TRY(ck_ensure(ctx, ctx->map, npx));
    CK_TRY(ck_ensure(ctx, ctx->labels, npx * 4));
    CK_TRY(ck_ensure(ctx, ctx->trange, ck_range_bytes(n, h, w)));
    CK_TRY(k_median15_planar(ctx, d_bgr, n, h, w, (uint8_t*)ctx->planes.p, pitch, (uint8_t*)ctx->trange.p));
    CK_TRY(k_canny_planar(ctx, (const uint8_t*)ctx->planes.p, n, h, w, pitch, 25, 75,
                          (uint8_t*)ctx->map.p, (int32_t*)ctx->labels.p, d_edges, nullptr, d_border_flag, nullptr,
                          (const uint8_t*)ctx->trange.p));
    return CK_OK;
}

int ck_board_edges(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space, uint8_t* edges, int out_space)
{
    CK_API_BEGIN(ctx)
    CK_TRY(check_img(ctx, bgr, n, h, w));
    if (!edges) return ck_fail(ctx, CK_ERR_ARG, "edges is NULL");
    const size_t npx = (size_t)n * h * w;
    const void* d_in;
    CK_TRY(ck_to_device(ctx, bgr, npx * 3, in_space, ctx->in_stage, &d_in));
    OutStage<uint8_t> o;
    CK_TRY(o.open(ctx, edges, npx, out_space, ctx->edges));
    CK_TRY(board_edges_dev(ctx, (const uint8_t*)d_in, n, h, w, o.dev));
    CK_TRY(o.deliver(ctx));
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_board_lines(ck_ctx* ctx, const uint8_t* edges, int n, int h, int w, int in_space,
                   int hough_thresh, float* lines, int cap, ck_board_result* res,
                   uint8_t* ghost_out, int ghost_space)
{
    CK_API_BEGIN(ctx)
    CK_TRY(check_img(ctx, edges, n, h, w));
    if (!lines || !res || cap <= 0) return ck_fail(ctx, CK_ERR_ARG, "lines/res NULL or cap <= 0");
    if (h < 3 || w < 3) return ck_fail(ctx, CK_ERR_ARG, "image smaller than 3x3");
    const size_t npx = (size_t)n * h * w;
    const void* d_in;
    CK_TRY(ck_to_device(ctx, edges, npx, in_space, ctx->in_stage2, &d_in));
    if (hough_thresh < 0) hough_thresh = (int)((h < w ? h : w) / 5.0);
    OutStage<uint8_t> ghost;
    CK_TRY(ghost.open(ctx, ghost_out, npx, ghost_space, ctx->out_stage));
    CK_TRY(k_board_lines(ctx, (const uint8_t*)d_in, n, h, w, hough_thresh, lines, cap, res, ghost.dev));
    CK_TRY(ghost.deliver(ctx));
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_board_detect(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space,
                    int hough_thresh, float* lines, int cap, ck_board_result* res)
{
    CK_API_BEGIN(ctx)
    CK_TRY(check_img(ctx, bgr, n, h, w));
    if (!lines || !res || cap <= 0) return ck_fail(ctx, CK_ERR_ARG, "lines/res NULL or cap <= 0");
    if (h < 3 || w < 3) return ck_fail(ctx, CK_ERR_ARG, "image smaller than 3x3");
    const size_t npx = (size_t)n * h * w;
    const void* d_in;
    CK_TRY(ck_to_device(ctx, bgr, npx * 3, in_space, ctx->in_stage, &d_in));
    CK_TRY(ck_ensure(ctx, ctx->edges, npx));
    CK_TRY(ck_ensure(ctx, ctx->bflag, (size_t)n * 4));
    // K2 leaves its hysteresis labels in ctx->labels, which is also K3's parent image: K3 keeps the edge
    // components Canny already built (frames with an edge on the image frame are relabelled from scratch)
    CK_TRY(board_edges_dev(ctx, (const uint8_t*)d_in, n, h, w, (uint8_t*)ctx->edges.p, (int*)ctx->bflag.p));
    if (hough_thresh < 0) hough_thresh = (int)((h < w ? h : w) / 5.0);
    CK_TRY(k_board_lines(ctx, (const uint8_t*)ctx->edges.p, n, h, w, hough_thresh, lines, cap, res, nullptr,
                         (const int*)ctx->bflag.p));
    return finish(ctx);
    CK_API_END(ctx)
}

static int upload_minv(ck_ctx* ctx, const double* M, int m_count, int n, const double** d_minv)
{
    if (!M) return ck_fail(ctx, CK_ERR_ARG, "M is NULL");
    if (m_count != 1 && m_count != n) return ck_fail(ctx, CK_ERR_ARG, "m_count must be 1 or n");
    std::vector<double> inv((size_t)m_count * 9);
    for (int i = 0; i < m_count; i++) ck_invert3x3(M + 9 * i, inv.data() + 9 * i);
    CK_TRY(ck_ensure(ctx, ctx->mats, inv.size() * sizeof(double)));
    // pageable source: the copy is staged by the runtime before the call returns
    CK_HIP(ctx, hipMemcpyAsync(ctx->mats.p, inv.data(), inv.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    CK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *d_minv = (const double*)ctx->mats.p;
    return CK_OK;
}

int ck_i420_to_bgr(ck_ctx* ctx, const uint8_t* i420, int n, int h, int w, int in_space, uint8_t* bgr, int out_space)
{
    CK_API_BEGIN(ctx)
    CK_TRY(check_img(ctx, i420, n, h, w));
    if (!bgr) return ck_fail(ctx, CK_ERR_ARG, "bgr is NULL");
    if ((h & 1) || (w & 1)) return ck_fail(ctx, CK_ERR_ARG, "I420 needs even dimensions, got %dx%d", w, h);
    const void* d_in;
    CK_TRY(ck_to_device(ctx, i420, (size_t)n * h * w * 3 / 2, in_space, ctx->in_stage2, &d_in));
    OutStage<uint8_t> o;
    CK_TRY(o.open(ctx, bgr, (size_t)n * h * w * 3, out_space, ctx->out_stage));
    CK_TRY(k_i420_to_bgr(ctx, (const uint8_t*)d_in, n, h, w, o.dev));
    CK_TRY(o.deliver(ctx));
    return finish(ctx);
    CK_API_END(ctx)
}

// the argument rules of both pyramid entry points, checked before any device work
static int check_pyr(ck_ctx* ctx, int h, int w, int levels)
{
    if (levels < 1) return ck_fail(ctx, CK_ERR_ARG, "pyramid levels %d: at least 1", levels);
    for (int l = 0; l < levels; l++, h = (h + 1) / 2, w = (w + 1) / 2)
        if (h < 2 || w < 2) return ck_fail(ctx, CK_ERR_ARG, "pyramid level %d would take a %dx%d image: sides below 2", l + 1, w, h);
    return CK_OK;
}

// bytes of n frames after `levels` halvings of h x w
static size_t pyr_out_bytes(int n, int h, int w, int levels)
{
    for (int l = 0; l < levels; l++) { h = (h + 1) / 2; w = (w + 1) / 2; }
    return (size_t)n * h * w * 3;
}

// levels `first` .. `levels` of the pyramid of n frames (h x w is the size level `first` reads), the last one into d_out;
// the levels between go through the context's ping-pong scratch
static int pyr_levels(ck_ctx* ctx, const uint8_t* d_in, int n, int h, int w, int first, int levels, uint8_t* d_out)
{
    for (int l = first; l <= levels; l++) {
        const int oh = (h + 1) / 2, ow = (w + 1) / 2;
        uint8_t* d_to = d_out;
        if (l < levels) {
            DevBuf& b = (l & 1) ? ctx->pyr1 : ctx->pyr0;
            CK_TRY(ck_ensure(ctx, b, (size_t)n * oh * ow * 3));
            d_to = (uint8_t*)b.p;
        }
        CK_TRY(k_pyr_down(ctx, d_in, n, h, w, d_to));
        d_in = d_to; h = oh; w = ow;
    }
    return CK_OK;
}

int ck_pyr_down(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int levels, int in_space, uint8_t* out, int out_space)
{
    CK_API_BEGIN(ctx)
    if (!bgr || !out) return ck_fail(ctx, CK_ERR_ARG, "image pointer is NULL");
    if (n <= 0 || h <= 0 || w <= 0) return ck_fail(ctx, CK_ERR_ARG, "bad shape n=%d h=%d w=%d", n, h, w);
    CK_TRY(check_pyr(ctx, h, w, levels));
    CK_TRY(check_img(ctx, bgr, n, h, w));
    const void* d_in;
    CK_TRY(ck_to_device(ctx, bgr, (size_t)n * h * w * 3, in_space, ctx->in_stage, &d_in));
    OutStage<uint8_t> o;
    CK_TRY(o.open(ctx, out, pyr_out_bytes(n, h, w, levels), out_space, ctx->out_stage));
    CK_TRY(pyr_levels(ctx, (const uint8_t*)d_in, n, h, w, 1, levels, o.dev));
    CK_TRY(o.deliver(ctx));
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_i420_to_bgr_pyr(ck_ctx* ctx, const uint8_t* i420, int n, int h, int w, int levels, int in_space, uint8_t* bgr, int out_space)
{
    CK_API_BEGIN(ctx)
    if (!i420 || !bgr) return ck_fail(ctx, CK_ERR_ARG, "image pointer is NULL");
    if (n <= 0 || h <= 0 || w <= 0) return ck_fail(ctx, CK_ERR_ARG, "bad shape n=%d h=%d w=%d", n, h, w);
    if ((h & 1) || (w & 1)) return ck_fail(ctx, CK_ERR_ARG, "I420 needs even dimensions, got %dx%d", w, h);
    CK_TRY(check_pyr(ctx, h, w, levels));
    CK_TRY(check_img(ctx, i420, n, h, w));
    const void* d_in;
    CK_TRY(ck_to_device(ctx, i420, (size_t)n * h * w * 3 / 2, in_space, ctx->in_stage2, &d_in));
    OutStage<uint8_t> o;
    CK_TRY(o.open(ctx, bgr, pyr_out_bytes(n, h, w, levels), out_space, ctx->out_stage));
    uint8_t* d_first = o.dev;                       // level 1, fused behind the conversion
    if (levels > 1) {
        CK_TRY(ck_ensure(ctx, ctx->pyr1, (size_t)n * (h / 2) * (w / 2) * 3));
        d_first = (uint8_t*)ctx->pyr1.p;
    }
    CK_TRY(k_i420_pyr_down(ctx, (const uint8_t*)d_in, n, h, w, d_first));
    if (levels > 1) CK_TRY(pyr_levels(ctx, d_first, n, h / 2, w / 2, 2, levels, o.dev));
    CK_TRY(o.deliver(ctx));
    return finish(ctx);
    CK_API_END(ctx)
}

// ---- overlays: the plan of ck_overlay.cpp, staged, and one launch of k_overlay.hip over its non-empty bins ----
int ck_overlay_draw(ck_ctx* ctx, uint8_t* img, int n, int h, int w, int c, int space,
                    const int32_t* prims, const int32_t* frame_start, const uint8_t* text, int text_len)
{
    CK_API_BEGIN(ctx)
    if (c != 1 && c != 3) return ck_fail(ctx, CK_ERR_ARG, "images of %d channels: 1 or 3", c);
    if (space != CK_HOST && space != CK_DEVICE) return ck_fail(ctx, CK_ERR_ARG, "bad memory space %d", space);
    char msg[CK_OV_MSG];
    if (ck_overlay_check(n, h, w, prims, frame_start, text_len, msg) != CK_OK) return ck_fail(ctx, CK_ERR_ARG, "%s", msg);
    if (n == 0 || frame_start[n] == 0) return CK_OK;
    if (!img) return ck_fail(ctx, CK_ERR_ARG, "image pointer is NULL");
    if (text_len > 0 && !text) return ck_fail(ctx, CK_ERR_ARG, "text is NULL");
    const int total = frame_start[n];
    const int nbx = (w + CK_OV_BIN - 1) / CK_OV_BIN, nby = (h + CK_OV_BIN - 1) / CK_OV_BIN;
    const size_t bins = (size_t)n * nbx * nby;
    int32_t bin_size = 0, n_refs = 0;
    std::vector<int32_t> bin_start(bins + 1);
    CK_TRY(ck_overlay_plan(n, h, w, prims, frame_start, text_len, &bin_size, bin_start.data(), nullptr, 0, &n_refs));
    if (n_refs == 0) return CK_OK;                               // everything lies outside the images
    size_t n_work = 0;
    for (size_t b = 0; b < bins; b++) n_work += bin_start[b + 1] > bin_start[b];
    if (n_work > 0x7fffffffu) return ck_fail(ctx, CK_ERR_ARG, "%zu bins to draw: too many", n_work);
    // one block of pinned memory goes up in one copy: work items | bin entries | records | text
    const size_t o_refs = n_work * 8, o_recs = o_refs + (size_t)n_refs, o_text = o_recs + (size_t)total * CK_OV_REC;
    const size_t bytes = o_text * sizeof(int32_t) + (size_t)text_len;
    CK_TRY(ck_ensure_pinned(ctx, ctx->host_pinned, bytes));
    int32_t* blob = (int32_t*)ctx->host_pinned.p;
    CK_TRY(ck_overlay_plan(n, h, w, prims, frame_start, text_len, &bin_size, bin_start.data(), blob + o_refs, n_refs, &n_refs));
    for (int i = 0; i < total; i++) ck_overlay_record(prims + (size_t)i * CK_OV_PRIM, blob + o_recs + (size_t)i * CK_OV_REC);
    if (text_len > 0) memcpy(blob + o_text, text, (size_t)text_len);
    size_t k = 0;
    for (size_t b = 0; b < bins; b++) {
        const int32_t first = bin_start[b], count = bin_start[b + 1] - first;
        if (count == 0) continue;
        int32_t blends = 0;
        for (int32_t j = 0; j < count && !blends; j++)
            blends = ((uint32_t)prims[(size_t)blob[o_refs + first + j] * CK_OV_PRIM + 6] >> 24) != 255;
        const size_t in_frame = b % ((size_t)nbx * nby);
        int32_t* wk = blob + k++ * 8;
        wk[0] = (int32_t)(b / ((size_t)nbx * nby)); wk[1] = (int32_t)(in_frame % nbx); wk[2] = (int32_t)(in_frame / nbx);
        wk[3] = first; wk[4] = count; wk[5] = blends; wk[6] = wk[7] = 0;
    }
    const void *d_img, *d_blob;
    const size_t img_bytes = (size_t)n * h * w * c;
    CK_TRY(ck_to_device(ctx, img, img_bytes, space, ctx->in_stage, &d_img));
    CK_TRY(ck_to_device(ctx, blob, bytes, CK_HOST, ctx->in_stage2, &d_blob));
    const int32_t* d32 = (const int32_t*)d_blob;
    CK_TRY(k_overlay(ctx, (uint8_t*)d_img, h, w, c, d32, (int)n_work, d32 + o_refs, d32 + o_recs, (const uint8_t*)(d32 + o_text)));
    if (space == CK_HOST) CK_TRY(ck_from_device(ctx, img, d_img, img_bytes, CK_HOST));
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_warp_perspective(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space,
                        const double* M, int m_count, int dsize, uint8_t* out, int out_space)
{
    CK_API_BEGIN(ctx)
    CK_TRY(check_img(ctx, bgr, n, h, w));
    if (!out || dsize <= 0) return ck_fail(ctx, CK_ERR_ARG, "out NULL or dsize <= 0");
    const void* d_in;
    CK_TRY(ck_to_device(ctx, bgr, (size_t)n * h * w * 3, in_space, ctx->in_stage, &d_in));
    const double* d_minv;
    CK_TRY(upload_minv(ctx, M, m_count, n, &d_minv));
    OutStage<uint8_t> o;
    CK_TRY(o.open(ctx, out, (size_t)n * dsize * dsize * 3, out_space, ctx->goban));
    CK_TRY(k_warp(ctx, (const uint8_t*)d_in, n, h, w, d_minv, m_count, dsize, o.dev));
    CK_TRY(o.deliver(ctx));
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_cnn_set_weights(ck_ctx* ctx, const float* const weights[12], int space)
{
    CK_API_BEGIN(ctx)
    if (!weights) return CK_ERR_ARG;
    for (int i = 0; i < 12; i++) if (!weights[i]) return ck_fail(ctx, CK_ERR_ARG, "weights[%d] is NULL", i);
    CK_TRY(k_cnn_pack_weights(ctx, weights, space));
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_cnn_set_mode(ck_ctx* ctx, int mode)
{
    CK_API_BEGIN(ctx)
    if (mode != CK_CNN_FP32 && mode != CK_CNN_BF16 && mode != CK_CNN_F16X2 && mode != CK_CNN_F16Q8) return ck_fail(ctx, CK_ERR_ARG, "unknown cnn mode %d", mode);
    ctx->cnn_mode = mode;
    return CK_OK;
    CK_API_END(ctx)
}

// where the classifier's answers of a call go (all optional): the softmax rows, labels and confidences per intersection
// and the region answers in `space`, the stones half of records in `rec_space`
struct CnnOut {
    float* y = nullptr;
    uint8_t* labels = nullptr;
    double* conf = nullptr;
    uint8_t* region_label = nullptr;
    double* region_conf = nullptr;
    int space = CK_HOST;
    ck_frame_record* rec = nullptr;
    int rec_space = CK_HOST;
};

// did the split-precision kernels of the last batch flag a value outside the fp16 range? (after a synchronisation)
static bool cnn_overflowed(const ck_ctx* ctx)
{
    return ck_cnn_split(ctx->cnn_mode) && ctx->cnn_flag.p && *(volatile int*)ctx->cnn_flag.p;
}

// one pass of the kernels of the context's mode, the answers queued for delivery; no synchronisation, no fallback
static int cnn_predict_dev(ck_ctx* ctx, const uint8_t* d_goban, int n, const CnnOut& o)
{
    if (!ctx->cnn.set) return ck_fail(ctx, CK_ERR_STATE, "ck_cnn_set_weights has not been called");
    CK_TRY(ck_ensure(ctx, ctx->ybuf, (size_t)n * 8100 * sizeof(float)));
    CK_TRY(ck_ensure(ctx, ctx->lblbuf, (size_t)n * 361));
    CK_TRY(ck_ensure(ctx, ctx->confbuf, (size_t)n * 361 * sizeof(double)));
    CK_TRY(ck_ensure(ctx, ctx->rlblbuf, (size_t)n * 100));
    CK_TRY(ck_ensure(ctx, ctx->rconfbuf, (size_t)n * 100 * sizeof(double)));
    int* d_flag = nullptr;
    if (ck_cnn_split(ctx->cnn_mode)) {
        // Safety net of the split-precision mode: an activation beyond the fp16 range (|x| > 65000; never seen with
        // 8-bit images and sane weights) would turn into inf.  The kernels raise a flag in host-mapped memory, which
        // cnn_run() looks at after the one synchronisation the call needs anyway.
        if (!ctx->cnn_flag.p) {
            CK_HIP(ctx, (hipError_t)ctx->cnn_flag.reserve(64, 64));
            CK_HIP(ctx, hipHostGetDevicePointer((void**)&ctx->cnn_flag_dev, ctx->cnn_flag.p, 0));
        }
        *(int*)ctx->cnn_flag.p = 0;
        d_flag = ctx->cnn_flag_dev;
    }
    CK_TRY(k_cnn_predict(ctx, d_goban, n, (float*)ctx->ybuf.p, (uint8_t*)ctx->lblbuf.p, (double*)ctx->confbuf.p, d_flag,
                         (uint8_t*)ctx->rlblbuf.p, (double*)ctx->rconfbuf.p));
    if (o.rec && o.rec_space == CK_DEVICE)
        CK_TRY(k_records_put_regions(ctx, (const uint8_t*)ctx->rlblbuf.p, (const double*)ctx->rconfbuf.p, n, o.rec));
    else if (o.rec) {            // records in host memory: both region arrays to pinned staging, scattered after the call's sync
        CK_TRY(ck_ensure_pinned(ctx, ctx->rec_host, (size_t)n * 900, 4096));
        CK_TRY(ck_from_device(ctx, ctx->rec_host.p, ctx->rconfbuf.p, (size_t)n * 800, CK_HOST));
        CK_TRY(ck_from_device(ctx, (uint8_t*)ctx->rec_host.p + (size_t)n * 800, ctx->rlblbuf.p, (size_t)n * 100, CK_HOST));
    }
    CK_TRY(ck_from_device(ctx, o.region_label, ctx->rlblbuf.p, (size_t)n * 100, o.space));
    CK_TRY(ck_from_device(ctx, o.region_conf, ctx->rconfbuf.p, (size_t)n * 100 * sizeof(double), o.space));
    CK_TRY(ck_from_device(ctx, o.y, ctx->ybuf.p, (size_t)n * 8100 * sizeof(float), o.space));
    CK_TRY(ck_from_device(ctx, o.labels, ctx->lblbuf.p, (size_t)n * 361, o.space));
    CK_TRY(ck_from_device(ctx, o.conf, ctx->confbuf.p, (size_t)n * 361 * sizeof(double), o.space));
    return CK_OK;
}

// the classifier on n goban images in HBM, complete on return: predict and synchronise; if the split-precision kernels
// flagged a value outside the fp16 range, the batch again with the f32 kernels (the images are still in place), delivered again
static int cnn_run(ck_ctx* ctx, const uint8_t* d_goban, int n, const CnnOut& o)
{
    CK_TRY(cnn_predict_dev(ctx, d_goban, n, o));
    CK_TRY(finish(ctx));
    if (!cnn_overflowed(ctx)) return CK_OK;
    const int mode = ctx->cnn_mode;
    ctx->cnn_mode = CK_CNN_FP32;
    const int rc = cnn_predict_dev(ctx, d_goban, n, o);
    ctx->cnn_mode = mode;
    ctx->cnn_fallbacks++;
    if (rc) return rc;
    return finish(ctx);
}

int ck_cnn_predict(ck_ctx* ctx, const uint8_t* goban, int n, int in_space,
                   float* y, uint8_t* labels, double* conf, int out_space)
{
    CK_API_BEGIN(ctx)
    if (!goban || n <= 0) return ck_fail(ctx, CK_ERR_ARG, "goban NULL or n <= 0");
    const void* d_in;
    CK_TRY(ck_to_device(ctx, goban, (size_t)n * 380 * 380 * 3, in_space, ctx->in_stage, &d_in));
    CnnOut o; o.y = y; o.labels = labels; o.conf = conf; o.space = out_space;
    return cnn_run(ctx, (const uint8_t*)d_in, n, o);
    CK_API_END(ctx)
}

int ck_cnn_maps(ck_ctx* ctx, const uint8_t* goban, int n, int in_space, float* pool2, float* pool4)
{
    CK_API_BEGIN(ctx)
    if (!goban || n <= 0 || n > 128) return ck_fail(ctx, CK_ERR_ARG, "goban NULL or n outside 1 .. 128");
    const void* d_in;
    CK_TRY(ck_to_device(ctx, goban, (size_t)n * 380 * 380 * 3, in_space, ctx->in_stage, &d_in));
    CK_TRY(cnn_predict_dev(ctx, (const uint8_t*)d_in, n, CnnOut()));     // (no cnn_run: these are the maps of this mode or none)
    CK_TRY(finish(ctx));
    if (cnn_overflowed(ctx))
        return ck_fail(ctx, CK_ERR_STATE, "an activation left the fp16 range: the maps of this batch are the f32 chain's (set CK_CNN_FP32)");
    // after one chunk the pooled conv2 output is still in act1 and the pooled conv4 output in act2 (k_cnn_predict)
    const size_t np = (size_t)n * 100;
    if (ctx->cnn_mode == CK_CNN_BF16) {
        // bf16 activations, conv4's channels padded to 96: widened on the host
        std::vector<uint16_t> raw;
        auto widen = [](uint16_t b) { uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f; };
        if (pool2) {
            raw.resize(np * 8192);
            CK_HIP(ctx, hipMemcpy(raw.data(), ctx->act1.p, raw.size() * 2, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < raw.size(); i++) pool2[i] = widen(raw[i]);
        }
        if (pool4) {
            raw.resize(np * 3456);
            CK_HIP(ctx, hipMemcpy(raw.data(), ctx->act2.p, raw.size() * 2, hipMemcpyDeviceToHost));
            for (size_t p = 0; p < np; p++)
                for (int px = 0; px < 36; px++)
                    for (int c = 0; c < 90; c++) pool4[(p * 36 + px) * 90 + c] = widen(raw[(p * 36 + px) * 96 + c]);
        }
        return CK_OK;
    }
    if (pool2) CK_HIP(ctx, hipMemcpy(pool2, ctx->act1.p, np * 8192 * sizeof(float), hipMemcpyDeviceToHost));
    if (pool4) CK_HIP(ctx, hipMemcpy(pool4, ctx->act2.p, np * 3240 * sizeof(float), hipMemcpyDeviceToHost));
    return CK_OK;
    CK_API_END(ctx)
}

int ck_stones_detect(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space,
                     const double* M, int m_count, uint8_t* labels, double* conf, int out_space)
{
    CK_API_BEGIN(ctx)
    CK_TRY(check_img(ctx, bgr, n, h, w));
    const void* d_in;
    CK_TRY(ck_to_device(ctx, bgr, (size_t)n * h * w * 3, in_space, ctx->in_stage, &d_in));
    const double* d_minv;
    CK_TRY(upload_minv(ctx, M, m_count, n, &d_minv));
    CK_TRY(ck_ensure(ctx, ctx->goban, (size_t)n * 380 * 380 * 3));
    CK_TRY(k_warp(ctx, (const uint8_t*)d_in, n, h, w, d_minv, m_count, 380, (uint8_t*)ctx->goban.p));
    CnnOut o; o.labels = labels; o.conf = conf; o.space = out_space;
    return cnn_run(ctx, (const uint8_t*)ctx->goban.p, n, o);
    CK_API_END(ctx)
}

int ck_cnn_regions(ck_ctx* ctx, const uint8_t* goban, int n, int in_space, uint8_t* region_label, double* region_conf,
                   int out_space)
{
    CK_API_BEGIN(ctx)
    if (!goban || n <= 0 || !region_label || !region_conf) return ck_fail(ctx, CK_ERR_ARG, "NULL argument or n <= 0");
    const void* d_in;
    CK_TRY(ck_to_device(ctx, goban, (size_t)n * 380 * 380 * 3, in_space, ctx->in_stage, &d_in));
    CnnOut o; o.region_label = region_label; o.region_conf = region_conf; o.space = out_space;
    return cnn_run(ctx, (const uint8_t*)d_in, n, o);
    CK_API_END(ctx)
}

int ck_cnn_regions_records(ck_ctx* ctx, const uint8_t* goban, int n, int in_space, ck_frame_record* rec, int rec_space)
{
    CK_API_BEGIN(ctx)
    if (!goban || n <= 0 || !rec) return ck_fail(ctx, CK_ERR_ARG, "NULL argument or n <= 0");
    if (rec_space != CK_HOST && rec_space != CK_DEVICE) return ck_fail(ctx, CK_ERR_ARG, "bad memory space %d", rec_space);
    const void* d_in;
    CK_TRY(ck_to_device(ctx, goban, (size_t)n * 380 * 380 * 3, in_space, ctx->in_stage, &d_in));
    CnnOut o; o.rec = rec; o.rec_space = rec_space;
    CK_TRY(cnn_run(ctx, (const uint8_t*)d_in, n, o));
    if (rec_space == CK_HOST) {
        const double* conf = (const double*)ctx->rec_host.p;
        const uint8_t* lab = (const uint8_t*)ctx->rec_host.p + (size_t)n * 800;
        for (int f = 0; f < n; f++) {
            memcpy(rec[f].region_conf, conf + (size_t)f * 100, 800);
            memcpy(rec[f].region_label, lab + (size_t)f * 100, 100);
        }
    }
    return CK_OK;
    CK_API_END(ctx)
}

int ck_board_detect_records(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space,
                            int hough_thresh, ck_frame_record* rec, int rec_space)
{
    CK_API_BEGIN(ctx)
    CK_TRY(check_img(ctx, bgr, n, h, w));
    if (!rec) return ck_fail(ctx, CK_ERR_ARG, "rec is NULL");
    if (rec_space != CK_HOST && rec_space != CK_DEVICE) return ck_fail(ctx, CK_ERR_ARG, "bad memory space %d", rec_space);
    // the board results are born on the host (K4's boxes, K6's peak order): n packed board halves in pinned memory,
    // then into the records -- a memcpy per record on the host, one upload + one small kernel for records in HBM
    const size_t part = offsetof(ck_frame_record, region_conf);
    const size_t lines_bytes = (size_t)n * CK_REC_LMAX * 2 * sizeof(float), res_bytes = (size_t)n * sizeof(ck_board_result);
    CK_TRY(ck_ensure_pinned(ctx, ctx->rec_host, (size_t)n * part + lines_bytes + res_bytes, 4096));
    uint8_t* parts = (uint8_t*)ctx->rec_host.p;
    float* lines = (float*)(parts + (size_t)n * part);
    ck_board_result* res = (ck_board_result*)((uint8_t*)lines + lines_bytes);
    CK_TRY(ck_board_detect(ctx, bgr, n, h, w, in_space, hough_thresh, lines, CK_REC_LMAX, res));
    for (int f = 0; f < n; f++) {
        ck_frame_record* r = (ck_frame_record*)(parts + (size_t)f * part);       // (only the head of it exists here)
        const int kept = res[f].n_lines < CK_REC_LMAX ? (res[f].n_lines < 0 ? 0 : res[f].n_lines) : CK_REC_LMAX;
        r->status = res[f].status; r->n_contours = res[f].n_contours; r->n_lines = res[f].n_lines;
        r->flags = res[f].n_lines > CK_REC_LMAX ? CK_REC_LINES_CUT : 0;
        r->biggest_area = res[f].biggest_area;
        memcpy(r->lines, lines + (size_t)f * CK_REC_LMAX * 2, (size_t)kept * 2 * sizeof(float));
        memset(&r->lines[kept][0], 0, (size_t)(CK_REC_LMAX - kept) * 2 * sizeof(float));
    }
    if (rec_space == CK_HOST) {
        for (int f = 0; f < n; f++) memcpy(&rec[f], parts + (size_t)f * part, part);
        return CK_OK;
    }
    CK_TRY(ck_ensure(ctx, ctx->rec_stage, (size_t)n * part));
    CK_HIP(ctx, hipMemcpyAsync(ctx->rec_stage.p, parts, (size_t)n * part, hipMemcpyHostToDevice, ctx->stream));
    CK_TRY(k_records_put_board(ctx, (const uint8_t*)ctx->rec_stage.p, n, rec));
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_stones_run(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space, const double* M, int m_count,
                  int mog2_handle, const double* learning_rates, uint8_t* region_label, double* region_conf,
                  int32_t* fgcount, uint8_t* labels, double* conf, int out_space)
{
    CK_API_BEGIN(ctx)
    CK_TRY(check_img(ctx, bgr, n, h, w));
    if (!region_label || !region_conf) return ck_fail(ctx, CK_ERR_ARG, "region outputs are NULL");
    const bool bg = mog2_handle >= 0;
    Mog2State* st = nullptr;
    if (bg) CK_TRY(mog2_of(ctx, mog2_handle, &st));
    if (bg && (!learning_rates || !fgcount)) return ck_fail(ctx, CK_ERR_ARG, "a background model needs learning_rates and fgcount");
    if (bg && (st->h != 380 || st->w != 380)) return ck_fail(ctx, CK_ERR_ARG, "the background model of a stones run is 380x380");
    const void* d_in;
    CK_TRY(ck_to_device(ctx, bgr, (size_t)n * h * w * 3, in_space, ctx->in_stage, &d_in));
    const double* d_minv;
    CK_TRY(upload_minv(ctx, M, m_count, n, &d_minv));
    CK_TRY(ck_ensure(ctx, ctx->goban, (size_t)n * 380 * 380 * 3));
    CK_TRY(k_warp(ctx, (const uint8_t*)d_in, n, h, w, d_minv, m_count, 380, (uint8_t*)ctx->goban.p));
    if (bg) {
        OutStage<int32_t> cnt;
        CK_TRY(cnt.open(ctx, fgcount, (size_t)n * 361 * sizeof(int32_t), out_space, ctx->fgcbuf));
        CK_TRY(k_mog2_run(ctx, *st, (const uint8_t*)ctx->goban.p, n, learning_rates, cnt.dev, nullptr, 379, 379));
        CK_TRY(cnt.deliver(ctx));
    }
    CnnOut o; o.region_label = region_label; o.region_conf = region_conf; o.labels = labels; o.conf = conf; o.space = out_space;
    return cnn_run(ctx, (const uint8_t*)ctx->goban.p, n, o);
    CK_API_END(ctx)
}

int ck_mog2_band_run(ck_ctx* ctx, int handle, const uint8_t* band, int n, int in_space, const double* learning_rates,
                     int last_band, int32_t* counts, int out_space)
{
    CK_API_BEGIN(ctx)
    Mog2State* stp;
    CK_TRY(mog2_of(ctx, handle, &stp));
    if (!band || !learning_rates || !counts || n <= 0) return ck_fail(ctx, CK_ERR_ARG, "NULL argument or n <= 0");
    Mog2State& st = *stp;
    const size_t zones = (size_t)((st.h + 19) / 20) * ((st.w + 19) / 20);
    const void* d_in;
    CK_TRY(ck_to_device(ctx, band, (size_t)n * st.h * st.w * 3, in_space, ctx->in_stage, &d_in));
    OutStage<int32_t> cnt;
    CK_TRY(cnt.open(ctx, counts, (size_t)n * zones * sizeof(int32_t), out_space, ctx->fgcbuf));
    CK_TRY(k_mog2_run(ctx, st, (const uint8_t*)d_in, n, learning_rates, cnt.dev, nullptr, last_band ? st.h - 1 : -1, st.w - 1));
    CK_TRY(cnt.deliver(ctx));
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_zone_counts(ck_ctx* ctx, const uint8_t* mask, int n, int in_space, int32_t* counts, int out_space)
{
    CK_API_BEGIN(ctx)
    if (!mask || !counts || n <= 0) return ck_fail(ctx, CK_ERR_ARG, "NULL argument or n <= 0");
    const void* d_in;
    CK_TRY(ck_to_device(ctx, mask, (size_t)n * 380 * 380, in_space, ctx->in_stage2, &d_in));
    OutStage<int32_t> cnt;
    CK_TRY(cnt.open(ctx, counts, (size_t)n * 361 * sizeof(int32_t), out_space, ctx->fgcbuf));
    CK_TRY(k_zone_counts(ctx, (const uint8_t*)d_in, n, 380, cnt.dev));
    CK_TRY(cnt.deliver(ctx));
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_contour_stones(ck_ctx* ctx, const uint8_t* goban, const uint8_t* fg, int n, int side, int in_space, const int32_t* rects,
                      int rs, int re, int cs, int ce, uint8_t* stones, int16_t* zones, uint8_t* mask)
{
    CK_API_BEGIN(ctx)
    if (!goban || !fg || !rects || !stones || n <= 0) return ck_fail(ctx, CK_ERR_ARG, "NULL argument or n <= 0");
    if (side < 19 * 4 || side > 4096) return ck_fail(ctx, CK_ERR_ARG, "goban image side %d", side);
    if (rs < 0 || cs < 0 || re > 19 || ce > 19 || re <= rs || ce <= cs)
        return ck_fail(ctx, CK_ERR_ARG, "intersection range rows [%d, %d) columns [%d, %d)", rs, re, cs, ce);
    const size_t px = (size_t)n * side * side;
    const void *d_img, *d_fg;
    CK_TRY(ck_to_device(ctx, goban, px * 3, in_space, ctx->in_stage, &d_img));
    CK_TRY(ck_to_device(ctx, fg, px, in_space, ctx->in_stage2, &d_fg));
    CK_TRY(k_contour_stones(ctx, (const uint8_t*)d_img, (const uint8_t*)d_fg, n, side, rects, rs, re, cs, ce, stones, zones, mask));
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_cluster_stones(ck_ctx* ctx, const void* goban, int n, int side, int is_f32, int in_space, const int32_t* rects,
                      const uint8_t* mask, const int32_t* jobs, int m, uint8_t* stones, uint8_t* trusted, uint8_t* ratios,
                      float* centers, uint8_t* labels, long long labels_cap, int32_t* passes, double* compactness, int32_t* winner)
{
    CK_API_BEGIN(ctx)
    if (!goban || !rects || !mask || !jobs || !stones || !trusted || n <= 0 || m <= 0)
        return ck_fail(ctx, CK_ERR_ARG, "NULL argument, n <= 0 or no job");
    if (side < 19 * 4 || side > 4096) return ck_fail(ctx, CK_ERR_ARG, "goban image side %d", side);
    const void* d_img;
    CK_TRY(ck_to_device(ctx, goban, (size_t)n * side * side * 3 * (is_f32 ? 4 : 1), in_space, ctx->in_stage, &d_img));
    CK_TRY(k_cluster_stones(ctx, d_img, n, side, is_f32 != 0, rects, mask, jobs, m, stones, trusted, ratios, centers, labels,
                            labels_cap, passes, compactness, winner));
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_rng_get(ck_ctx* ctx, uint64_t* state)
{
    CK_API_BEGIN(ctx)
    if (!state) return ck_fail(ctx, CK_ERR_ARG, "state is NULL");
    *state = ctx->rng_state;
    return CK_OK;
    CK_API_END(ctx)
}

int ck_rng_set(ck_ctx* ctx, uint64_t state)
{
    CK_API_BEGIN(ctx)
    ctx->rng_state = state;
    return CK_OK;
    CK_API_END(ctx)
}

int ck_contours_external(ck_ctx* ctx, const uint8_t* edges, int n, int h, int w, int in_space,
                         int32_t* counts, int32_t* table, int table_cap, int32_t* points, int points_cap)
{
    CK_API_BEGIN(ctx)
    CK_TRY(check_img(ctx, edges, n, h, w));
    if (!counts || !table || table_cap <= 0) return ck_fail(ctx, CK_ERR_ARG, "NULL table");
    const void* d_in;
    CK_TRY(ck_to_device(ctx, edges, (size_t)n * h * w, in_space, ctx->in_stage, &d_in));
    std::vector<std::vector<CkContour>> found;
    CK_TRY(k_contour_survey(ctx, (const uint8_t*)d_in, n, h, w, found));
    size_t nt = 0, np = 0;
    for (int f = 0; f < n; f++) {
        counts[f] = (int32_t)found[f].size();
        for (const CkContour& c : found[f]) {
            if ((int)nt >= table_cap) return ck_fail(ctx, CK_ERR_CAPACITY, "more than %d contours in the batch", table_cap);
            int32_t* t = table + nt * 4;
            t[0] = c.root % w; t[1] = c.root / w; t[2] = c.nvert; t[3] = (int32_t)(c.pts.size() / 2);
            nt++;
            if (points) {
                if (np + c.pts.size() / 2 > (size_t)points_cap) return ck_fail(ctx, CK_ERR_CAPACITY, "more than %d border pixels in the batch", points_cap);
                memcpy(points + np * 2, c.pts.data(), c.pts.size() * 4);
                np += c.pts.size() / 2;
            }
        }
    }
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_find_intersections(ck_ctx* ctx, const uint8_t* goban, int n, int side, int in_space, const int16_t* mtx, const int32_t* rects,
                          int16_t* grid, int16_t* lines, int32_t* nlines, uint8_t* edges)
{
    CK_API_BEGIN(ctx)
    if (!goban || !mtx || !rects || !grid || n <= 0) return ck_fail(ctx, CK_ERR_ARG, "NULL argument or n <= 0");
    if (side < 19 * 4 || side > 4096) return ck_fail(ctx, CK_ERR_ARG, "goban image side %d", side);
    const void* d_img;
    CK_TRY(ck_to_device(ctx, goban, (size_t)n * side * side * 3, in_space, ctx->in_stage, &d_img));
    const int16_t* found;
    const int32_t* counts;
    CK_TRY(k_grid_lines(ctx, (const uint8_t*)d_img, n, side, rects, &found, &counts, edges));
    if (lines) memcpy(lines, found, (size_t)n * 361 * CK_ZONE_LINES * 4 * sizeof(int16_t));
    if (nlines) memcpy(nlines, counts, (size_t)n * 361 * sizeof(int32_t));
    // update_grid, zone by zone; images are independent: a few host threads share them
    auto one_image = [&](int f) {
        int32_t seg[CK_ZONE_LINES * 4];
        int16_t* g = grid + (size_t)f * 361 * 2;
        memcpy(g, mtx, 361 * 2 * sizeof(int16_t));
        for (int z = 0; z < 361; z++) {
            const int k = counts[(size_t)f * 361 + z];
            if (!k) continue;
            const int16_t* l = found + ((size_t)f * 361 + z) * CK_ZONE_LINES * 4;
            for (int i = 0; i < k * 4; i++) seg[i] = l[i];
            ck_update_grid_host(seg, k, rects + 4 * z, g + 2 * z);
        }
    };
    ck_parallel_for(n, 8, one_image);
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_update_grid(const int32_t* lines, int k, const int32_t* box, int16_t* slot)
{
    if (!lines || !box || !slot || k < 0) return CK_ERR_ARG;
    for (int i = 0; i < k; i++)
        if (lines[4 * i] == lines[4 * i + 2] && lines[4 * i + 1] == lines[4 * i + 3]) return CK_ERR_ARG;   // zero length: the reference divides by zero
    ck_update_grid_host(lines, k, box, slot);
    return CK_OK;
}

int ck_mog2_create(ck_ctx* ctx, int h, int w, int* handle)
{
    CK_API_BEGIN(ctx)
    if (!handle || h <= 0 || w <= 0) return CK_ERR_ARG;
    const int idx = free_slot(ctx->mog2);
    Mog2State& st = ctx->mog2[idx];
    st.h = h; st.w = w; st.nframes = 0; st.alive = true;
    const size_t npx = (size_t)h * w;
    CK_TRY(ck_ensure(ctx, st.weight, npx * 5 * sizeof(float)));
    CK_TRY(ck_ensure(ctx, st.variance, npx * 5 * sizeof(float)));
    CK_TRY(ck_ensure(ctx, st.mean, npx * 15 * sizeof(float)));
    CK_TRY(ck_ensure(ctx, st.nmodes, npx));
    CK_HIP(ctx, hipMemsetAsync(st.nmodes.p, 0, npx, ctx->stream));
    *handle = idx;
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_mog2_apply(ck_ctx* ctx, int handle, const uint8_t* img3, int in_space,
                  double learning_rate, uint8_t* fgmask, int out_space)
{
    CK_API_BEGIN(ctx)
    Mog2State* stp;
    CK_TRY(mog2_of(ctx, handle, &stp));
    if (!img3 || !fgmask) return ck_fail(ctx, CK_ERR_ARG, "NULL image or mask");
    Mog2State& st = *stp;
    const size_t npx = (size_t)st.h * st.w;
    const void* d_in;
    CK_TRY(ck_to_device(ctx, img3, npx * 3, in_space, ctx->in_stage, &d_in));
    OutStage<uint8_t> fg;
    CK_TRY(fg.open(ctx, fgmask, npx, out_space, ctx->out_stage));
    CK_TRY(k_mog2_apply(ctx, st, (const uint8_t*)d_in, learning_rate, fg.dev));
    CK_TRY(fg.deliver(ctx));
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_mog2_get_state(ck_ctx* ctx, int handle, float* weight, float* variance, float* mean, uint8_t* nmodes)
{
    CK_API_BEGIN(ctx)
    Mog2State* stp;
    CK_TRY(mog2_of(ctx, handle, &stp));
    const Mog2State& st = *stp;
    const size_t npx = (size_t)st.h * st.w;
    CK_TRY(ck_from_device(ctx, weight, st.weight.p, npx * 5 * sizeof(float), CK_HOST));
    CK_TRY(ck_from_device(ctx, variance, st.variance.p, npx * 5 * sizeof(float), CK_HOST));
    CK_TRY(ck_from_device(ctx, mean, st.mean.p, npx * 15 * sizeof(float), CK_HOST));
    CK_TRY(ck_from_device(ctx, nmodes, st.nmodes.p, npx, CK_HOST));
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_mog2_destroy(ck_ctx* ctx, int handle)
{
    CK_API_BEGIN(ctx)
    if (handle < 0 || handle >= (int)ctx->mog2.size()) return CK_ERR_ARG;
    ctx->mog2[handle].alive = false;
    return CK_OK;
    CK_API_END(ctx)
}

// ---- training of the stone classifier (k_cnn_train.hip) -----------------------------------------------------------------

int ck_train_create(ck_ctx* ctx, const float* const weights[12], int space, int* handle)
{
    CK_API_BEGIN(ctx)
    if (!weights || !handle) return CK_ERR_ARG;
    for (int i = 0; i < 12; i++) if (!weights[i]) return ck_fail(ctx, CK_ERR_ARG, "weights[%d] is NULL", i);
    const int idx = free_slot(ctx->trainers);
    CK_TRY(k_train_create(ctx, ctx->trainers[idx], weights, space));
    *handle = idx;
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_train_destroy(ck_ctx* ctx, int handle)
{
    CK_API_BEGIN(ctx)
    CkTrainer* tr;
    CK_TRY(trainer_of(ctx, handle, &tr));
    CK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *tr = CkTrainer();                              // dead, and its buffers freed
    return CK_OK;
    CK_API_END(ctx)
}

// checks, staging and the gradient pass shared by ck_train_step and ck_train_grads: leaves the gradients in tr->g and
// the mean loss in *loss
static int train_pass(ck_ctx* ctx, int handle, const uint8_t* x, const uint8_t* labels, int n, int h, int w, int c, int in_space,
                      int dropout, uint64_t seed, long long step, bool want_masks, float* loss, CkTrainer** out)
{
    CkTrainer* tr;
    CK_TRY(trainer_of(ctx, handle, &tr));
    if (!x || !labels) return ck_fail(ctx, CK_ERR_ARG, "patches or labels NULL");
    if (n < 1 || h != 40 || w != 40 || c != 3)
        return ck_fail(ctx, CK_ERR_ARG, "patches of shape %d x %d x %d x %d: expected n x 40 x 40 x 3 with n >= 1", n, h, w, c);
    for (int i = 0; i < n; i++)
        if (labels[i] > 80) return ck_fail(ctx, CK_ERR_ARG, "label %d of patch %d: a class index is 0 .. 80", (int)labels[i], i);
    const void* d_x;
    CK_TRY(ck_to_device(ctx, x, (size_t)n * 4800, in_space, ctx->in_stage, &d_x));
    CK_TRY(ck_ensure(ctx, tr->lab, (size_t)n));
    CK_HIP(ctx, hipMemcpyAsync(tr->lab.p, labels, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    CK_TRY(k_train_grads(ctx, *tr, (const uint8_t*)d_x, (const uint8_t*)tr->lab.p, n, dropout ? 1 : 0, seed,
                         (uint64_t)(step < 0 ? tr->steps : step), want_masks));
    std::vector<float> per(n);
    CK_HIP(ctx, hipMemcpyAsync(per.data(), tr->lossv.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    CK_TRY(finish(ctx));
    double sum = 0;                              // the mean over the batch, summed in patch order
    for (int i = 0; i < n; i++) sum += per[i];
    if (loss) *loss = (float)(sum / n);
    *out = tr;
    return CK_OK;
}

int ck_train_step(ck_ctx* ctx, int handle, const uint8_t* x, const uint8_t* labels, int n, int h, int w, int c, int in_space,
                  double lr, int dropout, uint64_t seed, float* loss)
{
    CK_API_BEGIN(ctx)
    CkTrainer* tr;
    CK_TRY(train_pass(ctx, handle, x, labels, n, h, w, c, in_space, dropout, seed, -1, false, loss, &tr));
    CK_TRY(k_train_adam(ctx, *tr, (const float*)tr->g.p, lr));
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_train_grads(ck_ctx* ctx, int handle, const uint8_t* x, const uint8_t* labels, int n, int h, int w, int c, int in_space,
                   int dropout, uint64_t seed, long long step, float* loss, float* const grads[12],
                   uint8_t* mask1, uint8_t* mask2, uint8_t* mask3)
{
    CK_API_BEGIN(ctx)
    CkTrainer* tr;
    const bool masks = dropout && (mask1 || mask2 || mask3);
    CK_TRY(train_pass(ctx, handle, x, labels, n, h, w, c, in_space, dropout, seed, step, masks, loss, &tr));
    if (grads)
        for (int i = 0; i < 12; i++)
            CK_TRY(ck_from_device(ctx, grads[i], (const float*)tr->g.p + ck_cnn_offset(i), CK_CNN_COUNTS[i] * sizeof(float), CK_HOST));
    if (masks) {
        CK_TRY(ck_from_device(ctx, mask1, tr->mask1.p, (size_t)n * 8192, CK_HOST));
        CK_TRY(ck_from_device(ctx, mask2, tr->mask2.p, (size_t)n * 3240, CK_HOST));
        CK_TRY(ck_from_device(ctx, mask3, tr->mask3.p, (size_t)n * 160, CK_HOST));
    }
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_train_apply(ck_ctx* ctx, int handle, const float* const grads[12], double lr)
{
    CK_API_BEGIN(ctx)
    CkTrainer* tr;
    CK_TRY(trainer_of(ctx, handle, &tr));
    if (!grads) return ck_fail(ctx, CK_ERR_ARG, "grads is NULL");
    for (int i = 0; i < 12; i++) if (!grads[i]) return ck_fail(ctx, CK_ERR_ARG, "grads[%d] is NULL", i);
    for (int i = 0; i < 12; i++)
        CK_HIP(ctx, hipMemcpyAsync((float*)tr->g.p + ck_cnn_offset(i), grads[i], CK_CNN_COUNTS[i] * sizeof(float),
                                   hipMemcpyHostToDevice, ctx->stream));
    CK_TRY(k_train_adam(ctx, *tr, (const float*)tr->g.p, lr));
    return finish(ctx);
    CK_API_END(ctx)
}

static int train_get(ck_ctx* ctx, const DevBuf& src, float* const dst[12])
{
    if (!dst) return CK_OK;
    for (int i = 0; i < 12; i++)
        CK_TRY(ck_from_device(ctx, dst[i], (const float*)src.p + ck_cnn_offset(i), CK_CNN_COUNTS[i] * sizeof(float), CK_HOST));
    return CK_OK;
}

int ck_train_get_weights(ck_ctx* ctx, int handle, float* const weights[12])
{
    CK_API_BEGIN(ctx)
    CkTrainer* tr;
    CK_TRY(trainer_of(ctx, handle, &tr));
    CK_TRY(train_get(ctx, tr->w, weights));
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_train_get_adam_state(ck_ctx* ctx, int handle, float* const m[12], float* const v[12], long long* steps)
{
    CK_API_BEGIN(ctx)
    CkTrainer* tr;
    CK_TRY(trainer_of(ctx, handle, &tr));
    CK_TRY(train_get(ctx, tr->m, m));
    CK_TRY(train_get(ctx, tr->v, v));
    if (steps) *steps = tr->steps;
    return finish(ctx);
    CK_API_END(ctx)
}

int ck_train_handover(ck_ctx* ctx, int handle)
{
    CK_API_BEGIN(ctx)
    CkTrainer* tr;
    CK_TRY(trainer_of(ctx, handle, &tr));
    CK_TRY(finish(ctx));
    const float* w[12];
    for (int i = 0; i < 12; i++) w[i] = (const float*)tr->w.p + ck_cnn_offset(i);
    return ck_cnn_set_weights(ctx, w, CK_DEVICE);
    CK_API_END(ctx)
}

// ---- labelled patches from goban images (k_harvest.hip) ------------------------------------------------------------------
int ck_harvest_patches(ck_ctx* ctx, const uint8_t* goban, int n, int in_space, const int32_t* fgcount, int fg_space,
                       const int32_t* state_of, const uint8_t* positions, int n_pos, int calm_max, int empty_keep, uint32_t seed,
                       long long first_frame, uint8_t* x, uint8_t* labels, int32_t* src, int cap, int out_space, int32_t* n_found)
{
    CK_API_BEGIN(ctx)
    if (!n_found) return ck_fail(ctx, CK_ERR_ARG, "n_found is NULL");
    *n_found = 0;
    if (n < 0 || n > (1 << 20)) return ck_fail(ctx, CK_ERR_ARG, "n = %d: 0 .. 2^20 frames per call", n);
    if (cap < 0) return ck_fail(ctx, CK_ERR_ARG, "cap = %d is negative", cap);
    if (empty_keep < 0 || empty_keep > 256) return ck_fail(ctx, CK_ERR_ARG, "empty_keep = %d: 0 .. 256", empty_keep);
    if (n_pos < 0 || (n_pos > 0 && !positions)) return ck_fail(ctx, CK_ERR_ARG, "positions NULL or n_pos < 0");
    if (n == 0) return CK_OK;
    if (!goban || !fgcount || !state_of) return ck_fail(ctx, CK_ERR_ARG, "goban, fgcount or state_of is NULL");
    if (cap > 0 && (!x || !labels || !src)) return ck_fail(ctx, CK_ERR_ARG, "x, labels or src is NULL with cap > 0");
    if ((in_space != CK_HOST && in_space != CK_DEVICE) || (fg_space != CK_HOST && fg_space != CK_DEVICE))
        return ck_fail(ctx, CK_ERR_ARG, "bad memory space %d / %d", in_space, fg_space);
    for (int i = 0; i < n; i++)
        if (state_of[i] >= n_pos) return ck_fail(ctx, CK_ERR_ARG, "state_of[%d] = %d with %d positions", i, state_of[i], n_pos);
    for (size_t i = 0; i < (size_t)n_pos * 361; i++)
        if (positions[i] > 2)
            return ck_fail(ctx, CK_ERR_ARG, "position %d holds code %d at point %d: 0 empty, 1 black, 2 white", (int)(i / 361),
                           (int)positions[i], (int)(i % 361));
    if (in_space == CK_DEVICE && ((uintptr_t)goban & 3) != 0)
        return ck_fail(ctx, CK_ERR_ARG, "goban images in device memory must be 4-byte aligned");
    if (out_space != CK_HOST && cap > 0 && (((uintptr_t)x & 7) != 0 || ((uintptr_t)src & 3) != 0))
        return ck_fail(ctx, CK_ERR_ARG, "x in device memory must be 8-byte aligned, src 4-byte aligned");
    // one scratch block: state_of | positions | codes of the n * 100 candidates | block totals + the grand total
    const int nb = ck_harvest_blocks(n);
    const CkHarvestLayout L = ck_harvest_layout(n, n_pos, nb);
    CK_TRY(ck_ensure(ctx, ctx->harvest, L.total));
    uint8_t* scratch = (uint8_t*)ctx->harvest.p;
    CK_HIP(ctx, hipMemcpyAsync(scratch + L.state, state_of, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    if (n_pos > 0)
        CK_HIP(ctx, hipMemcpyAsync(scratch + L.pos, positions, (size_t)n_pos * 361, hipMemcpyHostToDevice, ctx->stream));
    const void *d_goban, *d_fg;
    CK_TRY(ck_to_device(ctx, goban, (size_t)n * 380 * 380 * 3, in_space, ctx->in_stage, &d_goban));
    CK_TRY(ck_to_device(ctx, fgcount, (size_t)n * 361 * sizeof(int32_t), fg_space, ctx->in_stage2, &d_fg));
    OutStage<uint8_t> ox, ol;
    OutStage<int32_t> os;
    if (cap > 0) {
        CK_TRY(ox.open(ctx, x, (size_t)cap * 4800, out_space, ctx->out_stage));
        CK_TRY(ol.open(ctx, labels, (size_t)cap, out_space, ctx->lblbuf));
        CK_TRY(os.open(ctx, src, (size_t)cap * 2 * sizeof(int32_t), out_space, ctx->harvest_src));
    }
    int32_t* d_blocks = (int32_t*)(scratch + L.blocks);
    CK_TRY(k_harvest(ctx, (const uint8_t*)d_goban, (const int32_t*)d_fg, (const int32_t*)(scratch + L.state), scratch + L.pos, n, calm_max,
                     empty_keep, seed, (uint32_t)(unsigned long long)first_frame, (int32_t*)(scratch + L.code), d_blocks,
                     ox.dev, ol.dev, os.dev, cap));
    int32_t total = 0;
    CK_HIP(ctx, hipMemcpyAsync(&total, d_blocks + nb, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    CK_TRY(finish(ctx));
    *n_found = total;
    // only what was found travels home: the rows beyond min(total, cap) of a host output stay as the caller left them
    const size_t got = (size_t)(total < cap ? total : cap);
    if (got > 0 && out_space == CK_HOST) {
        CK_TRY(ck_from_device(ctx, x, ox.dev, got * 4800, CK_HOST));
        CK_TRY(ck_from_device(ctx, labels, ol.dev, got, CK_HOST));
        CK_TRY(ck_from_device(ctx, src, os.dev, got * 2 * sizeof(int32_t), CK_HOST));
        CK_TRY(finish(ctx));
    }
    return CK_OK;
    CK_API_END(ctx)
}

int ck_augment_patches(ck_ctx* ctx, const uint8_t* x, int n, int in_space, const uint8_t* t, uint8_t* x_out, int out_space)
{
    CK_API_BEGIN(ctx)
    if (n < 0 || n > (1 << 24)) return ck_fail(ctx, CK_ERR_ARG, "n = %d: 0 .. 2^24 patches per call", n);
    if (n == 0) return CK_OK;
    if (!x || !t || !x_out) return ck_fail(ctx, CK_ERR_ARG, "x, t or x_out is NULL");
    for (int i = 0; i < n; i++)
        if (t[i] > 7) return ck_fail(ctx, CK_ERR_ARG, "t[%d] = %d: a transform code is 0 .. 7", i, (int)t[i]);
    const size_t bytes = (size_t)n * 4800;
    if ((in_space == CK_HOST) == (out_space == CK_HOST) && x < x_out + bytes && x_out < x + bytes)
        return ck_fail(ctx, CK_ERR_ARG, "x_out overlaps x: the transform does not work in place");
    if ((in_space != CK_HOST && ((uintptr_t)x & 3) != 0) || (out_space != CK_HOST && ((uintptr_t)x_out & 3) != 0))
        return ck_fail(ctx, CK_ERR_ARG, "patches in device memory must be 4-byte aligned");
    CK_TRY(ck_ensure(ctx, ctx->harvest, (size_t)n));
    CK_HIP(ctx, hipMemcpyAsync(ctx->harvest.p, t, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    const void* d_x;
    CK_TRY(ck_to_device(ctx, x, bytes, in_space, ctx->in_stage, &d_x));
    OutStage<uint8_t> out;
    CK_TRY(out.open(ctx, x_out, bytes, out_space, ctx->out_stage));
    CK_TRY(k_augment(ctx, (const uint8_t*)d_x, (const uint8_t*)ctx->harvest.p, n, out.dev));
    CK_TRY(out.deliver(ctx));
    return finish(ctx);
    CK_API_END(ctx)
}

}  // extern "C"
