// ck_common.h -- internal declarations shared by the HIP translation units of libck_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <exception>
#include <map>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/camkifu_amd.h"
#include "ck_buf.h"        // DevBuf, PinBuf: buffers that free themselves
#include "ck_cnn_pack.h"   // the classifier's weight arrays and their packs (host only)
#include "ck_jpeg_enc_stage.h"   // CkEncGeom: the steps of the encoder's Huffman stage (plain C++)
#include "ck_png_stage.h"        // CkPngGeom: the steps of the PNG encoder (plain C++)

// the context's stream, destroyed with it
struct CkStream {
    hipStream_t s = nullptr;
    CkStream() = default;
    CkStream(const CkStream&) = delete;
    CkStream& operator=(const CkStream&) = delete;
    ~CkStream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};

struct TimingSlot {
    double ms = 0;
    int launches = 0;
};

struct PendingEvent {
    hipEvent_t a, b;
    std::string name;
};

struct Mog2State {
    int h = 0, w = 0, nframes = 0;
    DevBuf weight, variance, mean, nmodes;
    bool alive = false;
    // learning rates of an ordered run: the model's own pinned staging + device copy (k_mog2_run)
    PinBuf rates_host;
    DevBuf rates_dev;
    hipEvent_t rates_done = nullptr;     // (events stay plain handles: ~ck_ctx destroys them)
    bool rates_busy = false;
};

// A trainer of the stone classifier (k_cnn_train.hip): master weights, the last gradients and both Adam moments as flat f32
// arrays in weight order (c1w c1b .. d2w d2b, CK_TRAIN_PARAMS floats; array i at ck_cnn_offset(i)), what one chunk keeps between forward and backward,
// the partial sums of the weight gradients, and the number of Adam updates applied so far.
#define CK_TRAIN_PARAMS 658665
static_assert(ck_cnn_offset(12) == CK_TRAIN_PARAMS, "the twelve arrays of ck_cnn_pack.h end to end");
#define CK_TRAIN_CHUNK 256
struct CkTrainer {
    bool alive = false;
    long long steps = 0;
    DevBuf w, g, m, v;
    DevBuf lab, a1, a2, p1, a3, a4, p2, h1, lg, dlg, dh1, dp2, dz4, dz3, dp1, dz2, dz1, part, lossv, mask1, mask2, mask3;
};

// the modes that carry f32 operands as split fp16 (and share the overflow flag and the f32 fallback)
static inline bool ck_cnn_split(int mode) { return mode == CK_CNN_F16X2 || mode == CK_CNN_F16Q8; }

// every buffer is a member of CnnPacks (ck_cnn_pack.h) under the same name: packed on the host, uploaded by k_cnn_pack_weights
struct CnnWeights {
    bool set = false;
    // repacked fp32 (correlation layout, [kh][kw][cin][cout] with the flip applied)
    DevBuf c1w, c1b, c2w, c2b, c3w, c3b, c4w, c4b, d1w, d1b, d2w, d2b;
    // bf16 packs for the MFMA path
    DevBuf c2w_bf, c3w_bf, c4w_bf;
    DevBuf c1w_f16;      // conv1 for the fused bf16 kernels: fp16 fragments (k_cnn_bf16.hip)
    DevBuf d1w_bfp;      // dense 1 for fc1_bf16_kernel: bf16 fragments over the padded maps
    // hi / lo fp16 planes for the split-precision mode
    DevBuf c1w_h2, c2w_h2, c3w_h2, c4w_h2, d1w_h2;
    // CK_CNN_F16Q8 (k_cnn_q8.hip): conv1 as fp16 fragments of both planes, the cross-term weights of conv2 .. conv4 as e4m3
    DevBuf c1w_q8, c2x_q8, c3x_q8, c4x_q8;
    bool q8_ok = false;  // every weight inside the e4m3 range of its block scale (else the mode runs the three-MFMA kernels)
};

// Members are destroyed last to first: the stream is declared before every buffer, so it outlives them all.
struct ck_ctx {
    // One thread at a time (include/camkifu_amd.h): `owner` is the token of the thread inside an entry point, 0 when
    // nobody is; a second thread gets CK_ERR_STATE instead of a silent race on the stream and the scratch buffers.
    std::atomic<unsigned long long> owner{0};
    int depth = 0;                   // entry points calling entry points on the owner's thread
    int device = 0;
    CkStream stream;
    std::string err;
    bool timing = false;
    std::map<std::string, TimingSlot> slots;
    std::vector<PendingEvent> pending;
    std::vector<hipEvent_t> event_pool;
    hipEvent_t handover = nullptr;   // ck_stream_wait: recorded on the host framework's stream, waited for on ours
    // pinned host memory: two arenas (the contour survey has the second, so that a caller's data in the first survives),
    // and the staging of per-frame result records (ck_board_detect_records / ck_cnn_regions_records): one half of n records
    PinBuf host_pinned, host_pinned2, rec_host;
    PinBuf cnn_flag{CK_PIN_MAPPED};  // host-mapped flag: the split-precision kernels met a value outside the fp16 range

    // scratch (grown on demand, never shrunk)
    DevBuf in_stage;     // staged host input
    DevBuf in_stage2;
    DevBuf planes;       // median output, planar n*3*h*pitch
    DevBuf trange;       // value bounds of the median's tiles (ck_range_bytes)
    DevBuf edges;        // n*h*w
    DevBuf map;          // n*h*w NMS map
    DevBuf labels;       // n*h*w int32 union-find parents
    DevBuf labels2;
    DevBuf runs;         // run-table labelling: bit map, rank prefix, row bases, run parents
    DevBuf ghost;        // n*h*w
    DevBuf misc;         // small per-frame counters
    DevBuf bflag;        // per frame: did Canny put an edge pixel on the image frame? (K2 -> K3 label reuse)
    DevBuf comp;         // per-frame component tables
    DevBuf lists;        // per-frame edge / border pixel lists
    DevBuf pts;          // compacted border points
    DevBuf accum;        // hough accumulators
    DevBuf peaks;
    DevBuf goban;        // n*380*380*3
    DevBuf act0, act1, act2;   // cnn activations
    DevBuf ybuf, lblbuf, confbuf, rlblbuf, rconfbuf, fgcbuf;
    DevBuf out_stage;
    DevBuf mats;
    DevBuf pyr0, pyr1;   // pyramid levels between the first and the last (ping-pong)
    DevBuf rec_stage;    // the device twin of rec_host, for records that live in HBM
    DevBuf harvest;      // ck_harvest_patches / ck_augment_patches: the small host inputs, the flags' codes, the block totals
    DevBuf harvest_src;  // staged (frame, region) pairs of a harvest that goes to the host
    DevBuf jenc_work;    // the encoder's Huffman stage on the device: sizes and offsets of a pass (CkEncWork),
    DevBuf jenc_bits;    // its unstuffed bits and the FF counts of their byte tiles,
    DevBuf jenc_pack;    // and its streams, one behind the other
    DevBuf jspan;        // CK_JPEG_ENTROPY_DEVICE_SPANS: candidates, entries and flags of a pass (k_jpeg_span.hip)
    DevBuf png_work;     // the PNG encoder: filtered rows, counters, codes, sizes and offsets of a pass (CkPngWork),
    DevBuf png_pack;     // and its zlib streams, one behind the other
    DevBuf png_inf;      // ck_png_inflate_device: jobs, records and streams of a call (ck_png_decode keeps them in in_stage)

    CnnWeights cnn;
    int* cnn_flag_dev = nullptr;     // cnn_flag as the device sees it
    int cnn_fallbacks = 0;           // batches the split-precision mode handed back to the f32 kernels
    int cnn_mode = CK_CNN_F16X2;     // f32-accurate and 2.3x faster than the k-ordered f32 chain (CK_CNN_FP32)
    std::vector<Mog2State> mog2;
    std::vector<CkTrainer> trainers;
    int jpeg_bad_frame = -1;         // ck_jpeg_decode: the frame its last CK_ERR_DATA is about (-1: none)
    long long jpeg_uploaded = 0;     // bytes the last ck_jpeg_decode / ck_jpeg_coefficients_device copied to the device
    int jpeg_entropy = CK_JPEG_ENTROPY_HOST;   // where ck_jpeg_decode runs the Huffman stage (ck_jpeg_set_entropy)
    int jpeg_span_bytes = 512;       // S of CK_JPEG_ENTROPY_DEVICE_SPANS (CK_SPAN_DEFAULT; ck_jpeg_set_span_bytes)
    long long jpeg_span_stats[4] = {0, 0, 0, 0};   // of the last decode in that mode (ck_jpeg_span_stats)
    int jpeg_enc_entropy = CK_JPEG_ENTROPY_HOST;   // where ck_jpeg_encode runs the Huffman stage (ck_jpeg_set_encode_entropy)
    int jpeg_enc_tables = CK_JPEG_TABLES_STANDARD;   // the Huffman tables ck_jpeg_encode writes (ck_jpeg_set_encode_tables)
    size_t jenc_freq_at = 0;         // where the last optimised pass left its counters in jenc_work, and of how many frames
    int jenc_freq_frames = 0;        // (0: the last pass was a standard one) -- ck_jpeg_encode_histograms
    long long jpeg_downloaded = 0;   // bytes the last ck_jpeg_encode / ck_jpeg_entropy_encode_device copied from the device
    int png_matches = CK_PNG_MATCH_NONE;   // what ck_png_encode makes of repeated bytes (ck_png_set_encode_matches)
    std::vector<long long> png_tokens;     // ck_png_run_stats: literal and match tokens of the frames of the last ck_png_encode,
    size_t png_count_at = 0;               // as far as their histograms have been read; those of its last pass are still in
    int png_count_frames = 0, png_count_runs = 0;   // png_work, at png_count_at, of so many frames, in this mode
    long long png_count_bands = 0;         // (bands of a frame)
    int png_inflate = CK_PNG_INFLATE_HOST;  // where ck_png_decode inflates (ck_png_set_inflate)
    long long png_uploaded = 0;            // ck_png_uploaded_bytes: of the last ck_png_decode
    long long png_inf_stats[4] = {0, 0, 0, 0};   // ck_png_inflate_stats
    uint64_t rng_state = 0xffffffffULL;   // cv::RNG of the stones thread (theRNG()): ck_cluster_stones draws from it

    ~ck_ctx();           // the events; every buffer frees itself, then the stream goes (ck_api.hip)
};

// Every scratch DevBuf of a context, once.  Scratch carries nothing from one entry-point call to the next, so
// ck_debug_scratch_fill may overwrite all of it between calls; it is the only user of this list -- teardown needs none,
// the buffers free themselves.  The weight packs, the MOG2 models and the trainers hold state and are not scratch.
#define CK_CTX_SCRATCH_BUFS 41
template <class F>
void ck_for_each_scratch(ck_ctx& c, F f)
{
    DevBuf* const all[] = {
        &c.in_stage, &c.in_stage2, &c.planes, &c.trange, &c.edges, &c.map, &c.labels, &c.labels2, &c.runs, &c.ghost,
        &c.misc, &c.bflag, &c.comp, &c.lists, &c.pts, &c.accum, &c.peaks, &c.goban, &c.act0, &c.act1, &c.act2,
        &c.ybuf, &c.lblbuf, &c.confbuf, &c.rlblbuf, &c.rconfbuf, &c.fgcbuf, &c.out_stage, &c.mats, &c.pyr0, &c.pyr1,
        &c.rec_stage, &c.harvest, &c.harvest_src, &c.jenc_work, &c.jenc_bits, &c.jenc_pack, &c.jspan,
        &c.png_work, &c.png_pack, &c.png_inf,
    };
    static_assert(sizeof all / sizeof all[0] == CK_CTX_SCRATCH_BUFS, "one entry per scratch buffer");
    for (DevBuf* b : all) f(*b);
}
// The scratch buffers are declared in one block, from in_stage up to the weight packs.  A DevBuf added there changes the
// size of the block and stops the build here until the list above (or a reason to leave it out) has it too.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
static_assert(offsetof(ck_ctx, cnn) - offsetof(ck_ctx, in_stage) == CK_CTX_SCRATCH_BUFS * sizeof(DevBuf),
              "a DevBuf joined or left the scratch block of ck_ctx: decide about it in ck_for_each_scratch");
#pragma clang diagnostic pop

extern thread_local std::string g_ck_create_error;

int ck_fail(ck_ctx* ctx, int code, const char* fmt, ...);
int ck_ensure(ck_ctx* ctx, DevBuf& b, size_t bytes);
int ck_ensure_pinned(ck_ctx* ctx, PinBuf& b, size_t bytes, size_t slack = 0);     // grows to bytes + bytes / 4 + slack

#define CK_HIP(ctx, call)                                                                 \
    do {                                                                                  \
        hipError_t e__ = (call);                                                          \
        if (e__ != hipSuccess)                                                            \
            return ck_fail((ctx), CK_ERR_HIP, "%s failed: %s (%s:%d)", #call,             \
                           hipGetErrorString(e__), __FILE__, __LINE__);                   \
    } while (0)

// ---- entry-point bracket: the one-thread-per-context contract, enforced, and nothing thrown across the C ABI ----
unsigned long long ck_thread_token();
void ck_note_busy(const ck_ctx* ctx);              // ck_last_error(ctx) on this thread then explains the refusal
struct CtxCall {
    ck_ctx* ctx;
    int code = CK_OK;
    explicit CtxCall(ck_ctx* c) : ctx(c)
    {
        if (!ctx) { code = CK_ERR_ARG; return; }
        const unsigned long long me = ck_thread_token();
        unsigned long long nobody = 0;
        if (ctx->owner.load(std::memory_order_acquire) == me) { ctx->depth++; return; }
        if (!ctx->owner.compare_exchange_strong(nobody, me, std::memory_order_acq_rel)) {
            ck_note_busy(ctx);
            code = CK_ERR_STATE;
            ctx = nullptr;
            return;
        }
        ctx->depth = 1;
        // the HIP device is per-thread state: whichever host thread drives this context now (a lane's worker, the
        // exchange thread of rank r > 0 ...) works on the context's device from here on
        if (hipSetDevice(ctx->device) != hipSuccess) {
            ctx->depth = 0;
            ctx->owner.store(0, std::memory_order_release);
            code = CK_ERR_HIP;
            ctx = nullptr;
        }
    }
    ~CtxCall()
    {
        if (ctx && --ctx->depth == 0) ctx->owner.store(0, std::memory_order_release);
    }
};
// From CK_API_BEGIN on, ctx is not NULL, this thread owns it, and the HIP device of this thread is ctx->device: an entry
// point neither checks the first nor sets the second again.
#define CK_API_BEGIN(ctx)                         \
    CtxCall call__(ctx);                          \
    if (call__.code != CK_OK) return call__.code; \
    try {
#define CK_API_END(ctx)                                                                                   \
    } catch (const std::exception& e__) {                                                                 \
        return ck_fail((ctx), CK_ERR_STATE, "C++ exception inside the library: %s", e__.what());          \
    } catch (...) {                                                                                       \
        return ck_fail((ctx), CK_ERR_STATE, "unknown C++ exception inside the library");                  \
    }

#define CK_TRY(call)                     \
    do {                                 \
        int rc__ = (call);               \
        if (rc__ != CK_OK) return rc__;  \
    } while (0)

#include "ck_pool.h"       // ck_parallel_for: host loops on the library's worker threads

// timing brackets: record HIP events on the ctx stream around a group of launches
struct TimeScope {
    ck_ctx* ctx;
    int idx = -1;
    TimeScope(ck_ctx* c, const char* name);
    ~TimeScope();
};
int ck_timing_collect(ck_ctx* ctx);

// debugging aid (CK_PROFILE_HOST set): host-side lap times of an entry point on stderr, `lap("what")` after each step;
// every lap ends with a stream synchronisation
struct HostLap {
    ck_ctx* ctx;
    const char* tag;
    std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
    void operator()(const char* what)
    {
        static const bool prof = getenv("CK_PROFILE_HOST") != nullptr;
        if (!prof) return;
        (void)hipStreamSynchronize(ctx->stream);
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[%s] %-18s %8.3f ms\n", tag, what, std::chrono::duration<double, std::milli>(now - t_start).count());
        t_start = now;
    }
};

// bring a possibly-host input to the device (returns device pointer in *dev)
int ck_to_device(ck_ctx* ctx, const void* src, size_t bytes, int space, DevBuf& stage, const void** dev);
// deliver a device result to a possibly-host output
int ck_from_device(ck_ctx* ctx, void* dst, const void* dev, size_t bytes, int space);

static inline int ck_pitch(int w) { return (w + 63) & ~63; }

// the 32-bit finaliser of MurmurHash3: the stateless hash under the trainer's dropout masks (k_cnn_train.hip) and the
// harvest's thinning of empty regions (k_harvest.hip)
__host__ __device__ inline uint32_t mix32(uint32_t h)
{
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

// ---- kernels (one launcher per stage; all asynchronous on ctx->stream) -----------------
// d_range (nullable): per (frame, channel, CK_RANGE_TILE^2 tile) two bytes lo, hi with lo <= every median of the tile <= hi
// (n * 3 * ceil(h / T) * ceil(w / T) * 2 bytes; what k_canny_planar takes to skip its flat tiles)
#define CK_RANGE_TILE 48
static inline size_t ck_range_bytes(int n, int h, int w)
{
    return (size_t)n * 3 * ((h + CK_RANGE_TILE - 1) / CK_RANGE_TILE) * ((w + CK_RANGE_TILE - 1) / CK_RANGE_TILE) * 2;
}
int k_median15_planar(ck_ctx* ctx, const uint8_t* d_bgr, int n, int h, int w, uint8_t* d_planes, int pitch, uint8_t* d_range = nullptr);
int k_gray_hist(ck_ctx* ctx, const uint8_t* d_planes, int n, int h, int w, int pitch, int* d_hist);
int k_median_planar(ck_ctx* ctx, const uint8_t* d_bgr, int n, int h, int w, int ksize, uint8_t* d_planes, int pitch, uint8_t* d_range = nullptr);
int k_planar_to_interleaved(ck_ctx* ctx, const uint8_t* d_planes, int n, int h, int w, int pitch, uint8_t* d_out);
int k_interleaved_to_planar(ck_ctx* ctx, const uint8_t* d_in, int n, int h, int w, int pitch, uint8_t* d_planes);
// canny: planar 3-channel input -> map (0/1/2) -> edges (0/255); labels = scratch n*h*w int32
// d_border_flag (nullable, n ints): set to 1 for frames that have an edge pixel on the image frame
int k_canny_planar(ck_ctx* ctx, const uint8_t* d_planes, int n, int h, int w, int pitch, int low, int high,
                   uint8_t* d_map, int32_t* d_labels, uint8_t* d_edges, uint8_t* d_map_out, int* d_border_flag = nullptr,
                   const int* d_thr = nullptr /* per-frame (low, high) pairs on the device, override low / high */,
                   const uint8_t* d_range = nullptr /* value bounds of the planes' tiles, from k_median_planar */);
int k_i420_to_bgr(ck_ctx* ctx, const uint8_t* d_i420, int n, int h, int w, uint8_t* d_bgr);
// cv2.pyrDown, one level: n x h x w x 3 -> n x (h+1)/2 x (w+1)/2 x 3 (h, w >= 2); and the same behind the I420 conversion
// (h, w even): bit for bit k_pyr_down of k_i420_to_bgr without the full-size BGR frames (k_pyramid.hip)
int k_pyr_down(ck_ctx* ctx, const uint8_t* d_bgr, int n, int h, int w, uint8_t* d_out);
int k_i420_pyr_down(ck_ctx* ctx, const uint8_t* d_i420, int n, int h, int w, uint8_t* d_out);
// baseline JPEG behind the Huffman decoder (k_jpeg.hip): coefficients + quant tables of n frames on the device -> BGR
int k_jpeg_reconstruct(ck_ctx* ctx, const int16_t* d_coef, const uint16_t* d_quant, int n, int h, int w, int sampling, uint8_t* d_bgr);
// baseline JPEG in front of the Huffman coder (k_jpeg_enc.hip): BGR + one set of quant tables on the device -> coefficients
int k_jpeg_forward(ck_ctx* ctx, const uint8_t* d_bgr, const uint16_t* d_quant, int n, int h, int w, int sampling, int16_t* d_coef);
// the Huffman stage on the device (k_jpeg_huff.hip): staged entropy-coded bytes + plan rows + table sets -> coefficients
// (zeroed here first) and one status word per strand
struct CkStrand;
struct CkHuffSet;
struct CkStrandGeom;
int k_jpeg_huff(ck_ctx* ctx, const uint8_t* d_bytes, long long n_bytes, const CkStrand* d_rows, int n_strands, const CkHuffSet* d_sets,
                int n_sets, const CkStrandGeom& g, long long cframe, int n_frames, int16_t* d_coef, uint32_t* d_status);
// the same kernel over the n_rows rows from first_row on, all of frame `frame`, whose coefficients alone are zeroed first
int k_jpeg_huff_frame(ck_ctx* ctx, const uint8_t* d_bytes, long long n_bytes, const CkStrand* d_rows, int first_row, int n_rows,
                      const CkHuffSet* d_sets, int n_sets, const CkStrandGeom& g, long long cframe, int n_frames, int frame, int16_t* d_coef,
                      uint32_t* d_status);
// parallel decoding inside a strand (k_jpeg_span.hip): the five steps of ck_jpeg_span.h over a pass, d_coef zeroed here first;
// J's pointers are HBM; n_spans = span0[n_strands].  Leaves J.verdict (n_strands words) for the caller to fetch.
struct CkSpanJob;
int k_jpeg_span(ck_ctx* ctx, const CkSpanJob& J, long long n_spans);
// the Huffman stage of the encoder on the device (k_jpeg_enc_huff.hip), m frames of one geometry.  CkEncWork: where the sizes
// and offsets of a pass lie in HBM -- per block, per block tile, per segment (seg_u0: nseg + 1 per frame) and per frame
// (frame_u0, out_off: m + 1); head[0] the lowest (frame << 32 | block) that cannot be coded or all ones, head[1] the bytes of
// the bit buffer; consts: the CkEncTables, the zigzag order (64 bytes) and the stream header.
struct CkEncWork {
    uint32_t *bits, *tile_bits;
    uint64_t *tile_off, *seg_bits, *seg_u0, *frame_u0, *head, *len, *out_off;
    const uint8_t* consts;
    // optimised tables (freq NULL: the standard ones): per frame 4 x 256 counters, a CkEncTables, four DHT slots with their
    // lengths, a header slot with its length; pre / post: the header in front of and behind the DHT segments (in consts)
    uint32_t *freq = nullptr, *dht_len = nullptr, *hlen = nullptr;
    uint8_t *tables = nullptr, *dht = nullptr, *headers = nullptr;
    const uint8_t *pre = nullptr, *post = nullptr;
    uint32_t pre_len = 0, post_len = 0;
};
// (optimised tables: histo and tables first, then) size every block and scan: fills all of the above but len and out_off
int k_jpeg_enc_measure(ck_ctx* ctx, const int16_t* d_coef, int m, const CkEncGeom& g, const CkEncWork& w);
// the codes into d_buf (total_u = head[1] bytes, zeroed here), the FF counts of its byte tiles, w.len and w.out_off
int k_jpeg_enc_put(ck_ctx* ctx, const int16_t* d_coef, int m, const CkEncGeom& g, const CkEncWork& w, uint32_t* d_buf, uint64_t total_u,
                   uint32_t* d_ff_cnt, uint32_t* d_ff_off, uint32_t hl);
// headers, stuffed bytes and markers into d_pack (pack_bytes of room), frame f at out_off[f]
int k_jpeg_enc_stuff(ck_ctx* ctx, int m, const CkEncGeom& g, const CkEncWork& w, const uint32_t* d_buf, uint64_t total_u,
                     const uint32_t* d_ff_off, uint32_t hl, uint8_t* d_pack, uint64_t pack_bytes);
// PNG (k_png.hip).  Reading: the inflated rows of n images (image i at d_rows + desc[i].off, h rows of 1 + rowbytes) are
// unfiltered in place and expanded to BGR; palettes: 768 bytes an image.
constexpr int CK_PNG_CHUNK = 24;           // bytes a lane handles per step: whole pixels at every depth (1 .. 64 bits a pixel)
constexpr int CK_PNG_GROUP_ROWS = 256;     // rows in flight: the lanes of the workgroup
int k_png_unfilter(ck_ctx* ctx, uint8_t* d_rows, const CkPngDesc* d_desc, const uint8_t* d_palettes, int n, int h, int w, uint8_t* d_bgr);
// The device inflate (k_png_inflate.hip): a wave per zlib stream.  Stream i lies at d_z + z_off; its first `cap` bytes go to
// d_out + out_off (a multiple of 16); pitch > 0: it holds rows of `pitch` bytes, `need` bytes of them, whose filter bytes
// are checked.  One verdict record (ck_png_inflate_stage.h) a stream.
struct CkInfJob;                  // (ck_png_inflate_stage.h, with the verdict record)
struct CkInfRecord;
int k_png_inflate(ck_ctx* ctx, const uint8_t* d_z, uint8_t* d_out, const CkInfJob* d_jobs, CkInfRecord* d_rec, int n);
// Writing, m frames: where the arrays of a pass lie in HBM -- per band (count, lens, codes: ck_png_pitch(runs) each; band_off),
// per tile (edge, before, after: the runs mode only, else NULL), per frame (out_off: m + 1; head: the bytes of all streams,
// then the bytes of each)
struct CkPngWork {
    uint8_t *filt, *lens;
    uint16_t* codes;
    uint32_t *count, *tile_bits, *tile_a, *tile_b, *band_a, *band_b, *adler;
    uint64_t *tile_off, *band_bits, *band_off, *frame_bits, *out_off, *head;      // tile_off: from the start of the band's block
    CkPngEdge* edge;
    uint32_t *before, *after;
};
// filter, (edges, join,) count, build, size, scan: fills all of the above.  runs: 0 literals only, 1 the runs mode
int k_png_enc_measure(ck_ctx* ctx, const uint8_t* d_bgr, int m, const CkPngGeom& g, int filter, const CkPngWork& wk, int runs);
// the zlib streams into d_pack (pack_bytes, zeroed here: head[0] and a dword to spare), frame f at out_off[f]
int k_png_enc_put(ck_ctx* ctx, int m, const CkPngGeom& g, const CkPngWork& wk, uint32_t* d_pack, uint64_t pack_bytes, int runs);
// overlays (k_overlay.hip): n_work non-empty bins of the plan of ck_overlay.cpp, drawn in place on images of h x w x c
int k_overlay(ck_ctx* ctx, uint8_t* d_img, int h, int w, int c, const int32_t* d_work, int n_work, const int32_t* d_refs,
              const int32_t* d_recs, const uint8_t* d_text);
int k_warp(ck_ctx* ctx, const uint8_t* d_bgr, int n, int h, int w, const double* d_minv, int m_count,
           int dsize, uint8_t* d_out);
int k_board_lines(ck_ctx* ctx, const uint8_t* d_edges, int n, int h, int w, int hough_thresh,
                  float* lines, int cap, ck_board_result* res, uint8_t* d_ghost_out,
                  const int* d_canny_border_flag = nullptr);
// d_nonfinite (nullable): set to 1 when a softmax came out inf / NaN
// one external contour of an edge map (k_contour_survey): first pixel (raster index = discovery key), length of the
// CHAIN_APPROX_SIMPLE vertex list, outer-border pixels as x0, y0, x1, y1, ...
struct CkContour {
    int root = 0;
    int nvert = 0;
    std::vector<int32_t> pts;
};
int k_contour_survey(ck_ctx* ctx, const uint8_t* d_edges, int n, int h, int w, std::vector<std::vector<CkContour>>& out);
int ck_goban_canny_dev(ck_ctx* ctx, const uint8_t* d_in, int n, int h, int w, uint8_t* d_edges, double* otsu_out);   // ck_api.hip
int k_contour_stones(ck_ctx* ctx, const uint8_t* d_goban, const uint8_t* d_fg, int n, int side, const int32_t* rects,
                     int rs, int re, int cs, int ce, uint8_t* stones, int16_t* zones_out, uint8_t* mask_out);
// SfClustering.find_stones for m jobs (k_cluster.hip); draws 21 numbers per job from ctx->rng_state
int k_cluster_stones(ck_ctx* ctx, const void* d_imgs, int n, int side, int is_f32, const int32_t* rects, const uint8_t* mask,
                     const int32_t* jobs, int m, uint8_t* stones, uint8_t* trusted, uint8_t* ratios, float* centers,
                     uint8_t* labels, long long labels_cap, int32_t* passes, double* compact, int32_t* winner);
double ck_otsu_level(const int* hist, size_t npx);                        // ck_api.hip: getThreshVal_Otsu_8u restated
// StonesFinder.find_intersections, device half: Canny of the grey image + HoughLinesP of the 361 zones -> host tables
// (*lines_out / *nlines_out point into the context's pinned host arena: valid until the next call on this context)
int k_grid_lines(ck_ctx* ctx, const uint8_t* d_goban, int n, int side, const int32_t* rects, const int16_t** lines_out,
                 const int32_t** nlines_out, uint8_t* edges_out);
int k_cnn_predict(ck_ctx* ctx, const uint8_t* d_goban, int n, float* d_y, uint8_t* d_labels, double* d_conf,
                  int* d_nonfinite = nullptr, uint8_t* d_rlabel = nullptr, double* d_rconf = nullptr);
int k_cnn_pack_weights(ck_ctx* ctx, const float* const w[12], int space);
// CK_CNN_BF16 (k_cnn_bf16.hip): conv1 + conv2 and conv3 + conv4 of np patches, pooled maps out as bf16
int k_cnn_bf16_convs(ck_ctx* ctx, const uint8_t* gob, int np, uint16_t* p2, uint16_t* q4);
int k_cnn_bf16_fc1(ck_ctx* ctx, const uint16_t* q4, int np, float* h1);
// CK_CNN_F16Q8 (k_cnn_q8.hip): the same two fused kernels with f32 maps in and out (drop-ins for the split-precision pair of k_cnn.hip)
int k_cnn_q8_conv12(ck_ctx* ctx, const uint8_t* gob, int np, float* p2, int* overflow);
int k_cnn_q8_conv34(ck_ctx* ctx, const float* p2, int np, float* p4, int* overflow);
// the classifier's training step (k_cnn_train.hip); d_x n x 40 x 40 x 3 and d_lab n bytes on the device
int k_train_create(ck_ctx* ctx, CkTrainer& tr, const float* const w[12], int space);
int k_train_grads(ck_ctx* ctx, CkTrainer& tr, const uint8_t* d_x, const uint8_t* d_lab, int n, int drop, uint64_t seed,
                  uint64_t step, bool want_masks);
int k_train_adam(ck_ctx* ctx, CkTrainer& tr, const float* d_g, double lr);
int k_mog2_apply(ck_ctx* ctx, Mog2State& st, const uint8_t* d_img, double lr, uint8_t* d_fg);
int k_mog2_run(ck_ctx* ctx, Mog2State& st, const uint8_t* d_gobans, int n, const double* learning_rates,
               int32_t* d_fgcount, uint8_t* d_last_fg, int skip_row, int skip_col);
int k_zone_counts(ck_ctx* ctx, const uint8_t* d_mask, int n, int side, int32_t* d_fgcount);
// per-frame records in HBM (k_records.hip): the board half from n packed 536-byte parts, the stones half from the classifier's
// contiguous region outputs
int k_records_put_board(ck_ctx* ctx, const uint8_t* d_parts, int n, ck_frame_record* d_rec);
int k_records_put_regions(ck_ctx* ctx, const uint8_t* d_rlabel, const double* d_rconf, int n, ck_frame_record* d_rec);
// labelled patches out of goban images and their augmentation (k_harvest.hip); the flag pass runs blocks of 1024 candidates
#define CK_HARVEST_BLOCK 1024
static inline int ck_harvest_blocks(int n) { return (int)(((long long)n * 100 + CK_HARVEST_BLOCK - 1) / CK_HARVEST_BLOCK); }
int k_harvest(ck_ctx* ctx, const uint8_t* d_goban, const int32_t* d_fgcount, const int32_t* d_state, const uint8_t* d_positions, int n,
              int calm_max, int empty_keep, uint32_t seed, uint32_t first_frame, int32_t* d_code, int32_t* d_blocks,
              uint8_t* d_x, uint8_t* d_labels, int32_t* d_src, int cap);
int k_augment(ck_ctx* ctx, const uint8_t* d_x, const uint8_t* d_t, int n, uint8_t* d_out);

#include "ck_host_geom.h"  // host geometry and the host decisions of k_board_lines (ck_host_geom.cpp)
