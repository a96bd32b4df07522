/*
 * camkifu_amd.h -- C-ABI of the MI355X-native CamKifu vision hot path (libck_hip.so).
 *
 * Drop-in boundary: the reference (ArnaudPel/CamKifu) is pure Python and reaches all of
 * its arithmetic through cv2 / Keras calls made from BoardFinderAuto._detect and
 * StonesFinder._doframe / SfNeural._find.  Each entry point below replaces one such call
 * site (cited as file:line under the reference's src/camkifu/), takes plain pointers and
 * sizes, and is what a ctypes binding in the reference would bind.
 *
 * Conventions
 *   - every function returns CK_OK (0) or a CK_ERR_* code; nothing throws or aborts across
 *     the boundary; ck_last_error() gives the message for the last failing call on a ctx.
 *   - images are uint8, row-major, channels interleaved (BGR) exactly as cv2 hands them,
 *     no row padding (stride = w * channels); batches are n such images back to back.
 *   - `*_space` arguments say where a pointer lives: CK_HOST or CK_DEVICE (HBM).  Input
 *     pointers are borrowed for the duration of the call only.
 *   - one ck_ctx per finder instance / thread: it owns a HIP stream and scratch buffers
 *     and is not re-entrant; different contexts may be used concurrently.
 *   - calls are synchronous: results are complete when the call returns.
 */
#ifndef CAMKIFU_AMD_H
#define CAMKIFU_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { CK_OK = 0, CK_ERR_ARG = 1, CK_ERR_HIP = 2, CK_ERR_CAPACITY = 3, CK_ERR_STATE = 4,
       CK_ERR_DATA = 5 /* the input bytes are not what the call can read: a JPEG stream it refuses or that is damaged */ };
enum { CK_HOST = 0, CK_DEVICE = 1 };
enum { CK_BACKEND_HIP = 1 };
enum { CK_CNN_FP32 = 0, CK_CNN_BF16 = 1, CK_CNN_F16X2 = 2, CK_CNN_F16Q8 = 3 };

/* per-frame status of the board path, mirrors the early exits of
 * BoardFinderAuto._detect (board/bf_auto.py:76-82) */
enum { CK_BOARD_LINES = 0,        /* lines were searched (n_lines may be 0)          */
       CK_BOARD_NO_CONTOUR = 1,   /* len(contours) == 0                 bf_auto.py:76 */
       CK_BOARD_TOO_SMALL = 2 };  /* not frame_area/3 < biggest.area     bf_auto.py:82 */

typedef struct ck_ctx ck_ctx;

/* ---- Alignment of device memory -------------------------------------------------------
 * An INPUT pointer in CK_DEVICE space may have ANY alignment of its element type: a uint8 image may start at any byte, an
 * int16 / uint16 array at any even address, an int32 / float array at any multiple of 4 -- a slice frames[1:], a row range
 * of a byte buffer, a tensor carved out of a pool.  So may these OUTPUTS: the `bgr` of ck_i420_to_bgr, ck_i420_to_bgr_pyr,
 * ck_jpeg_reconstruct, ck_jpeg_decode and ck_png_decode, the `out` of ck_pyr_down and ck_warp_perspective, the `edges` of
 * ck_board_edges, ck_goban_canny and ck_canny and the latter's `map_out`.  The kernels pick their wide (dword, 16-byte) forms
 * by the address where a store needs it and load unaligned elsewhere; the result is the same bytes either way, and for
 * these arguments no byte in front of or behind them is written.  Every OTHER device output (labels, confidences, masks,
 * counts, ghost maps, ...) has only ever been run on 16 bytes: keep it there.  (Host pointers go through the context's
 * staging buffers: no alignment is asked of them.)
 *
 * The exceptions, each refused before anything of the caller's is written, with the message ck_last_error gives:
 *
 *   entry point                     argument  bytes  refused with
 *   ck_jpeg_reconstruct             coef      16     CK_ERR_ARG "coefficients and quant tables must lie on 16 bytes"
 *   ck_jpeg_reconstruct             quant     16     CK_ERR_ARG "coefficients and quant tables must lie on 16 bytes"
 *   ck_jpeg_coefficients_device     coef      16     CK_ERR_ARG "coefficients and quant tables must lie on 16 bytes"
 *   ck_jpeg_coefficients_device     quant     16     CK_ERR_ARG "coefficients and quant tables must lie on 16 bytes"
 *   ck_jpeg_forward                 coef      16     CK_ERR_ARG "coefficients must lie on 16 bytes"
 *   ck_jpeg_entropy_encode_device   coef      16     CK_ERR_ARG "coefficients must lie on 16 bytes"
 *   ck_harvest_patches              goban     4      CK_ERR_ARG "goban images in device memory must be 4-byte aligned"
 *   ck_harvest_patches              x         8      CK_ERR_ARG "x in device memory must be 8-byte aligned, src 4-byte aligned"
 *   ck_harvest_patches              src       4      CK_ERR_ARG "x in device memory must be 8-byte aligned, src 4-byte aligned"
 *   ck_augment_patches              x         4      CK_ERR_ARG "patches in device memory must be 4-byte aligned"
 *   ck_augment_patches              x_out     4      CK_ERR_ARG "patches in device memory must be 4-byte aligned"
 *   ck_board_detect_records         rec       8      CK_ERR_ARG "records must be 8-byte aligned"
 *   ck_cnn_regions_records          rec       8      CK_ERR_ARG "records must be 8-byte aligned"
 *
 * (the coefficient arrays are read and written 16 bytes at a time, a patch a dword at a time, a record's doubles as
 * doubles.)  tests/test_gpu_alignment.py holds the inputs and the outputs named above to this at every offset within
 * 16 bytes. */

typedef struct ck_board_result {
    int32_t status;        /* CK_BOARD_*                                              */
    int32_t n_contours;    /* len(contours) returned by findContours(RETR_EXTERNAL)   */
    int32_t n_lines;       /* number of Hough lines found (may exceed the caller cap) */
    int32_t reserved;
    double  biggest_area;  /* sorted_boxes[-1].area (minAreaRect w*h)                 */
} ck_board_result;

/* ---- context ------------------------------------------------------------------------ */
int  ck_ctx_create(int device, ck_ctx** out);
/* The same with a HIP stream priority for the context's stream: 0 normal, 1 the device's highest, -1 its lowest.  A finder
 * whose calls are short and waited for (the board finder of the hold-off-aware file mode: a few frames per call, the fold
 * waits for the answer) gets its kernels onto the CUs ahead of the long launches of other contexts. */
int  ck_ctx_create_prio(int device, int priority, ck_ctx** out);
void ck_ctx_destroy(ck_ctx* ctx);
/* The same with a status: CK_OK when the context was freed; CK_ERR_STATE when another thread was still inside one of its
 * calls after 5 s -- the context is then NOT freed (nothing is pulled from under that thread) and the handle stays valid:
 * call again later.  ck_ctx_destroy is this call with the status dropped (it prints a line to stderr instead). */
int  ck_ctx_destroy2(ck_ctx* ctx);
/* Stream-ordered hand-over of device memory from a host framework (PyTorch: the caller passes torch's CURRENT stream, as a
 * hipStream_t): everything queued on `stream` up to now runs before anything this context launches from now on
 * (hipEventRecord on `stream`, hipStreamWaitEvent on the context's).  No host wait.  A host that allocates its outputs or
 * produces its inputs on a stream of its own calls this before it passes their pointers to an entry point below; results
 * need no call in the other direction: every entry point returns with its work complete. */
int  ck_stream_wait(ck_ctx* ctx, void* stream);
const char* ck_last_error(const ck_ctx* ctx);     /* ctx may be NULL: last create error */
int  ck_backend(const ck_ctx* ctx);               /* CK_BACKEND_HIP                     */
int  ck_version(void);
void* ck_stream(ck_ctx* ctx);                     /* the hipStream_t the ctx launches on */
/* kernel-time accounting with HIP events on the ctx stream (used by bench.py) */
int  ck_timing_enable(ck_ctx* ctx, int on);
int  ck_timing_reset(ck_ctx* ctx);
/* name: "median", "canny_nms", "ccl", "hough_vote", "warp", "cnn", ...; returns total ms
 * and number of launches recorded since the last reset */
int  ck_timing_get(ck_ctx* ctx, const char* name, double* total_ms, int* launches);
/* A testing aid.  Scratch memory carries nothing from one entry-point call to the next, so overwriting it between calls
 * must change no result: this call waits for the context's stream, sets every byte of every scratch buffer of the context
 * (device and pinned host alike, each over its whole capacity) and of the per-call buffers of its live trainers to `byte`
 * (0 .. 255, else CK_ERR_ARG), and waits again.  The classifier's weights, the MOG2 models and a trainer's weights and Adam
 * moments are state and stay as they are.  The two results that lie in scratch between calls on purpose are dropped with
 * it: ck_jpeg_encode_histograms and ck_png_run_stats answer afterwards as before the first encode (CK_ERR_STATE).
 * bytes_filled / buffers_filled (nullable): how much was overwritten, in how many buffers. */
int  ck_debug_scratch_fill(ck_ctx* ctx, int byte, long long* bytes_filled, int* buffers_filled);

/* ---- K1  cv2.medianBlur(frame, 15)                              board/bf_auto.py:72 */
int ck_median15(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space,
                uint8_t* out, int out_space);
/*          cv2.medianBlur(img, ksize), ksize odd in 3..17 (13 and 7 are SfContours.get_canny's,
 *          stone/sf_contours.py:336-337); same exact median, replicate border */
int ck_median(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int ksize, int in_space,
              uint8_t* out, int out_space);

/* ---- K2  cv2.Canny(median, low, high)  3-channel, aperture 3, L1  board/bf_auto.py:73
 * map_out (optional, same space as edges): NMS map before hysteresis
 * (0 candidate, 1 suppressed, 2 strong). */
int ck_canny(ck_ctx* ctx, const uint8_t* img3, int n, int h, int w, int in_space,
             int low, int high, uint8_t* edges, uint8_t* map_out, int out_space);

/* ---- SfContours.get_canny(img)                 stone/sf_contours.py:332-340
 *   median = medianBlur(medianBlur(img, 13), 7); otsu = threshold(cvtColor(median, BGR2GRAY), 12, 255, THRESH_OTSU)[0];
 *   return Canny(median, otsu / 2, otsu)
 * edges: n*h*w bytes {0,255}; otsu_out (nullable, host): n doubles, the Otsu levels used */
int ck_goban_canny(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space,
                   uint8_t* edges, int out_space, double* otsu_out);

/* ---- K1+K2 fused pipeline: the "filter pass"                  board/bf_auto.py:72-73 */
int ck_board_edges(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space,
                   uint8_t* edges, int out_space);

/* ---- K3..K6  findContours(RETR_EXTERNAL) -> 3 biggest minAreaRect -> drawContours
 *      -> HoughLines(1, pi/180, hough_thresh)          board/bf_auto.py:75-84, 105-133
 * lines: host, n * cap * 2 floats (rho, theta) in OpenCV's order; res: host, n entries.
 * ghost_out optional (n*h*w).  hough_thresh < 0 means int(min(h,w)/5). */
int ck_board_lines(ck_ctx* ctx, const uint8_t* edges, int n, int h, int w, int in_space,
                   int hough_thresh, float* lines, int cap, ck_board_result* res,
                   uint8_t* ghost_out, int ghost_space);

/* ---- K1..K6 stateless core of BoardFinderAuto._detect        board/bf_auto.py:72-84 */
int ck_board_detect(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space,
                    int hough_thresh, float* lines, int cap, ck_board_result* res);

/* ---- frame source: what cv2.VideoCapture.read() hands every consumer   core/vmanager.py:506-509, 584
 * (the reference decodes to BGR on the CPU).  A file reader that holds planar YUV 4:2:0 frames
 * (I420: Y h*w, U, V (h/2)*(w/2) each; e.g. a .y4m file) uploads 1.5 B/px and converts in HBM:
 * BT.601 studio range, the 20-bit fixed-point arithmetic of cv2.cvtColor(COLOR_YUV2BGR_I420).
 * i420: n frames of h*w*3/2 bytes; bgr: n x h x w x 3.  h and w must be even. */
int ck_i420_to_bgr(ck_ctx* ctx, const uint8_t* i420, int n, int h, int w, int in_space,
                   uint8_t* bgr, int out_space);

/* ---- frame source, compressed: baseline JPEG (Motion-JPEG frames of an .avi, .jpg stills)   core/vmanager.py:638-660 (cv2.imread),
 * stone/nn_manager.py:134.  The numbers are libjpeg's default decode path (slow-integer IDCT, "fancy" chroma upsampling,
 * fixed-point YCbCr -> RGB): what cv2.imread and Pillow give, bit for bit.  Two halves:
 *   host: marker parser + Huffman decoder -> per frame int16 coefficient blocks (component-planar: Y, then Cb, then Cr;
 *         blocks in raster order over the MCU-padded block grid; 64 values per block in natural, de-zigzagged order; not
 *         dequantised) and uint16 quant[3][64] (natural order, by component, table selectors resolved);
 *   GPU:  one kernel: dequantise, inverse DCT, upsample, convert, interleaved BGR (n x h x w x 3) out.
 * Accepted: SOF0, 8-bit, one component (grey: Y is written three times) or three taken as Y Cb Cr with luma sampling 1x1,
 * 2x1 or 2x2 and chroma 1x1, one interleaved scan, with or without restart intervals; a frame without DHT is decoded with the
 * tables of Annex K.3.  Everything else -- other frame types, other samplings, an Adobe APP14 segment with transform 0, several
 * scans, damaged entropy-coded data -- is CK_ERR_DATA with a message that names the cause (host-only calls: ck_last_error(NULL)). */
enum { CK_JPEG_GREY = 0, CK_JPEG_444 = 1, CK_JPEG_422 = 2, CK_JPEG_420 = 3 };
typedef struct ck_jpeg_info {
    int32_t h, w;
    int32_t sampling;          /* CK_JPEG_*                                                   */
    int32_t restart_interval;  /* MCUs between restart markers, 0: none                       */
    int32_t blocks;            /* 8x8 blocks per frame, all components, on the MCU-padded grid */
} ck_jpeg_info;
/* the headers of one stream (host only) */
int ck_jpeg_probe(const uint8_t* data, size_t len, ck_jpeg_info* info);
/* n streams that all have the geometry *geom (h, w, sampling; else CK_ERR_DATA) -> coef n * geom->blocks * 64 int16 and
 * quant n * 3 * 64 uint16 (host only; frames decode in parallel on the library's worker threads).  On CK_ERR_DATA *bad_frame
 * (nullable) is the first frame that failed. */
int ck_jpeg_coefficients(const uint8_t* const* data, const size_t* len, int n, const ck_jpeg_info* geom,
                         int16_t* coef, uint16_t* quant, int32_t* bad_frame);
/* coefficients + quant tables of n frames of h x w (in `in_space`, both) -> bgr */
int ck_jpeg_reconstruct(ck_ctx* ctx, const int16_t* coef, const uint16_t* quant, int n, int h, int w, int sampling,
                        int in_space, uint8_t* bgr, int out_space);
/* the three steps in one call: n streams in HOST memory, all of the first one's geometry -> bgr.  The coefficients are
 * decoded into pinned memory of the context and go up in one copy (a large batch in passes of about 256 MB each). */
int ck_jpeg_decode(ck_ctx* ctx, const uint8_t* const* data, const size_t* len, int n, uint8_t* bgr, int out_space);
/* the frame the context's last ck_jpeg_decode refused with CK_ERR_DATA, -1 when it refused none */
int ck_jpeg_bad_frame(ck_ctx* ctx, int32_t* frame);
/* the bytes the context's last ck_jpeg_decode or ck_jpeg_coefficients_device copied from host to device, all passes: the
 * coefficients and quant tables in host entropy mode; the entropy-coded segments, plan rows, table sets and quant tables in
 * device entropy mode */
int ck_jpeg_uploaded_bytes(ck_ctx* ctx, long long* bytes);

/* The Huffman stage on the GPU, opt-in.  A strand is one restart interval of one frame (the whole scan of a frame that has
 * none): it starts byte-aligned with the DC predictors at zero, so one GPU lane decodes it without knowing the others.
 * The host parses the headers and finds the restart markers by a byte scan (the plan); the compressed bytes go up as
 * they are, and one kernel decodes them into the coefficient layout above.  Both modes accept and refuse the same
 * streams and give the same coefficients.  A frame without restart intervals is decoded by one lane alone: correct, and slow.
 * A large batch goes through in passes under ck_jpeg_decode's rule, applied to what this mode stages: about 256 MB of
 * compressed bytes per pass, and at most 2 GiB of coefficients in HBM. */
enum { CK_JPEG_ENTROPY_HOST = 0, CK_JPEG_ENTROPY_DEVICE = 1 };
/* what ck_jpeg_decode does from now on; a new context has CK_JPEG_ENTROPY_HOST */
int ck_jpeg_set_entropy(ck_ctx* ctx, int mode);
/* ck_jpeg_coefficients with the Huffman stage on the GPU: streams in HOST memory -> coef and quant in `out_space` (on the
 * device both must lie on 16 bytes).  On CK_ERR_DATA *bad_frame (nullable) is the first frame that failed. */
int ck_jpeg_coefficients_device(ck_ctx* ctx, const uint8_t* const* data, const size_t* len, int n, const ck_jpeg_info* geom,
                                int16_t* coef, uint16_t* quant, int out_space, int32_t* bad_frame);
/* host only: the plan of n streams of the geometry *geom -> rows of 6 int64 {frame, begin, end, first_mcu, n_mcu, table_set};
 * begin / end are offsets into stream `frame`.  Table sets (DC and AC of each component, selectors resolved) are de-duplicated by content
 * across the call.  A `cap` (in rows) too small is CK_ERR_CAPACITY with *n_strands set, so a caller can size the array and
 * call again; strands may be NULL with cap 0. */
int ck_jpeg_plan(const uint8_t* const* data, const size_t* len, int n, const ck_jpeg_info* geom,
                 int64_t* strands, long long cap, long long* n_strands, int32_t* n_table_sets, int32_t* bad_frame);
/* host only: the plan, then every strand through the GPU kernel's decoder ON THE HOST -> what ck_jpeg_coefficients gives */
int ck_jpeg_coefficients_strands(const uint8_t* const* data, const size_t* len, int n, const ck_jpeg_info* geom,
                                 int16_t* coef, uint16_t* quant, int32_t* bad_frame);

/* Parallel decoding INSIDE a strand, opt-in as well: CK_JPEG_ENTROPY_DEVICE_SPANS for ck_jpeg_set_entropy.  Every strand is
 * cut into spans of S raw bytes.  A lane per span and per block slot of the MCU starts one span early on a guess and records
 * where it stands when it crosses into its span (Huffman streams fall into step after a short run); a walk per strand
 * picks the guesses that meet the true chain and decodes the few spans none met; a lane per span then writes its
 * coefficients, and a sum per strand turns DC differences into values.  A strand whose chain is not clean beyond doubt
 * has its frame decoded again by the one-lane kernel of CK_JPEG_ENTROPY_DEVICE, whose status decides: the mode accepts and
 * refuses the same streams as the host decoder, names the same frame and gives the same coefficients. */
enum { CK_JPEG_ENTROPY_DEVICE_SPANS = 2 };
/* S for the context, 8 .. 4096 bytes (anything else is CK_ERR_ARG); ck_jpeg_span_bytes gives the default */
int ck_jpeg_set_span_bytes(ck_ctx* ctx, int bytes);
int ck_jpeg_span_bytes(int32_t* bytes);
/* what the context's last ck_jpeg_decode / ck_jpeg_coefficients_device did in that mode, all passes: stats[0] spans,
 * [1] unresolved spans (decoded by the walk itself), [2] suspect strands, [3] frames handed to the one-lane kernel */
int ck_jpeg_span_stats(ck_ctx* ctx, long long* stats);
/* host only: the plan, then the steps the GPU kernels run, in their order ON THE HOST, the one-lane decoder for suspect
 * frames included -> what ck_jpeg_coefficients gives.  span_bytes: 8 .. 4096; stats (nullable): 4 values as above */
int ck_jpeg_coefficients_spans(const uint8_t* const* data, const size_t* len, int n, const ck_jpeg_info* geom, int span_bytes,
                               int16_t* coef, uint16_t* quant, int32_t* bad_frame, long long* stats);

/* ---- compressed output: baseline JPEG encode (.jpg stills, Motion-JPEG frames of an .avi)   core/vmanager.py:309-325 (cv2.imwrite)
 * The mirror of the calls above, and as exact: the streams are, byte for byte, what libjpeg's default compressor writes
 * (fixed-point RGB -> YCbCr, box downsampling without smoothing, slow-integer forward DCT, the quant tables of
 * jpeg_set_quality, the Huffman tables of Annex K.3 unless optimised ones are asked for, JFIF 1.01 headers) --
 * PIL.Image.save(.., "JPEG", quality=q, subsampling=s).
 *   GPU:  BGR frames -> per frame int16 quantised coefficient blocks, in the layout ck_jpeg_coefficients writes (one kernel)
 *   host: headers + Huffman coder -> one stream per frame
 * Optimised tables on request (ck_jpeg_set_encode_tables, below); no progressive or arithmetic coding, quality 1 .. 100. */
/* quant[3][64] uint16 (natural order, by component) of a quality; clamped to 1 .. 100 (host only) */
int ck_jpeg_quant(int quality, uint16_t* quant);
/* *bytes: the largest stream a frame of h x w can become (host only) */
int ck_jpeg_encode_bound(int h, int w, int sampling, size_t* bytes);
/* n BGR frames of h x w (in `in_space`) + one set of quant tables (HOST memory, entries 1 .. 255) -> coef, n * blocks * 64
 * int16 (in `out_space`; on the device it must lie on 16 bytes).  CK_JPEG_GREY encodes Y alone. */
int ck_jpeg_forward(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space, const uint16_t* quant, int sampling,
                    int16_t* coef, int out_space);
/* coefficients of n frames + one set of quant tables -> n streams: frame f at out + f * stride, len[f] bytes (host only;
 * the frames are coded in parallel on the library's worker threads).  stride must be at least ck_jpeg_encode_bound;
 * restart_interval in MCUs, 0: none.  CK_ERR_ARG names a coefficient the baseline Huffman tables cannot code. */
int ck_jpeg_entropy_encode(const int16_t* coef, const uint16_t* quant, int n, int h, int w, int sampling, int restart_interval,
                           uint8_t* out, size_t stride, size_t* len);
/* both halves in one call: n BGR frames (in `in_space`) -> n streams in HOST memory, laid out as above.  The coefficients
 * come down in one copy into pinned memory of the context (a large batch in passes of about 256 MB each). */
int ck_jpeg_encode(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space, int quality, int sampling,
                   int restart_interval, uint8_t* out, size_t stride, size_t* len);
/* The Huffman stage of the encoder on the GPU (CK_JPEG_ENTROPY_DEVICE, as for decoding): every block sizes its own code, prefix
 * sums place the blocks and the stuffed bytes, and only the finished streams come down -- in one copy per pass, frames end
 * to end on 16 bytes, behind two small copies of sizes (16 bytes, then 8 bytes per frame).  Byte for byte the streams of the
 * host coder, with its refusals.  A pass holds what ck_jpeg_encode's rule gives, its coefficients at most 2 GiB of HBM. */
/* what ck_jpeg_encode does from now on; a new context has CK_JPEG_ENTROPY_HOST */
int ck_jpeg_set_encode_entropy(ck_ctx* ctx, int mode);
/* ck_jpeg_entropy_encode with the Huffman stage on the GPU: coef in `in_space` (16-byte aligned on the device), quant in HOST
 * memory -> n streams in HOST memory at out + f * stride, len[f] bytes.  Same refusals, same frame, same message. */
int ck_jpeg_entropy_encode_device(ck_ctx* ctx, const int16_t* coef, int in_space, const uint16_t* quant, int n, int h, int w,
                                  int sampling, int restart_interval, uint8_t* out, size_t stride, size_t* len);
/* the bytes the context's last ck_jpeg_encode / ck_jpeg_entropy_encode_device copied from device to host, all passes: the
 * coefficients in the host mode; the streams, each rounded up to 16 bytes, and 16 + 8 * frames bytes of sizes per pass in
 * the device mode */
int ck_jpeg_downloaded_bytes(ck_ctx* ctx, long long* bytes);
/* host only: ck_jpeg_entropy_encode through the steps the GPU kernels run -- size, scan, put, stuff -- in plain loops over the
 * same tiles -> the same streams, the same refusals */
int ck_jpeg_entropy_encode_staged(const int16_t* coef, const uint16_t* quant, int n, int h, int w, int sampling, int restart_interval,
                                  uint8_t* out, size_t stride, size_t* len);
/* the tiles of those steps: blocks whose codes one workgroup assembles, unstuffed bytes one workgroup places (host only) */
int ck_jpeg_enc_tiles(int32_t* blocks_per_tile, int32_t* bytes_per_tile);
/* Optimised Huffman tables: libjpeg's optimize_coding, PIL.Image.save(.., optimize=True).  The coefficients, and so the pixels,
 * are those of the standard mode; every DHT segment carries a table fitted to its frame, and the stream is, byte for byte,
 * what libjpeg writes then.  Per frame: the symbols the coder emits are counted in its scan order (four tables of 256
 * counters: DC luma, AC luma, DC chroma, AC chroma -- a grey frame has the first two), each table goes through
 * jpeg_gen_optimal_table (the two least counts merge, the larger index among equals; no code is all ones; codes above
 * 16 bits are shortened pairwise), and the scan is coded with the result.  What the standard mode refuses is refused with
 * the same frame and message, before a table is made; a frame of more than 2^25 blocks is CK_ERR_ARG (32-bit counters).
 * ck_jpeg_encode_bound holds for both modes. */
enum { CK_JPEG_TABLES_STANDARD = 0, CK_JPEG_TABLES_OPTIMISED = 1 };
/* what ck_jpeg_encode writes from now on, in either entropy mode; a new context has CK_JPEG_TABLES_STANDARD */
int ck_jpeg_set_encode_tables(ck_ctx* ctx, int mode);
/* host only: the counters of n frames, counts[n][4][256] uint32 in the order above */
int ck_jpeg_histogram(const int16_t* coef, int n, int h, int w, int sampling, int restart_interval, uint32_t* counts);
/* host only: counts[256] -> bits[16] (the number of codes of 1 .. 16 bits) and vals[256], of which *count are used: the
 * body of a DHT segment */
int ck_jpeg_optimal_table(const uint32_t* counts, uint8_t* bits, uint8_t* vals, int32_t* count);
/* ck_jpeg_entropy_encode, _staged and _device with optimised tables: on the worker threads in two passes per frame; through
 * the kernels' steps in plain loops on the host (histo and tables in front of size, scan, put, stuff); on the GPU, where the
 * counters, the tables and the headers stay in HBM and ck_jpeg_downloaded_bytes counts what it counts in the standard mode */
int ck_jpeg_entropy_encode_opt(const int16_t* coef, const uint16_t* quant, int n, int h, int w, int sampling, int restart_interval,
                               uint8_t* out, size_t stride, size_t* len);
int ck_jpeg_entropy_encode_opt_staged(const int16_t* coef, const uint16_t* quant, int n, int h, int w, int sampling, int restart_interval,
                                      uint8_t* out, size_t stride, size_t* len);
int ck_jpeg_entropy_encode_opt_device(ck_ctx* ctx, const int16_t* coef, int in_space, const uint16_t* quant, int n, int h, int w,
                                      int sampling, int restart_interval, uint8_t* out, size_t stride, size_t* len);
/* a test hook: the counters the kernels left in HBM in the last pass of the context's last optimised encode on the GPU,
 * counts[n][4][256] as ck_jpeg_histogram gives them; n must be that pass's frames (CK_ERR_STATE otherwise, and after a
 * standard encode).  A copy of its own: ck_jpeg_downloaded_bytes does not count it. */
int ck_jpeg_encode_histograms(ck_ctx* ctx, int n, uint32_t* counts);

/* ---- lossless stills: PNG   core/vmanager.py:309-325 (cv2.imwrite of snapshot-N.png), :638-660 (cv2.imread), stone/nn_manager.py:134
 * Reading gives what cv2.imread's default mode gives: BGR, 8 bits; alpha and tRNS are dropped, never composited; 16-bit
 * samples give their high byte; grey of 1 / 2 / 4 bits is scaled by 255 / 85 / 17; a palette index beyond PLTE is black.
 *   host: the chunk walk (signature, every chunk's CRC-32, IHDR first, one PLTE in front of IDAT -- passed over in a grey
 *         image, its entries beyond 2^depth dropped, as libpng does --, consecutive IDAT chunks joined, IEND; ancillary chunks
 *         skipped, an unknown critical one and an IDAT behind another chunk refused) and an inflate of the library's own -- no libz -- whose verdict is zlib's;
 *         the frames of a batch on the worker threads.  The filter bytes are checked there (0 .. 4).
 *   GPU:  the inflated rows go up in one copy; one kernel undoes the filters along anti-diagonals (a lane per row, a chunk of
 *         24 bytes per step, a barrier between steps) and writes BGR.
 * Colour types 0, 2, 3, 4, 6 at every bit depth the standard allows them, not interlaced; sides up to 65535 and up to
 * 2^28 pixels.  Anything else, and any damage, is CK_ERR_DATA with the cause in ck_last_error.
 * Writing gives 8-bit RGB files with one IDAT: per row the filter with the least sum of |residual| (libpng's heuristic) or a
 * forced one; per band of 16 rows one deflate block with a dynamic Huffman code of its own, literals only -- no matches, no
 * runs: a flat image does not go below about one bit a byte (unless ck_png_set_encode_matches asks for runs).  Filter, count, build, size, scan and put are launches of
 * their own; the Adler-32 is computed on the GPU too; only the zlib streams come down, the container is put around them
 * on the host. */
typedef struct ck_png_info {
    int32_t h, w;
    int32_t color_type;        /* 0 grey, 2 RGB, 3 palette, 4 grey + alpha, 6 RGB + alpha        */
    int32_t bit_depth;         /* 1, 2, 4, 8, 16                                                 */
    int32_t palette_entries;   /* of PLTE, 0 without one                                         */
    int32_t reserved;
    long long rowbytes;        /* of an inflated row without its filter byte                     */
} ck_png_info;
/* host only: the chunk walk alone -> *info */
int ck_png_header(const uint8_t* data, size_t len, ck_png_info* info);
/* host only: everything the host does for a file -- the walk, the inflate, the sizes, the filter bytes -> *info */
int ck_png_probe(const uint8_t* data, size_t len, ck_png_info* info);
/* host only: a zlib stream -> its bytes.  The first cap of them go to out, *total counts all of them (call again with more
 * room when it is above cap); the verdict -- wrapper, blocks, distances, Adler-32 -- is zlib's and does not depend on cap */
int ck_png_inflate(const uint8_t* data, size_t len, uint8_t* out, size_t cap, size_t* total);
/* n files in HOST memory, all of the first one's height and width, each of its own colour type, depth and palette
 * -> BGR n x h x w x 3 in out_space.  *bad_frame (nullable): the file a CK_ERR_DATA is about, else -1 */
int ck_png_decode(ck_ctx* ctx, const uint8_t* const* data, const size_t* len, int n, uint8_t* bgr, int out_space, int32_t* bad_frame);
/* the most bytes ck_png_encode writes for one frame */
int ck_png_encode_bound(int h, int w, size_t* bytes);
/* BGR n x h x w x 3 in in_space -> n files at out + f * stride (HOST memory), len[f] bytes each.  filter: 0 .. 4 forces None /
 * Sub / Up / Avg / Paeth, -1 chooses per row.  stride must be at least ck_png_encode_bound */
int ck_png_encode(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space, int filter, uint8_t* out, size_t stride, size_t* len);
/* host only: ck_png_encode through the same steps in plain loops over host memory, the same bytes */
int ck_png_encode_staged(const uint8_t* bgr, int n, int h, int w, int filter, uint8_t* out, size_t stride, size_t* len);
/* The runs mode, on request: inside a band every maximal run of n equal filtered bytes is one literal and, for the n - 1
 * bytes behind it, matches of distance 1 -- as many of length 258 as fit, then one of the rest where it is 3 or more, else
 * one or two literals: what zlib's Z_RLE (cv2.imwrite's strategy) gains on flat images.  Runs cross rows, never a band's
 * edge.  The block header then declares 286 literal/length codes and two distance codes of one bit; the same pixels come
 * back, ck_png_encode_bound holds for both modes, and the literal-only mode's bytes are what they were. */
enum { CK_PNG_MATCH_NONE = 0, CK_PNG_MATCH_RUNS = 1 };
/* what ck_png_encode writes from now on; a new context has CK_PNG_MATCH_NONE */
int ck_png_set_encode_matches(ck_ctx* ctx, int mode);
/* host only: ck_png_encode_staged in either mode (matches: CK_PNG_MATCH_*) */
int ck_png_encode_staged_mode(const uint8_t* bgr, int n, int h, int w, int filter, int matches, uint8_t* out, size_t stride, size_t* len);
/* the tokens of the last ck_png_encode of this context, which took n frames: literals[f] and matches[f] of frame f (the
 * end-of-block symbols are not counted), read from the histograms its count step left in HBM */
int ck_png_run_stats(ck_ctx* ctx, int n, long long* literals, long long* matches);
/* the seams of the PNG kernels: rows of an encoder band, bytes of its bit-packing tile, bytes of the unfilter kernel's chunk,
 * rows of its workgroup */
int ck_png_tiles(int32_t* band_rows, int32_t* tile_bytes, int32_t* chunk_bytes, int32_t* group_rows);
/* The device inflate, on request: one wave per zlib stream decodes, for every bit offset of a window, the token that would
 * start there, follows the chain of real tokens, and applies them to a ring of 32768 bytes in LDS, from which the inflated
 * rows go to where the unfilter kernel reads them; only the zlib streams go up.  It accepts and refuses the same files as
 * the host mode, with the same frame, message and pixels.  A single stream can use one wave only: the mode is for batches. */
enum { CK_PNG_INFLATE_HOST = 0, CK_PNG_INFLATE_DEVICE = 1 };
/* where ck_png_decode inflates from now on; a new context has CK_PNG_INFLATE_HOST */
int ck_png_set_inflate(ck_ctx* ctx, int mode);
/* host only: ck_png_inflate through the steps of the device inflate in plain loops, in the kernel's order: the same bytes,
 * status and message.  h > 0: the stream holds h rows of 1 + rowbytes bytes, and the two checks of the PNG reader (enough
 * bytes, filter bytes up to 4) follow.  cause (nullable): 0 or the cause of the refusal; produced (nullable): the bytes
 * inflated, for a refused stream those in front of what was refused */
int ck_png_inflate_staged(const uint8_t* data, size_t len, uint8_t* out, size_t cap, size_t* total, int h, long long rowbytes,
                          int32_t* cause, long long* produced);
/* the inflate kernel alone on n zlib streams in HOST memory: the first cap[f] bytes of stream f go to out + f * stride (HOST
 * memory), total[f] counts all of them (0 for a refused stream), cause[f] and produced[f] are those of ck_png_inflate_staged.
 * A refused stream does not fail the call; nothing is written to out for it */
int ck_png_inflate_device(ck_ctx* ctx, const uint8_t* const* z, const size_t* zlen, int n, uint8_t* out, const size_t* cap, size_t stride,
                          size_t* total, int32_t* cause, long long* produced);
/* the bytes the last ck_png_decode of this context copied to the device, all passes, in either mode */
int ck_png_uploaded_bytes(ck_ctx* ctx, long long* bytes);
/* the last ck_png_decode in device mode or ck_png_inflate_device of this context: stats[0] streams, [1] window steps,
 * [2] tokens (literals and matches), [3] bytes produced */
int ck_png_inflate_stats(ck_ctx* ctx, long long* stats);
/* the seams of the inflate kernel: the bit offsets of a window step, the bytes that leave the ring at a time */
int ck_png_inflate_geometry(int32_t* window_bits, int32_t* flush_bytes);

/* ---- overlays: the finders' debug drawing (cv2.line / circle / rectangle / putText)   core/imgutil.py:71-118,
 * board/boardfinder.py:121-134, stone/stonesfinder.py:779-885, core/video.py:223-271
 * A display list is an ordered list of primitives per image, drawn in place by one kernel in which pixels own the work.
 *   prims       int32 [P][8] = {kind, x0, y0, x1, y1, size, colour, aux}; colour = b | g << 8 | r << 16 | alpha << 24
 *               (on a one-channel image the colour is its b byte)
 *   frame_start int32 [n + 1], CSR: frame f owns prims[frame_start[f] : frame_start[f + 1]]
 *   text        the bytes of every CK_OV_TEXT primitive: aux is its offset there, x1 its length
 * Coordinates are integer pixel positions, may lie outside the image, and the picture is clipped per pixel.  Every rule
 * is a per-pixel membership test in integer arithmetic ("Overlays", has them in full):
 *   CK_OV_SEGMENT (x0,y0)-(x1,y1), size = thickness t, odd: the 8-connected Bresenham path with OpenCV's LineIterator
 *               error rule, taken from the lexicographically smaller endpoint; major position i = 0 .. D visits minor
 *               offset floor((2 d i + D - 1) / (2 D)), D = max(|dx|, |dy|), d = min; dilated by a t x t square
 *   CK_OV_DISC  centre (x0,y0), size = radius r: dx^2 + dy^2 <= r^2 + r
 *   CK_OV_CIRCLE centre (x0,y0), size = r, x1 = thickness t, odd: in disc(r + (t - 1) / 2) and not in disc(r - (t + 1) / 2);
 *               a negative radius is the empty set
 *   CK_OV_RECT  corners inclusive, in either order; size = thickness inwards from the outline, 0: filled
 *   CK_OV_TEXT  (x0,y0) = top-left of the first cell, size = integer scale s: cells of 6s x 8s, the 5 x 7 glyph of the
 *               project's own font (csrc/ck_font5x7.h) in the cell's top-left; bytes outside 32 .. 126 draw '?'
 * Painted in list order: alpha 255 replaces the pixel, alpha 1 .. 254 leaves (c alpha + p (255 - alpha) + 127) / 255 per
 * channel, p as the earlier primitives of the call left it.  CK_ERR_ARG, before anything is launched, for an unknown kind,
 * |coordinate| > 32767, t even or above 15, r outside 0 .. 4095, s outside 1 .. 8, alpha 0, a text range outside the
 * byte string, a frame_start that is not monotone from 0, and c outside {1, 3}.  n = 0 and empty lists draw nothing. */
enum { CK_OV_SEGMENT = 1, CK_OV_CIRCLE = 2, CK_OV_DISC = 3, CK_OV_RECT = 4, CK_OV_TEXT = 5 };
/* draws on n images of h x w x c (in `space`), in place; prims, frame_start and text are in HOST memory */
int ck_overlay_draw(ck_ctx* ctx, uint8_t* img, int n, int h, int w, int c, int space,
                    const int32_t* prims, const int32_t* frame_start, const uint8_t* text, int text_len);
/* the plan ck_overlay_draw runs (host only): validates the list and bins it.  The image is cut into square bins of
 * *bin_size pixels, ceil(h / bin_size) rows of ceil(w / bin_size), numbered row by row, frame after frame; bin b owns
 * bin_prims[bin_start[b] : bin_start[b + 1]]: the indices (into prims) of the primitives of its frame whose bounding box
 * meets it, ascending.  *n_refs is the length of bin_prims.  bin_start (n * bins + 1 entries) and bin_prims may be NULL:
 * only the two sizes are returned.  CK_ERR_CAPACITY when bin_prims is given and cap < *n_refs (nothing is written to it). */
int ck_overlay_plan(int n, int h, int w, const int32_t* prims, const int32_t* frame_start, int text_len,
                    int32_t* bin_size, int32_t* bin_start, int32_t* bin_prims, int cap, int32_t* n_refs);
/* the seven row bytes of the glyph of byte ch (bit 4 = leftmost column), '?' for a byte outside 32 .. 126 (host only) */
int ck_overlay_glyph(int ch, uint8_t rows[7]);

/* ---- frame downsampling: CaptureReaderBase.downsample's cv2.pyrDown(img)   core/vmanager.py:484-498
 * OpenCV 3.1.0 pyrDown of 8-bit 3-channel frames, BORDER_DEFAULT, applied `levels` times: per level h x w becomes
 * (h+1)/2 x (w+1)/2 and dst[y,x] = (sum_{i,j=-2..2} k[i] k[j] src[r(2y+i), r(2x+j)] + 128) >> 8 with k = 1 4 6 4 1 and
 * r = BORDER_REFLECT_101 -- integer and exact.  out: n frames of the last level.
 * CK_ERR_ARG for levels < 1 and for a level that would read an image with a side below 2.
 * The second form takes I420 frames (h, w even, else CK_ERR_ARG) and equals ck_pyr_down of ck_i420_to_bgr bit for
 * bit; its first level converts and filters in one kernel, so the full-size BGR frames are never written. */
int ck_pyr_down(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int levels,
                int in_space, uint8_t* out, int out_space);
int ck_i420_to_bgr_pyr(ck_ctx* ctx, const uint8_t* i420, int n, int h, int w, int levels /* >= 1 */,
                       int in_space, uint8_t* bgr, int out_space);

/* ---- K7  cv2.getPerspectiveTransform(src4, dst4)            board/boardfinder.py:43-45
 * host only; src/dst 4x2 float32, M 3x3 float64 row-major. */
int ck_get_perspective_transform(const float* src4, const float* dst4, double* M9);

/* ---- K8  cv2.warpPerspective(frame, M, (dsize,dsize))         stone/stonesfinder.py:140
 * M: host, m_count x 9 doubles (m_count == 1: shared by all frames, else == n). */
int ck_warp_perspective(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space,
                        const double* M, int m_count, int dsize,
                        uint8_t* out, int out_space);

/* ---- K9  BackgroundSubtractorMOG2(detectShadows=False).apply stone/stonesfinder.py:113-115,171-176
 * one model per stream; stateful, frames must be applied in order. */
int ck_mog2_create(ck_ctx* ctx, int h, int w, int* handle);
int ck_mog2_apply(ck_ctx* ctx, int handle, const uint8_t* img3, int in_space,
                  double learning_rate, uint8_t* fgmask, int out_space);
int ck_mog2_destroy(ck_ctx* ctx, int handle);
/* the model's mixture, copied to HOST memory in the kernel's structure-of-arrays layout (npx = h * w, px = y * w + x):
 * weight[k*npx + px], variance[k*npx + px], mean[(k*3 + c)*npx + px] for the 5 mode slots k, nmodes[px].  Slots at or
 * above nmodes[px] hold no live mode and are unspecified.  Any pointer may be NULL (that array is skipped). */
int ck_mog2_get_state(ck_ctx* ctx, int handle, float* weight, float* variance, float* mean, uint8_t* nmodes);

/* ---- K10..K12 stone classifier                stone/nn_manager.py:216-298, nn_cache.py:16-52
 * weights: 12 float32 arrays in Keras-1 'tf' layout, order
 *   c1w[5,5,3,32] c1b c2w[5,5,32,32] c2b c3w[3,3,32,90] c3b c4w[3,3,90,90] c4b
 *   d1w[3240,160] d1b d2w[160,81] d2b
 * (conv kernels are applied as true convolutions, as Keras-1 on Theano does).
 * `space` may be CK_DEVICE: e.g. data_ptr() of PyTorch-ROCm tensors. */
int ck_cnn_set_weights(ck_ctx* ctx, const float* const weights[12], int space);
int ck_cnn_set_mode(ck_ctx* ctx, int mode);      /* CK_CNN_F16X2 (default): f32 operands split into hi + lo fp16, three fp16 MFMAs per product,
                                                    f32 accumulate -- as close to a float64 evaluation as the f32 chain is (profiles/r01_cnn_precision.txt);
                                                    CK_CNN_FP32: k-ordered f32 MFMA chain; CK_CNN_BF16: bf16 operands;
                                                    CK_CNN_F16Q8 (opt-in): the split of CK_CNN_F16X2 with its two cross terms (2^-11 of a product)
                                                    rounded to e4m3 and issued as one block-scaled MFMA per two taps -- a quarter faster, the
                                                    filter maps within 5e-5 of their scale instead of 1e-6; out-of-range values fall back */
/* goban: n x 380 x 380 x 3.  Any of y (n*100*81 softmax), labels (n*361, 0=E 1=B 2=W),
 * conf (n*361 doubles, max(y)/sum(y)) may be NULL. */
int ck_cnn_predict(ck_ctx* ctx, const uint8_t* goban, int n, int in_space,
                   float* y, uint8_t* labels, double* conf, int out_space);
/* The classifier's intermediate filter maps, for inspection and parity tests ("intermediate float filter maps within
 * 1e-4"): what the network of create_net (nn_manager.py:280-295) holds after its two MaxPooling2D layers, as computed by
 * the kernels of the context's mode, channels-last float32 in HOST memory:
 *   pool2 (n*100*16*16*32): relu(conv2(relu(conv1(x)))) max-pooled 2x2   (nn_manager.py:281-286)
 *   pool4 (n*100*6*6*90):   ... relu(conv4(relu(conv3(.)))) max-pooled 2x2 (nn_manager.py:287-292), the Flatten input
 * Region order i*10+j as everywhere; either may be NULL; n <= 128 (one chunk of the classifier's frame loop). */
int ck_cnn_maps(ck_ctx* ctx, const uint8_t* goban, int n, int in_space, float* pool2, float* pool4);

/* ---- training of the stone classifier: NNManager.train                       stone/nn_manager.py:133-214, 277-298
 * A trainer is a handle on a context (like a MOG2 model): f32 master weights, both Adam moments and the number of updates
 * applied.  One step = forward pass of the network of create_net on raw 0..255 BGR patches, softmax + categorical
 * cross-entropy (mean over the batch), backward pass, Adam (lr per call, beta1 0.9, beta2 0.999, eps 1e-8, no decay, bias-corrected
 * as Keras-1: lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t), w -= lr_t m / (sqrt(v) + eps)).  The gradients' products run on the f32-input MFMA, the forward
 * pass on the f64 MFMA rounded once to f32 (its ReLU and pool decisions are then those of exact arithmetic wherever f32 can tell
 * the values apart), all with fixed summation orders: the same patches, labels, seed and step number give the same bits in every weight.
 * x: n x h x w x c patches in `in_space` -- anything but n >= 1, h = w = 40, c = 3 is CK_ERR_ARG; labels: HOST, n class indices
 * 0 .. 80 (above 80: CK_ERR_ARG); any n fits (the batch goes through in chunks of 256 patches).
 * dropout != 0: 0.25 behind each pool and 0.5 behind dense 1, kept units divided by 1 - p; the keep-mask is a counter-based
 * function of (seed, step, layer, unit index) with no state, step = the number of updates the trainer has applied.
 * weights / grads / moments: 12 arrays in the order and layouts of ck_cnn_set_weights. */
int ck_train_create(ck_ctx* ctx, const float* const weights[12], int space, int* handle);
int ck_train_destroy(ck_ctx* ctx, int handle);
/* gradients of the batch, then one Adam update; *loss: the mean loss before the update */
int ck_train_step(ck_ctx* ctx, int handle, const uint8_t* x, const uint8_t* labels, int n, int h, int w, int c, int in_space,
                  double lr, int dropout, uint64_t seed, float* loss);
/* the inspection call (the counterpart of ck_cnn_maps): the same gradients, no update.  step < 0: the trainer's own count.
 * Outputs on the HOST, each nullable: grads (12 arrays), and with dropout the keep-masks (1 kept, 0 dropped) behind pool 1
 * (n x 16 x 16 x 32), pool 2 (n x 6 x 6 x 90) and dense 1 (n x 160). */
int ck_train_grads(ck_ctx* ctx, int handle, const uint8_t* x, const uint8_t* labels, int n, int h, int w, int c, int in_space,
                   int dropout, uint64_t seed, long long step, float* loss, float* const grads[12],
                   uint8_t* mask1, uint8_t* mask2, uint8_t* mask3);
/* one Adam update from 12 gradient arrays on the HOST */
int ck_train_apply(ck_ctx* ctx, int handle, const float* const grads[12], double lr);
int ck_train_get_weights(ck_ctx* ctx, int handle, float* const weights[12]);                 /* to the HOST */
/* first moments m, second moments v (each nullable, 12 HOST arrays), *steps = updates applied */
int ck_train_get_adam_state(ck_ctx* ctx, int handle, float* const m[12], float* const v[12], long long* steps);
/* hand the trainer's current weights to the context's classifier (ck_cnn_set_weights from device memory): ck_cnn_predict
 * and the other inference calls then run on them */
int ck_train_handover(ck_ctx* ctx, int handle);

/* ---- training data from goban images: NNManager.generate_xs / generate_ys for the regions whose label is certain
 *      (stone/nn_manager.py:220-254), selected and cut where the images lie.
 * goban: n x 380 x 380 x 3 in `in_space`; fgcount: n x 361 int32 foreground counts (ck_mog2_band_run / ck_zone_counts) in
 * `fg_space`; state_of: HOST, n int32 -- the reference position frame i shows, < 0: the frame is not harvested; positions:
 * HOST, n_pos x 361 codes 0 E / 1 B / 2 W.  Region q = 10 ri + cj of frame i is kept when state_of[i] >= 0, the counts of its
 * 2 x 2 zones (rows rs(ri).., columns rs(cj).., rs = 0, 2, .., 16, 17) sum to <= calm_max, and -- for a region whose label is
 * 0 -- hash(seed, first_frame + i, q) & 255 < empty_keep (0: no empty region, 256: all; the hash is stateless, so what is
 * kept does not depend on how a film is cut into calls).  label = the base-3 number of the block, (0,0) least significant,
 * then (0,1), (1,0), (1,1).  Outputs in `out_space`, in ascending (frame, region) order: x cap x 40 x 40 x 3 (the window at
 * pixel (20 rs(ri), 20 rs(cj))), labels cap bytes, src cap x 2 int32 (i, q).  *n_found: the number of kept regions; only
 * the first min(*n_found, cap) rows of the outputs are written.  CK_ERR_ARG before any launch: a code > 2,
 * state_of[i] >= n_pos, empty_keep outside 0 .. 256, cap < 0.  n = 0 is fine. */
int ck_harvest_patches(ck_ctx* ctx, const uint8_t* goban, int n, int in_space, const int32_t* fgcount, int fg_space,
                       const int32_t* state_of, const uint8_t* positions, int n_pos, int calm_max, int empty_keep, uint32_t seed,
                       long long first_frame, uint8_t* x, uint8_t* labels, int32_t* src, int cap, int out_space, int32_t* n_found);
/* x_out[k] = numpy.rot90(x[k], t[k] & 3, axes=(0, 1)), its columns mirrored when t[k] & 4; x: n x 40 x 40 x 3 in `in_space`,
 * t: HOST, n codes 0 .. 7 (above: CK_ERR_ARG), x_out in `out_space`, which may not overlap x (CK_ERR_ARG). */
int ck_augment_patches(ck_ctx* ctx, const uint8_t* x, int n, int in_space, const uint8_t* t, uint8_t* x_out, int out_space);

/* ---- K8 + K10..K12: frame + M -> 19x19 labels   stonesfinder.py:140 + nn_cache.py:33-41 */
int ck_stones_detect(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space,
                     const double* M, int m_count, uint8_t* labels, double* conf,
                     int out_space);

/* ---- the classifier's answers per REGION: what NNCache.predict_4_stones / predict_stone read (stone/nn_cache.py:16-31).
 * region_label: n*100 argmax labels (0..80, region (i, j) at i*10+j); region_conf: n*100 doubles max(y)/sum(y). */
int ck_cnn_regions(ck_ctx* ctx, const uint8_t* goban, int n, int in_space,
                   uint8_t* region_label, double* region_conf, int out_space);

/* ---- an ORDERED RUN of the stones path over n consecutive frames of one stream, one call:
 *      K8 warp -> K9 MOG2 in frame order -> K10..K12            stone/stonesfinder.py:123-176 + sf_neural.py:37-55
 * mog2_handle < 0: no background model (fgcount untouched).  learning_rates: host, n doubles (0.01 during the
 * first bg_init_frames frames, 0.005 afterwards: stonesfinder.py:171-176).  fgcount: n*361 int32, the number of
 * foreground pixels of the frame's MOG2 mask inside StonesFinder.getrect(r, c) -- what SfNeural.is_agitated sums
 * (sf_neural.py:178-180).  labels / conf (n*361, as ck_stones_detect) may be NULL.  Feeds ck_policy_run. */
int ck_stones_run(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space,
                  const double* M, int m_count, int mog2_handle, const double* learning_rates,
                  uint8_t* region_label, double* region_conf, int32_t* fgcount,
                  uint8_t* labels, double* conf, int out_space);

/* ---- the fixed-size per-frame RESULT RECORD of the fast-file path (SURVEY 8e "Collective": labels + conf + n_lines +
 * lines, Lmax = 64): what the stateless core of one frame leaves for the ordered fold -- the board half is what
 * BoardFinderAuto._detect reads after the image chain (board/bf_auto.py:76-84, 125-135), the stones half what
 * NNCache.predict_4_stones reads (stone/nn_cache.py:16-31).  The two entry points below write their half of n records IN
 * PLACE, in host memory or in HBM (`rec_space`), and leave the other half untouched: with the records in HBM a multi-GPU
 * host gathers them to the folding rank without a host copy on the other ranks (camkifu_amd/pipeline.py).
 * lines beyond min(n_lines, CK_REC_LMAX) are zero; flags: CK_REC_LINES_CUT when n_lines > CK_REC_LMAX (the strongest
 * CK_REC_LMAX lines are kept: OpenCV's order is most votes first). */
#define CK_REC_LMAX 64
enum { CK_REC_LINES_CUT = 1, CK_REC_FAILED = 2 };
typedef struct ck_frame_record {
    int32_t status;                   /* CK_BOARD_*                                      board half: 536 bytes */
    int32_t n_contours;
    int32_t n_lines;
    int32_t flags;                    /* CK_REC_*                                                             */
    double  biggest_area;
    float   lines[CK_REC_LMAX][2];    /* (rho, theta)                                                         */
    double  region_conf[100];         /* max(y) / sum(y), region (i, j) at i*10+j       stones half: 900 bytes */
    uint8_t region_label[100];        /* argmax label 0..80                                                   */
    uint8_t pad[4];
} ck_frame_record;                    /* 1440 bytes, no implicit padding                                      */
/* K1..K6 of n frames -> the board half of rec[0 .. n)                                board/bf_auto.py:72-84, 125-135 */
int ck_board_detect_records(ck_ctx* ctx, const uint8_t* bgr, int n, int h, int w, int in_space,
                            int hough_thresh, ck_frame_record* rec, int rec_space);
/* K10..K12 of n goban images -> the stones half of rec[0 .. n)                         stone/nn_cache.py:16-31 */
int ck_cnn_regions_records(ck_ctx* ctx, const uint8_t* goban, int n, int in_space,
                           ck_frame_record* rec, int rec_space);

/* ---- K9 sharded by PIXEL for multi-GPU batches: the model `handle` (ck_mog2_create(band_h, 380)) holds a horizontal band
 * of the goban image (a whole number of 20-pixel intersection rows; the last band is the one that ends at pixel row
 * 379).  band: n x band_h x 380 x 3, the band of n consecutive goban images in frame order; counts: n x (band_h/20
 * rounded up) x 19 int32 foreground pixels per intersection zone, the same numbers ck_stones_run gives for those rows. */
int ck_mog2_band_run(ck_ctx* ctx, int handle, const uint8_t* band, int n, int in_space,
                     const double* learning_rates, int last_band, int32_t* counts, int out_space);

/* ---- the 361 box sums of SfNeural.mark_targets / select_targets as one reduction   stone/sf_neural.py:72-83, 129-154
 * mask: n x 380 x 380 (non-zero = foreground); counts: n*361 int32 (pixels per getrect zone). */
int ck_zone_counts(ck_ctx* ctx, const uint8_t* mask, int n, int in_space, int32_t* counts, int out_space);

/* ---- SfContours.find_stones for n goban images in one call                         stone/sf_contours.py:48-111
 * (with analyse_fg :207-249, extract_contours_fg :251-300, _filter_contours :186-205, _find_centers :302-330,
 * find_color :128-184).  goban: n x side x side x 3 BGR, fg: n x side x side foreground masks (StonesFinder.get_foreground),
 * both in `in_space`.  rects: HOST, 19*19*4 int32 = StonesFinder.getrect(r, c) as (x0, y0, x1, y1), x along rows -- the
 * caller's grid, so a learnt PosGrid is honoured; rows [rs, re) and columns [cs, ce) are analysed, as the keyword
 * arguments of the reference method say.  Outputs on the HOST: stones n*19*19 (0 E, 1 B, 2 W; E outside the range),
 * zones (nullable) n*(re-rs)*(ce-cs)*4 int16 = the method's `zones` array, mask (nullable) n*hs*ws bytes = the hull
 * mask of the analysed view (hs = x1 - x0, ws = y1 - y0 of the range's corner rectangles).
 * CK_ERR_STATE where the reference itself raises (_find_centers dividing by a zero cell count). */
int ck_contour_stones(ck_ctx* ctx, const uint8_t* goban, const uint8_t* fg, int n, int side, int in_space, const int32_t* rects,
                      int rs, int re, int cs, int ce, uint8_t* stones, int16_t* zones, uint8_t* mask);

/* ---- SfClustering.find_stones for m jobs in one call                               stone/sf_clustering.py:48-168
 * A job is one region of one goban image: jobs = m x 5 int32 on the HOST (image index, rs, re, cs, ce), rows [rs, re) and
 * columns [cs, ce) of the intersections.  Per job: cv2.kmeans(pixels of the region's view, 3, None, (EPS, 15, 3), 3,
 * KMEANS_PP_CENTERS), the labels under the circle mask counted per zone, interpret_ratios, check_density.
 * goban: n x side x side x 3 in `in_space`, uint8 (is_f32 = 0) or float32 (is_f32 = 1: what SfClustering._find accumulates).
 * rects: HOST, the 19*19*4 getrect table as for ck_contour_stones; mask: HOST, side x side bytes, StonesFinder.getmask().
 * Outputs on the HOST, one row per job: stones 361 (0 E, 1 B, 2 W; E outside the region), trusted 1 (check_density; 0 also
 * where the compactness is 0 -- the reference fails there -- and the stones are then all E); nullable: ratios 361*3,
 * centers 9 floats (winning attempt, cluster order), labels (the winning attempt's label per pixel of the view, job after
 * job, labels_cap bytes available), passes 3 and compactness 3 (per attempt), winner 1 (the attempt kept).
 * Random numbers: the context holds a cv::RNG state (initially 0xffffffff, the library's default seed); a job draws 21
 * numbers, job j of a call starts 21 * j draws in, and the call leaves the state advanced by 21 * m.
 * CK_ERR_ARG: empty or out-of-range region, a view outside the image, a zone outside its view, fewer than 3 pixels. */
int ck_cluster_stones(ck_ctx* ctx, const void* goban, int n, int side, int is_f32, int in_space, const int32_t* rects,
                      const uint8_t* mask, const int32_t* jobs, int m, uint8_t* stones, uint8_t* trusted, uint8_t* ratios,
                      float* centers, uint8_t* labels, long long labels_cap, int32_t* passes, double* compactness, int32_t* winner);
int ck_rng_get(ck_ctx* ctx, uint64_t* state);
int ck_rng_set(ck_ctx* ctx, uint64_t state);

/* ---- cv2.findContours(edges, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) as SfContours reads it   stone/sf_contours.py:82, 266
 * For n edge maps (h x w, non-zero = edge): counts[f] = contours of map f; table: one row of 4 int32 per contour, map after
 * map, each map's contours in the order cv2 returns them (last found first): x, y of the contour's first point, the
 * length of its compressed vertex list (cont.shape[0]), the number of outer-border pixels; points (nullable): those
 * pixels as x, y pairs, contour after contour (the set drawContours(thickness=1) paints).  All outputs on the HOST. */
int ck_contours_external(ck_ctx* ctx, const uint8_t* edges, int n, int h, int w, int in_space,
                         int32_t* counts, int32_t* table, int table_cap, int32_t* points, int points_cap);

/* ---- StonesFinder.find_intersections for n goban images in one call                stone/stonesfinder.py:516-552
 * grey image, Otsu level, Canny(gray, level / 2, level), then cv2.HoughLinesP(zone, 1, pi / 180, int(3/4 side),
 * minLineLength=int(2/3 side), maxLineGap=0) in each of the 361 getrect zones and update_grid (:888-947) on what it finds.
 * goban: n x side x side x 3 BGR in `in_space`; mtx: HOST 19*19*2 int16 = PosGrid.mtx; rects: HOST 19*19*4 int32 =
 * StonesFinder.getrect(r, c).  Outputs on the HOST: grid n*19*19*2 int16 = the method's return value (positions negated
 * where a line was found, moved where a cross was found); nullable: lines n*361*CK_ZONE_LINES*4 int16 (x0, y0, x1, y1 per
 * line, in the order found), nlines n*361 int32, edges n*side*side (the Canny map). */
#define CK_ZONE_LINES 32
int ck_find_intersections(ck_ctx* ctx, const uint8_t* goban, int n, int side, int in_space, const int16_t* mtx, const int32_t* rects,
                          int16_t* grid, int16_t* lines, int32_t* nlines, uint8_t* edges);

/* update_grid for one zone (host only, no GPU needed)                                 stone/stonesfinder.py:888-947
 * lines: k x (x0, y0, x1, y1) in the zone's own coordinates, box: getrect of the zone, slot: the intersection's int16
 * (x, y), updated in place.  CK_ERR_ARG for a zero-length line (the reference divides by zero there). */
int ck_update_grid(const int32_t* lines, int k, const int32_t* box, int16_t* slot);

/* ======================================================================================================
 * Ordered (stateful) halves of the two finders -- host only, no GPU needed.  The per-frame finders call
 * them once per frame, the batch pipeline's fold calls them over the gathered per-frame records; the
 * arithmetic is the reference's Python float arithmetic restated operation for operation.
 * ====================================================================================================== */

/* ---- BoardFinderAuto._detect after the image chain: 4-frame line accumulation, group_intersections,
 *      connect_clusters, updt_corners                     board/bf_auto.py:76-102, 143-217; core/imgutil.py:38-68, 216-288, 464-530
 * status/lines/n_lines: this frame's result of ck_board_detect; frame_counter: VidProcessor.total_f_processed;
 * cur_hull: the 4 corners known so far (8 ints, x y) or NULL (GobanCorners.hull is None).
 * Out: *found (the return value of _detect), *update (corners must be replaced by `centers`),
 * centers (up to 4 x y pairs, hull-ordered), *n_centers, stats[2] = {clusters, intersections} or -1 when the
 * frame did not reach the grouping step.  CK_ERR_STATE: the reference would raise here (3-vertex hull indexed as 4). */
/* imgutil.get_ordered_hull (core/imgutil.py:236-288): convex hull of n integer points, clockwise on screen,
 * starting at the vertex nearest the image origin; out holds up to n x y pairs */
int  ck_ordered_hull(const int32_t* pts, int n, int32_t* out, int32_t* n_out);
typedef struct ck_boardfold ck_boardfold;
int  ck_boardfold_create(ck_boardfold** out);
void ck_boardfold_destroy(ck_boardfold* bf);
int  ck_boardfold_reset(ck_boardfold* bf);
int  ck_boardfold_step(ck_boardfold* bf, int h, int w, int status, const float* lines, int n_lines,
                       long long frame_counter, const int32_t* cur_hull, int32_t* found, int32_t* update,
                       int32_t* centers, int32_t* n_centers, int32_t* stats);

/* test hooks: Python's round(x, 10) as the fold computes it (integer arithmetic, exact) and by the long way (the decimal
 * string and back) -- tests hold the two, and CPython's own round, equal */
double ck_round10(double x);
double ck_round10_reference(double x);
/* The same fold over the board halves of n gathered records (ck_frame_record), frames *k_io .. n-1, with the hold-off
 * after a hit as a FRAME COUNT (the reference's 10 s of wall clock, bf_auto.py:43-49, for a file read at file_fps):
 * frames inside the hold-off are not looked at; every other frame goes through ck_boardfold_step with *counter_io as
 * its frame_counter.  order (nullable): frame k's record is recs[order[k]] -- the gather leaves the records rank by
 * rank, frame f at row (f mod world) * rows_per_rank + 1 + f / world, and the fold reads them where they lie.
 * Returns with *k_io == n (batch done) or just after the first frame whose step says `update` (outputs as
 * ck_boardfold_step's): the caller replaces its corners, derives the transform, sets *hold_io after a hit and calls
 * again with the new hull.  A hit WITHOUT update leaves the corners -- hence the transform -- as they are: the fold then
 * starts the hold-off itself (*hold_io = hold_after_same_hit) and goes on; hold_after_same_hit < 0 returns such hits too.
 * seen_looked_io[2]: frames offered / looked at (running totals).  On an error *k_io is the frame that raised it: that
 * frame IS in seen_looked_io (both counts, like the reference's step), only *counter_io is not advanced over it, as an
 * exception out of _detect leaves total_f_processed. */
int  ck_boardfold_run(ck_boardfold* bf, int h, int w, const ck_frame_record* recs, const int32_t* order, int n, int32_t* k_io,
                      long long* counter_io, int32_t* hold_io, long long* seen_looked_io, const int32_t* cur_hull,
                      int hold_after_same_hit, int32_t* found, int32_t* update, int32_t* centers, int32_t* n_centers,
                      int32_t* stats);

/* ---- SfNeural._find after the classifier: predict_all / mark_targets / select_targets / predict_moves /
 *      get_color_ratio / lookback / HeatPoint                                  stone/sf_neural.py:37-244
 * Runs frames [*frame_io, n) of an ordered run.  Per frame: region_label (100 argmax labels 0..80, region (i, j)
 * at i*10+j), region_conf (100 x max(y)/sum(y)), fgcount (361 foreground-pixel counts of the MOG2 mask over
 * StonesFinder.getrect(r, c); NULL = nothing moves), first_counter = total_f_processed of frame 0 of the run.
 * board: the goban as the controller holds it NOW (361 bytes, 0 E / 1 B / 2 W).
 * The call returns either with *frame_io == n (run finished, *kind == 0) or with a request the caller must apply
 * before calling again with the updated board: *kind 1 = StonesFinder.suggest (one triple), 2 = bulk_update;
 * moves = *n_moves triples (color, row, col); *frame_io / *phase_io say where to resume (pass them back unchanged;
 * start a run with 0 / 0).  cap >= 722 triples. */
typedef struct ck_policy ck_policy;
int  ck_policy_create(int bg_init_frames, ck_policy** out);
void ck_policy_destroy(ck_policy* p);
int  ck_policy_run(ck_policy* p, int n, long long first_counter, const uint8_t* region_label,
                   const double* region_conf, const int32_t* fgcount, const uint8_t* board,
                   int32_t* frame_io, int32_t* phase_io, int32_t* kind, int32_t* moves, int cap, int32_t* n_moves);
/* ck_policy_run reading the classifier's answers from the stones halves of n gathered records where they lie (order as
 * for ck_boardfold_run, nullable; fgcount stays in frame order): same protocol, same results */
int  ck_policy_run_records(ck_policy* p, int n, long long first_counter, const ck_frame_record* recs, const int32_t* order,
                           const int32_t* fgcount, const uint8_t* board,
                           int32_t* frame_io, int32_t* phase_io, int32_t* kind, int32_t* moves, int cap, int32_t* n_moves);
/* inspection / test hooks: any out pointer may be NULL.  targets 361 B, heat_color 361 B (0 = no watched prediction),
 * heat_energy 361 int32, heat_conf 361 doubles, flags[2] = {has_sampled, recolour events seen} */
int  ck_policy_get_state(const ck_policy* p, uint8_t* targets, uint8_t* heat_color, int32_t* heat_energy,
                         double* heat_conf, int32_t* flags);
int  ck_policy_set_state(ck_policy* p, const uint8_t* targets, int has_sampled /* <0: keep */);
int  ck_policy_watch(ck_policy* p, int r, int c, int color /*0 drops it*/, double confidence, long long stamp);

#ifdef __cplusplus
}
#endif
#endif
