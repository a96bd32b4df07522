// k_jpeg_span.hip -- the Huffman stage of a baseline JPEG decode on the GPU, parallel INSIDE a strand: the five steps of
// ck_jpeg_span.h, the same code the host runs (ck_jpeg_span.cpp), each its own launch on the context's stream.  No kernel
// waits for another workgroup; what one step leaves in HBM the next reads.
//
//   speculate   one lane per (span, block slot guessed)     "jpeg_span_speculate" in the timing table
//   resolve     one lane per strand                         "jpeg_span_resolve"
//   write       one lane per span                           "jpeg_span_write"
//   dc          one workgroup of 256 lanes per strand       "jpeg_span_dc"
//   verdict     one lane per strand                         "jpeg_span_verdict"
//
// The three decoding kernels run workgroups of one wave.  Each stages ONE table set in LDS, that of its first lane's
// strand (6 x 1420 bytes), as jpeg_huff_kernel does; a lane whose strand has another set reads global memory through the
// same (generic) pointer type.  In a Motion-JPEG film all frames share one set.
//
// Bounds (ck_jpeg_span.h states and keeps them): every decode loop consumes at least one bit per step and ends at the end
// of the lane's span -- two spans plus one symbol for speculate, one span plus one symbol for resolve and write; a row is
// checked against the staged block before a byte of it is read (ck_span_row_ok) and the reader loads nothing at or behind
// its strand's end, so no load goes outside the staged block; write stores only for a block whose ordinal is below the
// strand's n_mcu * bpm and the row check holds first_mcu + n_mcu inside the frame, so no store goes outside the strand's
// frame; the resolve walk has as many steps as its strand has spans.  Lanes past the last span or strand return before
// they touch anything.
#include "ck_common.h"
#include "ck_jpeg_span.h"

namespace {

constexpr int SPAN_LANES = 64;
constexpr int DC_LANES = 256;
constexpr int SET_DWORDS = (int)(sizeof(CkHuffSet) / 4);

__device__ const uint8_t d_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22,
                                         15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the table set of strand `s` into LDS, by the whole workgroup -> its index (a row's set is checked by every step again)
__device__ long long stage_set(const CkSpanJob& J, int s, uint32_t* s_set)
{
    long long set0 = J.rows[s].table_set;
    if (set0 < 0 || set0 >= J.n_sets) set0 = 0;
    const uint32_t* src = (const uint32_t*)(J.sets + set0);
    for (int i = threadIdx.x; i < SET_DWORDS; i += SPAN_LANES) s_set[i] = src[i];
    __syncthreads();
    return set0;
}

__global__ __launch_bounds__(SPAN_LANES) void span_speculate_kernel(CkSpanJob J, long long n_spans)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_set[SET_DWORDS];
    const long long first = (long long)blockIdx.x * SPAN_LANES;             // (first / bpm < n_spans: the grid is sized so)
    const long long set0 = stage_set(J, ck_span_strand(J, first / J.bpm), s_set);
    const long long lane = first + threadIdx.x;
    if (lane >= n_spans * J.bpm) return;
    ck_span_speculate(J, lane / J.bpm, (int)(lane % J.bpm), (const CkHuffSet*)s_set, set0);
}

__global__ __launch_bounds__(SPAN_LANES) void span_resolve_kernel(CkSpanJob J)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_set[SET_DWORDS];
    const int first = blockIdx.x * SPAN_LANES;
    const long long set0 = stage_set(J, first, s_set);
    const int s = first + (int)threadIdx.x;
    if (s >= J.n_strands) return;
    ck_span_resolve(J, s, (const CkHuffSet*)s_set, set0);
}

__global__ __launch_bounds__(SPAN_LANES) void span_write_kernel(CkSpanJob J, long long n_spans)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_set[SET_DWORDS];
    __shared__ uint8_t s_zigzag[64];
    const long long first = (long long)blockIdx.x * SPAN_LANES;
    s_zigzag[threadIdx.x] = d_zigzag[threadIdx.x];
    const long long set0 = stage_set(J, ck_span_strand(J, first), s_set);
    const long long i = first + threadIdx.x;
    if (i >= n_spans) return;
    ck_span_write(J, i, s_zigzag, (const CkHuffSet*)s_set, set0);
}

// per component: every lane sums the differences of its run of blocks, lane 0 turns the 256 sums into the sums before each
// run, every lane writes the values of its run
__global__ __launch_bounds__(DC_LANES) void span_dc_kernel(CkSpanJob J)
{
    __shared__ long long s_sum[DC_LANES];
    const int s = blockIdx.x, t = threadIdx.x;
    const CkStrand r = J.rows[s];
    if (!ck_span_row_ok(J, r)) return;                           // (the whole workgroup: nobody waits below)
    int16_t* coef = J.coef + r.frame * J.cframe;
    bool out = false;
    for (int c = 0; c < J.g.ncomp; c++) {
        const long long cnt = ck_span_dc_count(J.g, r.n_mcu, c), chunk = (cnt + DC_LANES - 1) / DC_LANES;
        const long long t0 = t * chunk < cnt ? t * chunk : cnt, t1 = t0 + chunk < cnt ? t0 + chunk : cnt;
        s_sum[t] = ck_span_dc_sum(coef, J.g, r.first_mcu, c, t0, t1);
        __syncthreads();
        if (t == 0) {
            long long run = 0;
            for (int i = 0; i < DC_LANES; i++) { const long long v = s_sum[i]; s_sum[i] = run; run += v; }
        }
        __syncthreads();
        out |= ck_span_dc_apply(coef, J.g, r.first_mcu, c, t0, t1, s_sum[t]);
        __syncthreads();
    }
    if (out) atomicOr(&J.flags[s], (uint32_t)CK_SPANF_DC_RANGE);
}

__global__ __launch_bounds__(SPAN_LANES) void span_verdict_kernel(CkSpanJob J)
{
    const int s = blockIdx.x * SPAN_LANES + (int)threadIdx.x;
    if (s < J.n_strands) ck_span_verdict(J, s);
}

}  // namespace

int k_jpeg_span(ck_ctx* ctx, const CkSpanJob& J, long long n_spans)
{
    if (J.n_strands <= 0 || J.n_sets <= 0 || J.n_frames <= 0 || n_spans < J.n_strands || J.bpm < 1 || J.bpm > 6 ||
        J.span_bytes < CK_SPAN_MIN || J.span_bytes > CK_SPAN_MAX)
        return ck_fail(ctx, CK_ERR_ARG, "k_jpeg_span: nothing to decode");
    const long long cand = n_spans * J.bpm;
    if ((cand + SPAN_LANES - 1) / SPAN_LANES > 0x7fffffffLL) return ck_fail(ctx, CK_ERR_ARG, "k_jpeg_span: %lld spans in one pass", n_spans);
    CK_HIP(ctx, hipMemsetAsync(J.coef, 0, (size_t)J.n_frames * (size_t)J.cframe * sizeof(int16_t), ctx->stream));
    const dim3 wave(SPAN_LANES);
    const dim3 per_strand((unsigned)((J.n_strands + SPAN_LANES - 1) / SPAN_LANES));
    {
        TimeScope ts(ctx, "jpeg_span_speculate");
        hipLaunchKernelGGL(span_speculate_kernel, dim3((unsigned)((cand + SPAN_LANES - 1) / SPAN_LANES)), wave, 0, ctx->stream, J, n_spans);
        CK_HIP(ctx, hipGetLastError());
    }
    {
        TimeScope ts(ctx, "jpeg_span_resolve");
        hipLaunchKernelGGL(span_resolve_kernel, per_strand, wave, 0, ctx->stream, J);
        CK_HIP(ctx, hipGetLastError());
    }
    {
        TimeScope ts(ctx, "jpeg_span_write");
        hipLaunchKernelGGL(span_write_kernel, dim3((unsigned)((n_spans + SPAN_LANES - 1) / SPAN_LANES)), wave, 0, ctx->stream, J, n_spans);
        CK_HIP(ctx, hipGetLastError());
    }
    {
        TimeScope ts(ctx, "jpeg_span_dc");
        hipLaunchKernelGGL(span_dc_kernel, dim3((unsigned)J.n_strands), dim3(DC_LANES), 0, ctx->stream, J);
        CK_HIP(ctx, hipGetLastError());
    }
    {
        TimeScope ts(ctx, "jpeg_span_verdict");
        hipLaunchKernelGGL(span_verdict_kernel, per_strand, wave, 0, ctx->stream, J);
        CK_HIP(ctx, hipGetLastError());
    }
    return CK_OK;
}
