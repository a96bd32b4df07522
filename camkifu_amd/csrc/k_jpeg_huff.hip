// k_jpeg_huff.hip -- the Huffman stage of a baseline JPEG decode on the GPU: one lane decodes one strand (one restart
// interval of one frame) with the decoder of ck_jpeg_strand.h, the same code the host runs, into the coefficient layout
// k_jpeg.hip reads.  Strands come in plan order, frame-major, so the lanes of a wave work on neighbouring intervals of
// similar length.  A frame without restart intervals is one strand: one lane decodes it alone (correct, and slow).
//
// One workgroup = one wave = 64 strands.  It stages ONE table set in LDS, that of its first strand (6 x 1420 bytes), and
// the zigzag order; a lane whose strand has another set reads its tables from global memory through the same (generic)
// pointer type.  In a Motion-JPEG film all frames share one set, so every lane is on the LDS path.
//
// Bounds: every strand's byte range lies inside the staged block (the launcher's caller builds the rows from the plan,
// this kernel checks them against `bytes` again), the decoder reads nothing at or beyond `end`, and its stores land inside
// the strand's frame (ck_strand_decode checks first_mcu + n_mcu against the frame).  A row that fails a check gets the
// status CK_STRAND_ROW and nothing is decoded for it.
#include "ck_common.h"
#include "ck_jpeg_strand.h"

namespace {

constexpr int HUFF_LANES = 64;
constexpr int SET_DWORDS = (int)(sizeof(CkHuffSet) / 4);
static_assert(sizeof(CkHuffTab) == 1420 && sizeof(CkHuffSet) == 6 * 1420, "the table set as the planner packs it");
static_assert(sizeof(CkStrand) == 48, "a plan row is 6 int64");

__device__ const uint8_t d_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22,
                                         15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__global__ __launch_bounds__(HUFF_LANES) void jpeg_huff_kernel(const uint8_t* __restrict__ bytes, long long n_bytes,
                                                               const CkStrand* __restrict__ rows, int n_strands,
                                                               const CkHuffSet* __restrict__ sets, int n_sets,
                                                               CkStrandGeom g, long long cframe,
                                                               int n_frames, int16_t* __restrict__ coef, uint32_t* __restrict__ status)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_set[SET_DWORDS];
    __shared__ uint8_t s_zigzag[64];
    const int lane = threadIdx.x;
    const int first = blockIdx.x * HUFF_LANES;
    long long set0 = rows[first].table_set;                      // (first < n_strands: the grid is ceil(n_strands / 64))
    if (set0 < 0 || set0 >= n_sets) set0 = 0;
    const uint32_t* src = (const uint32_t*)(sets + set0);
    for (int i = lane; i < SET_DWORDS; i += HUFF_LANES) s_set[i] = src[i];
    s_zigzag[lane] = d_zigzag[lane];
    __syncthreads();
    const int s = first + lane;
    if (s >= n_strands) return;
    const CkStrand r = rows[s];
    uint32_t st;
    if (r.frame < 0 || r.frame >= n_frames || r.begin < 0 || r.end < r.begin || r.end > n_bytes || r.table_set < 0 || r.table_set >= n_sets) {
        st = ck_strand_status(CK_STRAND_ROW, 0);
    } else {
        const CkHuffSet* set = r.table_set == set0 ? (const CkHuffSet*)s_set : sets + r.table_set;
        st = ck_strand_decode(bytes + r.begin, bytes + r.end, g, r.first_mcu, r.n_mcu, set, s_zigzag, coef + r.frame * cframe);
    }
    status[s] = st;
}

}  // namespace

// d_bytes: the staged entropy-coded segments (n_bytes of them, zeroed slack behind); d_rows: n_strands plan rows whose
// begin / end are offsets into d_bytes; d_sets: n_sets table sets; d_coef: n_frames * cframe int16, zeroed on the stream
// here; d_status: n_strands words.  "jpeg_huff" in the timing table.
int k_jpeg_huff(ck_ctx* ctx, const uint8_t* d_bytes, long long n_bytes, const CkStrand* d_rows, int n_strands, const CkHuffSet* d_sets,
                int n_sets, const CkStrandGeom& g, long long cframe, int n_frames, int16_t* d_coef, uint32_t* d_status)
{
    if (n_strands <= 0 || n_sets <= 0 || n_frames <= 0) return ck_fail(ctx, CK_ERR_ARG, "k_jpeg_huff: nothing to decode");
    CK_HIP(ctx, hipMemsetAsync(d_coef, 0, (size_t)n_frames * (size_t)cframe * sizeof(int16_t), ctx->stream));
    TimeScope ts(ctx, "jpeg_huff");
    const dim3 grid((unsigned)((n_strands + HUFF_LANES - 1) / HUFF_LANES));
    hipLaunchKernelGGL(jpeg_huff_kernel, grid, dim3(HUFF_LANES), 0, ctx->stream, d_bytes, n_bytes, d_rows, n_strands, d_sets, n_sets,
                       g, cframe, n_frames, d_coef, d_status);
    CK_HIP(ctx, hipGetLastError());
    return CK_OK;
}

// One frame again, for the span decoder (k_jpeg_span.hip) whose verdict on one of its strands was "suspect": rows
// first_row .. first_row + n_rows - 1 are the frame's, its coefficients alone are zeroed, and the status words land at the
// rows' own places in d_status.
int k_jpeg_huff_frame(ck_ctx* ctx, const uint8_t* d_bytes, long long n_bytes, const CkStrand* d_rows, int first_row, int n_rows,
                      const CkHuffSet* d_sets, int n_sets, const CkStrandGeom& g, long long cframe, int n_frames, int frame, int16_t* d_coef,
                      uint32_t* d_status)
{
    if (first_row < 0 || n_rows <= 0 || n_sets <= 0 || frame < 0 || frame >= n_frames) return ck_fail(ctx, CK_ERR_ARG, "k_jpeg_huff_frame: nothing to decode");
    CK_HIP(ctx, hipMemsetAsync(d_coef + (size_t)frame * (size_t)cframe, 0, (size_t)cframe * sizeof(int16_t), ctx->stream));
    TimeScope ts(ctx, "jpeg_huff");
    const dim3 grid((unsigned)((n_rows + HUFF_LANES - 1) / HUFF_LANES));
    hipLaunchKernelGGL(jpeg_huff_kernel, grid, dim3(HUFF_LANES), 0, ctx->stream, d_bytes, n_bytes, d_rows + first_row, n_rows, d_sets, n_sets,
                       g, cframe, n_frames, d_coef, d_status + first_row);
    CK_HIP(ctx, hipGetLastError());
    return CK_OK;
}
