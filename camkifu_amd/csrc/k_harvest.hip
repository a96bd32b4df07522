// k_harvest.hip -- labelled classifier patches cut out of goban images that already lie in HBM, and their augmentation.
//
// k_harvest: n goban images (n x 380 x 380 x 3), the foreground counts of their 361 zones, per frame the index of a reference
// position (state_of[i], < 0: the frame is not harvested) -> the kept regions' 40 x 40 x 3 windows, labels and (frame, region),
// in ascending (frame, region) order, the same in every run.  Three launches on the context's stream:
//   1. harvest_flag   one thread per (frame i, region q = 10 ri + cj): the label is the base-3 number of the 2 x 2 block of
//                     positions[state_of[i]] at rows rs(ri).., columns rs(cj).. (rs = 0, 2, .., 16, 17: NNManager.compute_label);
//                     the region is calm when the counts of its four zones sum to <= calm_max; an empty region (label 0) is
//                     kept iff harvest_mix(seed, first_frame + i, q) & 255 < empty_keep.  The block ranks its flags (ballot and
//                     popcount per wave, the waves' totals through LDS) and leaves rank << 8 | label per thread, -1 without a
//                     flag, and its total.
//   2. harvest_scan   one wave: exclusive scan of the blocks' totals, 64 at a time with a running carry -> block offsets, total
//   3. harvest_gather one wave per candidate: output slot k = block offset + rank; k >= cap writes nothing.  A window row is
//                     120 bytes that start 4-byte aligned in the image (rows of 1140 bytes, origins at multiples of 60 bytes,
//                     images 433 200 bytes apart) and 8-byte aligned in x (patches of 4800 bytes): a lane moves two dwords
//                     in, one 8-byte store out.
// k_augment: x_out[k] = rot90(x[k], t & 3) mirrored left-right when t & 4 (numpy's result, channels untouched); one workgroup
// per patch, the patch read into LDS as 1200 consecutive dwords and written as 1200 consecutive dwords whose bytes are picked
// from LDS through the inverse transform: both global accesses are coalesced.
#include "ck_common.h"

namespace {

constexpr int SIDE = 380, REGIONS = 100, PATCH = 40, CELL = 20;
constexpr int ROW_DW = SIDE * 3 / 4;                  // 285 dwords per image row
constexpr int IMG_DW = SIDE * ROW_DW;                 // 108 300 dwords per image
constexpr int PATCH_DW = PATCH * PATCH * 3 / 4;       // 1200
constexpr int FLAG_BLOCK = CK_HARVEST_BLOCK;

__host__ __device__ inline int region_start(int i) { return i * 2 < 17 ? i * 2 : 17; }

__host__ __device__ inline uint32_t harvest_mix(uint32_t seed, uint32_t frame, uint32_t q)
{
    uint32_t h = mix32(seed ^ 0x9e3779b9u);
    h = mix32(h + frame * 0x9e3779b1u);
    return mix32(h + q * 0x7f4a7c15u);
}

__global__ void __launch_bounds__(FLAG_BLOCK) harvest_flag(const int32_t* __restrict__ fgcount, const int32_t* __restrict__ state_of,
                                                           const uint8_t* __restrict__ positions, int n, int calm_max, int empty_keep,
                                                           uint32_t seed, uint32_t first_frame, int32_t* __restrict__ code,
                                                           int32_t* __restrict__ block_total)
{
    __shared__ int wave_total[FLAG_BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int g = blockIdx.x * FLAG_BLOCK + t;
    bool keep = false;
    int label = 0;
    if (g < n * REGIONS) {
        const int i = g / REGIONS, q = g % REGIONS;
        const int s = state_of[i];
        if (s >= 0) {
            const int r0 = region_start(q / 10), c0 = region_start(q % 10);
            const uint8_t* pos = positions + (size_t)s * 361 + r0 * 19 + c0;
            const int32_t* fg = fgcount + (size_t)i * 361 + r0 * 19 + c0;
            label = pos[0] + 3 * pos[1] + 9 * pos[19] + 27 * pos[20];
            const long long moving = (long long)fg[0] + fg[1] + fg[19] + fg[20];
            keep = moving <= calm_max && (label != 0 || (int)(harvest_mix(seed, first_frame + (uint32_t)i, (uint32_t)q) & 255u) < empty_keep);
        }
    }
    const unsigned long long mask = __ballot(keep);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[wave] = __popcll(mask);
    __syncthreads();
    int base = 0, total = 0;
    for (int w = 0; w < FLAG_BLOCK / 64; w++) {
        const int v = wave_total[w];
        if (w < wave) base += v;
        total += v;
    }
    if (g < n * REGIONS) code[g] = keep ? ((base + before) << 8 | label) : -1;
    if (t == 0) block_total[blockIdx.x] = total;
}

// block_total[0 .. nb) -> its exclusive prefix sums in place, the grand total in block_total[nb]
__global__ void __launch_bounds__(64) harvest_scan(int32_t* __restrict__ block_total, int nb)
{
    const int lane = threadIdx.x;
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += 64) {
        const int b = b0 + lane;
        const int v = b < nb ? block_total[b] : 0;
        int incl = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (b < nb) block_total[b] = carry + incl - v;
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) block_total[nb] = carry;
}

__global__ void __launch_bounds__(256) harvest_gather(const uint32_t* __restrict__ goban, const int32_t* __restrict__ code,
                                                      const int32_t* __restrict__ block_offset, int n, int cap,
                                                      uint2* __restrict__ x, uint8_t* __restrict__ labels, int32_t* __restrict__ src)
{
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= n * REGIONS) return;
    const int cd = code[g];
    if (cd < 0) return;
    const int k = block_offset[g / FLAG_BLOCK] + (cd >> 8);
    if (k >= cap) return;
    const int i = g / REGIONS, q = g % REGIONS;
    const int oy = region_start(q / 10) * CELL, ox = region_start(q % 10) * CELL;
    const uint32_t* from = goban + (size_t)i * IMG_DW + (size_t)oy * ROW_DW + ox * 3 / 4;
    uint2* to = x + (size_t)k * (PATCH_DW / 2);
    for (int p = lane; p < PATCH_DW / 2; p += 64) {
        const int row = p / 15, pair = p % 15;
        const uint32_t* s = from + row * ROW_DW + pair * 2;
        to[p] = make_uint2(s[0], s[1]);
    }
    if (lane == 0) {
        labels[k] = (uint8_t)(cd & 255);
        src[2 * k] = i;
        src[2 * k + 1] = q;
    }
}

__global__ void __launch_bounds__(256) augment_kernel(const uint32_t* __restrict__ x, const uint8_t* __restrict__ tcode,
                                                      uint32_t* __restrict__ out)
{
    __shared__ uint32_t tile[PATCH_DW];
    const int k = blockIdx.x, t = tcode[k];
    const uint32_t* from = x + (size_t)k * PATCH_DW;
    for (int d = threadIdx.x; d < PATCH_DW; d += 256) tile[d] = from[d];
    __syncthreads();
    const uint8_t* px = (const uint8_t*)tile;
    const int rot = t & 3, flip = t & 4;
    uint32_t* to = out + (size_t)k * PATCH_DW;
    for (int d = threadIdx.x; d < PATCH_DW; d += 256) {
        uint32_t word = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int b = 4 * d + j;
            const int oi = b / (PATCH * 3), rem = b % (PATCH * 3), oj = rem / 3, c = rem % 3;
            const int jj = flip ? PATCH - 1 - oj : oj;
            int sy, sx;                                      // rot90(m, r)[oi][jj] = m[sy][sx]
            if (rot == 0)      { sy = oi;             sx = jj; }
            else if (rot == 1) { sy = jj;             sx = PATCH - 1 - oi; }
            else if (rot == 2) { sy = PATCH - 1 - oi; sx = PATCH - 1 - jj; }
            else               { sy = PATCH - 1 - jj; sx = oi; }
            word |= (uint32_t)px[(sy * PATCH + sx) * 3 + c] << (8 * j);
        }
        to[d] = word;
    }
}

}  // namespace

// d_code: n * 100 int32 and d_blocks: ck_harvest_blocks(n) + 1 int32 of scratch; the total lands in d_blocks[ck_harvest_blocks(n)]
int k_harvest(ck_ctx* ctx, const uint8_t* d_goban, const int32_t* d_fgcount, const int32_t* d_state, const uint8_t* d_positions, int n,
              int calm_max, int empty_keep, uint32_t seed, uint32_t first_frame, int32_t* d_code, int32_t* d_blocks,
              uint8_t* d_x, uint8_t* d_labels, int32_t* d_src, int cap)
{
    const int nb = ck_harvest_blocks(n);
    TimeScope ts(ctx, "harvest");
    hipLaunchKernelGGL(harvest_flag, dim3(nb), dim3(FLAG_BLOCK), 0, ctx->stream, d_fgcount, d_state, d_positions, n, calm_max, empty_keep,
                       seed, first_frame, d_code, d_blocks);
    CK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(harvest_scan, dim3(1), dim3(64), 0, ctx->stream, d_blocks, nb);
    CK_HIP(ctx, hipGetLastError());
    if (cap > 0) {
        hipLaunchKernelGGL(harvest_gather, dim3((n * REGIONS + 3) / 4), dim3(256), 0, ctx->stream, (const uint32_t*)d_goban, d_code, d_blocks,
                           n, cap, (uint2*)d_x, d_labels, d_src);
        CK_HIP(ctx, hipGetLastError());
    }
    return CK_OK;
}

int k_augment(ck_ctx* ctx, const uint8_t* d_x, const uint8_t* d_t, int n, uint8_t* d_out)
{
    TimeScope ts(ctx, "augment");
    hipLaunchKernelGGL(augment_kernel, dim3(n), dim3(256), 0, ctx->stream, (const uint32_t*)d_x, d_t, (uint32_t*)d_out);
    CK_HIP(ctx, hipGetLastError());
    return CK_OK;
}
