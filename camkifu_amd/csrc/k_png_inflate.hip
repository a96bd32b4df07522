// k_png_inflate.hip -- inflate on the device: one wave per zlib stream, a workgroup of one wave, the steps of
// ck_png_inflate_stage.h (read its head first: the window step, the ring, the order of writes).
//
// A wave keeps in LDS the ring of the last 32768 bytes, the three code tables, the code lengths of a dynamic block and the
// work arrays of the Adler-32 (InfShared, about 39 KiB: four streams a CU).  Lane 0 reads a block's header and builds its
// tables (serial and short, once per block); the other lanes wait at a barrier.  In a window step lane l decodes the tokens
// that would start at offsets l, 64 + l, .. of the window; the chain through them is a scalar walk with readlane from a
// uniform offset, which carries the running sum of the output lengths as well, so every real token knows its place without
// a scan of its own.  Literals then go to the ring all at once and matches one after the other, the bytes of a match spread
// over the lanes.  Whenever half a ring is full it leaves for the rows region in 16-byte stores; only positions below the
// stream's `cap` are written, the ring and the Adler-32 cover the rest.  Nothing the kernel wrote to HBM is read back.
// Every loop advances the bit position or ends the stream: a damaged stream ends in a verdict record like a good one.
// Two choices of this file: there is no wave scan -- the scalar walk through the chain needs every real token's length anyway
// and carries their running sum, which is the exclusive prefix sum --; and a step writes at most CK_INF_STEP_BYTES = 16 384
// bytes, not 64 x 258, so that a step's bytes and the bytes pending for the flush together never exceed the ring.
#include "ck_common.h"
#include "ck_png_inflate_stage.h"

namespace {

struct InfShared {
    uint8_t ring[CK_INF_RING];
    uint16_t lit[CK_INF_LIT_CAP], dist[CK_INF_DIST_CAP], cl[CK_INF_CL_CAP];
    uint8_t lens[320];
    CkInfAdlerWork aw;
    CkInfBlock blk;
};
static_assert(sizeof(InfShared) * 4 <= 160 * 1024, "four streams a CU");

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni(uint64_t v) { return (uint64_t)uni((uint32_t)(v >> 32)) << 32 | uni((uint32_t)v); }
__device__ __forceinline__ uint32_t lane_of(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }

// what a wave knows about its stream between steps: the same in every lane
struct InfState {
    uint8_t* out;
    uint64_t cap, need, pitch;
    uint64_t produced, flushed;
    uint32_t A, B;
    int64_t bad_row;
    uint32_t bad_type;
};

// positions [flushed, to), at most CK_INF_FLUSH of them, leave the ring (all lanes; the ring is complete up to `to`)
__device__ void inf_flush(InfShared& sh, InfState& s, uint64_t to, int lane)
{
    const int L = (int)(to - s.flushed);
    if (lane < ck_inf_chunk_tiles(L)) {
        const int left = L - lane * CK_PNG_TILE_BYTES;
        ck_inf_tile_pair(sh.ring, s.flushed + (uint64_t)lane * CK_PNG_TILE_BYTES, left < CK_PNG_TILE_BYTES ? left : CK_PNG_TILE_BYTES, &sh.aw.a[1 + lane], &sh.aw.b[1 + lane]);
    }
    __syncthreads();
    if (lane == 0) {
        sh.blk.arg0 = s.A; sh.blk.arg1 = s.B;
        ck_inf_adler_chunk(&sh.aw, L, &sh.blk.arg0, &sh.blk.arg1);
    }
    __syncthreads();
    s.A = uni(sh.blk.arg0); s.B = uni(sh.blk.arg1);
    for (uint64_t p = s.flushed + (uint64_t)lane * 16; p < to && p < s.cap; p += 64 * 16) {
        const uint64_t end = to < s.cap ? to : s.cap;
        uint8_t* d = s.out + p;
        const uint8_t* r = sh.ring + (p & (CK_INF_RING - 1));
        if (p + 16 <= end && ((uintptr_t)d & 15) == 0) {
            *(uint4*)d = *(const uint4*)r;
        } else {
            for (uint64_t i = 0; p + i < end && i < 16; i++) d[i] = r[i];
        }
    }
    if (s.pitch && s.bad_row < 0) {
        uint32_t type = 0;
        long long row = ck_inf_row_check(sh.ring, s.flushed, to, s.need, s.pitch, (uint64_t)lane, 64, &type);
        long long best = row < 0 ? 0x7fffffffffffffffLL : row;
        for (int k = 32; k; k >>= 1) {
            const long long other = __shfl_xor(best, k);
            best = other < best ? other : best;
        }
        const unsigned long long who = __ballot(row >= 0 && row == best);
        if (who) {
            s.bad_row = (int64_t)uni((uint64_t)best);
            s.bad_type = lane_of(type, (uint32_t)__builtin_ctzll(who));
        }
    }
    __syncthreads();
    s.flushed = to;
}

__device__ __forceinline__ void inf_drain(InfShared& sh, InfState& s, int lane)
{
    while (s.produced - s.flushed >= (uint64_t)CK_INF_FLUSH) inf_flush(sh, s, s.flushed + CK_INF_FLUSH, lane);
}

}  // namespace

// -DCK_PNG_INFLATE_SERIAL=1 builds the form to measure the window against (tools/png_timing.py --inflate-variant): only lane
// 0 decodes, one token a step.  It still pays a step's walk, ballots and barriers, so the ratio is the gain over one token a
// step in this kernel, not over a tight single-lane decoder.  The library is never shipped that way.
#ifndef CK_PNG_INFLATE_SERIAL
#define CK_PNG_INFLATE_SERIAL 0
#endif
constexpr int SERIAL = CK_PNG_INFLATE_SERIAL;

__global__ __launch_bounds__(64) void png_inflate_kernel(const uint8_t* __restrict__ zs, uint8_t* __restrict__ outs, const CkInfJob* __restrict__ jobs,
                                                         CkInfRecord* __restrict__ recs)
{
    __shared__ __attribute__((aligned(16))) InfShared sh;
    const int lane = (int)threadIdx.x;
    const CkInfJob job = jobs[blockIdx.x];
    CkInfIn in;
    in.z = zs + job.z_off; in.bytes = (uint64_t)job.zlen;
    InfState s;
    s.out = outs + job.out_off; s.cap = (uint64_t)job.cap; s.need = (uint64_t)job.need; s.pitch = (uint64_t)job.pitch;
    s.produced = s.flushed = 0; s.A = 1; s.B = 0; s.bad_row = -1; s.bad_type = 0;
    CkInfRecord rec;
    rec.cause = CK_INF_OK; rec.arg0 = rec.arg1 = rec.reserved = 0; rec.produced = rec.steps = rec.tokens = 0;
    const uint64_t bits = ck_inf_bits(in);
    uint64_t pos = 16;
    bool refused = false;
    rec.cause = ck_inf_wrapper(in, &rec.arg0);
    if (rec.cause) refused = true; else rec.arg0 = 0;
    for (int last = 0; !refused && !last;) {
        __syncthreads();                                     // nobody reads the tables of the block before any more
        if (lane == 0) ck_inf_block(in, pos, sh.lit, sh.dist, sh.cl, sh.lens, &sh.blk);
        __syncthreads();
        const int32_t cause = (int32_t)uni((uint32_t)sh.blk.cause);
        if (cause) { rec.cause = cause; rec.arg0 = uni(sh.blk.arg0); rec.arg1 = uni(sh.blk.arg1); refused = true; break; }
        last = (int)uni((uint32_t)sh.blk.last);
        pos = uni(sh.blk.pos);
        if (uni((uint32_t)sh.blk.type) == 0) {               // a stored block: the whole wave copies, a piece of the ring at a time
            const uint32_t stored = uni(sh.blk.stored);
            for (uint32_t done = 0; done < stored;) {
                const uint32_t m = stored - done < (uint32_t)CK_INF_STEP_BYTES ? stored - done : (uint32_t)CK_INF_STEP_BYTES;
                for (uint32_t i = (uint32_t)lane; i < m; i += 64) sh.ring[(s.produced + i) & (CK_INF_RING - 1)] = in.z[(pos >> 3) + done + i];
                __syncthreads();
                s.produced += m; done += m;
                inf_drain(sh, s, lane);
            }
            pos += (uint64_t)stored * 8;
            continue;
        }
        for (;;) {                                           // window steps
            uint64_t tok[CK_INF_OPL];
            uint32_t q[CK_INF_OPL];
#pragma unroll
            for (int j = 0; j < CK_INF_OPL; j++) {
                const uint32_t o = (uint32_t)(64 * j + lane);
                q[j] = 0;
                tok[j] = ck_inf_pack(CK_INF_REFUSED, 0, 0, CK_INF_TOK_LITLEN);
                if (!SERIAL || o == 0) tok[j] = ck_inf_token(ck_inf_peek(in, pos + o), (int64_t)(bits - pos) - (int64_t)o, sh.lit, sh.dist);
            }
            auto get = [&](uint32_t o) -> uint64_t {
                uint64_t t = 0;
#pragma unroll
                for (int j = 0; j < CK_INF_OPL; j++)
                    if ((int)(o >> 6) == j) t = (uint64_t)lane_of((uint32_t)(tok[j] >> 32), o & 63) << 32 | lane_of((uint32_t)tok[j], o & 63);
                return t;
            };
            auto place = [&](uint32_t o, uint32_t at) {
#pragma unroll
                for (int j = 0; j < CK_INF_OPL; j++)
                    if ((int)(o >> 6) == j && lane == (int)(o & 63)) q[j] = at;
            };
            CkInfWalk w;
            ck_inf_walk(get, place, s.produced, SERIAL ? 1u : (uint32_t)CK_INF_WINDOW, &w);
            const uint64_t n = s.produced;
            if (!w.far) {
#pragma unroll
                for (int j = 0; j < CK_INF_OPL; j++)
                    if ((w.taken[j] >> lane & 1) && ck_inf_kind(tok[j]) == CK_INF_LITERAL) sh.ring[(n + q[j]) & (CK_INF_RING - 1)] = (uint8_t)ck_inf_val(tok[j]);
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < CK_INF_OPL; j++) {
                unsigned long long todo = w.taken[j];
                if (!w.far) todo &= __ballot(ck_inf_kind(tok[j]) == CK_INF_MATCH);
                while (todo) {
                    const uint32_t l = (uint32_t)__builtin_ctzll(todo);
                    todo &= todo - 1;
                    const uint64_t t = get((uint32_t)(64 * j) + l);
                    const uint64_t at = n + lane_of(q[j], l);
                    const uint32_t v = ck_inf_val(t), len = ck_inf_len(t);
                    if (ck_inf_kind(t) == CK_INF_LITERAL) {
                        if (lane == 0) sh.ring[at & (CK_INF_RING - 1)] = (uint8_t)v;
                    } else {
                        for (uint32_t i = (uint32_t)lane; i < len; i += 64) {
                            const uint8_t x = sh.ring[(at - v + (v >= len ? i : i % v)) & (CK_INF_RING - 1)];
                            sh.ring[(at + i) & (CK_INF_RING - 1)] = x;
                        }
                    }
                    __syncthreads();                         // the next token may read these bytes
                }
            }
            s.produced += w.bytes; pos += w.advance;
            rec.steps++; rec.tokens += w.tokens;
            inf_drain(sh, s, lane);
            if (w.end == CK_INF_REFUSED) { rec.cause = (int32_t)w.cause; refused = true; break; }
            if (w.end == CK_INF_EOB) break;
        }
    }
    rec.produced = (int64_t)s.produced;
    if (!refused) {
        if (s.produced > s.flushed) inf_flush(sh, s, s.produced, lane);
        const uint64_t tail = (pos + 7) >> 3;
        if (in.bytes - tail < 4) {
            rec.cause = CK_INF_ADLER_ENDS;
        } else {
            const uint32_t want = (uint32_t)in.z[tail] << 24 | (uint32_t)in.z[tail + 1] << 16 | (uint32_t)in.z[tail + 2] << 8 | in.z[tail + 3];
            const uint32_t got = s.B << 16 | s.A;
            if (want != got) { rec.cause = CK_INF_ADLER; rec.arg0 = want; rec.arg1 = got; }
            else if (s.pitch && s.produced < s.need) rec.cause = CK_INF_ROWS_SHORT;
            else if (s.pitch && s.bad_row >= 0) { rec.cause = CK_INF_ROW_FILTER; rec.arg0 = (uint32_t)s.bad_row; rec.arg1 = s.bad_type; }
        }
    }
    if (lane == 0) recs[blockIdx.x] = rec;
}

int k_png_inflate(ck_ctx* ctx, const uint8_t* d_z, uint8_t* d_out, const CkInfJob* d_jobs, CkInfRecord* d_rec, int n)
{
    TimeScope ts(ctx, "png_inflate");
    hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)n), dim3(64), 0, ctx->stream, d_z, d_out, d_jobs, d_rec);
    CK_HIP(ctx, hipGetLastError());
    return CK_OK;
}
