// k_cluster.hip -- SfClustering.find_stones for a list of jobs (reference: src/camkifu/stone/sf_clustering.py:48-168).
// A job is (image, rows [rs, re), columns [cs, ce)): cv2.kmeans(pixels, 3, None, (EPS, 15, 3), 3, KMEANS_PP_CENTERS) over the
// BGR pixels of the region's view, the masked labels counted per intersection zone, interpret_ratios and check_density.
//
// One 1024-thread workgroup per job, the whole call -- three attempts of k-means++ seeding and up to 100 passes each --
// inside one launch: workgroup barriers only, no host round trip.  A thread owns a contiguous run of the view's pixels in
// raster order.  Two forms of the same kernel:
//   resident   (uint8 images, <= 20 480 pixels): the run is <= 20 pixels, each packed into one VGPR (B, G, R, label) with its
//              seeding distance beside it; nothing is read from memory after the first load but the few centre pixels;
//   streaming  (larger views, float32 images): pixels are re-read each pass (L2-resident), distances and labels live in
//              per-job scratch.
// Bit parity without a serial loop: for uint8 pixels every sum below is a sum of integers (squared distances <= 195 075,
// channel values) that stays far below 2^53, so the double accumulators are exact in any order; the one sum of non-integers,
// the compactness, is only compared between attempts and is reduced in a FIXED order (run, wave butterfly, 16 partials in
// turn), so equal inputs give equal bits and the first attempt wins a tie as in the library.  No floating-point atomics.
#include <float.h>
#include <math.h>

#include <type_traits>

#include "ck_common.h"

namespace {

constexpr int GS = 19, NT = 1024, NW = NT / 64, PERC = 20, NV = 13;
constexpr int MAX_PASSES = 100;            // (TERM_CRITERIA_EPS, 15, 3) has no COUNT bit: the library's own cap
constexpr double EPS2 = 9.0;               // epsilon 3, squared

struct Job {
    int32_t img, x0, y0, hs, ws, rs, re, cs, ce, pad;
    uint64_t rng;                          // generator state this job starts from
    uint64_t lab_off;                      // offset of its pixels in the label buffers
    uint64_t scr_off;                      // the same in the streaming form's scratch
};

struct Out {                               // device arrays, one row per job
    uint8_t* stones;                       // 361
    uint8_t* trusted;                      // 1
    uint8_t* ratios;                       // 361 * 3
    float* centers;                        // 9
    int32_t* passes;                       // 3
    double* compact;                       // 3
    int32_t* winner;                       // 1
};

// cv::RNG::next
__device__ __host__ inline uint32_t rng_next(uint64_t& s)
{
    s = (uint64_t)(uint32_t)s * 4164903690u + (uint32_t)(s >> 32);
    return (uint32_t)s;
}

// normL2Sqr_ of two 3-vectors: ((0 + v0^2) + v1^2) + v2^2 in f32, no contraction
__device__ inline float sqd(float a0, float a1, float a2, float b0, float b1, float b2)
{
    const float v0 = a0 - b0, v1 = a1 - b1, v2 = a2 - b2;
    float s = 0.f;
    s = s + v0 * v0;
    s = s + v1 * v1;
    s = s + v2 * v2;
    return s;
}

// a value every lane holds alike, moved to scalar registers (the centres, counts and sums are the same in all 1024 threads:
// kept per lane they would crowd the resident pixels out of the register file)
__device__ inline float uni(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ inline int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ inline double uni(double v)
{
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)b >> 32));
    return __longlong_as_double((long long)((unsigned long long)hi << 32 | lo));
}

__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// fixed-order sum over the workgroup of NVAL values per thread; every thread leaves with the totals
template <int NVAL>
__device__ inline void block_sum(double* v, double (*part)[NV], double* tot)
{
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
#pragma unroll
    for (int x = 0; x < NVAL; x++) v[x] = wave_sum(v[x]);
    __syncthreads();                                   // the readers of the previous totals are through
    if (lane == 0)
#pragma unroll
        for (int x = 0; x < NVAL; x++) part[w][x] = v[x];
    __syncthreads();
    if (t < NVAL) {
        double s = 0;
        for (int k = 0; k < NW; k++) s += part[k][t];
        tot[t] = s;
    }
    __syncthreads();
#pragma unroll
    for (int x = 0; x < NVAL; x++) v[x] = uni(tot[x]);
}

// the sums of one pass: the compactness (double, fixed order) and 12 counts / channel sums, which for byte pixels are
// integers (a thread's share, a wave's and the workgroup's all fit an int) and cost half the cross-lane traffic as such
template <typename A>
__device__ inline void pass_sum(double comp, const A* a, double* res, double (*part)[NV], double* tot)
{
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    comp = wave_sum(comp);
    A r[NV - 1];
#pragma unroll
    for (int x = 0; x < NV - 1; x++) {
        r[x] = a[x];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) r[x] += __shfl_xor(r[x], d);
    }
    __syncthreads();
    if (lane == 0) {
        part[w][0] = comp;
#pragma unroll
        for (int x = 0; x < NV - 1; x++) part[w][1 + x] = (double)r[x];
    }
    __syncthreads();
    if (t < NV) {
        double s = 0;
        for (int k = 0; k < NW; k++) s += part[k][t];
        tot[t] = s;
    }
    __syncthreads();
#pragma unroll
    for (int x = 0; x < NV; x++) res[x] = uni(tot[x]);
}

template <bool RES, typename T>
__global__ __launch_bounds__(NT) void cluster_kernel(const T* __restrict__ imgs, int side, const int32_t* __restrict__ rects,
                                                     const uint8_t* __restrict__ mask, const Job* __restrict__ jobs,
                                                     const int32_t* __restrict__ list, uint8_t* __restrict__ lab_best,
                                                     uint8_t* __restrict__ lab_scr, float* __restrict__ dist_scr, Out out)
{
    __shared__ double part[NW][NV];
    __shared__ double tot[NV];
    __shared__ double scanw[NW];
    __shared__ unsigned long long keyw[NW];
    __shared__ int s_ci;
    __shared__ int s_tc[3];
    __shared__ uint8_t s_st[GS * GS];

    using Acc = typename std::conditional<std::is_same<T, uint8_t>::value, int, double>::type;
    const int j = list[blockIdx.x];
    const Job jb = jobs[j];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int ws = jb.ws, N = jb.hs * jb.ws;
    const int per = RES ? PERC : (N + NT - 1) / NT;
    constexpr int UNR = RES ? PERC : 1;    // the resident run is unrolled in full (its arrays must stay in registers)
    const int base = t * per;
    const T* im = imgs + (size_t)jb.img * side * side * 3;
    uint8_t* lbest = lab_best + jb.lab_off;
    uint8_t* lcur = RES ? nullptr : lab_scr + jb.scr_off;
    float* dscr = RES ? nullptr : dist_scr + jb.scr_off;

    auto fetch = [&](int i, float& a, float& b, float& c) {
        const int y = i / ws, x = i - y * ws;
        const T* p = im + ((size_t)(jb.x0 + y) * side + jb.y0 + x) * 3;
        a = (float)p[0]; b = (float)p[1]; c = (float)p[2];
    };
    auto fetch_uni = [&](int i, float& a, float& b, float& c) {        // i is the same in every lane
        fetch(i, a, b, c);
        a = uni(a); b = uni(b); c = uni(c);
    };

    uint32_t pix[PERC];                    // resident form: B | G << 8 | R << 16 | label << 24
    float dist[PERC];
    if constexpr (RES) {
#pragma unroll
        for (int k = 0; k < PERC; k++) {
            const int i = base + k;
            pix[k] = 0; dist[k] = 0.f;
            if (i < N) {
                const int y = i / ws, x = i - y * ws;
                const uint8_t* p = (const uint8_t*)im + ((size_t)(jb.x0 + y) * side + jb.y0 + x) * 3;
                pix[k] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
            }
        }
    }
    auto getpx = [&](int k, int i, float& a, float& b, float& c) {
        if constexpr (RES) {
            uint32_t w = pix[k];
            asm volatile("" : "+v"(w));        // unpack again at every use: hoisted out of the passes, 60 floats would not fit
            a = (float)(w & 255u); b = (float)(w >> 8 & 255u); c = (float)(w >> 16 & 255u);
        } else fetch(i, a, b, c);
    };
    auto getd = [&](int k, int i) -> float {
        if constexpr (RES) {
            float d = dist[k];
            asm volatile("" : "+v"(d));        // (the same for its conversions to double)
            return d;
        } else return dscr[i];
    };
    auto setd = [&](int k, int i, float d) { if constexpr (RES) dist[k] = d; else dscr[i] = d; };
    auto getl = [&](int k, int i) -> int { if constexpr (RES) return (int)(pix[k] >> 24); else return lcur[i]; };
    auto setl = [&](int k, int i, int l) {
        if constexpr (RES) pix[k] = (pix[k] & 0xffffffu) | (uint32_t)l << 24; else lcur[i] = (uint8_t)l;
    };

    uint64_t rng = jb.rng;                 // every thread draws the same numbers: no broadcast needed
    double best_comp = DBL_MAX;
    int winner = -1;
    float bestc[3][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };

    for (int a = 0; a < 3; a++) {
        float cen[3][3], oldc[3][3];
        // ---- k-means++ seeding (generateCentersPP): 1 + 2 * 3 draws ------------------------------------------------
        {
            const int c0 = (int)(rng_next(rng) % (uint32_t)N);
            fetch_uni(c0, cen[0][0], cen[0][1], cen[0][2]);
            double s[1] = { 0 };
#pragma unroll UNR
            for (int k = 0; k < per; k++) {
                const int i = base + k;
                if (i < N) {
                    float p0, p1, p2;
                    getpx(k, i, p0, p1, p2);
                    const float d = sqd(p0, p1, p2, cen[0][0], cen[0][1], cen[0][2]);
                    setd(k, i, d);
                    s[0] += (double)d;
                }
            }
            block_sum<1>(s, part, tot);
            double sum0 = s[0];
            for (int kc = 1; kc < 3; kc++) {
                // exclusive prefix of the threads' distance totals (raster order): where a walk p -= dist[i] crosses zero
                double T0 = 0;
#pragma unroll UNR
                for (int k = 0; k < per; k++) {
                    const int i = base + k;
                    if (i < N) T0 += (double)getd(k, i);
                }
                double incl = T0;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const double o = __shfl_up(incl, d);
                    if (lane >= d) incl += o;
                }
                double excl = __shfl_up(incl, 1);
                if (lane == 0) excl = 0;
                __syncthreads();
                if (lane == 63) scanw[wv] = incl;
                __syncthreads();
                double woff = 0;
                for (int k = 0; k < wv; k++) woff += scanw[k];
                woff = uni(woff);
                const double E = woff + excl;

                double best_sum = DBL_MAX;
                int best_ci = 0;
                for (int trial = 0; trial < 3; trial++) {
                    const double p = (double)rng_next(rng) * 2.3283064365386963e-10 * sum0;       // (double)rng * sum0
                    if (t == 0) s_ci = N - 1;
                    __syncthreads();
                    double q = p - E;
                    if ((t == 0 || q > 0) && q - T0 <= 0) {
                        int found = -1;
#pragma unroll UNR
                        for (int k = 0; k < per; k++) {
                            const int i = base + k;
                            if (i < N && found < 0) {
                                q -= (double)getd(k, i);
                                if (q <= 0) found = i;
                            }
                        }
                        if (found >= 0) atomicMin(&s_ci, found);
                    }
                    __syncthreads();
                    const int ci = uni(s_ci);
                    float c0f, c1f, c2f;
                    fetch_uni(ci, c0f, c1f, c2f);
                    double sv[1] = { 0 };
#pragma unroll UNR
                    for (int k = 0; k < per; k++) {
                        const int i = base + k;
                        if (i < N) {
                            float p0, p1, p2;
                            getpx(k, i, p0, p1, p2);
                            sv[0] += (double)fminf(sqd(p0, p1, p2, c0f, c1f, c2f), getd(k, i));
                        }
                    }
                    block_sum<1>(sv, part, tot);       // (its barriers also fence s_ci for the next trial)
                    if (sv[0] < best_sum) { best_sum = sv[0]; best_ci = ci; }
                }
                fetch_uni(best_ci, cen[kc][0], cen[kc][1], cen[kc][2]);
#pragma unroll UNR
                for (int k = 0; k < per; k++) {
                    const int i = base + k;
                    if (i < N) {
                        float p0, p1, p2;
                        getpx(k, i, p0, p1, p2);
                        setd(k, i, fminf(sqd(p0, p1, p2, cen[kc][0], cen[kc][1], cen[kc][2]), getd(k, i)));
                    }
                }
                sum0 = best_sum;
            }
        }

        // ---- the passes --------------------------------------------------------------------------------------------
        int cnt[3] = { 0, 0, 0 };
        double csum[3][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };
        double comp = 0, shift = DBL_MAX;
        int iter = 0;
        for (;;) {
            if (iter > 0) {
                // an empty cluster takes the farthest point of the most populous one
                for (int k = 0; k < 3; k++) {
                    if (cnt[k] != 0) continue;
                    int mk = 0;
                    for (int k1 = 1; k1 < 3; k1++)
                        if (cnt[mk] < cnt[k1]) mk = k1;
                    const float sc = 1.f / (float)cnt[mk];
                    const float o0 = (float)csum[mk][0] * sc, o1 = (float)csum[mk][1] * sc, o2 = (float)csum[mk][2] * sc;
                    unsigned long long key = 0;
#pragma unroll UNR
                    for (int q = 0; q < per; q++) {
                        const int i = base + q;
                        if (i < N && getl(q, i) == mk) {
                            float p0, p1, p2;
                            getpx(q, i, p0, p1, p2);
                            const float d = sqd(p0, p1, p2, o0, o1, o2);
                            const unsigned long long kk = (unsigned long long)__float_as_uint(d) << 32 | (uint32_t)i;
                            if (key <= kk) key = kk;                   // max_dist <= dist: the last of equals
                        }
                    }
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) {
                        const unsigned long long o = __shfl_xor(key, d);
                        if (o > key) key = o;
                    }
                    __syncthreads();
                    if (lane == 0) keyw[wv] = key;
                    __syncthreads();
                    key = keyw[0];
                    for (int q = 1; q < NW; q++)
                        if (keyw[q] > key) key = keyw[q];
                    const int fi = uni((int)(uint32_t)key);
                    if (fi >= base && fi < base + per) {
                        if constexpr (RES) {
#pragma unroll
                            for (int q = 0; q < PERC; q++)
                                if (base + q == fi) setl(q, fi, k);
                        } else setl(0, fi, k);
                    }
                    float p0, p1, p2;
                    fetch_uni(fi, p0, p1, p2);
                    cnt[mk]--; cnt[k]++;
                    csum[mk][0] -= (double)p0; csum[mk][1] -= (double)p1; csum[mk][2] -= (double)p2;
                    csum[k][0] += (double)p0; csum[k][1] += (double)p1; csum[k][2] += (double)p2;
                }
                shift = 0;
                for (int k = 0; k < 3; k++) {
                    const float sc = 1.f / (float)cnt[k];
                    double d = 0;
                    for (int c = 0; c < 3; c++) {
                        oldc[k][c] = cen[k][c];
                        cen[k][c] = uni((float)csum[k][c] * sc);
                        const float df = cen[k][c] - oldc[k][c];
                        const float sq = df * df;
                        d += (double)sq;
                    }
                    shift = d > shift ? d : shift;
                }
            }
            iter++;
            if (iter == MAX_PASSES || shift <= EPS2) break;
            // labels = nearest centre (first minimum wins); counts, channel sums and compactness in the same sweep
            double cv = 0;
            Acc av[NV - 1];
#pragma unroll
            for (int x = 0; x < NV - 1; x++) av[x] = 0;
#pragma unroll UNR
            for (int k = 0; k < per; k++) {
                const int i = base + k;
                if (i < N) {
                    float p0, p1, p2;
                    getpx(k, i, p0, p1, p2);
                    const float d0 = sqd(p0, p1, p2, cen[0][0], cen[0][1], cen[0][2]);
                    const float d1 = sqd(p0, p1, p2, cen[1][0], cen[1][1], cen[1][2]);
                    const float d2 = sqd(p0, p1, p2, cen[2][0], cen[2][1], cen[2][2]);
                    int l = 0;
                    float dm = d0;
                    if (dm > d1) { dm = d1; l = 1; }
                    if (dm > d2) { dm = d2; l = 2; }
                    setl(k, i, l);
                    cv += (double)dm;
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const bool hit = l == c;
                        av[c] += hit ? (Acc)1 : (Acc)0;
                        av[3 + 3 * c] += hit ? (Acc)p0 : (Acc)0;
                        av[4 + 3 * c] += hit ? (Acc)p1 : (Acc)0;
                        av[5 + 3 * c] += hit ? (Acc)p2 : (Acc)0;
                    }
                }
            }
            double v[NV];
            pass_sum<Acc>(cv, av, v, part, tot);
            comp = v[0];
            for (int c = 0; c < 3; c++) {
                cnt[c] = (int)v[1 + c];
                csum[c][0] = v[4 + 3 * c]; csum[c][1] = v[5 + 3 * c]; csum[c][2] = v[6 + 3 * c];
            }
        }
        if (t == 0) {
            out.passes[(size_t)j * 3 + a] = iter;
            out.compact[(size_t)j * 3 + a] = comp;
        }
        if (comp < best_comp) {
            best_comp = comp;
            winner = a;
            for (int k = 0; k < 3; k++)
                for (int c = 0; c < 3; c++) bestc[k][c] = cen[k][c];
#pragma unroll UNR
            for (int k = 0; k < per; k++) {
                const int i = base + k;
                if (i < N) lbest[i] = (uint8_t)getl(k, i);
            }
        }
    }

    // ---- cluster_colors' ratios, interpret_ratios, check_density ------------------------------------------------------
    int grey[3];
    for (int k = 0; k < 3; k++) grey[k] = (int)(((bestc[k][0] + bestc[k][1]) + bestc[k][2]) / 3.f);
    const int gmin = min(grey[0], min(grey[1], grey[2])), gmax = max(grey[0], max(grey[1], grey[2]));
    const int gmed = grey[0] + grey[1] + grey[2] - gmin - gmax;
    const int med = grey[0] == gmed ? 0 : grey[1] == gmed ? 1 : 2;
    int colour[3];
    for (int k = 0; k < 3; k++) colour[k] = grey[k] == gmin ? 1 : grey[k] == gmax ? 2 : 0;
    uint8_t* ratios = out.ratios + (size_t)j * GS * GS * 3;
    if (t < GS * GS) {
        s_st[t] = 0;
        for (int k = 0; k < 3; k++) ratios[t * 3 + k] = k == med ? 1 : 0;
    }
    if (t < 3) s_tc[t] = 0;
    __syncthreads();                                   // (also: every label of the winning attempt is in lbest)
    const int C = jb.ce - jb.cs, nz = (jb.re - jb.rs) * C;
    for (int z = wv; z < nz; z += NW) {
        const int r = jb.rs + z / C, c = jb.cs + z % C;
        const int32_t* q = rects + ((size_t)r * GS + c) * 4;
        const int a0 = q[0] - jb.x0, b0 = q[1] - jb.y0, zh = q[2] - q[0], zw = q[3] - q[1], area = zh * zw;
        int n0 = 0, n1 = 0, n2 = 0;
        for (int p = lane; p < area; p += 64) {
            const int y = a0 + p / zw, x = b0 + p % zw;
            if (mask[(size_t)(jb.x0 + y) * side + jb.y0 + x]) {
                const int l = lbest[(size_t)y * ws + x];
                n0 += l == 0; n1 += l == 1; n2 += l == 2;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            n0 += __shfl_xor(n0, d); n1 += __shfl_xor(n1, d); n2 += __shfl_xor(n2, d);
        }
        if (lane == 0) {
            const int n[3] = { n0, n1, n2 };
            int rt[3], bk = 0;
            for (int k = 0; k < 3; k++) {
                rt[k] = n[k] > 0 ? 100 * n[k] / area : (k == med ? 1 : 0);       // truncated, written only for labels that occur
                ratios[((size_t)r * GS + c) * 3 + k] = (uint8_t)rt[k];
                if (rt[k] > rt[bk]) bk = k;                                     // first maximum
            }
            s_st[r * GS + c] = (uint8_t)colour[bk];
        }
    }
    __syncthreads();
    if (t < GS * GS) atomicAdd(&s_tc[s_st[t]], 1);
    __syncthreads();
    // compactness 0: the reference's `if retval:` is false and it fails on None; here: nothing found, not trusted
    const bool usable = best_comp != 0.0;
    const bool trusted = usable && s_tc[0] >= 2 && s_tc[1] >= 2 && s_tc[2] >= 2;
    if (t < GS * GS) out.stones[(size_t)j * GS * GS + t] = usable ? s_st[t] : 0;
    if (t == 0) {
        out.trusted[j] = trusted ? 1 : 0;
        out.winner[j] = winner;
        for (int k = 0; k < 3; k++)
            for (int c = 0; c < 3; c++) out.centers[(size_t)j * 9 + k * 3 + c] = bestc[k][c];
    }
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

uint64_t ck_rng_advance(uint64_t state, long long draws)
{
    for (long long i = 0; i < draws; i++) rng_next(state);
    return state;
}

// imgs: n goban images on the device, uint8 (is_f32 = 0) or float32; rects / mask / jobs and every output on the HOST
int k_cluster_stones(ck_ctx* ctx, const void* d_imgs, int n, int side, int is_f32, const int32_t* rects, const uint8_t* mask,
                     const int32_t* jobs, int m, uint8_t* stones, uint8_t* trusted, uint8_t* ratios, float* centers,
                     uint8_t* labels, long long labels_cap, int32_t* passes, double* compact, int32_t* winner)
{
    std::vector<Job> jv((size_t)m);
    std::vector<int32_t> res_list, str_list;
    size_t lab_total = 0, scr_total = 0;
    uint64_t state = ctx->rng_state;
    for (int j = 0; j < m; j++) {
        const int32_t* q = jobs + (size_t)j * 5;
        const int img = q[0], rs = q[1], re = q[2], cs = q[3], ce = q[4];
        if (img < 0 || img >= n) return ck_fail(ctx, CK_ERR_ARG, "job %d: image %d of %d", j, img, n);
        if (rs < 0 || cs < 0 || re > GS || ce > GS || re <= rs || ce <= cs)
            return ck_fail(ctx, CK_ERR_ARG, "job %d: intersection range rows [%d, %d) columns [%d, %d)", j, rs, re, cs, ce);
        const int32_t* a = rects + ((size_t)rs * GS + cs) * 4;
        const int32_t* b = rects + ((size_t)(re - 1) * GS + ce - 1) * 4;
        const int x0 = a[0], y0 = a[1], x1 = b[2], y1 = b[3];
        if (x0 < 0 || y0 < 0 || x1 > side || y1 > side || x1 <= x0 || y1 <= y0)
            return ck_fail(ctx, CK_ERR_ARG, "job %d: zone rectangles give the view [%d, %d) x [%d, %d) of a %d image", j, x0, x1, y0, y1, side);
        const long long npx = (long long)(x1 - x0) * (y1 - y0);
        if (npx < 3) return ck_fail(ctx, CK_ERR_ARG, "job %d: %lld pixels, 3-means needs 3", j, npx);
        for (int r = rs; r < re; r++)
            for (int c = cs; c < ce; c++) {
                const int32_t* z = rects + ((size_t)r * GS + c) * 4;
                if (z[0] < x0 || z[1] < y0 || z[2] > x1 || z[3] > y1 || z[2] <= z[0] || z[3] <= z[1])
                    return ck_fail(ctx, CK_ERR_ARG, "job %d: zone (%d, %d) does not lie inside the analysed view", j, r, c);
            }
        Job& jb = jv[j];
        jb = Job{ img, x0, y0, x1 - x0, y1 - y0, rs, re, cs, ce, 0, state, lab_total, 0 };
        state = ck_rng_advance(state, 21);
        lab_total += (size_t)npx;
        if (!is_f32 && npx <= (long long)NT * PERC) res_list.push_back(j);
        else { jb.scr_off = scr_total; scr_total += (size_t)npx; str_list.push_back(j); }
    }
    if (labels && labels_cap < (long long)lab_total)
        return ck_fail(ctx, CK_ERR_CAPACITY, "labels: %lld bytes for %zu pixels", labels_cap, lab_total);

    // device layout: [jobs | lists | rects | mask | outputs] in `pts`, labels in `labels`, streaming scratch in `labels2` / `ghost`
    const size_t o_jobs = 0, o_list = up256(o_jobs + jv.size() * sizeof(Job)), o_rects = up256(o_list + (size_t)m * 4);
    const size_t o_mask = up256(o_rects + GS * GS * 16), o_st = up256(o_mask + (size_t)side * side);
    const size_t o_tr = up256(o_st + (size_t)m * 361), o_ra = up256(o_tr + m), o_ce = up256(o_ra + (size_t)m * 1083);
    const size_t o_pa = up256(o_ce + (size_t)m * 36), o_co = up256(o_pa + (size_t)m * 12), o_wi = up256(o_co + (size_t)m * 24);
    const size_t total = up256(o_wi + (size_t)m * 4);
    CK_TRY(ck_ensure(ctx, ctx->pts, total));
    CK_TRY(ck_ensure(ctx, ctx->labels, lab_total + 64));
    if (scr_total) {
        CK_TRY(ck_ensure(ctx, ctx->labels2, scr_total * 4 + 64));
        CK_TRY(ck_ensure(ctx, ctx->ghost, scr_total + 64));
    }
    uint8_t* d = (uint8_t*)ctx->pts.p;
    std::vector<int32_t> list(res_list);
    list.insert(list.end(), str_list.begin(), str_list.end());
    CK_HIP(ctx, hipMemcpyAsync(d + o_jobs, jv.data(), jv.size() * sizeof(Job), hipMemcpyHostToDevice, ctx->stream));
    CK_HIP(ctx, hipMemcpyAsync(d + o_list, list.data(), list.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    CK_HIP(ctx, hipMemcpyAsync(d + o_rects, rects, GS * GS * 16, hipMemcpyHostToDevice, ctx->stream));
    CK_HIP(ctx, hipMemcpyAsync(d + o_mask, mask, (size_t)side * side, hipMemcpyHostToDevice, ctx->stream));
    Out out{ d + o_st, d + o_tr, d + o_ra, (float*)(d + o_ce), (int32_t*)(d + o_pa), (double*)(d + o_co), (int32_t*)(d + o_wi) };
    const Job* d_jobs = (const Job*)(d + o_jobs);
    const int32_t* d_list = (const int32_t*)(d + o_list);
    const int32_t* d_rects = (const int32_t*)(d + o_rects);
    {
        TimeScope ts(ctx, "cluster");
        const int nres = (int)res_list.size(), nstr = (int)str_list.size();
        if (nres)
            hipLaunchKernelGGL((cluster_kernel<true, uint8_t>), dim3(nres), dim3(NT), 0, ctx->stream, (const uint8_t*)d_imgs, side, d_rects,
                               (const uint8_t*)(d + o_mask), d_jobs, d_list, (uint8_t*)ctx->labels.p, (uint8_t*)nullptr, (float*)nullptr, out);
        if (nstr && !is_f32)
            hipLaunchKernelGGL((cluster_kernel<false, uint8_t>), dim3(nstr), dim3(NT), 0, ctx->stream, (const uint8_t*)d_imgs, side, d_rects,
                               (const uint8_t*)(d + o_mask), d_jobs, d_list + nres, (uint8_t*)ctx->labels.p, (uint8_t*)ctx->ghost.p,
                               (float*)ctx->labels2.p, out);
        if (nstr && is_f32)
            hipLaunchKernelGGL((cluster_kernel<false, float>), dim3(nstr), dim3(NT), 0, ctx->stream, (const float*)d_imgs, side, d_rects,
                               (const uint8_t*)(d + o_mask), d_jobs, d_list + nres, (uint8_t*)ctx->labels.p, (uint8_t*)ctx->ghost.p,
                               (float*)ctx->labels2.p, out);
        CK_HIP(ctx, hipGetLastError());
    }
    auto back = [&](void* dst, size_t off, size_t bytes) -> int {
        if (dst) CK_HIP(ctx, hipMemcpyAsync(dst, d + off, bytes, hipMemcpyDeviceToHost, ctx->stream));
        return CK_OK;
    };
    CK_TRY(back(stones, o_st, (size_t)m * 361));
    CK_TRY(back(trusted, o_tr, (size_t)m));
    CK_TRY(back(ratios, o_ra, (size_t)m * 1083));
    CK_TRY(back(centers, o_ce, (size_t)m * 36));
    CK_TRY(back(passes, o_pa, (size_t)m * 12));
    CK_TRY(back(compact, o_co, (size_t)m * 24));
    CK_TRY(back(winner, o_wi, (size_t)m * 4));
    if (labels) CK_HIP(ctx, hipMemcpyAsync(labels, ctx->labels.p, lab_total, hipMemcpyDeviceToHost, ctx->stream));
    CK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->rng_state = state;                // advanced by 21 * m, once the call has gone through
    return CK_OK;
}
