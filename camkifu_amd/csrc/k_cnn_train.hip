// k_cnn_train.hip -- one training step of the stone classifier (the network of NNManager.create_net, nn_manager.py:277-298):
// a forward pass that keeps what the backward pass needs, softmax + categorical cross-entropy, the backward pass, Adam.
//
// Every product is ONE implicit GEMM C[M x N] = A[M x K] . B[K x N]: the gradients on the f32-input MFMA (tr_gemm,
// v_mfma_f32_32x32x2_f32: a k-ordered f32 fma chain, exact f32), the forward pass on the f64 MFMA with one rounding to f32
// (tr_gemm_f64: see there why).  A and B are read through small loader structs that turn (m, k) / (k, n) into an
// address -- the im2col view of a channels-last map, a weight array as stored, a transposed matrix --
// so nothing is ever unfolded in memory; an epilogue struct says what happens to C.
//     forward conv      M = patches x OH x OW   N = Cout   K = KH KW Cin      A = im2col(in)         B = w as stored
//     data gradient     M = patches x IH x IW   N = Cin    K = KH KW Cout     A = im2col'(dz), full  B = w as stored, (ci, co) swapped
//     weight gradient   M = KH KW Cin (+1)      N = Cout   K = patches x OH x OW   A = im2col(in)^T   B = dz
// The true convolution of Keras-1 on Theano is out[y][x] = sum in[y + KH-1-i][x + KW-1-j] w[i][j]: the flip lives in the
// index, the kernels stay un-flipped in memory.  The extra row (+1) of a weight gradient is a row of ones: it yields the
// bias gradient (the sum of dz over patches and positions) from the same product.
//
// Order of summation (what makes a step repeat bit for bit): a gradient product sums 16 k at a time in one MFMA chain and
// adds those sums upwards, a forward product sums k upwards in double; a weight gradient splits K into S slices (S a function of the shapes alone), each slice writes its own partial matrix, and
// tr_reduce adds the partials in slice order, then onto the sum of the earlier chunks.  No atomics anywhere.
//
// Stored between forward and backward, per patch: the post-ReLU maps a1 (36x36x32), a2 (32x32x32), a3 (14x14x90),
// a4 (12x12x90), the pooled maps p1 (16x16x32) and p2 (6x6x90) AFTER dropout, h1 (160) after ReLU and dropout.
// ReLU's derivative is taken from the stored output (out > 0, so relu'(0) = 0); a pooled gradient goes to the first
// maximum of its window in raster order, and only if the stored pooled value is > 0 (a dropped or all-zero window
// routes nothing); a kept unit's gradient is divided by 1 - p like its activation was.
#include "ck_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int BM = 128, KT = 16, SA = BM + 32;       // block tile rows, k per LDS tile, LDS row stride of A (halves on different banks)

// ---- loaders: A(m, k) and B(k, n).  KFAST says which index walks memory contiguously (the tile loader follows it) ----
// element (position pos = (p, y, x), tap-channel tc = (i, j, ci)) of the im2col view of a channels-last map, flip applied
template <int IH, int IW, int CI, int KH, int KW, typename T>
struct Patch {
    static constexpr int OH = IH - KH + 1, OW = IW - KW + 1;
    const T* in;
    __device__ float at(int pos, int tc) const
    {
        const int x = pos % OW, q = pos / OW, y = q % OH, p = q / OH;
        const int ci = tc % CI, tap = tc / CI, j = tap % KW, i = tap / KW;
        return (float)in[((size_t)(p * IH + y + KH - 1 - i) * IW + (x + KW - 1 - j)) * CI + ci];
    }
};
template <int IH, int IW, int CI, int KH, int KW, typename T>
struct AIm2col : Patch<IH, IW, CI, KH, KW, T> {           // forward: m = position, k = tap-channel
    static constexpr bool KFAST = true;
    __device__ float operator()(int m, int k) const { return this->at(m, k); }
};
template <int IH, int IW, int CI, int KH, int KW, typename T>
struct AIm2colT : Patch<IH, IW, CI, KH, KW, T> {          // weight gradient: m = tap-channel (row KH KW CI: ones), k = position
    static constexpr bool KFAST = false;
    __device__ float operator()(int m, int k) const { return m == KH * KW * CI ? 1.0f : this->at(k, m); }
};
// data gradient: m = input position (p, u, v), k = (i, j, co); dz[p][u - (KH-1-i)][v - (KW-1-j)][co], zero outside
template <int IH, int IW, int CO, int KH, int KW>
struct AFull {
    static constexpr bool KFAST = true;
    static constexpr int OH = IH - KH + 1, OW = IW - KW + 1;
    const float* dz;
    __device__ float operator()(int m, int k) const
    {
        const int v = m % IW, q = m / IW, u = q % IH, p = q / IH;
        const int co = k % CO, tap = k / CO, j = tap % KW, i = tap / KW;
        const int y = u - (KH - 1 - i), x = v - (KW - 1 - j);
        if (y < 0 || y >= OH || x < 0 || x >= OW) return 0.0f;
        return dz[((size_t)(p * OH + y) * OW + x) * CO + co];
    }
};
template <int CI, int CO>
struct BSwap {                                             // k = (tap, co), n = ci: w[tap][ci][co] as stored
    static constexpr bool KFAST = true;
    const float* w;
    __device__ float operator()(int k, int n) const { return w[((size_t)(k / CO) * CI + n) * CO + (k % CO)]; }
};
struct ARow {                                              // A(m, k) = p[m * ld + k]
    static constexpr bool KFAST = true;
    const float* p; int ld;
    __device__ float operator()(int m, int k) const { return p[(size_t)m * ld + k]; }
};
struct ARowT {                                             // A(m, k) = p[k * ld + m]; row `ones` is all ones (bias gradient)
    static constexpr bool KFAST = false;
    const float* p; int ld, ones;
    __device__ float operator()(int m, int k) const { return m == ones ? 1.0f : p[(size_t)k * ld + m]; }
};
struct BRow {                                              // B(k, n) = p[k * ld + n]
    static constexpr bool KFAST = false;
    const float* p; int ld;
    __device__ float operator()(int k, int n) const { return p[(size_t)k * ld + n]; }
};
struct BRowT {                                             // B(k, n) = p[n * ld + k]
    static constexpr bool KFAST = true;
    const float* p; int ld;
    __device__ float operator()(int k, int n) const { return p[(size_t)n * ld + k]; }
};

// ---- epilogues ----
struct EpBias {                                            // out = acc + bias (in double, rounded once), ReLU on request
    float* out; const float* bias; int N, relu;
    __device__ void operator()(int, int m, int n, double acc) const
    {
        const float v = (float)(acc + (double)bias[n]);
        out[(size_t)m * N + n] = relu ? fmaxf(v, 0.0f) : v;
    }
};
struct EpGate {                                            // gradient w.r.t. a stored activation: through ReLU (and dropout) where gate > 0
    float* out; const float* gate; int N; float keep;
    __device__ void operator()(int, int m, int n, float v) const
    {
        const size_t i = (size_t)m * N + n;
        out[i] = gate ? (gate[i] > 0.0f ? v / keep : 0.0f) : v;
    }
};
struct EpPart {                                            // slice z of a weight gradient
    float* part; int M, N;
    __device__ void operator()(int z, int m, int n, float v) const { part[((size_t)z * M + m) * N + n] = v; }
};

// one LDS tile: As[kk][mm] = A(m0 + mm, k0 + kk), Bs[kk][nn] = B(k0 + kk, n0 + nn), zero outside M, N and the slice
template <int BN, int SB, class LA, class LB>
__device__ inline void tr_load_tile(const LA& la, const LB& lb, float* As, float* Bs, int t, int m0, int n0, int k0, int M, int N, int kend)
{
#pragma unroll
    for (int r = 0; r < BM * KT / 256; r++) {
        const int idx = t + 256 * r;
        const int kk = LA::KFAST ? idx % KT : idx / BM, mm = LA::KFAST ? idx / KT : idx % BM;
        const int m = m0 + mm, k = k0 + kk;
        As[kk * SA + mm] = (m < M && k < kend) ? la(m, k) : 0.0f;
    }
#pragma unroll
    for (int r = 0; r < BN * KT / 256; r++) {
        const int idx = t + 256 * r;
        const int kk = LB::KFAST ? idx % KT : idx / BN, nn = LB::KFAST ? idx / KT : idx % BN;
        const int n = n0 + nn, k = k0 + kk;
        Bs[kk * SB + nn] = (n < N && k < kend) ? lb(k, n) : 0.0f;
    }
}

// 256 threads = 4 waves; the block computes 128 x (32 NT), wave w rows 32 w .. 32 w + 31 of it as NT 32 x 32 MFMA tiles.
// blockIdx.z = slice of K: k in [z * kslice, min(K, (z + 1) * kslice)), kslice a multiple of KT.
template <int NT, class LA, class LB, class EP>
__global__ __launch_bounds__(256) void tr_gemm(LA la, LB lb, EP ep, int M, int N, int K, int kslice)
{
    constexpr int BN = 32 * NT, SB = (BN % 64 == 0) ? BN + 32 : BN;
    __shared__ float As[KT * SA];
    __shared__ float Bs[KT * SB];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, half = lane >> 5, l31 = lane & 31;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int kbeg = blockIdx.z * kslice, kend = min(K, kbeg + kslice);
    // two levels of f32 sums: each LDS tile's 16 k in one MFMA chain from zero, the tiles' sums added upwards in `tot`
    // (the rounding error of a sum over K grows with K / 4 instead of K)
    f32x16 tot[NT];
#pragma unroll
    for (int i = 0; i < NT; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) tot[i][r] = 0.0f;

    for (int k0 = kbeg; k0 < kend; k0 += KT) {
        f32x16 acc[NT];
#pragma unroll
        for (int i = 0; i < NT; i++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][r] = 0.0f;
        tr_load_tile<BN, SB>(la, lb, As, Bs, t, m0, n0, k0, M, N, kend);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < KT; kk += 2) {               // lane l: A[row l & 31][k = l >> 5], B[k = l >> 5][col l & 31]
            const float a = As[(kk + half) * SA + wave * 32 + l31];
#pragma unroll
            for (int i = 0; i < NT; i++)
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[(kk + half) * SB + i * 32 + l31], acc[i], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NT; i++) tot[i] += acc[i];
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < NT; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) {                     // C: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
            const int m = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half, n = n0 + i * 32 + l31;
            if (m < M && n < N) ep((int)blockIdx.z, m, n, tot[i][r]);
        }
}

// The same product for the FORWARD pass, on v_mfma_f64_16x16x4_f64: the f32 operands widened, the whole sum over K and
// the bias in double, one rounding to f32 in the epilogue.  Behind every forward product sits a decision -- the sign a
// ReLU sees, the winner of a pool window -- and on real patches some windows' best two values are 1.5 float32 ulp apart:
// an f32 chain over K = 800 moves them by more than that and the gradient then goes to another position than in exact
// arithmetic (lab notes 13).  Correctly rounded maps decide as exact arithmetic does whenever f32 can tell the values apart.
// The wave's 32 x (32 NT) part is 2 x (2 NT) tiles of 16 x 16; lane l holds A[row l & 15][k = l >> 4], B[k = l >> 4][col l & 15],
// and of C column l & 15, rows (l >> 4) + 4 r in register r.
template <int NT, class LA, class LB, class EP>
__global__ __launch_bounds__(256) void tr_gemm_f64(LA la, LB lb, EP ep, int M, int N, int K)
{
    constexpr int BN = 32 * NT, SB = (BN % 64 == 0) ? BN + 32 : BN;
    __shared__ float As[KT * SA];
    __shared__ float Bs[KT * SB];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, quarter = lane >> 4, l15 = lane & 15;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    f64x4 acc[2][2 * NT];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int c = 0; c < 2 * NT; c++)
#pragma unroll
            for (int e = 0; e < 4; e++) acc[r][c][e] = 0.0;

    for (int k0 = 0; k0 < K; k0 += KT) {
        tr_load_tile<BN, SB>(la, lb, As, Bs, t, m0, n0, k0, M, N, K);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < KT; kk += 4) {
            const double a0 = As[(kk + quarter) * SA + wave * 32 + l15], a1 = As[(kk + quarter) * SA + wave * 32 + 16 + l15];
#pragma unroll
            for (int c = 0; c < 2 * NT; c++) {
                const double b = Bs[(kk + quarter) * SB + c * 16 + l15];
                acc[0][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[0][c], 0, 0, 0);
                acc[1][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[1][c], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int c = 0; c < 2 * NT; c++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int m = m0 + wave * 32 + r * 16 + quarter + 4 * e, n = n0 + c * 16 + l15;
                if (m < M && n < N) ep(0, m, n, acc[r][c][e]);
            }
}

// g[i] = (earlier chunks) + (part[0][i] + part[1][i] + ... in that order, summed in double and rounded once)
__global__ void tr_reduce(const float* part, int S, size_t count, float* g, int accumulate)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    double s = part[i];
    for (int z = 1; z < S; z++) s += (double)part[(size_t)z * count + i];
    g[i] = (float)(accumulate ? (double)g[i] + s : s);
}

// 2 x 2 max pool of a channels-last map (H x W even) of `np` patches
__global__ void tr_pool(const float* a, float* out, int np, int H, int W, int C)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int PH = H / 2, PW = W / 2;
    if (i >= (size_t)np * PH * PW * C) return;
    const int c = i % C;
    size_t q = i / C;
    const int x = q % PW; q /= PW;
    const int y = q % PH;
    const size_t p = q / PH;
    const float* s = a + ((p * H + 2 * y) * W + 2 * x) * C + c;
    out[i] = fmaxf(fmaxf(s[0], s[C]), fmaxf(s[(size_t)W * C], s[(size_t)W * C + C]));
}

// gradient of the pool: to the first maximum of the window in raster order, if the stored pooled value (after dropout)
// is > 0; divided by keep = 1 - p of the dropout behind the pool (1 when dropout is off)
__global__ void tr_pool_back(const float* a, const float* pooled, const float* dpooled, float* dz, int np, int H, int W, int C, float keep)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)np * H * W * C) return;
    const int c = i % C;
    size_t q = i / C;
    const int x = q % W; q /= W;
    const int y = q % H;
    const size_t p = q / H;
    const float* s = a + ((p * H + (y & ~1)) * W + (x & ~1)) * C + c;
    const float v[4] = { s[0], s[C], s[(size_t)W * C], s[(size_t)W * C + C] };
    int best = 0;
    for (int k = 1; k < 4; k++) if (v[k] > v[best]) best = k;
    const size_t j = ((p * (H / 2) + y / 2) * (W / 2) + x / 2) * C + c;
    const int mine = (y & 1) * 2 + (x & 1);
    dz[i] = (mine == best && pooled[j] > 0.0f) ? dpooled[j] / keep : 0.0f;
}

// Dropout in place: unit e of the layer (e = global patch index * units per patch + unit) is kept when the top 24 bits of
// mix32(mix32(lo(e) ^ key) + hi(e) * 0x9e3779b1 + key) are >= p * 2^24; key = a mix of (seed, step, layer).  Kept units are
// divided by 1 - p.  mask (nullable): 1 kept / 0 dropped, at the unit's global index.
__global__ void tr_dropout(float* a, size_t count, size_t first, uint32_t key, uint32_t thr, float keep, uint8_t* mask)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const unsigned long long e = first + i;
    const uint32_t u = mix32(mix32((uint32_t)e ^ key) + (uint32_t)(e >> 32) * 0x9e3779b1u + key);
    const bool on = (u >> 8) >= thr;
    a[i] = on ? a[i] / keep : 0.0f;
    if (mask) mask[e] = on ? 1 : 0;
}

// softmax + categorical cross-entropy of one patch per thread: loss[p] = -log softmax(lg)[label], dlg = (softmax - onehot) / n_total
__global__ void tr_softmax_xent(const float* lg, const uint8_t* label, int np, int n_total, float* loss, float* dlg)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    const float* z = lg + (size_t)p * 81;
    float mx = z[0];
    for (int c = 1; c < 81; c++) mx = fmaxf(mx, z[c]);
    float sum = 0.0f;
    for (int c = 0; c < 81; c++) sum += expf(z[c] - mx);
    const int lab = label[p];
    loss[p] = logf(sum) - (z[lab] - mx);
    for (int c = 0; c < 81; c++)
        dlg[(size_t)p * 81 + c] = (expf(z[c] - mx) / sum - (c == lab ? 1.0f : 0.0f)) / (float)n_total;
}

// Adam as Keras-1 compiles it: m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2; w -= lr_t m / (sqrt(v) + eps),
// lr_t = lr sqrt(1 - b2^t) / (1 - b1^t).  Weights and moments are held in f32; the arithmetic of one update is done in
// double, so an update is the correctly rounded function of its f32 inputs (a weight that nearly cancels keeps its digits).
__global__ void tr_adam(float* w, float* m, float* v, const float* g, size_t count, double lr_t, double b1, double b2, double eps)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const double gi = g[i];
    const double mi = b1 * (double)m[i] + (1.0 - b1) * gi;
    const double vi = b2 * (double)v[i] + (1.0 - b2) * (gi * gi);
    w[i] = (float)((double)w[i] - lr_t * mi / (sqrt(vi) + eps));
    m[i] = (float)mi;
    v[i] = (float)vi;
}

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

template <int NT, class LA, class LB, class EP>
int gemm(ck_ctx* ctx, LA la, LB lb, EP ep, int M, int N, int K, int S = 1, int kslice = 0)
{
    if (S == 1) kslice = cdiv(K, KT) * KT;
    dim3 grid(cdiv(M, BM), cdiv(N, 32 * NT), S);
    hipLaunchKernelGGL((tr_gemm<NT, LA, LB, EP>), grid, dim3(256), 0, ctx->stream, la, lb, ep, M, N, K, kslice);
    CK_HIP(ctx, hipGetLastError());
    return CK_OK;
}

template <int NT, class LA, class LB, class EP>
int gemm_f64(ck_ctx* ctx, LA la, LB lb, EP ep, int M, int N, int K)
{
    dim3 grid(cdiv(M, BM), cdiv(N, 32 * NT), 1);
    hipLaunchKernelGGL((tr_gemm_f64<NT, LA, LB, EP>), grid, dim3(256), 0, ctx->stream, la, lb, ep, M, N, K);
    CK_HIP(ctx, hipGetLastError());
    return CK_OK;
}

// the slices of a weight gradient: a function of the shapes alone
void split_k(int M, int N, int NT, int K, int* S, int* kslice)
{
    const int tiles = cdiv(M, BM) * cdiv(N, 32 * NT);
    int s = std::max(1, std::min(2048 / tiles, K / (KT * 4)));
    *kslice = cdiv(cdiv(K, s), KT) * KT;
    *S = cdiv(K, *kslice);
}

template <int NT, class LA, class LB>
int wgrad(ck_ctx* ctx, CkTrainer& tr, LA la, LB lb, int M, int N, int K, float* g, bool accumulate)
{
    int S, ks;
    split_k(M, N, NT, K, &S, &ks);
    const size_t count = (size_t)M * N;
    CK_TRY(ck_ensure(ctx, tr.part, (size_t)S * count * sizeof(float)));
    CK_TRY((gemm<NT>(ctx, la, lb, EpPart{ (float*)tr.part.p, M, N }, M, N, K, S, ks)));
    hipLaunchKernelGGL(tr_reduce, dim3(cdiv(count, 256)), dim3(256), 0, ctx->stream, (const float*)tr.part.p, S, count, g, accumulate ? 1 : 0);
    CK_HIP(ctx, hipGetLastError());
    return CK_OK;
}

uint32_t dropout_key(uint64_t seed, uint64_t step, uint32_t layer)
{
    uint32_t k = mix32((uint32_t)seed ^ 0x9e3779b9u);
    k = mix32(k ^ (uint32_t)(seed >> 32));
    k = mix32(k + (uint32_t)step * 0x9e3779b1u);
    k = mix32(k ^ (uint32_t)(step >> 32));
    return mix32(k + (layer + 1) * 0x7f4a7c15u);
}

int dropout(ck_ctx* ctx, float* a, size_t per_patch, int np, size_t first_patch, uint64_t seed, uint64_t step, int layer, float p, uint8_t* mask)
{
    const size_t count = per_patch * np;
    hipLaunchKernelGGL(tr_dropout, dim3(cdiv(count, 256)), dim3(256), 0, ctx->stream, a, count, first_patch * per_patch,
                       dropout_key(seed, step, layer), (uint32_t)(p * 16777216.0f), 1.0f - p, mask);
    CK_HIP(ctx, hipGetLastError());
    return CK_OK;
}

}  // namespace

int k_train_create(ck_ctx* ctx, CkTrainer& tr, const float* const w[12], int space)
{
    if (space != CK_HOST && space != CK_DEVICE) return ck_fail(ctx, CK_ERR_ARG, "bad memory space %d", space);
    const size_t bytes = CK_TRAIN_PARAMS * sizeof(float);
    DevBuf* bufs[] = { &tr.w, &tr.g, &tr.m, &tr.v };
    for (DevBuf* b : bufs) CK_TRY(ck_ensure(ctx, *b, bytes));
    for (int i = 0; i < 12; i++)
        CK_HIP(ctx, hipMemcpyAsync((float*)tr.w.p + ck_cnn_offset(i), w[i], CK_CNN_COUNTS[i] * sizeof(float),
                                   space == CK_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ctx->stream));
    CK_HIP(ctx, hipMemsetAsync(tr.g.p, 0, bytes, ctx->stream));
    CK_HIP(ctx, hipMemsetAsync(tr.m.p, 0, bytes, ctx->stream));
    CK_HIP(ctx, hipMemsetAsync(tr.v.p, 0, bytes, ctx->stream));
    tr.steps = 0;
    tr.alive = true;
    return CK_OK;
}

// Gradients of the mean loss over the n patches d_x (device, n x 40 x 40 x 3) with labels d_lab (device, n bytes, 0..80) into
// tr.g, the per-patch losses into tr.lossv; with want_masks (and dropout) the keep-masks into tr.mask1 .. mask3.
// The batch goes through in chunks of CK_TRAIN_CHUNK patches; the chunks' gradient sums are added in chunk order.
int k_train_grads(ck_ctx* ctx, CkTrainer& tr, const uint8_t* d_x, const uint8_t* d_lab, int n, int drop, uint64_t seed,
                  uint64_t step, bool want_masks)
{
    const int cap = std::min(n, CK_TRAIN_CHUNK);
    const size_t f = sizeof(float);
    CK_TRY(ck_ensure(ctx, tr.a1, cap * 41472 * f));  CK_TRY(ck_ensure(ctx, tr.a2, cap * 32768 * f));
    CK_TRY(ck_ensure(ctx, tr.p1, cap * 8192 * f));   CK_TRY(ck_ensure(ctx, tr.a3, cap * 17640 * f));
    CK_TRY(ck_ensure(ctx, tr.a4, cap * 12960 * f));  CK_TRY(ck_ensure(ctx, tr.p2, cap * 3240 * f));
    CK_TRY(ck_ensure(ctx, tr.h1, cap * 160 * f));    CK_TRY(ck_ensure(ctx, tr.lg, cap * 81 * f));
    CK_TRY(ck_ensure(ctx, tr.dlg, cap * 81 * f));    CK_TRY(ck_ensure(ctx, tr.dh1, cap * 160 * f));
    CK_TRY(ck_ensure(ctx, tr.dp2, cap * 3240 * f));  CK_TRY(ck_ensure(ctx, tr.dz4, cap * 12960 * f));
    CK_TRY(ck_ensure(ctx, tr.dz3, cap * 17640 * f)); CK_TRY(ck_ensure(ctx, tr.dp1, cap * 8192 * f));
    CK_TRY(ck_ensure(ctx, tr.dz2, cap * 32768 * f)); CK_TRY(ck_ensure(ctx, tr.dz1, cap * 41472 * f));
    CK_TRY(ck_ensure(ctx, tr.lossv, (size_t)n * f));
    uint8_t *mk1 = nullptr, *mk2 = nullptr, *mk3 = nullptr;
    if (want_masks && drop) {
        CK_TRY(ck_ensure(ctx, tr.mask1, (size_t)n * 8192)); CK_TRY(ck_ensure(ctx, tr.mask2, (size_t)n * 3240));
        CK_TRY(ck_ensure(ctx, tr.mask3, (size_t)n * 160));
        mk1 = (uint8_t*)tr.mask1.p; mk2 = (uint8_t*)tr.mask2.p; mk3 = (uint8_t*)tr.mask3.p;
    }
    float* W[12];
    float* G[12];
    for (int i = 0; i < 12; i++) { W[i] = (float*)tr.w.p + ck_cnn_offset(i); G[i] = (float*)tr.g.p + ck_cnn_offset(i); }
    float *a1 = (float*)tr.a1.p, *a2 = (float*)tr.a2.p, *p1 = (float*)tr.p1.p, *a3 = (float*)tr.a3.p, *a4 = (float*)tr.a4.p,
          *p2 = (float*)tr.p2.p, *h1 = (float*)tr.h1.p, *lg = (float*)tr.lg.p, *dlg = (float*)tr.dlg.p, *dh1 = (float*)tr.dh1.p,
          *dp2 = (float*)tr.dp2.p, *dz4 = (float*)tr.dz4.p, *dz3 = (float*)tr.dz3.p, *dp1 = (float*)tr.dp1.p, *dz2 = (float*)tr.dz2.p,
          *dz1 = (float*)tr.dz1.p;
    const float keep1 = drop ? 0.75f : 1.0f, keep3 = drop ? 0.5f : 1.0f;
    auto ew = [&](size_t count) { return dim3(cdiv(count, 256)); };

    for (int p0 = 0; p0 < n; p0 += CK_TRAIN_CHUNK) {
        const int c = std::min(CK_TRAIN_CHUNK, n - p0);
        const bool acc = p0 > 0;
        const uint8_t* x = d_x + (size_t)p0 * 4800;
        {
            TimeScope ts(ctx, "train_fwd");
            CK_TRY((gemm_f64<1>(ctx, AIm2col<40, 40, 3, 5, 5, uint8_t>{ { x } }, BRow{ W[0], 32 }, EpBias{ a1, W[1], 32, 1 }, c * 1296, 32, 75)));
            CK_TRY((gemm_f64<1>(ctx, AIm2col<36, 36, 32, 5, 5, float>{ { a1 } }, BRow{ W[2], 32 }, EpBias{ a2, W[3], 32, 1 }, c * 1024, 32, 800)));
            hipLaunchKernelGGL(tr_pool, ew((size_t)c * 8192), dim3(256), 0, ctx->stream, (const float*)a2, p1, c, 32, 32, 32);
            if (drop) CK_TRY(dropout(ctx, p1, 8192, c, p0, seed, step, 0, 0.25f, mk1));
            CK_TRY((gemm_f64<3>(ctx, AIm2col<16, 16, 32, 3, 3, float>{ { p1 } }, BRow{ W[4], 90 }, EpBias{ a3, W[5], 90, 1 }, c * 196, 90, 288)));
            CK_TRY((gemm_f64<3>(ctx, AIm2col<14, 14, 90, 3, 3, float>{ { a3 } }, BRow{ W[6], 90 }, EpBias{ a4, W[7], 90, 1 }, c * 144, 90, 810)));
            hipLaunchKernelGGL(tr_pool, ew((size_t)c * 3240), dim3(256), 0, ctx->stream, (const float*)a4, p2, c, 12, 12, 90);
            if (drop) CK_TRY(dropout(ctx, p2, 3240, c, p0, seed, step, 1, 0.25f, mk2));
            CK_TRY((gemm_f64<3>(ctx, ARow{ p2, 3240 }, BRow{ W[8], 160 }, EpBias{ h1, W[9], 160, 1 }, c, 160, 3240)));
            if (drop) CK_TRY(dropout(ctx, h1, 160, c, p0, seed, step, 2, 0.5f, mk3));
            CK_TRY((gemm_f64<3>(ctx, ARow{ h1, 160 }, BRow{ W[10], 81 }, EpBias{ lg, W[11], 81, 0 }, c, 81, 160)));
            hipLaunchKernelGGL(tr_softmax_xent, dim3(cdiv(c, 64)), dim3(64), 0, ctx->stream, (const float*)lg, d_lab + p0, c, n,
                               (float*)tr.lossv.p + p0, dlg);
            CK_HIP(ctx, hipGetLastError());
        }
        {
            TimeScope ts(ctx, "train_dgrad");
            CK_TRY((gemm<3>(ctx, ARow{ dlg, 81 }, BRowT{ W[10], 81 }, EpGate{ dh1, h1, 160, keep3 }, c, 160, 81)));
            CK_TRY((gemm<3>(ctx, ARow{ dh1, 160 }, BRowT{ W[8], 160 }, EpGate{ dp2, nullptr, 3240, 1.0f }, c, 3240, 160)));
            hipLaunchKernelGGL(tr_pool_back, ew((size_t)c * 12960), dim3(256), 0, ctx->stream, (const float*)a4, (const float*)p2,
                               (const float*)dp2, dz4, c, 12, 12, 90, keep1);
            CK_TRY((gemm<3>(ctx, AFull<14, 14, 90, 3, 3>{ dz4 }, BSwap<90, 90>{ W[6] }, EpGate{ dz3, a3, 90, 1.0f }, c * 196, 90, 810)));
            CK_TRY((gemm<1>(ctx, AFull<16, 16, 90, 3, 3>{ dz3 }, BSwap<32, 90>{ W[4] }, EpGate{ dp1, nullptr, 32, 1.0f }, c * 256, 32, 810)));
            hipLaunchKernelGGL(tr_pool_back, ew((size_t)c * 32768), dim3(256), 0, ctx->stream, (const float*)a2, (const float*)p1,
                               (const float*)dp1, dz2, c, 32, 32, 32, keep1);
            CK_TRY((gemm<1>(ctx, AFull<36, 36, 32, 5, 5>{ dz2 }, BSwap<32, 32>{ W[2] }, EpGate{ dz1, a1, 32, 1.0f }, c * 1296, 32, 800)));
            CK_HIP(ctx, hipGetLastError());
        }
        {
            TimeScope ts(ctx, "train_wgrad");
            CK_TRY((wgrad<3>(ctx, tr, ARowT{ h1, 160, 160 }, BRow{ dlg, 81 }, 161, 81, c, G[10], acc)));
            CK_TRY((wgrad<3>(ctx, tr, ARowT{ p2, 3240, 3240 }, BRow{ dh1, 160 }, 3241, 160, c, G[8], acc)));
            CK_TRY((wgrad<3>(ctx, tr, AIm2colT<14, 14, 90, 3, 3, float>{ { a3 } }, BRow{ dz4, 90 }, 811, 90, c * 144, G[6], acc)));
            CK_TRY((wgrad<3>(ctx, tr, AIm2colT<16, 16, 32, 3, 3, float>{ { p1 } }, BRow{ dz3, 90 }, 289, 90, c * 196, G[4], acc)));
            CK_TRY((wgrad<1>(ctx, tr, AIm2colT<36, 36, 32, 5, 5, float>{ { a1 } }, BRow{ dz2, 32 }, 801, 32, c * 1024, G[2], acc)));
            CK_TRY((wgrad<1>(ctx, tr, AIm2colT<40, 40, 3, 5, 5, uint8_t>{ { x } }, BRow{ dz1, 32 }, 76, 32, c * 1296, G[0], acc)));
        }
    }
    return CK_OK;
}

int k_train_adam(ck_ctx* ctx, CkTrainer& tr, const float* d_g, double lr)
{
    TimeScope ts(ctx, "train_adam");
    const double b1 = 0.9, b2 = 0.999, eps = 1e-8;
    const double t = (double)(tr.steps + 1);
    const double lr_t = lr * sqrt(1.0 - pow(b2, t)) / (1.0 - pow(b1, t));
    hipLaunchKernelGGL(tr_adam, dim3(cdiv(CK_TRAIN_PARAMS, 256)), dim3(256), 0, ctx->stream, (float*)tr.w.p, (float*)tr.m.p,
                       (float*)tr.v.p, d_g, (size_t)CK_TRAIN_PARAMS, lr_t, b1, b2, eps);
    CK_HIP(ctx, hipGetLastError());
    tr.steps++;
    return CK_OK;
}
