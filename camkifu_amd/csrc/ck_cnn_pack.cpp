// ck_cnn_pack.cpp -- the stone classifier's weights repacked once into the order its kernels read them (k_cnn.hip,
// k_cnn_bf16.hip, k_cnn_q8.hip).  Host arithmetic only; tests/test_cnn_pack_cpu.py holds every pack to exact bytes.
//
// Every pack but the plain copies is a sequence of MFMA fragments [64 lanes][elements]: lane = kslot * 16 + column, where
// the column is an output channel of a 16-wide tile and the k-slot one of the four quarters of the fragment's K range.
// There is one packer.  A pack is its shape, a map from a destination element (tile, step, lane, e) to the index of its
// weight in the Keras array (-1: padding, stays zero), and the encoder that writes the weight.
#include "ck_cnn_pack.h"

#include <math.h>
#include <string.h>

#include <utility>

namespace {

// ---- encoders: enc(w, d, plane, lane) writes weight w at d; `plane` is the distance from d to the same element of the
// pack's next plane, `lane` the fragment lane d belongs to ---------------------------------------------------------------
struct F32 { typedef float T; void operator()(float w, T* d, size_t, int) const { *d = w; } };
struct F16 { typedef uint16_t T; void operator()(float w, T* d, size_t, int) const { const _Float16 h = (_Float16)w; memcpy(d, &h, 2); } };
// float -> bf16 by the compiler's conversion, and by round to nearest even on the integer: the same bits on finite weights, not on NaN
struct Bf16Cast { typedef uint16_t T; void operator()(float w, T* d, size_t, int) const { const __bf16 b = (__bf16)w; memcpy(d, &b, 2); } };
struct Bf16Rne {
    typedef uint16_t T;
    void operator()(float w, T* d, size_t, int) const { uint32_t u; memcpy(&u, &w, 4); *d = (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16); }
};
// split precision: w x 2^8 as the nearest fp16 (plane 0) and the nearest fp16 of what that leaves (plane 1)
struct Split {
    typedef uint16_t T;
    void operator()(float w, T* d, size_t plane, int) const
    {
        const float wv = w * CK_CNN_WSCALE;
        const _Float16 hi = (_Float16)wv, lo = (_Float16)(wv - (float)hi);
        memcpy(d, &hi, 2);
        memcpy(d + plane, &lo, 2);
    }
};

// OCP e4m3 (no infinities, 0x7F = NaN, largest 448), round to nearest even; the caller keeps |v| <= 448
uint8_t e4m3_of(float v)
{
    if (v == 0.f || v != v) return 0;
    const uint8_t sgn = v < 0 ? 0x80 : 0;
    v = fabsf(v);
    if (v > 448.f) v = 448.f;
    int e;
    float m = frexpf(v, &e);
    e -= 1; m *= 2.f;                               // v = m 2^e, m in [1, 2)
    if (e < -6) return sgn | (uint8_t)lrintf(v * 512.f);        // subnormals: steps of 2^-9 (8 = the smallest normal's code)
    int q = (int)lrintf((m - 1.f) * 8.f);
    if (q == 8) { q = 0; e += 1; }
    if (e > 8 || (e == 8 && q > 6)) { e = 8; q = 6; }
    return sgn | (uint8_t)(((e + 7) << 3) | q);
}

// the e4m3 cross terms of the split weight under the block scale 2^CK_CNN_Q8_SW: lanes 0 .. 31 (groups 0, 1) carry
// w_lo x 2^11, lanes 32 .. 63 (groups 2, 3) w_hi; *wmax follows the largest |w_hi| (-> q8_ok)
struct Cross {
    typedef uint8_t T;
    float* wmax;
    void operator()(float w, T* d, size_t, int lane) const
    {
        const float SW = (float)(1 << CK_CNN_Q8_SW), wv = w * CK_CNN_WSCALE;
        const _Float16 hi = (_Float16)wv;
        const float lo = (float)(_Float16)(wv - (float)hi);
        if (fabsf((float)hi) > *wmax) *wmax = fabsf((float)hi);
        *d = lane < 32 ? e4m3_of(lo * 2048.f / SW) : e4m3_of((float)hi / SW);
    }
};

// ---- the packer ----------------------------------------------------------------------------------------------------------
// [tile][step][plane][64 lanes][elems], or with planes_first [plane][tile][step][64 lanes][elems]; an encoder of two planes
// writes both from the element of the first
struct Shape { int tiles, steps, elems, planes = 1; bool planes_first = false; };

template <class Enc, class Map>
CkBytes pack(Shape s, const float* src, Map map, Enc enc)
{
    typedef typename Enc::T T;
    const size_t frag = (size_t)64 * s.elems, nfrag = (size_t)s.tiles * s.steps;
    const size_t stride = s.planes_first ? frag : frag * s.planes;       // from a (tile, step)'s first fragment to the next one's
    const size_t plane = s.planes_first ? nfrag * frag : frag;
    CkBytes out(nfrag * frag * s.planes * sizeof(T), 0);
    for (int t = 0; t < s.tiles; t++)
        for (int st = 0; st < s.steps; st++) {
            T* d = (T*)out.data() + ((size_t)t * s.steps + st) * stride;
            for (int lane = 0; lane < 64; lane++)
                for (int e = 0; e < s.elems; e++, d++) {
                    const int i = map(t, st, lane, e);
                    if (i >= 0) enc(src[i], d, plane, lane);
                }
        }
    return out;
}

// ---- index maps ------------------------------------------------------------------------------------------------------------
// A Keras kernel [kh][kw][cin][cout] as the correlation the kernels compute: tap (i, j) of the kernels is tap
// (KH - 1 - i, KW - 1 - j) of the array (the flip of the Theano convolution); channels past CIN / COUT are padding.
struct Conv {
    int KH, KW, CIN, COUT;
    int at(int i, int j, int c, int o) const { return c < CIN && o < COUT ? (((KH - 1 - i) * KW + (KW - 1 - j)) * CIN + c) * COUT + o : -1; }
    int tiles() const { return (COUT + 15) / 16; }
};
constexpr Conv C1{5, 5, 3, 32}, C2{5, 5, 32, 32}, C3{3, 3, 32, 90}, C4{3, 3, 90, 90};
constexpr int D1_IN = 3240, D1_OUT = 160;

// B operand pack of conv_mfma16_f32_kernel: [channel tile of 16][group of 4 k-steps][lane = kslot*16 + col][4]
// with K = (kh, kw, cin padded to a multiple of 4) and k = 4*step + kslot; flip applied, padding zero
CkBytes conv_f32(Conv g, const float* k)
{
    const int CINP = (g.CIN + 3) / 4 * 4, KS = g.KH * g.KW * CINP / 4;
    return pack(Shape{g.tiles(), (KS + 3) / 4, 4}, k, [=](int t, int sg, int lane, int e) {
        const int kidx = 4 * (4 * sg + e) + lane / 16, ij = kidx / CINP;
        return ij < g.KH * g.KW ? g.at(ij / g.KW, ij % g.KW, kidx % CINP, t * 16 + lane % 16) : -1;
    }, F32());
}

// 16-bit packs of conv2 .. conv4 in MFMA fragment order: [16-channel tile][k-step][lane = kslot*16 + channel][8 consecutive cin],
// k-step = 32 input channels of one kernel tap; flip applied, padding channels zero.  As bf16 for the bf16 kernels; as split-precision
// packs: weights x 2^8 as hi / lo fp16 planes, [16-channel tile][k-step][plane][lane = kslot*16 + channel][8 consecutive cin]
template <class Enc>
CkBytes conv_k32(Conv g, const float* k, int planes, Enc enc)
{
    const int NB = (g.CIN + 31) / 32;
    return pack(Shape{g.tiles(), g.KH * g.KW * NB, 8, planes}, k, [=](int t, int st, int lane, int e) {
        const int ij = st / NB;
        return g.at(ij / g.KW, ij % g.KW, 32 * (st % NB) + 8 * (lane / 16) + e, t * 16 + lane % 16);
    }, enc);
}

// conv1's weights for conv12_bf16_kernel: fp16 A fragments [channel tile][k-step][lane = kslot * 16 + channel][8] (layout at
// the kernel): the 15 units f = 4 * step + kslot of (kernel row f / 3, kernel columns 2 * (f % 3) and + 1), the 8 elements
// two columns x cin padded to 4.  For conv12_q8_kernel: both planes of w x 2^8 in the same fragment order, [plane][...]
template <class Enc>
CkBytes conv1_rows(const float* k1, int planes, Enc enc)
{
    return pack(Shape{2, 4, 8, planes, true}, k1, [](int t, int s, int lane, int e) {
        const int f = 4 * s + lane / 16, j = 2 * (f % 3) + (e >> 2);
        return f > 14 || j > 4 ? -1 : C1.at(f / 3, j, e & 3, t * 16 + lane % 16);
    }, enc);
}

// cross-term weights of a convolution: [channel tile][unit pair][lane][32 bytes].  A unit is 32 input channels of one tap;
// `pairs` lists the two units (tap, channel block) of every scaled MFMA, -1 for an empty half.  Lane = group * 16 + output
// channel; group 0 / 1: w_lo of input channels 0..15 / 16..31 of the unit, group 2 / 3: w_hi.  Weights x 2^8, flip applied.
struct Unit { int i, j, cc; };
typedef std::vector<std::pair<Unit, Unit>> Pairs;
constexpr Unit NONE{-1, 0, 0};

CkBytes cross(Conv g, const float* k, const Pairs& pairs, float* wmax)
{
    return pack(Shape{g.tiles(), (int)pairs.size(), 32}, k, [&](int t, int u, int lane, int e) {
        const Unit& un = e < 16 ? pairs[u].first : pairs[u].second;
        return un.i < 0 ? -1 : g.at(un.i, un.j, 32 * un.cc + 16 * ((lane / 16) & 1) + e % 16, t * 16 + lane % 16);
    }, Cross{wmax});
}

// conv2 (K = 5), conv3 (K = 3): per kernel row the column pairs (0, 1), (2, 3) .. with the last column alone, then the last
// column's taps paired vertically.  (The kernels read the vertical pairs and never the lone halves of the rows, but their
// fragment index is row * ceil(K / 2) + pair: the slots stay.)
Pairs pairs_rows(int K)
{
    Pairs pr;
    for (int i = 0; i < K; i++)
        for (int j = 0; j < K; j += 2) pr.push_back({Unit{i, j, 0}, j + 1 < K ? Unit{i, j + 1, 0} : NONE});
    for (int i = 0; i < K; i += 2) pr.push_back({Unit{i, K - 1, 0}, i + 1 < K ? Unit{i + 1, K - 1, 0} : NONE});
    return pr;
}

Pairs pairs_conv4()
{   // pairs of consecutive k-steps (step = tap * 3 + channel block), the 27th alone
    Pairs pr;
    for (int s = 0; s < 27; s += 2)
        pr.push_back({Unit{s / 9, (s / 3) % 3, s % 3}, s + 1 < 27 ? Unit{(s + 1) / 9, ((s + 1) / 3) % 3, (s + 1) % 3} : NONE});
    return pr;
}

}  // namespace

void ck_cnn_pack(const float* const w[12], CnnPacks& P)
{
    const float *k1 = w[0], *k2 = w[2], *k3 = w[4], *k4 = w[6], *d1 = w[8];
    auto plain = [&](int i) { return CkBytes((const uint8_t*)w[i], (const uint8_t*)(w[i] + CK_CNN_COUNTS[i])); };
    P.c1b = plain(1); P.c2b = plain(3); P.c3b = plain(5); P.c4b = plain(7);
    P.d1b = plain(9); P.d2w = plain(10); P.d2b = plain(11);
    // ---- fp32 mode
    // A operand of conv1_mfma16_kernel: [channel tile][step][lane = kslot*16 + channel], K = 75 dense
    // in (kh, kw, cin) order, k = 4*step + kslot, flip applied, k = 75 zero
    P.c1w = pack(Shape{2, 19, 1}, k1, [](int t, int s, int lane, int) {
        const int kk = 4 * s + lane / 16;
        return kk < 75 ? C1.at(kk / 15, (kk % 15) / 3, kk % 3, t * 16 + lane % 16) : -1;
    }, F32());
    P.c2w = conv_f32(C2, k2);
    P.c3w = conv_f32(C3, k3);
    P.c4w = conv_f32(C4, k4);
    // A operand pack of fc1_mfma16_kernel: [output tile of 16][pair of k-steps][lane = kslot*16 + output][2],
    // k = 4*step + kslot ascending
    P.d1w = pack(Shape{D1_OUT / 16, D1_IN / 8, 2}, d1, [](int t, int sg, int lane, int e) {
        return (4 * (2 * sg + e) + lane / 16) * D1_OUT + t * 16 + lane % 16;
    }, F32());
    // ---- bf16 mode
    P.c2w_bf = conv_k32(C2, k2, 1, Bf16Rne());
    P.c3w_bf = conv_k32(C3, k3, 1, Bf16Rne());
    P.c4w_bf = conv_k32(C4, k4, 1, Bf16Rne());
    P.c1w_f16 = conv1_rows(k1, 1, F16());
    // dense-1 weights for fc1_bf16_kernel: bf16 A fragments [output tile][k-step][lane = kslot * 16 + output][8], k = px * 96 + ch over the
    // padded maps; `d1` is the Keras matrix [3240 = px * 90 + ch][160]
    P.d1w_bfp = pack(Shape{D1_OUT / 16, 36 * 96 / 32, 8}, d1, [](int t, int st, int lane, int e) {
        const int k = 32 * st + 8 * (lane / 16) + e, c = k % 96;
        return c < 90 ? (k / 96 * 90 + c) * D1_OUT + 16 * t + lane % 16 : -1;
    }, Bf16Cast());
    // ---- split-precision mode
    // conv1: [channel tile][step][plane][lane][8]; k = (kernel row 2*step + kslot/2, slot 8*(kslot%2) + e), slot = kw*3 + cin
    P.c1w_h2 = pack(Shape{2, 3, 8, 2}, k1, [](int t, int st, int lane, int e) {
        const int kq = lane / 16, i = 2 * st + (kq >> 1), slot = 8 * (kq & 1) + e;
        return i > 4 || slot > 14 ? -1 : C1.at(i, slot / 3, slot % 3, t * 16 + lane % 16);
    }, Split());
    P.c2w_h2 = conv_k32(C2, k2, 2, Split());
    P.c3w_h2 = conv_k32(C3, k3, 2, Split());
    P.c4w_h2 = conv_k32(C4, k4, 2, Split());
    // dense1 for fc1_h2_kernel: [output tile][k-step][plane][lane = kslot*16 + output][8 consecutive k], weights x 2^8;
    // 104 k-steps: the 3240 inputs, then zeros up to 3328
    P.d1w_h2 = pack(Shape{D1_OUT / 16, 104, 8, 2}, d1, [](int t, int st, int lane, int e) {
        const int k = 32 * st + 8 * (lane / 16) + e;
        return k < D1_IN ? k * D1_OUT + 16 * t + lane % 16 : -1;
    }, Split());
    // ---- e4m3 mode (it reads the split packs of conv2 .. conv4 as well).  Weights beyond the e4m3 range of their block scale:
    // the mode is not available with them (k_cnn_predict then runs the three-MFMA kernels instead)
    float wmax = 0.f;
    P.c1w_q8 = conv1_rows(k1, 2, Split());
    P.c2x_q8 = cross(C2, k2, pairs_rows(5), &wmax);
    P.c3x_q8 = cross(C3, k3, pairs_rows(3), &wmax);
    P.c4x_q8 = cross(C4, k4, pairs_conv4(), &wmax);
    P.q8_ok = wmax <= 448.f * (float)(1 << CK_CNN_Q8_SW);
}

#define F(m) { #m, &CnnPacks::m }
const CnnPackName CK_CNN_PACK_NAMES[CK_CNN_NPACKS] = {
    F(c1w), F(c1b), F(c2w), F(c2b), F(c3w), F(c3b), F(c4w), F(c4b), F(d1w), F(d1b), F(d2w), F(d2b),
    F(c2w_bf), F(c3w_bf), F(c4w_bf), F(c1w_f16), F(d1w_bfp),
    F(c1w_h2), F(c2w_h2), F(c3w_h2), F(c4w_h2), F(d1w_h2), F(c1w_q8), F(c2x_q8), F(c3x_q8), F(c4x_q8),
};
#undef F

extern "C" long long ck_cnn_pack_probe(const float* const w[12], const char* name, void* dst, size_t cap, int* q8_ok)
{
    CnnPacks P;
    ck_cnn_pack(w, P);
    if (q8_ok) *q8_ok = P.q8_ok;
    for (const CnnPackName& f : CK_CNN_PACK_NAMES)
        if (!strcmp(f.name, name)) {
            const CkBytes& b = P.*f.bytes;
            if (dst && cap) memcpy(dst, b.data(), b.size() < cap ? b.size() : cap);
            return (long long)b.size();
        }
    return -1;
}

extern "C" void ck_cnn_e4m3_probe(const float* v, size_t n, uint8_t* out)
{
    for (size_t i = 0; i < n; i++) out[i] = e4m3_of(v[i]);
}
