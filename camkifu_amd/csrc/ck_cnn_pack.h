// ck_cnn_pack.h -- the stone classifier's weights as its kernels read them (ck_cnn_pack.cpp): the twelve Keras arrays in,
// every device buffer of CnnWeights out as host bytes.  No HIP and no context in here: tests/test_cnn_pack_cpu.py pins every
// byte without a GPU, and tools/sanitize/cnn_pack_fuzz.cpp links ck_cnn_pack.cpp on its own.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

// floats in each of the twelve arrays c1w c1b c2w c2b c3w c3b c4w c4b d1w d1b d2w d2b (Keras-1 'tf' layout: [kh][kw][cin][cout],
// [in][out]), and in front of array i where the twelve lie end to end (the trainer's flat arrays)
constexpr size_t CK_CNN_COUNTS[12] = { 5 * 5 * 3 * 32, 32, 5 * 5 * 32 * 32, 32, 3 * 3 * 32 * 90, 90,
                                       3 * 3 * 90 * 90, 90, 3240 * 160, 160, 160 * 81, 81 };
constexpr size_t ck_cnn_offset(int i)
{
    size_t o = 0;
    for (int k = 0; k < i; k++) o += CK_CNN_COUNTS[k];
    return o;
}

// the split-precision and the e4m3 packs hold w x 2^8 (the lo halves stay normal fp16); the e4m3 weight operands carry the
// block scale 2^2 (H2_WSCALE of k_cnn.hip, Q8_WSCALE and Q8_SW of k_cnn_q8.hip)
constexpr float CK_CNN_WSCALE = 256.f;
constexpr int CK_CNN_Q8_SW = 2;

typedef std::vector<uint8_t> CkBytes;

// one member per DevBuf of CnnWeights (ck_common.h), same names, same order
struct CnnPacks {
    CkBytes c1w, c1b, c2w, c2b, c3w, c3b, c4w, c4b, d1w, d1b, d2w, d2b;
    CkBytes c2w_bf, c3w_bf, c4w_bf, c1w_f16, d1w_bfp;
    CkBytes c1w_h2, c2w_h2, c3w_h2, c4w_h2, d1w_h2;
    CkBytes c1w_q8, c2x_q8, c3x_q8, c4x_q8;
    bool q8_ok = false;      // every weight inside the e4m3 range of its block scale
};
constexpr int CK_CNN_NPACKS = 26;
struct CnnPackName { const char* name; CkBytes CnnPacks::*bytes; };
extern const CnnPackName CK_CNN_PACK_NAMES[CK_CNN_NPACKS];

// every pack of a weight set (host pointers) and q8_ok
void ck_cnn_pack(const float* const w[12], CnnPacks& out);

// Test hook (not part of the C-ABI of include/camkifu_amd.h): packs the weight set and copies the pack called `name` to
// dst (at most cap bytes).  -> the pack's size in bytes, -1 for an unknown name; *q8_ok (nullable) gets the set's flag.
extern "C" long long ck_cnn_pack_probe(const float* const w[12], const char* name, void* dst, size_t cap, int* q8_ok);
// ... and the e4m3 encoder of the cross-term packs on n values: out[i] = the code of v[i]
extern "C" void ck_cnn_e4m3_probe(const float* v, size_t n, uint8_t* out);
