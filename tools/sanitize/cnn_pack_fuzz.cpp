// cnn_pack_fuzz.cpp -- the classifier's weight packer (camkifu_amd/csrc/ck_cnn_pack.cpp, linked on its own) under
// AddressSanitizer + UBSan: random, denormal, huge and NaN / infinite weight sets are packed whole.  Every array lives in a
// heap block of exactly its size, so a read one float outside it is caught, as is a write outside a pack; the sizes of the
// packs and q8_ok are checked against what the kind of weights implies.
//
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/sanitize/cnn_pack_fuzz.cpp camkifu_amd/csrc/ck_cnn_pack.cpp
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>

#include "../../camkifu_amd/csrc/ck_cnn_pack.h"

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t next() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static float uniform() { return (float)((next() >> 40) / 16777216.0) * 2.f - 1.f; }       // [-1, 1)

enum Kind { RANDOM, DENORMAL, HUGE_W, NONFINITE, ZERO, NKINDS };
static const char* const KIND_NAMES[NKINDS] = { "random", "denormal", "huge", "nan / inf", "zero" };

static float draw(Kind kind)
{
    switch (kind) {
    case RANDOM: return uniform() * 0.1f;
    case DENORMAL: return uniform() * 1e-39f;                  // f32 denormals; x 2^8 they underflow fp16 altogether
    case HUGE_W: return uniform() * 3e38f;                     // x 2^8 overflows f32, fp16 and e4m3
    case NONFINITE: {
        const uint64_t r = next() % 4;
        return r == 0 ? NAN : r == 1 ? INFINITY : r == 2 ? -INFINITY : uniform();
    }
    default: return 0.f;
    }
}

int main()
{
    static const size_t bytes[CK_CNN_NPACKS] = {
        2 * 19 * 64 * 4, 32 * 4, 2 * 50 * 256 * 4, 32 * 4, 6 * 18 * 256 * 4, 90 * 4, 6 * 52 * 256 * 4, 90 * 4, 10 * 405 * 128 * 4, 160 * 4,
        160 * 81 * 4, 81 * 4, 2 * 25 * 512 * 2, 6 * 9 * 512 * 2, 6 * 27 * 512 * 2, 2 * 4 * 512 * 2, 10 * 108 * 512 * 2,
        2 * 3 * 1024 * 2, 2 * 25 * 1024 * 2, 6 * 9 * 1024 * 2, 6 * 27 * 1024 * 2, 10 * 104 * 1024 * 2,
        2 * 2 * 4 * 512 * 2, 2 * 18 * 2048, 6 * 8 * 2048, 6 * 14 * 2048,
    };
    for (int kind = 0; kind < NKINDS; kind++)
        for (int round = 0; round < 3; round++) {
            std::unique_ptr<float[]> w[12];
            const float* ptr[12];
            for (int i = 0; i < 12; i++) {
                w[i].reset(new float[CK_CNN_COUNTS[i]]);
                for (size_t k = 0; k < CK_CNN_COUNTS[i]; k++) w[i][k] = draw((Kind)kind);
                ptr[i] = w[i].get();
            }
            CnnPacks P;
            ck_cnn_pack(ptr, P);
            for (int k = 0; k < CK_CNN_NPACKS; k++)
                if ((P.*CK_CNN_PACK_NAMES[k].bytes).size() != bytes[k]) {
                    fprintf(stderr, "%s weights: pack %s has %zu bytes, not %zu\n", KIND_NAMES[kind], CK_CNN_PACK_NAMES[k].name,
                            (P.*CK_CNN_PACK_NAMES[k].bytes).size(), bytes[k]);
                    return 2;
                }
            // 0.1 x 2^8 = 25.6 and the denormals lie inside the e4m3 range of the block scale (1792); 3e38 x 2^8 and inf do not
            const bool want_ok = kind == RANDOM || kind == DENORMAL || kind == ZERO;
            if (P.q8_ok != want_ok) { fprintf(stderr, "%s weights: q8_ok = %d\n", KIND_NAMES[kind], (int)P.q8_ok); return 2; }
            if (memcmp(P.d2w.data(), ptr[10], P.d2w.size())) { fprintf(stderr, "d2w is not a copy\n"); return 2; }
            // the probe: an unknown name, a short buffer
            uint8_t few[7];
            int ok = -1;
            if (ck_cnn_pack_probe(ptr, "nothing", few, sizeof few, &ok) != -1 || ok != (int)want_ok) return 2;
            if (ck_cnn_pack_probe(ptr, "c4x_q8", few, sizeof few, nullptr) != (long long)bytes[25]) return 2;
        }
    float v[6] = { 0.f, -0.f, NAN, INFINITY, -1e-30f, 500.f };
    uint8_t code[6];
    ck_cnn_e4m3_probe(v, 6, code);
    if (code[0] || code[1] || code[2] || code[3] != 0x7E || code[4] != 0x80 || code[5] != 0x7E) { fprintf(stderr, "e4m3 edge codes\n"); return 2; }
    printf("cnn weight packer: %d kinds of weight sets x 3 packed clean\n", (int)NKINDS);
    return 0;
}
