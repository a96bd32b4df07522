// ck_jpeg.h -- the host half of the JPEG decoder (ck_jpeg.cpp): marker parser and Huffman decoder of baseline JPEG.
// No HIP and no context in here: tools/sanitize/jpeg_fuzz.cpp links ck_jpeg.cpp on its own.
//
// Accepted: SOF0, 8-bit samples, one component (grey) or three taken as Y Cb Cr (any component ids) with luma sampling
// 1x1, 2x1 or 2x2 and chroma 1x1, one interleaved scan; restart intervals; a frame without DHT gets the tables of Annex K.3
// (Motion-JPEG in AVI).  Everything else is refused with CK_ERR_DATA and a message that names the cause.  Every read is
// bounded by the buffer: no input byte can cause an access outside it or a loop without an end.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/camkifu_amd.h"

#define CK_JPEG_MSG 160

struct CkHuff {
    bool present = false;
    uint16_t look[512];          // the next 9 bits -> (length << 8) | symbol, 0 where the code is longer
    int32_t maxcode[18];         // largest code of each length (-1: none), [17] a sentinel
    int32_t valoff[17];          // index of the first symbol of each length minus its first code
    uint8_t vals[256];
};

struct CkJpegFrame {
    ck_jpeg_info info{};
    int ncomp = 0;
    int hs = 1, vs = 1;          // luma blocks per MCU, across and down
    int mcux = 0, mcuy = 0;      // MCUs across and down
    uint16_t quant[3][64];       // natural order, by component
    CkHuff dc[3], ac[3];         // by component, selectors resolved
    size_t scan = 0;             // offset of the entropy-coded segment
};

// geometry of a sampling: blocks per frame and the block grid of each component
static inline int ck_jpeg_luma_h(int sampling) { return sampling >= CK_JPEG_422 ? 2 : 1; }
static inline int ck_jpeg_luma_v(int sampling) { return sampling == CK_JPEG_420 ? 2 : 1; }
static inline long long ck_jpeg_blocks(int h, int w, int sampling)
{
    const int hs = ck_jpeg_luma_h(sampling), vs = ck_jpeg_luma_v(sampling);
    const long long mx = (w + 8 * hs - 1) / (8 * hs), my = (h + 8 * vs - 1) / (8 * vs);
    return mx * my * (hs * vs + (sampling == CK_JPEG_GREY ? 0 : 2));
}

// headers up to the scan -> *f.  CK_OK, CK_ERR_ARG (NULL / empty) or CK_ERR_DATA; msg (CK_JPEG_MSG bytes) says why.
int ck_jpeg_parse(const uint8_t* data, size_t len, CkJpegFrame* f, char* msg);
// the scan of a parsed frame -> coef: info.blocks * 64 int16, component-planar, blocks in raster order over the MCU-padded
// grid, natural order inside a block, not dequantised (zeroed here first).  CK_OK or CK_ERR_DATA.
int ck_jpeg_entropy(const uint8_t* data, size_t len, const CkJpegFrame& f, int16_t* coef, char* msg);
