// ck_png.h -- the host half of the PNG reader and writer (ck_png.cpp): plain C++, no HIP, no libz.  Reading: the chunk walk,
// an inflate of its own whose verdict is zlib's, the check of the filter bytes.  Writing: the steps of ck_png_stage.h run in
// plain loops (the staged encoder) and the container around a zlib stream.  Status codes are those of camkifu_amd.h; `msg`
// is a buffer of CK_PNG_MSG bytes that receives the cause of a refusal.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "../../include/camkifu_amd.h"

constexpr int CK_PNG_MSG = 200;
// the cap on what is read and written: sides up to 65535 (what the JPEG calls take) and 2^28 pixels, so that the inflated
// rows of a frame (at most 8 bytes a pixel and one a row) stay below 2^31 + 2^16 bytes
constexpr int CK_PNG_MAX_SIDE = 65535;
constexpr long long CK_PNG_MAX_PIXELS = 1LL << 28;

struct CkPngHead {
    int32_t h = 0, w = 0, color_type = 0, bit_depth = 0;
    int32_t channels = 0, bpp = 0;                           // samples of a pixel; the filters' byte distance (1 below 8 bits a pixel)
    int32_t palette_n = 0;                                   // entries of PLTE (0: none)
    int64_t rowbytes = 0;                                    // of a row without its filter byte
    uint8_t palette[768] = {0};                              // R, G, B
    const uint8_t* z = nullptr;                              // the zlib stream of the IDAT chunks: inside the file when there is one
    size_t zlen = 0;                                         // chunk, else in `joined`
    std::vector<uint8_t> joined;
    size_t inflated() const { return (size_t)h * (size_t)(1 + rowbytes); }
};

uint32_t ck_png_crc32(const uint8_t* p, size_t n, uint32_t crc = 0);
uint32_t ck_png_adler32(const uint8_t* p, size_t n, uint32_t adler = 1);
// signature, chunks and their CRCs, IHDR's fields -> hd (which points into `data`)
int ck_png_walk(const uint8_t* data, size_t len, CkPngHead* hd, char* msg);
// a zlib stream -> its bytes: the first `cap` of them into out (nullable when cap is 0), the count of all of them in *total.
// The verdict is zlib's, whatever cap is: wrapper, blocks, distances, Adler-32 over every byte.
int ck_png_unzip(const uint8_t* z, size_t zlen, uint8_t* out, size_t cap, size_t* total, char* msg);
// the filtered rows of a walked file -> rows (hd.inflated() bytes); refuses a short stream and a filter byte above 4
int ck_png_rows(const CkPngHead& hd, uint8_t* rows, char* msg);

// The same inflate through the steps of ck_png_inflate_stage.h in plain loops, in the order the kernel of k_png_inflate.hip
// runs them: the same bytes, status and message as ck_png_unzip for every input.  record (nullable) receives the verdict.
struct CkInfRecord;
int ck_png_unzip_staged(const uint8_t* z, size_t zlen, uint8_t* out, size_t cap, size_t* total, CkInfRecord* record, char* msg);
// with h > 0 the two checks of ck_png_rows follow the inflate: h rows of 1 + rowbytes bytes, filter bytes up to 4
int ck_png_unzip_staged_rows(const uint8_t* z, size_t zlen, uint8_t* out, size_t cap, size_t* total, CkInfRecord* record, char* msg, int h, long long rowbytes);
// a verdict record -> the text ck_png_unzip / ck_png_rows give for it (h, rowbytes: for the two causes of ck_png_rows)
void ck_png_inflate_message(const CkInfRecord& r, int h, long long rowbytes, char* msg);

// ---- writing ----
// a whole file around a zlib stream of zlen bytes: signature, IHDR (8-bit RGB), one IDAT, IEND
constexpr size_t CK_PNG_CONTAINER = 8 + 25 + 12 + 12;
size_t ck_png_wrap(const uint8_t* z, size_t zlen, int h, int w, uint8_t* out);
// the most bytes a file of an h x w frame can have: every literal 15 bits
size_t ck_png_bound(int h, int w);
// n BGR frames through the steps of ck_png_stage.h on the host -> files at out + f * stride, their sizes in len.
// filter: 0 .. 4 forces one type, -1 chooses per row.  runs: 0 literals only, 1 the runs mode (runs of equal bytes inside a
// band as matches of distance 1); ck_png_bound covers both.
int ck_png_stage_encode(const uint8_t* bgr, int n, int h, int w, int filter, uint8_t* out, size_t stride, size_t* len, char* msg, int runs = 0);
