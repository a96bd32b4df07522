// ck_jpeg_enc.h -- the host half of the JPEG encoder (ck_jpeg_enc.cpp): quant tables from a quality, JFIF headers and the
// Huffman coder of baseline JPEG, byte for byte what libjpeg's default compressor writes.  No HIP and no context in here:
// tools/sanitize/jpeg_enc_fuzz.cpp links ck_jpeg_enc.cpp and ck_jpeg.cpp on their own.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ck_jpeg.h"
#include "ck_jpeg_enc_stage.h"

#define CK_JPEG_ENC_HEADER_BOUND 1024   // SOI, APP0, 2 DQT, SOF0, 4 DHT, DRI, SOS, EOI: 629 bytes

// jpeg_set_quality(quality, force_baseline) over the tables of Annex K.1 / K.2 -> quant[3][64], natural order, by component
// (Y, Cb, Cr; the two chroma tables are equal).  quality is clamped to 1 .. 100.
void ck_jpeg_enc_quant(int quality, uint16_t* quant);

// the largest stream a frame of this geometry can become: 26 bits per coefficient (a 16-bit code and 10 value bits) doubled
// for byte stuffing, 4 bytes per MCU (padding of a restart interval, its stuffing, the marker), 1024 for the headers.
// 0 for a geometry the encoder refuses.
size_t ck_jpeg_enc_bound(int h, int w, int sampling);

// coef (ck_jpeg_blocks * 64 int16, the layout of ck_jpeg_entropy) + quant[3][64] -> one stream at out, *len bytes of at most
// cap.  CK_OK; CK_ERR_ARG for a geometry, table or restart interval outside baseline JPEG, a coefficient the tables of
// Annex K.3 have no code for (a DC difference above 11 bits, an AC value above 10) and a buffer that is too small: nothing
// is written beyond cap, whatever the coefficients are.  msg (CK_JPEG_MSG bytes) says why.
int ck_jpeg_enc_entropy(const int16_t* coef, const uint16_t* quant, int h, int w, int sampling, int restart_interval,
                        uint8_t* out, size_t cap, size_t* len, char* msg);

// the encode tables of Annex K.3 (built once) and the zigzag order, as the steps of ck_jpeg_enc_stage.h take them
const CkEncTables& ck_jpeg_enc_tables();
const uint8_t* ck_jpeg_enc_zigzag();

// everything in front of the entropy-coded data, in libjpeg's order -> out (CK_JPEG_ENC_HEADER_BOUND bytes of room); returns
// the bytes written.  The arguments are those ck_jpeg_enc_entropy has accepted.
size_t ck_jpeg_enc_headers(const uint16_t* quant, int h, int w, int sampling, int restart_interval, uint8_t* out);

// what ck_jpeg_enc_entropy refuses before it reads a coefficient (geometry, restart interval, quant tables), with its message
int ck_jpeg_enc_check(const uint16_t* quant, int h, int w, int sampling, int restart_interval, char* msg);

// a status word of ck_enc_block_bits (ck_jpeg_enc_stage.h) as ck_jpeg_enc_entropy words the refusal
void ck_jpeg_enc_status_message(uint32_t status, long long mcu, char* msg);

// ck_jpeg_enc_entropy for n frames (coef: n frames end to end, out + f * stride, len[f]) through the steps of
// ck_jpeg_enc_stage.h -- size, scan, put, stuff -- in plain loops over the tiles the kernels of k_jpeg_enc_huff.hip use: the
// same bytes, the same refusals.  On a refusal *bad is the lowest frame that has one and msg what ck_jpeg_enc_entropy says
// of it (the lowest MCU); every len[f] is 0 then.  stride is at least ck_jpeg_enc_bound.
int ck_jpeg_enc_staged(const int16_t* coef, const uint16_t* quant, int n, int h, int w, int sampling, int restart_interval,
                       uint8_t* out, size_t stride, size_t* len, int* bad, char* msg);

// ---- optimised Huffman tables (libjpeg's optimize_coding): tables fitted to each frame, the same coefficients ----
// the symbols ck_jpeg_enc_entropy would emit for the frame, counted: freq[4][256], table t = 2 * chroma + ac (the order of
// the DHT segments).  CK_ERR_ARG with the coder's message for a coefficient it refuses, and for a frame of more than 2^25
// blocks (the counters have 32 bits).
int ck_jpeg_enc_histogram(const int16_t* coef, int h, int w, int sampling, int restart_interval, uint32_t* freq, char* msg);
// jpeg_gen_optimal_table: freq[256] -> bits[16] (codes of length 1 .. 16) and vals[256], of which *count are used
void ck_jpeg_enc_optimal_table(const uint32_t* freq, uint8_t* bits, uint8_t* vals, int32_t* count);
// ck_jpeg_enc_entropy with the frame's own tables in its DHT segments: two passes over the coefficients.  The same
// refusals, made in the first pass; the room an MCU needs is that of codes of 16 bits throughout.
int ck_jpeg_enc_entropy_opt(const int16_t* coef, const uint16_t* quant, int h, int w, int sampling, int restart_interval,
                            uint8_t* out, size_t cap, size_t* len, char* msg);
// ck_jpeg_enc_staged with the histo and tables steps in front: the bytes and refusals of ck_jpeg_enc_entropy_opt
int ck_jpeg_enc_staged_opt(const int16_t* coef, const uint16_t* quant, int n, int h, int w, int sampling, int restart_interval,
                           uint8_t* out, size_t stride, size_t* len, int* bad, char* msg);
// the header without its DHT segments: SOI .. SOF0 -> pre (CK_ENC_HEADER_SLOT bytes of room), DRI and SOS -> post (64)
void ck_jpeg_enc_header_parts(const uint16_t* quant, int h, int w, int sampling, int restart_interval, uint8_t* pre, uint32_t* pre_len,
                              uint8_t* post, uint32_t* post_len);
static_assert(CK_ENC_HEADER_SLOT == CK_JPEG_ENC_HEADER_BOUND, "a frame's header slot on the device is the header bound");
