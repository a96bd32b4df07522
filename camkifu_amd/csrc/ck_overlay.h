// ck_overlay.h -- the host half of the overlay rasteriser (ck_overlay.cpp): validation of a display list, the record the
// kernel reads per primitive, and the plan that bins the primitives.  No HIP and no context in here:
// tools/sanitize/overlay_fuzz.cpp links ck_overlay.cpp on its own.
#pragma once
#include <stdint.h>

#define CK_OV_BIN 32        // side of a bin in pixels: one workgroup of k_overlay.hip draws one bin
#define CK_OV_PRIM 8        // int32 per primitive of a display list
#define CK_OV_REC 12        // int32 per record: the primitive, normalised, and its bounding box
#define CK_OV_MSG 200

// CK_OK, or CK_ERR_ARG and why in msg (CK_OV_MSG bytes): every limit of include/camkifu_amd.h, "overlays"
int ck_overlay_check(int n, int h, int w, const int32_t* prims, const int32_t* frame_start, int text_len, char* msg);

// one VALID primitive -> the record the kernel tests pixels against:
//   {kind, x0, y0, x1, y1, size, colour, aux, bx0, by0, bx1, by1}, the box inclusive and empty when bx1 < bx0
//   SEGMENT  endpoints in lexicographic order (so x1 >= x0)        RECT  x0 <= x1, y0 <= y1
//   CIRCLE   size = the outer disc's radius, x1 = the inner disc's (-1: none)
// the box is the primitive's own, not clipped to any image
void ck_overlay_record(const int32_t* prim, int32_t* rec);
