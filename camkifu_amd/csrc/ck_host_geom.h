// ck_host_geom.h -- what ck_host_geom.cpp defines (host only, no HIP): included by the file itself, by ck_common.h and by
// the stand-alone sanitizer programs, so that a definition and its callers cannot drift apart
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "../../include/camkifu_amd.h"

void ck_invert3x3(const double* s, double* d);
void ck_min_area_rect(const int32_t* pts, int n, float* out_wh);
void ck_min_area_rect_box(const int32_t* pts, int n, float* out_wha);     // + angle in degrees (cv2.minAreaRect's box[2])
std::vector<int32_t> ck_hull_points(const int32_t* pts, int n);           // strictly convex hull, x0, y0, x1, y1, ...
// the host decisions of k_board_lines, per frame, over parallel arrays of the frame's components
extern "C" int ck_board_round_want(int round, int nc, const double* ub, const double* area, const uint8_t* known, uint8_t* want);
extern "C" int ck_board_rank(int nc, const int32_t* root, const double* area, const uint8_t* known, int h, int w,
                             int32_t* sel, ck_board_result* res);
extern "C" int ck_hough_slab(int n, int h, int w, int small_n, int max_threads, size_t* row_bytes, int* rb, int* threads);
extern "C" void ck_peaks_to_lines(const int32_t* peaks, int np, int numrho, int cap, float* lines);
