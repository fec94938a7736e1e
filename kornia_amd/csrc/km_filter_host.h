// kornia_amd - host side of the filter family: the functions that one .hip defines and km_filter.hip calls.  Both the defining
// and the calling file include this header, so the compiler compares the two.
#pragma once

#include "km_common.h"

// large separable kernels, forward (km_filter_sep_big.hip)
int km_filter_sep_big_supported(int kH, int kW, int dtype);
int km_filter_sep_big_run(const void* x, const void* kx, const void* ky, void* y, int B, int C, int H, int W, int Bk, int kH, int kW,
                          int border, int same, int dtype, hipStream_t s);

// register-tiled full kH x kW forward for square odd 3/5/7 kernels (km_filter2d_fast.hip)
int km_filter2d_fast_tapgrad_run(const void* gy, const void* x, double* gk, int B, int C, int H, int W, int Bk, int K, int border, int dtype,
                                 hipStream_t s);
int km_filter2d_fast_supported(const void* x, const void* y, int H, int W, int kH, int kW, int border, int same, int dtype);
int km_filter2d_fast_run(const void* x, const void* k, void* y, int B, int C, int H, int W, int Bk, int K, int border, int flip, int dtype,
                         hipStream_t s);

// register-tiled fast path for small square odd kernels (km_blur_fast.hip)
int km_blur_fast_supported(const void* x, const void* y, int H, int W, int kH, int kW, int border, int same, int dtype);
int km_blur_fast_bwd_supported(const void* gy, const void* gx, int H, int W, int kH, int kW, int border, int same, int dtype);
int km_blur_fast_run(bool bwd, const void* x, const void* kx, const void* ky, void* y, int B, int C, int H, int W, int Bk, int K,
                     int border, int dtype, hipStream_t s);
