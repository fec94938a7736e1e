// kornia_amd - host side of the filter family: the record of one filter2d / filter2d_separable call and the functions that one .hip
// defines and km_filter.hip calls.  Both the defining and the calling file include this header, so the compiler compares the two.
#pragma once

#include "km_common.h"

// The geometry as the kernels of km_filter.hip take it (KmSepArgs / KmFullArgs embed it by value: members and order are kernel-argument layout).
struct KmFilterGeom {
    int B, C, H, W, Bk, kH, kW, border, same;
    int Ho, Wo;   // output size
    int pt, pl;   // top / left padding ('same'), 0 for 'valid'
};

// One call of a km_filter2d* entry point: `KmFilterCall c{{B, C, H, W, Bk, kH, kW, border, same}, dtype, stream}`, then km_filter_validate,
// which checks the arguments and derives Ho, Wo, pt, pl.  A function that takes a value different from the record's says so in an argument.
struct KmFilterCall : KmFilterGeom {
    int dtype;
    hipStream_t s;
};

// large separable kernels, forward (km_filter_sep_big.hip)
int km_filter_sep_big_supported(int kH, int kW, int dtype);
int km_filter_sep_big_run(const KmFilterCall& c, const void* x, const void* kx, const void* ky, void* y);

// register-tiled full kH x kW forward for square odd 3/5/7 kernels (km_filter2d_fast.hip)
int km_filter2d_fast_tapgrad_run(const KmFilterCall& c, const void* gy, const void* x, double* gk);
int km_filter2d_fast_supported(const KmFilterCall& c, const void* x, const void* y);
int km_filter2d_fast_run(const KmFilterCall& c, const void* x, const void* k, void* y, int border, int flip);

// register-tiled fast path for small square odd kernels (km_blur_fast.hip)
int km_blur_fast_supported(const KmFilterCall& c, const void* x, const void* y);
int km_blur_fast_bwd_supported(const KmFilterCall& c, const void* gy, const void* gx);
int km_blur_fast_run(const KmFilterCall& c, bool bwd, const void* x, const void* kx, const void* ky, void* y);
