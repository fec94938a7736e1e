// kornia_amd - ATen's source index of a bilinear resize along one axis, shared by the resize kernels (km_pyramid.hip) and the batched
// crop -> resize (km_crop_resize.hip).
#pragma once

#include "km_common.h"

// ATen area_pixel_compute_scale / area_pixel_compute_source_index (bilinear: negative sources clamp to 0)
template <typename R>
__device__ __forceinline__ void kmp_axis(int d, int n_in, int n_out, int align, int& i0, int& i1, R& l0, R& l1) {
    R src;
    if (align) {
        const R scale = n_out > 1 ? (R)(n_in - 1) / (R)(n_out - 1) : (R)0;
        src = scale * (R)d;
    } else {
        const R scale = (R)n_in / (R)n_out;
        src = scale * ((R)d + (R)0.5) - (R)0.5;
        if (src < (R)0) src = (R)0;
    }
    i0 = (int)src;
    if (i0 > n_in - 1) i0 = n_in - 1;
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    l1 = src - (R)i0;
    l0 = (R)1 - l1;
}
