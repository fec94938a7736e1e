// kornia_amd - coordinate generation and sampler primitives shared by the warp kernels.
//
// Semantics being reproduced (reference files relative to /root/reference):
//   * coordinate generators: kornia/geometry/transform/imgwarp.py:157-170 (warp_perspective),
//     :271-281 (warp_affine), :1541-1546 + kornia/geometry/linalg.py:219-239 +
//     kornia/geometry/conversions.py:303-307 (homography_warp / transform_points);
//     kornia/geometry/grid.py:65-77 (create_meshgrid).
//   * sampler: F.grid_sample as specified by torch/include/ATen/native/GridSampler.h and
//     UpSample.h:400-423 (the reference calls it at imgwarp.py:174,290,316,320,1546).
// Every floating-point operation is written in the order the reference performs it; see
// oracle/ko_impl.h for the CPU restatement these functions are tested against bit for bit.
#pragma once

#include "km_common.h"

enum { KM_COORD_PERSPECTIVE = 0, KM_COORD_AFFINE = 1, KM_COORD_HOMOGRAPHY = 2, KM_COORD_GRID = 3 /* explicit (B_G,h,w,2) grid */ };
enum { KM_INTERP_NEAREST = 0, KM_INTERP_BILINEAR = 1, KM_INTERP_BICUBIC = 2 };
enum { KM_PAD_ZEROS = 0, KM_PAD_BORDER = 1, KM_PAD_REFLECTION = 2, KM_PAD_FILL = 3 };

// [host-testable begin: coords]  (tests/test_tile_box_spec.py compiles this span for the host with g++)
// Per-launch geometry shared by forward and backward.
template <typename R>
struct KmWarpGeom {
    int B, C, H, W, h, w, B_M;
    int coord_mode, norm_coords, interp, pad, align;
    // torch.linspace parameters for KM_COORD_AFFINE (imgwarp.py:271-276), evaluated on the host in R
    R lin_lo_x, lin_hi_x, lin_step_x, lin_lo_y, lin_hi_y, lin_step_y;
};

template <typename R>
struct KmCoord {
    R u, v;    // base coordinates
    R gx, gy;  // normalised sampling coordinates
    R den;     // perspective: denominator; homography: scale s
    R X, Y;    // homography: numerators
    bool live; // homography: |Z| > eps
};

// create_meshgrid(normalized_coordinates=True), grid.py:73-75: (i / (n-1) - 0.5) * 2
__device__ __forceinline__ float km_mesh_f32(int i, int n) { return (((float)i / (float)(n - 1)) - 0.5f) * 2.0f; }
template <typename R>
__device__ __forceinline__ R km_mesh(int i, int n) {
    return (((R)i / (R)(n - 1)) - (R)0.5) * (R)2;
}

// torch.linspace scalar formula (two-sided, fused multiply-add)
template <typename R>
__device__ __forceinline__ R km_linspace(R lo, R hi, R step, int n, int i) {
    if (n == 1) return lo;
    if (i < n / 2) return km_fma(step, (R)i, lo);
    return km_fma(-step, (R)(n - 1 - i), hi);
}

// base coordinate along x (column j) / y (row i)
template <typename R, int CM>
__device__ __forceinline__ R km_base_x(const KmWarpGeom<R>& g, int j) {
    if (CM == KM_COORD_GRID) return (R)0;  // coordinates come from memory
    if (CM == KM_COORD_PERSPECTIVE) return (R)km_mesh_f32(j, g.w);  // always computed in fp32, then cast
    if (CM == KM_COORD_AFFINE) return km_linspace<R>(g.lin_lo_x, g.lin_hi_x, g.lin_step_x, g.w, j);
    return g.norm_coords ? km_mesh<R>(j, g.w) : (R)j;
}
template <typename R, int CM>
__device__ __forceinline__ R km_base_y(const KmWarpGeom<R>& g, int i) {
    if (CM == KM_COORD_GRID) return (R)0;
    if (CM == KM_COORD_PERSPECTIVE) return (R)km_mesh_f32(i, g.h);
    if (CM == KM_COORD_AFFINE) return km_linspace<R>(g.lin_lo_y, g.lin_hi_y, g.lin_step_y, g.h, i);
    return g.norm_coords ? km_mesh<R>(i, g.h) : (R)i;
}

// host side: fill the per-launch geometry.  torch.linspace(lo, hi, n, dtype=R) of warp_affine's base grid
// (imgwarp.py:271-276): endpoints rounded to R, step = (hi - lo) / (n - 1) in R
template <typename R>
static inline void km_geom_init(KmWarpGeom<R>& g, int B, int C, int H, int W, int h, int w, int B_M, int coord_mode, int norm_coords,
                                int interp, int pad, int align) {
    g.B = B; g.C = C; g.H = H; g.W = W; g.h = h; g.w = w; g.B_M = B_M;
    g.coord_mode = coord_mode; g.norm_coords = norm_coords; g.interp = interp; g.pad = pad; g.align = align;
    if (align) {
        g.lin_lo_x = (R)-1.0; g.lin_hi_x = (R)1.0; g.lin_lo_y = (R)-1.0; g.lin_hi_y = (R)1.0;
    } else {
        g.lin_lo_x = (R)(-1.0 + 1.0 / w); g.lin_hi_x = (R)(1.0 - 1.0 / w);
        g.lin_lo_y = (R)(-1.0 + 1.0 / h); g.lin_hi_y = (R)(1.0 - 1.0 / h);
    }
    g.lin_step_x = w > 1 ? (g.lin_hi_x - g.lin_lo_x) / (R)(w - 1) : (R)0;
    g.lin_step_y = h > 1 ? (g.lin_hi_y - g.lin_lo_y) / (R)(h - 1) : (R)0;
}
// [host-testable end: coords]

template <typename R, int CM>
__device__ __forceinline__ void km_gen_coord(const R (&m)[9], R u, R v, KmCoord<R>& c) {
    c.u = u;
    c.v = v;
    if (CM == KM_COORD_GRID) {
        // (gx, gy) are loaded by the caller (km_grid_coord)
        c.den = (R)1;
    } else if (CM == KM_COORD_PERSPECTIVE) {
        // imgwarp.py:167-169: ((m20*u) + (m21*v)) + m22 ; ((m00*u) + (m01*v) + m02) / den
        const R den = (m[6] * u + m[7] * v) + m[8];
        c.den = den;
        c.gx = ((m[0] * u + m[1] * v) + m[2]) / den;
        c.gy = ((m[3] * u + m[4] * v) + m[5]) / den;
    } else if (CM == KM_COORD_AFFINE) {
        c.den = (R)1;
        c.gx = (m[0] * u + m[1] * v) + m[2];
        c.gy = (m[3] * u + m[4] * v) + m[5];
    } else {
        // bmm([u v 1], H^T) as the k-ordered fma chain of the BLAS behind torch.bmm, then
        // convert_points_from_homogeneous: s = |Z| > eps ? 1/(Z+eps) : 1
        const R X = km_fma(v, m[1], u * m[0]) + m[2];
        const R Y = km_fma(v, m[4], u * m[3]) + m[5];
        const R Z = km_fma(v, m[7], u * m[6]) + m[8];
        const R eps = (R)1e-8;
        c.live = km_fabs(Z) > eps;
        const R s = c.live ? (R)1 / (Z + eps) : (R)1;
        c.X = X;
        c.Y = Y;
        c.den = s;
        c.gx = s * X;
        c.gy = s * Y;
    }
}

// explicit-grid mode: the normalised sampling position of output pixel (i, j) of image b, stored as (x, y) pairs in
// the image dtype (F.grid_sample requires grid.dtype == input.dtype); one 2-element load
template <typename T, typename R>
__device__ __forceinline__ void km_grid_coord(const T* grid, const KmWarpGeom<R>& g, uint32_t b, int i, int j, KmCoord<R>& c) {
    const T* gp = grid + (((size_t)(g.B_M == 1 ? 0 : b) * g.h + i) * g.w + j) * 2;
    km_ld2(gp, c.gx, c.gy);
}

// ---- ATen GridSampler.h primitives ---------------------------------------------------------------
template <typename R>
__device__ __forceinline__ R km_unnormalize(R g, int size, int align, R& mult) {
    if (align) {
        mult = (R)(size - 1) / 2;
        return ((g + 1) / 2) * (R)(size - 1);
    }
    mult = (R)size / 2;
    return km_fma(g + 1, (R)size / 2, (R)-0.5);  // ((g+1)*size - 1)/2 as one fused op (see oracle)
}

// (a NaN position clips to 0 with a zero derivative, like -inf: ATen's CPU sampler clamps with max(x, 0) in the operand order that drops a NaN)
template <typename R>
__device__ __forceinline__ R km_clip(R x, int size, R& grad) {
    if (!(x > (R)0)) {
        grad = 0;
        return 0;
    }
    const R mx = (R)(size - 1);
    if (x >= mx) {
        grad = 0;
        return mx;
    }
    grad = 1;
    return x;
}

template <typename R>
__device__ __forceinline__ R km_reflect(R x, int twice_low, int twice_high, R& grad) {
    if (twice_low == twice_high) {
        grad = 0;
        return 0;
    }
    int sign;
    const R mn = (R)twice_low / 2;
    const R span = (R)(twice_high - twice_low) / 2;
    x = x - mn;
    if (x < (R)0) {
        sign = -1;
        x = -x;
    } else {
        sign = 1;
    }
    const R extra = km_fmod(x, span);
    // parity of the fold count in floating point: the count itself passes INT_MAX for a far-away position (an undefined float -> int conversion).
    // A NaN / inf position has a NaN remainder and comes out NaN, which the clip that follows every reflection brings to 0
    const R flips = km_floor(x / span);
    const bool even = km_floor(flips * (R)0.5) * (R)2 == flips;  // (exact: halving and doubling round nothing)
    if (even) {
        grad = (R)sign;
        return extra + mn;
    }
    grad = (R)(-sign);
    return span - extra + mn;
}

// pad: zeros(0)/fill(3) -> identity, border(1) -> clip, reflection(2) -> reflect + clip
template <typename R>
__device__ __forceinline__ R km_compute_coord(R x, int size, int pad, int align, R& grad) {
    grad = 1;
    if (pad == KM_PAD_BORDER) {
        x = km_clip(x, size, grad);
    } else if (pad == KM_PAD_REFLECTION) {
        R gr, gc;
        x = align ? km_reflect(x, 0, 2 * (size - 1), gr) : km_reflect(x, -1, 2 * size - 1, gr);
        x = km_clip(x, size, gc);
        grad = gr * gc;
    }
    return x;
}

template <typename R>
__device__ __forceinline__ void km_cubic_coeffs(R t, R (&c)[4]) {
    const R A = (R)-0.75;
    R x = t + (R)1.0;
    c[0] = ((A * x - 5 * A) * x + 8 * A) * x - 4 * A;
    x = t;
    c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    x = (R)1.0 - t;
    c[2] = ((A + 2) * x - (A + 3)) * x * x + 1;
    x = x + (R)1.0;
    c[3] = ((A * x - 5 * A) * x + 8 * A) * x - 4 * A;
}

template <typename R>
__device__ __forceinline__ void km_cubic_coeffs_grad(R t, R (&c)[4]) {
    const R A = (R)-0.75;
    R x = -1 - t;
    c[0] = (-3 * A * x - 10 * A) * x - 8 * A;
    x = -t;
    c[1] = (-3 * (A + 2) * x - 2 * (A + 3)) * x;
    x = 1 - t;
    c[2] = (3 * (A + 2) * x - 2 * (A + 3)) * x;
    x = 2 - t;
    c[3] = (3 * A * x - 10 * A) * x + 8 * A;
}

// integer tap for bicubic: the tap position itself goes through the padding transform
// (get_value_bounded / add_value_bounded).  Returns the linear index or -1.
template <typename R>
__device__ __forceinline__ int km_tap_index(R x, R y, int W, int H, int pad, int align) {
    R g;
    x = km_compute_coord(x, W, pad, align, g);
    y = km_compute_coord(y, H, pad, align, g);
    // bounds decided on the float (the taps are whole numbers): a NaN position is OUT of bounds - ATen's CPU kernel converts it to INT64_MIN -
    // where the device's own conversion gives 0, i.e. column 0 / row 0 of the image
    const bool inb = (x >= (R)0) && (x <= (R)(W - 1)) && (y >= (R)0) && (y <= (R)(H - 1));
    return inb ? (int)y * W + (int)x : -1;
}

// bilinear tap set for one output pixel
template <typename R>
struct KmBilin {
    int i00, i01, i10, i11;  // clamped linear indices (always valid addresses)
    R w00, w01, w10, w11;    // weights, zeroed for out-of-bounds taps in forward use
    bool b00, b01, b10, b11;
    R wx0, wx1, wy0, wy1;    // (x - x0), (x1 - x), (y - y0), (y1 - y)
};

template <typename R>
__device__ __forceinline__ void km_bilinear_setup(R x, R y, int W, int H, KmBilin<R>& t) {
    const R xf = km_floor(x), yf = km_floor(y);
    // bounds decided in floating point so that NaN / huge coordinates are simply out of bounds
    const bool bx0 = (xf >= (R)0) && (xf <= (R)(W - 1));
    const bool bx1 = (xf >= (R)-1) && (xf <= (R)(W - 2));
    const bool by0 = (yf >= (R)0) && (yf <= (R)(H - 1));
    const bool by1 = (yf >= (R)-1) && (yf <= (R)(H - 2));
    const R x1f = xf + 1, y1f = yf + 1;
    t.wx1 = x1f - x;
    t.wx0 = x - xf;
    t.wy1 = y1f - y;
    t.wy0 = y - yf;
    t.w00 = t.wx1 * t.wy1;
    t.w01 = t.wx0 * t.wy1;
    t.w10 = t.wx1 * t.wy0;
    t.w11 = t.wx0 * t.wy0;
    const int x0 = bx0 ? (int)xf : 0, x1 = bx1 ? (int)x1f : 0;
    const int y0 = by0 ? (int)yf : 0, y1 = by1 ? (int)y1f : 0;
    t.b00 = bx0 && by0;
    t.b01 = bx1 && by0;
    t.b10 = bx0 && by1;
    t.b11 = bx1 && by1;
    t.i00 = y0 * W + x0;
    t.i01 = y0 * W + x1;
    t.i10 = y1 * W + x0;
    t.i11 = y1 * W + x1;
}

// ---- out-of-bounds taps: ZEROS THAT ARE STILL MULTIPLIED ---------------------------------------------------------------------------------
// ATen's CPU sampler - the reference - gathers a tap outside the image as 0 (mask_gather) and still multiplies it by its weight
// (GridSamplerKernel.cpp, ApplyGridSample<..., Bilinear, ...>::forward / backward).  For the finite weights of a finite position that leaves
// the sum unchanged - fma(0, w, acc) == acc - so nothing moves for ordinary inputs; for a NaN / inf position (a singular or NaN-carrying
// matrix, a projective denominator of exactly zero: every weight of the pixel is NaN) it is NaN, which is what the reference returns there:
// NaN forward, NaN into the grid - hence the matrix - gradient, and nothing scattered into the image gradient (the scatter IS masked).
// Every bilinear path that can meet such a position (the per-tap predicated paths: the fast paths' inside tests fail on NaN) goes through
// these; tests/golden/nonfinite_coords.npz is the reference's result.
template <typename R>
__device__ __forceinline__ R km_bilinear_masked(const KmBilin<R>& t, R v00, R v01, R v10, R v11) {
    R acc = km_fma(t.b00 ? v00 : (R)0, t.w00, (R)0);  // fma chain in nw, ne, sw, se order from 0
    acc = km_fma(t.b01 ? v01 : (R)0, t.w01, acc);
    acc = km_fma(t.b10 ? v10 : (R)0, t.w10, acc);
    return km_fma(t.b11 ? v11 : (R)0, t.w11, acc);
}
// grid_sample(ones) of _fill_and_warp (imgwarp.py:316): the same chain on an image of ones
template <typename R>
__device__ __forceinline__ R km_bilinear_ones(const KmBilin<R>& t) {
    return km_bilinear_masked<R>(t, (R)1, (R)1, (R)1, (R)1);
}
// d out / d (x, y) of one channel, times its upstream gradient, added to (gix, giy): taps outside the image are zeros that are still
// multiplied (ApplyGridSample<..., Bilinear, ...>::backward forms ((ne - nw) * s + (se - sw) * n) * gOut from masked gathers)
template <typename R>
__device__ __forceinline__ void km_bilinear_grid_terms(const KmBilin<R>& t, R s00, R s01, R s10, R s11, R go, R& gix, R& giy) {
    s00 = t.b00 ? s00 : (R)0; s01 = t.b01 ? s01 : (R)0; s10 = t.b10 ? s10 : (R)0; s11 = t.b11 ? s11 : (R)0;
    gix -= s00 * t.wy1 * go; giy -= s00 * t.wx1 * go;
    gix += s01 * t.wy1 * go; giy -= s01 * t.wx0 * go;
    gix -= s10 * t.wy0 * go; giy += s10 * t.wx1 * go;
    gix += s11 * t.wy0 * go; giy += s11 * t.wx0 * go;
}
template <typename R>
__device__ __forceinline__ bool km_finite(R v) { return (v - v) == (R)0; }  // (inf - inf and NaN - NaN are NaN; no fast-math in this build)

// matrix-gradient contribution of one output pixel: with r = (u, v, 1) the pixel adds
//   d/dm0k += ax r_k ,  d/dm1k += ay r_k ,  d/dm2k += az r_k
// for the (ax, ay, az) returned here (gix, giy = d loss / d (x, y) already scaled to normalised coordinates)
template <int CM>
__device__ __forceinline__ void km_gm_terms(const KmCoord<float>& cd, float gix, float giy, float& ax, float& ay, float& az) {
    typedef float R;
    if (CM == KM_COORD_PERSPECTIVE) {
        const R inv = __frcp_rn(cd.den);
        ax = gix * inv;
        ay = giy * inv;
        az = -km_fma(gix, cd.gx, giy * cd.gy) * inv;
    } else if (CM == KM_COORD_AFFINE) {
        ax = gix;
        ay = giy;
        az = 0;
    } else {
        const R s = cd.den;
        ax = gix * s;
        ay = giy * s;
        az = cd.live ? -km_fma(gix, cd.X, giy * cd.Y) * s * s : (R)0;
    }
}
