// kornia_amd - batched crop -> resize (-> flip): kornia.geometry.transform.crop_by_indices (kornia/geometry/transform/crop2d.py:405-500)
// for a whole batch in ONE launch, with the random flips of the augmentation layer riding in it.
//
// The reference reads the boxes back to the host (.tolist()) and loops over the batch in Python: per sample a slice and, when the slice is
// not of the output size, F.interpolate (shape_compensation "resize") or F.pad ("pad").  Here every sample's integer window comes from its
// float32 corners src (B,4,2) with the reference's index rule - x1 = (long)src[b,0,0], x2 = (long)src[b,1,0] + 1, y1 = (long)src[b,0,1],
// y2 = (long)src[b,3,1] + 1 - and is clamped to the image as Python slicing clamps it (negative indices count from the end, an overhang is cut
// off), so no box can make the kernel read outside the image.  Per sample:
//   * window == (oh, ow): a copy (the bits of every pixel, NaN and inf included);
//   * "resize", bilinear: ATen's CPU upsample_bilinear2d on the window (kmp_axis, the arithmetic of km_resize_bilinear_kernel);
//   * "resize", nearest: ATen's CPU nearest_idx (out == in: identity, out == 2 in: i >> 1, else min((long)floorf(i * (float)in / out), in - 1));
//   * "pad": the window at the top-left corner, zeros beyond it, cut where it is larger - except when every box of the batch is the same, where
//     the reference resizes whatever shape_compensation says (it takes the batch-wide slice + resize path first);
//   * an empty window (a box outside the image): zeros.
// Flips: sample b is mirrored in x when bit 0 of flip_all is set or flip_x[b] > 0.5, in y when bit 1 is set or flip_y[b] > 0.5 (flip_x /
// flip_y: the flip modules' batch_prob draws as they are, thresholded here as base.py:380 does) - output pixel (i, j) is written at the
// mirrored place, so the result is torch.flip of the unflipped one bit for bit.  A standalone flip is src == null (the window is the whole image) with (oh, ow) = (H, W).
// Masks (label masks of the container, augment.py:596-618) are always sampled nearest and take the round trip through the image dtype
// (km_mask.h), as km_warp2d_pair_fwd does; the first mask rides in the image's launch.
//
// Shape: grid.y = sample (wave-uniform window, flags and scales: scalar loads), grid.x walks (output row, group of 4 output columns) of the
// sample; a lane computes the source rows / columns and weights of its 4 pixels once and reuses them for every image and mask channel, and
// stores the 4 values as one vector store when the output rows allow it (ow % 4 == 0, aligned base).  The reads are gathers from the window
// rows; the window rows a wave touches are contiguous runs, served by L1 / L2.
#include "km_mask.h"
#include "km_resize_axis.h"
#include "km_sampler.h"

enum { KM_CROP_RESIZE = 0, KM_CROP_PAD = 1 };
enum { KM_CROP_NO_MASK = 7 };

struct KmCropArgs {
    const void* x;          // (B,C,H,W) image dtype, null when C == 0
    void* y;                // (B,C,oh,ow)
    const void* m;          // (B,Cm,H,W) mask dtype, null when Cm == 0
    void* my;               // (B,Cm,oh,ow)
    const float* src;       // (B,4,2) corners, null: the whole image
    const float* flip_x;    // (B) mirror x where > 0.5, nullable
    const float* flip_y;    // (B) mirror y where > 0.5, nullable
    int flip_all, B, C, Cm, H, W, oh, ow, interp, comp, align;
    int b0;                 // first sample of this launch (grid.y is limited)
    uint32_t groups;        // groups of 4 output columns per row
};

// torch's float -> int64 cast of a box coordinate, saturated (a NaN or an out-of-range value is undefined in C++)
__device__ __forceinline__ long long km_box_index(float v) {
    if (!(v == v)) return 0;
    v = fminf(fmaxf(v, -1.0e15f), 1.0e15f);
    return (long long)v;
}

// Python's clamp of a slice [s, t) over n elements: start and length
__device__ __forceinline__ void km_slice(long long s, long long t, int n, int& start, int& len) {
    s = s < 0 ? (s + n < 0 ? 0 : s + n) : (s > n ? n : s);
    t = t < 0 ? (t + n < 0 ? 0 : t + n) : (t > n ? n : t);
    start = (int)s;
    len = t > s ? (int)(t - s) : 0;
}

__device__ __forceinline__ void km_box_raw(const float* src, int b, long long (&r)[4]) {
    const float* p = src + (size_t)b * 8;
    r[0] = km_box_index(p[0]);
    r[1] = km_box_index(p[2]) + 1;
    r[2] = km_box_index(p[1]);
    r[3] = km_box_index(p[7]) + 1;
}

// ATen's nearest_idx (UpSample.h) for the scale computed from the sizes
__device__ __forceinline__ int km_nearest_idx(int i, int n_in, int n_out) {
    if (n_out == n_in) return i;
    if (n_out == 2 * n_in) return i >> 1;
    const float scale = (float)n_in / (float)n_out;
    const long long v = (long long)floorf((float)i * scale);
    return (int)(v < n_in - 1 ? v : n_in - 1);
}

template <typename E>
struct alignas(4 * sizeof(E) < 16 ? 4 * sizeof(E) : 16) KmVec4 {
    E v[4];
};

template <typename E, bool VEC>
__device__ __forceinline__ void km_store4(E* p, const E (&v)[4], int n) {
    if (VEC && n == 4) {
        KmVec4<E> w;
#pragma unroll
        for (int k = 0; k < 4; ++k) w.v[k] = v[k];
        *(KmVec4<E>*)p = w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) p[k] = v[k];
    }
}

// float -> the storage type, in registers (km_st's conversions)
__device__ __forceinline__ void km_to(float& d, float v) { d = v; }
__device__ __forceinline__ void km_to(km_bf16& d, float v) { d.bits = km_f32_to_bf16_bits(v); }
__device__ __forceinline__ void km_to(km_f16& d, float v) {
    KM_OPAQUE(v);
    d = (km_f16)v;
}

enum { KMC_COPY = 0, KMC_BILINEAR = 1, KMC_NEAREST = 2, KMC_ZERO = 3 };

template <int DT, int MD, bool VEC>
__global__ __launch_bounds__(256) void km_crop_resize_kernel(const KmCropArgs a) {
    typedef typename KmImgT<DT>::T T;
    const int b = (int)blockIdx.y + a.b0;
    const int H = a.H, W = a.W, oh = a.oh, ow = a.ow;
    // the sample's window and arithmetic (wave-uniform)
    int wx, ww, wy, wh;
    int mode;
    if (a.src) {
        long long r[4];
        km_box_raw(a.src, b, r);
        km_slice(r[0], r[1], W, wx, ww);
        km_slice(r[2], r[3], H, wy, wh);
        bool resize = !(wh == oh && ww == ow);
        if (resize && a.comp == KM_CROP_PAD) {
            // the reference's batch-wide path: every box the same -> resize, whatever the compensation
            for (int k = 0; k < a.B && resize; ++k) {
                long long q[4];
                km_box_raw(a.src, k, q);
                resize = q[0] == r[0] && q[1] == r[1] && q[2] == r[2] && q[3] == r[3];
            }
        }
        mode = !resize ? KMC_COPY : (wh == 0 || ww == 0) ? KMC_ZERO : (a.interp == KM_INTERP_NEAREST ? KMC_NEAREST : KMC_BILINEAR);
    } else {
        wx = 0; wy = 0; ww = W; wh = H;
        mode = KMC_COPY;  // (the caller checks (oh, ow) == (H, W))
    }
    const int fl = a.flip_all | ((a.flip_x && a.flip_x[b] > 0.5f) ? 1 : 0) | ((a.flip_y && a.flip_y[b] > 0.5f) ? 2 : 0);
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= (uint32_t)oh * a.groups) return;
    const int di = (int)(e / a.groups);
    const int dj0 = (int)(e - (uint32_t)di * a.groups) * 4;
    const int n = ow - dj0 < 4 ? ow - dj0 : 4;
    const int i = (fl & 2) ? oh - 1 - di : di;  // the unflipped output row this destination row holds

    // rows: bilinear (y0, y1, h0, h1); ny the copied / nearest row (-1: outside the window -> zero) - also the masks' row in bilinear mode
    int y0 = 0, y1 = 0, ny = -1;
    float h0 = 0.0f, h1 = 0.0f;
    if (mode == KMC_BILINEAR) kmp_axis<float>(i, wh, oh, a.align, y0, y1, h0, h1);
    if (mode == KMC_COPY) ny = i < wh ? i : -1;
    else if (mode != KMC_ZERO) ny = km_nearest_idx(i, wh, oh);
    int x0[4], x1[4], nx[4];
    float w0[4], w1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int dj = dj0 + (k < n ? k : 0);
        const int j = (fl & 1) ? ow - 1 - dj : dj;
        x0[k] = x1[k] = 0;
        w0[k] = w1[k] = 0.0f;
        if (mode == KMC_BILINEAR) kmp_axis<float>(j, ww, ow, a.align, x0[k], x1[k], w0[k], w1[k]);
        if (mode == KMC_COPY) nx[k] = j < ww ? j : -1;
        else if (mode == KMC_ZERO) nx[k] = -1;
        else nx[k] = km_nearest_idx(j, ww, ow);
    }
    const size_t plane = (size_t)H * W, oplane = (size_t)oh * ow;
    const size_t orow = (size_t)di * ow + dj0;
    const size_t base0 = (size_t)wy * W + wx;  // the window's top-left pixel

    if (a.C > 0) {
        const T* xs = (const T*)a.x + (size_t)b * a.C * plane + base0;
        T* ys = (T*)a.y + (size_t)b * a.C * oplane + orow;
        T zero;
        __builtin_memset(&zero, 0, sizeof(T));
        for (int c = 0; c < a.C; ++c) {
            const T* p = xs + (size_t)c * plane;
            T res[4];
            if (mode == KMC_BILINEAR) {
                const T* r0 = p + (size_t)y0 * W;
                const T* r1 = p + (size_t)y1 * W;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float v00 = km_ld(r0 + x0[k]), v01 = km_ld(r0 + x1[k]), v10 = km_ld(r1 + x0[k]), v11 = km_ld(r1 + x1[k]);
                    const float top = w0[k] * v00 + w1[k] * v01;
                    const float bot = w0[k] * v10 + w1[k] * v11;
                    km_to(res[k], h0 * top + h1 * bot);
                }
            } else {
                // copy / pad / nearest / empty: the stored element itself (its bits), or zero outside the window
#pragma unroll
                for (int k = 0; k < 4; ++k) res[k] = (ny >= 0 && nx[k] >= 0) ? p[(size_t)ny * W + nx[k]] : zero;
            }
            km_store4<T, VEC>(ys + (size_t)c * oplane, res, n);
        }
    }
    if constexpr (MD != KM_CROP_NO_MASK) {
        typedef typename KmMaskStore<MD>::T M;
        // masks: nearest whatever the image's interpolation (the container's mask flags), through the image dtype and back
        const M* ms = (const M*)a.m + (size_t)b * a.Cm * plane + base0;
        M* my = (M*)a.my + (size_t)b * a.Cm * oplane + orow;
        for (int c = 0; c < a.Cm; ++c) {
            const M* p = ms + (size_t)c * plane;
            M res[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float v = (ny >= 0 && nx[k] >= 0) ? km_img_round<DT>(km_mask_ld<MD>(p + (size_t)ny * W + nx[k])) : 0.0f;
                res[k] = km_mask_cast<MD>(v);
            }
            km_store4<M, VEC>(my + (size_t)c * oplane, res, n);
        }
    }
}

template <int DT, int MD>
static void km_crop_launch(KmCropArgs a, bool vec, hipStream_t s) {
    const uint64_t items = (uint64_t)a.oh * a.groups;
    const uint32_t gx = (uint32_t)((items + 255) / 256);
    for (int b0 = 0; b0 < a.B; b0 += 65535) {
        a.b0 = b0;
        const int nb = a.B - b0 < 65535 ? a.B - b0 : 65535;
        if (vec) hipLaunchKernelGGL((km_crop_resize_kernel<DT, MD, true>), dim3(gx, (uint32_t)nb), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((km_crop_resize_kernel<DT, MD, false>), dim3(gx, (uint32_t)nb), dim3(256), 0, s, a);
    }
}

template <int DT>
static void km_crop_dispatch_mask(const KmCropArgs& a, int mask_dtype, bool vec, hipStream_t s) {
    if (a.Cm == 0) return km_crop_launch<DT, KM_CROP_NO_MASK>(a, vec, s);
    switch (mask_dtype) {
        case KM_MASK_BOOL: return km_crop_launch<DT, KM_MASK_BOOL>(a, vec, s);
        case KM_MASK_U8: return km_crop_launch<DT, KM_MASK_U8>(a, vec, s);
        case KM_MASK_I32: return km_crop_launch<DT, KM_MASK_I32>(a, vec, s);
        case KM_MASK_I64: return km_crop_launch<DT, KM_MASK_I64>(a, vec, s);
        case KM_MASK_F32: return km_crop_launch<DT, KM_MASK_F32>(a, vec, s);
        case KM_MASK_BF16: return km_crop_launch<DT, KM_MASK_BF16>(a, vec, s);
        default: return km_crop_launch<DT, KM_MASK_F16>(a, vec, s);
    }
}

static size_t km_mask_elem_bytes(int md) {
    switch (md) {
        case KM_MASK_I32: case KM_MASK_F32: return 4;
        case KM_MASK_I64: return 8;
        case KM_MASK_BF16: case KM_MASK_F16: return 2;
        default: return 1;
    }
}

extern "C" {

// Batched crop -> resize (-> flip) of an image and its first label mask (include/kornia_amd.h).  x / out (B,C,H,W) -> (B,C,oh,ow) in dtype
// (f32 / bf16 / f16), both null when C == 0 (the mask alone; dtype still names the image dtype of its round trip); mask / mask_out
// (B,Cm,H,W) -> (B,Cm,oh,ow) in mask_dtype (KM_MASK_*), both null when Cm == 0; src (B,4,2) fp32 corners or null (the whole image, which
// needs (oh, ow) == (H, W)); flip_x / flip_y (B) fp32 or null: mirror where > 0.5, flip_all: bit 0 / 1 mirror every sample in x / y; interp KM_INTERP_BILINEAR / _NEAREST;
// compensation 0 = resize, 1 = pad; align: align_corners of the bilinear resize.
int km_crop_resize_fwd(const void* x, void* out, const void* mask, void* mask_out, const void* src, const void* flip_x, const void* flip_y, int flip_all, int B, int C,
                       int Cm, int H, int W, int oh, int ow, int interp, int compensation, int align, int dtype, int mask_dtype, void* stream) {
    KM_REQUIRE((x == nullptr) == (out == nullptr) && (C == 0 || x), "km_crop_resize_fwd: image pointers and C disagree (C=%d)", C);
    KM_REQUIRE((mask == nullptr) == (mask_out == nullptr) && (Cm == 0 || mask), "km_crop_resize_fwd: mask pointers and Cm disagree (Cm=%d)", Cm);
    KM_REQUIRE(B >= 0 && C >= 0 && Cm >= 0 && H > 0 && W > 0 && oh > 0 && ow > 0 && (int64_t)H * W < (1ll << 31) && (int64_t)oh * ow < (1ll << 31),
               "km_crop_resize_fwd: bad shape B=%d C=%d Cm=%d H=%d W=%d oh=%d ow=%d", B, C, Cm, H, W, oh, ow);
    KM_REQUIRE(src || (oh == H && ow == W), "km_crop_resize_fwd: without boxes the output must be the image's size");
    KM_REQUIRE(interp == KM_INTERP_BILINEAR || interp == KM_INTERP_NEAREST, "km_crop_resize_fwd: interp must be bilinear or nearest, got %d", interp);
    KM_REQUIRE(compensation == KM_CROP_RESIZE || compensation == KM_CROP_PAD, "km_crop_resize_fwd: bad compensation %d", compensation);
    KM_REQUIRE(flip_all >= 0 && flip_all <= 3, "km_crop_resize_fwd: flip_all must be 0..3, got %d", flip_all);
    KM_REQUIRE(dtype == KM_F32 || dtype == KM_BF16 || dtype == KM_F16, "km_crop_resize_fwd: image dtype must be f32 / bf16 / f16");
    KM_REQUIRE(Cm == 0 || (mask_dtype >= KM_MASK_BOOL && mask_dtype <= KM_MASK_F16), "km_crop_resize_fwd: bad mask dtype %d", mask_dtype);
    if (B == 0 || (C == 0 && Cm == 0)) return 0;
    KmCropArgs a;
    a.x = x; a.y = out; a.m = mask; a.my = mask_out;
    a.src = (const float*)src; a.flip_x = (const float*)flip_x; a.flip_y = (const float*)flip_y;
    a.flip_all = flip_all; a.B = B; a.C = C; a.Cm = Cm; a.H = H; a.W = W; a.oh = oh; a.ow = ow;
    a.interp = interp; a.comp = compensation; a.align = align ? 1 : 0; a.b0 = 0;
    a.groups = (uint32_t)((ow + 3) / 4);
    // one vector store per lane and channel when every group of 4 output columns starts on a multiple of 4 elements of an aligned base
    const size_t isz = dtype == KM_F32 ? 4 : 2;
    const size_t msz = Cm ? km_mask_elem_bytes(mask_dtype) : 1;
    const size_t ia = isz * 4 < 16 ? isz * 4 : 16, ma = msz * 4 < 16 ? msz * 4 : 16;
    const bool vec = (ow % 4) == 0 && ((uintptr_t)out % ia) == 0 && ((uintptr_t)mask_out % ma) == 0;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == KM_F32) km_crop_dispatch_mask<KM_F32>(a, mask_dtype, vec, s);
    else if (dtype == KM_BF16) km_crop_dispatch_mask<KM_BF16>(a, mask_dtype, vec, s);
    else km_crop_dispatch_mask<KM_F16>(a, mask_dtype, vec, s);
    return km_check_launch("km_crop_resize_fwd");
}

}  // extern "C"
