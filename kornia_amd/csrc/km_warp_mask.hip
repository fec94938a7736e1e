// kornia_amd - the augmentation container's mask warp: an image and its label mask under ONE geometric draw.
//
// kornia.augmentation.AugmentationSequential(..., data_keys=["input", "mask"]) (kornia/augmentation/container/augment.py:596-618,
// _2d/geometric/base.py:87-130) treats a mask element by element as
//   1. mask.to(image dtype)                                    (_preproc_mask)
//   2. the module's own warp with mode = 'nearest', the module's padding mode, align_corners and fill_value
//   3. .to(mask dtype)                                         (_postproc_mask: float -> integer truncates toward zero, bool is != 0)
// and the whole tensor takes the round trip, so a sample whose probability draw failed comes back as mask -> image dtype -> mask too.
// Here that is one kernel reading and writing the mask in its own dtype: the round trip happens in registers, and the sampling is the
// generic forward's nearest branch (km_warp.hip: same coordinate functions, same order of operations) - bit-identical to
//   warp_*(mask.to(image dtype), M, mode="nearest", ...).to(mask dtype).
//
// Lane -> element map: a lane owns V = max(1, 4 / sizeof(mask element)) CONSECUTIVE elements of one plane (4 for bool / uint8, 2 for
// 16-bit, 1 for 32 / 64-bit), so the 64 lanes of a wave cover 64 V consecutive elements: 256 contiguous bytes of stores per wave instruction
// (512 for int64).  When the plane size is a multiple of V the V results are packed into one 4-byte store per lane; otherwise each
// element is stored on its own (same bytes, V narrower instructions).  The taps are single-element gathers.
//
// km_warp2d_pair_fwd takes the image and the first mask either in ONE launch (km_warp_pair_kernel below: the coordinate computed once per
// pixel for both) or in TWO - the image through km_warp2d_fwd_masked, its kernels untouched, then this kernel on the same matrix and
// switch; the image is bit-identical to km_warp2d_fwd_masked either way.  Which one runs: KM_PAIR_FUSED_DEFAULT (km_common.h).
#include "km_warp_args.h"
#include "km_warp_host.h"
#include "km_mask.h"

struct KmMaskArgs {
    const void* src;         // (B,Cm,H,W) mask dtype
    void* dst;               // (B,Cm,H,W) mask dtype
    const float* mat;        // (B,9) normalised dst->src, fp32
    const uint8_t* apply;    // (B) nullable: 0 = the sample takes the dtype round trip only
    const float* fill;       // (Cm) fp32, pad == fill only
    KmWarpGeom<float> g;     // C = Cm, h = H, w = W, B_M = B
    uint32_t groups;         // V-element groups per plane
    uint32_t blocks_per_plane;
    const void* isrc;        // fused pair only: (B,C,H,W) image
    void* idst;
    const float* ifill;      // fused pair only: (C) fp32, pad == fill only
    int C;                   // fused pair only: image channels
};

template <int MD, int DT, int CM, int V>
__global__ __launch_bounds__(256) void km_warp_mask_kernel(const KmMaskArgs a) {
    typedef typename KmMaskStore<MD>::T M;
    const KmWarpGeom<float>& g = a.g;
    const uint32_t p = blockIdx.x / a.blocks_per_plane;  // plane = b * Cm + c (planes folded into grid.x: no limit on B * Cm below 2^31 blocks)
    const uint32_t grp = (blockIdx.x - p * a.blocks_per_plane) * 256u + threadIdx.x;
    if (grp >= a.groups) return;
    const uint32_t b = p / (uint32_t)g.C, c = p % (uint32_t)g.C;
    const size_t plane = (size_t)g.H * g.W;
    const M* __restrict__ sp = (const M*)a.src + (size_t)p * plane;
    M* __restrict__ dp = (M*)a.dst + (size_t)p * plane;
    const bool warp = !a.apply || a.apply[b];
    float m[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = warp ? a.mat[(size_t)b * 9 + k] : 0.0f;
    const int spad = (g.pad == KM_PAD_FILL) ? KM_PAD_ZEROS : g.pad;
    const float fill = (g.pad == KM_PAD_FILL) ? a.fill[c] : 0.0f;
    M res[V];
    const size_t e0 = (size_t)grp * V;
    // (row, column) of the group's first element by one 32-bit division (the plane holds < 2^31 elements), then stepped along the row
    int i = (int)((uint32_t)e0 / (uint32_t)g.W), j = (int)((uint32_t)e0 - (uint32_t)i * (uint32_t)g.W);
#pragma unroll
    for (int k = 0; k < V; ++k, ++j) {
        const size_t e = e0 + k;
        if (e >= plane) break;
        if (j == g.W) {
            j = 0;
            ++i;
        }
        float acc;
        if (!warp) {
            acc = km_img_round<DT>(km_mask_ld<MD>(sp + e));
        } else {
            // the generic forward's nearest branch (km_warp.hip, km_warp_fwd_kernel), operand for operand
            KmCoord<float> cd;
            km_gen_coord<float, CM>(m, km_base_x<float, CM>(g, j), km_base_y<float, CM>(g, i), cd);
            float mx, my, gdx, gdy;
            float x = km_unnormalize(cd.gx, g.W, g.align, mx);
            float y = km_unnormalize(cd.gy, g.H, g.align, my);
            x = km_compute_coord(x, g.W, spad, g.align, gdx);
            y = km_compute_coord(y, g.H, spad, g.align, gdy);
            const float xr = km_rint(x), yr = km_rint(y);
            const bool inb = (xr >= 0.0f) && (xr <= (float)(g.W - 1)) && (yr >= 0.0f) && (yr <= (float)(g.H - 1));
            const int idx = inb ? (int)yr * g.W + (int)xr : 0;
            acc = inb ? km_img_round<DT>(km_mask_ld<MD>(sp + idx)) : 0.0f;
            if (g.pad == KM_PAD_FILL) acc = acc + (1.0f - (inb ? 1.0f : 0.0f)) * fill;
            acc = km_img_round<DT>(acc);  // (the warp's store in the image dtype)
        }
        res[k] = km_mask_cast<MD>(acc);
    }
    if (sizeof(M) * V == 4 && (plane % V) == 0 && ((uintptr_t)a.dst & 3) == 0 && e0 + V <= plane) {
        uint32_t word;
        __builtin_memcpy(&word, res, 4);
        *(uint32_t*)(dp + e0) = word;  // one 4-byte store per lane (4-byte aligned base, plane size a multiple of V: every group starts on a word)
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (e0 + k < plane) dp[e0 + k] = res[k];
    }
}

template <int MD, int DT, int CM>
static void km_warp_mask_launch(const KmMaskArgs& a0, hipStream_t s) {
    constexpr int V = sizeof(typename KmMaskStore<MD>::T) >= 4 ? 1 : 4 / (int)sizeof(typename KmMaskStore<MD>::T);
    KmMaskArgs a = a0;
    const size_t plane = (size_t)a.g.H * a.g.W;
    a.groups = (uint32_t)((plane + V - 1) / V);
    a.blocks_per_plane = (a.groups + 255u) / 256u;
    const uint64_t nb = (uint64_t)a.blocks_per_plane * (uint64_t)a.g.B * (uint64_t)a.g.C;  // (< 2^31: checked by the caller)
    hipLaunchKernelGGL((km_warp_mask_kernel<MD, DT, CM, V>), dim3((uint32_t)nb), dim3(256), 0, s, a);
}

// ------------------------------------------------------------------------------------------------
// The pair in ONE launch: a lane per output pixel computes the sampling coordinate once and uses it for the image (bilinear or nearest,
// any padding: the generic forward's arithmetic, which the specialised forwards reproduce bit for bit) and for every mask channel
// (nearest, as above).  Image stores: 64 consecutive pixels per wave instruction, as the generic forward; mask stores: 64 consecutive
// elements (64 B for 1-byte masks).  Bicubic images take the two-launch form.
template <int MD, int DT, int CM, int INTERP>
__global__ __launch_bounds__(256) void km_warp_pair_kernel(const KmMaskArgs a) {
    typedef typename KmMaskStore<MD>::T M;
    typedef typename KmImgT<DT>::T T;
    const KmWarpGeom<float>& g = a.g;
    const uint32_t b = blockIdx.x / a.blocks_per_plane;
    const uint32_t e = (blockIdx.x - b * a.blocks_per_plane) * 256u + threadIdx.x;
    const uint32_t plane = (uint32_t)g.H * (uint32_t)g.W;
    if (e >= plane) return;
    const int Cm = g.C, C = a.C;
    const T* __restrict__ isp = (const T*)a.isrc + (size_t)b * C * plane;
    T* __restrict__ idp = (T*)a.idst + (size_t)b * C * plane;
    const M* __restrict__ msp = (const M*)a.src + (size_t)b * Cm * plane;
    M* __restrict__ mdp = (M*)a.dst + (size_t)b * Cm * plane;
    if (a.apply && !a.apply[b]) {  // block-uniform: the sample is copied, its mask takes the dtype round trip
        for (int c = 0; c < C; ++c) idp[(size_t)c * plane + e] = isp[(size_t)c * plane + e];
        for (int c = 0; c < Cm; ++c) mdp[(size_t)c * plane + e] = km_mask_cast<MD>(km_img_round<DT>(km_mask_ld<MD>(msp + (size_t)c * plane + e)));
        return;
    }
    float m[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = a.mat[(size_t)b * 9 + k];
    const int i = (int)(e / (uint32_t)g.W), j = (int)(e - (uint32_t)i * (uint32_t)g.W);
    const int spad = (g.pad == KM_PAD_FILL) ? KM_PAD_ZEROS : g.pad;
    KmCoord<float> cd;
    km_gen_coord<float, CM>(m, km_base_x<float, CM>(g, j), km_base_y<float, CM>(g, i), cd);
    float mx, my, gdx, gdy;
    float x = km_unnormalize(cd.gx, g.W, g.align, mx);
    float y = km_unnormalize(cd.gy, g.H, g.align, my);
    x = km_compute_coord(x, g.W, spad, g.align, gdx);
    y = km_compute_coord(y, g.H, spad, g.align, gdy);
    const float xr = km_rint(x), yr = km_rint(y);
    const bool inb = (xr >= 0.0f) && (xr <= (float)(g.W - 1)) && (yr >= 0.0f) && (yr <= (float)(g.H - 1));
    const int idx = inb ? (int)yr * g.W + (int)xr : 0;
    if (INTERP == KM_INTERP_BILINEAR) {
        KmBilin<float> t;
        km_bilinear_setup(x, y, g.W, g.H, t);
        const float inv_mask = (g.pad == KM_PAD_FILL) ? 1.0f - km_bilinear_ones(t) : 0.0f;
        for (int c = 0; c < C; ++c) {
            const T* img = isp + (size_t)c * plane;
            // (km_bilinear_masked with every tap inside is the generic forward's unmasked fma chain, operand for operand)
            float acc = km_bilinear_masked(t, km_ld(img + t.i00), km_ld(img + t.i01), km_ld(img + t.i10), km_ld(img + t.i11));
            if (g.pad == KM_PAD_FILL) acc = acc + inv_mask * a.ifill[c];
            km_st(idp + (size_t)c * plane + e, acc);
        }
    } else {
        for (int c = 0; c < C; ++c) {
            float acc = inb ? km_ld(isp + (size_t)c * plane + idx) : 0.0f;
            if (g.pad == KM_PAD_FILL) acc = acc + (1.0f - (inb ? 1.0f : 0.0f)) * a.ifill[c];
            km_st(idp + (size_t)c * plane + e, acc);
        }
    }
    for (int c = 0; c < Cm; ++c) {
        float acc = inb ? km_img_round<DT>(km_mask_ld<MD>(msp + (size_t)c * plane + idx)) : 0.0f;
        if (g.pad == KM_PAD_FILL) acc = acc + (1.0f - (inb ? 1.0f : 0.0f)) * a.fill[c];
        mdp[(size_t)c * plane + e] = km_mask_cast<MD>(km_img_round<DT>(acc));
    }
}

template <int MD, int DT, int CM>
static void km_warp_pair_launch(const KmMaskArgs& a0, hipStream_t s) {
    KmMaskArgs a = a0;
    const uint32_t plane = (uint32_t)a.g.H * (uint32_t)a.g.W;
    a.blocks_per_plane = (plane + 255u) / 256u;
    const uint64_t nb = (uint64_t)a.blocks_per_plane * (uint64_t)a.g.B;
    if (a.g.interp == KM_INTERP_NEAREST) hipLaunchKernelGGL((km_warp_pair_kernel<MD, DT, CM, KM_INTERP_NEAREST>), dim3((uint32_t)nb), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((km_warp_pair_kernel<MD, DT, CM, KM_INTERP_BILINEAR>), dim3((uint32_t)nb), dim3(256), 0, s, a);
}

template <int MD, int DT>
static void km_warp_mask_dispatch_cm(const KmMaskArgs& a, int coord_mode, bool fused, hipStream_t s) {
    if (fused) {
        if (coord_mode == KM_COORD_AFFINE) km_warp_pair_launch<MD, DT, KM_COORD_AFFINE>(a, s);
        else km_warp_pair_launch<MD, DT, KM_COORD_PERSPECTIVE>(a, s);
    } else {
        if (coord_mode == KM_COORD_AFFINE) km_warp_mask_launch<MD, DT, KM_COORD_AFFINE>(a, s);
        else km_warp_mask_launch<MD, DT, KM_COORD_PERSPECTIVE>(a, s);
    }
}

template <int MD>
static void km_warp_mask_dispatch_dt(const KmMaskArgs& a, int dtype, int coord_mode, bool fused, hipStream_t s) {
    if (dtype == KM_F32) km_warp_mask_dispatch_cm<MD, KM_F32>(a, coord_mode, fused, s);
    else if (dtype == KM_BF16) km_warp_mask_dispatch_cm<MD, KM_BF16>(a, coord_mode, fused, s);
    else km_warp_mask_dispatch_cm<MD, KM_F16>(a, coord_mode, fused, s);
}

extern "C" {

// Image + one label mask under the same normalised matrix and per-sample switch (kornia/augmentation/container/augment.py:596-618 with
// _2d/geometric/base.py:87-130).  src / dst (B,C,H,W) image dtype - both null: the mask alone; mask_src / mask_dst (B,Cm,H,W) in mask_dtype
// (KM_MASK_*); mat (B,9) fp32 normalised dst->src (coord_mode KM_WARP_AFFINE or KM_WARP_PERSPECTIVE); apply (B) uint8 or null; fill (C) fp32,
// mask_fill (Cm) fp32 - read only when pad == KM_FILL; dtype: the IMAGE dtype (f32 / bf16 / f16), also when the image pointer is null.
int km_warp2d_pair_fwd(const void* src, void* dst, const void* mask_src, void* mask_dst, const void* mat, const void* apply, int B, int C, int Cm,
                       int H, int W, int coord_mode, int interp, int pad, int align, const void* fill, const void* mask_fill, int dtype,
                       int mask_dtype, void* stream) {
    KM_REQUIRE(mat && (Cm == 0 || (mask_src && mask_dst)), "km_warp2d_pair_fwd: null matrix or mask pointer");
    KM_REQUIRE((src == nullptr) == (dst == nullptr), "km_warp2d_pair_fwd: image src and dst go together");
    KM_REQUIRE(B >= 0 && C >= 0 && Cm >= 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), "km_warp2d_pair_fwd: bad shape B=%d C=%d Cm=%d H=%d W=%d",
               B, C, Cm, H, W);
    KM_REQUIRE((((int64_t)H * W + 255) / 256) * B * (Cm > 0 ? Cm : 1) < (1ll << 31), "km_warp2d_pair_fwd: launch grid too large (B=%d Cm=%d H=%d W=%d)", B, Cm, H, W);
    KM_REQUIRE(coord_mode == KM_COORD_AFFINE || coord_mode == KM_COORD_PERSPECTIVE, "km_warp2d_pair_fwd: coord_mode must be affine or perspective");
    KM_REQUIRE(interp >= 0 && interp <= 2 && pad >= 0 && pad <= 3, "km_warp2d_pair_fwd: bad interp %d / pad %d", interp, pad);
    KM_REQUIRE(pad != KM_PAD_FILL || ((Cm == 0 || mask_fill) && (fill || !src || C == 0)), "km_warp2d_pair_fwd: pad=fill needs fill values");
    KM_REQUIRE(dtype == KM_F32 || dtype == KM_BF16 || dtype == KM_F16, "km_warp2d_pair_fwd: image dtype must be f32 / bf16 / f16");
    KM_REQUIRE(mask_dtype >= KM_MASK_BOOL && mask_dtype <= KM_MASK_F16, "km_warp2d_pair_fwd: bad mask dtype %d", mask_dtype);
    if (B == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    // one launch for image + first mask (km_warp_pair_kernel) or two (the image's own forward, then km_warp_mask_kernel): km_config_set
    // ("pair_fused", 1 / 0 / 2 = by coordinate generator) or KM_PAIR_ALGO; the default KM_PAIR_FUSED_DEFAULT is what measured faster
    // (profiles/README.md, r07): affine images keep their specialised forward (the box kernel beats the lane-per-pixel pair kernel by more
    // than the second launch costs), perspective ones take the pair kernel
    const int pf = km_config().pair_fused;
    const bool fused = src && C > 0 && Cm > 0 && interp != KM_INTERP_BICUBIC && (pf == 1 || (pf == 2 && coord_mode == KM_COORD_PERSPECTIVE));
    // the image's warp: same size, one normalised matrix per sample
    KmWarpCall c;
    c.src = src; c.mat = mat; c.dst = dst; c.fill = fill; c.apply = apply;
    c.B = B; c.C = C; c.H = H; c.W = W; c.h = H; c.w = W; c.B_M = B;
    c.coord_mode = coord_mode; c.norm_coords = 1; c.interp = interp; c.pad = pad; c.align = align; c.dtype = dtype;
    c.stream = s;
    if (src && C > 0 && !fused) {
        const int rc = km_warp_fwd_call("km_warp2d_fwd_masked", c);
        if (rc) return rc;
    }
    if (Cm == 0) return 0;
    KmMaskArgs a;
    a.src = mask_src; a.dst = mask_dst; a.mat = (const float*)mat; a.apply = (const uint8_t*)apply; a.fill = (const float*)mask_fill;
    a.isrc = src; a.idst = dst; a.ifill = (const float*)fill; a.C = C;
    c.C = Cm;  // the mask's geometry: the image's with the mask's channel count
    km_geom_init(a.g, c);
    a.groups = 0;
    a.blocks_per_plane = 0;
    switch (mask_dtype) {
        case KM_MASK_BOOL: km_warp_mask_dispatch_dt<KM_MASK_BOOL>(a, dtype, coord_mode, fused, s); break;
        case KM_MASK_U8: km_warp_mask_dispatch_dt<KM_MASK_U8>(a, dtype, coord_mode, fused, s); break;
        case KM_MASK_I32: km_warp_mask_dispatch_dt<KM_MASK_I32>(a, dtype, coord_mode, fused, s); break;
        case KM_MASK_I64: km_warp_mask_dispatch_dt<KM_MASK_I64>(a, dtype, coord_mode, fused, s); break;
        case KM_MASK_F32: km_warp_mask_dispatch_dt<KM_MASK_F32>(a, dtype, coord_mode, fused, s); break;
        case KM_MASK_BF16: km_warp_mask_dispatch_dt<KM_MASK_BF16>(a, dtype, coord_mode, fused, s); break;
        default: km_warp_mask_dispatch_dt<KM_MASK_F16>(a, dtype, coord_mode, fused, s); break;
    }
    return km_check_launch("km_warp2d_pair_fwd");
}

}  // extern "C"
