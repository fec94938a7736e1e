// kornia_amd - LDS box forward warp for border / reflection / fill padding (bilinear, RGB / grey, fp32 compute) for gfx950.
// Reference: F.grid_sample(padding_mode="border" | "reflection") behind kornia/geometry/transform/imgwarp.py:157-174, :271-290, and
// _fill_and_warp :293-320 for "fill".
// Own translation unit: the zeros box kernel of km_warp.hip - the headline configuration - keeps its code, registers and timing.
//
// Without this file these paddings run km_warp_fwd_kernel: a lane per pixel, four predicated gathers per channel (8 - 16 bytes requested
// per channel for 4 bytes of output).  Here a 256-thread block owns a 64 x 32 region of the output and walks the zeros box kernel's ladder
// (every decision block-uniform):
//   1. KmpWide:   the region as ONE tile, box up to 80 x 40 source pixels;
//   2. KmpSquare: its two 32 x 32 halves one after the other, box up to 52 x 50 each - any rotation at scale ~1;
//   3. a half whose box still does not fit: the generic kernel's per-pixel gathers.
// What differs from the zeros geometry is WHICH source pixels a tile needs.  The padding rule acts on the continuous position before its
// taps are split (km_compute_coord), so LDS holds real image pixels at the positions AFTER the rule - not a virtually extended image - and
// the tile's unfolded interval of positions (its corners through the forward's own arithmetic, +- 1 px) is folded to image space per axis:
//   border:      both ends clipped into [0, size - 1];
//   reflection:  fold points k (size - 1) with align_corners, k size - 0.5 without (followed by the clip).  No fold point inside the
//                interval: the mirrored interval; one: from the fold to the farther reflected end; two or more: the whole axis (an image
//                smaller than the tile's span - it fits);
//   fill:        the zeros geometry unchanged (the rule is the identity; the fill colour is blended per pixel).
// One more row and column for the x0 + 1 / y0 + 1 taps.  A tap at index `size` (position exactly size - 1) is out of bounds and staged as
// zero like everything outside the image: ATen's rule is a zero that is still multiplied.  The estimate only has to be a superset: every
// pixel checks its transformed footprint against the staged box (kmf_in_box), and a wave with a footprint outside it - estimate off, NaN /
// inf position under fill, a denominator that changes sign - redoes its rows with the per-pixel code: the result never depends on the
// estimate.
// Arithmetic = the generic kernel's, operation for operation: positions from the lean front end (bit-identical to km_gen_coord,
// km_lean.h), km_unnormalize, km_compute_coord with the same `spad`, km_bilinear_setup's weights, the fma chain nw, ne, sw, se from 0,
// `acc + inv_mask * fill[c]`: bit-identical to km_warp_fwd_kernel for every input (tests/test_gpu_warp_box_pad.py compares the two).
#include "km_warp_args.h"
#include "km_warp_host.h"
#include "km_warp_stage.h"

struct KmpWide   { static constexpr int TW = 64, TH = 32, PITCH = 80, ROWS = 40; };
struct KmpSquare { static constexpr int TW = 32, TH = 32, PITCH = 52, ROWS = 50; };
#define KMP_LDS_FLOATS(NC) ((KmpWide::ROWS * KmpWide::PITCH > KmpSquare::ROWS * KmpSquare::PITCH ? KmpWide::ROWS * KmpWide::PITCH : KmpSquare::ROWS * KmpSquare::PITCH) * (NC))
#define KMP_WAVES_PER_EU 4  // what the LDS of a block allows (38 KB for RGB: 4 blocks of 4 waves per CU)
// floor(a / b) for b > 0
__device__ __forceinline__ int kmp_floor_div(int a, int b) {
    const int q = a / b;
    return (a - q * b < 0) ? q - 1 : q;
}

// One axis of the box: every position of the tile lies in [a, b) (whole numbers); [lo, hi] receives the taps - floor and floor + 1 of the
// positions after the padding rule - as image indices.  hi may be `size` (the zero a position of exactly size - 1 still multiplies).
template <int PAD>
__device__ __forceinline__ void kmp_fold_axis(int a, int b, int size, int align, int& lo, int& hi) {
    const int top = size - 1;
    if (PAD == KM_PAD_FILL) {  // identity: the zeros geometry (kmf_tile_setup)
        lo = a; hi = b;
    } else if (size == 1) {  // every position becomes 0
        lo = 0; hi = 1;
    } else if (PAD == KM_PAD_BORDER) {  // monotone: positions < b land below clip(b) unless that is the clipped end itself
        const int fb = min(max(b, 0), top);
        lo = min(max(a, 0), top);
        hi = (fb == top) ? size : max(fb, lo + 1);
    } else {
        // period k of the reflection holds the whole numbers [k span, (k + 1) span): rising from 0 for even k, falling from `top` for odd k
        const int span = align ? top : size;
        const int ka = kmp_floor_div(a, span), kb = kmp_floor_div(b, span);
        const int ra = a - ka * span, rb = b - kb * span;
        const int fa = (ka & 1) ? top - ra : ra, fb = (kb & 1) ? top - rb : rb;
        if (ka == kb) {  // no fold point inside: the mirrored interval
            if (ka & 1) { lo = fb; hi = fa + 1; }
            else { lo = fa; hi = (fb == top) ? size : max(fb, fa + 1); }
        } else if (kb == ka + 1) {  // one: from the fold (at `top` into an odd period, at 0 into an even one) to the farther end
            if (kb & 1) { lo = min(fa, fb); hi = size; }
            else { lo = 0; hi = max(fa, fb) + 1; }
        } else {  // several periods: the whole axis
            lo = 0; hi = size;
        }
    }
}

// wave 0: row table (m1 v, m4 v, m7 v) + division guard; wave 1: the folded source box.  Same s_info slots as kmf_tile_setup (kmf_read_box
// reads them).  Needs a barrier before kmf_read_box.
template <int CM, int PAD, typename SH>
__device__ __forceinline__ void kmp_tile_setup(const KmWarpGeom<float>& g, const float (&m)[9], int j0, int i0, float4* s_rv, int* s_info) {
    const int tid_ = km_tid_pinned(), lane = tid_ & 63, wave = tid_ >> 6;
    static_assert(SH::TH <= 64, "one wave fills the row table");
    const int j1 = min(j0 + SH::TW - 1, g.w - 1), i1 = min(i0 + SH::TH - 1, g.h - 1);
    if (wave == 0) {
        bool ok = true;
        if (lane < SH::TH) {
            const float v = km_base_y<float, CM>(g, i0 + lane);
            const KmlHalf h = kml_row_half<CM>(m, v);
            s_rv[lane] = make_float4(h.a, h.b, h.c, 0.f);
            ok = kml_row_guard<CM>(g, m, v);
        }
        const bool all_ok = __all(ok);
        if (lane == 0) s_info[0] = all_ok ? 1 : 0;
    } else if (wave == 1) {
        // lanes 0..3 take one corner each (plain IEEE divisions: any operands); the position BEFORE the padding rule
        const int jc = (lane & 1) ? j1 : j0, ic = (lane & 2) ? i1 : i0;
        const KmlHalf cu = kml_col_half<CM>(m, km_base_x<float, CM>(g, jc));
        const KmlHalf rv = kml_row_half<CM>(m, km_base_y<float, CM>(g, ic));
        KmlPos p;
        kml_position<CM, false>(m, cu, rv, p);
        float mult;
        const float x = km_unnormalize(p.gx, g.W, g.align, mult), y = km_unnormalize(p.gy, g.H, g.align, mult);
        const float dsel = (CM == KM_COORD_AFFINE) ? 1.0f : p.den;
        float xmin = x, xmax = x, ymin = y, ymax = y, dmin = dsel, dmax = dsel;
#pragma unroll
        for (int off = 1; off <= 2; off <<= 1) {
            xmin = fminf(xmin, __shfl_down(xmin, off, 64)); xmax = fmaxf(xmax, __shfl_down(xmax, off, 64));
            ymin = fminf(ymin, __shfl_down(ymin, off, 64)); ymax = fmaxf(ymax, __shfl_down(ymax, off, 64));
            dmin = fminf(dmin, __shfl_down(dmin, off, 64)); dmax = fmaxf(dmax, __shfl_down(dmax, off, 64));
        }
        const bool finite4 = __all((lane > 3) || ((x == x) && (y == y) && (km_fabs(x) < 1.0e8f) && (km_fabs(y) < 1.0e8f) && (dsel == dsel)));
        if (lane == 0) {
            int staged = 0, xs = 0, ys = 0, nch = 0, nrows = 0;
            if (finite4 && ((dmin > 0.f) || (dmax < 0.f))) {  // (else: nothing to estimate from - the per-pixel code)
                // positions in [floor(min) - 1, floor(max) + 2): one pixel on each side for the rounding of positions inside the quad
                // relative to its corners (<< 1 px) - checked per pixel anyway
                int lox, hix, loy, hiy;
                kmp_fold_axis<PAD>((int)km_floor(xmin) - 1, (int)km_floor(xmax) + 2, g.W, g.align, lox, hix);
                kmp_fold_axis<PAD>((int)km_floor(ymin) - 1, (int)km_floor(ymax) + 2, g.H, g.align, loy, hiy);
                xs = lox & ~3;  // 16-byte aligned start (two's complement: rounds toward -inf)
                ys = loy;
                const int wcols = hix - xs + 1;
                nrows = hiy - loy + 1;
                nch = (wcols + 3) >> 2;
                staged = (wcols <= SH::PITCH && nrows <= SH::ROWS) ? 1 : 0;
            }
            s_info[1] = staged;
            s_info[2] = xs;
            s_info[3] = ys;
            s_info[4] = nch;
            s_info[5] = nrows;
        }
    }
}

// this thread's position in output row `li` of the tile, after the padding rule: what km_warp_fwd_kernel computes for the pixel
template <int CM>
__device__ __forceinline__ void kmp_position(const KmWarpGeom<float>& g, const float (&m)[9], const KmlHalf& cu, const float4* s_rv, int li, bool fast, int spad,
                                             float& x, float& y) {
    const float4 rv4 = s_rv[li];
    KmlHalf rv;
    rv.a = rv4.x; rv.b = rv4.y; rv.c = rv4.z;
    KmlPos p;
    if (fast) kml_position<CM, true>(m, cu, rv, p);
    else kml_position<CM, false>(m, cu, rv, p);
    float mult, gd;
    x = km_compute_coord(km_unnormalize(p.gx, g.W, g.align, mult), g.W, spad, g.align, gd);
    y = km_compute_coord(km_unnormalize(p.gy, g.H, g.align, mult), g.H, spad, g.align, gd);
}

// RPT consecutive rows of a thread by the generic kernel's per-pixel gathers: ladder step 3, and what a wave with a footprint outside its
// box falls back to.  Deliberately small - the registers of the kernel are the maximum over its paths.
template <typename T, int CM, int NC, int PAD, int RPT>
__device__ __forceinline__ void kmp_pixel_rows(const KmWarpArgs<T>& a, const float (&m)[9], const float4* s_rv, bool fast, uint32_t b, int j, int li_base, int i_base) {
    const KmWarpGeom<float>& g = a.g;
    const int W = g.W, H = g.H;
    const int spad = (PAD == KM_PAD_FILL) ? KM_PAD_ZEROS : PAD;
    const size_t src_plane = (size_t)H * W, dst_plane = (size_t)g.h * g.w;
    const T* __restrict__ src_b = a.src + (size_t)b * NC * src_plane;
    T* __restrict__ dst_b = a.dst + (size_t)b * NC * dst_plane;
    const KmlHalf cu = kml_col_half<CM>(m, km_base_x<float, CM>(g, j));
#pragma unroll 1
    for (int r = 0; r < RPT; ++r) {
        if (i_base + r >= g.h) break;
        float x, y;
        kmp_position<CM>(g, m, cu, s_rv, li_base + r, fast, spad, x, y);
        KmBilin<float> t;
        km_bilinear_setup(x, y, W, H, t);
        float inv_mask = 0.f;
        if (PAD == KM_PAD_FILL) inv_mask = 1.0f - km_bilinear_ones(t);  // 1 - grid_sample(ones): imgwarp.py:316
        T* __restrict__ out_px = dst_b + (size_t)(i_base + r) * g.w + j;
#pragma unroll 1
        for (int c = 0; c < NC; ++c) {
            const T* img = src_b + (size_t)c * src_plane;
            const float v00 = km_ld(img + t.i00), v01 = km_ld(img + t.i01);
            const float v10 = km_ld(img + t.i10), v11 = km_ld(img + t.i11);
            float acc = km_bilinear_masked(t, (float)v00, (float)v01, (float)v10, (float)v11);  // (out-of-bounds taps: zeros that are still multiplied - ATen's CPU rule)
            if (PAD == KM_PAD_FILL) acc = acc + inv_mask * a.fill[c];
            km_st(out_px + (size_t)c * dst_plane, acc);
        }
    }
}

// the tile once its box is known to fit (bx.staged): fill, positions, sample.  One barrier inside.
template <typename T, int CM, int NC, int PAD, typename SH>
__device__ __forceinline__ void kmp_tile_body(const KmWarpArgs<T>& a, const float (&m)[9], uint32_t b, int j0, int i0, const KmfBox& bx, const float4* s_rv, float* s_src) {
    constexpr int TW = SH::TW, TH = SH::TH, PITCH = SH::PITCH, ROWS = SH::ROWS;
    constexpr int RPT = TH / (256 / TW);  // output rows per thread (consecutive)
    static_assert(TW == 64 || TW == 32, "lane = output column");
    const KmWarpGeom<float>& g = a.g;
    const int tid = km_tid_pinned();
    const int j = j0 + (tid % TW);
    const int li_base = (tid / TW) * RPT;  // this thread's rows: li_base + r
    const int i_base = i0 + li_base;
    const int W = g.W, H = g.H;
    const int spad = (PAD == KM_PAD_FILL) ? KM_PAD_ZEROS : PAD;
    const size_t src_plane = (size_t)H * W, dst_plane = (size_t)g.h * g.w;
    const T* __restrict__ src_b = a.src + (size_t)b * NC * src_plane;
    T* __restrict__ dst_b = a.dst + (size_t)b * NC * dst_plane;

    // ---- the fill: requested before the positions.  fp32 storage: LDS-DMA, every pass in flight while the positions are computed ----
    constexpr bool DMA = sizeof(T) == 4;
    if constexpr (DMA) {
        kmf_stage_box_dma<NC, PITCH, ROWS>(reinterpret_cast<const float*>(src_b), src_plane, W, H, bx, s_src);
    } else {
        float oob[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) oob[c] = 0.f;
        kmf_stage_box_dyn<T, NC, PITCH>(src_b, src_plane, W, H, bx, s_src, oob);
    }

    // ---- this thread's positions ----
    const KmlHalf cu = kml_col_half<CM>(m, km_base_x<float, CM>(g, j));
    float xs[RPT], ys[RPT];
    bool inbox = true;
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        kmp_position<CM>(g, m, cu, s_rv, li_base + r, bx.fast, spad, xs[r], ys[r]);
        KmlTaps t;
        t.xf = km_floor(xs[r]); t.yf = km_floor(ys[r]);
        // (rows of the tile below the image bottom and columns right of it are not stored: no constraint)
        inbox = inbox & (kmf_in_box(t, bx) | (i_base + r >= g.h) | (j >= g.w));
    }
    if constexpr (DMA) KM_VMCNT0();
    __syncthreads();
    const bool all_in = __all(inbox);  // (by every lane of the wave: columns right of the image count as inside)
    if (j >= g.w) return;
    if (!all_in) {  // keeps the result independent of the box estimate
        kmp_pixel_rows<T, CM, NC, PAD, RPT>(a, m, s_rv, bx.fast, b, j, li_base, i_base);
        return;
    }
    // ---- sample: lane = output column, (x0, x0 + 1) of a row of the footprint with one ds_read2_b32 ----
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        if (i_base + r >= g.h) break;  // (the tile hangs over the bottom edge; the rows that follow do too)
        KmBilin<float> t;
        km_bilinear_setup(xs[r], ys[r], W, H, t);
        float inv_mask = 0.f;
        if (PAD == KM_PAD_FILL) inv_mask = 1.0f - km_bilinear_ones(t);
        const int xi = KM_F2I(km_floor(xs[r])) - bx.xs, yi = KM_F2I(km_floor(ys[r])) - bx.ys;
        const float* q0 = s_src + __mul24(yi, NC * PITCH) + xi;
        const float* q1 = q0 + NC * PITCH;
        T* __restrict__ out_px = dst_b + (size_t)(i_base + r) * g.w + j;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float v00 = q0[c * PITCH], v01 = q0[c * PITCH + 1], v10 = q1[c * PITCH], v11 = q1[c * PITCH + 1];
            float acc = km_fma(v11, t.w11, km_fma(v10, t.w10, km_fma(v01, t.w01, km_fma(v00, t.w00, 0.0f))));
            if (PAD == KM_PAD_FILL) acc = acc + inv_mask * a.fill[c];
            km_st(out_px + (size_t)c * dst_plane, acc);
        }
    }
}

template <typename T, int CM, int NC, int PAD>
__global__ __launch_bounds__(256, KMP_WAVES_PER_EU) void km_warp_fwd_box_pad_kernel(const KmWarpArgs<T> a) {
    static_assert(KmpWide::TH == KmpSquare::TH && KmpWide::TW == 2 * KmpSquare::TW, "a wide tile is two square ones side by side");
    __shared__ float4 s_rv[KmpWide::TH];
    __shared__ int s_info[8];
    __shared__ __attribute__((aligned(16))) float s_src[KMP_LDS_FLOATS(NC)];  // [row][channel][x]
    const KmWarpGeom<float>& g = a.g;
    uint32_t bid = km_xcd_remap(blockIdx.x, a.nblocks);
    const uint32_t tx = bid % a.tiles_x;
    bid /= a.tiles_x;
    const uint32_t ty = bid % a.tiles_y;
    const uint32_t b = bid / a.tiles_y;
    const int tid = km_tid_pinned();
    const int J0 = (int)tx * KmpWide::TW, I0 = (int)ty * KmpWide::TH;
    if (a.apply && !a.apply[b]) {  // block-uniform: this sample is not transformed
        km_fwd_copy_rows<T>(a, b, J0 + (tid % KmpWide::TW), I0 + (tid / KmpWide::TW) * (KmpWide::TH / 4), 1, KmpWide::TH / 4);
        return;
    }
    float m[9];
    {
        // (block-uniform, into scalar registers before the fill is requested: see kmb_region in km_warp.hip)
        const float* mp = a.mat + (size_t)(g.B_M == 1 ? 0 : b) * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(mp[k])));
    }
    // ---- 1. the region as one wide tile ----
    kmp_tile_setup<CM, PAD, KmpWide>(g, m, J0, I0, s_rv, s_info);
    __syncthreads();
    const KmfBox bxw = kmf_read_box(s_info);
    if (bxw.staged) {
        kmp_tile_body<T, CM, NC, PAD, KmpWide>(a, m, b, J0, I0, bxw, s_rv, s_src);
        return;
    }
    // (The zeros kernel's "3 before 2" for maps that minify - the per-pixel rows for a region whose output rows stay horizontal in the
    // source - measured SLOWER here than the squares: 256x3x224^2 bf16 at scale 0.8, 0.088 ms against 0.079.)
    // ---- 2. the two square halves, one after the other; 3. per pixel for a half whose box does not fit either ----
    for (int half = 0; half < 2; ++half) {
        const int j0 = J0 + half * KmpSquare::TW;
        if (j0 >= g.w) break;  // block-uniform
        __syncthreads();  // the previous attempt's readers are done with s_info, s_rv and s_src
        kmp_tile_setup<CM, PAD, KmpSquare>(g, m, j0, I0, s_rv, s_info);
        __syncthreads();
        const KmfBox bx = kmf_read_box(s_info);
        if (bx.staged) {
            kmp_tile_body<T, CM, NC, PAD, KmpSquare>(a, m, b, j0, I0, bx, s_rv, s_src);
        } else {
            constexpr int RPT = KmpSquare::TH / (256 / KmpSquare::TW);
            const int t2 = km_tid_pinned(), j = j0 + (t2 % KmpSquare::TW), li_base = (t2 / KmpSquare::TW) * RPT;
            if (j < g.w) kmp_pixel_rows<T, CM, NC, PAD, RPT>(a, m, s_rv, bx.fast, b, j, li_base, I0 + li_base);
        }
    }
}

template <typename T, int CM, int NC>
static void kmp_launch_nc(const KmWarpArgs<T>& a, hipStream_t s) {
    const dim3 grid(a.nblocks), block(256);
    if (a.g.pad == KM_PAD_BORDER) hipLaunchKernelGGL((km_warp_fwd_box_pad_kernel<T, CM, NC, KM_PAD_BORDER>), grid, block, 0, s, a);
    else if (a.g.pad == KM_PAD_REFLECTION) hipLaunchKernelGGL((km_warp_fwd_box_pad_kernel<T, CM, NC, KM_PAD_REFLECTION>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((km_warp_fwd_box_pad_kernel<T, CM, NC, KM_PAD_FILL>), grid, block, 0, s, a);
}

// bilinear + border / reflection / fill, RGB / grey, rows of whole 16-byte chunks, 32-bit byte offsets inside a plane, 24-bit row / column
// counts.  The launch policy (warp_fwd_algo) is the caller's.
template <typename T, int CM>
static int kmp_try(const KmWarpArgs<T>& a0, hipStream_t s) {
    const KmWarpGeom<float>& g = a0.g;
    const uint64_t nb = (uint64_t)((g.w + KmpWide::TW - 1) / KmpWide::TW) * (uint64_t)((g.h + KmpWide::TH - 1) / KmpWide::TH) * (uint64_t)g.B;
    if (g.interp != KM_INTERP_BILINEAR || !(g.pad == KM_PAD_BORDER || g.pad == KM_PAD_REFLECTION || g.pad == KM_PAD_FILL)) return 0;
    if (!(g.C == 3 || g.C == 1) || (g.W & 3) != 0 || ((uintptr_t)a0.src % (4 * sizeof(T))) != 0 || nb >= (1ull << 31)) return 0;
    if ((uint64_t)g.H * g.W * 4 >= (1ull << 32) || (uint64_t)g.h * g.w * 4 >= (1ull << 32) || g.W >= (1 << 23) || g.H >= (1 << 23)) return 0;
    KmWarpArgs<T> a = a0;
    a.tiles_x = (uint32_t)((g.w + KmpWide::TW - 1) / KmpWide::TW);
    a.tiles_y = (uint32_t)((g.h + KmpWide::TH - 1) / KmpWide::TH);
    a.nblocks = (uint32_t)nb;
    if (g.C == 3) kmp_launch_nc<T, CM, 3>(a, s);
    else kmp_launch_nc<T, CM, 1>(a, s);
    return 1;
}

template <typename T>
static int kmp_try_any(const KmWarpArgs<T>& a, int coord_mode, hipStream_t s) {
    if (coord_mode == KM_COORD_PERSPECTIVE) return kmp_try<T, KM_COORD_PERSPECTIVE>(a, s);
    if (coord_mode == KM_COORD_AFFINE) return kmp_try<T, KM_COORD_AFFINE>(a, s);
    return 0;  // homography_warp's base grids, explicit grids: the generic kernel
}
// (the storage types with fp32 compute; fp64 computes in double: the generic kernel)
int km_warp_fwd_box_pad_try_any(const KmWarpArgs<float>& a, int coord_mode, hipStream_t s) { return kmp_try_any(a, coord_mode, s); }
int km_warp_fwd_box_pad_try_any(const KmWarpArgs<km_bf16>& a, int coord_mode, hipStream_t s) { return kmp_try_any(a, coord_mode, s); }
int km_warp_fwd_box_pad_try_any(const KmWarpArgs<km_f16>& a, int coord_mode, hipStream_t s) { return kmp_try_any(a, coord_mode, s); }
