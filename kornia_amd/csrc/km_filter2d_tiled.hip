// kornia_amd - LDS-tiled dense kH x kW filter2d for the shapes the register-tiled kernels (km_filter2d_fast.hip: 'same', square odd
// 3 / 5 / 7, W % 4 == 0, 16-byte aligned, not fp64) leave out: 1 <= kH, kW <= 31 with kH * kW >= 2, 'same' and 'valid' padding, every
// border, every dtype, any width and alignment.  Forward, input adjoint and tap gradient; results are those of the generic kernels of
// km_filter.hip (forward and adjoint bit for bit, the tap gradient up to the order of its sums).
// Reference: kornia/filters/filter.py:121-150 (F.pad + grouped F.conv2d) and its autograd.
//
// Kernel 1, km_filter2d_tile_kernel (forward; adjoint through `flip`): a 256-thread block owns a 64 x 64 output tile (64 x 32 for fp64:
// the window of a 31 x 31 kernel is then 62 x 100 doubles = 49 600 B instead of 75 200 B, inside KM_LDS_LIMIT).  It stages the
// (TH + kH - 1) x (64 + kW - 1) input window in LDS in the compute type, THE BORDER RULE APPLIED WHILE STAGING (constant and 'valid':
// zeros), so the inner loop has no border logic and no bounds test.  A thread computes 4 columns x RPT rows (RPT = 4, fp64: 2): per window
// row and block of 8 taps along x it reads 12 consecutive window values (three 16-byte LDS reads) and feeds up to RPT x 8 x 4 = 128 fused
// multiply-adds from them.  The taps are block-uniform: read through a uniform pointer, they come by scalar loads.
//   LDS reads are conflict-free: the 16 lanes of a quarter wave hold the 16 column groups of one thread row, so one 16-byte read of theirs
//   covers 256 consecutive bytes - every bank once - whatever the row pitch is; the pitch only has to be a multiple of 4 elements for the
//   16-byte alignment (64 + 8 * ceil(kW / 8) + 4: room for the 12-value read of the last column group's last tap block).
//   Accumulation order per output: acc = 0, then km_fma(k[p][q], v, acc) with p outer and q inner, both ascending - the generic kernel's
//   and the oracle's (oracle/ko_impl.h ko_filter2d_fwd), so fp32 results are bit-identical to both.
//   flip = 1: gx[py][px] = sum_{p,q} k[p][q] * gy0[py + pt - p][px + pl - q] with gy0 the zero-extended gradient - the adjoint of the
//   constant-padded and of the 'valid' correlation, and the interior of every other one (km_filter.hip recomputes the pad-wide frame with
//   the exact pre-image kernel).  The window is staged MIRRORED (element (a, b) <- gy0[ys - a][xs - b]) and the tile is stored mirrored:
//   the inner loop is the forward's, untouched, and its (p, q) order is km_f2d_adjoint_pixel's for the pixel itself.
//
// Kernel 2, km_filter2d_tapgrad_tile_kernel: gk[b % Bk][p][q] += sum_{c,i,j} gy[b,c,i,j] * xpad[b,c,i+p,j+q] in ONE pass over the image
// (the generic kernel makes kH * kW passes).  A block walks a contiguous run of (plane, tile) pairs, the grid capped at 4 blocks per CU.
// Per pair it stages the 64 x 32 (fp64: 64 x 16) gy tile and the matching border-folded x window in LDS.  Lanes own taps: thread =
// (slice, p, group of 4 adjacent q), consecutive lanes on consecutive q groups; 256 / (kH * ceil(kW / 4)) slices share the tile's rows.
// Per pixel row and 8 pixels a lane reads 12 x values (three 16-byte reads, consecutive lanes consecutive addresses) and 8 gy values (two
// 16-byte broadcast reads) for 32 multiply-adds.  The x pitch is 64 + 4 * ceil(kW / 4): that is 4 * ceil(kW / 4) modulo the 64 banks, so
// the lanes' reads continue bank after bank from one tap row p into the next.
//   Precision as in the register-tiled tap gradient (kmf_tapgrad_run): products and short sums in the compute type (fp32 fma chains of
//   at most 64 products: one pixel row of a tile), everything above in fp64 - registers across rows, tiles and planes, then one LDS
//   reduction over the slices and ONE km_atomic_add per tap when the block's kernel index b % Bk changes and one at its end, instead
//   of one per (plane, tap).  Pixels outside the image are skipped, not multiplied by zero, as in the generic kernel.
//
// No MFMA (as N1 of VERDICT.md says for K = 3): the op is depthwise - one kernel per sample, shared by its channels, no reduction over
// channels to form a GEMM from -, its fp32 accumulation order is pinned bit for bit, and a Toeplitz GEMM formulation would spend most of
// its multiply-adds on structural zeros and change the rounding.
#include "km_filter_host.h"
#include "km_regtile.h"

#define KMT_TW 64
#define KMT_MAX_K 31

// four / twelve consecutive LDS values with 16-byte reads (p is 16-byte aligned)
struct __attribute__((aligned(16))) kmt_d2 { double x, y; };
__device__ __forceinline__ void kmt_lds4(const float* p, float* o) {
    KM_CHECK_ALIGNED(p, 16);
    const float4 v = *reinterpret_cast<const float4*>(p);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}
__device__ __forceinline__ void kmt_lds4(const double* p, double* o) {
    KM_CHECK_ALIGNED(p, 16);
    const kmt_d2 u = *reinterpret_cast<const kmt_d2*>(p), v = *reinterpret_cast<const kmt_d2*>(p + 2);
    o[0] = u.x; o[1] = u.y; o[2] = v.x; o[3] = v.y;
}
template <typename R>
__device__ __forceinline__ void kmt_lds12(const R* p, R (&w)[12]) {
    kmt_lds4(p, w); kmt_lds4(p + 4, w + 4); kmt_lds4(p + 8, w + 8);
}

// Stages a window of `rows` x `cols` into s[rows][pitch] (pitch <= 128; columns cols .. pitch-1 are zeroed): element (r, c) is the source
// pixel (ys + sgn * r, xs + sgn * c) taken through the border map, 0 where the map has no pixel.  Half a block per row, so the column map is
// fixed per thread and the row map is wave-uniform; 4 rows per trip with the loads issued together (clamped addresses, zeros selected after).
template <typename T, typename R>
__device__ __forceinline__ void kmt_stage(R* s, int rows, int cols, int pitch, const T* img, int sH, int sW, int ys, int xs, int sgn, int border) {
    const int c = threadIdx.x & 127;
    const int sx = c < cols ? km_border_map(xs + sgn * c, sW, border) : -1;
    for (int r0 = threadIdx.x >> 7; r0 < rows; r0 += 8) {
        R v[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r0 + 2 * u;
            const int sy = r < rows ? km_border_map(ys + sgn * r, sH, border) : -1;
            ok[u] = sy >= 0 && sx >= 0;
            v[u] = (R)km_ld(img + (size_t)(ok[u] ? sy : 0) * sW + (ok[u] ? sx : 0));
        }
        if (c < pitch) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (r0 + 2 * u < rows) s[(r0 + 2 * u) * pitch + c] = ok[u] ? v[u] : (R)0;
        }
    }
}

// =================================================================================================
// kernel 1: correlation tile
// =================================================================================================
template <typename T>
struct KmTileArgs {
    typedef typename KmTraits<T>::R R;
    const T* x;   // source planes (sH, sW): the input, or grad_out for flip
    T* y;         // destination planes (dH, dW)
    const R* k;   // (Bk, kH, kW)
    int C, Bk, kH, kW;
    int sH, sW, dH, dW;
    int oy, ox;   // source pixel of window element (0, 0) of tile (0, 0)
    int border;   // of the staging
    int flip;     // 1: window and tile mirrored (the adjoint)
    int pitch;    // LDS row pitch, elements
    int vec;      // 1: rows of the destination are aligned for 4-pixel stores
    uint32_t tiles_x, tiles_y, nblocks;
};

template <typename T, int RPT>
__global__ __launch_bounds__(256) void km_filter2d_tile_kernel(const KmTileArgs<T> a) {
    typedef typename KmTraits<T>::R R;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int TH = 16 * RPT;
    R* s_in = (R*)smem_raw;  // [TH + kH - 1][pitch]
    const int kH = a.kH, kW = a.kW, IP = a.pitch;
    const auto [tx, ty, bc] = km_tile_of(a);
    const int x0 = (int)tx * KMT_TW, y0 = (int)ty * TH;
    kmt_stage<T, R>(s_in, TH + kH - 1, KMT_TW + kW - 1, IP, a.x + (size_t)bc * a.sH * a.sW, a.sH, a.sW, y0 + a.oy, x0 + a.ox, a.flip ? -1 : 1, a.border);
    __syncthreads();

    const int cg = threadIdx.x & 15, rg = threadIdx.x >> 4;  // column group (4 px), row group (RPT rows)
    const R* kk = a.k + (size_t)((bc / (uint32_t)a.C) % (uint32_t)a.Bk) * kH * kW;  // block-uniform
    R acc[RPT][4];
#pragma unroll
    for (int r = 0; r < RPT; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0;
    const R* base = s_in + rg * RPT * IP + cg * 4;
    for (int wr = 0; wr < RPT + kH - 1; ++wr) {  // window row wr is tap row p = wr - r of the thread's output row r
        for (int q0 = 0; q0 < kW; q0 += 8) {
            R w[12];
            kmt_lds12(base + wr * IP + q0, w);
            const int nq = kW - q0;
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                const int p = wr - r;
                if (p < 0 || p >= kH) continue;
                const R* kp = kk + p * kW + q0;
                if (nq >= 8) {
#pragma unroll
                    for (int qq = 0; qq < 8; ++qq) {
                        const R kv = kp[qq];
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[r][c] = km_fma(kv, w[c + qq], acc[r][c]);
                    }
                } else {
#pragma unroll
                    for (int qq = 0; qq < 7; ++qq) {
                        if (qq < nq) {
                            const R kv = kp[qq];
#pragma unroll
                            for (int c = 0; c < 4; ++c) acc[r][c] = km_fma(kv, w[c + qq], acc[r][c]);
                        }
                    }
                }
            }
        }
    }

    // in-image outputs only; flip: local (r, c) is pixel (TH - 1 - r, 63 - c) of the tile, so a thread's 4 columns are still adjacent
    T* out = a.y + (size_t)bc * a.dH * a.dW;
    const int ox = a.flip ? x0 + KMT_TW - 4 - cg * 4 : x0 + cg * 4;
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int lr = rg * RPT + r;
        const int oy = a.flip ? y0 + TH - 1 - lr : y0 + lr;
        if (oy >= a.dH || ox >= a.dW) continue;
        R o[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = a.flip ? acc[r][3 - c] : acc[r][c];
        T* dst = out + (size_t)oy * a.dW + ox;
        if constexpr (sizeof(T) != 8) {
            if (a.vec && ox + 3 < a.dW) {
                km_st4(dst, o);
                continue;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (ox + c < a.dW) km_st(dst + c, o[c]);
    }
}

static int kmt_pitch(int kW) { return KMT_TW + 8 * ((kW + 7) / 8) + 4; }
template <typename R>
static size_t kmt_tile_lds(int kH, int kW) {
    return (size_t)(16 * (sizeof(R) == 8 ? 2 : 4) + kH - 1) * kmt_pitch(kW) * sizeof(R);
}

template <typename T>
static int kmt_run(const KmFilterCall& c, const void* x, const void* k, void* y, int flip) {
    typedef typename KmTraits<T>::R R;
    constexpr int RPT = sizeof(R) == 8 ? 2 : 4, TH = 16 * RPT;
    KmTileArgs<T> a;
    a.x = (const T*)x; a.y = (T*)y; a.k = (const R*)k;
    a.C = c.C; a.Bk = c.Bk; a.kH = c.kH; a.kW = c.kW;
    a.sH = flip ? c.Ho : c.H; a.sW = flip ? c.Wo : c.W;
    a.dH = flip ? c.H : c.Ho; a.dW = flip ? c.W : c.Wo;
    a.oy = flip ? c.pt + TH - 1 : -c.pt; a.ox = flip ? c.pl + KMT_TW - 1 : -c.pl;
    a.border = (!flip && c.same) ? c.border : KM_BORDER_CONSTANT;
    a.flip = flip;
    a.pitch = kmt_pitch(c.kW);
    a.vec = (a.dW % 4 == 0 && (uintptr_t)y % (4 * sizeof(T)) == 0) ? 1 : 0;
    if (km_set_grid(a, (a.dW + KMT_TW - 1) / KMT_TW, (a.dH + TH - 1) / TH, (uint64_t)c.B * c.C, "km_filter2d")) return -1;
    if (a.nblocks == 0) return 0;
    hipLaunchKernelGGL((km_filter2d_tile_kernel<T, RPT>), dim3(a.nblocks), dim3(256), kmt_tile_lds<R>(c.kH, c.kW), c.s, a);
    return km_check_launch(flip ? "km_filter2d_bwd_input(tiled)" : "km_filter2d_fwd(tiled)");
}

// =================================================================================================
// kernel 2: tap gradient
// =================================================================================================
struct KmTapSplit {
    int ngq;     // groups of 4 taps per tap row: ceil(kW / 4)
    int ng;      // tap groups: kH * ngq (<= 256)
    int slices;  // thread = slice * ng + group; slice s takes the tile rows s, s + slices, ...
    int xpitch;  // LDS row pitch of the x window
};

template <typename T>
struct KmTapTileArgs : KmTapSplit {
    const T* x;
    const T* gy;
    double* gk;  // (Bk, kH, kW) fp64 accumulators, zeroed by the caller
    KmFilterGeom g;
    uint32_t grid;                       // blocks launched; block i walks the pairs [i * nblocks / grid, (i + 1) * nblocks / grid)
    uint32_t tiles_x, tiles_y, nblocks;  // nblocks: (plane, tile) pairs
};

// dacc of every slice -> LDS, summed in slice order, one atomic per tap of kernel kb; dacc is cleared
template <typename T>
__device__ __forceinline__ void kmt_tap_flush(const KmTapTileArgs<T>& a, double* s_red, bool active, double (&dacc)[4], int kb) {
    const int tid = threadIdx.x, n = a.ng * 4;
    if (active) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            s_red[tid * 4 + t] = dacc[t];  // tid = slice * ng + group
            dacc[t] = 0.0;
        }
    }
    __syncthreads();
    for (int e = tid; e < n; e += 256) {
        double sm = 0.0;
        for (int s = 0; s < a.slices; ++s) sm += s_red[s * n + e];
        const int grp = e >> 2, p = grp / a.ngq, q = (grp - p * a.ngq) * 4 + (e & 3);
        if (q < a.g.kW && sm != 0.0) km_atomic_add(a.gk + ((size_t)kb * a.g.kH + p) * a.g.kW + q, sm);
    }
    __syncthreads();
}

template <typename T, int TH>
__global__ __launch_bounds__(256) void km_filter2d_tapgrad_tile_kernel(const KmTapTileArgs<T> a) {
    typedef typename KmTraits<T>::R R;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const KmFilterGeom& g = a.g;
    const int XH = TH + g.kH - 1, XP = a.xpitch;
    R* s_x = (R*)smem_raw;                          // [XH][XP]  border-folded input window
    R* s_g = s_x + XH * XP;                         // [TH][64]  grad_out tile
    double* s_red = (double*)(s_g + TH * KMT_TW);   // [slices][ng * 4]
    const int tid = threadIdx.x;
    const int slice = tid / a.ng, grp = tid - slice * a.ng, p = grp / a.ngq, qg = grp - p * a.ngq;
    const bool active = slice < a.slices;
    const int border = g.same ? g.border : KM_BORDER_CONSTANT;
    const size_t plane = (size_t)g.H * g.W, oplane = (size_t)g.Ho * g.Wo;

    double dacc[4] = {0.0, 0.0, 0.0, 0.0};
    int kb_cur = -1;
    const uint32_t first = (uint32_t)((uint64_t)blockIdx.x * a.nblocks / a.grid), last = (uint32_t)((uint64_t)(blockIdx.x + 1) * a.nblocks / a.grid);
    for (uint32_t pair = first; pair < last; ++pair) {
        const uint32_t tx = pair % a.tiles_x, rest = pair / a.tiles_x, ty = rest % a.tiles_y, bc = rest / a.tiles_y;
        const int kb = (int)((bc / (uint32_t)g.C) % (uint32_t)g.Bk);
        if (kb != kb_cur) {  // block-uniform
            if (kb_cur >= 0) kmt_tap_flush(a, s_red, active, dacc, kb_cur);
            kb_cur = kb;
        }
        const int x0 = (int)tx * KMT_TW, y0 = (int)ty * TH;
        const int nrows = g.Ho - y0 < TH ? g.Ho - y0 : TH, ncols = g.Wo - x0 < KMT_TW ? g.Wo - x0 : KMT_TW;
        kmt_stage<T, R>(s_x, XH, KMT_TW + g.kW - 1, XP, a.x + (size_t)bc * plane, g.H, g.W, y0 - g.pt, x0 - g.pl, 1, border);
        {
            const T* gyp = a.gy + (size_t)bc * oplane;
            const int j = tid & 63;
            for (int i = tid >> 6; i < TH; i += 4) {
                const bool ok = i < nrows && j < ncols;
                const R v = (R)km_ld(gyp + (ok ? (size_t)(y0 + i) * g.Wo + (x0 + j) : 0));
                s_g[i * KMT_TW + j] = ok ? v : (R)0;
            }
        }
        __syncthreads();
        if (active) {
            for (int i = slice; i < nrows; i += a.slices) {
                const R* xr = s_x + (i + p) * XP + 4 * qg;  // xr[j + t]: the pixel under tap (p, 4 qg + t) of output pixel (i, j)
                const R* gr = s_g + i * KMT_TW;
                R acc[4] = {0, 0, 0, 0};
                int j0 = 0;
                for (; j0 + 8 <= ncols; j0 += 8) {
                    R w[12], gv[8];
                    kmt_lds12(xr + j0, w);
                    kmt_lds4(gr + j0, gv); kmt_lds4(gr + j0 + 4, gv + 4);
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj)
#pragma unroll
                        for (int t = 0; t < 4; ++t) acc[t] = km_fma(gv[jj], w[jj + t], acc[t]);
                }
                if (j0 < ncols) {  // the image's last columns: pixels beyond them are skipped
                    R w[12], gv[8];
                    kmt_lds12(xr + j0, w);
                    kmt_lds4(gr + j0, gv); kmt_lds4(gr + j0 + 4, gv + 4);
#pragma unroll
                    for (int jj = 0; jj < 7; ++jj) {
                        if (j0 + jj < ncols) {
#pragma unroll
                            for (int t = 0; t < 4; ++t) acc[t] = km_fma(gv[jj], w[jj + t], acc[t]);
                        }
                    }
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) dacc[t] += (double)acc[t];
            }
        }
        __syncthreads();
    }
    if (kb_cur >= 0) kmt_tap_flush(a, s_red, active, dacc, kb_cur);
}

template <typename R>
static size_t kmt_tap_lds(int kH, int kW, KmTapSplit* split) {
    const int TH = sizeof(R) == 8 ? 16 : 32;
    const int ngq = (kW + 3) / 4, ng = kH * ngq, slices = 256 / ng < TH ? 256 / ng : TH, xpitch = KMT_TW + 4 * ngq;
    if (split) *split = KmTapSplit{ngq, ng, slices, xpitch};
    return ((size_t)(TH + kH - 1) * xpitch + (size_t)TH * KMT_TW) * sizeof(R) + (size_t)slices * ng * 4 * sizeof(double);
}

template <typename T>
static int kmt_tapgrad_run(const KmFilterCall& c, const void* gy, const void* x, double* gk) {
    typedef typename KmTraits<T>::R R;
    constexpr int TH = sizeof(R) == 8 ? 16 : 32;
    KmTapTileArgs<T> a;
    a.x = (const T*)x; a.gy = (const T*)gy; a.gk = gk; a.g = c;
    const size_t lds = kmt_tap_lds<R>(c.kH, c.kW, &a);
    if (km_set_grid(a, (c.Wo + KMT_TW - 1) / KMT_TW, (c.Ho + TH - 1) / TH, (uint64_t)c.B * c.C, "km_filter2d_bwd_kernel")) return -1;
    if (a.nblocks == 0) return 0;
    const int cus = km_device_cus();
    const uint32_t cap = (uint32_t)(cus > 0 ? cus : 1) * 4u;  // (LDS holds 3 - 4 blocks of a CU at a time; the host build of the kernels reports 0 CUs)
    a.grid = a.nblocks < cap ? a.nblocks : cap;
    hipLaunchKernelGGL((km_filter2d_tapgrad_tile_kernel<T, TH>), dim3(a.grid), dim3(256), lds, c.s, a);
    return km_check_launch("km_filter2d_bwd_kernel(tiled)");
}

// =================================================================================================
// host interface (km_filter_host.h)
// =================================================================================================
// 1 if the LDS-tiled kernels take this call: 1 <= kH, kW <= 31, at least two taps, and both kernels' LDS inside KM_LDS_LIMIT (fp64 shrinks
// its tiles for that); padding, border, dtype, width, alignment and kernel batch are all taken
int km_filter2d_tiled_supported(const KmFilterCall& c) {
    if (c.kH < 1 || c.kW < 1 || c.kH > KMT_MAX_K || c.kW > KMT_MAX_K || c.kH * c.kW < 2) return 0;
    const bool f64 = c.dtype == KM_F64;
    const size_t tile = f64 ? kmt_tile_lds<double>(c.kH, c.kW) : kmt_tile_lds<float>(c.kH, c.kW);
    const size_t tap = f64 ? kmt_tap_lds<double>(c.kH, c.kW, nullptr) : kmt_tap_lds<float>(c.kH, c.kW, nullptr);
    return tile <= KM_LDS_LIMIT && tap <= KM_LDS_LIMIT ? 1 : 0;
}

// flip = 0: y = filter2d(x, k) as the call says.  flip = 1: gx = the correlation of the zero-extended gy with the taps rotated by 180
// degrees: the whole adjoint for 'valid' and for a constant border, the interior of the others
int km_filter2d_tiled_run(const KmFilterCall& c, const void* x, const void* k, void* y, int flip) {
    return km_dispatch_dtype<float, double, km_bf16, km_f16>(c.dtype, -1, [&](auto t) { return kmt_run<KM_TAG_T(t)>(c, x, k, y, flip); });
}

int km_filter2d_tiled_tapgrad_run(const KmFilterCall& c, const void* gy, const void* x, double* gk) {
    return km_dispatch_dtype<float, double, km_bf16, km_f16>(c.dtype, -1, [&](auto t) { return kmt_tapgrad_run<KM_TAG_T(t)>(c, gy, x, gk); });
}
