// kornia_amd - median_blur (reference: kornia/filters/median.py:35-72 - a one-hot conv2d that writes a (B C, ky kx, H, W) copy of the
// image, then torch.median over it) as ONE pass: read x once, write y once, 2e bytes / element.
//
// What the reference computes, restated: zero-pad by (ky / 2, kx / 2), take the window's element of rank (n - 1) / 2, n = ky kx (padding
// zeros take part).  Selection is exact in every storage type, so the forward is bit-identical to the reference in f32 / f64 / bf16 / f16.
// Non-finite inputs: for n >= 2 an output is NaN exactly when its window holds a NaN or +-inf of the image (the one-hot convolution
// multiplies the other taps by 0, and 0 * inf is NaN); n == 1 is the identity.
// Gradient: grad_out of a pixel goes to the one window position that supplied the median; among equal values the SMALLEST ROW-MAJOR
// WINDOW POSITION (p kx + q) - the forward records it in a uint8 plane (`idx`, n <= 225), the backward gathers through it: no atomics,
// one rounding, the same bits from run to run.  A position in the padding drops its gradient.
//
// Two forwards:
//   * km_median_reg_kernel - 3x3 and 5x5, f32 / bf16 / f16 widened to f32, W % 4 == 0 and aligned rows: the register tiling of
//     km_filter2d_fast.hip (a lane owns 4 adjacent columns, a wave walks a strip of KMM_ROWS rows with the last K input rows in registers).
//     3x3: every column triple sorted once (min3 / med3 / max3) and shared by the up to three windows over it, then
//     med3(max3(lows), med3(mids), min3(highs)).  5x5: the generated network of km_median5_net.h (columns sorted once, sorted pairs and
//     quads shared between the windows).
//   * km_median_generic_kernel - every other odd (ky, kx) up to 15 x 15, f64, W % 4 != 0, unaligned: an LDS tile with its halo, one
//     output per thread, selection by rank - the first row-major candidate c with #(v < c) <= (n - 1) / 2 < #(v <= c) is the median and
//     the tie rule's position at once.
// Both take `apply` (B floats: a sample with apply <= 0.5 is copied through in the same launch - the augmentation layer's switch) and
// write `idx` only in the IDX instantiation (inference pays nothing for it).
#include "km_regtile.h"

#define KMM_ROWS 32   // rows of a wave's strip in the register-tiled kernel
#define KMM_MAXK 15   // largest window side of the generic kernel
#define KMM_TW 32     // its output tile: 32 x 8 pixels, one per thread
#define KMM_TH 8

__device__ __forceinline__ float kmm_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float kmm_max(float a, float b) { return fmaxf(a, b); }
#include "km_median5_net.h"

template <typename T>
struct KmMedArgs {
    const T* x;
    T* y;
    uint8_t* idx;        // (B C H W) window position of the median, IDX instantiations only
    const float* apply;  // (B) or null: the sample is filtered where apply > 0.5 and copied elsewhere
    int C, H, W, ky, kx;
    uint32_t tiles_x, tiles_y, nblocks;
};

// |v| as an integer: >= 0x7f800000 exactly for +-inf and NaN
__device__ __forceinline__ uint32_t kmm_absbits(float v) { return __float_as_uint(v) & 0x7fffffffu; }
__device__ __forceinline__ uint32_t kmm_umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ bool kmm_nonfinite(float v) { return kmm_absbits(v) >= 0x7f800000u; }
__device__ __forceinline__ bool kmm_nonfinite(double v) { return !(km_fabs(v) < (double)__builtin_inff()); }
__device__ __forceinline__ float kmm_nan(const float*) { return __builtin_nanf(""); }
__device__ __forceinline__ double kmm_nan(const double*) { return __builtin_nan(""); }

// the lane's four medians of a K x (4 + 2 PD) register window (rows in any order)
__device__ __forceinline__ void kmm_median4(const float (&w)[3][6], float (&out)[4]) {
    float lo[6], mi[6], hi[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        lo[c] = km_min3(w[0][c], w[1][c], w[2][c]);
        mi[c] = km_med3(w[0][c], w[1][c], w[2][c]);
        hi[c] = km_max3(w[0][c], w[1][c], w[2][c]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        out[c] = km_med3(km_max3(lo[c], lo[c + 1], lo[c + 2]), km_med3(mi[c], mi[c + 1], mi[c + 2]), km_min3(hi[c], hi[c + 1], hi[c + 2]));
}
__device__ __forceinline__ void kmm_median4(const float (&w)[5][8], float (&out)[4]) { kmm_median5x4(w, out); }

template <typename T, int K, bool IDX>
__global__ __launch_bounds__(256) void km_median_reg_kernel(const KmMedArgs<T> a) {
    constexpr int PD = (K - 1) / 2, NV = 4 + 2 * PD;
    const auto [tbx, tby, bc] = km_tile_of(a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gx = (int)tbx * 64 + lane;               // column group (4 px)
    const int r0 = ((int)tby * 4 + wave) * KMM_ROWS;   // first output row of this wave's strip
    const int H = a.H, W = a.W;
    if (gx * 4 >= W || r0 >= H) return;
    const int c0 = gx * 4;
    const size_t plane = (size_t)H * W;
    const T* img = a.x + (size_t)bc * plane;
    T* out = a.y + (size_t)bc * plane;
    const int n_rows = (r0 + KMM_ROWS <= H ? KMM_ROWS : H - r0);

    if (a.apply != nullptr && !(a.apply[bc / (uint32_t)a.C] > 0.5f)) {  // (block-uniform) the sample is not transformed: its rows as they are
        for (int r = r0; r < r0 + n_rows; ++r) {
            float v[4];
            km_ld4(img + (size_t)r * W + c0, v);
            km_st4(out + (size_t)r * W + c0, v);
        }
        return;
    }

    // halo columns: zero padding outside the row (the address stays inside it)
    int hl[PD], hr[PD];
    bool okl[PD], okr[PD];
#pragma unroll
    for (int q = 0; q < PD; ++q) {
        const int il = c0 - PD + q, ir = c0 + 4 + q;
        okl[q] = il >= 0; hl[q] = okl[q] ? il : 0;
        okr[q] = ir < W; hr[q] = okr[q] ? ir : 0;
    }

    float ring[K][NV];   // last K input rows: ring[.][i] = column c0 - PD + i
    uint32_t big[K];     // per row: the largest |v| (as an integer) of the lane's NV values - a NaN or inf anywhere in it shows here
    const int total = n_rows + K - 1;
    for (int it0 = 0; it0 < total; it0 += K) {
#pragma unroll
        for (int kk = 0; kk < K; ++kk) {
            const int it = it0 + kk;
            if (it < total) {
                const int srow = r0 - PD + it;  // wave-uniform
                if (srow >= 0 && srow < H) {
                    const T* rowp = img + (size_t)srow * W;
                    float o4[4];
                    km_ld4(rowp + c0, o4);
#pragma unroll
                    for (int q = 0; q < PD; ++q) {
                        const float vl = (float)km_ld(rowp + hl[q]), vr = (float)km_ld(rowp + hr[q]);
                        ring[kk][q] = okl[q] ? vl : 0.f;
                        ring[kk][PD + 4 + q] = okr[q] ? vr : 0.f;
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) ring[kk][PD + q] = o4[q];
                    uint32_t m = 0;
#pragma unroll
                    for (int q = 0; q < NV; ++q) m = kmm_umax(m, kmm_absbits(ring[kk][q]));
                    big[kk] = m;
                } else {
#pragma unroll
                    for (int q = 0; q < NV; ++q) ring[kk][q] = 0.f;
                    big[kk] = 0;
                }
                if (it >= K - 1) {
                    const int r = r0 + it - (K - 1);
                    float res[4];
                    kmm_median4(ring, res);
                    if constexpr (IDX) {
                        // the smallest row-major window position whose value equals the median (positions walked backwards, the last hit stays)
                        uint32_t packed = 0;
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            uint32_t pos = 0;
#pragma unroll
                            for (int p = K - 1; p >= 0; --p)
#pragma unroll
                                for (int q = K - 1; q >= 0; --q) pos = (ring[(kk + 1 + p) % K][c + q] == res[c]) ? (uint32_t)(p * K + q) : pos;
                            packed |= pos << (8 * c);
                        }
                        uint8_t* ip = a.idx + (size_t)bc * plane + (size_t)r * W + c0;
                        KM_CHECK_ALIGNED(ip, 4);
                        *reinterpret_cast<uint32_t*>(ip) = packed;
                    }
                    uint32_t m = big[0];
#pragma unroll
                    for (int p = 1; p < K; ++p) m = kmm_umax(m, big[p]);
                    if (m >= 0x7f800000u) {  // (rare) a NaN or inf among the lane's K x NV values: decide per output over its own window
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            bool bad = false;
#pragma unroll
                            for (int p = 0; p < K; ++p)
#pragma unroll
                                for (int q = 0; q < K; ++q) bad = bad || kmm_nonfinite(ring[p][c + q]);
                            res[c] = bad ? kmm_nan((const float*)nullptr) : res[c];
                        }
                    }
                    km_st4(out + (size_t)r * W + c0, res);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Generic forward: an LDS tile of (KMM_TH + ky - 1) x (KMM_TW + kx - 1) values (zeros outside the image), one output per thread.
template <typename T, bool IDX>
__global__ __launch_bounds__(256) void km_median_generic_kernel(const KmMedArgs<T> a) {
    typedef typename KmTraits<T>::R R;
    __shared__ R tile[(KMM_TH + KMM_MAXK - 1) * (KMM_TW + KMM_MAXK - 1)];
    uint32_t bid = blockIdx.x;
    const uint32_t tbx = bid % a.tiles_x;
    bid /= a.tiles_x;
    const uint32_t tby = bid % a.tiles_y;
    const uint32_t bc = bid / a.tiles_y;
    const int H = a.H, W = a.W, ky = a.ky, kx = a.kx;
    const int lx = threadIdx.x % KMM_TW, ly = threadIdx.x / KMM_TW;
    const int x0 = (int)tbx * KMM_TW, y0 = (int)tby * KMM_TH;
    const int ox = x0 + lx, oy = y0 + ly;
    const size_t plane = (size_t)H * W;
    const T* img = a.x + (size_t)bc * plane;
    T* out = a.y + (size_t)bc * plane;
    const bool inside = ox < W && oy < H;

    if (a.apply != nullptr && !(a.apply[bc / (uint32_t)a.C] > 0.5f)) {  // (block-uniform) copied through
        if (inside) out[(size_t)oy * W + ox] = img[(size_t)oy * W + ox];
        return;
    }
    const int py = ky / 2, px = kx / 2, tw = KMM_TW + kx - 1, th = KMM_TH + ky - 1;
    for (int t = (int)threadIdx.x; t < tw * th; t += 256) {
        const int sy = y0 - py + t / tw, sx = x0 - px + t % tw;
        R v = (R)0;
        if (sy >= 0 && sy < H && sx >= 0 && sx < W) v = (R)km_ld(img + (size_t)sy * W + sx);
        tile[t] = v;
    }
    __syncthreads();
    if (!inside) return;

    const int n = ky * kx, m = (n - 1) / 2;
    const R* w0 = tile + ly * tw + lx;  // the window's top-left value
    R med = w0[0];
    int pos = 0;
    if (n > 1) {
        bool bad = false;
        for (int p = 0; p < ky; ++p)
            for (int q = 0; q < kx; ++q) bad = bad || kmm_nonfinite(w0[p * tw + q]);
        if (bad) {
            med = kmm_nan((const R*)nullptr);
        } else {
            for (int cp = 0; cp < ky; ++cp) {
                bool found = false;
                for (int cq = 0; cq < kx; ++cq) {
                    const R c = w0[cp * tw + cq];
                    int lt = 0, le = 0;
                    for (int p = 0; p < ky; ++p)
                        for (int q = 0; q < kx; ++q) {
                            const R v = w0[p * tw + q];
                            lt += v < c ? 1 : 0;
                            le += v <= c ? 1 : 0;
                        }
                    if (lt <= m && m < le) {
                        med = c;
                        pos = cp * kx + cq;
                        found = true;
                        break;
                    }
                }
                if (found) break;
            }
        }
    }
    km_st(out + (size_t)oy * W + ox, med);
    if constexpr (IDX) a.idx[(size_t)bc * plane + (size_t)oy * W + ox] = (uint8_t)pos;
}

// ------------------------------------------------------------------------------------------------
// Backward, a gather: gx[i, j] = sum over (p, q) in row-major order of gy[i - p + ky/2, j - q + kx/2] where that output's median came
// from window position p kx + q.  fp32 accumulation (fp64 for f64), one rounding; one thread per input pixel.
template <typename T>
__global__ __launch_bounds__(256) void km_median_bwd_kernel(const T* gy, const uint8_t* idx, const float* apply, T* gx, int C, int H, int W, int ky, int kx,
                                                            uint64_t total) {
    typedef typename KmTraits<T>::R R;
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const uint64_t plane = (uint64_t)H * W;
    const uint64_t bc = e / plane;
    const uint32_t rem = (uint32_t)(e - bc * plane);
    const int i = (int)(rem / (uint32_t)W), j = (int)(rem % (uint32_t)W);
    if (apply != nullptr && !(apply[bc / (uint32_t)C] > 0.5f)) {  // the forward copied this sample
        gx[e] = gy[e];
        return;
    }
    const T* g = gy + bc * plane;
    const uint8_t* ix = idx + bc * plane;
    const int py = ky / 2, px = kx / 2;
    R acc = (R)0;
    for (int p = 0; p < ky; ++p) {
        const int oi = i - p + py;
        if (oi < 0 || oi >= H) continue;
        for (int q = 0; q < kx; ++q) {
            const int oj = j - q + px;
            if (oj < 0 || oj >= W) continue;
            const size_t o = (size_t)oi * W + oj;
            if ((int)ix[o] == p * kx + q) acc += (R)km_ld(g + o);
        }
    }
    km_st(gx + e, acc);
}

// ------------------------------------------------------------------------------------------------
template <typename T>
static bool kmm_fast_ok(const void* x, const void* y, const void* idx, int H, int W, int ky, int kx) {
    if (ky != kx || !(ky == 3 || ky == 5)) return false;
    if ((W & 3) != 0 || W < 4 || H < 1) return false;
    const size_t al = 4 * sizeof(T);
    return ((uintptr_t)x % al) == 0 && ((uintptr_t)y % al) == 0 && ((uintptr_t)idx % 4) == 0;
}

template <typename T>
static int kmm_fwd_fast(const void* x, void* y, void* idx, const void* apply, int B, int C, int H, int W, int K, hipStream_t s) {
    KmMedArgs<T> a;
    a.x = (const T*)x; a.y = (T*)y; a.idx = (uint8_t*)idx; a.apply = (const float*)apply;
    a.C = C; a.H = H; a.W = W; a.ky = K; a.kx = K;
    if (km_set_grid(a, (W / 4 + 63) / 64, (H + 4 * KMM_ROWS - 1) / (4 * KMM_ROWS), (uint64_t)B * C, "km_median_blur_fwd")) return -1;
    if (K == 3) {
        if (idx) hipLaunchKernelGGL((km_median_reg_kernel<T, 3, true>), dim3(a.nblocks), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((km_median_reg_kernel<T, 3, false>), dim3(a.nblocks), dim3(256), 0, s, a);
    } else {
        if (idx) hipLaunchKernelGGL((km_median_reg_kernel<T, 5, true>), dim3(a.nblocks), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((km_median_reg_kernel<T, 5, false>), dim3(a.nblocks), dim3(256), 0, s, a);
    }
    return km_check_launch("km_median_blur_fwd(reg)");
}

template <typename T>
static int kmm_fwd_generic(const void* x, void* y, void* idx, const void* apply, int B, int C, int H, int W, int ky, int kx, hipStream_t s) {
    KmMedArgs<T> a;
    a.x = (const T*)x; a.y = (T*)y; a.idx = (uint8_t*)idx; a.apply = (const float*)apply;
    a.C = C; a.H = H; a.W = W; a.ky = ky; a.kx = kx;
    if (km_set_grid(a, (W + KMM_TW - 1) / KMM_TW, (H + KMM_TH - 1) / KMM_TH, (uint64_t)B * C, "km_median_blur_fwd")) return -1;
    if (idx) hipLaunchKernelGGL((km_median_generic_kernel<T, true>), dim3(a.nblocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((km_median_generic_kernel<T, false>), dim3(a.nblocks), dim3(256), 0, s, a);
    return km_check_launch("km_median_blur_fwd(generic)");
}

template <typename T>
static int kmm_fwd(const void* x, void* y, void* idx, const void* apply, int B, int C, int H, int W, int ky, int kx, hipStream_t s) {
    if constexpr (sizeof(typename KmTraits<T>::R) == 4) {
        if (kmm_fast_ok<T>(x, y, idx, H, W, ky, kx)) return kmm_fwd_fast<T>(x, y, idx, apply, B, C, H, W, ky, s);
    }
    return kmm_fwd_generic<T>(x, y, idx, apply, B, C, H, W, ky, kx, s);
}

template <typename T>
static int kmm_bwd(const void* gy, const void* idx, const void* apply, void* gx, int B, int C, int H, int W, int ky, int kx, hipStream_t s) {
    const uint64_t total = (uint64_t)B * C * H * W;
    const uint64_t nb = (total + 255) / 256;
    KM_REQUIRE(nb < (1ull << 31), "km_median_blur_bwd: grid too large");
    hipLaunchKernelGGL((km_median_bwd_kernel<T>), dim3((uint32_t)nb), dim3(256), 0, s, (const T*)gy, (const uint8_t*)idx, (const float*)apply, (T*)gx, C, H, W,
                       ky, kx, total);
    return km_check_launch("km_median_blur_bwd");
}

static bool kmm_window_ok(int ky, int kx) { return ky >= 1 && kx >= 1 && (ky & 1) && (kx & 1) && ky <= KMM_MAXK && kx <= KMM_MAXK; }

extern "C" {

// 1 when km_median_blur_fwd / _bwd take this window and dtype: odd sides of 1 .. 15, f32 / f64 / bf16 / f16 (include/kornia_amd.h)
int km_median_blur_supported(int ky, int kx, int dtype) { return (kmm_window_ok(ky, kx) && dtype >= KM_F32 && dtype <= KM_F16) ? 1 : 0; }

int km_median_blur_fwd(const void* x, void* y, void* idx, const void* apply, int B, int C, int H, int W, int ky, int kx, int dtype, void* stream) {
    KM_REQUIRE(kmm_window_ok(ky, kx), "km_median_blur_fwd: the window must have odd sides of 1 .. %d, got (%d, %d)", KMM_MAXK, ky, kx);
    KM_REQUIRE(dtype >= KM_F32 && dtype <= KM_F16, "km_median_blur_fwd: bad dtype %d", dtype);
    KM_REQUIRE(B >= 0 && C >= 0 && H >= 0 && W >= 0 && (int64_t)H * W < (1ll << 31), "km_median_blur_fwd: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
    if ((uint64_t)B * C * H * W == 0) return 0;
    KM_REQUIRE(x && y, "km_median_blur_fwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    return km_dispatch_dtype<float, double, km_bf16, km_f16>(dtype, -1, [&](auto t) { return kmm_fwd<KM_TAG_T(t)>(x, y, idx, apply, B, C, H, W, ky, kx, s); });
}

int km_median_blur_bwd(const void* gy, const void* idx, const void* apply, void* gx, int B, int C, int H, int W, int ky, int kx, int dtype, void* stream) {
    KM_REQUIRE(kmm_window_ok(ky, kx), "km_median_blur_bwd: the window must have odd sides of 1 .. %d, got (%d, %d)", KMM_MAXK, ky, kx);
    KM_REQUIRE(dtype >= KM_F32 && dtype <= KM_F16, "km_median_blur_bwd: bad dtype %d", dtype);
    KM_REQUIRE(B >= 0 && C >= 0 && H >= 0 && W >= 0 && (int64_t)H * W < (1ll << 31), "km_median_blur_bwd: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
    if ((uint64_t)B * C * H * W == 0) return 0;
    KM_REQUIRE(gy && idx && gx, "km_median_blur_bwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    return km_dispatch_dtype<float, double, km_bf16, km_f16>(dtype, -1, [&](auto t) { return kmm_bwd<KM_TAG_T(t)>(gy, idx, apply, gx, B, C, H, W, ky, kx, s); });
}

}  // extern "C"
