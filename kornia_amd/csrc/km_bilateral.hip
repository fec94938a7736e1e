// kornia_amd - bilateral_blur / joint_bilateral_blur (reference: kornia/filters/bilateral.py:32-84 - pad, unfold the image and the guidance into
// (B, C, H, W, ky kx) copies, about ten elementwise passes over tensors of that size, two reductions) as ONE pass forward and ONE pass backward.
//
// What the reference computes, restated, for sample b and output pixel q (g: the guidance - the input itself for bilateral_blur):
//     D_qi = (sum_c |g^c(q+i) - g^c(q)|)^2  (l1)        D_qi = sum_c (g^c(q+i) - g^c(q))^2  (l2)
//     k_qi = s_i exp(coef_b D_qi),  coef_b = -0.5 / sigma_color_b^2        W_q = sum_i k_qi        y^c_q = (sum_i k_qi x^c(q+i)) / W_q
// q+i goes through the border rule of F.pad (constant: zeros, which take part in D and in the sums).  No tap is skipped and nothing is clamped:
// the reference's 0 * inf = NaN and inf - inf = NaN come out of the same arithmetic.  f32 / bf16 / f16 storage computes in fp32 with
// exp(a) = exp2(a log2(e)), log2(e) folded into coef (v_exp_f32); f64 in fp64 with exp.
//
// Forward, km_bilateral_fwd_kernel: an LDS tile with its halo per workgroup holding every input and guidance channel, widened and with the border
// resolved when it is filled - the tap loop is LDS reads and VALU only; one output pixel per thread.  Square windows 3 / 5 / 7 / 9 with up to 4 + 4
// channels are compile-time instantiations (f32 / bf16 / f16); everything else - other odd windows up to 15 x 15, up to 16 channels a side, f64 -
// takes run-time loops over a tile that the launcher shrinks until it fits 64 KB.  `wsum` (B, H, W) = W_q is written only when asked for.
//
// Backward, km_bilateral_bwd_kernel: a gather, no atomics, the same bits from run to run.  With G = grad_out and
// T_qi = sum_c G^c_q (x^c(q+i) - y^c_q) / W_q:
//     value gradient    gx^c(p)  = sum over (q, i) with map(q+i) = p  of  k_qi G^c_q / W_q
//     weight gradient   dL/dD_qi = coef k_qi T_qi;   dD/dg^c(q+i) = 2 S_qi sign(delta^c) (l1, sign(0) = 0) or 2 delta^c (l2);  dD/dg^c(q) = -that
// s and D are symmetric in (p, q), so pixel p forms every weight it needs from its own neighbourhood.  Interior tiles (no pixel within the
// pad of an edge) read x, g, y, G and wsum from LDS tiles with halo and make ONE exp per neighbour serve both directions; tiles at the border
// take the slower general path: the pre-images of p under the border rule (reflect: its mirror images, replicate: the run of padded positions
// of an edge pixel, circular: the wrapped copies, constant: none), each with the spatial weight at offset p~ - q - the adjoint of the pad.
// bilateral_blur: both gradients sum into gx; joint: the value gradient goes to gx, the weight gradient to gguide, each only when asked for.
#include "km_common.h"

#define KMB_MAXK 15         // largest window side
#define KMB_MAXC 16         // most channels of the input and of the guidance
#define KMB_TW 32           // output tile: 32 x 8 pixels, one per thread (the run-time forward shrinks it when the tile would pass KMB_LDS_BYTES)
#define KMB_TH 8
#define KMB_LDS_BYTES 65536

enum { KMB_CONSTANT = 0, KMB_REFLECT = 1, KMB_REPLICATE = 2, KMB_CIRCULAR = 3 };  // KM_CONSTANT .. KM_CIRCULAR of include/kornia_amd.h
enum { KMB_L1 = 0, KMB_L2 = 1 };                                                  // KM_DIST_L1 / KM_DIST_L2

// F.pad's border rule on one axis: the image coordinate that padded coordinate i reads; -1 for the zeros of `constant` (and for a position
// farther out than the pad, which only a thread without a pixel meets)
__device__ __forceinline__ int kmb_map(int i, int n, int border) {
    if (border == KMB_REFLECT) i = i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);
    else if (border == KMB_REPLICATE) i = i < 0 ? 0 : (i >= n ? n - 1 : i);
    else if (border == KMB_CIRCULAR) i = i < 0 ? i + n : (i >= n ? i - n : i);
    return (i >= 0 && i < n) ? i : -1;
}

// exp(coef D): fp32 as exp2 of (coef log2(e)) D, fp64 as exp
__device__ __forceinline__ float kmb_fold(float coef) { return coef * 1.4426950408889634f; }
__device__ __forceinline__ double kmb_fold(double coef) { return coef; }
__device__ __forceinline__ float kmb_exp(float a) { return km_exp2(a); }
__device__ __forceinline__ double kmb_exp(double a) { return exp(a); }

// one channel's share of the distance: |delta| (l1) or delta^2 (l2) added to d
template <typename R>
__device__ __forceinline__ R kmb_dist_add(R delta, bool l2, R d) {
    const R ad = km_fabs(delta);
    return km_fma(ad, l2 ? ad : (R)1, d);
}
// dD / d delta^c: 2 S sign(delta) (l1; S = sum_c |delta^c|, sign(0) = 0 as torch's abs) or 2 delta (l2)
template <typename R>
__device__ __forceinline__ R kmb_ddist(R delta, bool l2, R S) {
    const R sg = delta > (R)0 ? (R)1 : (delta < (R)0 ? (R)-1 : (delta == (R)0 ? (R)0 : delta));  // (NaN stays NaN)
    return (R)2 * (l2 ? delta : S * sg);
}

template <typename T>
struct KmbFwdArgs {
    typedef typename KmTraits<T>::R R;
    const T* x;      // (B, C, H, W)
    const T* g;      // (B, Cg, H, W) or null: self-guided
    const R* space;  // (Bs, ky kx)
    const R* coef;   // (Bc)
    T* y;
    R* wsum;         // (B, H, W) or null
    int C, Cg, H, W, ky, kx, border, dist, Bs, Bc;
    int tw, th;      // output tile (KMB_TW x KMB_TH in the compile-time instantiations)
    uint32_t tiles_x, tiles_y;
};

// K > 0: the K x K window with NX input channels and NG guidance channels (NG = 0: self-guided), all compile-time, the 32 x 8 tile.
// K = 0: run-time window, channel counts (at most MC a side) and tile.
template <typename T, int K, int NG, int NX, int MC>
__global__ __launch_bounds__(256) void km_bilateral_fwd_kernel(const KmbFwdArgs<T> a) {
    typedef typename KmTraits<T>::R R;
    constexpr int MCX = K ? NX : MC, MCG = K ? (NG ? NG : NX) : MC;
    R* tile;
    if constexpr (K != 0) {  // static: exactly the instantiation's planes
        __shared__ R tile_ct[(KMB_TH + (K ? K : 1) - 1) * (KMB_TW + (K ? K : 1) - 1) * (NG + NX)];
        tile = tile_ct;
    } else {  // dynamic: what the launcher's tile needs, at most KMB_LDS_BYTES
        extern __shared__ __attribute__((aligned(16))) char smem_raw[];
        tile = (R*)smem_raw;
    }
    const bool self = K ? NG == 0 : a.g == nullptr;
    const int nx = K ? NX : a.C, ng = K ? (NG ? NG : NX) : (self ? a.C : a.Cg);
    const int ky = K ? K : a.ky, kx = K ? K : a.kx;
    const int tw = K ? KMB_TW : a.tw, th = K ? KMB_TH : a.th;
    const int H = a.H, W = a.W, border = a.border;
    uint32_t bid = blockIdx.x;
    const uint32_t tbx = bid % a.tiles_x;
    bid /= a.tiles_x;
    const uint32_t tby = bid % a.tiles_y;
    const uint32_t b = bid / a.tiles_y;
    const int x0 = (int)tbx * tw, y0 = (int)tby * th;
    const int py = ky / 2, px = kx / 2, tww = tw + kx - 1, thh = th + ky - 1, pstride = tww * thh;
    const size_t plane = (size_t)H * W;

    // the tile: planes 0 .. nx - 1 the input, then (joint) the guidance; widened, border resolved
    const int planes = self ? nx : nx + ng;
    for (int pl = 0; pl < planes; ++pl) {
        const T* img = pl < nx ? a.x + ((size_t)b * a.C + pl) * plane : a.g + ((size_t)b * a.Cg + (pl - nx)) * plane;
        for (int t = (int)threadIdx.x; t < pstride; t += 256) {
            const int sy = kmb_map(y0 - py + t / tww, H, border), sx = kmb_map(x0 - px + t % tww, W, border);
            R v = (R)0;
            if (sy >= 0 && sx >= 0) v = (R)km_ld(img + (size_t)sy * W + sx);
            tile[pl * pstride + t] = v;
        }
    }
    __syncthreads();
    const int lx = (int)threadIdx.x % tw, ly = (int)threadIdx.x / tw;
    const int ox = x0 + lx, oy = y0 + ly;
    if (ly >= th || ox >= W || oy >= H) return;

    const bool l2 = a.dist == KMB_L2;
    const R c2 = kmb_fold(a.coef[a.Bc > 1 ? b : 0]);
    const R* sp = a.space + (size_t)(a.Bs > 1 ? b : 0) * (ky * kx);
    const R* gt = tile + (self ? 0 : nx * pstride);  // the guidance planes
    const int ctr = (ly + py) * tww + lx + px;
    R acc[MCX];
#pragma unroll
    for (int c = 0; c < MCX; ++c) acc[c] = (R)0;
    R wsum = (R)0;
    constexpr int UNR = K ? K : 1;  // the window's loops: fully unrolled when its side is compile-time
#pragma unroll UNR
    for (int p = 0; p < ky; ++p) {
#pragma unroll UNR
        for (int q = 0; q < kx; ++q) {
            const int nb = (ly + p) * tww + lx + q;
            R d = (R)0;
#pragma unroll
            for (int c = 0; c < MCG; ++c)
                if (c < ng) d = kmb_dist_add(gt[c * pstride + nb] - gt[c * pstride + ctr], l2, d);
            d = l2 ? d : d * d;
            const R k = sp[p * kx + q] * kmb_exp(c2 * d);
            wsum += k;
#pragma unroll
            for (int c = 0; c < MCX; ++c)
                if (c < nx) acc[c] = km_fma(k, tile[c * pstride + nb], acc[c]);
        }
    }
    const size_t o = (size_t)oy * W + ox;
    T* out = a.y + (size_t)b * a.C * plane + o;
#pragma unroll
    for (int c = 0; c < MCX; ++c)
        if (c < nx) km_st(out + c * plane, acc[c] / wsum);
    if (a.wsum != nullptr) km_st(a.wsum + (size_t)b * plane + o, wsum);
}

// ------------------------------------------------------------------------------------------------
template <typename T>
struct KmbBwdArgs {
    typedef typename KmTraits<T>::R R;
    const T *x, *g, *y, *gy;  // g null: self-guided
    const R* wsum;
    const R* space;
    const R* coef;
    T* gx;  // nullable (joint)
    T* gg;  // nullable; always null when self-guided (both gradients sum into gx)
    int C, Cg, H, W, ky, kx, border, dist, Bs, Bc;
    int lds_fits;  // the interior path's tiles fit KMB_LDS_BYTES
    uint32_t tiles_x, tiles_y;
};

// where the backward reads a sample's planes: global memory (border tiles) ...
template <typename T>
struct KmbGlobalSrc {
    typedef typename KmTraits<T>::R R;
    const T *x, *g, *y, *G;
    const R* w;
    size_t plane;
    int W;
    __device__ __forceinline__ R X(int c, int qy, int qx) const { return (R)km_ld(x + c * plane + (size_t)qy * W + qx); }
    __device__ __forceinline__ R Gd(int c, int qy, int qx) const { return (R)km_ld(g + c * plane + (size_t)qy * W + qx); }
    __device__ __forceinline__ R Y(int c, int qy, int qx) const { return (R)km_ld(y + c * plane + (size_t)qy * W + qx); }
    __device__ __forceinline__ R Go(int c, int qy, int qx) const { return (R)km_ld(G + c * plane + (size_t)qy * W + qx); }
    __device__ __forceinline__ R Ws(int qy, int qx) const { return w[(size_t)qy * W + qx]; }
};
// ... or the LDS tiles with halo (interior tiles): planes x | g (joint) | y | grad_out | wsum
template <typename R>
struct KmbLdsSrc {
    const R* t;
    int tww, pstride, ty0, tx0;  // the tile's row pitch, plane size, and the image coordinate of its first element
    int gb, yb, Gb, wb;          // first plane of g, y, grad_out, wsum (x: 0)
    __device__ __forceinline__ int at(int qy, int qx) const { return (qy - ty0) * tww + (qx - tx0); }
    __device__ __forceinline__ R X(int c, int qy, int qx) const { return t[c * pstride + at(qy, qx)]; }
    __device__ __forceinline__ R Gd(int c, int qy, int qx) const { return t[(gb + c) * pstride + at(qy, qx)]; }
    __device__ __forceinline__ R Y(int c, int qy, int qx) const { return t[(yb + c) * pstride + at(qy, qx)]; }
    __device__ __forceinline__ R Go(int c, int qy, int qx) const { return t[(Gb + c) * pstride + at(qy, qx)]; }
    __device__ __forceinline__ R Ws(int qy, int qx) const { return t[wb * pstride + at(qy, qx)]; }
};

struct KmbBwdCfg {
    int nx, ng, H, W, ky, kx, border;
    bool l2, do_val, do_w;
};

// Pixel p = (y, x) of an INTERIOR tile: every neighbour n = p + j is a pixel, p's only pre-image is p.  One exp per neighbour serves
//   A  p as the output pixel, tap j on n:         gg^c(p) -= coef k_A T_A dD^c(delta),   delta^c = g^c(n) - g^c(p), k_A = s_j e
//   B  n as the output pixel, tap -j on p:        gx^c(p) += k_B G^c_n / W_n,  gg^c(p) += coef k_B T_B dD^c(-delta),  k_B = s_(-j) e
template <typename R, int MC, typename Src>
__device__ __forceinline__ void kmb_bwd_interior(const Src& s, const KmbBwdCfg& f, const R* sp, R coef, int y, int x, R (&gxa)[MC], R (&gga)[MC]) {
    const int py = f.ky / 2, px = f.kx / 2;
    const R c2 = kmb_fold(coef);
    const R rwp = (R)1 / s.Ws(y, x);
    for (int jy = -py; jy <= py; ++jy)
        for (int jx = -px; jx <= px; ++jx) {
            const int ny = y + jy, nxp = x + jx;
            R d = (R)0;
#pragma unroll
            for (int c = 0; c < MC; ++c)
                if (c < f.ng) d = kmb_dist_add(s.Gd(c, ny, nxp) - s.Gd(c, y, x), f.l2, d);
            const R S = d;
            d = f.l2 ? d : d * d;
            const R e = kmb_exp(c2 * d);
            const R kA = sp[(jy + py) * f.kx + jx + px] * e, kB = sp[(py - jy) * f.kx + px - jx] * e;
            const R rwn = (R)1 / s.Ws(ny, nxp);
            R tA = (R)0, tB = (R)0;
#pragma unroll
            for (int c = 0; c < MC; ++c)
                if (c < f.nx) {
                    const R Gn = s.Go(c, ny, nxp);
                    if (f.do_val) gxa[c] = km_fma(kB * rwn, Gn, gxa[c]);
                    if (f.do_w) {
                        tA = km_fma(s.Go(c, y, x), s.X(c, ny, nxp) - s.Y(c, y, x), tA);
                        tB = km_fma(Gn, s.X(c, y, x) - s.Y(c, ny, nxp), tB);
                    }
                }
            if (f.do_w) {
                const R E = coef * (kA * (tA * rwp) + kB * (tB * rwn));
#pragma unroll
                for (int c = 0; c < MC; ++c)
                    if (c < f.ng) gga[c] -= E * kmb_ddist(s.Gd(c, ny, nxp) - s.Gd(c, y, x), f.l2, S);
            }
        }
}

// Pixel p = (y, x) of a tile at the border, the general form.
//   A  p as the output pixel: tap i reads r = map(p + i) (zeros outside a `constant` border); the derivative of D wrt g(p), the centre
//   B  p as a tap: every padded position p~ with map(p~) = p and every output pixel q = p~ - i inside the image, spatial weight s_i
template <typename R, int MC, typename Src>
__device__ __forceinline__ void kmb_bwd_border(const Src& s, const KmbBwdCfg& f, const R* sp, R coef, int y, int x, R (&gxa)[MC], R (&gga)[MC]) {
    const int py = f.ky / 2, px = f.kx / 2, H = f.H, W = f.W;
    const R c2 = kmb_fold(coef);
    if (f.do_w) {
        const R rwp = (R)1 / s.Ws(y, x);
        for (int iy = -py; iy <= py; ++iy)
            for (int ix = -px; ix <= px; ++ix) {
                const int ry = kmb_map(y + iy, H, f.border), rx = kmb_map(x + ix, W, f.border);
                const bool in = ry >= 0 && rx >= 0;
                R d = (R)0;
#pragma unroll
                for (int c = 0; c < MC; ++c)
                    if (c < f.ng) d = kmb_dist_add((in ? s.Gd(c, ry, rx) : (R)0) - s.Gd(c, y, x), f.l2, d);
                const R S = d;
                d = f.l2 ? d : d * d;
                const R k = sp[(iy + py) * f.kx + ix + px] * kmb_exp(c2 * d);
                R t = (R)0;
#pragma unroll
                for (int c = 0; c < MC; ++c)
                    if (c < f.nx) t = km_fma(s.Go(c, y, x), (in ? s.X(c, ry, rx) : (R)0) - s.Y(c, y, x), t);
                const R E = coef * (k * (t * rwp));
#pragma unroll
                for (int c = 0; c < MC; ++c)
                    if (c < f.ng) gga[c] -= E * kmb_ddist((in ? s.Gd(c, ry, rx) : (R)0) - s.Gd(c, y, x), f.l2, S);
            }
    }
    // candidates for p~ on an axis: the pixel itself (e = 0), the pad before the image (e < 0: coordinate e), the pad behind it (e > 0: n - 1 + e)
    for (int ey = -py; ey <= py; ++ey) {
        const int yt = ey < 0 ? ey : (ey == 0 ? y : H - 1 + ey);
        if (ey != 0 && kmb_map(yt, H, f.border) != y) continue;
        for (int ex = -px; ex <= px; ++ex) {
            const int xt = ex < 0 ? ex : (ex == 0 ? x : W - 1 + ex);
            if (ex != 0 && kmb_map(xt, W, f.border) != x) continue;
            for (int iy = -py; iy <= py; ++iy) {
                const int qy = yt - iy;
                if (qy < 0 || qy >= H) continue;
                for (int ix = -px; ix <= px; ++ix) {
                    const int qx = xt - ix;
                    if (qx < 0 || qx >= W) continue;
                    R d = (R)0;
#pragma unroll
                    for (int c = 0; c < MC; ++c)
                        if (c < f.ng) d = kmb_dist_add(s.Gd(c, y, x) - s.Gd(c, qy, qx), f.l2, d);
                    const R S = d;
                    d = f.l2 ? d : d * d;
                    const R k = sp[(iy + py) * f.kx + ix + px] * kmb_exp(c2 * d);
                    const R rwq = (R)1 / s.Ws(qy, qx);
                    R t = (R)0;
#pragma unroll
                    for (int c = 0; c < MC; ++c)
                        if (c < f.nx) {
                            const R Gq = s.Go(c, qy, qx);
                            if (f.do_val) gxa[c] = km_fma(k * rwq, Gq, gxa[c]);
                            if (f.do_w) t = km_fma(Gq, s.X(c, y, x) - s.Y(c, qy, qx), t);
                        }
                    if (f.do_w) {
                        const R E = coef * (k * (t * rwq));
#pragma unroll
                        for (int c = 0; c < MC; ++c)
                            if (c < f.ng) gga[c] += E * kmb_ddist(s.Gd(c, y, x) - s.Gd(c, qy, qx), f.l2, S);
                    }
                }
            }
        }
    }
}

template <typename T, int MC>
__global__ __launch_bounds__(256) void km_bilateral_bwd_kernel(const KmbBwdArgs<T> a) {
    typedef typename KmTraits<T>::R R;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];  // the interior path's planes (nothing when they do not fit)
    R* tile = (R*)smem_raw;
    uint32_t bid = blockIdx.x;
    const uint32_t tbx = bid % a.tiles_x;
    bid /= a.tiles_x;
    const uint32_t tby = bid % a.tiles_y;
    const uint32_t b = bid / a.tiles_y;
    const int H = a.H, W = a.W, ky = a.ky, kx = a.kx, py = ky / 2, px = kx / 2;
    const int x0 = (int)tbx * KMB_TW, y0 = (int)tby * KMB_TH;
    const int lx = (int)threadIdx.x % KMB_TW, ly = (int)threadIdx.x / KMB_TW;
    const int ox = x0 + lx, oy = y0 + ly;
    const size_t plane = (size_t)H * W;
    const bool self = a.g == nullptr;
    KmbBwdCfg f;
    f.nx = a.C; f.ng = self ? a.C : a.Cg; f.H = H; f.W = W; f.ky = ky; f.kx = kx; f.border = a.border;
    f.l2 = a.dist == KMB_L2;
    f.do_val = a.gx != nullptr;
    f.do_w = self || a.gg != nullptr;
    const R coef = a.coef[a.Bc > 1 ? b : 0];
    const R* sp = a.space + (size_t)(a.Bs > 1 ? b : 0) * (ky * kx);
    const T* xb = a.x + (size_t)b * a.C * plane;
    const T* gb = self ? xb : a.g + (size_t)b * a.Cg * plane;
    const T* yb = a.y + (size_t)b * a.C * plane;
    const T* Gb = a.gy + (size_t)b * a.C * plane;
    const R* wb = a.wsum + (size_t)b * plane;

    R gxa[MC], gga[MC];
#pragma unroll
    for (int c = 0; c < MC; ++c) gxa[c] = gga[c] = (R)0;

    // (block-uniform) interior: every pixel of the tile exists, its neighbourhood lies inside the image, and no padded position maps to it
    const bool interior = a.lds_fits && x0 - px >= 1 && x0 + KMB_TW - 1 + px <= W - 2 && y0 - py >= 1 && y0 + KMB_TH - 1 + py <= H - 2;
    if (interior) {
        const int tww = KMB_TW + kx - 1, thh = KMB_TH + ky - 1, pstride = tww * thh;
        KmbLdsSrc<R> s;
        s.t = tile; s.tww = tww; s.pstride = pstride; s.ty0 = y0 - py; s.tx0 = x0 - px;
        s.gb = self ? 0 : f.nx;
        s.yb = self ? f.nx : f.nx + f.ng;
        s.Gb = s.yb + f.nx;
        s.wb = s.Gb + f.nx;
        for (int pl = 0; pl <= s.wb; ++pl) {
            for (int t = (int)threadIdx.x; t < pstride; t += 256) {
                const size_t o = (size_t)(s.ty0 + t / tww) * W + (s.tx0 + t % tww);
                R v;
                if (pl == s.wb) v = wb[o];
                else if (pl >= s.Gb) v = (R)km_ld(Gb + (pl - s.Gb) * plane + o);
                else if (pl >= s.yb) v = (R)km_ld(yb + (pl - s.yb) * plane + o);
                else if (pl >= f.nx) v = (R)km_ld(gb + (pl - f.nx) * plane + o);
                else v = (R)km_ld(xb + pl * plane + o);
                tile[pl * pstride + t] = v;
            }
        }
        __syncthreads();
        kmb_bwd_interior<R, MC>(s, f, sp, coef, oy, ox, gxa, gga);
    } else {
        if (ox >= W || oy >= H) return;
        KmbGlobalSrc<T> s;
        s.x = xb; s.g = gb; s.y = yb; s.G = Gb; s.w = wb; s.plane = plane; s.W = W;
        kmb_bwd_border<R, MC>(s, f, sp, coef, oy, ox, gxa, gga);
    }
    const size_t o = (size_t)oy * W + ox;
    if (self) {
        T* out = a.gx + (size_t)b * a.C * plane + o;
#pragma unroll
        for (int c = 0; c < MC; ++c)
            if (c < f.nx) km_st(out + c * plane, gxa[c] + gga[c]);
    } else {
        if (a.gx != nullptr) {
            T* out = a.gx + (size_t)b * a.C * plane + o;
#pragma unroll
            for (int c = 0; c < MC; ++c)
                if (c < f.nx) km_st(out + c * plane, gxa[c]);
        }
        if (a.gg != nullptr) {
            T* out = a.gg + (size_t)b * a.Cg * plane + o;
#pragma unroll
            for (int c = 0; c < MC; ++c)
                if (c < f.ng) km_st(out + c * plane, gga[c]);
        }
    }
}

// ------------------------------------------------------------------------------------------------
template <typename T, int K, int NG, int NX>
static void kmb_launch_ct(const KmbFwdArgs<T>& a, uint32_t nb, hipStream_t s) {
    hipLaunchKernelGGL((km_bilateral_fwd_kernel<T, K, NG, NX, 1>), dim3(nb), dim3(256), 0, s, a);
}
template <typename T, int K, int NG>
static void kmb_launch_ct_nx(const KmbFwdArgs<T>& a, uint32_t nb, hipStream_t s) {
    switch (a.C) {
        case 1: kmb_launch_ct<T, K, NG, 1>(a, nb, s); break;
        case 2: kmb_launch_ct<T, K, NG, 2>(a, nb, s); break;
        case 3: kmb_launch_ct<T, K, NG, 3>(a, nb, s); break;
        default: kmb_launch_ct<T, K, NG, 4>(a, nb, s); break;
    }
}
template <typename T, int K>
static void kmb_launch_ct_ng(const KmbFwdArgs<T>& a, uint32_t nb, hipStream_t s) {
    switch (a.g ? a.Cg : 0) {
        case 0: kmb_launch_ct_nx<T, K, 0>(a, nb, s); break;
        case 1: kmb_launch_ct_nx<T, K, 1>(a, nb, s); break;
        case 2: kmb_launch_ct_nx<T, K, 2>(a, nb, s); break;
        case 3: kmb_launch_ct_nx<T, K, 3>(a, nb, s); break;
        default: kmb_launch_ct_nx<T, K, 4>(a, nb, s); break;
    }
}

template <typename T>
static int kmb_fwd(const void* x, const void* guide, const void* space, const void* coef, void* y, void* wsum, int B, int C, int Cg, int H, int W, int Bs, int Bc,
                   int ky, int kx, int border, int dist, hipStream_t s) {
    typedef typename KmTraits<T>::R R;
    KmbFwdArgs<T> a;
    a.x = (const T*)x; a.g = (const T*)guide; a.space = (const R*)space; a.coef = (const R*)coef; a.y = (T*)y; a.wsum = (R*)wsum;
    a.C = C; a.Cg = Cg; a.H = H; a.W = W; a.ky = ky; a.kx = kx; a.border = border; a.dist = dist; a.Bs = Bs; a.Bc = Bc;
    const int ng = guide ? Cg : 0;
    const bool ct = sizeof(R) == 4 && ky == kx && (ky == 3 || ky == 5 || ky == 7 || ky == 9) && C <= 4 && ng <= 4;
    a.tw = KMB_TW; a.th = KMB_TH;
    if (!ct) {  // shrink the tile (the wider side first) until all planes with their halo fit the LDS budget: 1 x 1 always does
        const size_t planes = (size_t)(C + ng);
        while ((size_t)(a.tw + kx - 1) * (a.th + ky - 1) * planes * sizeof(R) > KMB_LDS_BYTES) {
            if (a.tw > a.th) a.tw /= 2;
            else a.th /= 2;
        }
    }
    a.tiles_x = (uint32_t)((W + a.tw - 1) / a.tw);
    a.tiles_y = (uint32_t)((H + a.th - 1) / a.th);
    const uint64_t nb64 = (uint64_t)a.tiles_x * a.tiles_y * (uint64_t)B;
    KM_REQUIRE(nb64 < (1ull << 31), "km_bilateral_blur_fwd: grid too large");
    const uint32_t nb = (uint32_t)nb64;
    if constexpr (sizeof(R) == 4) {
        if (ct) {
            switch (ky) {
                case 3: kmb_launch_ct_ng<T, 3>(a, nb, s); break;
                case 5: kmb_launch_ct_ng<T, 5>(a, nb, s); break;
                case 7: kmb_launch_ct_ng<T, 7>(a, nb, s); break;
                default: kmb_launch_ct_ng<T, 9>(a, nb, s); break;
            }
            return km_check_launch("km_bilateral_blur_fwd");
        }
    }
    const size_t lds = (size_t)(a.tw + kx - 1) * (a.th + ky - 1) * (size_t)(C + ng) * sizeof(R);
    if (C <= 4 && (guide ? Cg : C) <= 4) hipLaunchKernelGGL((km_bilateral_fwd_kernel<T, 0, 0, 0, 4>), dim3(nb), dim3(256), lds, s, a);
    else hipLaunchKernelGGL((km_bilateral_fwd_kernel<T, 0, 0, 0, KMB_MAXC>), dim3(nb), dim3(256), lds, s, a);
    return km_check_launch("km_bilateral_blur_fwd(run-time)");
}

template <typename T>
static int kmb_bwd(const void* x, const void* guide, const void* space, const void* coef, const void* y, const void* wsum, const void* gy, void* gx, void* gguide,
                   int B, int C, int Cg, int H, int W, int Bs, int Bc, int ky, int kx, int border, int dist, hipStream_t s) {
    typedef typename KmTraits<T>::R R;
    KmbBwdArgs<T> a;
    a.x = (const T*)x; a.g = (const T*)guide; a.y = (const T*)y; a.gy = (const T*)gy; a.wsum = (const R*)wsum; a.space = (const R*)space; a.coef = (const R*)coef;
    a.gx = (T*)gx; a.gg = (T*)gguide;
    a.C = C; a.Cg = Cg; a.H = H; a.W = W; a.ky = ky; a.kx = kx; a.border = border; a.dist = dist; a.Bs = Bs; a.Bc = Bc;
    const size_t planes = (size_t)(3 * C + (guide ? Cg : 0) + 1);
    size_t lds = (size_t)(KMB_TW + kx - 1) * (KMB_TH + ky - 1) * planes * sizeof(R);
    a.lds_fits = lds <= KMB_LDS_BYTES ? 1 : 0;
    if (!a.lds_fits) lds = 0;
    a.tiles_x = (uint32_t)((W + KMB_TW - 1) / KMB_TW);
    a.tiles_y = (uint32_t)((H + KMB_TH - 1) / KMB_TH);
    const uint64_t nb64 = (uint64_t)a.tiles_x * a.tiles_y * (uint64_t)B;
    KM_REQUIRE(nb64 < (1ull << 31), "km_bilateral_blur_bwd: grid too large");
    const uint32_t nb = (uint32_t)nb64;
    if (C <= 4 && (guide ? Cg : C) <= 4) hipLaunchKernelGGL((km_bilateral_bwd_kernel<T, 4>), dim3(nb), dim3(256), lds, s, a);
    else hipLaunchKernelGGL((km_bilateral_bwd_kernel<T, KMB_MAXC>), dim3(nb), dim3(256), lds, s, a);
    return km_check_launch("km_bilateral_blur_bwd");
}

static int kmb_check(const char* who, const void* guide, int B, int C, int Cg, int H, int W, int Bs, int Bc, int ky, int kx, int border, int dist, int dtype) {
    KM_REQUIRE(ky >= 1 && kx >= 1 && (ky & 1) && (kx & 1) && ky <= KMB_MAXK && kx <= KMB_MAXK, "%s: the window must have odd sides of 1 .. %d, got (%d, %d)", who,
               KMB_MAXK, ky, kx);
    KM_REQUIRE(dtype >= KM_F32 && dtype <= KM_F16, "%s: bad dtype %d", who, dtype);
    KM_REQUIRE(border >= KMB_CONSTANT && border <= KMB_CIRCULAR, "%s: bad border code %d", who, border);
    KM_REQUIRE(dist == KMB_L1 || dist == KMB_L2, "%s: bad distance code %d", who, dist);
    KM_REQUIRE(B >= 0 && C >= 0 && H >= 0 && W >= 0 && (int64_t)H * W < (1ll << 31), "%s: bad shape B=%d C=%d H=%d W=%d", who, B, C, H, W);
    KM_REQUIRE(C <= KMB_MAXC && (guide == nullptr || (Cg >= 1 && Cg <= KMB_MAXC)), "%s: at most %d channels of input and of guidance, got %d and %d", who, KMB_MAXC, C,
               guide ? Cg : C);
    KM_REQUIRE((Bs == 1 || Bs == B) && (Bc == 1 || Bc == B), "%s: space has %d and coef %d samples, each must be 1 or B=%d", who, Bs, Bc, B);
    return 0;
}
static int kmb_check_pad(const char* who, int H, int W, int ky, int kx, int border) {
    KM_REQUIRE(border != KMB_REFLECT || (ky / 2 < H && kx / 2 < W), "%s: a reflect pad of (%d, %d) does not fit the %d x %d image", who, ky / 2, kx / 2, H, W);
    KM_REQUIRE(border != KMB_CIRCULAR || (ky / 2 <= H && kx / 2 <= W), "%s: a circular pad of (%d, %d) wraps the %d x %d image more than once", who, ky / 2, kx / 2, H, W);
    return 0;
}

extern "C" {

int km_bilateral_blur_fwd(const void* x, const void* guide, const void* space, const void* coef, void* y, void* wsum, int B, int C, int Cg, int H, int W, int Bs,
                          int Bc, int ky, int kx, int border, int dist, int dtype, void* stream) {
    const char* who = "km_bilateral_blur_fwd";
    if (kmb_check(who, guide, B, C, Cg, H, W, Bs, Bc, ky, kx, border, dist, dtype) != 0) return -1;
    if ((uint64_t)B * C * H * W == 0) return 0;
    if (kmb_check_pad(who, H, W, ky, kx, border) != 0) return -1;
    KM_REQUIRE(x && space && coef && y, "%s: null pointer", who);
    hipStream_t s = (hipStream_t)stream;
    return km_dispatch_dtype<float, double, km_bf16, km_f16>(dtype, -1, [&](auto t) { return kmb_fwd<KM_TAG_T(t)>(x, guide, space, coef, y, wsum, B, C, Cg, H, W, Bs, Bc, ky, kx, border, dist, s); });
}

int km_bilateral_blur_bwd(const void* x, const void* guide, const void* space, const void* coef, const void* y, const void* wsum, const void* gy, void* gx,
                          void* gguide, int B, int C, int Cg, int H, int W, int Bs, int Bc, int ky, int kx, int border, int dist, int dtype, void* stream) {
    const char* who = "km_bilateral_blur_bwd";
    if (kmb_check(who, guide, B, C, Cg, H, W, Bs, Bc, ky, kx, border, dist, dtype) != 0) return -1;
    if ((uint64_t)B * C * H * W == 0) return 0;
    if (kmb_check_pad(who, H, W, ky, kx, border) != 0) return -1;
    KM_REQUIRE(x && space && coef && y && wsum && gy, "%s: null pointer", who);
    KM_REQUIRE(guide ? (gx || gguide) : (gx && !gguide), "%s: self-guided takes gx alone, joint at least one of gx and gguide", who);
    hipStream_t s = (hipStream_t)stream;
    return km_dispatch_dtype<float, double, km_bf16, km_f16>(dtype, -1, [&](auto t) { return kmb_bwd<KM_TAG_T(t)>(x, guide, space, coef, y, wsum, gy, gx, gguide, B, C, Cg, H, W, Bs, Bc, ky, kx, border, dist, s); });
}

}  // extern "C"
