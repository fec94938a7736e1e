// kornia_amd - host side of the warp family: the record of one warp call, and every warp function that one .hip defines and
// another calls.  Both the defining and the calling file include this header, so the compiler compares the two.
#pragma once

#include "km_sampler.h"

// One warp call as its extern "C" entry point received it.  The entry point fills the record once, field by field; from there on
// the host code passes the record and nothing passes the sizes or the modes as a list of ints.
struct KmWarpCall {
    const void* src = nullptr;    // (B,C,H,W) image dtype
    const void* mat = nullptr;    // (B_M,9) compute dtype; KM_COORD_GRID: the grid again (what the null check looks at)
    void* dst = nullptr;          // fwd: (B,C,h,w)
    const void* gout = nullptr;   // bwd: (B,C,h,w)
    void* gsrc = nullptr;         // bwd: (B,C,H,W) compute dtype, nullable
    double* gmat = nullptr;       // bwd: (B_M,9), nullable
    const void* fill = nullptr;   // (C) compute dtype, pad == fill only
    const void* grid = nullptr;   // KM_COORD_GRID: (B_M,h,w,2) image dtype
    void* ggrid = nullptr;        // KM_COORD_GRID bwd: (B,h,w,2) compute dtype, nullable
    const void* apply = nullptr;  // fwd: (B) uint8 per-sample switch, nullable
    int B = 0, C = 0, H = 0, W = 0, h = 0, w = 0, B_M = 0;
    int coord_mode = 0, norm_coords = 0, interp = 0, pad = 0, align = 0, dtype = 0;
    hipStream_t stream = nullptr;
};

template <typename T>
struct KmWarpArgs;
template <typename T>
struct KmWarpGmArgs;

template <typename R>
static inline void km_geom_init(KmWarpGeom<R>& g, const KmWarpCall& c) {
    km_geom_init(g, c.B, c.C, c.H, c.W, c.h, c.w, c.B_M, c.coord_mode, c.norm_coords, c.interp, c.pad, c.align);
}

// 32-bit byte offsets inside a plane of the source and of the output: what every specialised warp kernel needs
static inline bool km_warp_planes_fit_u32(const KmWarpCall& c) {
    return (uint64_t)c.H * (uint64_t)c.W * 4 < (1ull << 32) && (uint64_t)c.h * (uint64_t)c.w * 4 < (1ull << 32);
}

// km_warp.hip: the forward of km_warp2d_fwd / km_warp2d_fwd_masked (`fn`: the name in the messages), checks included
int km_warp_fwd_call(const char* fn, const KmWarpCall& c);

// km_warp_cubic.hip: the LDS-staged bicubic forward; launches and returns 1 when it takes the case, 0 otherwise
int km_warp_fwd_cubic_try_any(const KmWarpArgs<float>& a, int coord_mode, hipStream_t s);
int km_warp_fwd_cubic_try_any(const KmWarpArgs<km_bf16>& a, int coord_mode, hipStream_t s);
int km_warp_fwd_cubic_try_any(const KmWarpArgs<km_f16>& a, int coord_mode, hipStream_t s);

// km_warp_bwd_tiled.hip: owner-computes grad_src for bilinear + zeros / fill
int km_warp_bwd_tiled_supported(const KmWarpCall& c);
int km_warp_bwd_tiled_dims_ok(const KmWarpCall& c);
int km_warp_bwd_tiled_run(const KmWarpCall& c);

// km_warp_gm.hip: the matrix gradient of the bilinear warps; km_warp_gm_box.hip: its box form (1 when it took the case)
int km_warp_gm_supported(const KmWarpCall& c);
int km_warp_gm_run(const KmWarpCall& c);
int km_warp_gm_box_try(const KmWarpGmArgs<float>& a, int coord_mode, hipStream_t s);

// km_warp_bwd_fused.hip: both gradients from one read of grad_out
int km_warp_bwd_fused_supported(const KmWarpCall& c);
size_t km_warp_bwd_fused_workspace(const KmWarpCall& c);
int km_warp_bwd_fused_run(const KmWarpCall& c, void* ws);
