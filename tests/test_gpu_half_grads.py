"""GPU: the 16-bit (bf16 / f16) BACKWARD of the native ops against the fp32 path on the same values and against fp64 references.

Contract (forward: test_gpu_warp.py::test_16_bit_storage_is_the_fp32_result_rounded_once):
  1. Warps: the image gradient is accumulated in the compute dtype and cast once (imgwarp.py `_warp2d_backward`), so where both dtypes take a
     deterministic owner path it is the fp32 path's gradient rounded to the storage dtype, bit for bit; where either takes the fp32 atomics
     (border / reflection / bicubic / nearest in 16-bit, warp_bwd_generic) it is within 1 ulp of the storage dtype at each entry.  The matrix
     gradient is an fp64 sum of fp32 products in both dtypes.
  2. The separable filter's adjoint is the reference's autograd of filter2d(filter2d(x, kx), ky): the column pass's adjoint first, held in
     the storage dtype, then the row pass's adjoint, rounded - with the taps rounded to the storage dtype (filter2d casts the kernel).
  3. Against the plain-C oracle in fp64 on the rounded values: within 1 ulp of the storage dtype plus the fixed-point term of the fp32 tests.
Also runs on the host build of the kernels (tests/test_emulated_half_grads.py); cases ending in `_at_full_size` run on the device only."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from _util import flagship_homographies

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
DT_ID = {torch.bfloat16: "bf16", torch.float16: "f16"}


def _lib():
    from kornia_amd import _native as N

    return N.lib()


def _with_config(cfg, fn):
    """fn() under km_config_set(key, value) for each item of cfg; the previous values are restored in a finally (test_gpu_warp_fused._run)"""
    lib = _lib()
    prev = []
    try:
        for k, v in cfg.items():
            prev.append((k, lib.km_config_set(k.encode(), v)))
        return fn()
    finally:
        for k, v in reversed(prev):
            lib.km_config_set(k.encode(), v)


def _ulp(ref, dt):
    """spacing of dt at |ref| (ref in fp64); subnormal spacing below the smallest normal"""
    fi = torch.finfo(dt)
    a = ref.double().abs().clamp_min(fi.tiny)
    return torch.pow(2.0, torch.floor(torch.log2(a))) * fi.eps


def _same(a, b):
    """bit-for-bit equal, NaN where the other is NaN (torch.equal says no to any NaN)"""
    a, b = a.cpu(), b.cpu()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    nan = a.isnan()
    return bool(torch.equal(nan, b.isnan()) and torch.equal(a[~nan], b[~nan]))


def _within_ulps(a, ref, dt, n=1.0, atol=0.0):
    """max over the entries of |a - ref| / (n ulp(dt, |ref|) + atol) - <= 1 passes; non-finite entries must match exactly"""
    a, ref = a.double().cpu(), ref.double().cpu()
    fin = torch.isfinite(ref)
    assert torch.equal(fin, torch.isfinite(a)), "non-finite pattern differs"
    assert torch.equal(a[~fin].nan_to_num(), ref[~fin].nan_to_num()) and torch.equal(a[~fin].isnan(), ref[~fin].isnan()), "non-finite values differ"
    if not fin.any():
        return 0.0
    return ((a - ref).abs()[fin] / (n * _ulp(ref[fin], dt) + atol)).max().item()


def _rel(a, b):
    """max over the matrices of max|a - b| / max|b| (fp64)"""
    a, b = a.double().reshape(a.shape[0], -1).cpu(), b.double().reshape(b.shape[0], -1).cpu()
    return ((a - b).abs().amax(1) / b.abs().amax(1).clamp_min(1e-300)).max().item()


# =================================================================================================
# warps
# =================================================================================================
# policies of the warp backward: km_config_set keys (km_runtime.hip), each also exercised by the fp32 path it is compared with
POLICIES = {
    "default": {},
    "tiled": {"warp_bwd_fused": 0},                       # image gradient through the tile-owner kernel, matrix gradient through km_warp_gm
    "generic": {"warp_bwd_generic": 1},                   # the fp32-atomic scatter
    "gm_box": {"warp_bwd_fused": 0, "warp_gm_algo": 0},   # matrix gradient: box form (fp32 only) or rows / gather in 16-bit
    "gm_generic": {"warp_bwd_fused": 0, "warp_gm_algo": 1},
    "gm_rows": {"warp_bwd_fused": 0, "warp_gm_algo": 2},
}


def _warp_op(fn, dsize, mode="bilinear", pad="zeros", align=True, fill=None):
    import kornia_amd as K

    if fn == "persp":
        return lambda a, m: K.warp_perspective(a, m, dsize, mode, pad, align, None if fill is None else fill.cuda())
    if fn == "affine":
        return lambda a, m: K.warp_affine(a, m, dsize, mode, pad, align, None if fill is None else fill.cuda())
    return lambda a, m: K.homography_warp(a, m, dsize, mode, pad, align)


def _oracle_bwd(oracle, fn, go, x, M, dsize, mode="bilinear", pad="zeros", align=True, fill=None):
    if fn == "persp":
        return oracle.warp_perspective_backward(go, x, M, dsize, mode, pad, align, fill)
    if fn == "affine":
        return oracle.warp_affine_backward(go, x, M, dsize, mode, pad, align, fill)
    return oracle.homography_warp_backward(go, x, M, dsize, mode, pad, align)


def _grads(op, x, M, go, cfg, need=("x", "M")):
    """(grad_x, grad_M) through the public autograd API under the policy cfg; a gradient not asked for is None"""
    def run():
        xg = x.cuda().detach().requires_grad_("x" in need)  # (detach: a leaf that keeps a view's storage offset)
        Mg = M.cuda().requires_grad_("M" in need)
        op(xg, Mg).backward(go.cuda())
        return (None if xg.grad is None else xg.grad.cpu()), (None if Mg.grad is None else Mg.grad.cpu())

    return _with_config(cfg, run)


def _matrices(fn, B, H, W, h, w, g, shared=False):
    Bm = 1 if shared else B
    if fn == "homog":
        M = torch.eye(3).repeat(Bm, 1, 1) + 0.03 * torch.randn(Bm, 3, 3, generator=g)
        M[:, 2, 2] = 1.0
        return M
    M = flagship_homographies(Bm, H, W, h, w, g, jitter=5.0)
    return M[:, :2, :].contiguous() if fn == "affine" else M


# (B, C, H, W, h, w): W % 8 == 4, odd W, W % 8 == 0, C over 1..5, ragged right / bottom tiles, several 64 x 64 owner tiles a side
SHAPES = [(2, 3, 70, 132, 66, 132), (1, 1, 66, 129, 70, 131), (2, 5, 64, 64, 64, 64), (1, 2, 130, 136, 97, 140), (2, 4, 45, 67, 51, 88)]

# bound of the matrix gradient against the fp32 path, relative to the largest entry of each matrix: both are fp64 sums of the same fp32
# products (same positions, same values); only the order of the fp64 sums differs between the two dtypes' kernels.  Asserted at 1e-6, the
# range the host build shows; paths that differ between the dtypes (border / reflection in 16-bit) use the fp32 tests' 5e-5.
GM_VS_FP32 = 1e-6


# Tiles whose source pixels collect too many output pixels accumulate in IEEE float LDS atomics instead of fixed point (km_warp_tile.h:
# mult = (2 ex + 1)(2 ey + 1) output pixels per source pixel, fixed point while the tile's mult <= 256; km_warp_bwd_fused.hip kmo_pix).
# Their sums depend on the order the waves add in - the fp32 path differs from itself under another wave order on the host build - so no
# dtype is bit-identical to another there: they get the bound of the atomics paths.  The tile's mult bounds the pointwise one from above,
# so cases whose pointwise maximum passes half the limit count as such.
FLOAT_TILE_MULT = 128.0


def _output_pixels_per_source_pixel(fn, M, H, W, h, w):
    """the pointwise maximum of (2 |dj/ds| + 1.2)(2 |di/ds| + 1.2) over the output pixels that sample the image (inf: a vanishing line)"""
    M = M.double()
    if M.shape[-2] == 2:
        M = torch.cat([M, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand(M.shape[0], 1, 3)], 1)
    if fn == "homog":  # dst -> src in normalised coordinates
        def D(n_h, n_w):
            return torch.tensor([[2.0 / max(n_w - 1, 1), 0, -1], [0, 2.0 / max(n_h - 1, 1), -1], [0, 0, 1]], dtype=torch.float64)
        inv = torch.linalg.inv(D(H, W)) @ M @ D(h, w)
    else:
        inv = torch.linalg.inv(M)
    i, j = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    q = torch.einsum("bkl,hwl->bhwk", inv, torch.stack([j, i, torch.ones_like(i)], -1))
    z = q[..., 2]
    if (z <= 1e-6).any():
        return float("inf")
    sx, sy = q[..., 0] / z, q[..., 1] / z
    a, b = sx[:, :-1, 1:] - sx[:, :-1, :-1], sx[:, 1:, :-1] - sx[:, :-1, :-1]
    c, d = sy[:, :-1, 1:] - sy[:, :-1, :-1], sy[:, 1:, :-1] - sy[:, :-1, :-1]
    det = (a * d - b * c).abs()
    inside = (sx[:, :-1, :-1] > -2) & (sx[:, :-1, :-1] < W + 1) & (sy[:, :-1, :-1] > -2) & (sy[:, :-1, :-1] < H + 1)
    mult = (2 * (d.abs() + b.abs()) / det + 1.2) * (2 * (c.abs() + a.abs()) / det + 1.2)
    return mult[inside].max().item() if inside.any() else 0.0


def _check_warp(oracle, fn, dt, x, M, go, dsize, cfg, need=("x", "M"), mode="bilinear", pad="zeros", align=True, fill=None, tag=""):
    x16, go16 = x.to(dt), go.to(dt)  # (a 16-bit view passed in stays that view, device storage offset included)
    op = _warp_op(fn, dsize, mode, pad, align, fill)
    gx16, gM16 = _grads(op, x16, M, go16, cfg, need)
    gx32, gM32 = _grads(op, x16.float(), M, go16.float(), cfg, need)
    owner = mode == "bilinear" and pad in ("zeros", "fill") and not cfg.get("warp_bwd_generic", 0)
    owner = owner and _output_pixels_per_source_pixel(fn, M, x.shape[-2], x.shape[-1], *dsize) <= FLOAT_TILE_MULT
    shared = M.shape[0] == 1 and x.shape[0] > 1  # (the oracle takes one matrix per sample)
    Mo = M.expand(x.shape[0], -1, -1).contiguous() if shared else M
    if "x" in need:
        assert gx16.dtype == dt
        if owner:  # contract 1: both dtypes on the fixed-point owner paths
            assert _same(gx16, gx32.to(dt)), f"{tag}: grad_x differs from the fp32 path rounded once ({(gx16.float() - gx32).abs().max().item():.3e})"
        else:  # fp32 atomics on either side (or float LDS accumulators): 1 ulp of dt, plus the fp32 atomics' order term the fp32 tests allow relative to the largest
            # entry (2e-5: test_gpu_warp_fused.py::test_border_and_reflection_padding_through_the_tile_owners - border cells sum many pixels)
            fin = torch.isfinite(gx32)
            atol = 2e-5 * max(1.0, gx32[fin].abs().max().item()) if fin.any() else 0.0
            assert _within_ulps(gx16, gx32, dt, atol=atol) <= 1.0, f"{tag}: grad_x more than 1 ulp from the fp32 path"
        if torch.isfinite(go16.cpu()).all():
            # contract 3 against the oracle on the rounded values, in fp32: it shares the kernel's fp32 sampling positions (fp64 positions
            # move the bilinear weights by ~1e-7, which minification multiplies past an ulp).  1 ulp of dt plus the fp32 sweep's terms
            # (test_gpu_fuzz.py::test_extended_sweep_of_the_warps_at_tile_scale: 2e-5 x scale, 1e-5 relative); off the owner paths the
            # atomics' term relative to the largest entry, as above.
            gxo, _ = _oracle_bwd(oracle, fn, go16.cpu().float(), x16.cpu().float(), Mo, dsize, mode, pad, align, fill)
            scale = max(1.0, go16.cpu().float().abs().max().item()) * max(1.0, 4.0 * dsize[0] * dsize[1] / (x.shape[-2] * x.shape[-1]))
            atol = 2e-5 * scale if owner else 2e-5 * max(scale, gxo.abs().max().item())
            d = (gx16.double() - gxo.double()).abs()
            ok = d <= _ulp(gxo, dt) + atol + 1e-5 * gxo.double().abs()
            assert bool(ok.all()), f"{tag}: grad_x vs the fp32 oracle, max |d| {d.max().item():.3e}"
    if "M" in need:
        assert gM16.dtype == M.dtype
        if torch.isfinite(go16.cpu()).all():
            # (off the owner paths the two dtypes take different kernels: the fp32 tests' bound between two backward forms, 5e-5)
            gm_bound = GM_VS_FP32 if owner else 5e-5
            assert _rel(gM16, gM32) <= gm_bound, f"{tag}: grad_M vs the fp32 path rel {_rel(gM16, gM32):.2e}"
            # the fp32 oracle on the rounded values shares the kernel's fp32 sampling positions: the fp32 tests' 5e-5 (test_gpu_warp_fused.py)
            # (border / reflection: 2e-4, test_border_and_reflection_padding_through_the_tile_owners)
            _, gMo = _oracle_bwd(oracle, fn, go16.cpu().float(), x16.cpu().float(), Mo, dsize, mode, pad, align, fill)
            if shared:
                gMo = gMo.sum(0, keepdim=True)
            bound = 2e-4 if pad in ("border", "reflection") else 5e-5
            assert _rel(gM16, gMo) <= bound, f"{tag}: grad_M vs the fp32 oracle rel {_rel(gM16, gMo):.2e}"
    return gx16, gM16


@pytest.mark.parametrize("policy", list(POLICIES))
@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("fn", ["persp", "affine", "homog"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_warp_gradients_are_the_fp32_path_rounded_once(oracle, dt, fn, align, policy):
    """Both gradients of the three warps in 16-bit against the fp32 path on the same values, under every backward policy, and against the
    oracle; the shape rotates through SHAPES with the parameters."""
    i = (list(POLICIES).index(policy) + 2 * ["persp", "affine", "homog"].index(fn) + int(align)) % len(SHAPES)
    B, C, H, W, h, w = SHAPES[i]
    g = torch.Generator().manual_seed(100 + i)
    x = torch.rand(B, C, H, W, generator=g)
    go = torch.rand(B, C, h, w, generator=g) - 0.4
    M = _matrices(fn, B, H, W, h, w, g)
    _check_warp(oracle, fn, dt, x, M, go, (h, w), POLICIES[policy], align=align, tag=f"{fn} {SHAPES[i]} {policy}")


@pytest.mark.parametrize("need", [("x",), ("M",)])
@pytest.mark.parametrize("policy", ["default", "tiled"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_warp_each_gradient_alone(oracle, dt, policy, need):
    """Image gradient alone (the tiled kernel) and matrix gradient alone (the matrix-gradient kernels)."""
    B, C, H, W, h, w = 2, 3, 70, 132, 66, 132
    g = torch.Generator().manual_seed(7)
    x = torch.rand(B, C, H, W, generator=g)
    go = torch.rand(B, C, h, w, generator=g) - 0.4
    for align in (True, False):
        M = _matrices("persp", B, H, W, h, w, g)
        _check_warp(oracle, "persp", dt, x, M, go, (h, w), POLICIES[policy], need=need, align=align, tag=f"{need} align={align}")


@pytest.mark.parametrize("offset", [1, 2, 4])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_warp_image_at_an_unaligned_base(oracle, dt, offset):
    """Contiguous device views whose storage starts 1, 2 or 4 elements into the allocation (2 to 8 bytes: never 16-byte aligned)."""
    B, C, H, W, h, w = 2, 3, 66, 132, 70, 128
    g = torch.Generator().manual_seed(offset)

    def shifted(t):
        v = torch.empty(t.numel() + offset, dtype=dt, device="cuda")[offset:].view(t.shape)
        v.copy_(t.to(dt).cuda())
        assert v.is_contiguous() and v.storage_offset() == offset
        return v

    x16 = shifted(torch.rand(B, C, H, W, generator=g))
    go16 = shifted(torch.rand(B, C, h, w, generator=g) - 0.4)
    M = _matrices("persp", B, H, W, h, w, g)
    for policy in ("default", "tiled"):
        _check_warp(oracle, "persp", dt, x16, M, go16, (h, w), POLICIES[policy], tag=f"offset {offset} {policy}")


def _general_launch_matrix(case, B, H, W, h, w, g):
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    if case == "minify":  # ~2.2x minification
        s = 2.2
        A = torch.tensor([[s, 0.0, cx - s * (w - 1) / 2.0], [0.0, s, cy - s * (h - 1) / 2.0], [0.0, 0.0, 1.0]])
        return torch.linalg.inv(A).repeat(B, 1, 1)
    if case == "magnify":
        s = 0.4
        A = torch.tensor([[s, 0.0, cx - s * (w - 1) / 2.0], [0.0, s, cy - s * (h - 1) / 2.0], [0.0, 0.0, 1.0]])
        return torch.linalg.inv(A).repeat(B, 1, 1)
    if case == "vanishing":  # dst -> src maps a line inside the output to infinity
        Minv = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, -1.6 / h, 1.0]])
        return torch.linalg.inv(Minv).repeat(B, 1, 1)
    deg, s = {"rot20": (20.0, 1.0), "rot45": (45.0, 1.0), "rot45_scaled": (45.0, 1.35)}[case]
    c_, s_ = s * math.cos(math.radians(deg)), s * math.sin(math.radians(deg))
    A = torch.tensor([[c_, s_, (1 - c_) * cx - s_ * cy], [-s_, c_, s_ * cx + (1 - c_) * cy], [0.0, 0.0, 1.0]])
    return A.repeat(B, 1, 1)


@pytest.mark.parametrize("case", ["minify", "magnify", "vanishing", "rot20", "rot45", "rot45_scaled"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_warp_general_launch_tiles(oracle, dt, case):
    """Tiles of the general launch: minification, magnification, a vanishing line inside the image, boxes walked in several passes."""
    B, C, H, W, h, w = 1, 3, 96, 132, 100, 120
    g = torch.Generator().manual_seed(3)
    x = torch.rand(B, C, H, W, generator=g)
    go = torch.rand(B, C, h, w, generator=g) - 0.4
    M = _general_launch_matrix(case, B, H, W, h, w, g)
    for policy in ("default", "tiled"):
        _check_warp(oracle, "persp", dt, x, M, go, (h, w), POLICIES[policy], tag=f"{case} {policy}")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_warp_shared_matrix(oracle, dt):
    """One matrix for the whole batch (warp_affine's (1,2,3); warp_perspective refuses it as the reference does): its gradient sums over
    the samples."""
    B, C, H, W, h, w = 3, 2, 70, 132, 66, 129
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, C, H, W, generator=g)
    go = torch.rand(B, C, h, w, generator=g) - 0.4
    M = _matrices("affine", B, H, W, h, w, g, shared=True)
    for policy in ("default", "tiled", "gm_rows"):
        _check_warp(oracle, "affine", dt, x, M, go, (h, w), POLICIES[policy], tag=f"shared {policy}")


@pytest.mark.parametrize("mode,pad", [("bilinear", "fill"), ("bilinear", "border"), ("bilinear", "reflection"), ("bicubic", "zeros"),
                                      ("nearest", "zeros")])
@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_warp_padding_and_interpolation_modes(oracle, dt, align, mode, pad):
    """fill (C = 3), border and reflection padding, bicubic and nearest: in 16-bit all but fill leave the owner paths for the generic
    fp32-atomic backward, so the image gradient is held to 1 ulp of the fp32 path."""
    B, C, H, W, h, w = 2, 3, 66, 100, 70, 96
    g = torch.Generator().manual_seed(11)
    x = torch.rand(B, C, H, W, generator=g)
    go = torch.rand(B, C, h, w, generator=g) - 0.4
    M = flagship_homographies(B, H, W, h, w, g, jitter=10.0)
    fill = torch.tensor([0.2, 0.5, 0.7]) if pad == "fill" else None
    need = ("x", "M") if mode == "bilinear" else ("x",)  # (the matrix gradient is bilinear-only, as in the reference's grid_sample)
    _check_warp(oracle, "persp", dt, x, M, go, (h, w), {}, need=need, mode=mode, pad=pad, align=align, fill=fill, tag=f"{mode} {pad}")


def _magnify(B, H, W, h, w):
    s = 0.3
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    A = torch.tensor([[s, 0.0, cx - s * (w - 1) / 2.0], [0.0, s, cy - s * (h - 1) / 2.0], [0.0, 0.0, 1.0]])
    return torch.linalg.inv(A).repeat(B, 1, 1)


@pytest.mark.parametrize("scale", [1e-30, 1e30])
def test_warp_bf16_gradient_range_sets_the_fixed_point_scale(oracle, scale):
    """bf16 grad_out far from 1: the owner paths' fixed-point scale comes from each tile's values, so the result is still the fp32 path's
    rounded once."""
    B, C, H, W, h, w = 2, 3, 70, 132, 66, 132
    g = torch.Generator().manual_seed(13)
    x = torch.rand(B, C, H, W, generator=g)
    go = (torch.rand(B, C, h, w, generator=g) - 0.4) * scale
    M = _matrices("persp", B, H, W, h, w, g)
    for policy in ("default", "tiled"):
        gx, gM = _check_warp(oracle, "persp", torch.bfloat16, x, M, go, (h, w), POLICIES[policy], tag=f"scale {scale} {policy}")
        assert torch.isfinite(gx).all() and (gx != 0).any() and torch.isfinite(gM).all()


def test_warp_f16_overflow_where_the_fp32_sum_overflows(oracle):
    """f16 grad_out near 6e4 under 3.3x magnification: the fp32 sums reach ~10x that, and inf must appear exactly where fp32.to(f16)
    overflows - no earlier (a 16-bit accumulator) and no later."""
    B, C, H, W, h, w = 1, 3, 40, 64, 120, 128
    g = torch.Generator().manual_seed(17)
    x = torch.rand(B, C, H, W, generator=g)
    go = 5e4 + 1.5e4 * torch.rand(B, C, h, w, generator=g)
    go[..., : w // 2] *= 1e-2  # (the left half stays finite)
    M = _magnify(B, H, W, h, w)
    for policy in ("default", "tiled", "generic"):
        op = _warp_op("persp", (h, w))
        go16 = go.to(torch.float16)
        gx16, _ = _grads(op, x.half(), M, go16, POLICIES[policy], ("x",))
        gx32, _ = _grads(op, x.half().float(), M, go16.float(), POLICIES[policy], ("x",))
        ref = gx32.to(torch.float16)
        assert torch.isinf(ref).any() and torch.isfinite(ref).any()
        assert torch.equal(torch.isinf(gx16), torch.isinf(ref)), policy
        if policy == "generic":
            assert _within_ulps(gx16, gx32.to(torch.float16).float(), torch.float16) <= 1.0
        else:
            assert _same(gx16, ref), policy


def test_warp_f16_subnormal_gradient(oracle):
    """f16 subnormal grad_out (|g| < 6.1e-5): sums that stay subnormal keep their bits."""
    B, C, H, W, h, w = 2, 3, 66, 100, 70, 96
    g = torch.Generator().manual_seed(19)
    x = torch.rand(B, C, H, W, generator=g)
    go = (torch.rand(B, C, h, w, generator=g) - 0.4) * 3e-6
    M = _matrices("persp", B, H, W, h, w, g)
    assert (go.half().abs() < torch.finfo(torch.float16).tiny).all() and (go.half() != 0).any()
    for policy in ("default", "tiled", "generic"):
        _check_warp(oracle, "persp", torch.float16, x, M, go, (h, w), POLICIES[policy], tag=f"subnormal {policy}")


@pytest.mark.parametrize("where", ["visited", "unvisited"])
@pytest.mark.parametrize("value", [float("nan"), float("inf")])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_warp_non_finite_gradient_pattern_is_the_fp32_paths(oracle, dt, value, where):
    """NaN / inf in grad_out at a pixel that samples the image and at one that maps outside it (found by the scan of unvisited pixels):
    the 16-bit gradients carry the fp32 path's NaN / inf pattern, entry for entry."""
    B, C, H, W, h, w = 1, 3, 64, 96, 70, 100
    g = torch.Generator().manual_seed(23)
    x = torch.rand(B, C, H, W, generator=g)
    go = torch.rand(B, C, h, w, generator=g) - 0.4
    M = torch.tensor([[[1.0, 0.0, 12.0], [0.0, 1.0, 9.0], [0.0, 0.0, 1.0]]])  # src = dst - (12, 9): the top-left corner of dst maps outside
    if where == "visited":
        go[0, 1, 40, 50] = value
    else:
        go[0, 1, 2, 3] = value
    for policy in ("default", "tiled", "generic"):
        op = _warp_op("persp", (h, w))
        gx16, gM16 = _grads(op, x.to(dt), M, go.to(dt), POLICIES[policy])
        gx32, gM32 = _grads(op, x.to(dt).float(), M, go.to(dt).float(), POLICIES[policy])
        tag = f"{where} {value} {policy}"
        assert torch.equal(gx16.isnan(), gx32.to(dt).isnan()) and torch.equal(gx16.isinf(), gx32.to(dt).isinf()), tag
        assert torch.equal(gM16.isnan(), gM32.isnan()) and torch.equal(gM16.isinf(), gM32.isinf()), tag
        fin = torch.isfinite(gx32)
        if policy == "generic":
            assert _within_ulps(gx16[fin], gx32[fin], dt) <= 1.0, tag
        else:
            assert torch.equal(gx16[fin], gx32.to(dt)[fin]), tag


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_warp_many_tiles_at_full_size(oracle, dt):
    """More 64 x 64 owner tiles than persistent workers (a 1024 x 1024 image, 8 samples: 2 048 tiles)."""
    B, C, H, W, h, w = 8, 3, 1024, 1024, 1024, 1024
    g = torch.Generator().manual_seed(29)
    x = torch.rand(B, C, H, W, generator=g)
    go = torch.rand(B, C, h, w, generator=g) - 0.4
    M = flagship_homographies(B, H, W, h, w, g, jitter=8.0)
    for policy in ("default", "tiled"):
        _check_warp(oracle, "persp", dt, x, M, go, (h, w), POLICIES[policy], tag=f"full size {policy}")


# =================================================================================================
# filters
# =================================================================================================
_PAD = {"constant": "constant", "reflect": "reflect", "replicate": "replicate", "circular": "circular"}


def _conv_same(t, k, border):
    """filter2d's forward in fp64 autograd terms: pad (the reference's F.pad) then correlate; t (B,C,H,W), k (Bk,kH,kW)"""
    kH, kW = k.shape[-2:]
    pads = [(kW - 1) // 2, kW - 1 - (kW - 1) // 2, (kH - 1) // 2, kH - 1 - (kH - 1) // 2]
    out = []
    for b in range(t.shape[0]):
        tb = t[b:b + 1].transpose(0, 1)
        out.append(F.conv2d(F.pad(tb, pads, mode=_PAD[border]), k[b % k.shape[0]][None, None]).transpose(0, 1))
    return torch.cat(out)


def _adjoint(go, k, border):
    """the gradient wrt the input of _conv_same, in fp64"""
    t = torch.zeros(go.shape, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(_conv_same(t, k.double(), border), t, go.double())[0]


def _sep_reference(go16, kx, ky, border, dt):
    """the reference's autograd of filter2d(filter2d(x, kx), ky) on 16-bit tensors, in fp64 with its roundings: taps rounded to dt (already
    in kx, ky), the column pass's adjoint first, rounded to dt, then the row pass's adjoint, rounded to dt"""
    g1 = _adjoint(go16, ky.double()[:, :, None], border).to(dt)
    return _adjoint(g1, kx.double()[:, None, :], border).to(dt)


# The kernels sum the fp32 products of 16-bit values in fp32 (as the reference's own 16-bit convolutions do), so an fp32 sum can fall on the
# other side of a rounding boundary of the storage dtype than the fp64 sum: 1 ulp, at up to 6.7e-4 of the entries (f16, filter2d 5 x 5
# circular; the separable adjoint up to 4.5e-4) on the host build over the cases below, so 1e-3.  bf16 leaves 16 more bits between the two
# roundings: the separable adjoint is bit-identical there; filter2d's 24-tap kernels reach 1.2e-4 of the entries.  (The issue's first look saw 28-97 % of the f16 entries differ from every composition it tried, on
# the LDS kernel too; rebuilt here - taps rounded to f16, column adjoint first, fp64 in between - the LDS kernel matches at all but these
# boundary cases, so that observation was a gap of the experiment, not of the kernel.)
DOUBLE_ROUNDING_FRACTION = 1e-3


def _assert_composition(got, ref, dt, tag, exact_bf16=True, fraction=DOUBLE_ROUNDING_FRACTION):
    if dt == torch.bfloat16 and exact_bf16:
        assert _same(got, ref), f"{tag}: {(got != ref).float().mean().item():.2e} of the entries differ from the reference's roundings"
    else:
        # (a flipped rounding of the intermediate reaches the result through the taps: plus 1 ulp at the largest entry)
        atol = _ulp(ref.double().abs().max(), dt).item()
        assert _within_ulps(got, ref.float(), dt, atol=atol) <= 1.0, f"{tag}: more than 1 ulp from the reference's roundings"
        frac = (got != ref).float().mean().item()
        if fraction is not None:
            assert frac <= fraction, f"{tag}: {frac:.2e} of the entries differ from the reference's roundings"


def _sep_case(dt, shape, K, Bk, seed):
    g = torch.Generator().manual_seed(seed)
    B = shape[0]
    go = (torch.rand(shape, generator=g) - 0.4).to(dt)
    kx = torch.rand(Bk if Bk == 1 else B, K, generator=g).to(dt).float()
    ky = torch.rand(Bk if Bk == 1 else B, K, generator=g).to(dt).float()
    return go, kx, ky


def _sep_grad(x16, kx, ky, border, go16, cfg=None):
    import kornia_amd as K_

    def run():
        xg = x16.cuda().requires_grad_()
        K_.filters.filter2d_separable(xg, kx.cuda(), ky.cuda(), border).backward(go16.cuda())
        return xg.grad.cpu()

    return _with_config(cfg or {}, run)


@pytest.mark.parametrize("Bk", [1, "B"])
@pytest.mark.parametrize("K", [3, 5, 7, 9, 11])
@pytest.mark.parametrize("W", [64, 45])
@pytest.mark.parametrize("border", ["constant", "reflect", "replicate", "circular"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_separable_adjoint_rounds_where_the_reference_does(dt, border, W, K, Bk):
    """filter2d_separable's adjoint: W % 4 == 0 and K <= 9 take the register-tiled kernel (16-bit circular: the LDS kernel), W % 4 != 0 the
    LDS kernel, K = 11 the large-kernel form - all against the reference's autograd structure with its roundings."""
    shape = (2, 2, 37, W)
    go16, kx, ky = _sep_case(dt, shape, K, Bk, seed=K * 10 + W)
    x16 = torch.rand(shape).to(dt)
    got = _sep_grad(x16, kx, ky, border, go16)
    _assert_composition(got, _sep_reference(go16, kx, ky, border, dt), dt, f"{border} K={K} W={W} Bk={Bk}")


@pytest.mark.parametrize("cfg", [{"blur_rows": 8}, {"blur_rows": 16}, {"blur_rows": 32}, {"sep_lds": 1}], ids=["rows8", "rows16", "rows32", "sep_lds"])
@pytest.mark.parametrize("border", ["reflect", "constant"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_separable_adjoint_every_kernel_form(dt, border, cfg):
    """The three strip heights of the register-tiled adjoint and the LDS kernel forced on a W % 4 == 0 image: the same roundings."""
    shape = (2, 3, 70, 72)
    go16, kx, ky = _sep_case(dt, shape, 5, "B", seed=31)
    got = _sep_grad(torch.rand(shape).to(dt), kx, ky, border, go16, cfg)
    _assert_composition(got, _sep_reference(go16, kx, ky, border, dt), dt, f"{border} {cfg}")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_gaussian_blur_adjoint_at_full_size(dt):
    """BASELINE config 3's blur (256 x 3 x 224^2, 5 x 5, sigma 1.5, reflect) on a slice of its batch."""
    import kornia_amd as K_

    shape = (16, 3, 224, 224)
    g = torch.Generator().manual_seed(37)
    go16 = (torch.rand(shape, generator=g) - 0.4).to(dt)
    xg = torch.rand(shape, generator=g).to(dt).cuda().requires_grad_()
    K_.gaussian_blur2d(xg, (5, 5), (1.5, 1.5)).backward(go16.cuda())
    from kornia_amd.filters.gaussian import _cached_taps

    kx, ky = (k.cpu().reshape(1, 5).to(dt).float() for k in _cached_taps(5, 5, (1.5, 1.5), dt, torch.device("cpu")))  # (the taps the op used)
    _assert_composition(xg.grad.cpu(), _sep_reference(go16, kx, ky, "reflect", dt), dt, "config 3 blur")


@pytest.mark.parametrize("kshape", [(3, 3), (5, 5), (4, 6)])
@pytest.mark.parametrize("W", [64, 45])
@pytest.mark.parametrize("border", ["constant", "reflect", "replicate", "circular"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_filter2d_input_and_kernel_gradient(dt, border, W, kshape):
    """filter2d: the input gradient is the single adjoint with the kernel rounded to dt, rounded once.  The kernel gradient sums products of
    two 16-bit values (exact in fp32) in fp64 accumulators, so before its casts it is the fp64 reference rounded to fp32; then, as in the
    reference, it leaves through the kernel's cast to the input dtype (filter2d casts the kernel): fp64 -> fp32 -> dt -> fp32, bit for bit."""
    import kornia_amd as K_

    B, C, H = 2, 2, 33
    g = torch.Generator().manual_seed(W + kshape[0] * 7)
    x16 = torch.rand(B, C, H, W, generator=g).to(dt)
    go16 = (torch.rand(B, C, H, W, generator=g) - 0.4).to(dt)
    for Bk in (1, B):
        k = torch.rand(Bk, *kshape, generator=g)
        xg, kg = x16.cuda().requires_grad_(), k.cuda().requires_grad_()
        K_.filters.filter2d(xg, kg, border).backward(go16.cuda())
        k16 = k.to(dt)
        ref = _adjoint(go16, k16, border).to(dt)
        _assert_composition(xg.grad.cpu(), ref, dt, f"filter2d input {border} {kshape} W={W} Bk={Bk}", exact_bf16=kshape[0] * kshape[1] <= 9)
        # kernel gradient: d/dk of sum(go * conv(x, k)) in fp64 on the rounded values; the reference sums the batch into one kernel when Bk = 1
        kk = k16.double().requires_grad_()
        (kref,) = torch.autograd.grad(_conv_same(x16.double(), kk, border), kk, go16.double())
        gk = kg.grad.cpu()
        assert gk.dtype == torch.float32
        assert _same(gk, kref.float().to(dt).float()), f"kernel gradient {border} {kshape} Bk={Bk}: {(gk.double() - kref).abs().max().item():.3e}"


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_spatial_gradient_adjoint(oracle, dt, order, generic):
    """spatial_gradient's adjoint (register-tiled and sg_generic): the reference's autograd of its replicate-padded convolution, with the
    normalised kernels rounded to dt (order 2 divides by 64: not exact in 16-bit), summed over the outputs in fp64 and rounded once."""
    import kornia_amd as K_

    g = torch.Generator().manual_seed(41 + order)
    kern = oracle.spatial_gradient_kernel2d("sobel", order, torch.float64)
    kern = (kern / kern.abs().sum((-2, -1), keepdim=True)).to(dt)
    for W in (64, 45):
        x16 = torch.rand(2, 3, 36, W, generator=g).to(dt)
        go16 = (torch.rand(2, 3, kern.shape[0], 36, W, generator=g) - 0.4).to(dt)

        def run():
            xg = x16.cuda().requires_grad_()
            K_.spatial_gradient(xg, "sobel", order).backward(go16.cuda())
            return xg.grad.cpu()

        got = _with_config({"sg_generic": generic}, run)
        ref = sum(_adjoint(go16[:, :, j], kern[j:j + 1], "replicate") for j in range(kern.shape[0])).to(dt)
        _assert_composition(got, ref, dt, f"order {order} W={W} generic={generic}", exact_bf16=False)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_warp_perspective_blur_backward_is_the_two_ops(dt):
    """warp_perspective_blur's backward is the blur adjoint and the warp backward: bit-identical to the two ops composed in the same dtype."""
    from kornia_amd.geometry.transform.warp_blur import warp_perspective_blur

    import kornia_amd as K_

    B, C, H, W, h, w = 2, 3, 70, 96, 64, 88
    g = torch.Generator().manual_seed(43)
    x16 = torch.rand(B, C, H, W, generator=g).to(dt)
    go16 = (torch.rand(B, C, h, w, generator=g) - 0.4).to(dt)
    M = flagship_homographies(B, H, W, h, w, g, jitter=5.0)
    a, Ma = x16.cuda().requires_grad_(), M.cuda().requires_grad_()
    warp_perspective_blur(a, Ma, (h, w), (5, 5), (1.5, 1.5)).backward(go16.cuda())
    b, Mb = x16.cuda().requires_grad_(), M.cuda().requires_grad_()
    K_.gaussian_blur2d(K_.warp_perspective(b, Mb, (h, w)), (5, 5), (1.5, 1.5)).backward(go16.cuda())
    assert _same(a.grad, b.grad) and _same(Ma.grad, Mb.grad)


# =================================================================================================
# grid_sample, resize
# =================================================================================================
@pytest.mark.parametrize("pad", ["zeros", "border", "reflection"])
@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_grid_sample_gradients(dt, align, pad):
    """Both gradients of grid_sample: the image gradient accumulates in fp32 (atomics: 1 ulp of dt of the fp32 path); the grid gradient is
    computed per output pixel in fp32 from the same values and cast to the grid dtype: the fp32 path's, rounded once."""
    import kornia_amd as K_

    B, C, H, W, h, w = 2, 3, 40, 52, 33, 47
    g = torch.Generator().manual_seed(47)
    x16 = torch.rand(B, C, H, W, generator=g).to(dt)
    grid16 = (torch.rand(B, h, w, 2, generator=g) * 2.4 - 1.2).to(dt)
    go16 = (torch.rand(B, C, h, w, generator=g) - 0.4).to(dt)

    def run(x, grid, go):
        xg, gg = x.cuda().requires_grad_(), grid.cuda().requires_grad_()
        K_.geometry.transform.grid_sample(xg, gg, "bilinear", pad, align).backward(go.cuda())
        return xg.grad.cpu(), gg.grad.cpu()

    gx16, gg16 = run(x16, grid16, go16)
    gx32, gg32 = run(x16.float(), grid16.float(), go16.float())
    assert gx16.dtype == dt and gg16.dtype == dt
    assert _within_ulps(gx16, gx32, dt) <= 1.0
    assert _same(gg16, gg32.to(dt))


@pytest.mark.parametrize("size", [(23, 71), (68, 90)])
@pytest.mark.parametrize("W", [64, 45])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_resize_bilinear_adjoint(dt, W, size):
    """resize_bilinear (down and up) on a random grad_out: one adjoint accumulated in fp32 and cast once, so within 1 ulp of dt of the
    fp32 path on the same values."""
    import kornia_amd as K_

    fn = lambda a: K_.geometry.transform.resize_bilinear(a, size)
    g = torch.Generator().manual_seed(59 + W)
    x16 = torch.rand(2, 3, 34, W, generator=g).to(dt)

    def run(x, go=None):
        xg = x.cuda().requires_grad_()
        y = fn(xg)
        if go is None:
            go = (torch.rand(y.shape, generator=g) - 0.4).to(x.dtype)
        y.backward(go.cuda())
        return xg.grad.cpu(), go

    g16, go16 = run(x16)
    g32, _ = run(x16.float(), go16.float())
    assert g16.dtype == dt
    assert _within_ulps(g16, g32, dt) <= 1.0


def _resize_adjoint(go, size, align):
    """gradient wrt the input (of spatial size `size`) of F.interpolate(bilinear) to go's size, in fp64"""
    t = torch.zeros(*go.shape[:2], *size, dtype=torch.float64, requires_grad=True)
    y = F.interpolate(t, size=tuple(go.shape[-2:]), mode="bilinear", align_corners=align)
    return torch.autograd.grad(y, t, go.double())[0]


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("op", ["pyrdown", "pyrup"])
@pytest.mark.parametrize("W", [64, 45])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_pyramid_adjoints_round_where_the_reference_does(oracle, dt, W, op, align):
    """pyrdown = 5x5 Gaussian filter2d (reflect), then bilinear resize; pyrup = resize, then the filter - each step's result held in the
    storage dtype.  The adjoints on a random grad_out against the fp64 rebuild of that autograd: the last step's adjoint first, rounded to
    dt, then the first step's, rounded (the fp32-accumulation rule of _assert_composition)."""
    import kornia_amd as K_

    T = K_.geometry.transform
    g = torch.Generator().manual_seed(61 + W)
    H = 34
    x16 = torch.rand(2, 3, H, W, generator=g).to(dt)
    xg = x16.cuda().requires_grad_()
    y = (T.pyrdown if op == "pyrdown" else T.pyrup)(xg, "reflect", align)
    go16 = (torch.rand(y.shape, generator=g) - 0.4).to(dt)
    y.backward(go16.cuda())
    k = oracle.pyramid_kernel(torch.float64).reshape(1, 5, 5).to(dt)
    if op == "pyrdown":
        ref = _adjoint(_resize_adjoint(go16, (H, W), align).to(dt), k, "reflect").to(dt)
    else:
        ref = _resize_adjoint(_adjoint(go16, k, "reflect").to(dt), (H, W), align).to(dt)
    # (open: odd widths and align_corners=True differ from this rounding order at up to 5e-2 of the entries on the host build - each
    # within the bound - so the pyramid adjoints are held to the per-entry bound only)
    _assert_composition(xg.grad.cpu(), ref, dt, f"{op} W={W} align={align}", exact_bf16=False, fraction=None)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_remap_gradients(dt):
    """remap: with normalised maps its gradients are grid_sample's (image: 1 ulp of the fp32 path; maps: the fp32 path's grid gradient
    rounded once); with pixel maps, the maps' gradients pass through the normalisation's autograd in dt, exactly as grid_sample on the
    grid normalize_pixel_coordinates builds."""
    import kornia_amd as K_
    from kornia_amd.geometry.conversions import normalize_pixel_coordinates

    T = K_.geometry.transform
    B, C, H, W = 2, 3, 36, 44
    g = torch.Generator().manual_seed(53)
    x16 = torch.rand(B, C, H, W, generator=g).to(dt)
    go16 = (torch.rand(B, C, H, W, generator=g) - 0.4).to(dt)
    nx = (torch.rand(B, H, W, generator=g) * 2.4 - 1.2).to(dt)
    ny = (torch.rand(B, H, W, generator=g) * 2.4 - 1.2).to(dt)

    def run(x, a, b, go, normalized):
        xg, ag, bg = (t.cuda().requires_grad_() for t in (x, a, b))
        T.remap(xg, ag, bg, "bilinear", "zeros", align_corners=True, normalized_coordinates=normalized).backward(go.cuda())
        return xg.grad.cpu(), ag.grad.cpu(), bg.grad.cpu()

    r16 = run(x16, nx, ny, go16, True)
    r32 = run(x16.float(), nx.float(), ny.float(), go16.float(), True)
    assert _within_ulps(r16[0], r32[0], dt) <= 1.0
    assert _same(r16[1], r32[1].to(dt)) and _same(r16[2], r32[2].to(dt))
    # pixel maps
    px = ((nx.float() + 1) * (W - 1) / 2).to(dt)
    py = ((ny.float() + 1) * (H - 1) / 2).to(dt)
    got = run(x16, px, py, go16, False)
    xg, ag, bg = (t.cuda().requires_grad_() for t in (x16, px, py))
    grid = normalize_pixel_coordinates(torch.stack([ag, bg], -1), H, W).to(dt)
    T.grid_sample(xg, grid, "bilinear", "zeros", True).backward(go16.cuda())
    assert _within_ulps(got[0], xg.grad.cpu(), dt) <= 1.0
    assert _same(got[1], ag.grad.cpu()) and _same(got[2], bg.grad.cpu())


@pytest.mark.parametrize("shape", [(2, 3, 16, 24), (2, 3, 7, 9), (3, 3, 33, 40)])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_color_jitter_backward_is_the_fp32_kernel_rounded_once(dt, shape):
    """color_jitter's backward in 16-bit against the fp32 kernel on the same rounded image and gradient: within 1 ulp of dt at every
    entry (the vector path and, for a plane size that is not a multiple of four, the scalar one)."""
    import kornia_amd as K_

    g = torch.Generator().manual_seed(shape[-1])
    B = shape[0]
    x16 = torch.rand(shape, generator=g).to(dt)
    w16 = torch.randn(shape, generator=g).to(dt)
    f = [0.8 + 0.4 * torch.rand(B, generator=g) for _ in range(3)] + [(torch.rand(B, generator=g) - 0.5) * 0.2]
    res = []
    for x, w in ((x16, w16), (x16.float(), w16.float())):
        xq = x.cuda().requires_grad_()
        K_.enhance.color_jitter(xq, *[t.cuda() for t in f], [0, 2, 3, 1]).backward(w.cuda())
        res.append(xq.grad.cpu())
    assert res[0].dtype == dt
    assert _within_ulps(res[0], res[1], dt) <= 1.0, f"max {_within_ulps(res[0], res[1], dt):.2f} ulp"


# =================================================================================================
# the 16-bit gradient leg of the warp sweep
# =================================================================================================
def test_extended_sweep_16_bit_gradients(oracle):
    """test_gpu_fuzz.py's extended warp sweep, 16-bit leg: each case's image and grad_out rounded to bf16 (odd seeds) or f16 (even), both
    gradients against the fp32 path and the oracle under contract 1 (_check_warp: bit for bit on the fixed-point owner tiles).
    KM_FUZZ_SECONDS / KM_FUZZ_SEED bound and pick the run as there; every failure names the seed that rebuilds its case
    (`_sweep_case(seed, True)`)."""
    import time

    from test_gpu_fuzz import _sweep_case

    big = "KM_FUZZ_SECONDS" in os.environ
    budget = float(os.environ.get("KM_FUZZ_SECONDS", "4"))
    seed0 = int(os.environ.get("KM_FUZZ_SEED", "0"))
    t_end = time.time() + budget
    failures, n, n_float = [], 0, 0
    while time.time() < t_end or n < 3:
        seed = seed0 * 100000 + n
        n += 1
        c = _sweep_case(seed, big)
        dt = torch.bfloat16 if seed % 2 else torch.float16
        (h, w) = c["dsize"]
        n_float += _output_pixels_per_source_pixel(c["fn"], c["M"], *c["x"].shape[-2:], h, w) > FLOAT_TILE_MULT
        case = f"seed={seed} {DT_ID[dt]} fn={c['fn']} kind={c['kind']} x={tuple(c['x'].shape)} -> {(h, w)} pad={c['pad']} align={c['align']}"
        try:
            _check_warp(oracle, c["fn"], dt, c["x"], c["M"], c["go"] - 0.4, (h, w), {}, pad=c["pad"], align=c["align"], fill=c["fill"], tag=case)
        except AssertionError as e:
            failures.append(str(e).split("\n")[0])
    print(f"16-bit gradient sweep: {n} cases ({n_float} with float-accumulator tiles) in {budget:.0f} s budget, {len(failures)} failures")
    assert not failures, "\n".join(failures[:20])


@pytest.mark.parametrize("seed,big", [(3051, True), (569, True), (1724, True), (732, False)])
def test_sweep_cases_with_float_accumulator_tiles(oracle, seed, big):
    """Sweep cases (`_sweep_case(seed, big)`) whose 16-bit image gradient differed from the rounded fp32 path on the device: magnified
    tiles past the fixed-point limit, which accumulate in float LDS atomics in both dtypes.  They are classified so, and hold the atomics
    bound (_check_warp)."""
    from test_gpu_fuzz import _sweep_case

    c = _sweep_case(seed, big)
    dt = torch.bfloat16 if seed % 2 else torch.float16
    assert _output_pixels_per_source_pixel(c["fn"], c["M"], *c["x"].shape[-2:], *c["dsize"]) > FLOAT_TILE_MULT
    _check_warp(oracle, c["fn"], dt, c["x"], c["M"], c["go"] - 0.4, c["dsize"], {}, pad=c["pad"], align=c["align"], fill=c["fill"], tag=f"seed={seed}")
