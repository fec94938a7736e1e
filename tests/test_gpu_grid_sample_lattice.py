"""GPU (and, through tests/test_emulated_grid_sample_lattice.py, the host build of the kernels): the explicit-grid sampler (km_grid_sample2d_fwd /
_bwd: grid_sample, remap, the cached grid of HomographyWarper) where the CALLER puts every coordinate - exactly on an integer, a rounding tie,
the -1 / +1 edge, a clip boundary, a reflection fold, several image widths away, at NaN / inf - which a matrix-made field and the
`rand * 2.4 - 1.2` grids of tests/test_gpu_grid_sample.py never do.

The reference is ATen's CPU ``F.grid_sample`` (the sampler the reference library calls) on identical inputs in the same dtype, live for finite
grids.  For grids that hold NaN / inf it is the recorded forward of tests/golden/nonfinite_grid.npz (tests/make_golden_nonfinite_grid.py):
ATen's own CPU backward reads out of bounds on such a grid under border / reflection and takes the process down, so NO test here calls ATen's
backward on a non-finite grid; the native backward is held to being the adjoint of the native forward instead.

Bounds (none was tuned on the kernels' results):
  * bilinear / nearest forward: ``torch.equal``; bicubic forward: 5e-7 for images in [0, 1) (test_gpu_grid_sample.py's fixture bound);
  * fp32 gradients: the rtol / atol of test_gpu_grid_sample.py::test_grid_sample_vs_oracle (image 1e-5 / 1e-5, grid 1e-4 / 1e-4) with the
    absolute part relative to the largest entry of the reference tensor (border padding piles many taps onto one source pixel);
  * fp64: 1e-12 of the largest entry;
  * 16-bit: the contract of tests/test_gpu_half_grads.py, restated at the tests below."""
import functools

import pytest
import torch
import torch.nn.functional as F

from _util import golden
from make_golden_nonfinite_grid import MODES, PADS, SOURCES as NF_SOURCES, VALUES as NF_VALUES, inputs as nf_inputs, key as nf_key
from test_gpu_half_grads import _same, _ulp, _within_ulps
from test_gpu_median import unaligned

pytestmark = pytest.mark.gpu
nan, inf = float("nan"), float("inf")
B = 2
SRCS = [(1, 1), (1, 6), (6, 1), (2, 2), (3, 2), (5, 7), (8, 4)]  # H x W; 8 x 4: the normalised lattice is exact in bf16 / f16
FDT = {"f32": torch.float32, "f64": torch.float64}
HDT = {"bf16": torch.bfloat16, "f16": torch.float16}
SID = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


# =================================================================================================
# the lattice
# =================================================================================================
def pixel_list(n):
    """coordinates in PIXELS along an axis of n cells: every integer and nearest-rounding tie around both edges, both clip boundaries (0, n - 1),
    both reflection folds of each align_corners (0 / n - 1 and -0.5 / n - 0.5), points in the first, second and third reflected copy"""
    return [-3, -1.5, -1, -0.5, -0.25, 0, 0.25, 0.5, 1, 1.5, 2.5, n - 2, n - 1.5, n - 1, n - 0.5, n, n + 0.5, n + 1, 2 * n - 1, 2 * n - 0.5,
            3 * n + 0.3, -2 * n - 0.7]


def normalise(p, n, align):
    """pixel -> normalised coordinate (the inverse of ATen's unnormalize), in fp64.  n == 1 with align_corners: every coordinate is pixel 0 (the
    unnormalise scale is 0) - the pixel value itself is used, so the grid still holds values of every size"""
    p = torch.as_tensor(p, dtype=torch.float64)
    if align:
        return p.clone() if n == 1 else 2 * p / (n - 1) - 1
    return (2 * p + 1) / n - 1


def lattice_axis(n, align, dt, nudged):
    """the axis' normalised coordinates in dt: the pixel list (and -0.0), or every point of it one ulp of dt above and below"""
    g = torch.cat([normalise(pixel_list(n), n, align), torch.tensor([-0.0], dtype=torch.float64)]).to(dt)
    if not nudged:
        return g
    up, dn = torch.full_like(g, inf), torch.full_like(g, -inf)
    return torch.cat([torch.nextafter(g, up), torch.nextafter(g, dn)])


@functools.lru_cache(maxsize=None)
def case(src, dn, align, nudged):
    """(image (B,5,H,W) in [0, 1), grid (B,n+33,65,2), grad_out (B,5,n+33,65), n): the lattice - outer product of the two axes' lists - in the
    upper left n x n corner of a grid of random coordinates in [-1.3, 1.3), whose last 33 x 65 block makes the launch cross an output tile's
    edge in both directions (tiles are 64 x 16) with a ragged last tile.  Cached: built once, shared by the tests, never written to."""
    H, W = src
    dt = {**FDT, **HDT}[dn]
    g = torch.Generator().manual_seed(1000 * H + 10 * W + int(align))
    lx, ly = lattice_axis(W, align, dt, nudged), lattice_axis(H, align, dt, nudged)
    n = lx.numel()
    h, w = n + 33, 65
    x = torch.rand(B, 5, H, W, generator=g, dtype=torch.float64).to(dt)
    grid = (torch.rand(B, h, w, 2, generator=g, dtype=torch.float64) * 2.6 - 1.3).to(dt)
    gy, gx = torch.meshgrid(ly, lx, indexing="ij")
    grid[:, :n, :n, 0] = gx
    grid[:, :n, :n, 1] = gy
    go = (torch.rand(B, 5, h, w, generator=g, dtype=torch.float64) - 0.4).to(dt)
    return x, grid, go, n


def native(x, grid, go, mode, pad, align, need=(True, True)):
    """(y, grad_x, grad_grid) of the native op, on the host"""
    import kornia_amd as K

    xg, gg = x.cuda().requires_grad_(need[0]), grid.cuda().requires_grad_(need[1])
    y = K.grid_sample(xg, gg, mode, pad, align)
    y.backward(go.cuda())
    return y.detach().cpu(), None if xg.grad is None else xg.grad.cpu(), None if gg.grad is None else gg.grad.cpu()


def aten(x, grid, go, mode, pad, align):
    """the same of ATen's CPU sampler; a (1,h,w,2) grid is expanded as autograd would (its gradient is the sum over the batch).  FINITE grids only."""
    assert torch.isfinite(grid).all()
    xr, gr = x.clone().requires_grad_(), grid.clone().requires_grad_()
    y = F.grid_sample(xr, gr.expand(x.shape[0], -1, -1, -1), mode, pad, align)
    y.backward(go)
    return y.detach(), xr.grad, gr.grad


def off_by(got, ref, rtol, atol, more=0.0):
    """max of |got - ref| / (atol * max|ref| + rtol * |ref| + more): <= 1 passes (0 / 0 counts as 0)"""
    got, ref = got.double(), ref.double()
    tol = atol * ref.abs().max() + rtol * ref.abs() + more
    d = (got - ref).abs()
    return torch.where(d == 0, torch.zeros_like(d), d / tol).max().item()


GRAD_TOL = {"f32": ((1e-5, 1e-5), (1e-4, 1e-4)), "f64": ((0.0, 1e-12), (0.0, 1e-12))}  # (rtol, atol) of the image / the grid gradient


@pytest.mark.parametrize("align", [False, True], ids=["ac0", "ac1"])
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dn", list(FDT))
@pytest.mark.parametrize("src", SRCS, ids=SID)
def test_lattice_matches_aten(src, dn, mode, pad, align):
    """Both lattices (exact: C in {1, 3, 5}, a grid per sample and one shared by the batch; one ulp either side of every point: two of those
    pairings): forward and both gradients against ATen's CPU sampler; the grid gradient of nearest is exactly zero.

    MEASURED (fp32 only; the rule: where the bound above does not hold, ATen in fp32 is measured against ATen in fp64 on that very case and 4x
    that error is allowed on top - two correct fp32 orderings can each be that far from the truth in opposite directions).  The cases that
    take it are those whose gradient is a sum that cancels to (nearly) nothing, so that "relative to the largest entry" is relative to noise:
    see MEASURED below the test.  A case that takes it prints its figures."""
    for nudged in (False, True):
        x, grid, go, n = case(src, dn, align, nudged)
        for C, B_G in (((1, B), (1, 1), (3, B), (3, 1), (5, B), (5, 1)) if not nudged else ((3, B), (1, 1))):
            tag = f"nudged={nudged} C={C} B_G={B_G}"
            xc, gc, goc = x[:, :C].contiguous(), grid[:B_G].contiguous(), go[:, :C].contiguous()
            y, gx, gg = native(xc, gc, goc, mode, pad, align)
            yr, gxr, ggr = aten(xc, gc, goc, mode, pad, align)
            if mode != "bicubic":
                assert torch.equal(y, yr), (tag, (y - yr).abs().max().item(), (y != yr).nonzero()[:4].tolist())
            else:
                assert (y - yr).abs().max().item() <= (5e-7 if dn == "f32" else 1e-12 * yr.abs().max().item()), tag
            (rx, ax), (rg, ag) = GRAD_TOL[dn]
            assert gx.shape == gxr.shape and gg.shape == ggr.shape == gc.shape and gx.dtype == gg.dtype == x.dtype
            more = [0.0, 0.0]
            if dn == "f64":
                # (1e-12 "of the largest entry" presumes the largest entry is not itself rounding noise: on a 1 x 1 source under border / reflection
                # every tap is the one pixel and the bicubic grid gradient - pixel x (derivative coefficients, which sum to 0) - cancels to ~1e-17
                # in both samplers.  The scale is therefore at least ONE TERM of that sum: unnormalise scale x largest pixel x largest grad_out.)
                more[1] = 1e-12 * (max(src) / 2) * xc.abs().max().item() * goc.abs().max().item()  # (max(src) / 2: the larger axis' scale)
            if dn == "f32" and (off_by(gx, gxr, rx, ax) > 1.0 or off_by(gg, ggr, rg, ag) > 1.0):
                _, gx64, gg64 = aten(xc.double(), gc.double(), goc.double(), mode, pad, align)
                more = [4 * (gxr.double() - gx64).abs().max().item(), 4 * (ggr.double() - gg64).abs().max().item()]
                print(f"MEASURED {SID(src)} {mode} {pad} ac{int(align)} {tag}: ATen fp32 - fp64 grad_x {more[0] / 4:.3e} grad_grid {more[1] / 4:.3e};"
                      f" native - ATen fp32 grad_x {(gx - gxr).abs().max().item():.3e} grad_grid {(gg - ggr).abs().max().item():.3e}")
            assert off_by(gx, gxr, rx, ax, more[0]) <= 1.0, (tag, "grad_x", off_by(gx, gxr, rx, ax, more[0]))
            assert off_by(gg, ggr, rg, ag, more[1]) <= 1.0, (tag, "grad_grid", off_by(gg, ggr, rg, ag, more[1]))
            if mode == "nearest":
                assert (gg == 0).all(), tag


# MEASURED on the host build of the kernels (tests/test_emulated_grid_sample_lattice.py, the only run so far that took the measured bound):
# the 1 x 1 source, bicubic, border and reflection, align_corners=False, every (C, B_G) - 16 runs.  Every tap is the one pixel, so the grid
# gradient is pixel x (the derivative coefficients, which sum to 0): entries of ~1e-8 that are all rounding.  ATen fp32 against ATen fp64:
# grid gradient 1.7e-07 .. 1.5e-06 (image gradient 4.2e-04 .. 4.9e-03 on sums of ~5e3); native against ATen fp32: grid gradient 4.6e-08 ..
# 1.6e-07 - inside 1x the measured error, 4x is allowed.  (The image gradient met its ordinary bound in all of them.)


# =================================================================================================
# kinks: the grid gradient's sign and zero pattern, stated directly
# =================================================================================================
def _expected_sign(p, n, pad, align):
    """sign of d(sampling position) / d(coordinate) at pixel position p of an axis of n cells, or None within 0.2 px of a kink
    (clip boundaries 0 and n - 1; folds 0 / n - 1 with align_corners, -0.5 / n - 0.5 without)"""
    if pad == "zeros":
        return 1
    if pad == "border":
        if min(abs(p), abs(p - (n - 1))) < 0.2:
            return None
        return 1 if 0 < p < n - 1 else 0
    lo, span = (0.0, float(n - 1)) if align else (-0.5, float(n))
    if span == 0:
        return 0
    t = (p - lo) % (2 * span)
    if min(t, abs(t - span), 2 * span - t) < 0.2:
        return None
    s, q = (1, t + lo) if t < span else (-1, 2 * span - t + lo)  # q: the reflected position, then clipped to [0, n - 1]
    if min(abs(q), abs(q - (n - 1))) < 0.2:
        return None
    return s if 0 < q < n - 1 else 0


@pytest.mark.parametrize("align", [False, True], ids=["ac0", "ac1"])
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("dn", list(FDT))
@pytest.mark.parametrize("src", SRCS, ids=SID)
def test_grid_gradient_sign_and_zero_pattern_at_the_kinks(src, dn, pad, align):
    """Without ATen.  The image is the ramp x + 8 y and grad_out is 1, so the bilinear grid gradient of a pixel is (sx W', 8 sy H') with W', H' the
    unnormalise scales (positive) and sx, sy in {+1, 0, -1}: 0 where the position is clipped (border; reflection's clamp), -1 on a mirrored
    stretch - the sign flips across a fold -, +1 otherwise.  Asserted at every lattice point at least 0.2 px away from a kink (on the kink itself the
    side is a matter of the coordinate's rounding: the ATen comparison above decides there).  Zeros padding mixes in the zeros outside the
    image, so only border / reflection are asserted pointwise; every padding gets the all-modes checks below."""
    H, W = src
    dt = FDT[dn]
    px, py = pixel_list(W), pixel_list(H)
    gy, gx = torch.meshgrid(normalise(py, H, align).to(dt), normalise(px, W, align).to(dt), indexing="ij")
    grid = torch.stack([gx, gy], -1)[None].contiguous()
    jj, ii = torch.meshgrid(torch.arange(W, dtype=dt), torch.arange(H, dtype=dt), indexing="xy")
    x = (jj + 8 * ii)[None, None].contiguous()
    go = torch.ones(1, 1, len(py), len(px), dtype=dt)
    if pad != "zeros":
        _, _, gg = native(x, grid, go, "bilinear", pad, align)
        for a, (plist, n) in enumerate(((px, W), (py, H))):
            if n == 1 and align:
                continue  # (normalise() is not a pixel position on the scale-0 axis; asserted below)
            for k, p in enumerate(plist):
                want = _expected_sign(p, n, pad, align)
                if want is None:
                    continue
                got = gg[0, :, k, 0] if a == 0 else gg[0, k, :, 1]
                # (the other axis' weights multiply this component: they sum to 1 under border / reflection, every tap being inside the image)
                assert (torch.sign(got) == want).all(), (("x", "y")[a], p, want, got.tolist())
    for mode in MODES:
        _, _, gg = native(x, grid, go, mode, pad, align)
        if mode == "nearest":
            assert (gg == 0).all()  # exactly zero, as ATen defines it
        if align and W == 1:
            assert (gg[..., 0] == 0).all(), mode  # the unnormalise scale (W - 1) / 2 is 0: exactly zero in every mode and padding
        if align and H == 1:
            assert (gg[..., 1] == 0).all(), mode


# =================================================================================================
# views of the grid, an odd storage offset
# =================================================================================================
def _odd_offset(t):
    """t on the device, contiguous, one element past an aligned address: the kernel loads a coordinate PAIR with one request"""
    if t.dtype != torch.float64:
        return unaligned(t)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype).cuda()  # (unaligned() asserts an address that is no multiple of 8: fp64 pairs are 16 bytes)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dn", list(FDT) + list(HDT))
def test_grid_views_and_odd_storage_offset_give_the_contiguous_copys_bits(dn, mode):
    import kornia_amd as K

    x, grid, go, n = case((5, 7), dn, False, False)
    x, go = x[:, :3].contiguous().cuda(), go[:, :3].contiguous().cuda()

    def run(g):
        xg, gg = x.detach().requires_grad_(), g.requires_grad_()  # (detach: a leaf that keeps a view's storage offset)
        y = K.grid_sample(xg, gg, mode, "reflection", False)
        y.backward(go[..., : y.shape[-2], : y.shape[-1]])
        return y.detach(), gg.grad

    base = grid.cuda()
    y0, gg0 = run(base.clone())
    # transposed storage: (B,w,h,2) memory seen as (B,h,w,2)
    yt, ggt = run(base.transpose(1, 2).contiguous().transpose(1, 2).detach())
    assert _same(yt, y0) and _same(ggt, gg0)
    # a slice of a larger grid (strided rows, a storage offset of one pair and one row)
    big = torch.zeros(B, base.shape[1] + 2, base.shape[2] + 3, 2, dtype=base.dtype).cuda()
    big[:, 1:-1, 1:-2] = base
    ys, ggs = run(big[:, 1:-1, 1:-2].detach())
    assert _same(ys, y0) and _same(ggs, gg0)
    # one grid expand()ed over the batch (stride 0) against its materialised copy
    ye, gge = run(base[:1].expand(B, -1, -1, -1).detach())
    yc, ggc = run(base[:1].expand(B, -1, -1, -1).contiguous())
    assert _same(ye, yc) and _same(gge, ggc)
    # odd storage offset of the grid (and of the image)
    yo, ggo = run(_odd_offset(grid).detach())
    assert _same(yo, y0) and _same(ggo, gg0)
    x = _odd_offset(x.cpu())
    yo, ggo = run(_odd_offset(grid).detach())
    assert _same(yo, y0) and _same(ggo, gg0)


# =================================================================================================
# callers: remap, HomographyWarper
# =================================================================================================
@pytest.mark.parametrize("align", [False, True], ids=["ac0", "ac1"])
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("src", [(5, 7), (1, 6), (3, 2)], ids=SID)
def test_remap_in_pixel_coordinates_is_grid_sample_on_the_normalised_grid(src, mode, pad, align):
    """remap's pixel maps are the lattice's pixel lists themselves (remap's pixel convention is align_corners=True's whatever the sampler is told:
    normalize_pixel_coordinates, `2 / (size - 1).clamp(1e-8) * p - 1`, restated here in the tensor operations it uses), one map shared by the
    batch; the result is grid_sample's on that grid, bit for bit."""
    import kornia_amd as K

    H, W = src
    x = case(src, "f32", align, False)[0][:, :3].contiguous().cuda()
    my, mx = torch.meshgrid(torch.tensor(pixel_list(H), dtype=torch.float32), torch.tensor(pixel_list(W), dtype=torch.float32), indexing="ij")
    mx, my = mx[None].cuda(), my[None].cuda()
    got = K.remap(x, mx, my, mode, pad, align_corners=align)
    fx = torch.tensor(2.0) / torch.tensor(float(W - 1)).clamp(1e-8)
    fy = torch.tensor(2.0) / torch.tensor(float(H - 1)).clamp(1e-8)
    grid = torch.stack([fx.cuda() * mx - 1, fy.cuda() * my - 1], -1)
    assert _same(got, K.grid_sample(x, grid, mode, pad, align))
    # normalised maps pass through untouched
    assert _same(K.remap(x, grid[..., 0], grid[..., 1], mode, pad, align_corners=align, normalized_coordinates=True), got)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mode", MODES)
def test_homography_warper_with_a_precomputed_grid_is_grid_sample_on_that_grid(mode, pad):
    """HomographyWarper.precompute_warp_grid keeps the homography and regenerates the grid in registers; `_warped_grid` is that grid built by
    tensor operations.  Sampling the latter with grid_sample gives the former's bits.  The homography is dyadic (a swap of the axes, scales
    0.5 / -1, a shift of 0.25, last row (0, 0, 1)): every product is exact and every sum has one rounding, so the grid does not depend on the
    order in which a matrix product is summed - which the two sides are free to choose differently."""
    import kornia_amd as K

    x = case((5, 7), "f32", False, False)[0][:, :3].contiguous().cuda()
    Hm = torch.tensor([[[0.0, 0.5, 0.25], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], [[0.5, 0.0, -0.25], [0.0, 2.0, 0.5], [0.0, 0.0, 1.0]]]).cuda()
    for align in (False, True):
        warper = K.HomographyWarper(33, 65, mode, pad, True, align)
        warper.precompute_warp_grid(Hm)
        got = warper(x)
        grid = warper._warped_grid
        assert grid.shape == (B, 33, 65, 2)
        assert _same(got, K.grid_sample(x, grid, mode, pad, align))


# =================================================================================================
# 16-bit storage
# =================================================================================================
@pytest.mark.parametrize("align", [False, True], ids=["ac0", "ac1"])
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dn", list(HDT))
@pytest.mark.parametrize("src", [(8, 4), (5, 7)], ids=SID)
def test_16_bit_lattice_is_the_fp32_path_rounded_once(src, dn, mode, pad, align):
    """The contract of tests/test_gpu_half_grads.py (forward: test_gpu_warp.py::test_16_bit_storage_is_the_fp32_result_rounded_once), on the lattice:
      * forward: EXACTLY the native fp32 forward of the same (rounded) image and grid, rounded once to the storage dtype;
      * image gradient: accumulated in fp32 atomics and cast once - within 1 ulp of the storage dtype of the fp32 path's at each entry
        (test_gpu_half_grads.py::test_grid_sample_gradients);
      * grid gradient: computed per output pixel in fp32 from the same values and cast: the fp32 path's, rounded once, bit for bit;
      * against fp64 (ATen's CPU sampler on the rounded values, positions in fp64): within 1 ulp of the storage dtype plus the fp32 tests' bound
        (this file's GRAD_TOL), on the lattice of the 8 x 4 source: without align_corners it is exact in both 16-bit types, and with it the points
        that sit on a kink are (-1, 0, 1, 2: the others move off their kink by the storage rounding, far more than fp32 arithmetic moves them),
        so the fp32 and the fp64 positions are on the same side of every kink; nearest and bicubic included."""
    dt = HDT[dn]
    x16, grid16, go16, n = case(src, dn, align, False)
    x16, go16 = x16[:, :3].contiguous(), go16[:, :3].contiguous()
    y16, gx16, gg16 = native(x16, grid16, go16, mode, pad, align)
    y32, gx32, gg32 = native(x16.float(), grid16.float(), go16.float(), mode, pad, align)
    assert y16.dtype == gx16.dtype == gg16.dtype == dt
    assert _same(y16, y32.to(dt)), (y16.float() - y32).abs().max().item()
    assert _within_ulps(gx16, gx32, dt) <= 1.0
    assert _same(gg16, gg32.to(dt))
    if src == (8, 4):  # the lattice corner only: the random coordinates around it are not exact in fp32 arithmetic
        xl, gl, gol = x16.double(), grid16[:, :n, :n].double().contiguous(), go16[:, :, :n, :n].double().contiguous()
        _, gxl16, ggl16 = native(x16, grid16[:, :n, :n].contiguous(), go16[:, :, :n, :n].contiguous(), mode, pad, align)
        _, gxr, ggr = aten(xl, gl, gol, mode, pad, align)
        (rx, ax), (rg, ag) = GRAD_TOL["f32"]
        for got, ref, rtol, atol in ((gxl16, gxr, rx, ax), (ggl16, ggr, rg, ag)):
            tol = _ulp(ref, dt) + atol * ref.abs().max() + rtol * ref.abs()
            assert ((got.double() - ref).abs() <= tol).all(), ((got.double() - ref).abs() / tol).max().item()


# =================================================================================================
# grids that hold NaN / inf: the recorded forward of ATen's CPU sampler; the backward is the forward's adjoint
# =================================================================================================
def _landing(v, n, pad):
    """the cell of an axis of n cells a non-finite coordinate v is brought to: border clips +inf to the last cell and NaN, like -inf, to cell 0;
    reflection has no remainder for any of the three (NaN), which its clamp brings to cell 0"""
    return n - 1 if (pad == "border" and v == inf) else 0


@pytest.mark.parametrize("align", [False, True], ids=["ac0", "ac1"])
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dn", list(FDT))
@pytest.mark.parametrize("name", list(NF_SOURCES))
def test_non_finite_grid_forward_matches_the_recorded_reference(name, dn, mode, pad, align):
    """NaN, +inf and -inf coordinates, alone and paired with finite ones.  Zeros padding: such a position is out of bounds with NaN weights (NaN for
    bilinear and bicubic, 0 for nearest).  Border: NaN clips to coordinate 0, like -inf.  Reflection: NaN and both infinities have no remainder
    (NaN), which the clamp that follows brings to coordinate 0 as well."""
    import kornia_amd as K

    d = golden("nonfinite_grid")
    x, grid = nf_inputs(name, FDT[dn])
    ref = torch.from_numpy(d[nf_key(name, dn, mode, pad, align)])
    got = K.grid_sample(x.cuda(), grid.cuda(), mode, pad, align).cpu()
    if mode == "bicubic":
        assert torch.equal(got.isnan(), ref.isnan())
        assert (got - ref).nan_to_num().abs().max().item() <= (5e-7 if dn == "f32" else 1e-12)
    else:
        assert _same(got, ref), (got - ref).abs().nan_to_num(9.0).max().item()
    if mode != "bicubic" and pad != "zeros":
        assert torch.isfinite(got).all()  # in words: border / reflection bring EVERY position into the image
        H, W = NF_SOURCES[name]
        for i, vy in enumerate(NF_VALUES[:3]):  # both coordinates non-finite: the pixel they land on
            for j, vx in enumerate(NF_VALUES[:3]):
                assert (got[0, :, i, j] == x[0, :, _landing(vy, H, pad), _landing(vx, W, pad)]).all(), (vx, vy)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dn", list(FDT))
def test_non_finite_grid_backward_is_the_adjoint_of_the_forward(dn, mode, pad):
    """No reference exists (ATen's CPU backward faults on these grids and is NOT called).  What is asserted of the native backward:
      * it returns;
      * the sample of the batch whose grid is finite gets, bit for bit, the output and the grid gradient it gets alone, and the image gradient
        it gets alone (exactly for nearest with an integer grad_out, whose sums are exact in any order; within 1e-6 of the largest entry
        otherwise - the order of the atomics, test_zz_gpu_nonfinite_paths.py's bound);
      * under border / reflection with bilinear or nearest - where the forward treats a non-finite coordinate as clipped (to 0; +inf under border
        to the last cell) - nothing that is not finite reaches the image gradient, the gradient with respect to the non-finite coordinate itself is exactly 0 (the clip's
        derivative) and every grid gradient is finite; and since every tap is inside the image and a pixel's weights sum to 1, the image
        gradient sums to what grad_out sums to: the pixels with non-finite coordinates scatter their whole weight, like any other;
      * under zeros padding a non-finite position is out of bounds: it scatters nothing (the image gradient is finite)."""
    dt = FDT[dn]
    for align in (False, True):
        x0, g0 = nf_inputs("5x7", dt)
        gen = torch.Generator().manual_seed(11)
        x = torch.cat([x0, x0.flip(-1)])
        g1 = (torch.rand(g0.shape, generator=gen, dtype=torch.float64) * 2.6 - 1.3).to(dt)
        grid = torch.cat([g0, g1])
        go = torch.randint(-3, 4, (2, 2, *g0.shape[1:3]), generator=gen).to(dt)
        y, gx, gg = native(x, grid, go, mode, pad, align)
        y1, gx1, gg1 = native(x[1:], grid[1:], go[1:], mode, pad, align)
        assert torch.equal(y[1:], y1) and torch.equal(gg[1:], gg1) and torch.isfinite(y1).all() and torch.isfinite(gg1).all()
        if mode == "nearest":
            assert torch.equal(gx[1:], gx1)
        else:
            assert (gx[1:] - gx1).abs().max().item() <= 1e-6 * max(1.0, gx1.abs().max().item())
        if pad == "zeros":
            assert torch.isfinite(gx).all()
        elif mode != "bicubic":
            assert torch.isfinite(gx).all() and torch.isfinite(gg).all()
            bad = ~torch.isfinite(grid)
            assert (gg[bad] == 0).all()
            tol = 1e-5 if dn == "f32" else 1e-12
            assert abs(gx[0].double().sum().item() - go[0].double().sum().item()) <= tol * go[0].abs().sum().item()
            # both coordinates non-finite: the whole of such a pixel's grad_out lands on the one pixel the forward reads for it - take those
            # pixels out and exactly that is what the image gradient loses
            both = bad.all(-1)[0]
            grid2, go2 = grid.clone(), go.clone()
            grid2[0][both] = -1.0  # (any finite coordinate: its grad_out is zeroed)
            go2[0][:, both] = 0
            _, gx2, _ = native(x, grid2, go2, mode, pad, align)
            moved = gx[0] - gx2[0]
            want = torch.zeros_like(moved)
            for i, j in both.nonzero().tolist():
                want[:, _landing(grid[0, i, j, 1].item(), 5, pad), _landing(grid[0, i, j, 0].item(), 7, pad)] += go[0, :, i, j]
            assert (moved - want).abs().max().item() <= tol * max(1.0, go[0].abs().sum().item())


def _bad_matrices(n, H, W, g):
    """the matrices of tests/test_zz_gpu_nonfinite_paths.py that make EVERY position NaN: all zeros (singular), a NaN entry; then ordinary ones"""
    from _util import flagship_homographies

    M = flagship_homographies(n, H, W, H, W, g, jitter=3.0)
    M[0] = 0.0
    M[1, 0, 2] = nan
    return M


@pytest.mark.parametrize("pad", ["border", "reflection"])
@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_warps_with_a_matrix_that_is_no_map_sample_pixel_0_0_under_border_and_reflection(mode, pad):
    """The three warps share the sampler's clip and reflection: a singular or NaN-carrying matrix makes every position of its sample NaN, which
    border / reflection padding bring to coordinate (0, 0).  Forward: the sample's output is its pixel (0, 0) everywhere.  Backward (bilinear
    fp32: the one-read tile-owner kernel's border / reflection path; nearest: the atomics): the whole of grad_out lands on pixel (0, 0), nothing
    non-finite anywhere, and the ordinary samples get what they get without their neighbours."""
    import kornia_amd as K

    H, W, n = 40, 57, 4
    g = torch.Generator().manual_seed(H + W)
    x = torch.rand(n, 3, H, W, generator=g)
    M = _bad_matrices(n, H, W, g)
    go = torch.randint(-2, 3, (n, 3, H, W), generator=g).float()
    Hn = torch.eye(3).repeat(n, 1, 1) + 0.02 * (M - M[3]).nan_to_num().clamp(-1, 1)
    Hn[0] = nan                      # (homography_warp applies its matrix as it is: both numerators must be NaN for a NaN position)
    Hn[1, 0, 2] = Hn[1, 1, 2] = nan
    for fn, Min in ((K.warp_perspective, M), (K.warp_affine, M[:, :2].contiguous()), (K.homography_warp, Hn)):
        xg, Mg = x.cuda().requires_grad_(), Min.cuda().requires_grad_()
        y = fn(xg, Mg, (H, W), mode=mode, padding_mode=pad)
        y.backward(go.cuda())
        torch.cuda.synchronize()
        y, gx = y.detach().cpu(), xg.grad.cpu()
        assert torch.isfinite(y).all() and torch.isfinite(gx).all(), fn.__name__
        for b in (0, 1):
            assert (y[b] == x[b, :, :1, :1]).all(), (fn.__name__, b)
            want = torch.zeros(3, H, W)
            want[:, 0, 0] = go[b].sum((-1, -2))
            assert (gx[b] - want).abs().max().item() <= 1e-5 * go[b].abs().sum((-1, -2)).max().item(), (fn.__name__, b)
        x2, M2 = x[2:].cuda().requires_grad_(), Min[2:].cuda().requires_grad_()
        y2 = fn(x2, M2, (H, W), mode=mode, padding_mode=pad)
        y2.backward(go[2:].cuda())
        assert torch.equal(y[2:], y2.detach().cpu())
        assert (gx[2:] - x2.grad.cpu()).abs().max().item() <= 1e-6 * max(1.0, gx[2:].abs().max().item())


# =================================================================================================
# finite coordinates far outside the image, under reflection
# =================================================================================================
# ATen's CPU sampler folds d = |x - low| as d - trunc(d / (2 span)) * (2 span); the native one takes an exact fmod(d, span) and the parity of
# floor(d / span).  With p the precision (24 bits in fp32, 53 in fp64) and d < 2^p: d is a multiple of its own spacing u <= 1, and so is every
# multiple of the (half-)integer span below it, so ATen's product and difference are exact; and its quotient cannot round up to the next
# integer k + 1, which would need the distance of d from (k + 1) 2 span - a positive multiple of u - to be at most d 2^-p < u.  So the two agree
# bit for bit while |pixel coordinate| < 2^p, WHATEVER the span (not 2^p / span); from 2^p on d is an even integer with u > 1 and ATen's
# quotient does round across multiples.  Confirmed on the host build, 4096 random mantissas per octave, sources 5 x 7, 3 x 2 and 2 x 65, both
# align_corners, bilinear and nearest: no difference in any octave below 2^24 (fp32) / 2^53 (fp64); without align_corners 716 / 70 of 8192
# outputs (5 x 7 / 2 x 65) differ in the octave [2^24, 2^25) and 787 / 94 in [2^53, 2^54) (power-of-two spans - 3 x 2 - hold an octave or
# more longer).
# Bicubic without align_corners holds to 2^(p - 1) only: its taps are whole numbers that go through the reflection one by one, and from 2^(p - 1)
# on `tap + 0.5` is a tie that rounds the half away, so the reflected tap comes out as a HALF-integer - which the native sampler truncates to
# an index and ATen's vector conversion of this build rounds to nearest in fp64 (found on the first device run of this test, same on the host
# build: position 2^52 + 2 on a 5 x 7 source reads column 3 natively and column 4 in ATen).  Below 2^(p - 1) every tap arithmetic is exact.
AGREE_BITS = {"f32": 24, "f64": 53}


def _far_grid(dn, W, H, align, lo_bits, hi_bits, count):
    """(1,2,count,2) normalised coordinates whose PIXEL positions are +-2^e * (1 + random mantissa) for e in [lo_bits, hi_bits) along x, with a
    tame y, and the same with the axes swapped"""
    dt = FDT[dn]
    g = torch.Generator().manual_seed(lo_bits * 64 + hi_bits)
    e = torch.randint(lo_bits, hi_bits, (count,), generator=g).double()
    p = torch.pow(2.0, e) * (1 + torch.rand(count, generator=g, dtype=torch.float64)) * (torch.randint(0, 2, (count,), generator=g) * 2 - 1)
    p = torch.minimum(p.abs(), torch.tensor(2.0 ** hi_bits * (1 - 2.0 ** -20), dtype=torch.float64)) * torch.sign(p)
    tame = torch.rand(count, generator=g, dtype=torch.float64) * 2.6 - 1.3
    gx, gy = normalise(p, W, align), normalise(p, H, align)
    return torch.stack([torch.stack([gx, tame], -1), torch.stack([tame, gy], -1)])[None].to(dt)


@pytest.mark.parametrize("align", [False, True], ids=["ac0", "ac1"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dn", list(FDT))
def test_reflection_far_outside_matches_aten_up_to_the_derived_bound(dn, mode, align):
    """Pixel coordinates from 2^4 up to 2^24 (fp32) / 2^53 (fp64), both signs, random mantissas, spans 2 .. 65: the same bits as ATen's CPU sampler (bicubic:
    its bound, and without align_corners one octave less - see above), the gradients' usual bounds."""
    for H, W in ((5, 7), (3, 2), (2, 65)):
        x = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(W), dtype=torch.float64).to(FDT[dn])
        bits = AGREE_BITS[dn] - (1 if mode == "bicubic" and not align else 0)
        # (_far_grid keeps 2^-20 of head-room below 2^bits: the normalised coordinate is rounded to the dtype and unnormalised again)
        grid = _far_grid(dn, W, H, align, 4, bits, 2048)
        go = torch.ones(1, 3, *grid.shape[1:3], dtype=FDT[dn])
        y, gx, gg = native(x, grid, go, mode, "reflection", align)
        yr, gxr, ggr = aten(x, grid, go, mode, "reflection", align)
        if mode != "bicubic":
            assert torch.equal(y, yr), ((y - yr).abs().max().item(), int((y != yr).sum()))
        else:
            assert (y - yr).abs().max().item() <= (5e-7 if dn == "f32" else 1e-12)
        (rx, ax), (rg, ag) = GRAD_TOL[dn]
        assert off_by(gx, gxr, rx, ax) <= 1.0 and off_by(gg, ggr, rg, ag) <= 1.0


@pytest.mark.parametrize("align", [False, True], ids=["ac0", "ac1"])
@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("dn", list(FDT))
def test_reflection_beyond_the_bound_stays_finite_and_inside_the_images_range(dn, mode, align):
    """Beyond 2^24 / 2^53 pixels the two samplers' results are both noise (the coordinate's spacing exceeds a pixel) and no agreement is asked:
    only that the output is finite and within [min, max] of the image - a pixel for nearest, a convex combination for bilinear (its two weights
    per axis are a and 1 - a exactly; the four-term fma chain rounds, hence 4 spacings of slack).  Includes normalised 3e9 and 1e30, fold counts
    past INT_MAX (the parity is computed in floating point), the largest finite number, whose pixel position overflows to inf (-> coordinate 0)."""
    dt = FDT[dn]
    fi = torch.finfo(dt)
    for H, W in ((5, 7), (3, 2), (1, 6)):
        x = case((H, W), dn, align, False)[0][:1, :3].contiguous()
        far = _far_grid(dn, W, H, align, AGREE_BITS[dn], AGREE_BITS[dn] + 40, 512)
        hand = torch.tensor([3e9, -3e9, 1e30, -1e30, fi.max, -fi.max, fi.max / 8, 2.0 ** 31 * W, -(2.0 ** 33) * W + 1, 2.0 ** 63, -(2.0 ** 64)], dtype=torch.float64)
        tame = torch.linspace(-1.3, 1.3, hand.numel(), dtype=torch.float64)
        extra = torch.stack([torch.stack([hand, tame], -1), torch.stack([tame, hand], -1)])[None].to(dt)
        for grid in (far, extra, torch.stack([hand, hand.flip(0)], -1)[None, None].to(dt)):
            go = torch.ones(1, 3, *grid.shape[1:3], dtype=dt)
            y, gx, gg = native(x, grid, go, mode, "reflection", align)
            assert torch.isfinite(y).all() and torch.isfinite(gx).all() and torch.isfinite(gg).all()
            lo, hi = x.amin((-1, -2)).reshape(1, 3, 1, 1), x.amax((-1, -2)).reshape(1, 3, 1, 1)
            slack = 4 * fi.eps if mode == "bilinear" else 0.0
            assert (y >= lo * (1 - slack)).all() and (y <= hi * (1 + slack)).all()
