"""GPU (and, through tests/test_emulated_nonfinite_pixels.py, the host build of the kernels): a NaN, a +inf or a -inf PIXEL through the native
ops, against what the reference returns for the same image (tests/golden/nonfinite_pixels.npz and nonfinite_pixels_2.npz; images, planted pixels and calls are the table of
tests/nonfinite_pixel_cases.py).  For every recorded case:
  * the NaN mask is the fixture's, entry for entry; so are the inf mask and the signs of the infinities;
  * every entry that is finite in the fixture is finite here and agrees at the tolerance the op's own test uses (Case.tol; 0 = bit for bit);
    in 16-bit storage within 1 ulp of the storage dtype of the fp32 record (the native path computes in fp32 and rounds once; the reference
    rounds after every torch op, so its own 16-bit values are the coarser ones - its 16-bit NaN / inf masks are what is compared);
  * the clean sample of the batch is bit for bit what the same call returns for that sample alone;
  * both members of every path pair give the same bits: the aligned image and the same values one element past an aligned address, W = 24
    and W = 23 each against the fixture, and the launch policies of km_config_set (_POLICIES below).
Stated difference ("Non-finite pixel values"): the bf16 spatial_gradient, where the reference's bf16 convolution puts NaN outside
the window (nonfinite_pixel_cases.STATED): the native result is held to the fp32 record's pattern.  Sorted late, like the coordinate file."""
import math

import pytest
import torch

import nonfinite_pixel_cases as P
from _util import golden
from test_gpu_half_grads import _with_config, _within_ulps
from test_gpu_median import unaligned

pytestmark = pytest.mark.gpu

_FIX = {}


def fixture():
    if not _FIX:
        _FIX.update(golden("nonfinite_pixels"))
        _FIX.update(golden("nonfinite_pixels_2"))
    return _FIX


def recorded(case, sn, dn, what="y"):
    """(kinds, ...) tensor in the storage dtype, or None where the reference has no CPU op for that dtype (the generator lists those)"""
    a = fixture().get(P.key(case, sn, dn, what))
    return None if a is None else torch.from_numpy(a).movedim(-1, 0).to(P.DTYPES[dn])


def agree(out, ref, tol, what, values=None):
    """the three assertions of the module docstring for one result; values: the fp32 record, for a 16-bit ref"""
    out, ref = out.detach().cpu(), ref.cpu()
    if values is not None:
        ref = torch.where(torch.isfinite(ref) & torch.isfinite(values), values.to(ref.dtype), ref)
    assert out.dtype == ref.dtype and out.shape == ref.shape, what
    assert torch.equal(out.isnan(), ref.isnan()), (what, "NaN mask", int((out.isnan() != ref.isnan()).sum()))
    inf = ref.isinf()
    assert torch.equal(out.isinf(), inf) and torch.equal(out[inf], ref[inf]), (what, "inf mask / signs", int((out.isinf() != inf).sum()))
    fin = torch.isfinite(ref)
    if ref.dtype in (torch.bfloat16, torch.float16):
        e = _within_ulps(out, ref, ref.dtype, 1.0, tol)
        assert e <= 1.0, (what, e)
    elif tol == 0.0:
        assert torch.equal(out[fin], ref[fin]), (what, (out[fin] - ref[fin]).abs().max().item())
    elif fin.any():
        assert (out[fin] - ref[fin]).abs().max().item() <= tol, (what, (out[fin] - ref[fin]).abs().max().item())


def same_bits(a, b, tol=0.0):
    """two native paths: the same NaN entries, the same infinities, the finite entries bit for bit (tol = 0) or within tol - twice the
    storage dtype's spacing for a 16-bit pair whose fp32 results are within tol"""
    a, b = a.detach().cpu(), b.detach().cpu()
    nan, fin = a.isnan(), torch.isfinite(a)
    if not (a.dtype == b.dtype and a.shape == b.shape and torch.equal(nan, b.isnan()) and torch.equal(fin, torch.isfinite(b)) and torch.equal(a[~nan & ~fin], b[~nan & ~fin])):
        return False
    if tol == 0.0:
        return torch.equal(a[fin], b[fin])
    if a.dtype in (torch.bfloat16, torch.float16):
        return _within_ulps(a, b, a.dtype, 1.0, tol) <= 1.0
    return not fin.any() or (a[fin] - b[fin]).abs().max().item() <= tol


# the launch policies under which a case runs again (km_config_set keys, csrc/km_runtime.hip): every one must give the default's bits
def _policies(name):
    if name.startswith(("sep_", "box_blur")):
        return [{"sep_lds": 1}, {"blur_rows": 8}, {"blur_rows": 16}, {"blur_rows": 32}]
    if name.startswith(("sg_", "sobel")):
        return [{"sg_generic": 1}]
    if name.startswith("pyr"):
        return [{"pyrdown_separable": 1}, {"pyrdown_separable": 1, "blur_rows": 16}]
    if name.startswith(("warp_", "homography_warp", "remap", "grid_sample")):
        return [{"warp_fwd_algo": 1}, {"warp_fwd_algo": 3}, {"warp_fwd_algo": 4}]
    return []


# the warp backward: the one-read (fused) backward on and off, and the generic kernels
_BWD_POLICIES = [{"warp_bwd_fused": 0}, {"warp_bwd_fused": 1}, {"warp_bwd_generic": 1}, {"warp_bwd_fused": 0, "warp_bwd_generic": 1}]


@pytest.mark.parametrize("name", [c.name for c in P.ALL_CASES])
def test_forward_matches_the_reference_on_every_path(name):
    """Every case of the table: the paths are named by the shapes (nonfinite_pixel_cases.SHAPES: w24 the register-tiled / vector / LDS-staged
    kernels - km_blur_reg_kernel, the x2 up-sampling, km_warp_fwd_cubic_kernel; w23 the LDS / generic / gather kernels; tall two strips; box
    the box forward km_warp_fwd_box_kernel) and by _policies."""
    import kornia_amd as K

    case = P.BY_NAME[name]
    run = case.native()
    for sn in case.shapes:
        for dn in case.dtypes_for(sn) + case.extra_for(sn):
            ref, ref32 = recorded(case, sn, dn), None
            if dn in ("bf16", "f16"):
                ref32 = recorded(case, sn, "f32")
                if ref is None or (name, dn) in P.STATED:  # not recorded in this dtype (Case.extra), or a stated difference: the fp32 record on the same (dyadic, so unrounded) inputs
                    ref = ref32.to(P.DTYPES[dn])
            for i, kind in enumerate(P.KINDS):
                what = (name, sn, dn, kind)
                x = P.image(sn, kind).to(P.DTYPES[dn])
                out = run(K, x.cuda())
                v32 = None if ref32 is None else ref32[i]
                tol = case.tol if ref32 is None or case.tol16 is None else case.tol16
                agree(out[0], ref[i], tol, what, v32)
                alone = run(K, x[1:].cuda())
                assert same_bits(out[1:], alone) and torch.isfinite(alone.float()).all(), (what, "the clean sample")
                if dn != "f64":  # (one fp64 element is 8 bytes: the helper's image is for the 2- and 4-byte dtypes)
                    other = run(K, unaligned(x))
                    agree(other[0], ref[i], tol, what + ("one element past an aligned address",), v32)
                    assert same_bits(other, out, tol), (what, "one element past an aligned address")
                for cfg in _policies(name):
                    got = _with_config(cfg, lambda: run(K, x.cuda()))
                    agree(got[0], ref[i], tol, what + (str(cfg),), v32)
                    assert same_bits(got, out, tol), (what, cfg)


def test_f16_result_overflows_to_inf():
    """f16 only: a finite image (60000) under a 2-tap box of weight 1 each - the reference's result is +inf, not the largest finite value"""
    import kornia_amd as K

    case = P.OVERFLOW
    for sn in case.shapes:
        ref = torch.from_numpy(fixture()[P.key(case, sn, "f16")])  # (no axis of kinds: one finite image)
        x = P.overflow_image(sn).half()
        out = case.native()(K, x.cuda())
        assert ref.isinf().all() and (ref > 0).all()
        agree(out[0], ref, 0.0, sn)
        assert same_bits(case.native()(K, unaligned(x)), out)


@pytest.mark.parametrize("name", [c.name for c in P.CASES if c.grad])
def test_planted_grad_out_through_the_linear_adjoints(name):
    """A NaN / inf in grad_out through the adjoint of every linear op (filter2d interior and frame, the separable adjoint fused and two-pass,
    spatial_gradient, resize, pyrdown, pyrup): the reference's x.grad of the clean image.  Integer grad_out and dyadic taps: exact for the filters."""
    import kornia_amd as K

    case = P.BY_NAME[name]
    tol = 1e-5 if case.tol else 0.0  # (tests/test_gpu_golden.py holds the gradients of the ops with non-dyadic weights to 1e-5)
    for sn in case.shapes:
        ref = recorded(case, sn, "f32", "gx")
        for i, kind in enumerate(P.KINDS):
            def grad(x, first=0):
                x = x.requires_grad_()
                y = case.native()(K, x)
                go = P.grad_out((y.shape[0] + first,) + tuple(y.shape[1:]), kind)  # (the batch's grad_out, of which a sample alone takes its own)
                y.backward(go[first:].cuda())
                return x.grad

            gx = grad(P.image(sn, None).cuda())
            agree(gx[0], ref[i], tol, (name, sn, kind))
            alone = grad(P.image(sn, None)[1:].cuda(), 1)
            assert same_bits(gx[1:], alone) and torch.isfinite(alone).all(), (name, sn, kind, "the clean sample")
            assert same_bits(grad(unaligned(P.image(sn, None))), gx, tol), (name, sn, kind, "unaligned")
            for cfg in _policies(name):
                got = _with_config(cfg, lambda: grad(P.image(sn, None).cuda()))
                agree(got[0], ref[i], tol, (name, sn, kind, str(cfg)))
                assert same_bits(got, gx, tol), (name, sn, kind, cfg)


@pytest.mark.parametrize("order", ["0", "1", "2", "3", "0123", "2031"])
def test_color_jitter_gradients_with_a_non_finite_pixel(order):
    """The image and factor gradients of color_jitter through the reference's autograd with a non-finite pixel in the image: the backward
    recomputes the stage chain (km_color_jitter_bwd_kernel), so a clamp that drops a NaN there shows as a finite gradient.  Pattern exact;
    finite entries at the tolerance of tests/test_gpu_color.py::test_backward_matches_autograd_through_the_reference_ops (2e-5 of the
    largest finite entry for the image, 2e-3 for the factors)."""
    import kornia_amd as K

    d = fixture()
    for sn in P.TWO:
        for kind in P.KINDS:
            base = f"jitterbwd_{order}__{sn}__{kind}__f32__"
            x = P.image(sn, kind).cuda().requires_grad_()
            f = [torch.tensor(v, device="cuda", requires_grad=True) for v in (P.BF, P.CF, P.SF, P.HF)]
            given = [f[0], f[1], f[2], f[3] / (2.0 * math.pi)]  # (color_jitter takes the hue shift in turns)
            out = K.enhance.color_jitter(x, *[given[s] if str(s) in order else None for s in range(4)], [int(s) for s in order])
            w = torch.randint(-2, 3, out.shape, generator=torch.Generator().manual_seed(5)).float()
            (out * w.cuda()).sum().backward()
            ref = torch.from_numpy(d[base + "gx"])
            scale = ref[torch.isfinite(ref)].abs().max().item() if torch.isfinite(ref).any() else 0.0
            agree(x.grad[:1], ref, 2e-5 * scale, (order, sn, kind, "gx"))
            # the clean sample: the same bits as the same call on that sample alone
            x1 = P.image(sn, kind)[1:].cuda().requires_grad_()
            f1 = [v.detach()[1:] for v in given]
            out1 = K.enhance.color_jitter(x1, *[f1[s] if str(s) in order else None for s in range(4)], [int(s) for s in order])
            (out1 * w[1:].cuda()).sum().backward()
            assert same_bits(x.grad[1:], x1.grad) and torch.isfinite(x1.grad).all(), (order, sn, kind, "the clean sample")
            for s in order:
                rf = torch.from_numpy(d[base + f"gf{s}"])
                fin = torch.isfinite(rf)
                agree(f[int(s)].grad, rf, 2e-3 * max(rf[fin].abs().max().item(), 1.0) if fin.any() else 0.0, (order, sn, kind, "factor", s))


def test_filter2d_tap_gradient_with_a_non_finite_pixel():
    import kornia_amd as K

    d = fixture()
    for sn in P.TWO:
        for kind in P.KINDS:
            taps = torch.tensor(P.K33Z, device="cuda", requires_grad=True)
            y = K.filters.filter2d(P.image(sn, kind).cuda(), taps, "reflect")
            w = torch.randint(-2, 3, y.shape, generator=torch.Generator().manual_seed(6)).float()
            (y * w.cuda()).sum().backward()
            agree(taps.grad, torch.from_numpy(d[f"f2dtaps__{sn}__{kind}__f32__gk"]), 1e-4, (sn, kind))


@pytest.mark.parametrize("loss,threshold", P.LOSSES)
def test_masked_warp_loss_with_a_non_finite_pixel(loss, threshold):
    """km_warp_loss (one launch): the loss of an image with a non-finite pixel against the reference's composition, masked and not; finite
    results at the 2e-6 of tests/test_zz_gpu_registration.py::test_single_level_loss_vs_reference"""
    import kornia_amd as K

    Hn = torch.tensor(P.HN).cuda()
    for sn in P.TWO:
        for kind in P.KINDS:
            src, dst = P.image(sn, kind), P.image(sn, None).flip(-1)
            ref = torch.from_numpy(fixture()[f"loss_{loss}_{threshold}__{sn}__{kind}__f32__y"])
            out = K.geometry.transform.masked_warp_loss(src.cuda(), dst.cuda(), Hn, loss, threshold=threshold)
            agree(out, ref, 2e-6, (loss, threshold, sn, kind))
            other = K.geometry.transform.masked_warp_loss(unaligned(src), unaligned(dst), Hn, loss, threshold=threshold)
            assert same_bits(other, out, 2e-6), (loss, threshold, sn, kind, "unaligned")


def test_transform_points_with_a_non_finite_point():
    import kornia_amd as K

    for kind in P.KINDS:
        ref = torch.from_numpy(fixture()[f"points__{kind}__f32__y"])
        out = K.geometry.linalg.transform_points(torch.tensor(P.PER).cuda(), P.points(kind).cuda())
        agree(out, ref, 1e-6, kind)  # (tests/test_gpu_points.py: 1e-6 of coordinates of this size)
        alone = K.geometry.linalg.transform_points(torch.tensor(P.PER[1:]).cuda(), P.points(kind)[1:].cuda())
        assert same_bits(out[1:], alone) and torch.isfinite(alone).all(), (kind, "the clean sample")


@pytest.mark.parametrize("pad,sn", P.WARP_GRADS)
def test_warp_gradients_with_a_non_finite_pixel(pad, sn):
    """Both gradients of the bilinear warp_perspective with non-finite PIXELS and a finite grad_out: the image gradient does not depend on the
    pixels, the matrix gradient of that sample does (it is a sum of grad_out x pixel differences).  Intended paths - w24 / w23: the small-image
    backward; box (64 x 64, C = 3): the tile-owner kernel; stage (70 x 100): ragged tile rows and columns of the one-read backward's LDS
    staging, the shape of tests/test_gpu_warp_fused.py::test_source_tile_staging_does_not_depend_on_the_address_or_the_tile_shape - each by
    default, with the one-read backward off and on, and on the generic kernels (_BWD_POLICIES), at an aligned and an unaligned address.
    Image gradient: 1e-5 (that test's bound); matrix gradient: the reference's NaN / inf pattern, finite entries to 5e-5 of the largest."""
    import kornia_amd as K

    def grads(x, first=0):
        x, M = x.requires_grad_(), torch.tensor(P.PER[first:]).cuda().requires_grad_()
        y = P.warp_grad_call(K, x, M, pad)
        y.backward(P.grad_out((y.shape[0] + first,) + tuple(y.shape[1:]), None)[first:].cuda())
        return x.grad, M.grad

    def check(gx, gM, rx, rM, what):
        agree(gx[0], rx, 1e-5, what + ("gx",))
        fin = torch.isfinite(rM)
        agree(gM, rM, 5e-5 * rM[fin].abs().max().item(), what + ("gM",))

    for kind in P.KINDS:
        rx, rM = (torch.from_numpy(fixture()[f"warpbwd_{pad}__{sn}__{kind}__f32__{g}"]) for g in ("gx", "gM"))
        gx, gM = grads(P.image(sn, kind).cuda())
        check(gx, gM, rx, rM, (pad, sn, kind))
        ax, aM = grads(P.image(sn, kind)[1:].cuda(), 1)
        # (not bit for bit: the scatter kernels add into the image gradient with atomics, whose order changes from launch to launch, and the
        # matrix gradient is a reduction over blocks that end in no fixed order; one ulp of an entry of size 4 is 5e-7)
        assert torch.isfinite(ax).all() and torch.isfinite(aM).all() and same_bits(gx[1:], ax, 1e-6), (pad, sn, kind, "the clean sample")
        assert (gM[1:] - aM).abs().max().item() <= 5e-5 * aM.abs().max().item(), (pad, sn, kind, "the clean sample's matrix gradient")
        ox, oM = grads(unaligned(P.image(sn, kind)))
        check(ox, oM, rx, rM, (pad, sn, kind, "unaligned"))
        assert same_bits(ox, gx, 1e-6), (pad, sn, kind, "unaligned")
        for cfg in _BWD_POLICIES:
            px, pM = _with_config(cfg, lambda: grads(P.image(sn, kind).cuda()))
            check(px, pM, rx, rM, (pad, sn, kind, str(cfg)))
            # (two kernels sum an entry's up to nine products of |grad_out| <= 2 in different orders: 1e-5, the image gradient's bound above)
            assert same_bits(px, gx, 1e-5), (pad, sn, kind, cfg)
            assert torch.equal(torch.isfinite(pM), torch.isfinite(gM)), (pad, sn, kind, cfg)


@pytest.mark.parametrize("factor", [1.25, 9.999999e17, 1e18])
@pytest.mark.parametrize("value", [1.0, 1.9999999, 2.0, 9.999999e17, 1e18, -0.0])
def test_color_wave_vote_boundary(value, factor):
    """km_color_jitter_kernel runs the plain fminf / fmaxf chain for a wave whose pixels are all in [+0, 2) with factors below 1e18 in
    magnitude (KMC_TAME_MASK32 / 16, KMC_FACTOR_LIMIT_BITS) and the NaN-keeping chain otherwise: a value and a factor just below and at
    their limits, larger values, and a -0; in fp32 and, for the packed test of 16-bit storage, in bf16 and f16 (the nearest storable
    values: 1.9921875 / 1.9990234 are the last below 2).  Brightness
    alone is torch.clamp(x * f, 0, 1) bit for bit on either chain; and the chain brightness - saturation - hue gives, for every pixel but the
    planted one, the same bits whether or not a NaN next to it sends the wave to the NaN-keeping chain."""
    import kornia_amd as K

    for sn in P.TWO:
        x = P.image(sn, None)
        x[0, 1, 7, 9] = value
        f = torch.tensor([factor, 0.75])
        out = K.enhance.adjust_brightness_accumulative(x.cuda(), f.cuda())
        assert torch.equal(out.cpu(), torch.clamp(x * f.view(-1, 1, 1, 1), 0.0, 1.0)), (sn, value, factor)
        xn = x.clone()
        xn[0, 1, 7, 10] = nan = float("nan")
        args = (f.cuda(), None, torch.tensor(P.SF).cuda(), torch.tensor(P.HF).cuda() / (2.0 * math.pi), [0, 2, 3])
        a, b = K.enhance.color_jitter(x.cuda(), *args).cpu(), K.enhance.color_jitter(xn.cuda(), *args).cpu()
        keep = torch.ones_like(x, dtype=torch.bool)
        keep[0, :, 7, 10] = False
        assert b[0, :, 7, 10].isnan().all() and same_bits(a[keep], b[keep]), (sn, value, factor)
        for dt in (torch.bfloat16, torch.float16):  # 16-bit storage: the vote is taken on the packed words
            xh, xnh = x.to(dt), xn.to(dt)
            outh = K.enhance.adjust_brightness_accumulative(xh.cuda(), f.cuda().to(dt)).cpu()
            want = torch.clamp(xh.float() * f.to(dt).float().view(-1, 1, 1, 1), 0.0, 1.0).to(dt)
            assert same_bits(outh, want), (sn, value, factor, dt)  # (a factor of 1e18 is inf in f16: 0 x inf is NaN on both sides)
            ah, bh = K.enhance.color_jitter(xh.cuda(), *args).cpu(), K.enhance.color_jitter(xnh.cuda(), *args).cpu()
            assert bh[0, :, 7, 10].isnan().all() and same_bits(ah[keep], bh[keep]), (sn, value, factor, dt)
