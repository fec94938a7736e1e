"""GPU (and, through tests/test_emulated_bilateral.py, the host build of the kernels): bilateral_blur, joint_bilateral_blur and their modules on
the native path (km_bilateral_blur_fwd / _bwd) against the reference's recorded outputs and float64 gradients (tests/golden/bilateral_blur.npz)
and, for the shapes the fixture lacks, against the restatement that tests/test_bilateral_golden.py anchors to it bit for bit.

Bounds (none fitted to the kernel): float32 forward 1e-5 on [0, 1] images - the project's stated fp32 bound (BASELINE.json north_star); the
reference's own float32 stays within 3e-7 of its float64 over the fixture.  float64 forward 1e-12.  Gradients: 1e-5 of the largest absolute
entry of the float64 gradient (the reference's own float32 gradients: 6.6e-7 on that scale).  16-bit storage: the float32 result of the widened
input rounded once, bit for bit, and within 1 ulp of the fixture's float32 output rounded to the type.  Each test prints what it measured."""
import pytest
import torch

from test_bilateral_golden import (BORDERS, DISTS, F32_BOUND, F64_BOUND, GRAD_BOUND, GRAD_WINDOWS, SIGMA_SPACE, case_inputs, cases, fixture, kname, pad_fits,
                                   parse_case, restate, restate_grads)
from test_gpu_written_outputs import CASES, FILLS, _run_case, case, same_bits, unchanged

pytestmark = pytest.mark.gpu

TW, TH = 32, 8  # the kernels' output tile (KMB_TW, KMB_TH, csrc/km_bilateral.hip)
CT_WINDOWS = [3, 5, 7, 9]  # the compile-time instantiations; (3, 7) and 11 take the run-time kernel
SEAM_SHAPES = [(h, 5) for h in (1, 2, TH - 1, TH, TH + 1, 2 * TH + 3)] + [(3, w) for w in (1, 3, TW - 1, TW, TW + 1, 2 * TW + 3)] + [(2 * TH + 3, 2 * TW + 3)]


def KF():
    import kornia_amd.filters as F

    return F


def quantised(shape, seed):
    return torch.randint(0, 65, shape, generator=torch.Generator().manual_seed(seed)).float() / 64


def run(x, g, k, sc, ss, border, dist):
    return KF().bilateral_blur(x, k, sc, ss, border, dist) if g is None else KF().joint_bilateral_blur(x, g, k, sc, ss, border, dist)


def dev(t):
    return None if t is None else t.cuda()


def test_forward_parity_float32_and_float64():
    d = fixture()
    worst32 = worst64 = 0.0
    for key in cases():
        x, g, k, sc, border, dist = case_inputs(key)
        out = run(dev(x), dev(g), k, sc, SIGMA_SPACE, border, dist)
        assert out.dtype == torch.float32 and out.shape == x.shape
        worst32 = max(worst32, (out.cpu() - d[f"y__{key}__f32"]).abs().max().item())
        x, g, k, sc, border, dist = case_inputs(key, torch.float64)
        out = run(dev(x), dev(g), k, sc, SIGMA_SPACE, border, dist)
        assert out.dtype == torch.float64
        worst64 = max(worst64, (out.cpu() - d[f"y__{key}__f64"]).abs().max().item())
    print(f"bilateral forward: max |native - reference| float32 {worst32:.3e} (bound {F32_BOUND:.0e}), float64 {worst64:.3e} (bound {F64_BOUND:.0e})")
    assert worst32 <= F32_BOUND and worst64 <= F64_BOUND


@pytest.mark.parametrize("func", ["self", "joint"])
def test_tensor_sigmas(func):
    d = fixture()
    x, g = d["x__2x3x13x17"], (d["g__2x3x13x17"] if func == "joint" else None)
    for dn, dt, bound in (("f32", torch.float32, F32_BOUND), ("f64", torch.float64, F64_BOUND)):
        out = run(dev(x.to(dt)), dev(None if g is None else g.to(dt)), (5, 5), d["ts__sigma_color"].to(dt).cuda(), d["ts__sigma_space"].to(dt).cuda(), "reflect", "l1")
        assert (out.cpu() - d[f"ts__{func}__{dn}"]).abs().max().item() <= bound
    # host tensors for the sigmas are moved, a (1,) / (1, 2) pair is shared by the batch
    a = run(dev(x), dev(g), (5, 5), torch.tensor([0.5]), torch.tensor([list(SIGMA_SPACE)]), "reflect", "l1")
    assert torch.equal(a, run(dev(x), dev(g), (5, 5), 0.5, SIGMA_SPACE, "reflect", "l1"))


def _ulps_apart(a: torch.Tensor, b: torch.Tensor) -> int:
    """largest distance in units of the last place between two non-negative 16-bit tensors"""
    return int((a.view(torch.int16).int() - b.view(torch.int16).int()).abs().max())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_16_bit_storage_is_the_float32_result_rounded_once(dt):
    d = fixture()
    for key in cases():
        func, shape, k, dist, border, sc = parse_case(key)
        if shape == (1, 1, 9, 12) and k != (5, 5):
            continue
        x, g, k, sc, border, dist = case_inputs(key)
        x16, g16 = x.to(dt), (None if g is None else g.to(dt))  # (multiples of 1/64: exact in both types)
        out = run(dev(x16), dev(g16), k, sc, SIGMA_SPACE, border, dist)
        y32 = run(dev(x16.float()), dev(None if g16 is None else g16.float()), k, sc, SIGMA_SPACE, border, dist)
        assert out.dtype == dt and same_bits(out.cpu(), y32.to(dt).cpu()), key
        assert _ulps_apart(out.cpu(), d[f"y__{key}__f32"].to(dt)) <= 1, key


def _seam_check(x, g, k, border, dist, sc=0.5):
    if not pad_fits(border, k, x.shape[2], x.shape[3]):
        return 0.0
    out = run(dev(x), dev(g), k, sc, SIGMA_SPACE, border, dist)
    return (out.cpu() - restate(x, g, k, sc, SIGMA_SPACE, border, dist)).abs().max().item()


@pytest.mark.parametrize("k", CT_WINDOWS + [(3, 7), 11], ids=str)
def test_tile_seams(k):
    """every H at one width and every W at one height around the tile's sides, one shape with both large: RGB self-guided (compile-time for the
    square windows up to 9), all four borders where the pad fits"""
    worst = 0.0
    for n, (h, w) in enumerate(SEAM_SHAPES):
        x = quantised((2, 3, h, w), 100 + n)
        for border in BORDERS:
            worst = max(worst, _seam_check(x, None, k, border, DISTS[n % 2]))
    print(f"bilateral seams {k}: max |native - restatement| {worst:.3e}")
    assert worst <= F32_BOUND


@pytest.mark.parametrize("which", ["self-C5", "joint-3-1", "joint-2-4", "self-C16-15x15"])
def test_channel_paths_at_the_seams(which):
    """the run-time channel loops (5 channels self-guided; 16 with a 15 x 15 window, where the launcher shrinks the tile) and two joint pairs
    - RGB guiding one channel, 2 channels guiding 4 - at shapes with ragged tiles, constant and replicate borders"""
    worst = 0.0
    for n, (h, w) in enumerate([(TH + 1, TW + 1), (2 * TH + 3, 2 * TW + 3), (3, TW - 1)]):
        if which == "self-C5":
            x, g, k = quantised((1, 5, h, w), n), None, 5
        elif which == "joint-3-1":
            x, g, k = quantised((2, 1, h, w), n), quantised((2, 3, h, w), 50 + n), 5
        elif which == "joint-2-4":
            x, g, k = quantised((1, 4, h, w), n), quantised((1, 2, h, w), 50 + n), (3, 7)
        else:
            x, g, k = quantised((1, 16, h, w), n), None, 15
        for border in ("constant", "replicate"):
            for dist in DISTS:
                worst = max(worst, _seam_check(x, g, k, border, dist))
    print(f"bilateral channel paths {which}: max |native - restatement| {worst:.3e}")
    assert worst <= F32_BOUND


def _native_grads(x, g, k, sc, border, dist, gout, dt=torch.float32):
    xd = x.to(dt).cuda().requires_grad_()
    gd = None if g is None else g.to(dt).cuda().requires_grad_()
    run(xd, gd, k, sc, SIGMA_SPACE, border, dist).backward(gout.to(dt).cuda())
    return xd.grad.cpu(), (None if gd is None else gd.grad.cpu())


def _grad_err(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("kernel", GRAD_WINDOWS, ids=kname)
def test_gradients_against_the_reference(kernel, dist):
    d = fixture()
    x, g, gout = d["x__2x3x13x17"], d["g__2x3x13x17"], d["grad__gout"]
    worst = {torch.float32: 0.0, torch.float64: 0.0}
    for border in BORDERS:
        tag = f"{kname(kernel)}__{dist}__{border}"
        for dt in worst:
            gx, _ = _native_grads(x, None, kernel, 0.5, border, dist, gout, dt)
            jx, jg = _native_grads(x, g, kernel, 0.5, border, dist, gout, dt)
            assert gx.dtype == dt and jg.shape == g.shape
            for got, ref in ((gx, d[f"grad__self__{tag}__gx"]), (jx, d[f"grad__joint__{tag}__gx"]), (jg, d[f"grad__joint__{tag}__gg"])):
                worst[dt] = max(worst[dt], _grad_err(got, ref))
    print(f"bilateral gradients {kname(kernel)} {dist}: max error of the largest entry float32 {worst[torch.float32]:.3e} (bound {GRAD_BOUND:.0e}), "
          f"float64 {worst[torch.float64]:.3e}")
    assert worst[torch.float32] <= GRAD_BOUND and worst[torch.float64] <= 1e-12


@pytest.mark.parametrize("border", BORDERS)
def test_gradients_where_tiles_are_interior(border):
    """an image large enough for tiles that touch no border (the LDS path of the backward) beside the ones that do, against autograd through the
    restatement in float64; only one of the two gradients asked for gives the same bits as both"""
    h, w = 3 * TH + 5, 3 * TW + 7
    x, g = quantised((1, 3, h, w), 7), quantised((1, 2, h, w), 8)
    gout = torch.randn(1, 3, h, w, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    worst = 0.0
    for k, dist in ((5, "l1"), ((3, 7), "l2")):
        gx, _ = _native_grads(x, None, k, 0.5, border, dist, gout)
        jx, jg = _native_grads(x, g, k, 0.5, border, dist, gout)
        rx, _ = restate_grads(x, None, k, 0.5, SIGMA_SPACE, border, dist, gout)
        rjx, rjg = restate_grads(x, g, k, 0.5, SIGMA_SPACE, border, dist, gout)
        worst = max(worst, _grad_err(gx, rx), _grad_err(jx, rjx), _grad_err(jg, rjg))
        xd, gd = x.cuda().requires_grad_(), g.cuda()
        run(xd, gd, k, 0.5, SIGMA_SPACE, border, dist).backward(gout.float().cuda())
        assert torch.equal(xd.grad.cpu(), jx)
        xd, gd = x.cuda(), g.cuda().requires_grad_()
        run(xd, gd, k, 0.5, SIGMA_SPACE, border, dist).backward(gout.float().cuda())
        assert torch.equal(gd.grad.cpu(), jg)
    print(f"bilateral gradients, interior tiles, {border}: max error of the largest entry {worst:.3e}")
    assert worst <= GRAD_BOUND


@pytest.mark.parametrize("func", ["self", "joint"])
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("kernel", [(3, 3), (3, 5)], ids=kname)
def test_gradcheck_f64(kernel, dist, border, func):
    """sigma_color = 0.5 and a random float64 image (no exact ties between neighbours: the finite difference does not straddle the kink of |.|)"""
    gen = torch.Generator().manual_seed(13)
    x = torch.rand(1, 2, 6, 7, generator=gen, dtype=torch.float64).cuda().requires_grad_()
    if func == "self":
        assert torch.autograd.gradcheck(lambda t: KF().bilateral_blur(t, kernel, 0.5, SIGMA_SPACE, border, dist), (x,), eps=1e-6, atol=1e-7, rtol=1e-5)
    else:
        g = torch.rand(1, 3, 6, 7, generator=gen, dtype=torch.float64).cuda().requires_grad_()
        assert torch.autograd.gradcheck(lambda t, u: KF().joint_bilateral_blur(t, u, kernel, 0.5, SIGMA_SPACE, border, dist), (x, g), eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("dist", DISTS)
def test_gradient_at_exact_ties_is_zero_from_that_tap(dist):
    """A constant image: every tap ties with the centre in every channel, so the gradient through the weights is 0 (l1: sign(0) = 0 as torch's
    abs; l2: 2 delta = 0) and gx is the value gradient alone - what the joint form gives for the input with the same image as guidance.  Under
    `replicate` every tap reads a pixel, the weights of an output sum to its W, and so sum(gx) = sum(grad_out) up to rounding."""
    x = torch.full((2, 3, TH + 3, TW + 5), 0.375)
    gout = torch.randn(x.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    gx, _ = _native_grads(x, None, 5, 0.5, "replicate", dist, gout)
    jx, jg = _native_grads(x, x.clone(), 5, 0.5, "replicate", dist, gout)
    assert torch.equal(gx, jx) and torch.equal(jg, torch.zeros_like(jg))
    assert abs(gx.double().sum().item() - gout.float().double().sum().item()) <= 1e-5 * gout.abs().sum().item()


def test_backward_is_deterministic():
    x, g = quantised((2, 3, 2 * TH + 3, 2 * TW + 3), 4), quantised((2, 2, 2 * TH + 3, 2 * TW + 3), 5)
    gout = torch.randn(x.shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    a = _native_grads(x, g, 5, 0.1, "reflect", "l1", gout)
    b = _native_grads(x, g, 5, 0.1, "reflect", "l1", gout)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(_native_grads(x, None, 5, 0.1, "reflect", "l1", gout)[0], _native_grads(x, None, 5, 0.1, "reflect", "l1", gout)[0])


@pytest.mark.parametrize("which", ["nan", "inf"])
def test_non_finite_fixture_images(which):
    d = fixture()
    ref = d[f"nf_{which}__y"]
    out = KF().bilateral_blur(d[f"nf_{which}__x"].cuda(), (3, 3), 0.5, SIGMA_SPACE).cpu()
    assert torch.equal(torch.isnan(out), torch.isnan(ref)) and int(torch.isnan(out).sum()) == 9 and not bool(torch.isinf(out).any())
    assert (out - ref)[~torch.isnan(ref)].abs().max().item() <= F32_BOUND


def test_errors_and_scope():
    from kornia_amd import NativeLibraryError
    from kornia_amd.core.exceptions import ShapeError, TypeCheckError

    F = KF()
    d = fixture()
    assert list(d["raises__type"]) == ["RuntimeError", "RuntimeError", "ValueError"]
    x = torch.rand(1, 1, 8, 8).cuda()
    for k in (4, (3, 4)):
        with pytest.raises(RuntimeError):
            F.bilateral_blur(x, k, 0.5, SIGMA_SPACE)
    with pytest.raises(ValueError, match="color_distance_type only accepts l1 or l2"):
        F.bilateral_blur(x, (3, 3), 0.5, SIGMA_SPACE, "reflect", "l3")
    with pytest.raises(ShapeError):
        F.bilateral_blur(x[0], 3, 0.5, SIGMA_SPACE)
    with pytest.raises(TypeCheckError):
        F.bilateral_blur([[1.0]], 3, 0.5, SIGMA_SPACE)
    with pytest.raises(Exception, match="guidance and input should have the same batch size and spatial dimensions"):
        F.joint_bilateral_blur(x, torch.rand(1, 1, 8, 9).cuda(), 3, 0.5, SIGMA_SPACE)
    with pytest.raises(ShapeError):
        F.bilateral_blur(x, 3, torch.rand(1, 1).cuda(), SIGMA_SPACE)
    with pytest.raises(RuntimeError, match="Padding size"):  # (a reflect pad that does not fit: F.pad's own error in the reference)
        F.bilateral_blur(torch.rand(1, 1, 2, 8).cuda(), 5, 0.5, SIGMA_SPACE)
    with pytest.raises(NotImplementedError, match="15"):
        F.bilateral_blur(torch.rand(1, 1, 20, 20).cuda(), 17, 0.5, SIGMA_SPACE)
    with pytest.raises(NotImplementedError, match="16"):
        F.bilateral_blur(torch.rand(1, 17, 8, 8).cuda(), 3, 0.5, SIGMA_SPACE)
    with pytest.raises(NotImplementedError, match="16"):
        F.joint_bilateral_blur(x, torch.rand(1, 17, 8, 8).cuda(), 3, 0.5, SIGMA_SPACE)
    with pytest.raises(NotImplementedError, match="sigma"):
        F.bilateral_blur(x, 3, torch.tensor([0.5]).cuda().requires_grad_(), SIGMA_SPACE)
    with pytest.raises(NotImplementedError, match="sigma"):
        F.bilateral_blur(x, 3, 0.5, torch.tensor([[1.0, 1.0]]).cuda().requires_grad_())
    if x.device.type == "cuda":  # (the emulated device keeps tensors in host memory: there is no other kind of tensor there)
        with pytest.raises(NativeLibraryError):
            F.bilateral_blur(torch.rand(1, 1, 8, 8), 3, 0.5, SIGMA_SPACE)


def test_the_c_abi_refuses_what_the_header_says():
    from kornia_amd import _native as N

    x = torch.rand(1, 1, 8, 8).cuda()
    y = torch.empty_like(x)
    sp, co = torch.full((1, 289), 1 / 289.0).cuda(), torch.tensor([-2.0]).cuda()
    lib, st = N.lib(), N.stream_ptr(x.device)

    def fwd(C=1, ky=3, kx=3, border=0, H=8, W=8):
        return lib.km_bilateral_blur_fwd(x.data_ptr(), None, sp.data_ptr(), co.data_ptr(), y.data_ptr(), None, 1, C, C, H, W, 1, 1, ky, kx, border, 0, 0, st)

    assert fwd() == 0
    for kw, word in ((dict(ky=4), "odd"), (dict(kx=17, ky=17), "odd"), (dict(C=17), "channels"), (dict(border=1, ky=5, kx=5, H=2, W=32), "reflect")):
        assert fwd(**kw) < 0 and word in lib.km_last_error().decode()


def test_modules_int_windows_strides_and_empty_batches():
    F = KF()
    x, g = quantised((2, 3, 12, 17), 1), quantised((2, 2, 12, 17), 2)
    xd, gd = x.cuda(), g.cuda()
    assert torch.equal(F.BilateralBlur((5, 5), 0.1, SIGMA_SPACE, "replicate", "l2")(xd), F.bilateral_blur(xd, (5, 5), 0.1, SIGMA_SPACE, "replicate", "l2"))
    assert torch.equal(F.JointBilateralBlur(3, 0.5, SIGMA_SPACE)(xd, gd), F.joint_bilateral_blur(xd, gd, 3, 0.5, SIGMA_SPACE))
    assert torch.equal(F.bilateral_blur(xd, 5, 0.5, SIGMA_SPACE), F.bilateral_blur(xd, (5, 5), 0.5, SIGMA_SPACE))
    # strided and channels-last inputs are made contiguous
    xs, gs = xd[..., 1:], gd[..., 1:]
    assert not xs.is_contiguous()
    assert torch.equal(F.joint_bilateral_blur(xs, gs, 3, 0.5, SIGMA_SPACE), F.joint_bilateral_blur(xs.contiguous(), gs.contiguous(), 3, 0.5, SIGMA_SPACE))
    xl = xd.contiguous(memory_format=torch.channels_last)
    assert torch.equal(F.bilateral_blur(xl, 3, 0.5, SIGMA_SPACE), F.bilateral_blur(xd, 3, 0.5, SIGMA_SPACE))
    xg = xs.detach().requires_grad_()
    F.bilateral_blur(xg, 3, 0.5, SIGMA_SPACE).sum().backward()
    xc = xs.contiguous().requires_grad_()
    F.bilateral_blur(xc, 3, 0.5, SIGMA_SPACE).sum().backward()
    assert torch.equal(xg.grad, xc.grad)
    # B = 0: an empty tensor, no launch
    e = F.bilateral_blur(torch.empty(0, 3, 8, 8).cuda(), 3, 0.5, SIGMA_SPACE)
    assert e.shape == (0, 3, 8, 8)
    assert F.joint_bilateral_blur(torch.empty(0, 3, 8, 8).cuda(), torch.empty(0, 1, 8, 8).cuda(), 3, 0.5, SIGMA_SPACE).shape == (0, 3, 8, 8)
    # no autograd node when nothing needs a gradient
    assert not F.bilateral_blur(xd, 3, 0.5, SIGMA_SPACE).requires_grad
    with torch.no_grad():
        assert not F.bilateral_blur(xd.clone().requires_grad_(), 3, 0.5, SIGMA_SPACE).requires_grad


# =====================================================================================================================================
# the guarded cases of tests/test_gpu_written_outputs.py for km_bilateral_blur_fwd / _bwd: registered in its table at import (that file's
# `test_table` was parametrised before, so `test_guarded_cases` below runs them under both fills; its coverage test finds them in CASES).
# Every buffer the package allocates - y, wsum, gx, gguide - comes through the guard; the inputs are held unchanged.
def _guarded_case(dt, shape, k, border, dist, sc):
    B, C, H, W = shape
    x, g = quantised(shape, 21).to(dt), quantised((B, 2, H, W), 22).to(dt)
    gout = (torch.randint(-2, 3, shape, generator=torch.Generator().manual_seed(23)).float() / 2).to(dt)
    xd, gd, god = x.cuda(), g.cuda(), gout.cuda()
    res = {}
    with unchanged(xd, gd, god):
        y0 = run(xd, None, k, sc, SIGMA_SPACE, border, dist)  # (the forward alone: no wsum, no autograd node)
        xs = xd.detach().requires_grad_()
        ys = run(xs, None, k, sc, SIGMA_SPACE, border, dist)
        ys.backward(god)
        xj, gj = xd.detach().requires_grad_(), gd.detach().requires_grad_()
        yj = run(xj, gj, k, sc, SIGMA_SPACE, border, dist)
        yj.backward(god)
        xo = xd.detach().requires_grad_()
        run(xo, gd, k, sc, SIGMA_SPACE, border, dist).backward(god)  # gx alone
        go = gd.detach().requires_grad_()
        run(xd, go, k, sc, SIGMA_SPACE, border, dist).backward(god)  # gguide alone
    assert torch.equal(y0, ys.detach()) and torch.equal(xo.grad, xj.grad) and torch.equal(go.grad, gj.grad)
    if dt == torch.float32:
        assert (ys.detach().cpu() - restate(x, None, k, sc, SIGMA_SPACE, border, dist)).abs().max().item() <= F32_BOUND
        assert (yj.detach().cpu() - restate(x, g, k, sc, SIGMA_SPACE, border, dist)).abs().max().item() <= F32_BOUND
        rx, _ = restate_grads(x, None, k, sc, SIGMA_SPACE, border, dist, gout)
        rjx, rjg = restate_grads(x, g, k, sc, SIGMA_SPACE, border, dist, gout)
        assert max(_grad_err(xs.grad.cpu(), rx), _grad_err(xj.grad.cpu(), rjx), _grad_err(gj.grad.cpu(), rjg)) <= GRAD_BOUND
    else:
        assert same_bits(ys.detach().cpu(), run(xd.float(), None, k, sc, SIGMA_SPACE, border, dist).to(dt).cpu())
    res.update(y=ys.detach().cpu(), gx=xs.grad.cpu(), yj=yj.detach().cpu(), gxj=xj.grad.cpu(), gguide=gj.grad.cpu())
    return res


_GUARDED = [("f32-3x3-constant-l1", torch.float32, (2, 3, TH + 1, TW + 5), 3, "constant", "l1", 0.5),
            ("f32-5x5-reflect-l2-interior", torch.float32, (1, 3, 3 * TH + 5, 3 * TW + 7), 5, "reflect", "l2", 0.5),
            ("f32-3x7-circular-l1", torch.float32, (2, 1, 9, 37), (3, 7), "circular", "l1", 0.1),
            ("bf16-5x5-replicate-l1", torch.bfloat16, (2, 3, 13, 17), 5, "replicate", "l1", 0.5),
            ("f16-9x9-reflect-l2", torch.float16, (1, 4, 16, 24), 9, "reflect", "l2", 0.5)]
for _name, *_a in _GUARDED:
    case(f"bilateral-{_name}")(lambda oracle, a=tuple(_a): _guarded_case(*a))
# the coverage test of that file runs the cases it has not seen yet in the table's order until every entry point is met: put these ahead of
# the table's others, so that a process that has not run them here reaches them at once
_mine = {k: CASES.pop(k) for k in [k for k in CASES if k.startswith("bilateral-")]}
_rest = dict(CASES)
CASES.clear()
CASES.update(_mine)
CASES.update(_rest)


@pytest.mark.parametrize("name", [f"bilateral-{n[0]}" for n in _GUARDED])
def test_guarded_cases(oracle, name):
    """the case under both fills: its own assertions hold under each, the guard bands are intact (checked inside `guarded`), the inputs are
    unchanged, and the two runs agree bit for bit - every element was written and nothing was read first"""
    a, b = (_run_case(name, oracle, fill) for fill in FILLS)
    assert a.keys() == b.keys() and len(a) == 5
    for k in a:
        assert same_bits(a[k], b[k]), f"{k}: the results under the fills 0xFF and 0x7B differ - an element never written, or read before it was"
