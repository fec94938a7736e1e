"""GPU (and, through tests/test_emulated_median.py, the host build of the kernels): median_blur, MedianBlur and RandomMedianBlur on the native
path (km_median_blur_fwd / _bwd) against the reference's recorded outputs (tests/golden/median_blur.npz) and, for the shapes the fixture does not
hold, against the restatement that tests/test_median_golden.py anchors to it.  Selection is exact in every dtype: every forward comparison
is ``torch.equal``; gradients are compared with integer ``grad_out``, for which every order of summation is exact."""
import pytest
import torch

from test_median_golden import DTYPES, GRAD_KERNELS, KERNELS, SHAPES, fixture, kname, restate, restate_grad, sname

pytestmark = pytest.mark.gpu

STRIP = 32  # rows of a wave's strip in the register-tiled kernel (KMM_ROWS, csrc/km_median.hip)
# register-kernel edges: every H at one width and every W at one height (W = 4: one lane with both halos in the padding; 260: a row wider
# than one wave's 256 columns; H < K, the strip seams), one shape with both large, and two widths that no lane tiles
EDGE_SHAPES = ([(h, 12) for h in (1, 2, 4, STRIP - 1, STRIP, STRIP + 1, 2 * STRIP + 3)] + [(STRIP + 1, w) for w in (4, 8, 260)]
               + [(2 * STRIP + 3, 260), (9, 5), (9, 7)])


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal with NaN equal to NaN"""
    a, b = a.cpu(), b.cpu()
    return a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))


def unaligned(x: torch.Tensor) -> torch.Tensor:
    """x on the device as a contiguous tensor that starts one element past an aligned address: the register kernels refuse it (rows must be
    16-byte aligned), so the generic kernel runs"""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype).cuda()
    view = buf[1:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 8 != 0
    return view


def quantised(shape, seed, levels=128):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-levels, levels + 1, shape, generator=g).float() / 64


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("kernel", KERNELS, ids=kname)
def test_parity_with_the_reference(kernel, dname):
    import kornia_amd.filters as KF

    d = fixture()
    for shape in SHAPES:
        x = d[f"x__{sname(shape)}"].to(DTYPES[dname])
        ref = d[f"y__{sname(shape)}__{kname(kernel)}__{dname}"].to(DTYPES[dname])
        out = KF.median_blur(x.cuda(), kernel)
        assert out.shape == x.shape and out.dtype == x.dtype and torch.equal(out.cpu(), ref), (shape, kernel, dname)
    if kernel[0] == kernel[1]:  # an int is the square window; the module form
        x = d[f"x__{sname(SHAPES[3])}"].to(DTYPES[dname]).cuda()
        assert torch.equal(KF.MedianBlur(kernel[0])(x), KF.median_blur(x, kernel))


@pytest.mark.parametrize("dname", ["f32", "bf16"])
@pytest.mark.parametrize("k", [3, 5])
def test_register_kernel_edges(k, dname):
    """Full-precision random images (normal values: ties are rare in f32, common in bf16): the register kernel, the generic kernel on an
    unaligned copy of the same image, and the restatement agree bit for bit."""
    import kornia_amd.filters as KF

    g = torch.Generator().manual_seed(77 + k)
    for h, w in EDGE_SHAPES:
        x = torch.randn(2, 3, h, w, generator=g).to(DTYPES[dname])  # B C = 6: the plane strides
        want, _ = restate(x, k)
        fast = KF.median_blur(x.cuda(), k)
        assert torch.equal(fast.cpu(), want), (h, w)
        slow = KF.median_blur(unaligned(x), k)
        assert torch.equal(slow, fast), (h, w)


@pytest.mark.parametrize("dname", ["f32", "bf16"])
@pytest.mark.parametrize("k", [3, 5])
def test_strided_inputs(k, dname):
    import kornia_amd.filters as KF

    x = torch.randn(2, 3, 12, 17, generator=torch.Generator().manual_seed(5)).to(DTYPES[dname])
    xs = x.cuda()[..., 1:]  # a column slice: W = 16, rows start one element past the allocation's
    assert not xs.is_contiguous()
    assert torch.equal(KF.median_blur(xs, k).cpu(), restate(x[..., 1:], k)[0])
    xl = x.cuda().contiguous(memory_format=torch.channels_last)
    out = KF.median_blur(xl, k)
    assert torch.equal(out.cpu(), restate(x, k)[0])


def _ties_image():
    g = torch.Generator().manual_seed(31)
    return (torch.randint(0, 8, (2, 3, STRIP + 1, 24), generator=g).float() - 3).to(torch.bfloat16)  # 8 distinct values, zero among them


@pytest.mark.parametrize("kernel", [(3, 3), (5, 5), (3, 5)], ids=kname)
@pytest.mark.parametrize("path", ["aligned", "unaligned"])
def test_ties_follow_the_first_position_rule(path, kernel):
    import kornia_amd.filters as KF

    x = _ties_image()
    gout = torch.randint(-2, 3, x.shape, generator=torch.Generator().manual_seed(32)).to(torch.bfloat16)
    xd = (x.cuda() if path == "aligned" else unaligned(x)).requires_grad_()
    y = KF.median_blur(xd, kernel)
    assert torch.equal(y.detach().cpu(), restate(x, kernel)[0])
    y.backward(gout.cuda())
    want, routed = restate_grad(x, kernel, gout)
    assert torch.equal(xd.grad.cpu(), want)
    # what is not routed into the padding arrives: sum of x.grad == sum of grad_out over the outputs whose median is no padding zero
    assert not bool(routed.all())
    assert xd.grad.double().sum().item() == gout.double()[routed].sum().item()


@pytest.mark.parametrize("dname", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("kernel", GRAD_KERNELS, ids=kname)
def test_tie_free_gradient_equals_the_reference(kernel, dname):
    import kornia_amd.filters as KF

    d = fixture()
    dt = DTYPES[dname]
    x = d["grad__x"].to(dt).cuda().requires_grad_()
    assert torch.equal(x.detach().cpu().float(), d["grad__x"])  # 1 .. 240 are exact in every dtype
    KF.median_blur(x, kernel).backward(d["grad__gout"].to(dt).cuda())
    assert x.grad.dtype == dt and torch.equal(x.grad.cpu().float(), d[f"grad__{kname(kernel)}"])


@pytest.mark.parametrize("kernel", [(3, 3), (3, 5)], ids=kname)
def test_gradcheck_f64(kernel):
    import kornia_amd.filters as KF

    x = (torch.randperm(42, generator=torch.Generator().manual_seed(9)).double() + 1).view(1, 1, 6, 7).cuda().requires_grad_()
    assert torch.autograd.gradcheck(lambda t: KF.median_blur(t, kernel), (x,), eps=1e-3, atol=1e-9, rtol=0)


def test_backward_is_deterministic():
    import kornia_amd.filters as KF

    x = _ties_image().float()
    gout = torch.randn(x.shape, generator=torch.Generator().manual_seed(4)).cuda()
    grads = []
    for _ in range(2):
        xd = x.cuda().requires_grad_()
        KF.median_blur(xd, 5).backward(gout)
        grads.append(xd.grad.clone())
    assert torch.equal(grads[0], grads[1])


@pytest.mark.parametrize("which", ["nan", "inf"])
def test_non_finite_fixture_images(which):
    import kornia_amd.filters as KF

    d = fixture()
    out = KF.median_blur(d[f"nf_{which}__x"].cuda(), (3, 3))
    assert same(out, d[f"nf_{which}__y"]) and int(torch.isnan(out).sum()) == 4


@pytest.mark.parametrize("dname", ["f32", "bf16", "f64"])
@pytest.mark.parametrize("k", [5, 3])
def test_inf_at_a_corner(k, dname):
    import kornia_amd.filters as KF

    x = quantised((1, 2, 9, 12), 8).to(DTYPES[dname])
    x[0, 0, 0, 0] = float("inf")
    x[0, 1, 8, 11] = float("-inf")
    x[0, 1, 4, 5] = float("nan")
    want, _ = restate(x, k)
    r = k // 2 + 1
    assert int(torch.isnan(want).sum()) == 2 * r * r + k * k  # the r x r pixels nearest each corner, the k x k around the NaN
    assert same(KF.median_blur(x.cuda(), k), want)
    if dname != "f64":
        assert same(KF.median_blur(unaligned(x), k), want)
    assert same(KF.median_blur(x.cuda(), (1, 1)), x)  # n == 1: the identity, inf and NaN included


def test_errors():
    import kornia_amd.filters as KF
    from kornia_amd import NativeLibraryError
    from kornia_amd.core.exceptions import ShapeError, TypeCheckError

    d = fixture()
    x = torch.zeros(1, 1, 6, 6).cuda()
    for k, name in zip(d["even__kernels"].tolist(), d["even__raises"]):
        assert name == "RuntimeError"
        with pytest.raises(RuntimeError):
            KF.median_blur(x, tuple(k))
    with pytest.raises(RuntimeError):
        KF.median_blur(x, 4)
    with pytest.raises(ShapeError):
        KF.median_blur(x[0], 3)
    with pytest.raises(TypeCheckError):
        KF.median_blur([[1.0]], 3)
    with pytest.raises(NotImplementedError, match="15"):
        KF.median_blur(x, 17)
    with pytest.raises(NotImplementedError, match="15"):
        KF.median_blur(x, (3, 17))
    if x.device.type == "cuda":  # (the emulated device keeps tensors in host memory: there is no other kind of tensor there)
        with pytest.raises(NativeLibraryError):
            KF.median_blur(torch.zeros(1, 1, 6, 6), 3)


@pytest.mark.parametrize("seed", [3, 11])
def test_random_median_blur_matches_the_reference_draws(seed):
    import kornia_amd.augmentation as A

    d = fixture()
    x = d["aug__x"].cuda()
    torch.manual_seed(seed)
    aug = A.RandomMedianBlur((3, 3), p=0.5)
    out = aug(x)
    bp = d[f"rmb__seed{seed}__batch_prob"]
    assert torch.equal(torch.get_rng_state()[:64], d[f"rmb__seed{seed}__rng_after"])
    assert torch.equal(aug._params["batch_prob"].to(bp.dtype), bp)
    assert seed == 3 or 0 < int((bp > 0.5).sum()) < 5  # (seed 3 transforms all five samples, seed 11 three of them)
    want = torch.where((bp > 0.5).view(-1, 1, 1, 1), restate(d["aug__x"], 3)[0], d["aug__x"])
    assert torch.equal(out.cpu(), want) and torch.equal(out.cpu(), d[f"rmb__seed{seed}__out"])
    # replay, inverse, the unaligned (generic) kernel with the same switch
    assert torch.equal(aug(x, params=aug._params), out)
    assert torch.equal(A.RandomMedianBlur((3, 3), p=0.5)(unaligned(d["aug__x"]), params=aug._params), out)
    # p = 1 and p = 0 draw nothing
    state = torch.get_rng_state()
    assert torch.equal(A.RandomMedianBlur(p=1.0)(x).cpu(), restate(d["aug__x"], 3)[0]) and torch.equal(A.RandomMedianBlur(p=0.0)(x), x)
    assert torch.equal(torch.get_rng_state(), state)


# The container case against Kornia: the warp's bound, scaled.  tests/test_gpu_aug_masks.py holds RandomAffine pipelines on [0, 1] images to 2e-5
# of Kornia's output; the error of a bilinear warp is proportional to the values it blends, this image spans [-2, 2] (4 x the range), and a
# median is non-expansive in the maximum norm (|med(a) - med(b)| <= max |a - b|), so the filter adds nothing: 8e-5.  Masks: that file's 2e-3.
SEQ_IMG_BOUND = 8e-5
SEQ_MASK_FRAC = 2e-3


@pytest.mark.parametrize("seed", [3, 11])
def test_container_with_a_mask(seed):
    import kornia_amd.augmentation as A

    d = fixture()
    x, mk = d["aug__x"].cuda(), d["aug__mask"].cuda()
    key = f"seq__seed{seed}"

    def affine():
        return A.RandomAffine(degrees=15.0, translate=(0.1, 0.1), scale=(0.8, 1.2), p=0.7)

    torch.manual_seed(seed)
    seq = A.AugmentationSequential(affine(), A.RandomMedianBlur((5, 5)), data_keys=["input", "mask"])
    out, mout = seq(x, mk)
    assert torch.equal(torch.get_rng_state()[:64], d[key + "__rng_after"])
    n = 0
    for item in seq._params:
        for k, v in item.data.items():
            if isinstance(v, torch.Tensor):
                ref = d[f"{key}__{item.name}__{k}"]
                assert v.shape == ref.shape and torch.equal(v.to(ref.dtype), ref), (item.name, k)
                n += 1
    assert n >= 8 and seq._params[1].name == "RandomMedianBlur_1"
    err = (out.cpu() - d[key + "__out"]).abs().max().item()
    assert err <= SEQ_IMG_BOUND, err
    assert mout.dtype == mk.dtype and (mout.cpu() != d[key + "__mask_out"]).float().mean().item() <= SEQ_MASK_FRAC
    # the child leaves the mask alone and filters exactly what the affine child handed it; its inverse is the identity
    only = A.AugmentationSequential(affine(), data_keys=["input", "mask"])
    warped, mwarped = only(x, mk, params=seq._params[:1])
    assert torch.equal(mout, mwarped)
    bp = seq._params[1].data["batch_prob"]
    assert torch.equal(out.cpu(), torch.where((bp > 0.5).view(-1, 1, 1, 1), restate(warped.cpu(), 5)[0], warped.cpu()))
    xi, mi = seq.inverse(out, mout)
    xo, mo = only.inverse(out, mout, params=seq._params[:1])
    assert torch.equal(xi, xo) and torch.equal(mi, mo)
    with pytest.raises(NotImplementedError, match="RandomMedianBlur"):
        A.AugmentationSequential(torch.nn.Identity())


def test_gradient_through_the_module():
    import kornia_amd.augmentation as A

    d = fixture()
    x0 = d["grad__x"].repeat(3, 1, 1, 1)[:5]  # B = 5, tie-free channels
    gout = torch.randint(-2, 3, x0.shape, generator=torch.Generator().manual_seed(2)).float()
    torch.manual_seed(11)  # (three of the five samples are transformed)
    aug = A.RandomMedianBlur((3, 3), p=0.5)
    x = x0.cuda().requires_grad_()
    y = aug(x)
    on = aug._params["batch_prob"] > 0.5
    assert 0 < int(on.sum()) < 5
    y.backward(gout.cuda())
    want = torch.where(on.view(-1, 1, 1, 1), restate_grad(x0, 3, gout)[0], gout)
    assert torch.equal(x.grad.cpu(), want)
