"""GPU (and, through tests/test_emulated_aug_masks.py, the host build of the kernels): label masks, RandomPerspective and inverse() in
kornia_amd.augmentation's container, against what Kornia draws and returns for the same ``torch.manual_seed`` (tests/golden/aug_masks.npz,
tests/make_golden_aug_masks.py) and bit for bit against the compositions they replace:

* masks: ``warp_*(mask.to(image dtype), M, mode="nearest", ...).to(mask dtype)`` (the container's treatment of a mask, augment.py:596-618);
* km_perspective_params_chain_fwd: km_perspective_transform_fwd followed by km_homography_chain_fwd;
* inverse: the warp of the closed-form inverse of the forward matrix (km_inv3, restated below).  The reference inverts with torch.linalg.inv
  (kornia/core/utils.py:202-218): LAPACK's last bits differ from the closed form's, and a nearest sample flips where a coordinate lands on a
  rounding boundary - the fixture bounds below hold that difference."""
import pytest
import torch

from _util import golden

pytestmark = pytest.mark.gpu

MASK_DTYPES = [torch.bool, torch.uint8, torch.int32, torch.int64, torch.float32, torch.bfloat16, torch.float16]
IMG_DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _pipelines():
    import kornia_amd.augmentation as A

    return {
        "config3": (lambda: A.AugmentationSequential(A.RandomAffine(degrees=15.0, translate=(0.1, 0.1), scale=(0.8, 1.2), shear=5.0, p=1.0),
                                                     A.ColorJitter(0.2, 0.2, 0.2, 0.1, p=1.0), A.RandomGaussianBlur((5, 5), (0.1, 2.0), p=1.0),
                                                     data_keys=["input", "mask"]), torch.float32, 1),
        "persp_border": (lambda: A.AugmentationSequential(A.RandomPerspective(0.4, p=0.6),
                                                          A.RandomAffine(degrees=20.0, translate=(0.1, 0.1), scale=(0.9, 1.1), padding_mode="border", p=0.7),
                                                          data_keys=["input", "mask"]), torch.bfloat16, 1),
        "area_fill": (lambda: A.AugmentationSequential(A.RandomPerspective(0.5, sampling_method="area_preserving", p=0.8),
                                                       A.RandomAffine(degrees=25.0, shear=(-5.0, 5.0), padding_mode="fill", fill_value=0.3, p=0.7),
                                                       data_keys=["input", "mask", "mask"], same_on_batch=True), torch.float32, 2),
    }


# Bounds against Kornia, measured on the host build: fp32 pipelines - image <= 1.5e-5, masks and inverse masks identical, inverse image <= 2.6e-4
# (the fixture stores that image in float16: half an f16 ulp at 0.5 is 2.4e-4).  The bf16 pipeline is compared with Kornia's float32 run of
# the same draws (Kornia would warp a bf16 image with bf16 homographies - `.to(input)`, perspective.py:95 - where this package keeps float32
# matrices): the image within the suite's 16-bit bound, the masks against Kornia's float32 masks taken through bf16 (the
# container's round trip: int64 257 -> 256) within the nearest-sampling bound.
IMG_BOUND = {"config3": 2e-5, "persp_border": 1e-2, "area_fill": 2e-5}
INV_IMG_BOUND = {"config3": 1e-3, "persp_border": 1e-2, "area_fill": 1e-3}
MASK_FRAC = 2e-3


@pytest.mark.parametrize("seed", [3, 11])
@pytest.mark.parametrize("name", ["config3", "persp_border", "area_fill"])
def test_seeded_pipeline_with_masks_matches_the_reference(name, seed):
    d = {k: torch.from_numpy(v) for k, v in golden("aug_masks").items()}
    make, dt, nm = _pipelines()[name]
    key = f"{name}__seed{seed}"
    masks = [d[f"{name}__mask{i}"].cuda() for i in range(nm)]
    torch.manual_seed(seed)
    aug = make()
    outs = aug(d["x"].to(dt).cuda(), *masks)
    assert torch.equal(torch.get_rng_state()[:64], d[key + "__rng_after"])
    n = 0
    for item in aug._params:
        for k, v in item.data.items():
            if isinstance(v, torch.Tensor):
                ref = d[f"{key}__{item.name}__{k}"]
                assert v.shape == ref.shape and torch.equal(v.to(ref.dtype), ref), (item.name, k)
                n += 1
    assert n >= 8
    assert outs[0].dtype == dt
    out = outs[0].float().cpu()
    ref = d[key + "__out"].float()
    assert (out - ref).abs().max().item() <= IMG_BOUND[name], (out - ref).abs().max().item()

    def through(t):  # Kornia's float32-image mask taken through the image dtype of this run
        return t if dt == torch.float32 else t.to(dt).to(t.dtype)

    for i in range(nm):
        mo, mr = outs[1 + i].cpu(), through(d[f"{key}__mask{i}"])
        assert mo.dtype == mr.dtype and mo.shape == mr.shape
        frac = (mo != mr).float().mean().item()
        assert frac <= MASK_FRAC, (i, frac)
    inv = aug.inverse(*outs)
    for i in range(nm):
        mi, mr = inv[1 + i].cpu(), through(d[f"{key}__inv_mask{i}"])
        assert mi.dtype == mr.dtype and (mi != mr).float().mean().item() <= MASK_FRAC, (i, (mi != mr).float().mean().item())
    if seed == 3:
        err = (inv[0].float().cpu() - d[key + "__inv_out"].float()).abs().max().item()
        assert err <= INV_IMG_BOUND[name], err


def _affine_and_persp(B, H, W, seed):
    import kornia_amd.augmentation as A

    torch.manual_seed(seed)
    return [A.RandomAffine(degrees=30.0, translate=(0.1, 0.2), scale=(0.8, 1.2), shear=8.0, padding_mode=pad, fill_value=0.7, p=0.6)
            for pad in ("zeros", "border", "reflection", "fill")] + [A.RandomPerspective(0.5, p=0.6), A.RandomPerspective(0.3, resample="nearest", p=1.0)]


@pytest.mark.parametrize("img_dtype", IMG_DTYPES)
def test_masks_are_the_native_composition_bit_for_bit(img_dtype):
    import kornia_amd as K
    import kornia_amd.augmentation as A

    B, H, W = 3, 21, 30
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, 3, H, W, generator=g).to(img_dtype).cuda()
    labels = torch.randint(-3, 300, (B, 2, H, W), generator=g)
    labels[0, 0, :2] = 257  # (257 -> 256 through bfloat16: the reference's round trip)
    for mod in _affine_and_persp(B, H, W, 7):
        for mdt in MASK_DTYPES:
            mk = (labels > 100) if mdt == torch.bool else (labels.to(mdt) / 7).to(mdt) if mdt.is_floating_point else labels.clamp(min=0 if mdt == torch.uint8 else -3).to(mdt)
            mk = mk.cuda()
            seq = A.AugmentationSequential(mod, data_keys=["mask", "input"])
            mo, xo = seq(mk, x)
            M = mod.transform_matrix
            fill = torch.full((2,), 0.7) if mod.padding_mode == "fill" else None
            warp = K.warp_affine if isinstance(mod, A.RandomAffine) else K.warp_perspective
            Mw = M[:, :2, :] if isinstance(mod, A.RandomAffine) else M
            ref = warp(mk.to(img_dtype), Mw, (H, W), mode="nearest", padding_mode=mod.padding_mode, align_corners=False, fill_value=fill).to(mdt)
            keep = (seq._params[0].data["batch_prob"] > 0.5).cuda().view(-1, 1, 1, 1)
            ref = torch.where(keep, ref, mk.to(img_dtype).to(mdt))  # (a sample whose draw failed: the round trip alone, as in the reference)
            assert mo.dtype == mdt and torch.equal(mo, ref), (type(mod).__name__, mod.padding_mode, mdt, (mo != ref).sum().item())
            # the pair launch's image is the image-only pipeline's image; a replay of the parameters gives the same masks
            assert torch.equal(xo, A.AugmentationSequential(mod)(x, params=seq._params))
            mo2, xo2 = A.AugmentationSequential(mod, data_keys=["mask", "input"])(mk, x, params=seq._params)
            assert torch.equal(mo2, mo) and torch.equal(xo2, xo)
    if img_dtype == torch.bfloat16:
        m64 = torch.full((1, 1, 4, 4), 257, dtype=torch.int64).cuda()
        m64[0, 0, 0] = 300
        out, o64 = A.AugmentationSequential(A.RandomAffine(0.0, p=1.0), data_keys=["input", "mask"])(x[:1, :, :4, :4].contiguous(), m64)
        assert o64[0, 0, 0].tolist() == [300] * 4 and o64[0, 0, 1].tolist() == [256] * 4


def test_perspective_chain_is_the_two_launch_path():
    from kornia_amd import _native as N
    import kornia_amd.augmentation as A

    B, H, W = 37, 50, 70
    torch.manual_seed(2)
    mod = A.RandomPerspective(0.6, p=0.5)
    params = mod.forward_parameters((B, 3, H, W))
    dev = torch.device("cuda")
    m, M, apply = A.perspective_chain(params, dev, H, W, with_matrix=True)
    sp, ep = params["start_points"].cuda().contiguous(), params["end_points"].cuda().contiguous()
    M2 = torch.empty(B, 3, 3, device=dev)
    m2 = torch.empty(B, 9, device=dev)
    N.check(N.lib().km_perspective_transform_fwd(sp.data_ptr(), ep.data_ptr(), M2.data_ptr(), B, 0, N.stream_ptr(dev)), "pt")
    N.check(N.lib().km_homography_chain_fwd(M2.data_ptr(), 3, None, m2.data_ptr(), B, H, W, H, W, 0, N.stream_ptr(dev)), "chain")
    assert torch.equal(M, M2) and torch.equal(m, m2)
    assert torch.equal(apply.cpu().bool(), params["batch_prob"] > 0.5)


def _inv3(M: torch.Tensor) -> torch.Tensor:
    """km_inv3 (kornia_amd/csrc/km_chain.hip) restated: columns a, b, c; rows of the inverse = cross products / det, cross products as
    fma(a1, b2, -(a2 b1)) - float64 products of float32 operands are exact, so the fma is one float32 rounding."""
    M = M.float().cpu()
    a, b, c = M[:, :, 0], M[:, :, 1], M[:, :, 2]

    def cross(u, v):
        def f(p, q, r, s):  # fma(p, q, -(r * s))
            t = (r * s)  # float32 product
            return (p.double() * q.double() - t.double()).float()
        return torch.stack([f(u[:, 1], v[:, 2], u[:, 2], v[:, 1]), f(u[:, 2], v[:, 0], u[:, 0], v[:, 2]), f(u[:, 0], v[:, 1], u[:, 1], v[:, 0])], 1)

    r0, r1, r2 = cross(b, c), cross(c, a), cross(a, b)
    det = (a[:, 0] * r0[:, 0] + a[:, 1] * r0[:, 1]) + a[:, 2] * r0[:, 2]
    return torch.stack([r0 / det[:, None], r1 / det[:, None], r2 / det[:, None]], 1)


def test_inverse_is_the_closed_form_composition_bit_for_bit():
    import kornia_amd as K
    import kornia_amd.augmentation as A

    B, H, W = 4, 33, 47
    g = torch.Generator().manual_seed(9)
    x = torch.rand(B, 3, H, W, generator=g).cuda()
    mk = torch.randint(0, 50, (B, 1, H, W), generator=g, dtype=torch.uint8).cuda()
    for mod in _affine_and_persp(B, H, W, 13):
        seq = A.AugmentationSequential(mod, data_keys=["input", "mask"])
        y, ym = seq(x, mk)
        xi, mi = seq.inverse(y, ym)
        Minv = _inv3(mod.transform_matrix).cuda()
        affine = isinstance(mod, A.RandomAffine)
        warp = K.warp_affine if affine else K.warp_perspective
        Mw = Minv[:, :2, :] if affine else Minv
        fill = torch.full((3,), 0.7) if mod.padding_mode == "fill" else None
        keep = (seq._params[0].data["batch_prob"] > 0.5).cuda().view(-1, 1, 1, 1)
        ref = warp(y, Mw, (H, W), mode=mod.resample, padding_mode=mod.padding_mode, align_corners=False, fill_value=fill)
        refm = warp(ym.float(), Mw, (H, W), mode="nearest", padding_mode=mod.padding_mode, align_corners=False,
                    fill_value=torch.full((1,), 0.7) if fill is not None else None).to(torch.uint8)
        assert torch.equal(xi, torch.where(keep, ref, y)), type(mod).__name__
        assert torch.equal(mi, torch.where(keep, refm, ym)), type(mod).__name__
        # the module-level inverse of the image is the container's
        assert torch.equal(mod.inverse(y), xi)


def test_errors():
    import kornia_amd.augmentation as A

    x = torch.rand(2, 3, 8, 8).cuda()
    with pytest.raises(NotImplementedError):
        A.AugmentationSequential(A.RandomAffine(10.0), data_keys=["input", "keypoints"])
    with pytest.raises(NotImplementedError):
        A.AugmentationSequential(A.RandomAffine(10.0), data_keys=["input", "bbox_xyxy"])
    with pytest.raises(NotImplementedError):
        A.AugmentationSequential(A.RandomAffine(10.0), data_keys=["input", "mask"], random_apply=1)
    seq = A.AugmentationSequential(A.RandomPerspective(0.3), data_keys=["input", "mask"])
    with pytest.raises(ValueError):
        seq.inverse(x, torch.zeros(2, 1, 8, 8).cuda())  # nothing to invert yet
    with pytest.raises(ValueError):
        seq(x, torch.zeros(3, 1, 8, 8).cuda())
    with pytest.raises(ValueError):
        seq(x, torch.zeros(2, 1, 8, 9).cuda())
    with pytest.raises(NotImplementedError):
        seq(x, [torch.zeros(2, 1, 8, 8).cuda()])
    with pytest.raises(NotImplementedError):  # masks need a geometric child, also when data_keys is given with the call
        A.AugmentationSequential(A.ColorJitter(0.1))(x, torch.zeros(2, 1, 8, 8).cuda(), data_keys=["input", "mask"])
    with pytest.raises(NotImplementedError):
        A.RandomPerspective(0.3, sampling_method="other")
    with pytest.raises(AssertionError):
        A.RandomPerspective(1.5)
    # an unbatched image with an unbatched mask
    y, ym = A.AugmentationSequential(A.RandomPerspective(0.3, p=1.0), data_keys=["input", "mask"])(x[0], torch.ones(1, 8, 8, dtype=torch.bool).cuda())
    assert y.shape == (1, 3, 8, 8) and ym.shape == (1, 1, 8, 8) and ym.dtype == torch.bool


@pytest.mark.parametrize("img_dtype", IMG_DTYPES)
def test_one_launch_and_two_launch_pair_are_the_same(img_dtype):
    """km_warp2d_pair_fwd as one launch (km_warp_pair_kernel) and as two (the image's own forward + the mask kernel): the same bits, for every
    padding, both interpolations, both coordinate generators, with and without the switch, one and three mask channels."""
    from kornia_amd import _native as N
    import kornia_amd.augmentation as A

    B, H, W = 3, 19, 33
    g = torch.Generator().manual_seed(21)
    x = torch.rand(B, 3, H, W, generator=g).to(img_dtype).cuda()
    lab = torch.randint(0, 300, (B, 3, H, W), generator=g)
    lib = N.lib()
    prev = lib.km_config_set(b"pair_fused", 1)
    try:
        for mod in _affine_and_persp(B, H, W, 17) + [A.RandomAffine(20.0, resample="nearest", padding_mode="reflection", p=0.5)]:
            params = mod.forward_parameters((B, 3, H, W))
            p = mod._device_params(params, x.device, False)
            m, _, apply = mod._chain(p, x.device, H, W)
            for mk in (lab[:, :1].to(torch.uint8).cuda(), lab.cuda(), (lab[:, :2] > 150).cuda()):
                kw = dict(affine=mod._AFFINE, resample=mod.resample, padding_mode=mod.padding_mode, fill_value=0.7, apply=apply)
                res = []
                for fused in (1, 0):
                    lib.km_config_set(b"pair_fused", fused)
                    res.append(A.warp_pair(x, mk, m, **kw))
                assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), (type(mod).__name__, mod.padding_mode, mk.dtype)
    finally:
        lib.km_config_set(b"pair_fused", prev)


def test_many_mask_planes():
    """B * Cm above the 65535 of one grid dimension (one-hot masks of a large batch)."""
    import kornia_amd.augmentation as A

    B, Cm, H, W = 2, 40000, 2, 3
    mk = (torch.arange(B * Cm * H * W) % 3 == 0).view(B, Cm, H, W).cuda()
    m = torch.tensor([[1.0, 0, 0, 0, 1, 0, 0, 0, 1]]).repeat(B, 1).cuda()
    _, mo = A.warp_pair(None, mk, m, True, resample="nearest", image_dtype=torch.float32)
    assert torch.equal(mo, mk)  # (the identity: linspace base grid of warp_affine, align_corners=False)
