"""GPU (and, through tests/test_emulated_aug_crop.py, the host build of the kernels): RandomResizedCrop, RandomHorizontalFlip, RandomVerticalFlip
and crop_by_indices on the native path (km_crop_resize_fwd), against what Kornia draws and returns for the same ``torch.manual_seed``
(tests/golden/aug_crop.npz, tests/make_golden_aug_crop.py) and bit for bit against the package's own per-sample composition:
slice -> ``resize_bilinear`` (masks: ``F.interpolate(mode="nearest")``) -> ``torch.flip`` / ``select_samples``."""
import pytest
import torch
import torch.nn.functional as F

from _util import golden

pytestmark = pytest.mark.gpu

IMG_DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _pipelines():
    import kornia_amd.augmentation as A

    return {
        "rrc_hflip_jitter": (lambda: A.AugmentationSequential(A.RandomResizedCrop((24, 32)), A.RandomHorizontalFlip(), A.ColorJitter(0.2, 0.2, 0.2, 0.1, p=1.0),
                                                              data_keys=["input", "mask"]), torch.float32, False),
        "rrc_same_vflip": (lambda: A.AugmentationSequential(A.RandomResizedCrop((24, 32), scale=(0.3, 1.0), ratio=(0.5, 2.0), same_on_batch=True),
                                                            A.RandomVerticalFlip(p=0.7), data_keys=["input", "mask"]), torch.bfloat16, False),
        "rrc_resample_affine": (lambda: A.AugmentationSequential(A.RandomResizedCrop((24, 32), cropping_mode="resample"),
                                                                 A.RandomAffine(degrees=20.0, translate=(0.1, 0.1), scale=(0.9, 1.1), p=0.7),
                                                                 data_keys=["input", "mask"]), torch.float32, True),
        "flips": (lambda: A.AugmentationSequential(A.RandomHorizontalFlip(), A.RandomVerticalFlip(p=0.5), data_keys=["input", "mask"]), torch.float32, True),
    }


# Bounds against Kornia, measured on the host build (max |error|): the fp32 slice pipeline (bilinear resize of the window, flip, ColorJitter)
# 9.6e-7; the resample crop + affine 6.3e-6 (two warps; Kornia's matrices come from torch.linalg.solve / inv) and its inverse 2.5e-4 (the
# fixture stores it in float16: half an f16 ulp at 0.5 is 2.4e-4); the direct crop_by_indices cases 2.4e-7 (bilinear), 0 (copy, pad,
# nearest); every mask identical.  The bf16 pipeline (3.9e-3) is compared with Kornia's float32 run of the same draws, its masks against
# Kornia's float32 masks taken through bf16 (int64 257 -> 256).
IMG_BOUND = {"rrc_hflip_jitter": 2e-6, "rrc_same_vflip": 1e-2, "rrc_resample_affine": 2e-5}
INV_IMG_BOUND = {"rrc_resample_affine": 1e-3}
MASK_FRAC = {"rrc_hflip_jitter": 0.0, "rrc_same_vflip": 0.0, "rrc_resample_affine": 2e-3, "flips": 0.0}


def _golden():
    return {k: torch.from_numpy(v) for k, v in golden("aug_crop").items()}


@pytest.mark.parametrize("seed", [3, 11])
@pytest.mark.parametrize("name", ["rrc_hflip_jitter", "rrc_same_vflip", "rrc_resample_affine", "flips"])
def test_seeded_pipeline_matches_the_reference(name, seed):
    d = _golden()
    make, dt, inverse = _pipelines()[name]
    key = f"{name}__seed{seed}"
    x = d["x"].to(dt).cuda()
    mk = d[f"{name}__mask"].cuda()
    torch.manual_seed(seed)
    aug = make()
    out, mout = aug(x, mk)
    assert torch.equal(torch.get_rng_state()[:64], d[key + "__rng_after"])
    n = 0
    for item in aug._params:
        for k, v in item.data.items():
            if isinstance(v, torch.Tensor):
                ref = d[f"{key}__{item.name}__{k}"]
                assert v.shape == ref.shape and torch.equal(v.to(ref.dtype), ref), (item.name, k)
                n += 1
    assert n >= 4
    assert out.dtype == dt and mout.dtype == mk.dtype
    if name == "flips":
        # Kornia's output rebuilt from its parameters: flips are exact
        ph = d[f"{key}__RandomHorizontalFlip_0__batch_prob"] > 0.5
        pv = d[f"{key}__RandomVerticalFlip_1__batch_prob"] > 0.5
        ref, refm = d["x"].clone(), d[f"{name}__mask"].clone()
        for t in (ref, refm):
            t[ph] = t[ph].flip(-1)
            t[pv] = t[pv].flip(-2)
        assert torch.equal(out.cpu(), ref) and torch.equal(mout.cpu(), refm)
        xi, mi = aug.inverse(out, mout)
        assert torch.equal(xi, x) and torch.equal(mi, mk)
        return
    err = (out.float().cpu() - d[key + "__out"].float()).abs().max().item()
    assert err <= IMG_BOUND[name], err

    def through(t):  # Kornia's float32-image mask taken through the image dtype of this run
        return t if dt == torch.float32 else t.to(dt).to(t.dtype)

    mr = through(d[key + "__mask_out"])
    assert mout.shape == mr.shape and (mout.cpu() != mr).float().mean().item() <= MASK_FRAC[name]
    if inverse:
        xi, mi = aug.inverse(out, mout)
        assert xi.shape == x.shape and mi.shape == mk.shape
        assert (mi.cpu() != d[key + "__inv_mask"]).float().mean().item() <= MASK_FRAC[name]
        if seed == 3:
            e = (xi.float().cpu() - d[key + "__inv_out"].float()).abs().max().item()
            assert e <= INV_IMG_BOUND[name], e
    else:
        with pytest.raises(NotImplementedError):
            aug.inverse(out, mout)


def test_affine_after_the_crop_samples_at_the_crop_size():
    import kornia_amd.augmentation as A

    torch.manual_seed(0)
    aug = A.AugmentationSequential(A.RandomResizedCrop((224, 224), cropping_mode="resample"), A.RandomAffine(10.0, p=1.0))
    y = aug(torch.rand(2, 3, 256, 300).cuda())
    assert y.shape == (2, 3, 224, 224)
    assert aug._params[1].data["center"].tolist() == [[111.5, 111.5]] * 2
    assert aug._params[1].data["forward_input_shape"].tolist() == [2, 3, 224, 224]


@pytest.mark.parametrize("name", ["boxes", "boxes_ac_true", "boxes_ac_false", "same_pad", "equal", "pad", "size_none", "nearest"])
def test_crop_by_indices_matches_the_reference(name):
    from kornia_amd.geometry.transform import crop_by_indices

    import make_golden_aug_crop as M

    d = _golden()
    kw = dict(next(c[2] for c in M.crop_cases(None) if c[0] == name))
    boxes = d[f"cbi__{name}__boxes"]
    for b in (boxes, boxes.cuda()):
        out = crop_by_indices(d["x"].cuda(), b, **kw)
        ref = d[f"cbi__{name}__out"]
        err = (out.cpu() - ref).abs().max().item()
        assert out.shape == ref.shape and err <= 2e-6, err


def _composition(x, mask, src, size, interp, align, fx, fy, image_dtype):
    """The package's own per-sample composition: slice -> resize_bilinear (masks: CPU F.interpolate nearest through the image dtype) ->
    torch.flip / select_samples."""
    from kornia_amd.augmentation import select_samples
    from kornia_amd.geometry.transform import resize_bilinear

    oh, ow = size
    s = src.to(torch.long).cpu()
    outs, mouts = [], []
    for i in range(x.shape[0]):
        x1, x2, y1, y2 = int(s[i, 0, 0]), int(s[i, 1, 0]) + 1, int(s[i, 0, 1]), int(s[i, 3, 1]) + 1
        w = x[i:i + 1, :, y1:y2, x1:x2]
        if tuple(w.shape[-2:]) != (oh, ow):
            w = resize_bilinear(w, (oh, ow), align) if interp == "bilinear" else F.interpolate(w.cpu(), size=(oh, ow), mode="nearest").cuda()
        outs.append(w)
        if mask is not None:
            m = mask[i:i + 1, :, y1:y2, x1:x2].to(image_dtype)
            if tuple(m.shape[-2:]) != (oh, ow):
                m = F.interpolate(m.cpu().float(), size=(oh, ow), mode="nearest").to(image_dtype).cuda()
            mouts.append(m.to(mask.dtype))
    out = torch.cat(outs)
    mout = torch.cat(mouts) if mask is not None else None
    for f, dim in ((fx, -1), (fy, -2)):
        if f is not None:
            keep = (f > 0.5).cuda()
            out = select_samples(out.flip(dim), out, keep)
            if mout is not None:
                mout = torch.where(keep.view(-1, 1, 1, 1), mout.flip(dim), mout)
    return out, mout


def _boxes(B, H, W, g, kinds):
    out = []
    for k in kinds:
        if k == "up":
            w, h = int(torch.randint(2, 10, (1,), generator=g)), int(torch.randint(2, 8, (1,), generator=g))
        elif k == "down":
            w, h = int(torch.randint(20, W + 1, (1,), generator=g)), int(torch.randint(18, H + 1, (1,), generator=g))
        elif k == "eq":
            w, h = 16, 12
        elif k == "col":
            w, h = 1, int(torch.randint(1, H + 1, (1,), generator=g))
        else:
            w, h = int(torch.randint(1, W + 1, (1,), generator=g)), 1
        x0, y0 = int(torch.randint(0, W - w + 1, (1,), generator=g)), int(torch.randint(0, H - h + 1, (1,), generator=g))
        out.append([[x0, y0], [x0 + w - 1, y0], [x0 + w - 1, y0 + h - 1], [x0, y0 + h - 1]])
    return torch.tensor(out[:B], dtype=torch.float32)


@pytest.mark.parametrize("img_dtype", IMG_DTYPES)
def test_kernel_is_the_native_composition_bit_for_bit(img_dtype):
    from kornia_amd.geometry.transform.crop2d import crop_resize

    B, H, W = 6, 30, 41
    g = torch.Generator().manual_seed(11)
    x = torch.rand(B, 3, H, W, generator=g).to(img_dtype).cuda()
    labels = torch.randint(0, 300, (B, 1, H, W), generator=g)
    labels[:, :, :3] = 257
    mask = labels.cuda()
    fx = torch.tensor([0.0, 1.0, 1.0, 0.0, 1.0, 0.0])
    fy = torch.tensor([1.0, 0.0, 1.0, 0.0, 0.0, 1.0])
    cases = [
        (_boxes(B, H, W, g, ["up", "down", "eq", "up", "down", "eq"]), (12, 16)),
        (_boxes(1, H, W, g, ["down"]).expand(B, 4, 2).contiguous(), (12, 16)),  # identical boxes
        (_boxes(B, H, W, g, ["col", "row", "up", "down", "col", "row"]), (12, 16)),  # windows of width / height 1
        (_boxes(B, H, W, g, ["up", "down", "eq", "down", "up", "eq"]), (1, 9)),  # an output of height 1
        (_boxes(B, H, W, g, ["up", "down", "eq", "down", "up", "eq"]), (7, 1)),  # an output of width 1
    ]
    for src, size in cases:
        for align in (False, True):
            for flips in ((None, None), (fx, fy)):
                out, mout = crop_resize(x, mask, src.cuda(), size, "bilinear", align, "resize", flips[0], flips[1])
                ref, refm = _composition(x, mask, src, size, "bilinear", align, *flips, img_dtype)
                assert torch.equal(out, ref), (size, align, (out.float() - ref.float()).abs().max().item())
                assert torch.equal(mout, refm), (size, align)
        out, _ = crop_resize(x, None, src.cuda(), size, "nearest", False, "resize")
        ref, _ = _composition(x, None, src, size, "nearest", False, None, None, img_dtype)
        assert torch.equal(out, ref), size
    if img_dtype == torch.bfloat16:  # (the round trip: int64 257 -> 256 through bfloat16)
        src = torch.tensor([[[0.0, 0], [15, 0], [15, 11], [0, 11]]]).expand(B, 4, 2)
        _, mout = crop_resize(x, mask, src.cuda(), (12, 16))
        assert mout[:, :, :3].eq(256).all()


def test_window_of_the_output_size_is_a_copy_of_the_bits():
    from kornia_amd.geometry.transform import crop_by_indices

    x = torch.rand(2, 2, 10, 12)
    x[0, 0, 1, 2], x[1, 1, 3, 4], x[0, 1, 2, 3] = float("nan"), float("inf"), -0.0
    src = torch.tensor([[[1.0, 0], [8, 0], [8, 5], [1, 5]], [[4.0, 3], [11, 3], [11, 8], [4, 8]]])
    out = crop_by_indices(x.cuda(), src, (6, 8)).cpu()
    ref = torch.cat([x[0:1, :, 0:6, 1:9], x[1:2, :, 3:9, 4:12]])
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))


def test_boxes_outside_the_image_never_read_outside_it():
    from kornia_amd.geometry.transform import crop_by_indices

    x = torch.rand(3, 1, 8, 10)
    # an overhang right / bottom (cut as Python slicing cuts it), a box entirely outside (empty window: zeros)
    src = torch.tensor([[[6.0, 5], [14, 5], [14, 11], [6, 11]], [[0.0, 0], [9, 0], [9, 7], [0, 7]], [[20.0, 20], [25, 20], [25, 24], [20, 24]]])
    out = crop_by_indices(x.cuda(), src.cuda(), (4, 5)).cpu()
    from kornia_amd.geometry.transform import resize_bilinear

    assert torch.equal(out[0:1], resize_bilinear(x[0:1, :, 5:8, 6:10].cuda(), (4, 5)).cpu())
    assert torch.equal(out[2], torch.zeros(1, 4, 5))


def _count_calls(monkeypatch):
    """Wrap kornia_amd._native.lib() so that every call of km_crop_resize_fwd is counted."""
    from kornia_amd import _native as N

    real = N.lib
    calls = []

    class Wrap:
        def __init__(self, h):
            self._h = h

        def __getattr__(self, name):
            fn = getattr(self._h, name)
            if name != "km_crop_resize_fwd":
                return fn

            def counted(*a):
                calls.append(a)
                return fn(*a)
            return counted

    monkeypatch.setattr(N, "lib", lambda: Wrap(real()))
    return calls


@pytest.mark.parametrize("img_dtype", IMG_DTYPES)
def test_fused_crop_and_flips_are_the_children_one_by_one(img_dtype, monkeypatch):
    import kornia_amd.augmentation as A

    B, H, W = 7, 33, 45
    g = torch.Generator().manual_seed(3)
    x = torch.rand(B, 3, H, W, generator=g).to(img_dtype).cuda()
    mk = torch.randint(0, 50, (B, 1, H, W), generator=g, dtype=torch.uint8).cuda()
    mk2 = (torch.rand(B, 2, H, W, generator=g) > 0.5).to(torch.uint8).cuda()
    calls = _count_calls(monkeypatch)
    for seed in (1, 2):
        torch.manual_seed(seed)
        seq = A.AugmentationSequential(A.RandomResizedCrop((20, 24)), A.RandomHorizontalFlip(p=0.5), A.RandomVerticalFlip(p=0.6),
                                       data_keys=["input", "mask"])
        calls.clear()
        y, ym = seq(x, mk)
        assert len(calls) == 1  # crop + resize + both flips, image and mask: one launch
        # the same draws replayed child by child
        y1, m1 = x, mk
        for item, (_, m) in zip(seq._params, seq._kids):
            y1, m1 = A.AugmentationSequential(m, data_keys=["input", "mask"])(y1, m1, params=[item])
        assert torch.equal(y, y1) and torch.equal(ym, m1)
        assert torch.equal(seq(x, params=seq._params, data_keys=["input"]), y)  # image only, fused
        # the flips' parameters and matrices are those of their own calls
        for k in (1, 2):
            M = seq._kids[k][1].transform_matrix
            assert M.shape == (B, 3, 3) and M.device == y.device
        # a second mask: a mask-only launch on the same draws
        seq2 = A.AugmentationSequential(*[m for _, m in seq._kids], data_keys=["input", "mask", "mask"])
        calls.clear()
        y2, _, mo2 = seq2(x, mk2, mk2, params=seq._params)
        assert len(calls) == 2 and torch.equal(y2, y)


def test_flip_matrices_and_inverse():
    import kornia_amd.augmentation as A

    x = torch.rand(4, 3, 9, 13).cuda()
    torch.manual_seed(5)
    h = A.RandomHorizontalFlip(p=0.5)
    y = h(x)
    keep = h._params["batch_prob"] > 0.5
    M = h.transform_matrix.cpu()
    for i in range(4):
        ref = torch.tensor([[-1.0, 0, 12], [0, 1, 0], [0, 0, 1]]) if keep[i] else torch.eye(3)
        assert torch.equal(M[i], ref)
        assert torch.equal(y[i], x[i].flip(-1) if keep[i] else x[i])
    assert torch.equal(h.inverse(y), x)
    v = A.RandomVerticalFlip(p=1.0)
    assert torch.equal(v(x), x.flip(-2))
    assert torch.equal(v.transform_matrix[0].cpu(), torch.tensor([[1.0, 0, 0], [0, -1, 8], [0, 0, 1]]))


def test_device_boxes_do_not_synchronise(monkeypatch):
    """crop_by_indices with device boxes and an explicit size reads nothing back: one native call, no .tolist() / .item() / .cpu() of the
    boxes (torch.cuda.set_sync_debug_mode reports the synchronising copies where the runtime supports it)."""
    from kornia_amd.geometry.transform import crop_by_indices

    x = torch.rand(4, 3, 20, 30).cuda()
    src = torch.tensor([[[1.0, 2], [10, 2], [10, 9], [1, 9]]]).repeat(4, 1, 1).cuda()
    calls = _count_calls(monkeypatch)
    tolist = torch.Tensor.tolist
    reads = []
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: reads.append(1) or tolist(self))
    on_gpu = x.device.type == "cuda"  # (the emulated device keeps tensors in host memory: no stream to synchronise with there)
    prev = torch.cuda.get_sync_debug_mode() if on_gpu else None
    try:
        if on_gpu:
            torch.cuda.set_sync_debug_mode("error")
        out = crop_by_indices(x, src, (8, 8))
    finally:
        if on_gpu:
            torch.cuda.set_sync_debug_mode(prev)
    assert out.shape == (4, 3, 8, 8) and len(calls) == 1 and not reads


def test_autograd_falls_back_to_the_differentiable_composition():
    import kornia_amd.augmentation as A
    from kornia_amd.geometry.transform import crop_by_indices

    x = torch.rand(3, 2, 16, 20).cuda().requires_grad_(True)
    src = torch.tensor([[[1.0, 2], [10, 2], [10, 9], [1, 9]], [[0.0, 0], [19, 0], [19, 15], [0, 15]], [[4.0, 4], [11, 4], [11, 11], [4, 11]]])
    out = crop_by_indices(x, src, (8, 8))
    out.sum().backward()
    assert x.grad is not None and x.grad.abs().sum() > 0
    with torch.no_grad():
        assert torch.equal(out, crop_by_indices(x, src, (8, 8)))
    torch.manual_seed(4)
    seq = A.AugmentationSequential(A.RandomResizedCrop((8, 8)), A.RandomHorizontalFlip())
    y = seq(x)
    y.sum().backward()
    with torch.no_grad():
        assert torch.equal(y, seq(x, params=seq._params))


def test_errors():
    import kornia_amd.augmentation as A
    from kornia_amd.geometry.transform import crop_by_indices

    with pytest.raises(AssertionError):
        A.RandomResizedCrop((0, 5))
    with pytest.raises(AssertionError):
        A.RandomResizedCrop((5.0, 5))
    with pytest.raises(ValueError):
        A.RandomResizedCrop((5, 5), scale=(1.0, 0.5))
    with pytest.raises(ValueError):
        A.RandomResizedCrop((5, 5), ratio=(2.0, 1.0))
    with pytest.raises(TypeError):
        A.RandomResizedCrop((5, 5), scale=(0.1, 0.5, 1.0))
    with pytest.raises(NotImplementedError):
        A.RandomResizedCrop((5, 5), p=0.5)
    x = torch.rand(2, 3, 12, 14).cuda()
    src = torch.tensor([[[0.0, 0], [5, 0], [5, 3], [0, 3]], [[1.0, 1], [3, 1], [3, 8], [1, 8]]])
    with pytest.raises(ValueError):
        crop_by_indices(x, src)  # size=None with boxes of different sizes
    with pytest.raises(NotImplementedError):
        crop_by_indices(x, src, (4, 4), antialias=True)
    rrc = A.RandomResizedCrop((6, 6))
    y = rrc(x)
    with pytest.raises(NotImplementedError):
        rrc.inverse(y)
    with pytest.raises(NotImplementedError):
        A.AugmentationSequential(A.RandomResizedCrop((6, 6)), data_keys=["input", "mask"]).inverse(y, torch.zeros(2, 1, 6, 6).cuda(),
                                                                                                 params=[A.ParamItem("RandomResizedCrop_0", rrc._params)])
    # the RandomResizedCrop module itself is unchanged by a p it refuses, and a foreign child is still refused
    with pytest.raises(NotImplementedError):
        A.AugmentationSequential(torch.nn.Identity())
