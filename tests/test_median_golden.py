"""CPU: the restatement of kornia.filters.median_blur that the device tests use - zero-pad, unfold the window, sort, take element (n - 1) // 2,
NaN where the window holds a NaN or inf (n >= 2) - and of its gradient under the package's tie rule (the smallest row-major window position whose
value equals the median) equal the reference's recorded outputs and gradients bit for bit (tests/golden/median_blur.npz, written by
tests/make_golden_median.py).  That anchors the restatement for the shapes the fixture does not hold."""
import pytest
import torch
import torch.nn.functional as F

from _util import golden

DTYPES = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}
KERNELS = [(3, 3), (5, 5), (7, 7), (3, 5), (5, 1), (1, 1), (9, 3), (15, 15)]
SHAPES = [(2, 3, 13, 17), (1, 1, 2, 3), (1, 2, 1, 9), (2, 2, 16, 24)]
GRAD_KERNELS = [(3, 3), (5, 5), (3, 7)]

_cache = {}


def fixture() -> dict:
    """The fixture as torch tensors, loaded once and left unchanged."""
    if not _cache:
        for k, v in golden("median_blur").items():
            _cache[k] = v if v.dtype.kind in "US" else torch.from_numpy(v)
    return _cache


def sname(shape) -> str:
    return "x".join(str(v) for v in shape)


def kname(k) -> str:
    return f"{k[0]}x{k[1]}"


def pair(kernel_size):
    return (kernel_size, kernel_size) if isinstance(kernel_size, int) else (int(kernel_size[0]), int(kernel_size[1]))


def restate(x: torch.Tensor, kernel_size):
    """(median, position): the reference's values in x's dtype and the tie rule's window position p * kx + q (int64)."""
    ky, kx = pair(kernel_size)
    B, C, H, W = x.shape
    n = ky * kx
    xd = x.detach().cpu().double()  # (exact for every dtype: selection only)
    win = F.pad(xd, (kx // 2, kx // 2, ky // 2, ky // 2)).unfold(2, ky, 1).unfold(3, kx, 1).reshape(B, C, H, W, n)
    med = win.sort(dim=-1).values[..., (n - 1) // 2]
    if n >= 2:
        med = torch.where((~torch.isfinite(win)).any(dim=-1), torch.full_like(med, float("nan")), med)
    pos = (win == med[..., None]).to(torch.uint8).argmax(dim=-1)  # (the first of equal maxima)
    return med.to(x.dtype), pos


def restate_grad(x: torch.Tensor, kernel_size, gout: torch.Tensor):
    """(x.grad, routed): grad_out of every output added at the input pixel its median came from (float64 sums, rounded once to x's dtype);
    ``routed``: the outputs whose position lies inside the image (the others drop their gradient)."""
    ky, kx = pair(kernel_size)
    B, C, H, W = x.shape
    _, pos = restate(x, kernel_size)
    i = torch.arange(H).view(1, 1, H, 1) + pos // kx - ky // 2
    j = torch.arange(W).view(1, 1, 1, W) + pos % kx - kx // 2
    routed = (i >= 0) & (i < H) & (j >= 0) & (j < W)
    plane = (torch.arange(B * C).view(B, C, 1, 1) * (H * W)).expand(B, C, H, W)
    flat = (plane + i.clamp(0, H - 1) * W + j.clamp(0, W - 1))[routed]
    g = torch.zeros(B * C * H * W, dtype=torch.float64)
    g.index_put_((flat,), gout.detach().cpu().double()[routed], accumulate=True)
    return g.view(B, C, H, W).to(x.dtype), routed


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("kernel", KERNELS, ids=kname)
def test_restatement_equals_the_reference(kernel, dname):
    d = fixture()
    for shape in SHAPES:
        x = d[f"x__{sname(shape)}"].to(DTYPES[dname])
        ref = d[f"y__{sname(shape)}__{kname(kernel)}__{dname}"].to(DTYPES[dname])
        out, pos = restate(x, kernel)
        assert out.dtype == ref.dtype and torch.equal(out, ref), (shape, kernel, dname)
        assert int(pos.max()) < kernel[0] * kernel[1]


@pytest.mark.parametrize("which", ["nan", "inf"])
def test_restatement_non_finite(which):
    d = fixture()
    x, ref = d[f"nf_{which}__x"], d[f"nf_{which}__y"]
    out, _ = restate(x, (3, 3))
    want = torch.zeros(3, 3, dtype=torch.bool)
    want[:2, :2] = True  # the four pixels whose windows hold the corner
    assert torch.equal(torch.isnan(ref[0, 0]), want)
    assert torch.equal(torch.isnan(out), torch.isnan(ref)) and torch.equal(out.nan_to_num(7.0), ref.nan_to_num(7.0))


@pytest.mark.parametrize("kernel", GRAD_KERNELS, ids=kname)
def test_gradient_restatement_equals_the_reference(kernel):
    d = fixture()
    x, gout = d["grad__x"], d["grad__gout"]
    for ch in x.flatten(0, 1):
        assert torch.equal(ch.flatten().sort().values, torch.arange(1.0, ch.numel() + 1))  # tie-free
    g, routed = restate_grad(x, kernel, gout)
    assert torch.equal(g, d[f"grad__{kname(kernel)}"])
    assert not bool(routed.all()) and g.sum().item() == gout[routed].sum().item()


def test_even_sizes_raise_runtime_error_in_the_reference():
    d = fixture()
    assert d["even__kernels"].tolist() == [[4, 4], [3, 4], [2, 3]] and list(d["even__raises"]) == ["RuntimeError"] * 3


def test_package_has_the_reference_signatures():
    """median_blur, MedianBlur and RandomMedianBlur exist with the reference's names, parameter names and defaults
    (kornia/filters/median.py:35, :97; kornia/augmentation/_2d/intensity/median_blur.py:59-61)."""
    import inspect

    import kornia_amd
    import kornia_amd.augmentation as A
    import kornia_amd.filters as KF

    assert kornia_amd.median_blur is KF.median_blur and kornia_amd.MedianBlur is KF.MedianBlur
    assert list(inspect.signature(KF.median_blur).parameters) == ["input", "kernel_size"]
    assert list(inspect.signature(KF.MedianBlur.__init__).parameters) == ["self", "kernel_size"]
    sig = inspect.signature(A.RandomMedianBlur.__init__).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("kernel_size", (3, 3)), ("same_on_batch", False), ("p", 0.5), ("keepdim", False)]
    assert "RandomMedianBlur" in A.__all__
