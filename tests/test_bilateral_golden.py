"""CPU: the restatement of kornia.filters.bilateral_blur / joint_bilateral_blur that the device tests use for the shapes the fixture lacks -
border rule as an index map, the window gathered by indices, the weights ``s_i exp(coef D)`` and the two sums - equals the reference's recorded
float32 outputs bit for bit and its float64 outputs and gradients to rounding (tests/golden/bilateral_blur.npz, written by
tests/make_golden_bilateral.py)."""
import pytest
import torch

from _util import golden

BORDERS = ["constant", "reflect", "replicate", "circular"]
DISTS = ["l1", "l2"]
GRAD_WINDOWS = [(5, 5), (3, 7)]
SIGMA_SPACE = (1.5, 1.1)
F32_BOUND = 1e-5    # the project's stated fp32 bound on [0, 1] images (BASELINE.json, north_star)
F64_BOUND = 1e-12
GRAD_BOUND = 1e-5   # of the largest absolute entry of the fixture's float64 gradient

_cache = {}


def fixture() -> dict:
    """The fixture as torch tensors (string arrays as they are), loaded once and left unchanged."""
    if not _cache:
        for k, v in golden("bilateral_blur").items():
            _cache[k] = v if v.dtype.kind in "US" else torch.from_numpy(v)
    return _cache


def sname(shape) -> str:
    return "x".join(str(v) for v in shape)


def kname(k) -> str:
    return f"{k[0]}x{k[1]}"


def parse_case(key: str):
    """'joint__2x3x13x17__5x5__l1__reflect__sc0.5' -> (func, shape, window, dist, border, sigma_color)"""
    func, shape, k, dist, border, sc = key.split("__")
    return func, tuple(int(v) for v in shape.split("x")), tuple(int(v) for v in k.split("x")), dist, border, float(sc[2:])


def cases():
    return [str(k) for k in fixture()["cases"]]


def pair(kernel_size):
    return (kernel_size, kernel_size) if isinstance(kernel_size, int) else (int(kernel_size[0]), int(kernel_size[1]))


def pad_fits(border, kernel_size, H, W) -> bool:
    ky, kx = pair(kernel_size)
    if border == "reflect":
        return ky // 2 < H and kx // 2 < W
    if border == "circular":
        return ky // 2 <= H and kx // 2 <= W
    return True


def _axis_map(n: int, pad: int, border: str):
    """for the padded coordinates -pad .. n - 1 + pad: the image coordinate each reads, and whether it reads one at all"""
    i = torch.arange(-pad, n + pad)
    if border == "reflect":
        j = torch.where(i < 0, -i, torch.where(i >= n, 2 * (n - 1) - i, i))
    elif border == "replicate":
        j = i.clamp(0, n - 1)
    elif border == "circular":
        j = i % n
    else:
        j = i
    ok = (j >= 0) & (j < n)
    return j.clamp(0, n - 1), ok


def _windows(t: torch.Tensor, ky: int, kx: int, border: str) -> torch.Tensor:
    """(B, C, H, W, ky kx): the window of every pixel, row-major, through the border rule (zeros outside a constant border)"""
    B, C, H, W = t.shape
    jy, oky = _axis_map(H, ky // 2, border)
    jx, okx = _axis_map(W, kx // 2, border)
    padded = torch.where((oky[:, None] & okx[None, :]), t[:, :, jy][:, :, :, jx], torch.zeros((), dtype=t.dtype))
    rows = torch.arange(H)[:, None] + torch.arange(ky)[None, :]  # (H, ky)
    cols = torch.arange(W)[:, None] + torch.arange(kx)[None, :]  # (W, kx)
    win = padded[:, :, rows[:, None, :, None], cols[None, :, None, :]]  # (B, C, H, W, ky, kx)
    return win.reshape(B, C, H, W, ky * kx)


def _gauss1d(k: int, sigma: torch.Tensor) -> torch.Tensor:
    """(B, k) normalised samples of a Gaussian centred on k // 2; sigma (B, 1)"""
    r = (torch.arange(k, dtype=sigma.dtype) - float(k // 2)).expand(sigma.shape[0], -1)
    w = torch.exp(-r.pow(2.0) / (2 * sigma.pow(2.0)))
    return w / w.sum(-1, keepdim=True)


def space_kernel(ky: int, kx: int, sigma_space, dtype) -> torch.Tensor:
    s = torch.tensor([sigma_space], dtype=dtype) if isinstance(sigma_space, tuple) else sigma_space.to(dtype)
    return (_gauss1d(ky, s[:, 0, None])[..., None] * _gauss1d(kx, s[:, 1, None]).view(-1, 1, kx)).reshape(-1, ky * kx)


def restate(x: torch.Tensor, guide, kernel_size, sigma_color, sigma_space, border: str = "reflect", dist: str = "l1") -> torch.Tensor:
    """The reference's result in x's dtype on the CPU (differentiable wrt x and guide)."""
    ky, kx = pair(kernel_size)
    xw = _windows(x, ky, kx, border)
    g = x if guide is None else guide
    gw = xw if guide is None else _windows(guide, ky, kx, border)
    delta = gw - g.unsqueeze(-1)
    if dist == "l1":
        D = delta.abs().sum(1, keepdim=True).square()
    else:
        D = delta.square().sum(1, keepdim=True)
    if isinstance(sigma_color, torch.Tensor):
        sigma_color = sigma_color.to(x.dtype).view(-1, 1, 1, 1, 1)
    colour = (-0.5 / sigma_color**2 * D).exp()
    k = space_kernel(ky, kx, sigma_space, x.dtype).view(-1, 1, 1, 1, ky * kx) * colour
    return (xw * k).sum(-1) / k.sum(-1)


def restate_grads(x, guide, kernel_size, sigma_color, sigma_space, border, dist, gout):
    """float64 gradients of the restatement wrt x (and guide) for grad_out ``gout``"""
    xr = x.detach().double().clone().requires_grad_()
    gr = None if guide is None else guide.detach().double().clone().requires_grad_()
    restate(xr, gr, kernel_size, sigma_color, sigma_space, border, dist).backward(gout.double())
    return xr.grad, (None if gr is None else gr.grad)


def case_inputs(key: str, dtype=torch.float32):
    d = fixture()
    func, shape, k, dist, border, sc = parse_case(key)
    x = d[f"x__{sname(shape)}"].to(dtype)
    g = d[f"g__{sname(shape)}"].to(dtype) if func == "joint" else None
    return x, g, k, sc, border, dist


def test_the_design_covers_every_factor():
    seen = [set() for _ in range(6)]
    for key in cases():
        for s, v in zip(seen, parse_case(key)):
            s.add(v)
    assert seen[0] == {"self", "joint"} and seen[1] == {(2, 3, 13, 17), (1, 1, 9, 12), (2, 4, 16, 24)}
    assert seen[2] == {(3, 3), (5, 5), (9, 9), (3, 7), (15, 15)} and seen[3] == set(DISTS) and seen[4] == set(BORDERS) and seen[5] == {0.1, 0.5}
    # the reference's own float32 stays this close to its float64 - what the 1e-5 bound is a margin over
    d = fixture()
    assert d["self_err"].max().item() < 5e-7 and d["grad_self_err"].max().item() < 1e-6


@pytest.mark.parametrize("key", golden("bilateral_blur")["cases"].tolist())
def test_restatement_equals_the_reference(key):
    d = fixture()
    x, g, k, sc, border, dist = case_inputs(key)
    out = restate(x, g, k, sc, SIGMA_SPACE, border, dist)
    assert torch.equal(out, d[f"y__{key}__f32"]), (out - d[f"y__{key}__f32"]).abs().max().item()
    x, g, k, sc, border, dist = case_inputs(key, torch.float64)
    out = restate(x, g, k, sc, SIGMA_SPACE, border, dist)
    assert (out - d[f"y__{key}__f64"]).abs().max().item() <= F64_BOUND


@pytest.mark.parametrize("func", ["self", "joint"])
def test_restatement_tensor_sigmas(func):
    d = fixture()
    x, g = d["x__2x3x13x17"], (d["g__2x3x13x17"] if func == "joint" else None)
    out = restate(x, g, (5, 5), d["ts__sigma_color"], d["ts__sigma_space"], "reflect", "l1")
    assert torch.equal(out, d[f"ts__{func}__f32"])


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("kernel", GRAD_WINDOWS, ids=kname)
def test_gradient_restatement_equals_the_reference(kernel, dist, border):
    d = fixture()
    x, g, gout = d["x__2x3x13x17"], d["g__2x3x13x17"], d["grad__gout"]
    tag = f"{kname(kernel)}__{dist}__{border}"
    gx, _ = restate_grads(x, None, kernel, 0.5, SIGMA_SPACE, border, dist, gout)
    ref = d[f"grad__self__{tag}__gx"]
    assert (gx - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    gx, gg = restate_grads(x, g, kernel, 0.5, SIGMA_SPACE, border, dist, gout)
    for got, ref in ((gx, d[f"grad__joint__{tag}__gx"]), (gg, d[f"grad__joint__{tag}__gg"])):
        assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


@pytest.mark.parametrize("which", ["nan", "inf"])
def test_restatement_non_finite(which):
    d = fixture()
    x, ref = d[f"nf_{which}__x"], d[f"nf_{which}__y"]
    want = torch.zeros(7, 7, dtype=torch.bool)
    want[2:5, 2:5] = True  # the nine pixels whose windows hold the centre
    assert torch.equal(torch.isnan(ref[0, 0]), want) and not bool(torch.isinf(ref).any())
    out = restate(x, None, (3, 3), 0.5, SIGMA_SPACE)
    assert torch.equal(torch.isnan(out), torch.isnan(ref)) and torch.equal(out.nan_to_num(7.0), ref.nan_to_num(7.0))


def test_what_the_reference_raises():
    d = fixture()
    assert list(d["raises__what"]) == ["kernel_size=4", "kernel_size=(3, 4)", "color_distance_type=l3"]
    assert list(d["raises__type"]) == ["RuntimeError", "RuntimeError", "ValueError"]


def test_exp2_form_stays_close_to_the_reference():
    """What the fp32 kernels evaluate - exp2((coef log2 e) D) with the product rounded once - against the reference's exp(coef D), over the
    fixture's own images: the weights differ by 1.2e-7 at most."""
    d = fixture()
    worst = 0.0
    for sc in (0.1, 0.5):
        x = d["x__2x3x13x17"]
        delta = _windows(x, 5, 5, "reflect") - x.unsqueeze(-1)
        for D in (delta.abs().sum(1).square(), delta.square().sum(1)):
            coef = torch.tensor(-0.5 / sc**2, dtype=torch.float32)
            worst = max(worst, (torch.exp2((coef * 1.4426950408889634) * D) - (coef * D).exp()).abs().max().item())
    assert worst <= 1.2e-7, worst


def test_package_has_the_reference_signatures():
    """names, parameter names, order, defaults and __repr__ of kornia/filters/bilateral.py:87-202"""
    import inspect

    import kornia_amd
    import kornia_amd.filters as KF

    tail = [("kernel_size", inspect.Parameter.empty), ("sigma_color", inspect.Parameter.empty), ("sigma_space", inspect.Parameter.empty),
            ("border_type", "reflect"), ("color_distance_type", "l1")]
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]  # noqa: E731
    assert sig(KF.bilateral_blur) == [("input", inspect.Parameter.empty)] + tail
    assert sig(KF.joint_bilateral_blur) == [("input", inspect.Parameter.empty), ("guidance", inspect.Parameter.empty)] + tail
    assert sig(KF.BilateralBlur.__init__)[1:] == tail and sig(KF.JointBilateralBlur.__init__)[1:] == tail
    assert repr(KF.BilateralBlur((3, 3), 0.1, (1.5, 1.5))) == ("BilateralBlur(kernel_size=(3, 3), sigma_color=0.1, sigma_space=(1.5, 1.5), "
                                                              "border_type=reflect, color_distance_type=l1)")
    assert repr(KF.JointBilateralBlur(5, 0.5, (1.0, 2.0), "replicate", "l2")) == ("JointBilateralBlur(kernel_size=5, sigma_color=0.5, sigma_space=(1.0, 2.0), "
                                                                                  "border_type=replicate, color_distance_type=l2)")
    for name in ("bilateral_blur", "joint_bilateral_blur", "BilateralBlur", "JointBilateralBlur"):
        assert getattr(kornia_amd, name) is getattr(KF, name)
