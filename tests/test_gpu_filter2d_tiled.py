"""GPU: the LDS-tiled dense filter2d kernels (csrc/km_filter2d_tiled.hip: everything up to 31 x 31 that the register-tiled 3 / 5 / 7 kernels
leave out) against the generic kernels they replace - `km_config_set("sep_lds", 1)` selects those - and against float64 tensor operations.
Bounds: forward and input gradient equal the generic kernels' bit for bit (same fma order); the tap gradient sums in another order and is held
to the gk bound of tests/test_gpu_filters.py::test_filter2d_backward (atol 1e-2, rtol 1e-4; a 16-bit kernel.grad is the fp64 sum rounded once
to that type by the Python layer, so two sums inside the bound may land on neighbouring values: one ulp of the type is added).  Integer data
in -3 .. 3 (16-bit cases: kernels of at most 28 taps, outputs below 9 * 28 < 2^8, exact in bf16) must equal float64: every partial sum is an
integer below 2^24.  Random data against float64 of the same inputs: that file's bounds (fp32 1e-5, fp64 1e-12 relative); a 16-bit storage
type rounds the fp32 result once: one ulp of it)."""
import pytest
import torch

from _util import launch_policy
from test_gpu_written_outputs import FILLS, _run_case, case, same_bits, unchanged

pytestmark = pytest.mark.gpu

TW, TH = 64, 64  # the forward / adjoint tile of csrc/km_filter2d_tiled.hip (fp64: 64 x 32; the tap gradient: 64 x 32, fp64 64 x 16)
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
ULP = {BF16: 2.0 ** -7, F16: 2.0 ** -10}  # relative size of one unit in the last place, at most
IMAGES = [(2, 2, TH + 1, TW + 5), (1, 1, 2 * TH + 3, 2 * TW + 1)]
# (shape, kernel, border or 'valid', Bk, dtype): every kernel shape with every border and 'valid' in fp32, images and Bk alternating; H = 16
# under 31 x 31 (reflect pad 15 = H - 1, H <= 2 pd: the generic adjoint behind the tiled forward); the other dtypes on fewer
TABLE = [(IMAGES[0] if (i + j) % 2 else IMAGES[(i + j) // 2 % 2], ks, b, 1 + (i + j) % 2, F32)
         for i, ks in enumerate([(9, 9), (4, 6), (1, 31), (31, 1), (15, 15)]) for j, b in enumerate(["constant", "reflect", "replicate", "circular", "valid"])]
TABLE += [((2, 2, 16, TW + 5), (31, 31), b, Bk, F32) for b, Bk in (("reflect", 1), ("replicate", 2), ("constant", 1))]
TABLE += [(IMAGES[0], (9, 9), "reflect", 2, F64), (IMAGES[1], (4, 6), "circular", 1, F64), (IMAGES[0], (15, 15), "valid", 1, F64), (IMAGES[0], (31, 1), "replicate", 1, F64),
          (IMAGES[0], (4, 6), "reflect", 2, BF16), (IMAGES[1], (6, 4), "constant", 1, BF16), (IMAGES[0], (1, 28), "replicate", 1, BF16), (IMAGES[0], (5, 5), "valid", 2, BF16),
          (IMAGES[0], (4, 6), "circular", 1, F16)]


def _id(c):
    s, ks, b, Bk, dt = c
    return f"{'x'.join(map(str, s))}-{ks[0]}x{ks[1]}-{b}-Bk{Bk}-{str(dt)[6:]}"


def _inputs(c, integer):
    s, ks, b, Bk, dt = c
    g = torch.Generator().manual_seed(7)
    out = s[:2] + ((s[2] - ks[0] + 1, s[3] - ks[1] + 1) if b == "valid" else s[2:])
    draw = (lambda *sh: torch.randint(-3, 4, sh, generator=g).double()) if integer else (lambda *sh: torch.rand(*sh, generator=g, dtype=F64) - 0.25)
    return draw(*s).to(dt), draw(Bk, *ks).to(dt), draw(*out).to(dt)


def _native(c, x, k, go, **policy):
    import kornia_amd as K

    xg, kg = x.cuda().requires_grad_(), k.cuda().requires_grad_()
    with launch_policy(**policy):
        y = K.filter2d(xg, kg, "constant" if c[2] == "valid" else c[2], False, "valid" if c[2] == "valid" else "same")
        y.backward(go.cuda())
    return y.detach().cpu(), xg.grad.cpu(), kg.grad.cpu()


def _ref64(c, x, k, go):
    import torch.nn.functional as Fn  # (the `_conv64` of tests/test_gpu_filters.py, with 'valid')

    (B, C, H, W), (kH, kW), b, Bk, dt = c
    x64, k64 = x.double().clone().requires_grad_(), k.double().clone().requires_grad_()
    pl, pt = (kW - 1) // 2, (kH - 1) // 2
    xp = x64 if b == "valid" else Fn.pad(x64, (pl, kW - 1 - pl, pt, kH - 1 - pt), mode=b)
    w = k64[torch.arange(B) % Bk][:, None].expand(B, C, kH, kW).reshape(B * C, 1, kH, kW)
    y = Fn.conv2d(xp.reshape(1, B * C, *xp.shape[-2:]), w, groups=B * C).view(go.shape)
    y.backward(go.double())
    return y.detach(), x64.grad, k64.grad


@pytest.mark.parametrize("c", TABLE, ids=_id)
def test_same_bits_as_the_generic_kernels(c):
    x, k, go = _inputs(c, integer=False)
    (y, gx, gk), (y0, gx0, gk0) = _native(c, x, k, go), _native(c, x, k, go, sep_lds=1)
    assert torch.equal(y, y0), f"forward: {(y.double() - y0.double()).abs().max().item():.3e}"
    assert torch.equal(gx, gx0), f"input gradient: {(gx.double() - gx0.double()).abs().max().item():.3e}"
    assert torch.allclose(gk.double(), gk0.double(), atol=1e-2, rtol=1e-4 + ULP.get(c[4], 0.0)), f"tap gradient: {(gk.double() - gk0.double()).abs().max().item():.3e}"


def _exact(c):
    (x, k, go), dt = _inputs(c, integer=True), c[4]
    ref = _ref64(c, x, k, go)
    assert max(ref[0].abs().max(), ref[1].abs().max()).item() < (2 ** 24 if dt in (F32, F64) else 2 ** 8) and 0 < ref[2].abs().max().item() < 2 ** 24
    xd, kd, god = x.cuda(), k.cuda(), go.cuda()
    with unchanged(xd, kd, god):
        got = _native(c, xd, kd, god)
    for name, a, r in zip(("y", "gx", "gk"), got, ref):
        assert a.dtype == dt and torch.equal(a, r.to(dt)), f"{name}: {(a.double() - r).abs().max().item()}"
    return dict(zip(("y", "gx", "gk"), got))  # (integer data: the fp64 atomics behind gk are exact in any order)


@pytest.mark.parametrize("c", TABLE, ids=_id)
def test_integer_data_equals_float64(c):
    _exact(c)


@pytest.mark.parametrize("dt", [F32, F64, BF16, F16], ids=lambda d: str(d)[6:])
def test_random_data_against_float64(dt):
    c = (IMAGES[0], (9, 9), "reflect", 2, dt)
    x, k, go = _inputs(c, integer=False)
    tol = {F32: 1e-5, F64: 1e-12}.get(dt) or ULP[dt]  # (16-bit: the fp32 result rounded once to the type)
    for name, a, r in zip(("y", "gx", "gk"), _native(c, x, k, go), _ref64(c, x, k, go)):
        lim = dict(atol=tol, rtol=tol) if name != "gk" else dict(atol=1e-2 if dt != F64 else 0, rtol=1e-4 + tol if dt != F32 else 1e-4)
        assert torch.allclose(a.double(), r, **lim), f"{name}: {(a.double() - r).abs().max().item():.3e}"


# ---- every element written, nothing else: four cases in the guard table of tests/test_gpu_written_outputs.py, as tests/test_gpu_bilateral.py does
_GUARDED = [TABLE[1], TABLE[14], TABLE[25], TABLE[-5]]
for _c in _GUARDED:
    case(f"filter2d-tiled-{_id(_c)}")(lambda oracle, c=_c: _exact(c))


@pytest.mark.parametrize("name", [f"filter2d-tiled-{_id(c)}" for c in _GUARDED])
def test_guarded_cases(oracle, name):
    a, b = (_run_case(name, oracle, fill) for fill in FILLS)
    bad = [k for k in a if not same_bits(a[k], b[k])]  # (an element never written, or read before it was)
    assert a.keys() == b.keys() and len(a) == 3 and not bad, f"{bad}: the results under the fills 0xFF and 0x7B differ"


def test_tap_gradient_reads_the_image_once():
    """the km_filter2d_bwd_kernel launch alone, 3 warm-ups and the median of 10 per mode: the generic kernel (sep_lds = 1) streams the planes 225 times"""
    import kornia_amd as K
    from kornia_amd import _native as N

    R = 2.0  # a third of the ratio measured on the MI355X (5.5: 0.153 ms against 0.028 ms) is 1.8; the floor of 2 holds
    x, go, k = torch.rand(2, 3, 256, 256).cuda(), torch.rand(2, 3, 256, 256).cuda(), torch.rand(1, 15, 15).cuda().requires_grad_()
    K.filter2d(x, k, "reflect").backward(go)  # through the public interface once: the launch below is the one its backward makes
    gk = torch.zeros(1, 15, 15, dtype=F64, device="cuda")

    def median_ms(ts=()):
        for _ in range(13):
            gk.zero_()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            N.launch("km_filter2d_bwd_kernel", x.device, go.data_ptr(), x.data_ptr(), gk.data_ptr(), 2, 3, 256, 256, 1, 15, 15, 1, 1, 0)
            ev[1].record()
            ev[1].synchronize()
            ts += (ev[0].elapsed_time(ev[1]),)
        return sorted(ts[3:])[5], gk.clone()

    t_tiled, gk_tiled = median_ms()
    with launch_policy(sep_lds=1):
        t_generic, gk_generic = median_ms()
    print(f"tap gradient 2x3x256x256, 15x15: generic {t_generic:.4f} ms, tiled {t_tiled:.4f} ms, ratio {t_generic / t_tiled:.1f} (bound {R})")
    assert torch.allclose(gk_tiled, gk_generic, atol=1e-2, rtol=1e-4) and torch.allclose(k.grad.double(), gk_tiled, atol=1e-2, rtol=1e-4)
    assert t_generic >= R * t_tiled
