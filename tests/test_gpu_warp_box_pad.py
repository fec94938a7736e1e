"""The LDS box forward for border / reflection / fill padding (csrc/km_warp_box_pad.hip) against the generic per-pixel kernel
(launch policy warp_fwd_algo = 1), bit for bit, and against the CPU oracle - at the smallest shapes that reach every branch of the
kernel: partial tiles on both axes, an output width that is no multiple of 4, one / two / many fold points inside a tile."""
import math

import pytest
import torch

from _util import flagship_homographies, launch_policy
from test_gpu_written_outputs import same_bits

pytestmark = pytest.mark.gpu

PADS = ["border", "reflection", "fill"]


def _about_centre(scale, deg, H, W, h, w, shift=(0.0, 0.0)):
    """(2,2,3) src -> dst: rotation by `deg` and scaling by `scale` that takes the source centre to the output centre (+ shift)"""
    a, b = scale * math.cos(math.radians(deg)), scale * math.sin(math.radians(deg))
    cx, cy, ox, oy = (W - 1) / 2, (H - 1) / 2, (w - 1) / 2 + shift[0], (h - 1) / 2 + shift[1]
    return torch.tensor([[a, b, ox - a * cx - b * cy], [-b, a, oy + b * cx - a * cy]]).expand(2, 2, 3).contiguous()


# name: (source H, W, output h, w, matrices) - the branch each one reaches is in its comment
def _maps():
    g = torch.Generator().manual_seed(7)
    shift = torch.tensor([[1.0, 0.0, -7.5], [0.0, 1.0, 5.25]]).expand(2, 2, 3).contiguous()
    nan = shift.clone()
    nan[1] = float("nan")
    return {
        "shift": (45, 72, 37, 69, shift),  # one fold / clip point inside a tile, on two edges
        "rot30": (45, 72, 37, 69, _about_centre(0.9, 30.0, 45, 72, 37, 69)),  # the square halves, all four edges outside somewhere
        "homography": (45, 72, 37, 69, flagship_homographies(2, 45, 72, 37, 69, g, jitter=3.0)),  # perspective mode
        "zoom_out": (8, 8, 32, 64, _about_centre(1 / 6, 0.0, 8, 8, 32, 64)),  # several reflection periods in a tile: the whole image staged
        "minify3": (136, 200, 37, 69, _about_centre(1 / 3, 0.0, 136, 200, 37, 69)),  # box too large: the per-pixel rows inside the kernel
        "shift_nan": (45, 72, 37, 69, nan),  # sample 1: every position NaN (clipped into the image under border / reflection)
        "masked": (45, 72, 45, 72, _about_centre(1.0, 10.0, 45, 72, 45, 72, (3.0, -2.0))),  # km_warp2d_fwd_masked, apply = [1, 0]
    }


MAPS = _maps()


def _run(name, x, pad, align, fill):
    import kornia_amd as K
    from kornia_amd.geometry.transform.imgwarp import COORD_AFFINE, _warp

    _, _, h, w, M = MAPS[name]
    if name == "masked":
        with torch.no_grad():
            return _warp(x, M.cuda(), (h, w), COORD_AFFINE, 1, "bilinear", pad, align, fill, torch.tensor([1, 0], dtype=torch.uint8).cuda())
    fn = K.warp_perspective if M.shape[1] == 3 else K.warp_affine
    return fn(x, M.cuda(), (h, w), "bilinear", pad, align, fill)


def _both(name, x, pad, align, fill):
    with launch_policy(warp_fwd_algo=3 if name == "minify3" else 0):  # (by default an output smaller than its source keeps the generic kernel)
        box = _run(name, x, pad, align, fill)
    with launch_policy(warp_fwd_algo=1):
        generic = _run(name, x, pad, align, fill)
    return box.cpu(), generic.cpu()


@pytest.mark.parametrize("name", list(MAPS))
@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("pad", PADS)
def test_same_bits_as_the_generic_kernel_fp32(oracle, pad, align, name):
    H, W, h, w, M = MAPS[name]
    C = 3 if pad == "fill" or (list(MAPS).index(name) + int(align)) % 2 == 0 else 1  # (the public fill colour is RGB)
    x = torch.rand(2, C, H, W, generator=torch.Generator().manual_seed(3))
    fill = torch.tensor([0.1, 0.5, 0.9]) if pad == "fill" else None
    box, generic = _both(name, x.cuda(), pad, align, fill)
    assert same_bits(box, generic), f"max |d| = {(box - generic).abs().max().item():.3e}"
    fn = oracle.warp_perspective if M.shape[1] == 3 else oracle.warp_affine
    ref, ref64 = fn(x, M, (h, w), "bilinear", pad, align, fill), fn(x.double(), M.double(), (h, w), "bilinear", pad, align, None if fill is None else fill.double())
    if name == "masked":
        ref[1], ref64[1] = x[1], x[1].double()
    # the fp32 oracle: test_gpu_warp.py's bound for a forward - equality.  The fp64 one: an fp32 position of magnitude <= 512 px carries
    # <= ~10 roundings of 2^-24 relative, 3e-4 px, and a bilinear surface over values in [0, 1] has slope <= 2 per px: 1e-3
    assert same_bits(box, ref), f"max |d| = {(box - ref).abs().max().item():.3e}"
    assert torch.allclose(box.double(), ref64, atol=1e-3, rtol=0, equal_nan=True), f"max |d| = {(box.double() - ref64).abs().max().item():.3e}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("pad,align,name", [("border", False, "rot30"), ("reflection", True, "shift"), ("fill", False, "homography"), ("reflection", False, "zoom_out"),
                                            ("border", True, "shift_nan"), ("fill", True, "masked"), ("border", False, "minify3")])
def test_same_bits_as_the_generic_kernel_16_bit(pad, align, name, dtype):
    H, W = MAPS[name][:2]
    x = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(3)).to(dtype)
    box, generic = _both(name, x.cuda(), pad, align, torch.tensor([0.1, 0.5, 0.9]) if pad == "fill" else None)
    assert same_bits(box, generic)


def test_the_box_kernel_is_taken():
    """the km_warp2d_fwd launch alone at 16x3x512x512 fp32, border, 5 degrees: 3 warm-ups and the median of 10, default policy against
    warp_fwd_algo = 1 (the per-pixel kernel: what every launch of these paddings was before the box kernel, ratio 1)"""
    from kornia_amd import _native as N

    # Measured on the MI355X: generic 0.0302 - 0.0368 ms, box 0.0198 - 0.0246 ms, ratio 1.45 - 1.52 (the box launch moves its 100 MB at
    # ~5 TB/s: no forward of this shape can be twice as fast as the generic one).  Half the measured ratio would be 0.75 - a bound the
    # generic kernel passes against itself - so R is the ratio less 20 %: the 5 % lease-to-lease spread on each of the two times, twice over
    R = 1.2
    B, S = 16, 512
    c, s = math.cos(math.radians(5.0)), math.sin(math.radians(5.0))
    x, out = torch.rand(B, 3, S, S).cuda(), torch.empty(B, 3, S, S).cuda()
    m = torch.tensor([c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0]).expand(B, 9).contiguous().cuda()  # normalised coordinates, dst -> src

    def median_ms(ts=()):
        for _ in range(13):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            N.launch("km_warp2d_fwd", x.device, x.data_ptr(), m.data_ptr(), out.data_ptr(), B, 3, S, S, S, S, B, 1, 1, 1, 1, 0, None, 0)
            ev[1].record()
            ev[1].synchronize()
            ts += (ev[0].elapsed_time(ev[1]),)
        return sorted(ts[3:])[5], out.clone()

    t_box, o_box = median_ms()
    with launch_policy(warp_fwd_algo=1):
        t_generic, o_generic = median_ms()
    print(f"forward 16x3x512x512 fp32, border, 5 degrees: generic {t_generic:.4f} ms, box {t_box:.4f} ms, ratio {t_generic / t_box:.2f} (bound {R})")
    assert same_bits(o_box, o_generic)
    assert t_generic >= R * t_box
