"""Generates tests/golden/bilateral_blur.npz from the reference (Kornia) - run in a checkout next to the reference tree, not by the suite:

    python tests/make_golden_bilateral.py

``kornia.filters.bilateral_blur`` and ``joint_bilateral_blur`` (2-channel guidance) in float32 AND float64 on windows {3x3, 5x5, 9x9, 3x7, 15x15}
x {l1, l2} x 4 borders x sigma_color {0.1, 0.5} x shapes {(2,3,13,17), (1,1,9,12), (2,4,16,24)}.  The full cross product is 480 cases and
8 MB of outputs, so the grid is covered by a rotating design (every case listed in ``cases``):

  * (1,1,9,12): every window x border x distance, sigma_color and the function rotating;
  * (2,3,13,17): every window x function, border / distance / sigma_color rotating;
  * (2,4,16,24): one case per border, the rest rotating;

so that every value of every factor meets every shape.  Windows whose reflect pad does not fit are skipped (none at these shapes).  Besides:
one case with ``sigma_color`` a (B,) tensor and ``sigma_space`` a (B,2) tensor; the reference's float64 gradients wrt input (and wrt input and
guidance for the joint form) for a fixed ``randn`` grad_out at 5x5 and (3,7), both distances, all four borders, on (2,3,13,17); two non-finite
7x7 images with 3x3 windows (a NaN, then a +inf, at the centre); the exception type names the reference raises for even windows and a bad
distance name; and for every float32 entry the reference's own max |float32 - float64| (``self_err``, in the order of ``cases``).
Arrays only.  Images hold multiples of 1/64 in [0, 1]."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

WINDOWS = [(3, 3), (5, 5), (9, 9), (3, 7), (15, 15)]
DISTS = ["l1", "l2"]
BORDERS = ["constant", "reflect", "replicate", "circular"]
SIGMA_COLORS = [0.1, 0.5]
SHAPES = [(2, 3, 13, 17), (1, 1, 9, 12), (2, 4, 16, 24)]
FUNCS = ["self", "joint"]
SIGMA_SPACE = (1.5, 1.1)  # (sigma_y, sigma_x): unequal, so that a swapped pair shows
GRAD_WINDOWS = [(5, 5), (3, 7)]
GRAD_SHAPE = (2, 3, 13, 17)
GUIDE_CHANNELS = 2


def sname(shape) -> str:
    return "x".join(str(v) for v in shape)


def kname(k) -> str:
    return f"{k[0]}x{k[1]}"


def case_key(func, shape, k, dist, border, sc) -> str:
    return f"{func}__{sname(shape)}__{kname(k)}__{dist}__{border}__sc{sc}"


def design():
    """the rotating design of the module docstring: a list of (func, shape, window, dist, border, sigma_color)"""
    cases = []
    n = 0
    for k in WINDOWS:  # (1,1,9,12): window x border x distance
        for border in BORDERS:
            for dist in DISTS:
                cases.append((FUNCS[n % 2], SHAPES[1], k, dist, border, SIGMA_COLORS[(n // 2) % 2]))
                n += 1
    n = 0
    for k in WINDOWS:  # (2,3,13,17): window x function
        for func in FUNCS:
            cases.append((func, SHAPES[0], k, DISTS[n % 2], BORDERS[(n + n // 4) % 4], SIGMA_COLORS[(n // 2) % 2]))
            n += 1
    for n, border in enumerate(BORDERS):  # (2,4,16,24): one per border
        cases.append((FUNCS[n % 2], SHAPES[2], WINDOWS[(2 * n + 1) % 5], DISTS[(n // 2) % 2], border, SIGMA_COLORS[(n + 1) % 2]))
    return cases


def pad_fits(border, k, shape) -> bool:
    return border != "reflect" or (k[0] // 2 < shape[2] and k[1] // 2 < shape[3])


def main() -> None:
    from ref_shim import import_reference

    K = import_reference()
    F = K.filters
    g = torch.Generator().manual_seed(2207)
    d = {}
    for shape in SHAPES:
        d[f"x__{sname(shape)}"] = torch.randint(0, 65, shape, generator=g).float() / 64
        d[f"g__{sname(shape)}"] = torch.randint(0, 65, (shape[0], GUIDE_CHANNELS, shape[2], shape[3]), generator=g).float() / 64

    def run(func, x, gd, k, sc, ss, border, dist):
        if func == "self":
            return F.bilateral_blur(x, k, sc, ss, border, dist)
        return F.joint_bilateral_blur(x, gd, k, sc, ss, border, dist)

    # i. the parity design
    keys, self_err = [], []
    for func, shape, k, dist, border, sc in design():
        if not pad_fits(border, k, shape):
            continue
        x, gd = d[f"x__{sname(shape)}"], d[f"g__{sname(shape)}"]
        y32 = run(func, x, gd, k, sc, SIGMA_SPACE, border, dist)
        y64 = run(func, x.double(), gd.double(), k, sc, SIGMA_SPACE, border, dist)
        assert y32.dtype == torch.float32 and y64.dtype == torch.float64 and y32.shape == x.shape
        key = case_key(func, shape, k, dist, border, sc)
        d[f"y__{key}__f32"], d[f"y__{key}__f64"] = y32, y64
        keys.append(key)
        self_err.append((y32.double() - y64).abs().max().item())
    # an int kernel size is the square window
    assert torch.equal(F.bilateral_blur(d["x__1x1x9x12"], 3, 0.5, SIGMA_SPACE), F.bilateral_blur(d["x__1x1x9x12"], (3, 3), 0.5, SIGMA_SPACE))
    # ii. tensor sigmas
    x, gd = d["x__2x3x13x17"], d["g__2x3x13x17"]
    d["ts__sigma_color"] = torch.tensor([0.2, 0.6])
    d["ts__sigma_space"] = torch.tensor([[1.5, 1.1], [0.8, 2.0]])
    for func in FUNCS:
        for dn, dt in (("f32", torch.float32), ("f64", torch.float64)):
            d[f"ts__{func}__{dn}"] = run(func, x.to(dt), gd.to(dt), (5, 5), d["ts__sigma_color"].to(dt), d["ts__sigma_space"].to(dt), "reflect", "l1")
    # iii. float64 gradients for a fixed grad_out
    gout = torch.randn(GRAD_SHAPE, generator=g, dtype=torch.float64)
    d["grad__gout"] = gout
    grad_err = []
    for k in GRAD_WINDOWS:
        for dist in DISTS:
            for border in BORDERS:
                tag = f"{kname(k)}__{dist}__{border}"
                res = {}
                for dt in (torch.float64, torch.float32):
                    xr = x.to(dt).clone().requires_grad_()
                    F.bilateral_blur(xr, k, 0.5, SIGMA_SPACE, border, dist).backward(gout.to(dt))
                    xj, gj = x.to(dt).clone().requires_grad_(), gd.to(dt).clone().requires_grad_()
                    F.joint_bilateral_blur(xj, gj, k, 0.5, SIGMA_SPACE, border, dist).backward(gout.to(dt))
                    res[dt] = (xr.grad, xj.grad, gj.grad)
                d[f"grad__self__{tag}__gx"], d[f"grad__joint__{tag}__gx"], d[f"grad__joint__{tag}__gg"] = res[torch.float64]
                # the reference's own float32 gradients against its float64 ones, on the scale of the largest entry
                grad_err.append(max(((a.double() - b).abs().max() / b.abs().max()).item() for a, b in zip(res[torch.float32], res[torch.float64])))
    # iv. non-finite: a NaN / a +inf at the centre of a 7 x 7 image, 3 x 3 window
    for name, bad in (("nan", float("nan")), ("inf", float("inf"))):
        xn = torch.randint(0, 65, (1, 1, 7, 7), generator=g).float() / 64
        xn[0, 0, 3, 3] = bad
        d[f"nf_{name}__x"] = xn
        d[f"nf_{name}__y"] = F.bilateral_blur(xn, (3, 3), 0.5, SIGMA_SPACE)
    # v. what the reference raises
    names = []
    z = torch.rand(1, 1, 8, 8)
    for k, dist in ((4, "l1"), ((3, 4), "l1"), ((3, 3), "l3")):
        try:
            F.bilateral_blur(z, k, 0.5, SIGMA_SPACE, "reflect", dist)
            names.append("none")
        except Exception as e:  # noqa: BLE001
            names.append(type(e).__name__)
    arrays = {k: v.contiguous().numpy() for k, v in d.items()}
    arrays["cases"] = np.array(keys)
    arrays["self_err"] = np.array(self_err)
    arrays["grad_self_err"] = np.array(grad_err)
    arrays["raises__what"] = np.array(["kernel_size=4", "kernel_size=(3, 4)", "color_distance_type=l3"])
    arrays["raises__type"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "bilateral_blur.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes;", len(keys), "cases; reference fp32 vs fp64: forward max", max(self_err), "gradient max (of the largest entry)",
          max(grad_err), names)


if __name__ == "__main__":
    torch.set_num_threads(4)
    main()
