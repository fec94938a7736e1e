"""TEST INFRASTRUCTURE ONLY - the case table that tests/make_golden_nonfinite_pixels.py (against the reference) and
tests/test_zz_gpu_nonfinite_pixels.py (against the native path) share: which images carry a NaN / +inf / -inf PIXEL where, and which call
each recorded result is.  A case is a function of (K, x): K is the reference package in the generator and kornia_amd in the tests, x the
image in the dtype and on the device of the run; everything else a case needs (taps, matrices, factors) it makes from constants, so that the
two sides cannot drift apart.

Values are multiples of 1/8 (so of 1/64) in [0, 1] and the taps dyadic wherever the op leaves the choice, so finite entries are exact in every dtype and
in every order of summation: a difference is a difference of RULE (a skipped tap, a min / max that drops a NaN), not of rounding."""
from __future__ import annotations

import math
from typing import Callable, NamedTuple, Optional

import torch

nan, inf = float("nan"), float("inf")
KINDS = {"nan": nan, "pinf": inf, "ninf": -inf}
DTYPES = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}
# w24: W % 4 == 0 - the register-tiled / vector / LDS-staged paths; w23: the LDS / generic / scalar paths; tall: two strips of the
# register-tiled kernels (rows 15 | 16 and 31 | 32 are strip seams at blur_rows 16 and 32); box: the smallest size at which the warp's
# box forward and the tile-owner backward run (64 x 64, C = 3)
# stage: the smallest size of tests/test_gpu_warp_fused.py::test_source_tile_staging_does_not_depend_on_the_address_or_the_tile_shape (ragged
# tile rows and columns of the one-read backward's LDS staging)
SHAPES = {"w24": (2, 3, 20, 24), "w23": (2, 3, 19, 23), "tall": (2, 3, 40, 24), "box": (2, 3, 64, 64), "stage": (2, 3, 70, 100)}
# (channel, row, column) of the planted pixels of sample 0; negative rows count from the bottom.  The LAST sample is clean.
SITES = {
    "w24": [(1, 7, 9), (0, 0, 0), (2, -1, 5), (0, 11, 3), (0, 11, 4)],
    "w23": [(1, 7, 9), (0, 0, 0), (2, -1, 5), (0, 11, 3), (0, 11, 4)],
    "tall": [(0, 15, 6), (1, 16, 13), (2, 31, 2), (0, 32, 20), (1, -1, 11)],
    "box": [(1, 20, 30), (0, 0, 0), (2, -1, 40), (0, 33, 3), (0, 33, 4)],
    "stage": [(1, 20, 30), (0, 0, 0), (2, -1, 40), (0, 33, 3), (0, 33, 4), (1, 65, 97)],
}


def image(shape_name: str, kind: Optional[str]) -> torch.Tensor:
    """fp32 image of `shape_name`: multiples of 1/8 in [0, 1], sample 0 with the planted value of `kind` (None: clean)."""
    shape = SHAPES[shape_name]
    g = torch.Generator().manual_seed(1000 + sum(shape))
    x = torch.randint(0, 9, shape, generator=g).float() / 8
    if kind is not None:
        for c, r, col in SITES[shape_name]:
            x[0, c, r, col] = KINDS[kind]
    return x


def grad_out(shape, kind: Optional[str]) -> torch.Tensor:
    """integer grad_out in [-2, 2] of `shape` (B first), sample 0 with `kind` at an interior entry, at flat entry 0 and in the last row
    (None: all finite)"""
    g = torch.Generator().manual_seed(2000 + sum(shape))
    go = torch.randint(-2, 3, tuple(shape), generator=g).float()
    if kind is None:
        return go
    v = go[0].reshape(-1, shape[-2], shape[-1])
    v[0, 0, 0] = KINDS[kind]
    v[-1, shape[-2] // 2, shape[-1] // 2] = KINDS[kind]
    v[v.shape[0] // 2, -1, 1] = KINDS[kind]
    return go


def _k(x, rows):
    """taps (1 or B, ...): of a per-sample table the LAST x.shape[0] entries, so that the clean sample alone keeps its own"""
    return torch.tensor(rows, dtype=x.dtype, device=x.device)[-x.shape[0]:]


# ---- taps: all dyadic ---------------------------------------------------------------------------------------------------------------------
K33Z = [[[0.0, 0.25, 0.0], [0.25, 0.0, 0.25], [0.0, 0.25, 0.0]]]                      # zero taps: 0 x inf is NaN in the reference
K33B = K33Z + [[[0.125, 0.0, 0.125], [0.0, 0.5, 0.0], [0.125, 0.0, 0.125]]]          # one kernel per sample
B5 = [1.0, 4.0, 6.0, 4.0, 1.0]
K55 = [[[a * b / 256 for b in B5] for a in B5]]
K77 = [[[(1.0 + (i == 3) + (j == 3)) / 64 for j in range(7)] for i in range(7)]]
K46 = [[[(1.0 + (i % 2)) / 32 for j in range(6)] for i in range(4)]]


def _binomial(n):
    return [[math.comb(n - 1, i) / 2.0 ** (n - 1) for i in range(n)]]


def _flat(n):  # K = 11 / 23: ones with a heavier centre, over a power of two
    return [[(1.0 + 3.0 * (i == n // 2)) / 32 for i in range(n)]]


SEP = {"3": _binomial(3), "5": _binomial(5), "9": _binomial(9), "11": _flat(11), "23": _flat(23)}


def _f2d(k, border, padding="same", normalized=False):
    return lambda K, x: K.filters.filter2d(x, _k(x, k), border, normalized, padding)


def _sep(kx, ky, border):
    return lambda K, x: K.filters.filter2d_separable(x, _k(x, kx), _k(x, ky), border)


def _resize_ref(size, ac):
    return lambda K, x: K.geometry.transform.resize(x, size(x) if callable(size) else size, "bilinear", ac)


def _resize_nat(size, ac):
    return lambda K, x: K.geometry.transform.resize_bilinear(x, size(x) if callable(size) else size, ac)


def _same_size(x):
    return (x.shape[-2], x.shape[-1])


def _twice_less_one(x):  # align_corners=True: every other output is the mean of two neighbours
    return (2 * x.shape[-2] - 1, 2 * x.shape[-1] - 1)


# ---- colour ---------------------------------------------------------------------------------------------------------------------------------
# per sample; the hue shift in RADIANS (adjust_hue's unit) and dyadic like the rest, so that a 16-bit factor tensor holds the same numbers
BF, CF, SF, HF = [1.25, 0.75], [1.5, 0.5], [0.5, 1.5], [0.75, -1.5]
_STAGE = ["adjust_brightness_accumulative", "adjust_contrast_with_mean_subtraction", "adjust_saturation_with_gray_subtraction", "adjust_hue"]


def _factor(x, stage):
    return torch.tensor([BF, CF, SF, HF][stage], dtype=torch.float32, device=x.device)[-x.shape[0]:]


def _stage(stage):
    return lambda K, x: getattr(K.enhance, _STAGE[stage])(x, _factor(x, stage).to(x.dtype))


def _jitter_ref(order):
    def run(K, x):
        for s in order:
            x = _stage(int(s))(K, x)
        return x
    return run


def _jitter_nat(order):
    def run(K, x):
        f = [torch.tensor(v, dtype=torch.float32, device=x.device)[-x.shape[0]:] for v in (BF, CF, SF, HF)]
        return K.enhance.color_jitter(x, f[0], f[1], f[2], f[3] / (2.0 * math.pi), [int(s) for s in order])  # (hue in turns here)
    return run


# ---- warps: dyadic matrices, so positions and bilinear weights are exact (the clean sample 1 has the projective row) ---------------------------------------------------------------------
AFF = [[[1.0, 0.125, -1.5], [-0.0625, 1.0, 2.25]], [[0.875, -0.125, 2.5], [0.125, 1.125, -1.75]]]
PER = [[[1.0, 0.125, -1.5], [-0.0625, 1.0, 2.25], [0.0, 0.0, 1.0]], [[0.875, -0.125, 2.5], [0.125, 1.125, -1.75], [0.0, 1.0 / 1024, 1.0]]]
FILL = [0.25, 0.5, 0.75]


def _warp(api, mode, pad):
    def run(K, x):
        M = torch.tensor(PER if api == "warp_perspective" else AFF, dtype=torch.float32, device=x.device).to(x.dtype)[-x.shape[0]:]
        kw = dict(mode=mode, padding_mode=pad)
        if pad == "fill":
            kw["fill_value"] = torch.tensor(FILL, device=x.device)
        return getattr(K.geometry.transform, api)(x, M, (x.shape[-2], x.shape[-1]), **kw)
    return run


class Case(NamedTuple):
    name: str
    ref: Callable                       # (reference package, x) -> result
    shapes: tuple                       # names of SHAPES
    tol: float = 0.0                    # fp32 / fp64 absolute tolerance of the finite entries: the one the op's own test uses; 0 = torch.equal
    dtypes: tuple = ("f32",)
    nat: Optional[Callable] = None      # (kornia_amd, x) -> result, where the native call is spelled differently
    grad: bool = False                  # also record d/dx with a planted grad_out on the CLEAN image (the linear adjoints)
    extra: tuple = ()                   # 16-bit dtypes that are not recorded: the fp32 record, rounded, is what the native path must give
    tol16: Optional[float] = None       # absolute term next to the 1 ulp of a 16-bit comparison, where it is not `tol`

    def native(self):
        return self.nat or self.ref

    def dtypes_for(self, shape_name: str) -> tuple:
        """the 16-bit / fp64 results are recorded at the two small shapes; the tall and the box image are there for fp32 paths"""
        return self.dtypes + MORE_DTYPES.get(self.name, ()) if shape_name in TWO or self.dtypes == ("f16",) else ("f32",)

    def extra_for(self, shape_name: str) -> tuple:
        return self.extra if shape_name in TWO else ()


ALL = ("f32", "f64", "bf16", "f16")
HALF = ("f32", "bf16", "f16")
THREE = ("w24", "w23", "tall")
TWO = ("w24", "w23")
BORDERS = ("constant", "reflect", "replicate", "circular")

CASES: list[Case] = []
# filter2d: exact (tests/test_gpu_golden.py compares torch.equal)
for _b in BORDERS:
    CASES.append(Case(f"f2d_3x3z_{_b}", _f2d(K33Z, _b), TWO, dtypes=ALL if _b == "reflect" else ("f32",), grad=_b in ("reflect", "constant")))
CASES += [
    Case("f2d_3x3z_valid", _f2d(K33Z, "constant", "valid"), TWO),
    Case("f2d_3x3_batch_reflect", _f2d(K33B, "reflect"), TWO),
    Case("f2d_3x3_batch_valid", _f2d(K33B, "replicate", "valid"), TWO),
    Case("f2d_5x5_reflect", _f2d(K55, "reflect"), TWO, dtypes=("f32", "bf16")),
    Case("f2d_5x5_circular", _f2d(K55, "circular"), TWO),
    Case("f2d_5x5_valid", _f2d(K55, "reflect", "valid"), TWO),
    Case("f2d_7x7_replicate", _f2d(K77, "replicate"), TWO),
    Case("f2d_4x6_constant", _f2d(K46, "constant"), TWO),
    Case("f2d_4x6_circular", _f2d(K46, "circular"), TWO),
]
# separable: K = 3 / 5 / 9 the register-tiled kernel, 11 / 23 the sliding window, 4 x 2 the LDS kernel
for _n, _t in SEP.items():
    CASES.append(Case(f"sep_{_n}_reflect", _sep(_t, _t, "reflect"), THREE if _n in ("5", "9", "11") else TWO, dtypes=ALL if _n == "5" else ("f32",), grad=_n in ("5", "11")))
CASES += [
    Case("sep_5_constant", _sep(SEP["5"], SEP["5"], "constant"), TWO),
    Case("sep_5_replicate", _sep(SEP["5"], SEP["5"], "replicate"), TWO),
    Case("sep_5_circular", _sep(SEP["5"], SEP["5"], "circular"), TWO),
    Case("sep_9x3_replicate", _sep(SEP["9"], SEP["3"], "replicate"), THREE),
    Case("sep_4x2_reflect", _sep([[0.25, 0.25, 0.25, 0.25]], [[0.5, 0.5]], "reflect"), TWO, grad=True),
    Case("box_blur_4x2", lambda K, x: K.filters.box_blur(x, (4, 2)), TWO),
    Case("box_blur_2x2_sep", lambda K, x: K.filters.box_blur(x, (2, 2), "replicate", True), TWO),
]
for _m in ("sobel", "diff"):
    for _o in (1, 2):
        for _nz in (True, False):
            CASES.append(Case(f"sg_{_m}_{_o}_{int(_nz)}", (lambda m, o, nz: lambda K, x: K.filters.spatial_gradient(x, m, o, nz))(_m, _o, _nz),
                              THREE if (_o, _nz) == (1, True) else TWO, dtypes=("f32", "f16") if (_m, _o, _nz) == ("sobel", 1, True) else ("f32",), grad=_nz and _o == 1))
CASES.append(Case("sobel", lambda K, x: K.filters.sobel(x), TWO, tol=1e-7))
# pyramid: 1e-6 against the reference (tests/test_gpu_pyramid.py), resize 2e-6
for _b in BORDERS:
    for _ac in (False, True):
        if _b == "reflect" or not _ac:
            CASES.append(Case(f"pyrdown_{_b}_{int(_ac)}", (lambda b, ac: lambda K, x: K.geometry.transform.pyrdown(x, b, ac))(_b, _ac),
                              THREE if _b == "reflect" else TWO, tol=1e-6, dtypes=("f32", "bf16") if (_b, _ac) == ("reflect", False) else ("f32",), grad=_b == "reflect"))
CASES += [
    Case("pyrdown_f15_0", lambda K, x: K.geometry.transform.pyrdown(x, "reflect", False, 1.5), TWO, tol=1e-6),
    Case("pyrdown_f15_1", lambda K, x: K.geometry.transform.pyrdown(x, "replicate", True, 1.5), TWO, tol=1e-6),
    Case("pyrup_0", lambda K, x: K.geometry.transform.pyrup(x, "reflect", False), TWO, tol=1e-6, dtypes=HALF, grad=True),
    Case("pyrup_1", lambda K, x: K.geometry.transform.pyrup(x, "replicate", True), ("w24",), tol=1e-6, grad=True),
    Case("resize_up_0", _resize_ref((37, 41), False), ("w23",), tol=2e-6, nat=_resize_nat((37, 41), False), grad=True),
    Case("resize_up_1", _resize_ref(_twice_less_one, True), TWO, tol=2e-6, nat=_resize_nat(_twice_less_one, True)),
    Case("resize_same_0", _resize_ref(_same_size, False), TWO, tol=2e-6, nat=_resize_nat(_same_size, False)),
    Case("resize_same_1", _resize_ref(_same_size, True), TWO, tol=2e-6, nat=_resize_nat(_same_size, True)),
    Case("resize_down_0", _resize_ref((9, 13), False), TWO, tol=2e-6, nat=_resize_nat((9, 13), False), dtypes=HALF, grad=True),
    Case("resize_down_1", _resize_ref((10, 12), True), TWO, tol=2e-6, nat=_resize_nat((10, 12), True)),
    Case("resize_one_row", _resize_ref((1, 16), False), TWO, tol=2e-6, nat=_resize_nat((1, 16), False)),
    Case("resize_one_col", _resize_ref((16, 1), True), TWO, tol=2e-6, nat=_resize_nat((16, 1), True)),
]
# colour: 5e-6 (tests/test_gpu_color.py TOL); the reference's colour ops need a floating dtype its CPU kernels have: f32 / bf16 / f16
# f16 is held to the fp32 record (Case.extra), not to the reference's own f16 result: its rgb_to_hsv adds eps = 1e-8 in f16, where it is 0, so
# every BLACK pixel of a clean f16 image is 0 / 0 = NaN after adjust_hue - the native path computes in fp32, where the pixel stays black.
# The fused sequence keeps one intermediate image in the storage dtype (in front of the contrast stage) and the reference rounds after
# every torch op, so in 16-bit neither is the other's rounding: 1e-2 there, as tests/test_gpu_color.py::test_half_precision_and_errors.
for _s, _n in enumerate(("brightness", "contrast", "saturation", "hue")):
    CASES.append(Case(_n, _stage(_s), TWO, tol=5e-6, dtypes=("f32", "bf16"), extra=("f16",)))
for _o in ("0123", "2031"):
    CASES.append(Case(f"jitter_{_o}", _jitter_ref(_o), TWO, tol=1e-5, dtypes=("f32", "bf16"), extra=("f16",), nat=_jitter_nat(_o), tol16=1e-2))
# warps: bilinear / nearest exact (tests/test_gpu_golden.py), bicubic 2e-6.  The reference computes a 16-bit warp's sampling positions in
# the 16-bit dtype (other pixels than the fp32 warp reads); the native path computes them in fp32 and rounds the result once
# (tests/test_gpu_warp.py::test_16_bit_storage_is_the_fp32_result_rounded_once), so 16-bit warps are held to the fp32 record
for _api in ("warp_perspective", "warp_affine"):
    for _mode in ("bilinear", "bicubic", "nearest"):
        for _pad in ("zeros", "border", "reflection", "fill"):
            if _api == "warp_affine" and _pad in ("reflection", "fill") and _mode != "bilinear":
                continue
            CASES.append(Case(f"{_api}_{_mode}_{_pad}", _warp(_api, _mode, _pad), ("w24", "w23", "box") if (_api, _pad) == ("warp_perspective", "zeros") and _mode == "bilinear" else TWO, tol=2e-6 if _mode == "bicubic" else 0.0,
                              extra=("bf16", "f16") if (_api, _pad) == ("warp_perspective", "zeros") else ()))

# ---- the second file (tests/golden/nonfinite_pixels_2.npz: one committed file holds at most 1 MiB) -------------------------------------------
# further dtypes of cases above, so that every op family's fp64 and 16-bit instantiations see a non-finite pixel
MORE_DTYPES = {
    "f2d_5x5_circular": ("f64",), "f2d_4x6_constant": ("f64", "f16"), "f2d_7x7_replicate": ("bf16",), "sep_11_reflect": ("f64", "bf16"), "sep_4x2_reflect": ("f64", "f16"),
    "sg_sobel_1_1": ("f64", "bf16"), "sg_diff_2_0": ("f64",), "pyrdown_reflect_0": ("f64", "f16"), "pyrdown_f15_0": ("f64",), "pyrup_0": ("f64",),
    "resize_up_1": ("f64", "bf16"), "resize_same_0": ("f64",), "resize_down_0": ("f64",),
    "warp_perspective_bilinear_zeros": ("f64",), "warp_perspective_bicubic_zeros": ("f64",), "warp_perspective_nearest_border": ("f64",), "warp_affine_bilinear_reflection": ("f64",),
}

# Stated difference: the reference's bf16 spatial_gradient (ATen's bf16 conv3d on the CPU) returns NaN / inf OUTSIDE the
# 3 x 3 window of a planted pixel - two columns to its left, and in the row's last column for pixel (0, 0) - which no tap reaches; its fp32, fp64
# and f16 results do not.  The record is kept; the native bf16 result is held to the fp32 record's pattern, as a Case.extra dtype is.
STATED = {("sg_sobel_1_1", "bf16")}

# crop_by_indices: one box per sample (x, y corners: top-left, top-right, bottom-right, bottom-left).  Sample 0's window is 16 columns by the
# whole height, so every planted pixel is inside it; the clean sample's is the output size itself (the copy path - also what keeps its
# result the same when it is called alone, where the reference resizes whatever shape_compensation says)
def _boxes(x, second):
    H = x.shape[-2]
    b0 = [[0.0, 0.0], [15.0, 0.0], [15.0, H - 1.0], [0.0, H - 1.0]]
    (x1, y1), (w, h) = second
    b1 = [[x1, y1], [x1 + w - 1.0, y1], [x1 + w - 1.0, y1 + h - 1.0], [x1, y1 + h - 1.0]]
    return torch.tensor([b0, b1], device=x.device)[-x.shape[0]:]


def _crop(size, interpolation, compensation="resize", origin=(4.0, 2.0)):
    def run(K, x):
        kw = {} if interpolation == "nearest" else {"align_corners": False}
        return K.geometry.transform.crop_by_indices(x, _boxes(x, (origin, (size[1], size[0]))), size, interpolation, shape_compensation=compensation, **kw)
    return run


def _label_mask(x):  # uint8 labels 0 .. 6, (B,1,H,W)
    B, _, H, W = x.shape
    r, c = torch.arange(H, device=x.device)[:, None], torch.arange(W, device=x.device)[None, :]
    return ((r * 3 + c * 5) % 7).to(torch.uint8).expand(B, 1, H, W).contiguous()


_FLIP_X, _FLIP_Y = [1.0, 0.0], [1.0, 1.0]  # per sample


def _crop_flip_mask_ref(K, x):
    """the crop of the image (bilinear) and of a uint8 label mask (nearest), both then mirrored per sample: image and mask side by side in x's dtype"""
    size, B = (10, 12), x.shape[0]
    boxes = _boxes(x, ((4.0, 2.0), (12.0, 10.0)))
    img = K.geometry.transform.crop_by_indices(x, boxes, size, "bilinear", align_corners=False)
    msk = K.geometry.transform.crop_by_indices(_label_mask(x).to(x.dtype), boxes, size, "nearest").to(torch.uint8)
    out = torch.cat([img, msk.to(x.dtype)], 1)
    rows = []
    for i in range(B):
        dims = [d for d, f in ((-1, _FLIP_X[-B:][i]), (-2, _FLIP_Y[-B:][i])) if f > 0.5]
        rows.append(torch.flip(out[i], dims) if dims else out[i])
    return torch.stack(rows)


def _crop_flip_mask_nat(K, x):
    B = x.shape[0]
    fx, fy = (torch.tensor(f, device=x.device)[-B:] for f in (_FLIP_X, _FLIP_Y))
    img, msk = K.geometry.transform.crop2d.crop_resize(x, _label_mask(x), _boxes(x, ((4.0, 2.0), (12.0, 10.0))), (10, 12), "bilinear", False, "resize", fx, fy)
    assert msk.dtype == torch.uint8
    return torch.cat([img, msk.to(x.dtype)], 1)


# an explicit sampling map in pixels: every position an ODD multiple of 1/16, so none sits on a pixel centre, where the last bit of the
# normalise / un-normalise round trip would decide whether a zero-weight tap - and with it a NaN - is read
def _maps(x):
    B, _, H, W = x.shape
    r, c = torch.arange(H, dtype=x.dtype, device=x.device)[:, None], torch.arange(W, dtype=x.dtype, device=x.device)[None, :]
    mx = torch.stack([c * 0.875 + r * 0.25 - 1.6875, c * 1.125 - r * 0.25 + 0.8125])
    my = torch.stack([r * 1.125 - c * 0.125 + 0.5625, r * 0.875 + c * 0.125 - 0.9375])
    return mx[-B:], my[-B:]


def _remap(mode, pad, align):
    return lambda K, x: K.geometry.transform.remap(x, *_maps(x), mode=mode, padding_mode=pad, align_corners=align)


def _grid(x):
    mx, my = _maps(x)
    H, W = x.shape[-2:]
    return torch.stack([(2.0 * mx + 1.0) / W - 1.0, (2.0 * my + 1.0) / H - 1.0], -1)  # align_corners=False


def _grid_sample_ref(mode, pad):
    return lambda K, x: torch.nn.functional.grid_sample(x, _grid(x), mode, pad, align_corners=False)


def _grid_sample_nat(mode, pad):
    return lambda K, x: K.geometry.transform.grid_sample(x, _grid(x), mode, pad, align_corners=False)


HN = [[[1.0, 0.0625, 0.03125], [-0.03125, 1.0, -0.0625], [0.0, 0.015625, 1.0]], [[0.9375, -0.0625, 0.0625], [0.0625, 1.0625, -0.03125], [0.0, 0.0, 1.0]]]


def _homography_warp(mode, pad, align):
    def run(K, x):
        Hn = torch.tensor(HN, dtype=x.dtype, device=x.device)[-x.shape[0]:]
        return K.geometry.transform.homography_warp(x, Hn, (x.shape[-2], x.shape[-1]), mode, pad, align)
    return run


def _warp_blur_ref(ksize, sigma):
    def run(K, x):
        M = torch.tensor(PER, dtype=x.dtype, device=x.device)[-x.shape[0]:]
        return K.filters.gaussian_blur2d(K.geometry.transform.warp_perspective(x, M, (x.shape[-2], x.shape[-1])), ksize, sigma, "reflect")
    return run


def _warp_blur_nat(ksize, sigma):
    def run(K, x):
        M = torch.tensor(PER, dtype=x.dtype, device=x.device)[-x.shape[0]:]
        return K.geometry.transform.warp_perspective_blur(x, M, (x.shape[-2], x.shape[-1]), ksize, sigma)
    return run


# a general (non-dyadic) projective matrix: positions and the bicubic weights of both signs are rounded, unlike PER's
GEN = [[[0.97, 0.11, -1.3], [-0.07, 1.04, 2.1], [1e-3, -7e-4, 1.0]], [[1.03, -0.09, 0.7], [0.05, 0.96, -1.9], [-5e-4, 9e-4, 1.0]]]


def _warp_general(mode):
    def run(K, x):
        M = torch.tensor(GEN, dtype=torch.float32, device=x.device).to(x.dtype)[-x.shape[0]:]
        return K.geometry.transform.warp_perspective(x, M, (x.shape[-2], x.shape[-1]), mode=mode, padding_mode="zeros")
    return run


# tolerances: resize 2e-6 as above (the crop's resize is F.interpolate); the samplers with a general grid 1e-5, the bound of
# tests/test_gpu_config_parity.py for homography_warp (positions are not dyadic after the normalisation); warp + Gaussian blur 1e-6 as the pyramid
CASES2 = [
    Case("crop_bilinear_resize", _crop((10, 12), "bilinear"), TWO, tol=2e-6, extra=("bf16",)),
    Case("crop_nearest_resize", _crop((10, 12), "nearest"), TWO),
    Case("crop_bilinear_pad", _crop((12, 20), "bilinear", "pad", (0.0, 2.0)), TWO),
    Case("crop_nearest_pad", _crop((12, 20), "nearest", "pad", (0.0, 2.0)), TWO),
    Case("crop_flip_mask", _crop_flip_mask_ref, TWO, tol=2e-6, nat=_crop_flip_mask_nat),
    Case("remap_bilinear_zeros", _remap("bilinear", "zeros", False), TWO, tol=1e-5),
    Case("remap_bilinear_border_ac", _remap("bilinear", "border", True), TWO, tol=1e-5),
    Case("remap_nearest_reflection", _remap("nearest", "reflection", False), TWO),
    Case("remap_bicubic_zeros", _remap("bicubic", "zeros", False), TWO, tol=1e-5),
    Case("grid_sample_bilinear_border", _grid_sample_ref("bilinear", "border"), TWO, tol=1e-5, nat=_grid_sample_nat("bilinear", "border")),
    Case("grid_sample_bicubic_reflection", _grid_sample_ref("bicubic", "reflection"), TWO, tol=1e-5, nat=_grid_sample_nat("bicubic", "reflection")),
    Case("homography_warp_bilinear_zeros", _homography_warp("bilinear", "zeros", False), ("w24", "w23", "box"), tol=1e-5),
    Case("homography_warp_bilinear_border_ac", _homography_warp("bilinear", "border", True), TWO, tol=1e-5),
    Case("homography_warp_nearest_zeros", _homography_warp("nearest", "zeros", False), TWO),
    Case("warp_perspective_blur_5", _warp_blur_ref((5, 5), (1.5, 1.5)), ("w24", "w23", "box"), tol=1e-6, nat=_warp_blur_nat((5, 5), (1.5, 1.5))),
    Case("warp_perspective_bicubic_zeros_general", _warp_general("bicubic"), TWO, tol=2e-6),
    Case("warp_perspective_blur_3", _warp_blur_ref((3, 3), (0.75, 0.75)), TWO, tol=1e-6, nat=_warp_blur_nat((3, 3), (0.75, 0.75))),
]
ALL_CASES = CASES + CASES2
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


def in_second_file(case: Case, dname: str) -> bool:
    return case in CASES2 or dname in MORE_DTYPES.get(case.name, ())


# masked_warp_loss: loss_fn(homography_warp(src, H), dst, 'none').masked_select(homography_warp(ones, H) > threshold).mean(); threshold None:
# the plain mean.  src is the image with the planted pixels, dst a clean one.
LOSSES = [("l1", 0.9), ("l1", None), ("mse", 0.9), ("mse", None)]


def loss_reference(K, src, dst, kind, threshold):
    Hn = torch.tensor(HN, dtype=src.dtype)
    fn = torch.nn.functional.l1_loss if kind == "l1" else torch.nn.functional.mse_loss
    warped = K.geometry.transform.homography_warp(src, Hn, src.shape[-2:])
    if threshold is None:
        return fn(warped, dst)
    ones = K.geometry.transform.homography_warp(torch.ones_like(src), Hn, src.shape[-2:])
    return fn(warped, dst, reduction="none").masked_select(ones > threshold).mean()


def points(kind: Optional[str]) -> torch.Tensor:
    """(2, 7, 2) points, multiples of 1/4; sample 0 with `kind` as one point's x and another point's y"""
    p = torch.randint(-40, 41, (2, 7, 2), generator=torch.Generator().manual_seed(7)).float() / 4
    if kind is not None:
        p[0, 2, 0] = KINDS[kind]
        p[0, 5, 1] = KINDS[kind]
    return p


# both gradients of the bilinear warp with non-finite PIXELS (grad_out is finite): shapes and the path each is there for
WARP_GRADS = [("zeros", "w24"), ("zeros", "w23"), ("zeros", "box"), ("zeros", "stage"), ("fill", "box"), ("border", "w23")]


def warp_grad_call(K, x, M, pad):
    kw = dict(mode="bilinear", padding_mode=pad)
    if pad == "fill":
        kw["fill_value"] = torch.tensor(FILL, device=x.device)
    return K.geometry.transform.warp_perspective(x, M, (x.shape[-2], x.shape[-1]), **kw)

# f16 only: a finite image whose result overflows - 60000 under a 2-tap box of weight 1 each; the reference gives inf
OVERFLOW = Case("f16_overflow_2tap", _sep([[1.0, 1.0]], [[1.0]], "replicate"), ("w24", "w23"), dtypes=("f16",))


def overflow_image(shape_name: str) -> torch.Tensor:
    x = image(shape_name, None)
    x[0] = 60000.0
    return x


def key(case: Case, shape_name: str, dname: str, what: str = "y") -> str:
    """the fixture's array of a case: sample 0 of the result for each of KINDS, stacked in that order along a new LAST axis (the three differ
    near the planted pixels only, which the compressor then stores once)"""
    return f"{case.name}__{shape_name}__{dname}__{what}"
