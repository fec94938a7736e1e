"""CPU: the C-ABI library builds, loads and exports every symbol include/kornia_amd.h declares; the
host-side mirror validates arguments like the reference and refuses to run without a HIP device
(no CPU fallback).  No compute call is made here."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "kornia_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(km_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from kornia_amd import _native, build

    path = build.build()
    assert os.path.exists(path)
    lib = ctypes.CDLL(path)
    declared = _declared_symbols()
    assert len(declared) >= 18
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/kornia_amd.h but not exported"
    # the Python binding covers the whole header too
    assert sorted(_native.exported_symbols()) == declared
    lib.km_abi_version.restype = ctypes.c_int
    assert lib.km_abi_version() == _native.ABI_VERSION


def test_bad_arguments_return_error_codes_without_a_gpu():
    from kornia_amd import _native

    lib = _native.lib()
    rc = lib.km_warp2d_fwd(None, None, None, 1, 3, 8, 8, 8, 8, 1, 0, 1, 1, 0, 1, None, 0, None)
    assert rc < 0 and b"null pointer" in lib.km_last_error()
    buf = ctypes.create_string_buffer(64)
    rc = lib.km_filter2d_fwd(buf, buf, buf, 2, 3, 8, 8, 3, 3, 3, 1, 1, 0, None)  # Bk=3 does not divide B=2
    assert rc < 0 and b"must divide" in lib.km_last_error()
    rc = lib.km_homography_chain_fwd(buf, 4, buf, buf, 1, 8, 8, 8, 8, 0, None)
    assert rc < 0 and b"rows must be 2 or 3" in lib.km_last_error()
    # bit 0: fused forward, bit 1: fused adjoint;  23x23 (SimCLR-style blur): forward only;  99 taps: neither
    assert lib.km_filter2d_sep_supported(5, 5, 1, 0) == 3 and lib.km_filter2d_sep_supported(23, 23, 1, 0) == 1
    assert lib.km_filter2d_sep_supported(99, 5, 1, 0) == 0
    assert lib.km_warp2d_bwd_needs_zero_init(1, 0, 0) == 0 and lib.km_warp2d_bwd_needs_zero_init(2, 0, 0) == 1
    # the tail of the fused loss step
    rc = lib.km_warp_masked_loss_finish(buf, 4, 2, buf, None, buf, None)  # B_M must be 1 or B
    assert rc < 0 and b"B_M in {1, B}" in lib.km_last_error()
    rc = lib.km_warp_masked_loss_finish(None, 4, 4, buf, None, buf, None)
    assert rc < 0 and b"null pointer" in lib.km_last_error()
    rc = lib.km_scale_f64(buf, buf, 2, buf, 0, 9, None)  # a bf16 scale
    assert rc < 0 and b"dtypes must be f32 (0) or f64 (1)" in lib.km_last_error()
    assert lib.km_scale_f64(None, None, 0, None, 0, 0, None) == 0  # nothing to do


def test_warp_entry_points_host_contract_without_a_gpu():
    """What the warp entry points decide on the host, before any launch: the argument checks with their messages, the empty
    calls, and the two predicates the Python layer plans its buffers with (closed forms over every mode code)."""
    from kornia_amd import _native

    lib = _native.lib()
    buf = ctypes.create_string_buffer(64)

    def fwd(src=buf, mat=buf, dst=buf, B=1, C=3, H=8, W=8, h=8, w=8, B_M=1, cm=0, interp=1, pad=0, fill=None, dtype=0, fn=lib.km_warp2d_fwd, extra=()):
        return fn(src, mat, dst, *extra, B, C, H, W, h, w, B_M, cm, 1, interp, pad, 1, fill, dtype, None)

    def rejected(rc, fragment):
        assert rc < 0 and fragment in lib.km_last_error(), (rc, fragment, lib.km_last_error())

    rejected(fwd(src=None, mat=None, dst=None), b"null pointer")
    rejected(fwd(B=2, B_M=3), b"matrix batch 3 must be 1 or 2")
    rejected(fwd(cm=3), b"bad coord_mode 3")
    rejected(fwd(interp=3), b"bad interp 3")
    rejected(fwd(pad=4), b"bad pad 4")
    rejected(fwd(pad=3), b"pad=fill needs fill values")
    rejected(fwd(dtype=4), b"bad dtype 4")
    rejected(fwd(H=65536, W=32768), b"image plane exceeds 2^31 elements")
    rejected(fwd(H=0), b"bad shape")
    rejected(fwd(dst=None), b"km_warp2d_fwd: null dst")
    assert fwd(src=None, mat=None, dst=None, B=0) == 0 and fwd(src=None, mat=None, dst=None, h=0) == 0  # empty outputs

    masked = dict(fn=lib.km_warp2d_fwd_masked, extra=(buf,))
    rejected(fwd(h=4, w=4, **masked), b"needs equal source and destination sizes")
    rc = fwd(src=None, mat=None, dst=None, fn=lib.km_warp2d_fwd_masked, extra=(None,))
    assert rc < 0 and lib.km_last_error().startswith(b"km_warp2d_fwd_masked:") and b"null pointer" in lib.km_last_error()

    def bwd_ws(gout=buf, gsrc=buf, gmat=buf, B=1):
        return lib.km_warp2d_bwd_ws(gout, buf, buf, gsrc, gmat, B, 3, 8, 8, 8, 8, 1, 0, 1, 1, 0, 1, None, 0, None, 0, None)

    rejected(bwd_ws(gout=None), b"km_warp2d_bwd: null gout")
    assert bwd_ws(gsrc=None, gmat=None) == 0
    assert lib.km_warp2d_bwd(None, None, None, None, None, 0, 3, 8, 8, 8, 8, 1, 0, 1, 1, 0, 1, None, 0, None) == 0

    rejected(lib.km_grid_sample2d_fwd(buf, buf, buf, 1, 3, 8, 8, 8, 8, 1, 1, 3, 1, 0, None), b"pad=fill needs fill values")

    def grid_bwd(gout=buf, gsrc=buf, ggrid=buf):
        return lib.km_grid_sample2d_bwd(gout, buf, buf, gsrc, ggrid, 1, 3, 8, 8, 8, 8, 1, 1, 0, 1, 0, None)

    rejected(grid_bwd(gout=None), b"km_grid_sample2d_bwd: null gout")
    assert grid_bwd(gsrc=None, ggrid=None) == 0

    def loss(W=8, dtype=0):
        return lib.km_warp_masked_loss(buf, buf, buf, buf, 1, 3, 8, W, 8, 8, 1, 0, 1, 1, 0, 0.0, dtype, None)

    rejected(loss(dtype=1), b"dtype must be f32 / bf16 / f16")
    rejected(loss(W=1), b"at least two columns")

    modes = [(interp, pad, dtype) for interp in range(3) for pad in range(4) for dtype in range(4)]
    for interp, pad, dtype in modes:
        owner = interp == 1 and pad in (0, 3) and dtype != 1
        assert lib.km_warp2d_bwd_needs_zero_init(interp, pad, dtype) == (0 if owner else 1), (interp, pad, dtype)
    shapes = [(2, 3, 65, 64, 7, 9), (1, 1, 1, 1, 1, 1), (3, 4, 130, 200, 64, 64), (2, 5, 64, 64, 8, 8), (2, 2, 64, 65, 8, 8), (0, 3, 8, 8, 8, 8),
              (1, 3, 8, 8, 0, 8), (1, 3, 32768, 32768, 8, 8), (1, 3, 8, 8, 32768, 32768), (1, 3, 32767, 32768, 8, 8)]
    for B, C, H, W, h, w in shapes:
        for interp, pad, dtype in modes:
            none = (min(B, C, H, W, h, w) <= 0 or interp != 1 or dtype == 1 or (pad in (1, 2) and dtype != 0) or (pad == 3 and C not in (1, 3))
                    or 4 * H * W >= 2**32 or 4 * h * w >= 2**32)
            want = 0 if none else 80 * -(-W // 64) * -(-H // 64) * B * max(C // 3, C % 3)
            assert lib.km_warp2d_bwd_workspace_bytes(B, C, H, W, h, w, interp, pad, dtype) == want, (B, C, H, W, h, w, interp, pad, dtype)


def test_filter_entry_points_host_contract_without_a_gpu():
    """What the filter-family entry points (filter2d, separable, spatial gradient, pyramid, median, bilateral, canny) decide on the host,
    before any launch: every argument check with its message (one defect per call), which message wins when a call has two defects, the
    empty calls that return 0 with null pointers, every "grid too large" that int arguments reach without a launch, and the two
    predicates as closed forms: the LDS budgets in the headers of km_filter.hip / km_filter_sep_big.hip, the window range of km_median.hip."""
    from kornia_amd import _native

    lib = _native.lib()
    raw = ctypes.create_string_buffer(4096 + 32)
    buf = (ctypes.addressof(raw) + 15) & ~15  # 16-byte aligned: the register-tiled paths take it
    odd = buf + 4                               # element-aligned only: the generic paths
    P = dict(constant=0, reflect=1, replicate=2, circular=3)

    def rejected(rc, fragment, who=None):
        msg = lib.km_last_error()
        assert rc < 0 and fragment in msg and (who is None or msg.startswith(who + b":")), (rc, fragment, who, msg)

    # ---- filter2d / filter2d_separable: the shared validation, then each entry point's own checks ----
    def f2d(fn, ptrs=None, B=1, C=3, H=8, W=8, Bk=1, kH=3, kW=3, border=P["reflect"], same=1, dtype=0):
        n_ptr = 4 if "sep" in fn else 3
        ptrs = (buf,) * n_ptr if ptrs is None else ptrs
        return getattr(lib, fn)(*ptrs, B, C, H, W, Bk, kH, kW, border, same, dtype, None)

    for fn in ("km_filter2d_fwd", "km_filter2d_bwd_input", "km_filter2d_bwd_kernel", "km_filter2d_sep_fwd", "km_filter2d_sep_bwd_input"):
        who, nulls = fn.encode(), (None,) * (4 if "sep" in fn else 3)
        rejected(f2d(fn, H=0), b"bad shape B=1 C=3 H=0 W=8", who)
        rejected(f2d(fn, B=-1), b"bad shape B=-1", who)
        rejected(f2d(fn, H=65536, W=32768), b"image plane exceeds 2^31 elements", who)
        rejected(f2d(fn, kH=0), b"bad kernel size 0x3", who)
        rejected(f2d(fn, B=2, Bk=3), b"kernel batch 3 must divide the input batch 2", who)
        rejected(f2d(fn, Bk=0), b"kernel batch 0 must divide", who)
        rejected(f2d(fn, border=4), b"bad border 4", who)
        rejected(f2d(fn, dtype=4), b"bad dtype 4", who)
        rejected(f2d(fn, dtype=-1), b"bad dtype -1", who)
        rejected(f2d(fn, H=2, kH=5), b"reflect padding must be smaller than the image", who)  # pad 2 >= H
        rejected(f2d(fn, W=2, kW=6, border=P["circular"]), b"circular padding must not exceed the image", who)  # rear pad 3 > W
        rejected(f2d(fn, kH=9, same=0), b"'valid' needs kernel <= image", who)
        rejected(f2d(fn, ptrs=nulls), b"null pointer", who)
        for i in range(len(nulls)):
            rejected(f2d(fn, ptrs=tuple(None if j == i else buf for j in range(len(nulls)))), b"null pointer", who)
        # two defects: the checks run in the order above (shape, plane, kernel, batch, border, dtype, pad, pointers)
        rejected(f2d(fn, H=0, kH=0), b"bad shape", who)
        rejected(f2d(fn, border=4, dtype=4), b"bad border 4", who)
        rejected(f2d(fn, ptrs=nulls, dtype=4), b"bad dtype 4", who)
        # empty batch: nothing is looked at
        assert f2d(fn, ptrs=nulls, B=0) == 0 and f2d(fn, ptrs=nulls, C=0) == 0
        assert f2d(fn, ptrs=nulls, B=0, H=0, kH=0, border=9, dtype=9) == 0

    rejected(f2d("km_filter2d_bwd_input", kH=130, border=P["constant"]), b"km_filter2d_bwd_input: kernel too large")  # rear pad 65 >= 64 pre-images
    rejected(f2d("km_filter2d_bwd_input", kW=130, border=P["constant"]), b"km_filter2d_bwd_input: kernel too large")
    rejected(f2d("km_filter2d_bwd_input", ptrs=(None,) * 3, kH=130, border=P["constant"]), b"null pointer")
    rejected(f2d("km_filter2d_bwd_kernel", kH=256, kW=256, border=P["constant"]), b"km_filter2d_bwd_kernel: kernel too large")
    rejected(f2d("km_filter2d_sep_bwd_input", kH=34, border=P["constant"]), b"km_filter2d_sep_bwd_input: kernel larger than the tile; use the generic path")
    rejected(f2d("km_filter2d_sep_bwd_input", kW=66, border=P["constant"]), b"kernel larger than the tile")
    rejected(f2d("km_filter2d_sep_bwd_input", ptrs=(None,) * 4, kH=34, border=P["constant"]), b"null pointer")
    rejected(f2d("km_filter2d_sep_fwd", kH=99, border=P["constant"]), b"km_filter2d_sep: kernel 99x3 needs 68008 B of LDS (> 65536); use the two-pass generic path")
    rejected(f2d("km_filter2d_sep_bwd_input", kH=33, kW=33, border=P["constant"]), b"km_filter2d_sep: kernel 33x33 needs 143624 B of LDS (> 65536)")

    # "grid too large": 2^31 planes of one tile each (B C = 65536 x 32768); the aligned buffer reaches the register-tiled launchers, the
    # element-aligned one, fp64 and the kernel sizes beyond them the generic ones
    big = dict(B=65536, C=32768)
    for ptrs in ((buf,) * 3, (odd,) * 3):
        rejected(f2d("km_filter2d_fwd", ptrs=ptrs, **big), b"km_filter2d: grid too large")
        rejected(f2d("km_filter2d_bwd_input", ptrs=ptrs, **big), b"km_filter2d: grid too large")
    rejected(f2d("km_filter2d_fwd", kH=4, kW=4, **big), b"km_filter2d: grid too large")
    rejected(f2d("km_filter2d_bwd_input", H=4, **big), b"km_filter2d: grid too large")  # H <= 2 pd: no frame pass, the generic adjoint
    rejected(f2d("km_filter2d_bwd_kernel", **big), b"km_filter2d_bwd_kernel: grid too large")
    for fn in ("km_filter2d_sep_fwd", "km_filter2d_sep_bwd_input"):
        rejected(f2d(fn, **big), b"km_blur: grid too large")
        rejected(f2d(fn, ptrs=(odd,) * 4, **big), b"km_filter2d_sep: grid too large")
        rejected(f2d(fn, dtype=1, **big), b"km_filter2d_sep: grid too large")
    rejected(f2d("km_filter2d_sep_fwd", kH=23, kW=23, border=P["constant"], **big), b"km_filter2d_sep: grid too large")  # the big-kernel forward

    # ---- km_filter2d_sep_supported: the LDS budgets of km_filter.hip (64 x 32 tile) and km_filter_sep_big.hip (64 x 64 tile) ----
    def sep_supported(kH, kW, same, dtype):
        elem = 8 if dtype == 1 else 4  # compute type: fp64 for f64 data, fp32 otherwise
        mask = 0
        pitch = (64 + kW - 1 + 8 + 3) // 4 * 4
        if dtype != 1 and (kH >= 10 or kW >= 10) and pitch <= 128 and ((64 + kH - 1) * pitch + (64 + kH - 1) * 64) * 4 <= 65536:
            mask |= 1
        if kH - 1 > 32 or kW - 1 > 64:
            return mask
        IW, IH = 64 + kW - 1, 32 + kH - 1
        if (IH * IW + IH * 64 + kW + kH) * elem <= 65536:
            mask |= 1
        lt = (kH - 1) // 2 if same else 0
        rb = kH - 1 - lt if same else 0
        ll = (kW - 1) // 2 if same else 0
        rr = kW - 1 - ll if same else 0
        EH, UW, EW, VH = 32 + lt + 2 * rb, 64 + (kW - 1) + ll + 2 * rr, 64 + ll + 2 * rr, 32 + (kH - 1) + lt + 2 * rb
        if (VH * UW + EH * UW + 32 * UW + 32 * EW + kW + kH) * elem <= 65536:
            mask |= 2
        return mask

    sizes = (1, 2, 3, 5, 9, 10, 11, 23, 33, 34, 65, 66, 99)
    seen = set()
    for kH in sizes:
        for kW in sizes:
            for same in (0, 1):
                for dtype in range(4):
                    want = sep_supported(kH, kW, same, dtype)
                    assert lib.km_filter2d_sep_supported(kH, kW, same, dtype) == want, (kH, kW, same, dtype, want)
                    seen.add(want)
    assert seen == {0, 1, 3}  # (the adjoint's tile never fits where the forward's does not)

    # ---- spatial gradient ----
    def sg(fn="fwd", x=buf, kern=buf, out=buf, mag=None, B=1, C=3, H=8, W=8, n_out=2, kS=3, dtype=0):
        if fn == "fwd":
            return lib.km_spatial_gradient_fwd(x, kern, out, mag, B, C, H, W, n_out, kS, 0.0, dtype, None)
        return lib.km_spatial_gradient_bwd(x, kern, out, B, C, H, W, n_out, kS, dtype, None)

    for fn in ("fwd", "bwd"):
        who = b"km_spatial_gradient_" + fn.encode()
        rejected(sg(fn, W=0), b"bad shape", who)
        rejected(sg(fn, H=65536, W=32768), b"image plane exceeds 2^31 elements", who)
        rejected(sg(fn, n_out=4), b"n_out must be 1..3, got 4", who)
        rejected(sg(fn, n_out=0), b"n_out must be 1..3, got 0", who)
        rejected(sg(fn, kS=7), b"kernel size must be odd and <= 5, got 7", who)
        rejected(sg(fn, kS=2), b"kernel size must be odd and <= 5, got 2", who)
        rejected(sg(fn, dtype=4), b"bad dtype", who)
        rejected(sg(fn, x=None), b"null pointer", who)
        rejected(sg(fn, kern=None), b"null pointer", who)
        rejected(sg(fn, out=None), b"null pointer", who)
        rejected(sg(fn, W=0, n_out=4), b"bad shape", who)
        rejected(sg(fn, x=None, dtype=4), b"bad dtype", who)
        assert sg(fn, x=None, kern=None, out=None, B=0) == 0 and sg(fn, x=None, kern=None, out=None, C=0, W=0, kS=9) == 0
        for n_out, kS in ((1, 3), (2, 3), (3, 5)):
            rejected(sg(fn, B=65536, C=16384, H=17, n_out=n_out, kS=kS), b"km_spatial_gradient: grid too large")
    rejected(sg(out=None, mag=buf, n_out=3), b"km_spatial_gradient_fwd: magnitude needs n_out == 2")
    rejected(sg(x=None, out=None, mag=buf, n_out=3), b"null pointer")

    # ---- pyramid: pyrdown, bilinear resize and its adjoint ----
    def pyr(fn, x=buf, y=buf, B=1, C=3, H=8, W=8, oh=4, ow=4, border=P["reflect"], align=0, dtype=0):
        if fn == "km_pyrdown_fwd":
            return lib.km_pyrdown_fwd(x, y, B, C, H, W, oh, ow, border, align, dtype, None)
        return getattr(lib, fn)(x, y, B, C, H, W, oh, ow, align, dtype, None)

    for fn in ("km_pyrdown_fwd", "km_resize_bilinear_fwd"):
        who = fn.encode()
        rejected(pyr(fn, H=0), b"bad shape B=1 C=3 H=0 W=8 -> 4x4", who)
        rejected(pyr(fn, oh=-1), b"bad shape", who)
        rejected(pyr(fn, dtype=4), b"unknown dtype code 4", who)
        rejected(pyr(fn, x=None), b"null pointer", who)
        rejected(pyr(fn, y=None), b"null pointer", who)
        rejected(pyr(fn, H=0, dtype=4), b"bad shape", who)
        rejected(pyr(fn, x=None, dtype=4), b"unknown dtype code 4", who)
        for empty in (dict(B=0), dict(C=0), dict(oh=0), dict(ow=0)):
            assert pyr(fn, x=None, y=None, **empty) == 0
        rejected(pyr(fn, x=None, y=None, oh=0, dtype=4), b"unknown dtype code 4", who)  # (an empty output is still validated)
        rejected(pyr(fn, align=1, **big), b"km_pyramid: grid too large")
    rejected(pyr("km_pyrdown_fwd", border=4), b"km_pyrdown_fwd: unknown border code 4")
    rejected(pyr("km_pyrdown_fwd", H=2), b"km_pyrdown_fwd: reflect padding needs H, W > 2 (got 2x8)")
    rejected(pyr("km_pyrdown_fwd", x=None, border=4), b"null pointer")
    rejected(pyr("km_pyrdown_fwd", oh=0, border=4), b"unknown border code 4")
    rejected(pyr("km_pyrdown_fwd", **big), b"km_pyrdown_fwd: grid too large")               # the factor-2 kernel
    rejected(pyr("km_resize_bilinear_fwd", oh=16, ow=16, **big), b"km_resize_bilinear_fwd: grid too large")  # the x2 kernel
    who = b"km_resize_bilinear_bwd"
    rejected(pyr("km_resize_bilinear_bwd", oh=0), b"bad shape B=1 C=3 H=8 W=8 <- 0x4", who)
    rejected(pyr("km_resize_bilinear_bwd", W=0), b"bad shape", who)
    rejected(pyr("km_resize_bilinear_bwd", dtype=4), b"unknown dtype code 4", who)
    rejected(pyr("km_resize_bilinear_bwd", x=None), b"null pointer", who)
    rejected(pyr("km_resize_bilinear_bwd", y=None), b"null pointer", who)
    rejected(pyr("km_resize_bilinear_bwd", W=0, dtype=4), b"bad shape", who)
    assert pyr("km_resize_bilinear_bwd", x=None, y=None, B=0) == 0 and pyr("km_resize_bilinear_bwd", x=None, y=None, C=0) == 0
    rejected(pyr("km_resize_bilinear_bwd", B=1, C=1, H=1 << 20, W=1 << 20), b"km_resize_bilinear_bwd: grid too large")  # block rows
    rejected(pyr("km_resize_bilinear_bwd", B=65536, C=65536), b"km_resize_bilinear_bwd: grid too large")              # planes

    # ---- median ----
    def med(fn="fwd", ptrs=None, B=1, C=3, H=8, W=8, ky=3, kx=3, dtype=0):
        if fn == "fwd":
            x, y, idx, apply = (buf, buf, buf, None) if ptrs is None else ptrs
            return lib.km_median_blur_fwd(x, y, idx, apply, B, C, H, W, ky, kx, dtype, None)
        gy, idx, apply, gx = (buf, buf, None, buf) if ptrs is None else ptrs
        return lib.km_median_blur_bwd(gy, idx, apply, gx, B, C, H, W, ky, kx, dtype, None)

    for fn in ("fwd", "bwd"):
        who = b"km_median_blur_" + fn.encode()
        rejected(med(fn, ky=4), b"the window must have odd sides of 1 .. 15, got (4, 3)", who)
        rejected(med(fn, kx=17), b"the window must have odd sides of 1 .. 15, got (3, 17)", who)
        rejected(med(fn, ky=0), b"the window must have odd sides", who)
        rejected(med(fn, dtype=4), b"bad dtype 4", who)
        rejected(med(fn, B=-1), b"bad shape B=-1 C=3 H=8 W=8", who)
        rejected(med(fn, H=65536, W=32768), b"bad shape", who)
        rejected(med(fn, ptrs=(None,) * 4), b"null pointer", who)
        rejected(med(fn, ky=4, dtype=4), b"the window must have odd sides", who)
        rejected(med(fn, B=-1, dtype=4), b"bad dtype 4", who)
        for empty in (dict(B=0), dict(C=0), dict(H=0), dict(W=0)):
            assert med(fn, ptrs=(None,) * 4, **empty) == 0
        rejected(med(fn, ptrs=(None,) * 4, H=0, ky=4), b"the window must have odd sides", who)
    rejected(med(ptrs=(None, buf, buf, None)), b"null pointer")
    rejected(med(ptrs=(buf, None, buf, None)), b"null pointer")
    rejected(med("bwd", ptrs=(None, buf, None, buf)), b"null pointer")
    rejected(med("bwd", ptrs=(buf, None, None, buf)), b"null pointer")
    rejected(med("bwd", ptrs=(buf, buf, None, None)), b"null pointer")
    rejected(med(**big), b"km_median_blur_fwd: grid too large")                                   # register-tiled 3 x 3
    rejected(med(ptrs=(odd, odd, odd, None), **big), b"km_median_blur_fwd: grid too large")       # generic
    rejected(med(ky=7, kx=7, **big), b"km_median_blur_fwd: grid too large")
    rejected(med("bwd", H=16, W=16, **big), b"km_median_blur_bwd: grid too large")                # 2^39 pixels, 256 per block
    for ky in range(-1, 19):
        for kx in range(-1, 19):
            for dtype in range(-1, 6):
                want = 1 if (1 <= ky <= 15 and 1 <= kx <= 15 and ky % 2 == 1 and kx % 2 == 1 and 0 <= dtype <= 3) else 0
                assert lib.km_median_blur_supported(ky, kx, dtype) == want, (ky, kx, dtype)

    # ---- bilateral ----
    def bil(fn="fwd", ptrs=None, guide=None, B=1, C=3, Cg=0, H=8, W=8, Bs=1, Bc=1, ky=3, kx=3, border=P["reflect"], dist=0, dtype=0):
        if fn == "fwd":
            x, space, coef, y, wsum = (buf, buf, buf, buf, buf) if ptrs is None else ptrs
            return lib.km_bilateral_blur_fwd(x, guide, space, coef, y, wsum, B, C, Cg, H, W, Bs, Bc, ky, kx, border, dist, dtype, None)
        x, space, coef, y, wsum, gy, gx, gg = (buf, buf, buf, buf, buf, buf, buf, None) if ptrs is None else ptrs
        return lib.km_bilateral_blur_bwd(x, guide, space, coef, y, wsum, gy, gx, gg, B, C, Cg, H, W, Bs, Bc, ky, kx, border, dist, dtype, None)

    for fn, n_ptr in (("fwd", 5), ("bwd", 8)):
        who = b"km_bilateral_blur_" + fn.encode()
        rejected(bil(fn, ky=4), b"the window must have odd sides of 1 .. 15, got (4, 3)", who)
        rejected(bil(fn, kx=17), b"the window must have odd sides of 1 .. 15, got (3, 17)", who)
        rejected(bil(fn, dtype=4), b"bad dtype 4", who)
        rejected(bil(fn, border=4), b"bad border code 4", who)
        rejected(bil(fn, dist=2), b"bad distance code 2", who)
        rejected(bil(fn, H=-1), b"bad shape B=1 C=3 H=-1 W=8", who)
        rejected(bil(fn, H=65536, W=32768), b"bad shape", who)
        rejected(bil(fn, C=17), b"at most 16 channels of input and of guidance, got 17 and 17", who)
        rejected(bil(fn, guide=buf, Cg=0), b"at most 16 channels of input and of guidance, got 3 and 0", who)
        rejected(bil(fn, guide=buf, Cg=17), b"at most 16 channels of input and of guidance, got 3 and 17", who)
        rejected(bil(fn, B=4, Bs=2), b"space has 2 and coef 1 samples, each must be 1 or B=4", who)
        rejected(bil(fn, B=4, Bc=3), b"space has 1 and coef 3 samples, each must be 1 or B=4", who)
        rejected(bil(fn, H=2, ky=5), b"a reflect pad of (2, 1) does not fit the 2 x 8 image", who)
        rejected(bil(fn, W=2, kx=7, border=P["circular"]), b"a circular pad of (1, 3) wraps the 8 x 2 image more than once", who)
        rejected(bil(fn, ptrs=(None,) * n_ptr), b"null pointer", who)
        rejected(bil(fn, ky=4, dtype=4), b"the window must have odd sides", who)
        rejected(bil(fn, ptrs=(None,) * n_ptr, H=2, ky=5), b"a reflect pad", who)
        for empty in (dict(B=0), dict(C=0), dict(H=0), dict(W=0)):
            assert bil(fn, ptrs=(None,) * n_ptr, **empty) == 0
        rejected(bil(fn, ptrs=(None,) * n_ptr, H=0, dist=2), b"bad distance code 2", who)  # (an empty call is still validated)
        assert bil(fn, ptrs=(None,) * n_ptr, H=0, ky=5) == 0                                # ... but its pad is not
        rejected(bil(fn, B=1 << 30, C=1, H=9), b"km_bilateral_blur_" + fn.encode() + b": grid too large")  # two 32 x 8 tiles a sample
    for i in (0, 1, 2, 3):  # x, space, coef, y; wsum is optional in the forward
        rejected(bil(ptrs=tuple(None if j == i else buf for j in range(5))), b"null pointer")
    for i in (0, 1, 2, 3, 4, 5):
        rejected(bil("bwd", ptrs=tuple(None if j == i else (None if j == 7 else buf) for j in range(8))), b"null pointer")
    rejected(bil("bwd", ptrs=(buf,) * 6 + (None, None)), b"km_bilateral_blur_bwd: self-guided takes gx alone, joint at least one of gx and gguide")
    rejected(bil("bwd", ptrs=(buf,) * 8), b"self-guided takes gx alone")
    rejected(bil("bwd", guide=buf, Cg=1, ptrs=(buf,) * 6 + (None, None)), b"joint at least one of gx and gguide")
    rejected(bil(B=1 << 30, C=16, H=9, ky=15, kx=15, dtype=1), b"km_bilateral_blur_fwd: grid too large")  # the run-time forward, its tile shrunk

    # ---- canny ----
    def nms(ptrs=(buf, buf, buf), B=1, H=8, W=8):
        return lib.km_canny_nms_fwd(*ptrs, B, H, W, 0.1, 0.2, 1e-6, None)

    def hyst(ptrs=(buf, buf, buf), B=1, H=8, W=8):
        return lib.km_canny_hysteresis_sweep(*ptrs, B, H, W, None)

    for call, who in ((nms, b"km_canny_nms_fwd"), (hyst, b"km_canny_hysteresis_sweep")):
        for i in range(3):
            rejected(call(ptrs=tuple(None if j == i else buf for j in range(3))), b"null pointer", who)
        rejected(call(B=-1), b"bad shape", who)
        rejected(call(H=-1), b"bad shape", who)
        rejected(call(ptrs=(None,) * 3, W=-1), b"null pointer", who)
        for empty in (dict(B=0), dict(H=0), dict(W=0)):
            assert call(ptrs=(None,) * 3, **empty) == 0
        assert call(ptrs=(None,) * 3, B=0, H=-1) == 0
    rejected(nms(B=2, H=1 << 20, W=1 << 20), b"km_canny_nms_fwd: grid too large")              # 64 x 16 tiles
    rejected(hyst(B=2, H=1 << 21, W=1 << 21), b"km_canny_hysteresis_sweep: grid too large")  # 64 x 64 tiles


def test_launch_contract():
    """_native.launch(name, device, *args): the entry point gets (*args, stream_ptr(device)) under exactly one device_guard(device); 0 returns
    None without asking for the error text, anything else raises NativeLibraryError with the name, the code and km_last_error().  `lib`,
    `stream_ptr` and `device_guard` are replaced AFTER import, as tests/emu/mode.py and tests/guarded_alloc.py do."""
    from kornia_amd import _native as N

    events = []

    class Guard:
        def __init__(self, device):
            self.device = device

        def __enter__(self):
            events.append(("enter", self.device))

        def __exit__(self, *exc):
            events.append(("exit", self.device))
            return False

    class Lib:  # (hands the entry points out through __getattr__, like the recorder of tests/guarded_alloc.py)
        rc = 0

        def __getattr__(self, name):
            if name == "km_last_error":
                return lambda: events.append(("last_error",)) or b"fake: bad shape"
            return lambda *args: events.append((name, args)) or self.rc

    lib, dev = Lib(), torch.device("cuda", 3)
    saved = N.lib, N.stream_ptr, N.device_guard
    N.lib, N.stream_ptr, N.device_guard = (lambda: lib), (lambda device: ("stream of", device)), Guard
    try:
        assert N.launch("km_fake_fwd", dev, 1, None, 2.5) is None
        assert events == [("enter", dev), ("km_fake_fwd", (1, None, 2.5, ("stream of", dev))), ("exit", dev)]
        del events[:]
        lib.rc = -7
        with pytest.raises(N.NativeLibraryError) as err:
            N.launch("km_fake_bwd", dev)
        assert all(part in str(err.value) for part in ("km_fake_bwd", "rc=-7", "fake: bad shape"))
        assert events == [("enter", dev), ("km_fake_bwd", (("stream of", dev),)), ("exit", dev), ("last_error",)]
        try:
            N.check(-7, "km_fake_bwd")
        except N.NativeLibraryError as same:
            assert str(same) == str(err.value)  # exactly what check(rc, name) raises
    finally:
        N.lib, N.stream_ptr, N.device_guard = saved


def test_patch_installs_the_hook_table_and_unpatch_restores_it():
    """patch() = the rebound module attributes + the eleven method hooks, each reachable as before; unpatch() puts every original object back."""
    import sys
    import types

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_shim

    if not ref_shim.reference_available():
        pytest.skip("reference tree not present (GPU box)")
    ref_shim.import_reference()
    import importlib

    import kornia_amd.kornia_patch as P

    geometric = "kornia.augmentation._2d.geometric."
    hooked = [("kornia.augmentation._2d.intensity.color_jitter", "ColorJitter", "apply_transform"),
              ("kornia.geometry.transform.image_registrator", "ImageRegistrator", "get_single_level_loss"),
              ("kornia.augmentation.base", "_AugmentationBase", "transform_inputs"),
              ("kornia.augmentation.base", "_AugmentationBase", "_blend_by_prob"),
              ("kornia.augmentation._2d.intensity.gaussian_blur", "RandomGaussianBlur", "apply_transform"),
              (geometric + "affine", "RandomAffine", "compute_transformation"),
              (geometric + "affine", "RandomAffine", "apply_transform"),
              (geometric + "perspective", "RandomPerspective", "apply_transform"),
              (geometric + "shear", "RandomShear", "apply_transform"),
              (geometric + "translate", "RandomTranslate", "apply_transform"),
              (geometric + "rotation", "RandomRotation", "apply_transform")]
    classes = [(getattr(importlib.import_module(m), c), a) for m, c, a in hooked]

    def kornia_modules():
        return [mod for name, mod in list(sys.modules.items()) if mod is not None and (name == "kornia" or name.startswith("kornia."))]

    def raw(cls, attr):  # (the object in the class's own namespace where it has one: a staticmethod stays a staticmethod)
        return cls.__dict__[attr] if attr in cls.__dict__ else getattr(cls, attr)

    assert not P.is_patched()
    originals = [raw(cls, attr) for cls, attr in classes]
    for mod_name, table in P._NATIVE.items():  # (patch() imports them before it scans)
        importlib.import_module(mod_name)
    targets = {id(getattr(sys.modules[m], name)): getattr(sys.modules[m], name) for m, table in P._NATIVE.items() for name in table}
    rebound = sum(1 for mod in kornia_modules() for value in list(vars(mod).values()) if id(value) in targets and targets[id(value)] is value)
    for _ in range(2):
        n = P.patch()
        try:
            assert n == rebound + 11
            assert [(cls, attr) for cls, attr, _ in P._patched_methods] == classes
            for (cls, attr), original in zip(classes, originals):
                assert raw(cls, attr) is not original
                inner = original.__func__ if isinstance(original, staticmethod) else original
                assert getattr(cls, attr).__wrapped__ is inner, (cls, attr)
            assert isinstance(classes[3][0].__dict__["_blend_by_prob"], staticmethod)
            dispatchers = [value for mod in kornia_modules() for value in vars(mod).values()
                           if isinstance(value, types.FunctionType) and hasattr(value, "__kornia_amd_native__")]  # (functions only: no lazy module is touched)
            assert len(dispatchers) == rebound
            natives = {id(f) for table in P._NATIVE.values() for f in table.values()}
            assert all(id(d.__wrapped__) in targets and id(d.__kornia_amd_native__) in natives for d in dispatchers)
        finally:
            assert P.unpatch() == n
        assert not P.is_patched() and not P._patched_methods
        assert all(raw(cls, attr) is original for (cls, attr), original in zip(classes, originals))
        assert all(getattr(sys.modules[m], name) is targets[id(getattr(sys.modules[m], name))] for m, table in P._NATIVE.items() for name in table)


def test_no_cpu_fallback():
    import kornia_amd as K

    x = torch.rand(1, 3, 8, 8)
    with pytest.raises(K.NativeLibraryError, match="no CPU fallback"):
        K.warp_perspective(x, torch.eye(3)[None], (8, 8))
    with pytest.raises(K.NativeLibraryError):
        K.gaussian_blur2d(x, (3, 3), (1.0, 1.0))
    with pytest.raises(K.NativeLibraryError):
        K.spatial_gradient(x)
    with pytest.raises(K.NativeLibraryError):
        K.transform_points(torch.eye(3)[None], torch.rand(1, 4, 2))
    with pytest.raises(K.NativeLibraryError):
        K.remap(x, torch.zeros(1, 8, 8), torch.zeros(1, 8, 8))
    with pytest.raises(K.NativeLibraryError):
        K.grid_sample(x, torch.zeros(1, 4, 4, 2))
    with pytest.raises(K.NativeLibraryError):
        K.enhance.color_jitter(x, 1.1, 0.9, 1.2, 0.05)
    with pytest.raises(K.NativeLibraryError):
        K.enhance.adjust_hue(x, 0.3)


def test_host_side_argument_checks_of_the_next_rows():
    """remap / grid_sample / colour ops validate on the host before touching the library; the matrix builders are plain
    tensor expressions off-device (and differentiable)."""
    import kornia_amd as K
    from kornia_amd.core.exceptions import ShapeError

    x = torch.rand(2, 3, 8, 8)
    with pytest.raises(ShapeError):
        K.remap(x, torch.zeros(8, 8), torch.zeros(2, 8, 8))
    with pytest.raises(ValueError, match="pixel_coordinates must be of shape"):
        K.geometry.normalize_pixel_coordinates(torch.zeros(4, 3), 8, 8)
    n = K.geometry.normalize_pixel_coordinates(torch.tensor([[0.0, 0.0], [7.0, 7.0]]), 8, 8)
    assert torch.allclose(n, torch.tensor([[-1.0, -1.0], [1.0, 1.0]]))
    t = torch.zeros(2, 2, requires_grad=True)
    M = K.get_affine_matrix2d(t, torch.full((2, 2), 3.5), torch.ones(2, 2), torch.tensor([10.0, -20.0]))
    assert M.shape == (2, 3, 3) and M.requires_grad
    M.sum().backward()
    assert t.grad is not None and torch.allclose(t.grad, torch.ones(2, 2))
    Hm = K.get_perspective_transform(torch.tensor([[[0.0, 0], [1, 0], [1, 1], [0, 1]]]), torch.tensor([[[0.0, 0], [2, 0], [2, 2], [0, 2]]]))
    assert torch.allclose(Hm, torch.diag(torch.tensor([2.0, 2.0, 1.0]))[None], atol=1e-6)


def test_validation_matches_reference_conventions():
    """Error types / message fragments pinned by the reference's tests: tests/geometry/transform/
    test_imgwarp.py:232-249, tests/filters/test_filters.py:104-133, tests/filters/test_gaussian.py:356-390."""
    import kornia_amd as K
    from kornia_amd.core import BaseError, ShapeError, TypeCheckError

    x = torch.rand(1, 3, 8, 8)
    with pytest.raises(TypeError, match="Input src type is not a torch.Tensor"):
        K.warp_perspective(1, torch.eye(3)[None], (4, 4))
    with pytest.raises(TypeError, match="Input M type is not a torch.Tensor"):
        K.warp_affine(x, 1, (4, 4))
    with pytest.raises(ValueError, match="BxCxHxW"):
        K.warp_perspective(x[0], torch.eye(3)[None], (4, 4))
    with pytest.raises(ValueError, match="Bx3x3"):
        K.warp_perspective(x, torch.eye(2, 3)[None], (4, 4))
    with pytest.raises(ValueError):
        K.warp_affine(x, torch.eye(3)[None], (4, 4))
    with pytest.raises(ValueError, match="Padding_tensor only supported for 3 channels"):
        K.warp_perspective(x, torch.eye(3)[None], (4, 4), padding_mode="fill", fill_value=torch.zeros(2))
    with pytest.raises(TypeCheckError):
        K.filter2d(1, torch.ones(1, 3, 3))
    with pytest.raises(ShapeError):
        K.filter2d(x[0], torch.ones(1, 3, 3))
    with pytest.raises(ShapeError):
        K.filter2d(x, torch.ones(3, 3))
    with pytest.raises(BaseError, match="Invalid border, a. Ex"):
        K.filter2d(x, torch.ones(1, 3, 3), border_type="a")
    with pytest.raises(BaseError, match="Invalid padding mode, a. Ex"):
        K.filter2d(x, torch.ones(1, 3, 3), padding="a")
    with pytest.raises(BaseError, match="sigma must be positive"):
        K.gaussian_blur2d(x, (3, 3), (0.0, 1.0))
    with pytest.raises(BaseError, match="Kernel size must be"):
        K.gaussian_blur2d(x, (4, 3), (1.0, 1.0))
    with pytest.raises(ShapeError):
        K.gaussian_blur2d(x, (3, 3), torch.ones(1, 3))
    with pytest.raises(ValueError, match="batch size must be the same"):
        K.transform_points(torch.eye(3)[None].expand(2, 3, 3), torch.rand(3, 4, 2))
    with pytest.raises(TypeError, match="same device"):
        K.homography_warp(x, torch.eye(3, device="meta")[None], (4, 4))


def test_check_switch_and_kernel_builders():
    from kornia_amd.core import KORNIA_CHECK, are_checks_enabled, disable_checks, enable_checks
    from kornia_amd.core.exceptions import BaseError
    from kornia_amd.filters import get_gaussian_kernel1d, get_gaussian_kernel2d, get_spatial_gradient_kernel2d, normalize_kernel2d

    assert are_checks_enabled()
    with pytest.raises(BaseError):
        KORNIA_CHECK(False, "boom")
    disable_checks()
    try:
        assert KORNIA_CHECK(False, "boom") is True
    finally:
        enable_checks()
    k = get_gaussian_kernel1d(5, 1.5)
    assert torch.allclose(k, torch.tensor([[0.1201, 0.2339, 0.2921, 0.2339, 0.1201]]), atol=1e-4)
    k2 = get_gaussian_kernel2d((3, 5), (1.0, 2.0))
    assert k2.shape == (1, 3, 5) and abs(k2.sum().item() - 1.0) < 1e-6
    s = get_spatial_gradient_kernel2d("sobel", 1)
    assert s.shape == (2, 3, 3) and torch.equal(s[1], s[0].t())
    assert torch.allclose(normalize_kernel2d(s).abs().sum((-1, -2)), torch.ones(2))
    assert get_spatial_gradient_kernel2d("diff", 2).shape == (3, 3, 3)
    assert get_spatial_gradient_kernel2d("sobel", 2).shape == (3, 5, 5)


def test_host_side_conventions():
    from kornia_amd.filters.filter import _compute_padding
    from kornia_amd.geometry import convert_affinematrix_to_homography, create_meshgrid, normal_transform_pixel

    assert _compute_padding([5, 6]) == [2, 3, 2, 2]  # width pair first; even kernels pad (k-1)//2 in front
    assert _compute_padding([2, 2]) == [0, 1, 0, 1]
    n = normal_transform_pixel(3, 5)
    assert torch.allclose(n, torch.tensor([[[0.5, 0.0, -1.0], [0.0, 1.0, -1.0], [0.0, 0.0, 1.0]]]))
    h = convert_affinematrix_to_homography(torch.eye(2, 3)[None])
    assert torch.equal(h, torch.eye(3)[None])
    g = create_meshgrid(2, 3)
    assert g.shape == (1, 2, 3, 2) and torch.equal(g[0, 0, :, 0], torch.tensor([-1.0, 0.0, 1.0]))


def test_product_never_references_the_checkers():
    """oracle/ and tests/emu/ are test infrastructure: no file of the package (Python or HIP) may import, load or even
    name them, and the library the package loads is the hipcc build."""
    import kornia_amd
    from kornia_amd import _native

    pkg = os.path.dirname(os.path.abspath(kornia_amd.__file__))
    offenders = []
    for base, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(base, f), errors="replace").read()
                if re.search(r"\b(import oracle|from oracle|emu_lib|build_emu|emulated_device|libkornia_amd_emu|oracle\.oracle|oracle/_)", text):
                    offenders.append(os.path.join(base, f))
    assert not offenders, offenders
    assert _native.library_path().endswith(os.path.join("kornia_amd", "lib", "libkornia_amd.so")) or os.environ.get("KORNIA_AMD_LIB")


def test_streaming_store_helper_keeps_the_non_temporal_mark(tmp_path):
    """km_st_c<STREAM> (csrc/km_common.h) must compile to `global_store_dword ... nt` for STREAM = true and to a plain store for false, in the
    shape the forward uses it (restrict plane pointers + 32-bit offsets, rows and channels unrolled).  Round 2's bool-argument form compiled to
    plain stores in EVERY instantiation - its if / else was merged before the constant arrived and the merge dropped the mark - and nobody
    noticed for a round: this reads the ISA (hipcc cross-compiles without a GPU)."""
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    csrc = os.path.join(ROOT, "kornia_amd", "csrc")
    src = tmp_path / "nt_probe.hip"
    src.write_text('''
#include "km_common.h"
template <bool STREAM>
__global__ void probe(float* p, const float* __restrict__ q, uint32_t w, size_t plane) {
    float* __restrict__ dp[3];
    for (int c = 0; c < 3; ++c) dp[c] = p + c * plane;
    const uint32_t off = blockIdx.x * 256 + threadIdx.x;
    const float v = q[off];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) km_st_c<STREAM>(km_at_mut(dp[c], off + r * w), v + r + c);
}
template __global__ void probe<true>(float*, const float*, uint32_t, size_t);
template __global__ void probe<false>(float*, const float*, uint32_t, size_t);
''')
    out = tmp_path / "nt_probe.s"
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", f"-I{csrc}", str(src), "-o", str(out)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    kernels, cur = {}, None
    for line in out.read_text().splitlines():
        if line.startswith("_Z5probeILb"):
            cur = "stream" if "ILb1E" in line else "plain"
            kernels[cur] = []
        elif cur and "global_store_dword" in line:
            kernels[cur].append(line.strip())
        elif ".end_amdhsa_kernel" in line:
            cur = None
    assert len(kernels["stream"]) == 12 and all(s.endswith(" nt") for s in kernels["stream"]), kernels["stream"]
    assert len(kernels["plain"]) == 12 and not any(" nt" in s for s in kernels["plain"]), kernels["plain"]
