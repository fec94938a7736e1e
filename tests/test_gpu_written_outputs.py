"""GPU (and, through tests/test_emulated_written_outputs.py, the host build of the kernels): every native launch writes all of its output,
nothing outside it, and reads nothing it has not initialised.

tests/guarded_alloc.py hands the package poisoned buffers between guard bands.  Two layers run under it:

  * the existing parity tests, unchanged (re-exported below as tests/test_emulated_kernels.py re-exports them): their assertions compare with
    the oracle and the reference's fixtures, so a hole or a poisoned accumulator now fails them instead of holding the previous call's value;
  * a table of one case per writing entry point (CASES), at the smallest shapes that reach the tails, each run under the fills 0xFF and 0x7B:
    the two runs must agree bit for bit - in every dtype, integer masks included, where no single sentinel is safe - the inputs must come
    back unchanged, and the results are compared with the oracle by the bound the op's own test uses.

`test_every_writing_entry_point_has_a_guarded_case` keeps the table complete: a new `km_*` symbol without a case fails it."""
import importlib
import itertools
import math

import pytest
import torch

from guarded_alloc import current, guarded, same_bits, unchanged

pytestmark = pytest.mark.gpu

MODULES = ("test_gpu_golden test_gpu_warp test_gpu_warp_fused test_gpu_warp_gm_box test_gpu_warp_blur test_gpu_warp_bwd_slots test_gpu_filters "
           "test_gpu_grid_sample test_gpu_color test_gpu_pyramid test_gpu_median test_gpu_aug_modules test_gpu_aug_crop test_gpu_aug_masks "
           "test_gpu_augmentation test_gpu_edge_cases test_zz_gpu_registration test_zz_gpu_canny").split()
# left out, each for one reason
SKIP = {
    ("test_gpu_edge_cases", "test_mixed_dtypes_and_streams"): "HIP streams: about the device, not about what a launch writes (the host build skips it too)",
    ("test_gpu_edge_cases", "test_two_threads_two_streams_share_no_launch_state"): "HIP streams and host threads: the patched allocation calls are process-wide",
}

for _m in MODULES:
    _mod = importlib.import_module(_m)
    for _name in dir(_mod):
        if _name.endswith("_at_full_size"):  # BASELINE-size property tests: seconds each on the device, minutes on the host build
            continue
        if _name.startswith("test_") and callable(getattr(_mod, _name)) and (_m, _name) not in SKIP:
            globals()[f"{_name}__{_m.replace('test_zz_gpu_', 'zz_').replace('test_gpu_', '')}"] = getattr(_mod, _name)


def guard_fixture(request):
    """every test of this module under the guard (fill 0xFF); the table's tests enter it themselves, once per fill"""
    if request.node.name.startswith(("test_table", "test_every_writing", "test_the_guard")):
        yield
        return
    with guarded(0xFF):
        yield


@pytest.fixture(autouse=True)
def _guarded(request):
    yield from guard_fixture(request)


# =====================================================================================================================================
# the case table: one case per writing entry point.  A case takes the oracle, runs under whatever guard is active, holds its inputs in
# `unchanged(...)`, asserts against the oracle with the bound of the op's own test, and returns {name: tensor} - what the two fills
# must agree on bit for bit.  Two kinds of result are sums whose order the hardware is free to choose, so that two runs of one launch on
# the SAME memory differ in the last bits; they are named and bounded apart:
#   "acc_": sums of fp64 atomics (matrix, tap and factor gradients, the masked loss): 1e-6 relative to the largest entry
#           (tests/test_gpu_edge_cases.py::test_batch_traversal_direction_does_not_change_results);
#   "atm_": image gradients that the kernel ACCUMULATES into a buffer the package zeroes for it (`km_warp2d_bwd_needs_zero_init()` without a
#           workspace, `km_grid_sample2d_bwd`: global fp32 atomics, include/kornia_amd.h) - read off the guard's own record of how the package
#           allocated the gradient, not restated here.  Where it is `empty` the tile owners write every pixel once and the bits must agree.
#           Seen on the MI355X (five runs of every such case, three under one fill): fp32 storage differs from run to run under ONE fill
#           through the generic scatter, border / reflection without a workspace, bicubic and grid_sample (f16 grid_sample once); 16-bit
#           storage and nearest came out equal in those runs (the cast hides the last fp32 bits; two addends commute) but sum the same way,
#           so they keep the bound; border / reflection with a workspace (the fused tile owners) is `empty`, equal, and held to equal bits.
#           Bound: 1 ulp of the storage dtype plus 2e-5 of the largest entry, the order term of tests/test_gpu_half_grads.py::_check_warp.
#           A hole or a value read before it was written is the fill - NaN under 0xFF, 1.3e36 (61 280 in f16) under 0x7B - far outside it.
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DT_NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
ACC_REL = 1e-6
CASES = {}
FILLS = (0xFF, 0x7B)


def case(name):
    def deco(fn):
        assert name not in CASES, name
        CASES[name] = fn
        return fn
    return deco


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _lib():
    from kornia_amd import _native as N

    return N.lib()


def _stream():
    from kornia_amd import _native as N

    return N.stream_ptr(torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cuda"))


def _raw(guard_site, shape, dtype, zero=False):
    """a guarded buffer for a case that calls the C ABI itself (the entry points the Python layer does not use)"""
    from guarded_alloc import current

    return current().alloc(shape, dtype, "cuda", zero, guard_site)


# ---- warps ----------------------------------------------------------------------------------------------------------------------------
from test_gpu_half_grads import (FLOAT_TILE_MULT, POLICIES, _check_warp, _matrices, _oracle_bwd, _output_pixels_per_source_pixel, _rel, _ulp,  # noqa: E402
                                 _warp_op, _with_config, _within_ulps)

WARP_SHAPES = [(70, 93, 37, 53), (70, 93, 66, 68), (64, 128, 64, 64)]  # H, W, h, w: ragged owner tiles and box regions, W % 4 != 0; the 16-byte paths
WARP_PADS = ["zeros", "border", "reflection", "fill"]


def _oracle_fwd(oracle, fn, x, M, dsize, mode, pad, align, fill):
    if fn == "persp":
        return oracle.warp_perspective(x, M, dsize, mode, pad, align, fill)
    if fn == "affine":
        return oracle.warp_affine(x, M, dsize, mode, pad, align, fill)
    return oracle.homography_warp(x, M, dsize, mode, pad, align)


def _corner_matrix(fn, B):
    """a scale about the top-left corner that keeps the samples inside the first 40 % of the source: the owner tiles right of and below it
    are never visited"""
    if fn == "homog":  # dst -> src, normalised: x_src = -1 + 0.4 (x_dst + 1)
        M = torch.tensor([[0.4, 0.0, -0.6], [0.0, 0.4, -0.6], [0.0, 0.0, 1.0]])
    else:              # src -> dst, pixels
        M = torch.tensor([[2.5, 0.0, 0.0], [0.0, 2.5, 0.0], [0.0, 0.0, 1.0]])
    M = M.repeat(B, 1, 1)
    return M[:, :2, :].contiguous() if fn == "affine" else M


def _warp_case(oracle, fn, dt, C, shape, pad, policy, need, mode="bilinear", shared=False, corner=False, align=True, seed=0):
    H, W, h, w = shape
    B = 2
    g = _gen(1000 + seed)
    x = torch.rand(B, C, H, W, generator=g).to(dt)
    go = (torch.rand(B, C, h, w, generator=g) - 0.4).to(dt)
    M = _corner_matrix(fn, 1 if shared else B) if corner else _matrices(fn, B, H, W, h, w, g, shared=shared)
    fill = (torch.tensor([0.2, 0.5, 0.7, 0.4])[:C] if pad == "fill" else None)
    cfg = POLICIES[policy]
    op = _warp_op(fn, (h, w), mode, pad, align, fill)
    xd, Md, god = x.cuda(), M.cuda(), go.cuda()
    res = {}
    # a map so dense that its tiles accumulate in float LDS atomics, in the order the waves come (test_gpu_half_grads.py, FLOAT_TILE_MULT)
    dense = _output_pixels_per_source_pixel(fn, M, H, W, h, w) > FLOAT_TILE_MULT
    # the deterministic owner paths of test_gpu_half_grads.py, contract 1: which bound against the oracle applies
    owner = mode == "bilinear" and pad in ("zeros", "fill") and not cfg.get("warp_bwd_generic", 0) and not dense

    def run():
        with unchanged(xd, Md, god):
            res["y"] = op(xd, Md).cpu()
            if need:
                xg, Mg = xd.detach().requires_grad_("x" in need), Md.detach().requires_grad_("M" in need)  # (detach: the same storage)
                since = len(current().records)
                op(xg, Mg).backward(god)
                if "x" in need:
                    # (accumulated into a buffer the package zeroed for the kernel, or in the float LDS tiles of a dense map: "atm_")
                    summed = dense or current().zero_initialised("geometry/transform/imgwarp.py", (B, C, H, W), since)
                    res["atm_gx" if summed else "gx"] = xg.grad.cpu()
                if "M" in need:
                    res["acc_gM"] = Mg.grad.cpu()

    _with_config(cfg, run)
    gx_name = "gx" if "gx" in res else "atm_gx"
    Mo = M.expand(B, -1, -1).contiguous() if shared else M
    if dt == F32:
        ref = _oracle_fwd(oracle, fn, x, Mo, (h, w), mode, pad, align, fill)
        # bit-identical, but for the LDS-staged bicubic forward (zeros padding, C in {1, 3}, W % 4 == 0), whose taps are fused multiply-adds:
        # 2e-6 (tests/test_gpu_warp.py::test_bicubic_lds_staged_kernel_is_bit_identical)
        staged = mode == "bicubic" and pad == "zeros" and C in (1, 3) and W % 4 == 0
        d = (res["y"] - ref).abs().max().item()
        assert d <= 2e-6 if staged else torch.equal(res["y"], ref), f"forward differs from the oracle: {d:.3e}"
        if need:
            gxo, gMo = _oracle_bwd(oracle, fn, go, x, Mo, (h, w), mode, pad, align, fill)
            if "x" in need:  # the fp32 sweep's bound (test_gpu_half_grads.py::_check_warp, contract 3, with the spacing of fp32)
                scale = max(1.0, go.abs().max().item()) * max(1.0, 4.0 * h * w / (H * W))
                atol = 2e-5 * scale if owner else 2e-5 * max(scale, gxo.abs().max().item())
                d = (res[gx_name].double() - gxo.double()).abs()
                assert bool((d <= _ulp(gxo, F32) + atol + 1e-5 * gxo.double().abs()).all()), f"grad_x vs the oracle, max |d| {d.max().item():.3e}"
            if "M" in need:
                gMo = gMo.sum(0, keepdim=True) if shared else gMo
                bound = 2e-4 if pad in ("border", "reflection") else 5e-5
                assert _rel(res["acc_gM"], gMo) <= bound, f"grad_M vs the oracle rel {_rel(res['acc_gM'], gMo):.2e}"
    else:
        # the 16-bit forward is the fp32 path's result rounded once (test_gpu_warp.py::test_16_bit_storage_is_the_fp32_result_rounded_once);
        # the gradients: the whole contract of test_gpu_half_grads.py, against the fp32 path and the oracle
        y32 = _with_config(cfg, lambda: op(xd.float(), Md).to(dt).cpu())
        assert same_bits(res["y"], y32), "the 16-bit forward is not the fp32 path's rounded once"
        if need:
            gx, gM = _check_warp(oracle, fn, dt, x, M, go, (h, w), cfg, need=need, mode=mode, pad=pad, align=align, fill=fill, tag="table")
            assert gx is None or gx_name != "gx" or same_bits(gx, res["gx"])
    return res


def _add_warp_cases():
    fns = ["persp", "affine", "homog"]
    needs = [("x",), ("M",), ("x", "M")]
    # every (policy, dtype, need) - so that gsrc, gm and the workspace are each met as `empty` and as `zeros` - with the function, the shape,
    # the channel count, the padding and the shared matrix rotating through the combinations
    for i, (policy, dt, need) in enumerate(itertools.product(POLICIES, (F32, BF16, F16), needs)):
        fn = fns[(i + i // 3) % 3]
        shape = WARP_SHAPES[(i // 2) % 3]
        C = (1, 3, 4)[(i + i // 9) % 3]
        pad = WARP_PADS[(i + i // 4) % 4]
        if pad == "fill" and (fn == "homog" or (fn == "persp" and C != 3)):  # (homography_warp has no fill; warp_perspective's is RGB only)
            pad = "zeros"
        shared = fn == "affine" and i % 2 == 1
        name = f"warp-{fn}-{DT_NAME[dt]}-C{C}-{'x'.join(map(str, shape))}-{pad}-{policy}-{''.join(need)}{'-shared' if shared else ''}"
        CASES[name] = (lambda oracle, a=(fn, dt, C, shape, pad, policy, need), s=shared, i=i: _warp_case(oracle, *a, shared=s, align=bool(i % 2), seed=i))
    # every padding with every function that takes it, forward + both gradients, default policy (fp32), at the ragged shape
    for fn, pad in itertools.product(fns, WARP_PADS):
        if pad == "fill" and fn == "homog":
            continue
        CASES[f"warp-{fn}-f32-C3-70x93x37x53-{pad}-default-xM-pads"] = (lambda oracle, fn=fn, pad=pad: _warp_case(oracle, fn, F32, 3, WARP_SHAPES[0], pad, "default", ("x", "M"), seed=77))
    # bicubic and nearest: forward and the image gradient (the matrix gradient is bilinear-only, as in the reference's grid_sample)
    for mode, dt, fn in itertools.product(("bicubic", "nearest"), (F32, BF16, F16), fns):
        shape = WARP_SHAPES[(fns.index(fn) + (mode == "nearest")) % 3]
        CASES[f"warp-{fn}-{DT_NAME[dt]}-C3-{'x'.join(map(str, shape))}-{mode}"] = (lambda oracle, a=(fn, dt, 3, shape, "zeros", "default", ("x",)), mode=mode: _warp_case(oracle, *a, mode=mode, seed=55))
    # an owner tile nobody visits
    for fn, dt, policy in itertools.product(fns, (F32, BF16, F16), ("default", "tiled")):
        CASES[f"warp-{fn}-{DT_NAME[dt]}-C3-70x93x37x53-corner-{policy}"] = (lambda oracle, a=(fn, dt, 3, WARP_SHAPES[0], "zeros", policy, ("x", "M")): _warp_case(oracle, *a, corner=True, seed=66))


_add_warp_cases()


@case("warp2d_bwd-abi")
def _case_warp2d_bwd_abi(oracle):
    """km_warp2d_bwd (the entry point without a workspace; the Python layer calls km_warp2d_bwd_ws): gsrc as km_warp2d_bwd_needs_zero_init says,
    gmat zeroed, against the public backward under the policy that takes the same kernels"""
    import kornia_amd as K
    from kornia_amd import _native as N

    B, C, H, W, h, w = 2, 3, 70, 93, 37, 53
    g = _gen(5)
    x, go = torch.rand(B, C, H, W, generator=g).cuda(), (torch.rand(B, C, h, w, generator=g) - 0.4).cuda()
    m = _matrices("homog", B, H, W, h, w, g).view(B, 9).contiguous().cuda()  # dst -> src, normalised: what the sampler reads
    zero = bool(_lib().km_warp2d_bwd_needs_zero_init(1, 0, 0))
    gsrc = _raw("km_warp2d_bwd gsrc", (B, C, H, W), F32, zero)
    gm = _raw("km_warp2d_bwd gmat", (B, 9), torch.float64, True)
    with unchanged(x, go, m):
        N.check(_lib().km_warp2d_bwd(go.data_ptr(), x.data_ptr(), m.data_ptr(), gsrc.data_ptr(), gm.data_ptr(), B, C, H, W, h, w, B, 2, 1, 1, 0, 1, None, 0,
                                     _stream()), "km_warp2d_bwd")
    xg, mg = x.detach().requires_grad_(), m.view(B, 3, 3).detach().requires_grad_()
    _with_config(POLICIES["tiled"], lambda: K.homography_warp(xg, mg, (h, w), "bilinear", "zeros", True).backward(go))
    assert torch.allclose(gsrc.cpu(), xg.grad.cpu(), atol=2e-5, rtol=1e-5)
    assert _rel(gm.view(B, 3, 3).cpu(), mg.grad.cpu()) <= 5e-5
    return {"gsrc": gsrc.cpu(), "acc_gm": gm.cpu()}


# ---- the augmentation layer's warps: per-sample switch, image + mask pair, select ----------------------------------------------------------
MASK_DTYPES = (torch.uint8, torch.bool, torch.int64)


def _labels(B, Cm, H, W, mdt, g):
    lab = torch.randint(0, 200, (B, Cm, H, W), generator=g)
    return (lab > 100) if mdt == torch.bool else lab.to(mdt)


@case("warp-fwd_masked-and-chain")
def _case_warp_masked(oracle):
    """km_warp2d_fwd_masked / km_affine_params_chain_fwd / km_perspective_params_chain_fwd / km_perspective_transform_fwd / km_affine_matrix2d_fwd:
    `apply` with zeros and ones mixed - a sample whose draw failed is a copy, the others are the plain warp by the module's own matrix"""
    import kornia_amd as K
    import kornia_amd.augmentation as A

    res = {}
    for B, H, W in ((1, 37, 53), (5, 37, 53), (300, 7, 9)):  # (1: one lane of one block; 300: more samples than one pass of a parameter kernel's block)
        g = _gen(B)
        for dt in (F32, BF16):
            x = torch.rand(B, 3, H, W, generator=g).to(dt).cuda()
            torch.manual_seed(B)
            aff = A.RandomAffine(degrees=30.0, translate=(0.1, 0.2), scale=(0.8, 1.2), shear=8.0, padding_mode="border", p=0.5)
            per = A.RandomPerspective(0.5, p=0.5)
            pa = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in aff.forward_parameters((B, 3, H, W)).items()}
            pp = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in per.forward_parameters((B, 3, H, W)).items()}
            keep_a, keep_p = pa["batch_prob"] > 0.5, pp["batch_prob"] > 0.5
            assert B == 1 or (0 < int(keep_a.sum()) < B and 0 < int(keep_p.sum()) < B)
            with unchanged(x, *[v for v in list(pa.values()) + list(pp.values()) if isinstance(v, torch.Tensor)]):
                ya = A.random_affine(x, pa, padding_mode="border")
                yp = A.random_perspective(x, pp)
                m, Ma, apply = A.affine_chain(pa, "cuda", H, W, with_matrix=True)
                m2, Mp, apply2 = A.perspective_chain(pp, "cuda", H, W, with_matrix=True)
                Mpt = K.get_perspective_transform(pp["start_points"], pp["end_points"])
                Maf = A.affine_matrix(pa, x.device)
            ka, kp = keep_a.view(-1, 1, 1, 1), keep_p.view(-1, 1, 1, 1)
            assert torch.equal(apply.bool(), keep_a) and torch.equal(apply2.bool(), keep_p) and torch.equal(Mp, Mpt)
            assert torch.allclose(Ma, Maf, atol=1e-5, rtol=1e-5)
            assert torch.equal(ya, torch.where(ka, K.warp_affine(x, Ma[:, :2].contiguous(), (H, W), "bilinear", "border", False), x))
            assert torch.equal(yp, torch.where(kp, K.warp_perspective(x, Mp, (H, W), "bilinear", "zeros", False), x))
            res.update({f"{B}{DT_NAME[dt]}{k}": v.cpu() for k, v in dict(ya=ya, yp=yp, m=m, Ma=Ma, ap=apply, m2=m2, Mp=Mp, ap2=apply2, Maf=Maf).items()})
    return res


@case("warp-pair-select-inverse")
def _case_warp_pair(oracle):
    """km_warp2d_pair_fwd / km_select_samples_fwd / km_inverse_chain_fwd: the image as the masked warp returns it, the mask as the nearest warp
    through the image dtype (tests/test_gpu_aug_masks.py), for uint8 / bool / int64 masks, `apply` mixed"""
    import kornia_amd as K
    import kornia_amd.augmentation as A

    B, H, W = 4, 37, 53
    g = _gen(21)
    res = {}
    M = torch.eye(3).repeat(B, 1, 1) + torch.tensor([[0.05, 0.08, 2.0], [-0.06, 0.04, -1.5], [1e-4, -2e-4, 0.0]]) * torch.rand(B, 1, 1, generator=g)
    Md = M.cuda()
    apply = torch.tensor([1, 0, 1, 0], dtype=torch.uint8).cuda()
    keep = apply.bool().view(-1, 1, 1, 1)
    for affine, pad in ((True, "zeros"), (True, "fill"), (False, "zeros"), (False, "reflection")):
        Mw = (torch.cat([Md[:, :2], torch.tensor([[[0.0, 0.0, 1.0]]]).cuda().expand(B, 1, 3)], 1) if affine else Md).contiguous()
        with unchanged(Mw):
            m = A.inverse_chain(torch.linalg.inv(Mw.cpu()).cuda(), H, W, affine)  # the inverse of the inverse: the sampler's matrix for Mw
        res[f"m{affine}"] = m.cpu()
        for dt, mdt in itertools.product((F32, BF16, F16), MASK_DTYPES):
            x = torch.rand(B, 3, H, W, generator=g).to(dt).cuda()
            mk = _labels(B, 2, H, W, mdt, g).cuda()
            with unchanged(x, mk, m, apply):
                out, mout = A.warp_pair(x, mk, m, affine, "bilinear", pad, False, 0.7 if pad == "fill" else None, apply)
                _, mout1 = A.warp_pair(None, mk, m, affine, "bilinear", pad, False, 0.7 if pad == "fill" else None, apply, image_dtype=dt)
                sel = A.select_samples(out, x, keep.view(-1))
            warp = K.warp_affine if affine else K.warp_perspective
            Mr = Mw[:, :2].contiguous() if affine else Mw
            kw = dict(padding_mode=pad, align_corners=False)
            # (the chain went through two inversions of the matrix: the image within the bound of a rebuilt matrix, tests/test_gpu_augmentation.py)
            ref = warp(x, Mr, (H, W), mode="bilinear", fill_value=torch.full((3,), 0.7) if pad == "fill" else None, **kw)
            tol = 2e-5 if dt == F32 else 2 * torch.finfo(dt).eps
            assert torch.equal(out[~apply.bool()], x[~apply.bool()]) and (out.float() - torch.where(keep, ref, x).float()).abs().max().item() <= tol
            assert mout.dtype == mdt and torch.equal(mout, mout1) and torch.equal(mout[~apply.bool()], mk.to(dt).to(mdt)[~apply.bool()])
            assert torch.equal(sel, out)  # (select of the warped pair by its own switch: the untouched samples are x on both sides)
            res.update({f"{affine}{pad}{DT_NAME[dt]}{mdt}out": out.cpu(), f"{affine}{pad}{DT_NAME[dt]}{mdt}mask": mout.cpu(), f"{affine}{pad}{DT_NAME[dt]}{mdt}sel": sel.cpu()})
    return res


@case("inverse_chain")
def _case_inverse_chain(oracle):
    """km_inverse_chain_fwd, rows 2 and 3, at B = 1 and B = 300 (four full blocks of 64 and a ragged one of 44): the closed-form inverse
    (tests/test_gpu_aug_masks.py::_inv3) through km_homography_chain_fwd, bit for bit"""
    import kornia_amd.augmentation as A
    from kornia_amd.geometry.conversions import _ChainFunction
    from test_gpu_aug_masks import _inv3

    H, W = 37, 53
    res = {}
    for B, affine in itertools.product((1, 300), (True, False)):
        g = _gen(7 * B + affine)
        M = torch.eye(3).repeat(B, 1, 1) + torch.tensor([[0.05, 0.08, 2.0], [-0.06, 0.04, -1.5], [0.0, 0.0, 0.0]]) * (torch.rand(B, 1, 1, generator=g) - 0.3)
        if not affine:
            M[:, 2, :2] = (torch.rand(B, 2, generator=g) - 0.5) * 4e-4
        Md = M.cuda()
        with unchanged(Md):
            m = A.inverse_chain(Md, H, W, affine)
        Mi = _inv3(M).cuda()
        ref = _ChainFunction.apply(Mi[:, :2].contiguous() if affine else Mi, (H, W), (H, W), True).reshape(B, 9)
        assert m.shape == (B, 9) and torch.equal(m, ref), (B, affine, (m - ref).abs().max().item())
        res[f"m{B}{affine}"] = m.cpu()
    return res


# ---- explicit grids -----------------------------------------------------------------------------------------------------------------------
def _grid_case(oracle, mode, pad, shared, dt):
    import kornia_amd as K

    B, C, H, W, h, w = 2, 3, 40, 45, 37, 53
    g = _gen(31)
    x = torch.rand(B, C, H, W, generator=g).to(dt)
    grid = (torch.rand(1 if shared else B, h, w, 2, generator=g) * 2.4 - 1.2).to(dt)
    go = (torch.rand(B, C, h, w, generator=g) - 0.4).to(dt)
    xd, gd, god = x.cuda(), grid.cuda(), go.cuda()
    res = {}
    for align in (False, True):
        with unchanged(xd, gd, god):
            xg, gg = xd.detach().requires_grad_(), gd.detach().requires_grad_()
            y = K.grid_sample(xg, gg, mode, pad, align)
            y.backward(god)
            ym = K.remap(xd, gd[..., 0], gd[..., 1], mode, pad, align, normalized_coordinates=True)
        # (gsrc is zeroed by the caller and accumulated by fp32 atomics - include/kornia_amd.h; the grid's gradient is one value per lane)
        res.update({f"y{align}": y.detach().cpu(), f"atm_gx{align}": xg.grad.cpu(), f"gg{align}": gg.grad.cpu(), f"remap{align}": ym.cpu()})
        if dt == F32:  # tests/test_gpu_grid_sample.py::test_grid_sample_vs_oracle
            ge = grid.expand(B, -1, -1, -1).contiguous()
            ref = oracle.grid_sample(x, ge, mode, pad, align)
            assert torch.equal(y.detach().cpu(), ref) if mode != "bicubic" else torch.allclose(y.detach().cpu(), ref, atol=1e-6)
            assert torch.equal(ym.cpu(), y.detach().cpu())
            gx_o, gg_o = oracle.grid_sample_backward(go, x, ge, mode, pad, align)
            assert torch.allclose(xg.grad.cpu(), gx_o, atol=1e-5, rtol=1e-5)
            assert torch.allclose(gg.grad.cpu(), gg_o.sum(0, keepdim=True) if shared else gg_o, atol=1e-4, rtol=1e-4)
        else:      # tests/test_gpu_grid_sample.py::test_half_precision_and_errors
            assert y.dtype == dt and torch.allclose(y.detach().float().cpu(), oracle.grid_sample(x.float(), grid.float().expand(B, -1, -1, -1).contiguous(), mode, pad, align), atol=5e-2)
    return res


for _mode, _pad, _shared, _dt in [("bilinear", "zeros", False, F32), ("bilinear", "border", True, F32), ("bilinear", "reflection", False, F32), ("nearest", "zeros", True, F32),
                                  ("bicubic", "border", False, F32), ("bilinear", "zeros", True, BF16), ("bilinear", "reflection", False, F16)]:
    CASES[f"grid_sample-{_mode}-{_pad}-{'shared' if _shared else 'perbatch'}-{DT_NAME[_dt]}"] = (lambda oracle, a=(_mode, _pad, _shared, _dt): _grid_case(oracle, *a))


# ---- filters ------------------------------------------------------------------------------------------------------------------------------
BORDERS = ["constant", "reflect", "replicate", "circular"]
FILTER_IMAGES = [(2, 3, 37, 53), (2, 3, 40, 64)]


def _filter2d_case(oracle, ks, border, shape, Bk):
    import kornia_amd as K

    g = _gen(41 + ks[0])
    x = torch.rand(*shape, generator=g)
    k = torch.rand(Bk, *ks, generator=g)
    go = torch.rand(*shape, generator=g)
    xd, kd, god = x.cuda(), k.cuda(), go.cuda()
    with unchanged(xd, kd, god):
        y0 = K.filter2d(xd, kd, border)  # (the forward alone: no autograd node)
        xg, kg = xd.detach().requires_grad_(), kd.detach().requires_grad_()
        y = K.filter2d(xg, kg, border)
        y.backward(god)
        xg1 = xd.detach().requires_grad_()
        K.filter2d(xg1, kd, border).backward(god)  # the input adjoint alone
        kg1 = kd.detach().requires_grad_()
        K.filter2d(xd, kg1, border).backward(god)  # the tap gradient alone
    assert torch.equal(y0.cpu(), oracle.filter2d(x, k, border)) and torch.equal(y0, y.detach())
    gx_o, gk_o = oracle.filter2d_backward(go, x, k, border)
    small = ks in ((3, 3), (5, 5), (7, 7))  # tests/test_gpu_filters.py::test_register_tiled_filter2d / ::test_filter2d_backward
    assert torch.allclose(xg.grad.cpu(), gx_o, atol=2e-5 if small else 1e-5, rtol=1e-5)
    assert torch.allclose(kg.grad.cpu(), gk_o, atol=2e-3 if small else 1e-2, rtol=1e-4)
    assert torch.equal(xg1.grad, xg.grad)
    return {"y": y0.cpu(), "gx": xg.grad.cpu(), "acc_gk": kg.grad.cpu(), "acc_gk1": kg1.grad.cpu()}


for _i, (_ks, _shape) in enumerate(itertools.product([(3, 3), (5, 5), (7, 7), (4, 6)], FILTER_IMAGES)):
    for _Bk in (1, 2):
        _border = BORDERS[(_i + _Bk) % 4]
        CASES[f"filter2d-{_ks[0]}x{_ks[1]}-{_border}-{'x'.join(map(str, _shape))}-Bk{_Bk}"] = (lambda oracle, a=(_ks, _border, _shape, _Bk): _filter2d_case(oracle, *a))


def _separable_case(oracle, K_, border, shape, Bk, dt):
    import kornia_amd as K

    g = _gen(51 + K_)
    x = torch.rand(*shape, generator=g).to(dt)
    kx, ky = torch.rand(Bk, K_, generator=g), torch.rand(Bk, K_, generator=g)
    kx, ky = kx / kx.sum(-1, keepdim=True), ky / ky.sum(-1, keepdim=True)
    go = torch.rand(*shape, generator=g).to(dt)
    xd, kxd, kyd, god = x.cuda(), kx.cuda(), ky.cuda(), go.cuda()
    with unchanged(xd, kxd, kyd, god):
        xg = xd.detach().requires_grad_()
        y = K.filter2d_separable(xg, kxd, kyd, border)
        y.backward(god)
    if dt == F32:  # tests/test_gpu_filters.py::test_register_tiled_blur_fast_path / ::test_large_separable_kernels
        assert torch.equal(y.detach().cpu(), oracle.filter2d_separable(x, kx, ky, border))
        gx_o = oracle.filter2d_separable_backward(go, x, kx, ky, border)
        assert torch.allclose(xg.grad.cpu(), gx_o, atol=2e-5 if K_ <= 9 else 5e-5, rtol=1e-5 if K_ <= 9 else 1e-4)
    else:          # tests/test_gpu_filters.py::test_half_precision_blur
        ref = oracle.filter2d_separable(x.float(), kx.to(dt).float(), ky.to(dt).float(), border)
        assert y.dtype == dt and (y.detach().float().cpu() - ref).abs().max().item() <= (1e-2 if dt == BF16 else 2e-3)
    return {"y": y.detach().cpu(), "gx": xg.grad.cpu()}


for _i, (_K, _shape) in enumerate(itertools.product([5, 9, 11, 23], FILTER_IMAGES)):
    for _Bk in (1, 2):
        _border = BORDERS[(_i + _Bk) % 4]
        CASES[f"separable-{_K}-{_border}-{'x'.join(map(str, _shape))}-Bk{_Bk}-f32"] = (lambda oracle, a=(_K, _border, _shape, _Bk, F32): _separable_case(oracle, *a))
    CASES[f"separable-{_K}-{BORDERS[_i % 4]}-{'x'.join(map(str, _shape))}-Bk1-bf16"] = (lambda oracle, a=(_K, BORDERS[_i % 4], _shape, 1, BF16): _separable_case(oracle, *a))


@case("spatial_gradient-sobel")
def _case_spatial_gradient(oracle):
    import kornia_amd as K

    res = {}
    for shape in FILTER_IMAGES:
        g = _gen(61)
        x = torch.rand(*shape, generator=g)
        xd = x.cuda()
        for mode, order in (("sobel", 1), ("diff", 1), ("sobel", 2), ("diff", 2)):
            ref = oracle.spatial_gradient(x, mode, order)
            go = torch.rand(ref.shape, generator=g)
            god = go.cuda()
            with unchanged(xd, god):
                xg = xd.detach().requires_grad_()
                out = K.spatial_gradient(xg, mode, order)
                out.backward(god)
            assert torch.equal(out.detach().cpu(), ref)  # tests/test_gpu_filters.py::test_register_tiled_spatial_gradient
            assert torch.allclose(xg.grad.cpu(), oracle.spatial_gradient_backward(go, x, mode, order), atol=1e-5, rtol=1e-5)
            res.update({f"{shape}{mode}{order}": out.detach().cpu(), f"{shape}{mode}{order}g": xg.grad.cpu()})
        with unchanged(xd):
            s = K.sobel(xd)
        assert torch.equal(s.cpu(), oracle.sobel(x))
        res[f"{shape}sobel"] = s.cpu()
    return res


def _median_case(oracle, k, shape, dt, view):
    import kornia_amd.filters as KF
    from test_gpu_median import unaligned
    from test_median_golden import restate, restate_grad

    g = _gen(70 + k)
    x = torch.randn(*shape, generator=g).to(dt)
    go = torch.randint(-2, 3, shape, generator=g).to(dt)  # small integers: every order of the backward's sums is exact, in bf16 too
    xd = unaligned(x) if view == "unaligned" else x.cuda()
    god = go.cuda()
    with unchanged(xd, god):
        y0 = KF.median_blur(xd, k)  # without the index plane
        xg = xd.detach().requires_grad_()
        y = KF.median_blur(xg, k)   # with it
        y.backward(god)
    want, _ = restate(x, k)
    assert torch.equal(y0.cpu(), want) and torch.equal(y.detach(), y0)
    assert torch.equal(xg.grad.cpu(), restate_grad(x, k, go)[0])
    return {"y": y0.cpu(), "gx": xg.grad.cpu()}


for _k, _shape, _dt, _view in [(3, (2, 3, 64, 64), F32, "aligned"), (5, (2, 3, 64, 64), BF16, "aligned"), (7, (2, 3, 64, 64), F32, "aligned"), (3, (2, 3, 37, 53), BF16, "aligned"),
                               (5, (2, 3, 37, 53), F32, "aligned"), (7, (2, 3, 37, 53), F16, "aligned"), (3, (2, 3, 37, 53), F32, "unaligned"), (5, (2, 3, 64, 64), F32, "unaligned"),
                               (7, (2, 3, 37, 53), BF16, "unaligned")]:
    CASES[f"median-{_k}-{'x'.join(map(str, _shape))}-{DT_NAME[_dt]}-{_view}"] = (lambda oracle, a=(_k, _shape, _dt, _view): _median_case(oracle, *a))


# ---- pyramid ------------------------------------------------------------------------------------------------------------------------------
@case("pyramid")
def _case_pyramid(oracle):
    """km_pyrdown_fwd / km_resize_bilinear_fwd / _bwd and the adjoints of pyrdown / pyrup (tests/test_gpu_pyramid.py)"""
    import kornia_amd as K

    T = K.geometry.transform
    res = {}
    g = _gen(81)
    for (H, W), size in (((37, 53), (23, 71)), ((64, 64), (32, 32))):
        x = torch.rand(2, 3, H, W, generator=g)
        xd = x.cuda()
        for align in (False, True):
            go = torch.rand(2, 3, *size, generator=g)
            god = go.cuda()
            with unchanged(xd, god):
                xg = xd.detach().requires_grad_()
                r = T.resize_bilinear(xg, size, align)
                r.backward(god)
                xg2 = xd.detach().requires_grad_()
                down = T.pyrdown(xg2, "reflect", align)
                down.sum().backward()
                xg3 = xd.detach().requires_grad_()
                up = T.pyrup(xg3, "reflect", align)
                up.sum().backward()
            assert torch.equal(r.detach().cpu(), oracle.resize_bilinear(x, size, align))
            ref = torch.ops.aten.upsample_bilinear2d_backward(go, list(size), [2, 3, H, W], align, None, None)
            assert (xg.grad.cpu() - ref).abs().max().item() <= 2e-6
            assert torch.equal(down.detach().cpu(), oracle.pyrdown(x, "reflect", align)) and torch.equal(up.detach().cpu(), oracle.pyrup(x, "reflect", align))
            # adjoint identity <A x, 1> = <x, A^T 1> in fp64 sums (tests/test_gpu_filters.py::test_blur_adjoint_identity_at_full_size: 1e-6 relative)
            for out, grad in ((down, xg2.grad), (up, xg3.grad)):
                lhs, rhs = out.detach().double().sum().item(), (x.double() * grad.cpu().double()).sum().item()
                assert abs(lhs - rhs) / abs(lhs) < 1e-6
            res.update({f"{H}{align}r": r.detach().cpu(), f"{H}{align}gr": xg.grad.cpu(), f"{H}{align}d": down.detach().cpu(), f"{H}{align}gd": xg2.grad.cpu(),
                        f"{H}{align}u": up.detach().cpu(), f"{H}{align}gu": xg3.grad.cpu()})
        xb = x.to(BF16).cuda()
        with unchanged(xb):
            db, rb = T.pyrdown(xb), T.resize_bilinear(xb, size)
        assert (db.float().cpu() - oracle.pyrdown(x.to(BF16).float())).abs().max().item() <= 1e-2  # ::test_half_precision
        assert (rb.float().cpu() - oracle.resize_bilinear(x.to(BF16).float(), size)).abs().max().item() <= 1e-2
        res.update({f"{H}db": db.cpu(), f"{H}rb": rb.cpu()})
    return res


# ---- colour -------------------------------------------------------------------------------------------------------------------------------
@case("color_jitter")
def _case_color(oracle):
    """km_color_jitter_fwd / _fwd_masked / _bwd / km_color_params_ws_fwd / km_color_params_fwd: `apply` and `enable` mixed, the contrast stage's
    workspace passed as it was allocated (the launch that makes the table zeroes it), both plane sizes (vector and scalar path), 16-bit"""
    import color_ref
    import kornia_amd.augmentation as A
    from kornia_amd import _native as N
    from kornia_amd.enhance.adjust import color_jitter, color_jitter_from_table

    res = {}
    for (H, W), order in itertools.product(((7, 9), (16, 24)), ("0123", "2031")):
        B = 2
        stages = [int(c) for c in order]
        g = _gen(91 + H)
        x = torch.rand(B, 3, H, W, generator=g)
        w = torch.randn(B, 3, H, W, generator=g)
        f = [0.8 + 0.4 * torch.rand(B, generator=g) for _ in range(3)] + [(torch.rand(B, generator=g) - 0.5) * 0.2]
        xd, wd, fd = x.cuda(), w.cuda(), [t.cuda() for t in f]
        apply = torch.tensor([True, False]).cuda()
        enable = torch.tensor([1, 1, 0, 1]).cuda()
        with unchanged(xd, wd, apply, enable, *fd):
            xg = xd.detach().requires_grad_()
            fg = [t.detach().requires_grad_() for t in fd]
            y = color_jitter(xg, *fg, stages)
            (y * wd).sum().backward()
            ya = color_jitter(xd, *fd, stages, apply=apply)
            ye = color_jitter(xd, *fd, stages, enable=enable)
            xga = xd.detach().requires_grad_()
            (color_jitter(xga, *fd, stages, apply=apply) * wd).sum().backward()
            # the augmentation entry: table, switches and the zeroed workspace from one launch, then the fused kernel on an `empty` gray_ws
            P = {"brightness_factor": fd[0], "contrast_factor": fd[1], "saturation_factor": fd[2], "hue_factor": fd[3], "order": torch.tensor(stages),
                 "batch_prob": torch.tensor([0.9, 0.1]).cuda()}
            yaug = A.color_jitter(xd, P)
            # the same by hand: the table's launch zeroes a workspace handed over as allocated, color_jitter_from_table accumulates into it
            tab, en, ap = _raw("table", (B, 4), F32), _raw("enable", (4,), torch.uint8), _raw("apply", (B,), torch.uint8)
            gray_ws = _raw("gray_ws", (B,), torch.float64)
            N.check(_lib().km_color_params_ws_fwd(*(t.data_ptr() for t in fd), P["batch_prob"].data_ptr(), tab.data_ptr(), en.data_ptr(), ap.data_ptr(), gray_ws.data_ptr(), B,
                                                  _stream()), "km_color_params_ws_fwd")
            ytab = color_jitter_from_table(xd, tab, en, ap, stages, gray_ws)
            y16 = color_jitter(xd.to(BF16), *fd, stages, apply=apply)
        ref = color_ref.color_jitter(x, *f, stages)
        assert torch.allclose(y.detach().cpu(), ref, atol=2e-5, rtol=0)  # tests/test_gpu_color.py::test_all_orders_vs_restatement
        assert torch.equal(ya[1], xd[1]) and torch.equal(ya[0], y.detach()[0]) and torch.equal(yaug, ya) and torch.equal(ytab, ya)
        refe = color_ref.color_jitter(x, f[0], f[1], torch.ones(B), f[3], stages)
        assert torch.allclose(ye.cpu(), refe, atol=2e-5, rtol=0)
        xr, fr = x.clone().requires_grad_(), [t.clone().requires_grad_() for t in f]
        (color_ref.color_jitter(xr, *fr, stages) * w).sum().backward()  # ::test_backward_matches_autograd_through_the_reference_ops
        assert ((xg.grad.cpu() - xr.grad).abs() > 2e-5 * xr.grad.abs().max()).float().mean().item() <= 1e-4
        for k in range(4):
            assert torch.allclose(fg[k].grad.cpu(), fr[k].grad, rtol=2e-3, atol=2e-3 * fr[k].grad.abs().max().item())
        assert torch.equal(xga.grad[1], wd[1]) and torch.allclose(xga.grad[0], xg.grad[0], atol=1e-6)
        assert y16.dtype == BF16 and torch.allclose(y16.float().cpu()[0], color_ref.color_jitter(x.to(BF16).float(), *f, stages)[0], atol=1e-2)
        tag = f"{H}{order}"
        res.update({tag + "y": y.detach().cpu(), tag + "gx": xg.grad.cpu(), tag + "ya": ya.cpu(), tag + "ye": ye.cpu(), tag + "gxa": xga.grad.cpu(), tag + "aug": yaug.cpu(), tag + "tab": ytab.cpu(),
                    tag + "y16": y16.cpu(), **{f"acc_{tag}gf{k}": fg[k].grad.cpu() for k in range(4)}})
    # km_color_params_fwd (the entry point without the workspace; the Python layer calls km_color_params_ws_fwd) against the same quantities as
    # torch ops (tests/test_gpu_color.py::test_parameter_table_kernel_matches_the_torch_assembly), B = 1 and B = 300
    for B in (1, 300):
        g = _gen(B)
        f = [(0.8 + 0.4 * torch.rand(B, generator=g)).cuda() for _ in range(3)] + [((torch.rand(B, generator=g) - 0.5) * 0.2).cuda()]
        f[2] = torch.ones(B).cuda()  # saturation neutral: its stage switch is off
        prob = torch.rand(B, generator=g).cuda()
        table, enable, apply = _raw("km_color_params_fwd params", (B, 4), F32), _raw("km_color_params_fwd enable", (4,), torch.uint8), _raw("km_color_params_fwd apply", (B,), torch.uint8)
        table2, enable2, apply2 = _raw("km_color_params_ws_fwd params", (B, 4), F32), _raw("km_color_params_ws_fwd enable", (4,), torch.uint8), _raw("km_color_params_ws_fwd apply", (B,), torch.uint8)
        ws = _raw("km_color_params_ws_fwd gray_sum", (B,), torch.float64)
        with unchanged(prob, *f):
            N.check(_lib().km_color_params_fwd(*(t.data_ptr() for t in f), prob.data_ptr(), table.data_ptr(), enable.data_ptr(), apply.data_ptr(), B, _stream()), "km_color_params_fwd")
            N.check(_lib().km_color_params_ws_fwd(*(t.data_ptr() for t in f), prob.data_ptr(), table2.data_ptr(), enable2.data_ptr(), apply2.data_ptr(), ws.data_ptr(), B, _stream()),
                    "km_color_params_ws_fwd")
        assert torch.equal(table[:, :3], torch.stack(f[:3], 1)) and torch.allclose(table[:, 3], f[3] * (2 * math.pi), rtol=1e-6, atol=0)
        assert enable.tolist() == [1, 1, 0, 1] and torch.equal(apply.bool(), prob > 0.5)
        assert torch.equal(table2, table) and torch.equal(enable2, enable) and torch.equal(apply2, apply) and torch.equal(ws, torch.zeros_like(ws))
        res.update({f"table{B}": table.cpu(), f"enable{B}": enable.cpu(), f"apply{B}": apply.cpu(), f"ws{B}": ws.cpu()})
    return res


# ---- crop -> resize -> flip ---------------------------------------------------------------------------------------------------------------------
@case("crop_resize")
def _case_crop_resize(oracle):
    """km_crop_resize_fwd with a uint8 mask and both flips against the package's own composition (tests/test_gpu_aug_crop.py)"""
    from kornia_amd.geometry.transform.crop2d import crop_resize
    from test_gpu_aug_crop import _composition

    B, H, W = 2, 40, 52
    g = _gen(101)
    res = {}
    src = torch.tensor([[[3.0, 2], [41, 2], [41, 30], [3, 30]], [[10.0, 5], [19, 5], [19, 12], [10, 12]]])  # one window shrinks, one grows
    fx, fy = torch.tensor([1.0, 0.0]), torch.tensor([0.0, 1.0])
    for dt, size in itertools.product((F32, BF16, F16), ((17, 23), (32, 32))):
        x = torch.rand(B, 3, H, W, generator=g).to(dt).cuda()
        mask = torch.randint(0, 200, (B, 1, H, W), generator=g).to(torch.uint8).cuda()
        srcd, fxd, fyd = src.cuda(), fx.cuda(), fy.cuda()
        for align, flips in itertools.product((False, True), ((None, None), (fxd, fyd))):
            with unchanged(x, mask, srcd, fxd, fyd):
                out, mout = crop_resize(x, mask, srcd, size, "bilinear", align, "resize", flips[0], flips[1])
            ref, refm = _composition(x, mask, src, size, "bilinear", align, None if flips[0] is None else fx, None if flips[1] is None else fy, dt)
            assert torch.equal(out, ref) and torch.equal(mout, refm)
            res.update({f"{DT_NAME[dt]}{size}{align}{flips[0] is None}": out.cpu(), f"{DT_NAME[dt]}{size}{align}{flips[0] is None}m": mout.cpu()})
        with unchanged(x, mask):
            out, mout = crop_resize(x, mask, None, (H, W), flip_all=3)  # a pure flip of every sample
        assert torch.equal(out, x.flip(-1).flip(-2)) and torch.equal(mout, mask.flip(-1).flip(-2))
        res[f"{DT_NAME[dt]}{size}flip"] = out.cpu()
    return res


# ---- points, Canny, the masked loss, taps --------------------------------------------------------------------------------------------------------
@case("transform_points")
def _case_transform_points(oracle):
    import kornia_amd as K
    from test_gpu_filters import _transform_points_expr, _transform_points_grads

    res = {}
    for D, n_pts, shared in itertools.product((2, 3), (64, 65), (False, True)):
        B = 3
        g = _gen(100 * D + n_pts)
        T = (torch.eye(D + 1)[None] + 0.1 * torch.randn(B, D + 1, D + 1, generator=g))[: 1 if shared else B]
        P = torch.rand(B, n_pts, D, generator=g) * 2 - 1
        go = torch.randn(B, n_pts, D, generator=g)
        Td, Pd, god = T.cuda(), P.cuda(), go.cuda()
        with unchanged(Td, Pd, god):
            Tg, Pg = Td.detach().requires_grad_(), Pd.detach().requires_grad_()
            out = K.transform_points(Tg, Pg)
            out.backward(god)
        assert torch.equal(out.detach().cpu(), oracle.transform_points(T, P))  # tests/test_gpu_filters.py::test_transform_points
        gT64, gP64 = _transform_points_grads(_transform_points_expr, T, P, go, torch.float64)
        gT32, gP32 = _transform_points_grads(_transform_points_expr, T, P, go, F32)
        for got, r64, r32 in ((Tg.grad, gT64, gT32), (Pg.grad, gP64, gP32)):  # ::test_transform_points_backward_fp32_against_fp64
            bracket = (r32 - r64).abs().max().item() + 2.0 ** -23 * r64.abs().max().item()
            assert (got.double().cpu() - r64).abs().max().item() <= 2 * bracket
        tag = f"{D}{n_pts}{shared}"
        res.update({tag + "y": out.detach().cpu(), tag + "gP": Pg.grad.cpu(), "acc_" + tag + "gT": Tg.grad.cpu()})
    return res


@case("canny")
def _case_canny(oracle):
    """km_canny_nms_fwd + km_canny_hysteresis_sweep at 1x3x37x53 against the tensor expressions of the same arithmetic
    (tests/test_zz_gpu_canny.py::test_canny_native_tail_matches_the_tensor_expressions)"""
    import kornia_amd as K
    C = importlib.import_module("kornia_amd.filters.canny")  # (the package attribute of that name is the function)
    from test_zz_gpu_canny import _agree

    shape = (1, 3, 37, 53)
    x = torch.rand(*shape, generator=_gen(7))
    yy, xx = torch.meshgrid(torch.arange(shape[2], dtype=torch.float32), torch.arange(shape[3], dtype=torch.float32), indexing="ij")
    x = 0.15 * x + 0.85 * (torch.sin(xx / 9.0) * torch.cos(yy / 7.0))[None, None] * 0.5 + 0.4
    xd = x.cuda()
    res = {}
    for hyst in (True, False):
        grads = K.spatial_gradient(K.gaussian_blur2d(C._to_gray(xd), (5, 5), (1, 1)), normalized=False)
        with unchanged(xd, grads):
            mag_n, edges_n = C._canny_tail_native(grads, 0.05, 0.4, hyst, 1e-6)
        mag_c, edges_c = K.filters.canny(xd.clone().requires_grad_(), 0.05, 0.4, hysteresis=hyst)
        mag_c, edges_c = mag_c.detach(), edges_c.detach()
        assert _agree(mag_n > 0, mag_c > 0) < 2e-3 and _agree(edges_n, edges_c) < 2e-3
        keep = (mag_n > 0) & (mag_c > 0)
        assert torch.allclose(mag_n[keep], mag_c[keep], atol=1e-6, rtol=0)
        assert set(edges_n.unique().tolist()) <= ({0.0, 1.0} if hyst else {0.0, 0.5, 1.0})
        res.update({f"mag{hyst}": mag_n.cpu(), f"edges{hyst}": edges_n.cpu()})
    return res


@case("masked_loss")
def _case_masked_loss(oracle):
    """km_warp_masked_loss / km_warp_masked_loss_finish / km_scale_f64 at one pyramid level, 2x3x48x52 (tests/test_zz_gpu_registration.py)"""
    import kornia_amd as K
    from kornia_amd import _native as N

    t = K.geometry.transform
    B = 2
    g = _gen(11)
    src, dst = torch.rand(B, 3, 48, 52, generator=g), torch.rand(B, 3, 48, 52, generator=g)
    H = torch.eye(3)[None].repeat(B, 1, 1) + 0.05 * (torch.rand(B, 3, 3, generator=g) - 0.5)
    sd, dd = src.cuda(), dst.cuda()
    res = {}
    for kind, Hm, dt in itertools.product(("l1", "mse"), (H, H[:1]), (F32, torch.float64)):
        ref, gref = oracle.masked_warp_loss(src, dst, Hm, kind, False)
        Hd = Hm.to(dt).cuda()
        with unchanged(sd, dd, Hd):
            Hg = Hd.detach().requires_grad_()
            loss = t.masked_warp_loss(sd, dd, Hg, kind, False)
            (2.5 * loss).backward()
        assert Hg.grad.dtype == dt and abs(loss.item() - ref.item()) < 1e-6 and _rel(Hg.grad.cpu().float(), 2.5 * gref) < 5e-5
        res.update({f"acc_{kind}{Hm.shape[0]}{dt}loss": loss.detach().cpu().reshape(1, 1), f"acc_{kind}{Hm.shape[0]}{dt}g": Hg.grad.cpu()})
    # the tail of km_scale_f64: n = 9 and n = 2 * 9 + 1 values (no multiple of anything), every output dtype
    for n, odt in itertools.product((9, 19), (F32, torch.float64)):
        a = torch.randn(n, generator=g, dtype=torch.float64).cuda()
        s = torch.tensor([2.5], dtype=odt).cuda()
        out = _raw("km_scale_f64 out", (n,), odt)
        with unchanged(a, s):
            N.check(_lib().km_scale_f64(a.data_ptr(), s.data_ptr(), N.dtype_code(odt), out.data_ptr(), N.dtype_code(odt), n, _stream()), "km_scale_f64")
        assert torch.equal(out, (a * 2.5).to(odt))
        res[f"scale{n}{odt}"] = out.cpu()
    return res


@case("gaussian_taps")
def _case_gaussian_taps(oracle):
    """km_gaussian_taps_fwd / km_gaussian_taps_dtype_fwd at B = 1 and B = 300 against the oracle's taps and each other
    (tests/test_gpu_augmentation.py::test_gaussian_taps_dtype_entry_point_is_the_cast_round_trip)"""
    import kornia_amd.augmentation as A

    res = {}
    for B in (1, 300):
        g = _gen(B)
        sigma = (0.1 + 1.9 * torch.rand(B, generator=g)).cuda()
        prob = (torch.rand(B, generator=g) < 0.6).float().cuda()
        s2 = sigma.unsqueeze(-1).expand(-1, 2).contiguous()
        for ks in ((5, 5), (3, 7)):
            with unchanged(sigma, prob, s2):
                ox, oy = A.gaussian_taps(s2, ks)
                ax, ay = A.gaussian_taps(s2, ks, apply=prob > 0.5)
                taps = {dt: A.gaussian_taps(sigma, ks, batch_prob=prob, round_to=dt) for dt in (F32, BF16, F16)}
            assert torch.allclose(ox.cpu(), oracle.gaussian_kernel1d(ks[1], sigma.cpu().view(B, 1)), atol=3e-7)  # (exp() on the GPU vs the CPU: test_gaussian_blur2d)
            assert torch.allclose(oy.cpu(), oracle.gaussian_kernel1d(ks[0], sigma.cpu().view(B, 1)), atol=3e-7)
            on = (prob > 0.5).view(-1, 1)
            ident = lambda k: torch.nn.functional.one_hot(torch.tensor(k // 2), k).float().cuda()  # noqa: E731
            assert torch.equal(ax, torch.where(on, ox, ident(ks[1]))) and torch.equal(ay, torch.where(on, oy, ident(ks[0])))
            for dt, (nx, ny) in taps.items():
                assert torch.equal(nx, ax.to(dt).float()) and torch.equal(ny, ay.to(dt).float())
                res.update({f"{B}{ks}{DT_NAME[dt]}x": nx.cpu(), f"{B}{ks}{DT_NAME[dt]}y": ny.cpu()})
            res.update({f"{B}{ks}ox": ox.cpu(), f"{B}{ks}oy": oy.cpu(), f"{B}{ks}ax": ax.cpu(), f"{B}{ks}ay": ay.cpu()})
    return res


@case("warp_blur")
def _case_warp_blur(oracle):
    """km_warp2d_blur_fwd (+ its backward: the separable adjoint, then the warp's) against the two ops one after the other
    (tests/test_gpu_warp_blur.py)"""
    import kornia_amd as K

    T = K.geometry.transform
    res = {}
    g = _gen(121)
    for H, W, h, w in WARP_SHAPES:
        x = torch.rand(2, 3, H, W, generator=g)
        go = torch.rand(2, 3, h, w, generator=g) - 0.4
        M = _matrices("persp", 2, H, W, h, w, g)
        xd, Md, god = x.cuda(), M.cuda(), go.cuda()
        with unchanged(xd, Md, god):
            xg, Mg = xd.detach().requires_grad_(), Md.detach().requires_grad_()
            y = T.warp_perspective_blur(xg, Mg, (h, w), (5, 5), (1.5, 1.5))
            y.backward(god)
        ref = oracle.gaussian_blur2d(oracle.warp_perspective(x, M, (h, w)), (5, 5), (1.5, 1.5))
        assert torch.equal(y.detach().cpu(), ref)
        gw_o = oracle.gaussian_blur2d_backward(go, oracle.warp_perspective(x, M, (h, w)), (5, 5), (1.5, 1.5))
        gx_o, gM_o = oracle.warp_perspective_backward(gw_o, x, M, (h, w))
        assert torch.allclose(xg.grad.cpu(), gx_o, atol=2e-5, rtol=1e-5) and _rel(Mg.grad.cpu(), gM_o) <= 5e-5
        res.update({f"{H}{h}y": y.detach().cpu(), f"{H}{h}gx": xg.grad.cpu(), f"acc_{H}{h}gM": Mg.grad.cpu()})
    return res


@case("homography_chain")
def _case_chain(oracle):
    """km_homography_chain_fwd / _bwd through normalize_homography, B = 1 and B = 300"""
    import kornia_amd as K

    res = {}
    for B in (1, 300):
        g = _gen(B)
        M = _matrices("persp", B, 70, 93, 37, 53, g)
        Md = M.cuda()
        go = torch.randn(B, 3, 3, generator=g).cuda()
        with unchanged(Md, go):
            Mg = Md.detach().requires_grad_()
            A_ = K.normalize_homography(Mg, (70, 93), (37, 53))
            A_.backward(go)
        assert torch.allclose(A_.detach().cpu(), oracle.normalize_homography(M, (70, 93), (37, 53)), atol=1e-6, rtol=1e-6)
        res.update({f"A{B}": A_.detach().cpu(), f"gM{B}": Mg.grad.cpu()})
    return res


@case("stream_copy")
def _case_stream_copy(oracle):
    from kornia_amd import _native as N

    src = torch.rand(4096 + 4, generator=_gen(3)).cuda()
    res = {}
    for nt in (0, 1):
        dst = _raw("km_stream_copy dst", (4096 + 4,), F32)
        with unchanged(src):
            N.check(_lib().km_stream_copy(src.data_ptr(), dst.data_ptr(), 4 * (4096 + 4), nt, _stream()), "km_stream_copy")
        assert torch.equal(dst, src)
        res[f"dst{nt}"] = dst.cpu()
    return res


# =====================================================================================================================================
# the runners
# =====================================================================================================================================
_RAN = {}  # case -> the km_* symbols it called (this process)

# entry points that write no device memory: version, features, configuration, capability and size queries, diagnostics
NON_WRITING = {"km_abi_version", "km_abi_features", "km_last_error", "km_device_info", "km_set_traversal", "km_config_set", "km_config_get",
               "km_filter2d_sep_supported", "km_warp2d_blur_supported", "km_median_blur_supported", "km_warp2d_bwd_needs_zero_init", "km_warp2d_bwd_workspace_bytes"}


# a short list of cases that between them call every writing entry point: what the coverage test runs first in a process that has not run
# the table itself (a worker of a parallel run)
ONE_OF_EACH = ("warp2d_bwd-abi", "inverse_chain", "warp-fwd_masked-and-chain", "warp-pair-select-inverse", "grid_sample-bilinear-zeros-perbatch-f32", "filter2d-3x3-reflect-2x3x37x53-Bk1",
               "separable-5-reflect-2x3x37x53-Bk1-f32", "spatial_gradient-sobel", "median-3-2x3x37x53-f32-unaligned", "pyramid", "color_jitter", "crop_resize", "transform_points",
               "canny", "masked_loss", "gaussian_taps", "warp_blur", "homography_chain", "stream_copy", "warp-persp-f32-C3-70x93x37x53-zeros-default-xM-pads")


def _run_case(name, oracle, fill):
    with guarded(fill) as g:
        res = CASES[name](oracle)
    _RAN.setdefault(name, set()).update(g.called)
    return res


@pytest.mark.parametrize("name", list(CASES))
def test_table(oracle, name):
    """The case under both fills: its own assertions against the oracle hold under each, the guard bands are intact, the inputs unchanged,
    and the two runs agree bit for bit (sums of fp64 atomics: ACC_REL) - every element was written and nothing was read first."""
    a, b = (_run_case(name, oracle, fill) for fill in FILLS)
    assert a.keys() == b.keys() and a
    for k in a:
        if k.startswith("acc_"):
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype
            rel = _rel(a[k].reshape(1, -1), b[k].reshape(1, -1))
            assert rel <= ACC_REL, f"{k}: the two fills differ by {rel:.2e} of the largest entry"
        elif k.startswith("atm_"):
            far = _within_ulps(a[k], b[k], a[k].dtype, atol=2e-5 * max(1.0, b[k].double().abs().max().item()))
            assert far <= 1.0, f"{k}: the two fills differ by {far:.2e} of the bound of the fp32 atomics' order"
        else:
            assert same_bits(a[k], b[k]), f"{k}: the results under the fills 0xFF and 0x7B differ - an element never written, or read before it was"


def test_every_writing_entry_point_has_a_guarded_case(oracle):
    """The symbols called under the guard over the table are the exported ones minus those that write nothing: a new entry point without a
    guarded case fails here.  (Cases another worker process of a parallel run took are run here once.)"""
    from kornia_amd import _native

    want = set(_native.exported_symbols()) - NON_WRITING
    for name in sorted(CASES, key=lambda n: n not in ONE_OF_EACH):  # (the short list first; the rest only while a symbol is still missing)
        if name not in _RAN and not want <= set().union(*_RAN.values()):
            _run_case(name, oracle, FILLS[0])
    called = set().union(*_RAN.values())
    assert want - called == set(), f"no guarded case calls {sorted(want - called)}"
    assert called - NON_WRITING - want == set(), sorted(called - NON_WRITING - want)


def test_the_guard_sees_a_stray_write_and_a_hole():
    """The mechanism's own teeth, without a kernel: a one-element overrun of a payload trips the band check and names the allocation; a
    buffer nobody writes differs between the two fills."""
    from guarded_alloc import GuardBandOverwritten, current

    with pytest.raises(GuardBandOverwritten, match=r"test buffer .*\(3, 5\).*offset 60"):
        with guarded(0xFF):
            t = current().alloc((3, 5), F32, "cuda", False, "test buffer")
            # (the payload is aligned as the allocator's own blocks are: 256 bytes and more on the device, 64 on the host build)
            assert t.is_contiguous() and t.data_ptr() % (256 if torch.cuda.is_available() else 64) == 0 and bool(t.isnan().all())
            t.as_strided((16,), (1,))[15] = 1.0  # one element past the payload
    with pytest.raises(GuardBandOverwritten, match=r"offset -1"):
        with guarded(0x7B):
            t = current().alloc((8,), torch.uint8, "cuda", True, "test buffer")
            assert t.tolist() == [0] * 8
            t.as_strided((1,), (1,), t.storage_offset() - 1)[0] = 0  # one byte before it
    holes = []
    for fill in FILLS:
        with guarded(fill):
            holes.append(current().alloc((4,), torch.int64, "cuda", False, "test buffer").cpu())
    assert not same_bits(*holes)
