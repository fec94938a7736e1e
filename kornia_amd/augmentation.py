"""The augmentation layer's callers of the hot path, parameter-driven.

The reference's ``RandomAffine`` / ``ColorJitter`` / ``RandomGaussianBlur`` (kornia/augmentation/_2d/geometric/affine.py:125-162,
_2d/intensity/color_jitter.py:126-159, _2d/intensity/gaussian_blur.py:95-114) split every call into *sample parameters*
(host-side random generators) and *apply them* (``compute_transformation`` + ``apply_transform`` + the ``batch_prob``
blend of ``_AugmentationBase.transform_inputs``, augmentation/base.py:348-393).  This module is the second half, taking the
parameter dictionaries the reference's generators produce (or a replay of them, ``AugmentationSequential(x, params=...)``):

* :func:`random_affine` - parameters (B,...) -> pixel matrix -> normalise / invert in ONE launch (``km_affine_params_chain_fwd``:
  the prologue of the warp) -> sample; under autograd the same through ``km_affine_matrix2d_fwd`` + ``warp_affine``;
* :func:`color_jitter` - the four adjustments in the sampled order, one fused kernel (+ one reduction pass for the contrast mean);
* :func:`random_gaussian_blur` - per-sample sigma -> taps (``km_gaussian_taps_fwd``, one launch) -> fused separable blur;
* the per-sample apply probability (``batch_prob``, base.py:348-393) rides INSIDE the three launches - the warp copies the samples
  that are not transformed (``km_warp2d_fwd_masked``), the colour kernel passes them through (``km_color_jitter_fwd_masked``), the
  blur gives them the identity kernel (``km_gaussian_taps_fwd``) - so ``torch.where``'s extra pass per stage does not exist;
  :func:`select_samples` (one pass that reads only the kept side, 2e instead of 3e) serves every other augmentation through
  ``patch()``; nothing of this runs when the parameters carry no draw (p = 1);
* :func:`apply_sequence` - the three stages in the order of BASELINE config 3.  It captures into a HIP graph
  (``kornia_amd.graph.capture``) when the parameters are device tensors: nothing in it synchronises.

Parameters stay in float32 whatever the image dtype (the reference rounds them to the image dtype first, which costs a
third of a pixel in bfloat16).  No host synchronisation anywhere: the apply masks are device data.
"""
from __future__ import annotations

import math
from typing import Any, Mapping, Optional, Sequence, Tuple

import torch

from . import _native as N
from .enhance.adjust import color_jitter as _color_jitter, color_jitter_from_table
from .filters.filter import filter2d_separable, filter2d_separable_taps
from .filters.gaussian import gaussian_blur2d
from .geometry.transform.builders import get_affine_matrix2d, get_perspective_transform
from .geometry.transform.imgwarp import COORD_PERSPECTIVE, _warp, _warp_affine_from_chain, warp_affine, warp_perspective

__all__ = ["AugmentationSequential", "ColorJitter", "ParamItem", "RandomAffine", "RandomGaussianBlur", "RandomHorizontalFlip", "RandomPerspective",
           "RandomResizedCrop", "RandomVerticalFlip", "affine_chain", "affine_matrix",
           "apply_sequence", "color_jitter", "gaussian_taps", "inverse_chain", "perspective_chain", "random_affine", "random_gaussian_blur",
           "random_perspective", "select_samples", "warp_pair"]


def _p(params: Mapping[str, Any], key: str, device) -> torch.Tensor:
    v = params[key]
    if type(v) is torch.Tensor and v.dtype is torch.float32 and v.device == device:  # (the modules' own device views: nothing to convert)
        return v
    return torch.as_tensor(v, dtype=torch.float32).to(device=device, dtype=torch.float32)


def _apply_mask(params: Mapping[str, Any], device) -> Optional[torch.Tensor]:
    """(B,) bool ``batch_prob > 0.5`` (base.py:380), or None when the parameters carry no probability draw."""
    if "batch_prob" not in params or params["batch_prob"] is None:
        return None
    return torch.atleast_1d(torch.as_tensor(params["batch_prob"]).to(device) > 0.5)


def _prob(params: Mapping[str, Any], device, B: int) -> Optional[torch.Tensor]:
    """``batch_prob`` as a contiguous (B,) float32 device tensor for the parameter kernels (which threshold it), or None."""
    if "batch_prob" not in params or params["batch_prob"] is None:
        return None
    p = params["batch_prob"]
    if not (type(p) is torch.Tensor and p.dtype is torch.float32 and p.device == device and p.dim() == 1 and p.is_contiguous()):
        p = torch.as_tensor(p).to(device=device, dtype=torch.float32).reshape(-1).contiguous()
    if p.numel() != B:
        raise ValueError(f"batch_prob has {p.numel()} entries, expected the batch size {B}")
    return p


def select_samples(transformed: torch.Tensor, original: torch.Tensor, apply: Optional[torch.Tensor]) -> torch.Tensor:
    """``torch.where(apply[:, None, None, None], transformed, original)`` (base.py:348-361) as one native pass that reads only the
    side it keeps; ``apply`` (B,) bool on the device, ``None`` = every sample was transformed."""
    if apply is None:
        return transformed
    if (transformed.shape != original.shape or transformed.dtype != original.dtype or transformed.dtype not in (torch.float32, torch.bfloat16, torch.float16)
            or apply.shape[0] != transformed.shape[0] or (torch.is_grad_enabled() and (transformed.requires_grad or original.requires_grad))):
        return torch.where(apply.view(-1, *([1] * (transformed.dim() - 1))), transformed, original)
    t, o = transformed.contiguous(), original.contiguous()
    flags = apply.to(device=t.device, dtype=torch.uint8).contiguous()
    out = torch.empty_like(t)
    B = t.shape[0]
    with N.device_guard(t.device):
        N.check(N.lib().km_select_samples_fwd(t.data_ptr(), o.data_ptr(), flags.data_ptr(), out.data_ptr(), B, t.numel() // max(B, 1),
                                              N.dtype_code(t.dtype), N.stream_ptr(t.device)), "km_select_samples_fwd")
    return out


def gaussian_taps(sigma: torch.Tensor, kernel_size, apply: Optional[torch.Tensor] = None, batch_prob: Optional[torch.Tensor] = None,
                  round_to: Optional[torch.dtype] = None) -> tuple:
    """Per-sample 1-D Gaussian taps from ``sigma`` (B,2) = (sigma_y, sigma_x) - or (B,): the same sigma for both axes -:
    ``(taps_x (B,kx), taps_y (B,ky))`` in float32, one launch (``km_gaussian_taps_fwd`` / ``km_gaussian_taps_dtype_fwd``) for the ~16
    elementwise launches of the reference's two ``get_gaussian_kernel1d`` calls.
    ``apply`` (B,) bool: a sample whose entry is False gets the identity kernel (odd sizes), so the blur returns it unchanged - bit for
    bit when the image is finite (0 * inf is NaN).  ``batch_prob`` (B,) float: the same switch from the augmentation layer's draw itself
    (``> 0.5``), thresholded inside the launch.  ``round_to``: the image dtype - the taps come out rounded to it (still float32 values), what
    ``filter2d``'s cast of its kernel to the input dtype does (filter.py:126).  A sigma of 0 gives the identity kernel too (the sigma -> 0
    limit), NaN gives NaN taps."""
    ky, kx = (kernel_size, kernel_size) if isinstance(kernel_size, int) else (int(kernel_size[0]), int(kernel_size[1]))
    s = sigma.detach().to(torch.float32).contiguous()
    B = s.shape[0]
    tx = torch.empty(B, kx, device=s.device, dtype=torch.float32)
    ty = torch.empty(B, ky, device=s.device, dtype=torch.float32)
    if s.dim() == 1 or batch_prob is not None or round_to not in (None, torch.float32):
        if apply is not None:
            raise ValueError("gaussian_taps: with a (B,) sigma, a `batch_prob` or a 16-bit `round_to` the per-sample switch is `batch_prob` (the layer's draw, "
                             "thresholded inside the launch); `apply` (flags) goes with a (B,2) float32 sigma alone")
        if s.dim() not in (1, 2) or (s.dim() == 2 and s.shape[1] != 2):
            raise ValueError("gaussian_taps: sigma must be (B,) or (B,2)")
        prob = None if batch_prob is None else batch_prob.detach().to(device=s.device, dtype=torch.float32).reshape(-1).contiguous()
        if prob is not None and prob.numel() != B:
            raise ValueError(f"batch_prob has {prob.numel()} entries, expected the batch size {B}")
        with N.device_guard(s.device):
            N.check(N.lib().km_gaussian_taps_dtype_fwd(s.data_ptr(), int(s.dim() == 2), N.ptr(prob), tx.data_ptr(), ty.data_ptr(), B, kx, ky,
                                                       N.dtype_code(round_to or torch.float32), N.stream_ptr(s.device)), "km_gaussian_taps_dtype_fwd")
        return tx, ty
    flags = None if apply is None else N.flags(apply, s.device, B)
    with N.device_guard(s.device):
        N.check(N.lib().km_gaussian_taps_fwd(s.data_ptr(), N.ptr(flags), tx.data_ptr(), ty.data_ptr(), B, kx, ky, N.stream_ptr(s.device)), "km_gaussian_taps_fwd")
    return tx, ty


def affine_matrix(params: Mapping[str, Any], device) -> torch.Tensor:
    """RandomAffine.compute_transformation (affine.py:125-141): (B,3,3) float32 pixel matrix from the sampled
    ``translations, center, scale, angle, shear_x, shear_y`` (shears in degrees)."""
    d2r = math.pi / 180.0
    return get_affine_matrix2d(_p(params, "translations", device), _p(params, "center", device), _p(params, "scale", device),
                               _p(params, "angle", device), _p(params, "shear_x", device) * d2r, _p(params, "shear_y", device) * d2r)


def affine_chain(params: Mapping[str, Any], device, height: int, width: int, with_matrix: bool = False):
    """The sampled parameters -> ``(m, M, apply)`` in ONE launch (``km_affine_params_chain_fwd`` = compute_transformation +
    warp_affine's normalise / invert chain + the ``batch_prob > 0.5`` switch): m (B,9) float32, the normalised dst->src matrix the
    warp kernel reads for a same-size warp of a (height, width) image; M (B,3,3) the pixel matrix (the module's
    ``transform_matrix``) when ``with_matrix``, else None; apply (B) uint8 when the parameters carry a probability draw, else None."""
    device = torch.device(device)
    t, c, sc, ang, sx, sy = (_p(params, k, device).contiguous() for k in ("translations", "center", "scale", "angle", "shear_x", "shear_y"))
    B = ang.numel()
    if t.shape != (B, 2) or c.shape != (B, 2) or sc.shape != (B, 2) or sx.numel() != B or sy.numel() != B:
        raise ValueError("translations / center / scale must be (B,2) and angle / shear_x / shear_y (B,)")
    prob = _prob(params, device, B)
    m = torch.empty(B, 9, device=device, dtype=torch.float32)
    M = torch.empty(B, 3, 3, device=device, dtype=torch.float32) if with_matrix else None
    apply = torch.empty(B, device=device, dtype=torch.uint8) if prob is not None else None
    with N.device_guard(device):
        N.check(N.lib().km_affine_params_chain_fwd(t.data_ptr(), c.data_ptr(), sc.data_ptr(), ang.data_ptr(), sx.data_ptr(), sy.data_ptr(), N.ptr(prob),
                                                   N.ptr(M), m.data_ptr(), N.ptr(apply), B, int(height), int(width), int(height), int(width),
                                                   N.stream_ptr(device)), "km_affine_params_chain_fwd")
    return m, M, apply


def random_affine(input: torch.Tensor, params: Mapping[str, Any], resample: str = "bilinear", align_corners: bool = False,
                  padding_mode: str = "zeros", fill_value: Optional[torch.Tensor] = None) -> torch.Tensor:
    """RandomAffine.apply_transform + the batch_prob blend (affine.py:143-162, base.py:380-393)."""
    N.require_device(input, "input")
    if input.dim() == 4 and input.dtype in (torch.float32, torch.bfloat16, torch.float16) and not (torch.is_grad_enabled() and input.requires_grad):
        # parameters -> normalised inverse matrix (+ the per-sample switch) in one launch, the switch applied inside the warp's own launch
        if padding_mode == "fill" and fill_value is None:
            fill_value = torch.zeros(input.shape[1], device=input.device, dtype=input.dtype)
        m, _, apply = affine_chain(params, input.device, input.shape[-2], input.shape[-1])
        return _warp_affine_from_chain(input, m, resample, padding_mode, align_corners, fill_value, apply)
    mask = _apply_mask(params, input.device)
    M = affine_matrix(params, input.device)
    size = (input.shape[-2], input.shape[-1])
    out = warp_affine(input, M[:, :2, :], size, resample, padding_mode, align_corners, fill_value)
    return select_samples(out, input, mask)


def random_perspective(input: torch.Tensor, params: Mapping[str, Any], resample: str = "bilinear", align_corners: bool = False) -> torch.Tensor:
    """RandomPerspective.compute_transformation + apply_transform + the batch_prob blend (perspective.py:92-115, base.py:380-393):
    ``start_points`` / ``end_points`` (B,4,2) -> homography (``km_perspective_transform_fwd``, one launch) -> normalise / invert (one
    launch) -> warp with the per-sample switch inside its launch (``km_warp2d_fwd_masked``: samples whose draw failed are copied)."""
    N.require_device(input, "input")
    dev = input.device
    M = get_perspective_transform(_p(params, "start_points", dev), _p(params, "end_points", dev))
    size = (input.shape[-2], input.shape[-1])
    mask = _apply_mask(params, dev)
    if mask is not None and input.dim() == 4 and mask.numel() == input.shape[0] and not (torch.is_grad_enabled() and input.requires_grad):
        return _warp(input, M, size, COORD_PERSPECTIVE, 1, resample, "zeros", align_corners, torch.zeros(3), mask)
    return select_samples(warp_perspective(input, M, size, resample, "zeros", align_corners), input, mask)


def perspective_chain(params: Mapping[str, Any], device, height: int, width: int, with_matrix: bool = False):
    """RandomPerspective's sampled corners -> ``(m, M, apply)`` in ONE launch (``km_perspective_params_chain_fwd`` = get_perspective_transform +
    warp_perspective's normalise / invert chain + the ``batch_prob > 0.5`` switch), as :func:`affine_chain` does for RandomAffine: m (B,9) float32
    for a same-size warp of a (height, width) image, M (B,3,3) the pixel homography when ``with_matrix``, apply (B) uint8 or None."""
    device = torch.device(device)
    sp, ep = (_p(params, k, device).contiguous() for k in ("start_points", "end_points"))
    B = sp.shape[0]
    if sp.shape != (B, 4, 2) or ep.shape != (B, 4, 2):
        raise ValueError("start_points / end_points must be (B,4,2)")
    prob = _prob(params, device, B)
    m = torch.empty(B, 9, device=device, dtype=torch.float32)
    M = torch.empty(B, 3, 3, device=device, dtype=torch.float32) if with_matrix else None
    apply = torch.empty(B, device=device, dtype=torch.uint8) if prob is not None else None
    with N.device_guard(device):
        N.check(N.lib().km_perspective_params_chain_fwd(sp.data_ptr(), ep.data_ptr(), N.ptr(prob), N.ptr(M), m.data_ptr(), N.ptr(apply), B, int(height),
                                                        int(width), int(height), int(width), N.stream_ptr(device)), "km_perspective_params_chain_fwd")
    return m, M, apply


def inverse_chain(M: torch.Tensor, height: int, width: int, affine: bool) -> torch.Tensor:
    """(B,3,3) forward pixel matrix -> (B,9) float32, the normalised matrix the sampler reads for the INVERSE warp of a (height, width) image
    (``km_inverse_chain_fwd``: the closed-form 3x3 inverse, then warp_affine's - ``affine`` - or warp_perspective's normalise / invert chain)."""
    Mc = M.detach().to(torch.float32).reshape(-1, 3, 3).contiguous()
    B = Mc.shape[0]
    m = torch.empty(B, 9, device=Mc.device, dtype=torch.float32)
    with N.device_guard(Mc.device):
        N.check(N.lib().km_inverse_chain_fwd(Mc.data_ptr(), 2 if affine else 3, m.data_ptr(), B, int(height), int(width), N.stream_ptr(Mc.device)),
                "km_inverse_chain_fwd")
    return m


def _fill_vector(fill_value, C: int, device) -> torch.Tensor:
    """A fill value - a number, a one-element tensor or one value per channel - as the (C,) float32 device vector the sampler reads."""
    f = torch.as_tensor(fill_value if fill_value is not None else 0.0, dtype=torch.float32).detach().to(device=device, dtype=torch.float32).reshape(-1)
    if f.numel() == 1:
        return f.expand(C).contiguous()
    if f.numel() != C:
        raise ValueError(f"fill_value has {f.numel()} entries for {C} channels")
    return f.contiguous()


def warp_pair(image: Optional[torch.Tensor], mask: torch.Tensor, m: torch.Tensor, affine: bool, resample: str = "bilinear", padding_mode: str = "zeros",
              align_corners: bool = False, fill_value=None, apply: Optional[torch.Tensor] = None, image_dtype: Optional[torch.dtype] = None):
    """An image and its label mask under one normalised (B,9) float32 matrix and per-sample switch, in one native call
    (``km_warp2d_pair_fwd``): the image as :func:`_warp_affine_from_chain` / the masked perspective warp return it (bit-identical), the mask
    as ``warp(mask.to(image dtype), mode="nearest", ...).to(mask.dtype)`` - the augmentation container's treatment of masks
    (kornia/augmentation/container/augment.py:596-618).  ``image`` None: the mask alone (``image_dtype`` names the dtype of its round trip).
    Returns ``(image_out or None, mask_out)``.  Forward only."""
    from .geometry.transform.imgwarp import _mode_codes, _prepare_fill
    dt = image.dtype if image is not None else image_dtype
    if dt not in (torch.float32, torch.bfloat16, torch.float16):
        raise TypeError(f"the pair warp takes float32 / bfloat16 / float16 images, got {dt}")
    N.require_device(mask, "mask")
    B, Cm, H, W = mask.shape
    dev = mask.device
    if image is not None and (image.dim() != 4 or image.shape[0] != B or tuple(image.shape[-2:]) != (H, W) or image.device != dev):
        raise ValueError(f"mask {tuple(mask.shape)} does not match the image {tuple(image.shape)}")
    if m.dtype != torch.float32 or tuple(m.shape) != (B, 9):
        raise TypeError("the pair warp takes a (B,9) float32 matrix")
    interp, pad = _mode_codes(resample, padding_mode)
    x = image.detach().contiguous() if image is not None else None
    C = x.shape[1] if x is not None else 0
    out = torch.empty_like(x) if x is not None else None
    mk = mask.detach().contiguous()
    mout = torch.empty_like(mk)
    fill = mfill = None
    if padding_mode == "fill":
        fv = torch.zeros(C or 1) if fill_value is None else fill_value
        fill = _prepare_fill(fv if isinstance(fv, torch.Tensor) else torch.full((C,), float(fv)), C, dev, torch.float32) if C else None
        mfill = _fill_vector(fv, Cm, dev)  # (one value, or one per mask channel: a per-colour fill has no meaning for a label mask)
    flags = N.flags(apply, dev, B) if apply is not None else None
    with N.device_guard(dev):
        N.check(N.lib().km_warp2d_pair_fwd(N.ptr(x), N.ptr(out), mk.data_ptr(), mout.data_ptr(), m.data_ptr(), N.ptr(flags), B, C, Cm, H, W,
                                           1 if affine else 0, interp, pad, int(bool(align_corners)), N.ptr(fill), N.ptr(mfill), N.dtype_code(dt),
                                           N.mask_dtype_code(mk.dtype), N.stream_ptr(dev)), "km_warp2d_pair_fwd")
    return out, mout


def color_jitter(input: torch.Tensor, params: Mapping[str, Any], order: Optional[Sequence[int]] = None) -> torch.Tensor:
    """ColorJitter.apply_transform (color_jitter.py:126-159): brightness / contrast / saturation / hue in ``params['order']``
    (or the module's fixed ``order``), each stage skipped when its factors are all neutral."""
    N.require_device(input, "input")
    dev = input.device
    bf, cf, sf, hf = (_p(params, k, dev) for k in ("brightness_factor", "contrast_factor", "saturation_factor", "hue_factor"))
    if order is None:
        order = torch.as_tensor(params["order"]).tolist()  # sampled on the host by the reference's generator
    order = [int(i) for i in order]
    B = input.shape[0] if input.dim() == 4 else -1
    if (input.dim() == 4 and input.shape[1] == 3 and all(f.dim() == 1 and f.numel() == B for f in (bf, cf, sf, hf))
            and not (torch.is_grad_enabled() and any(f.requires_grad for f in (bf, cf, sf, hf)))):
        # factor table, stage switches and the per-sample switch in one launch (km_color_params_fwd), then the fused kernel
        prob = _prob(params, dev, B)
        table = torch.empty(B, 4, device=dev, dtype=torch.float32)
        enable = torch.empty(4, device=dev, dtype=torch.uint8)
        apply = torch.empty(B, device=dev, dtype=torch.uint8) if prob is not None else None
        bf, cf, sf, hf = (f.contiguous() for f in (bf, cf, sf, hf))
        gray_ws = torch.empty(B, device=dev, dtype=torch.float64)  # the contrast stage's accumulators: zeroed by the same launch
        with N.device_guard(dev):
            N.check(N.lib().km_color_params_ws_fwd(bf.data_ptr(), cf.data_ptr(), sf.data_ptr(), hf.data_ptr(), N.ptr(prob), table.data_ptr(), enable.data_ptr(),
                                                   N.ptr(apply), gray_ws.data_ptr(), B, N.stream_ptr(dev)), "km_color_params_ws_fwd")
        return color_jitter_from_table(input, table, enable, apply, order, gray_ws)
    enable = torch.stack([(bf != 0).any(), (cf != 1).any(), (sf != 1).any(), (hf != 0).any()])
    return _color_jitter(input, bf, cf, sf, hf, order, enable=enable, apply=_apply_mask(params, dev))


def random_gaussian_blur(input: torch.Tensor, params: Mapping[str, Any], kernel_size=(5, 5), border_type: str = "reflect",
                         separable: bool = True) -> torch.Tensor:
    """RandomGaussianBlur.apply_transform (gaussian_blur.py:95-114): per-sample ``sigma`` (B,), same in both directions."""
    N.require_device(input, "input")
    sigma1 = _p(params, "sigma", input.device)
    if separable and input.dtype in (torch.float32, torch.bfloat16, torch.float16) and sigma1.dim() == 1:
        # taps in float32 from the float32 sigma (the reference rounds sigma to the image dtype first), rounded to the image dtype inside the
        # same launch - filter2d_separable's cast of any kernel (kornia/filters/filter.py:126) - and handed to the fused filter as they are
        ky, kx = (kernel_size, kernel_size) if isinstance(kernel_size, int) else (int(kernel_size[0]), int(kernel_size[1]))
        has_prob = "batch_prob" in params and params["batch_prob"] is not None
        if not has_prob or (kx % 2 == 1 and ky % 2 == 1):
            # the switch rides in the taps: a sample that is not blurred gets the identity kernel: 1 * x + 0 * neighbours = x bit for bit
            # for FINITE images (an inf / NaN pixel of an untouched sample spreads NaN over its neighbourhood, -0.0 comes back as +0.0:
            # patch() therefore keeps the select pass for RandomGaussianBlur; this entry function states the precondition)
            taps_x, taps_y = gaussian_taps(sigma1, kernel_size, batch_prob=torch.as_tensor(params["batch_prob"]) if has_prob else None, round_to=input.dtype)
            return filter2d_separable_taps(input, taps_x, taps_y, border_type)
        taps_x, taps_y = gaussian_taps(sigma1, kernel_size, round_to=input.dtype)
        return select_samples(filter2d_separable_taps(input, taps_x, taps_y, border_type), input, _apply_mask(params, input.device))
    sigma = sigma1.unsqueeze(-1).expand(-1, 2)
    out = gaussian_blur2d(input, kernel_size, sigma.to(input.dtype), border_type, separable)
    return select_samples(out, input, _apply_mask(params, input.device))


def apply_sequence(input: torch.Tensor, affine: Mapping[str, Any], jitter: Mapping[str, Any], blur: Mapping[str, Any],
                   kernel_size=(5, 5)) -> torch.Tensor:
    """BASELINE config 3: RandomAffine -> ColorJitter -> RandomGaussianBlur with replayed parameters."""
    return random_gaussian_blur(color_jitter(random_affine(input, affine), jitter), blur, kernel_size)


# =====================================================================================================================================
# The modules (round 6): BASELINE config 3 AS IT IS WRITTEN - ``AugmentationSequential(RandomAffine(...), ColorJitter(...),
# RandomGaussianBlur(...))(x)`` - with the PARAMETER SAMPLING inside the call.
#
# The functions above take parameter dictionaries somebody else sampled; on a machine without Kornia (the GPU box of this project: the
# reference tree may not travel) that left config 3's public spelling without an implementation and its sampling - which SURVEY.md 8(f) calls
# the real wall time of the layer - outside every timing.  These classes are the missing half, written against the behaviour of
# kornia/augmentation/base.py:179-272 (``__batch_prob_generator__``, ``forward_parameters``), random_generator/_2d/affine.py:161-213,
# random_generator/_2d/color_jitter.py:97-110, random_generator/_2d/gaussian_blur.py:75-79 and container/augment.py:431-500:
#
#   * the draws come from torch's GLOBAL CPU generator in the reference's order - batch_prob first (only for 0 < p < 1), then each quantity as
#     ``low + torch.rand(n) * (high - low)`` in float32 (torch.distributions.Uniform.rsample), a degenerate range still consuming its draw,
#     ``torch.randperm(4)`` last for the colour order - so ``torch.manual_seed(s)`` followed by the same pipeline gives THE SAME parameters as
#     Kornia does (tests/golden/aug_modules.npz: the reference's ``_params`` for seeded calls, compared entry for entry);
#   * a module's draws land in ONE host buffer and cross to the device as ONE copy (the reference moves every parameter tensor on its own);
#     ``_params`` exposes host views with the reference's keys, so a replay through Kornia - or of Kornia's through this - works;
#   * the apply step is the functions above: the per-sample probability switch inside the launches, no blend pass, no host synchronisation.
# Round 7 adds RandomPerspective, label masks in the container (``data_keys`` with "mask" entries) and ``inverse()``; keypoints, boxes,
# dictionaries, lists of masks and ``random_apply`` still raise.  RandomResizedCrop and the two random flips run on the batched crop kernel
# (``km_crop_resize_fwd``); flips right after a slice-mode crop ride in its launch, and children after a crop sample at its size.
from collections import namedtuple

ParamItem = namedtuple("ParamItem", ["name", "data"])  # (module name, parameter dictionary): what ``AugmentationSequential._params`` holds


def _range_pair(value, name: str, center: float, bounds, scalar_ok: bool = True) -> torch.Tensor:
    """(low, high) as a float32 tensor: a single number v means (center - v, center + v) clamped to ``bounds`` - computed in float32 tensor
    arithmetic, as the reference's ``_range_bound`` does, so that the bounds are the same bits - a pair is taken as given."""
    t = value.detach().to(torch.float32).cpu() if isinstance(value, torch.Tensor) else torch.tensor(value, dtype=torch.float32)
    if t.dim() == 0:
        if not scalar_ok or float(t) < 0:
            raise ValueError(f"If {name} is a single number, it must be non negative. Got {t}.")
        t = (t.repeat(2) * torch.tensor([-1.0, 1.0]) + center).clamp(bounds[0], bounds[1])
    if t.shape != (2,):
        raise ValueError(f"{name} must be a number or a (low, high) pair. Got {tuple(t.shape)}.")
    if not (bounds[0] <= float(t[0]) <= float(t[1]) <= bounds[1]):
        raise ValueError(f"{name} out of bounds. Expected inside {bounds} and low <= high, got {t.tolist()}.")
    return t


class _Draws:
    """The host buffer of one module's draws: ``floats`` float32 values in one (pinned) allocation, handed out as contiguous pieces."""

    def __init__(self, floats: int):
        self.buf = torch.empty(max(int(floats), 1), dtype=torch.float32, pin_memory=torch.cuda.is_available())
        self.k = 0

    def piece(self, *shape: int) -> torch.Tensor:
        n = 1
        for v in shape:
            n *= int(v)
        out = self.buf[self.k:self.k + n]
        if len(shape) > 1:
            out = out.view(*shape)
        self.k += n
        return out

    @staticmethod
    def uniforms(lo: torch.Tensor, span: torch.Tensor, B: int, same_on_batch: bool) -> torch.Tensor:
        """k consecutive draws at once, (k, B): ``lo[i] + torch.rand(B) * span[i]`` for i = 0 .. k-1 IN THAT ORDER.  ONE call of the generator
        for what the reference draws in k calls: torch's CPU generator fills a float32 tensor element by element, so ``torch.rand(k * B)`` is
        the concatenation of k ``torch.rand(B)`` (tests/test_gpu_aug_modules.py::test_one_call_of_the_generator_is_k_calls pins that) - and the
        host's share of a call is what bounds config 3 as it is written."""
        k = lo.numel()
        r = torch.rand(k * (1 if same_on_batch else B), dtype=torch.float32).view(k, -1)
        v = lo.view(k, 1) + r * span.view(k, 1)
        return v.expand(k, B) if same_on_batch else v

    @staticmethod
    def uniform(lo_hi: torch.Tensor, B: int, same_on_batch: bool, out: torch.Tensor) -> torch.Tensor:
        """``low + torch.rand(n) * (high - low)`` in float32 from the global CPU generator (torch.distributions.Uniform.rsample), one value
        repeated over the batch for ``same_on_batch``, written to ``out`` (B values, any stride)."""
        r = torch.rand(1 if same_on_batch else B, dtype=torch.float32)
        v = lo_hi[0] + r * (lo_hi[1] - lo_hi[0])
        out.copy_(v.expand(B) if same_on_batch else v)
        return out


class _RandomOp(torch.nn.Module):
    """What the three modules share: p / same_on_batch / keepdim, the probability draw, one host buffer -> one device copy, replay."""

    _FLOATS_PER_SAMPLE = 1  # float32 values the module draws / derives per sample, batch_prob included

    def __init__(self, p: float, same_on_batch: bool, keepdim: bool, p_batch: float = 1.0):
        super().__init__()
        self.p, self.p_batch, self.same_on_batch, self.keepdim = float(p), float(p_batch), bool(same_on_batch), bool(keepdim)
        # (per-call state lives in a plain dict: torch.nn.Module.__setattr__ costs ~10 us per assignment, and the host's share bounds the call)
        object.__setattr__(self, "_st", {"params": {}, "host_buf": None, "dev_buf": None})

    @property
    def _params(self) -> dict:
        return self._st["params"]

    @property
    def _host_buf(self):
        return self._st["host_buf"]

    @property
    def _dev_buf(self):
        return self._st["dev_buf"]

    @_dev_buf.setter
    def _dev_buf(self, v):
        self._st["dev_buf"] = v

    def _sample(self, d: _Draws, shape, params: dict) -> None:
        raise NotImplementedError

    def _apply(self, x: torch.Tensor, params: dict) -> torch.Tensor:
        raise NotImplementedError

    _GEOMETRIC = False  # a geometric module warps masks with its draw; the others leave them alone

    def _batch_prob(self, B: int, out: torch.Tensor) -> torch.Tensor:
        # base.py:179-215: a batch-level gate (p_batch) first, then the per-sample gates; certain outcomes consume nothing
        gate = 1.0
        if 0.0 < self.p_batch < 1.0:
            gate = float((torch.rand(1) < self.p_batch).item())
        elif self.p_batch <= 0.0:
            gate = 0.0
        if self.p >= 1.0 or self.p <= 0.0:  # (certain outcomes: one fill of the piece, no draw)
            out.fill_(gate if self.p >= 1.0 else 0.0)
            return out
        elif self.same_on_batch:
            e = (torch.rand(1) < self.p).to(torch.float32).expand(B)
        else:
            e = (torch.rand(B) < self.p).to(torch.float32)
        out.copy_(e * gate)
        return out

    def forward_parameters(self, batch_shape, draws: Optional[_Draws] = None) -> dict:
        """Sample this call's parameters on the host (the reference's keys; every float tensor a piece of ONE buffer - the container's,
        when it hands one in: then the whole pipeline's draws cross to the device as one copy)."""
        B = int(batch_shape[0])
        d = draws if draws is not None else _Draws(self._FLOATS_PER_SAMPLE * B)
        params: dict = {"batch_prob": self._batch_prob(B, d.piece(B))}
        self._sample(d, batch_shape, params)
        shp = tuple(int(v) for v in batch_shape)
        st = self._st.get("shape_t")
        if st is None or st[0] != shp:  # (the same small tensor for every call at this shape: torch.tensor(...) is 4 us a time)
            st = self._st["shape_t"] = (shp, torch.tensor(shp, dtype=torch.long))
        params["forward_input_shape"] = st[1]
        self._st["host_buf"], self._st["dev_buf"] = d.buf, None
        return params

    def _device_params(self, params: Mapping[str, Any], device, own: bool) -> dict:
        """The parameters as the apply step wants them: this module's own sample crosses to the device as ONE copy of the draw buffer (the
        float tensors of ``params`` are pieces of it); foreign parameters (a replay) go tensor by tensor, as the functions above take them."""
        out = dict(params)
        buf = self._host_buf if own else None
        dev = self._dev_buf if own else None
        if buf is None:
            # a replay: host float tensors that are pieces of ONE allocation (this package's own `_params` are) cross as one copy too
            fl = [v for v in params.values() if isinstance(v, torch.Tensor) and v.dtype == torch.float32 and v.numel() and v.device.type == "cpu" and v.is_contiguous()]
            if len(fl) > 1 and all(v.untyped_storage().data_ptr() == fl[0].untyped_storage().data_ptr() for v in fl):
                buf = torch.empty(0, dtype=torch.float32).set_(fl[0].untyped_storage())
                dev = None
        if buf is not None:
            if dev is None:
                dev = buf.to(device, non_blocking=True)
            base = buf.data_ptr()
            # where the float tensors of `params` sit in the buffer: the same for every call of this module at this batch size (the pieces are
            # handed out in a fixed order) - found once, checked by (key, address offset) since, and each device-side view made by ONE as_strided
            # (a slice + a view per tensor were 30 us of a call whose host share bounds it: profiles/r06/run20_*)
            lkey = "layout" if own else "layout_replay"
            lay = self._st.get(lkey)
            if lay is not None and (lay[0] != buf.numel() or len(lay[1]) > len(params)):
                lay = None
            if lay is not None:
                for k, off, shape, strides in lay[1]:
                    v = params.get(k)
                    if v is None or v.data_ptr() - base != 4 * off or v.shape != shape:
                        lay = None
                        break
            if lay is None:
                found = []
                for k, v in params.items():
                    if isinstance(v, torch.Tensor) and v.dtype == torch.float32 and v.numel() and v.device.type == "cpu" and v.is_contiguous():
                        off = (v.data_ptr() - base) // 4
                        if 0 <= off and off + v.numel() <= buf.numel():
                            found.append((k, off, v.shape, v.stride()))
                lay = self._st[lkey] = (buf.numel(), found)
            for k, off, shape, strides in lay[1]:
                out[k] = dev.as_strided(shape, strides, off)
        if self.p >= 1.0 and self.p_batch >= 1.0:
            out["batch_prob"] = None  # every sample is transformed: no switch in the launches at all
        return out

    def forward(self, input: torch.Tensor, params: Optional[Mapping[str, Any]] = None, _own: bool = False) -> torch.Tensor:
        N.require_device(input, "input")
        if input.dim() not in (3, 4):
            raise ValueError(f"expected a (B, C, H, W) or (C, H, W) image tensor, got {tuple(input.shape)}")
        x = input.unsqueeze(0) if input.dim() == 3 else input
        own = params is None or _own  # (_own: the container sampled these through this module's forward_parameters a moment ago)
        if params is None:
            params = self.forward_parameters(x.shape)
        elif not _own:
            self._st["host_buf"] = None
        self._st["params"] = dict(params)
        self._st["device"] = x.device
        out = self._apply(x, self._device_params(self._st["params"], x.device, own))
        return out[0] if (input.dim() == 3 and self.keepdim) else out


class _GeometricOp(_RandomOp):
    """What RandomAffine and RandomPerspective share beyond the draws: the parameters -> (m, M, apply) chain, label masks warped with the
    image's draw (``km_warp2d_pair_fwd``), the inverse warp (``km_inverse_chain_fwd`` + the same pair launch) and ``transform_matrix``."""

    _GEOMETRIC = True
    _AFFINE = True  # the warp's coordinate generator: affine or perspective

    def _chain(self, params: Mapping[str, Any], device, H: int, W: int, with_matrix: bool = False):
        raise NotImplementedError

    def _fill(self):
        return self.fill_value

    def _warp_with_masks(self, x: torch.Tensor, masks: list, m: torch.Tensor, apply, image_dtype: torch.dtype, image=True):
        """The image (unless ``image`` is False: it was warped elsewhere) + the first mask in one pair launch, further masks mask-only on the
        same matrix and switch."""
        kw = dict(affine=self._AFFINE, resample=self.resample, padding_mode=self.padding_mode, align_corners=self.align_corners,
                  fill_value=self._fill(), apply=apply, image_dtype=image_dtype)
        out, res = x, []
        for k, mk in enumerate(masks):
            o, mo = warp_pair(x if (image and k == 0) else None, mk, m, **kw)
            if image and k == 0:
                out = o
            res.append(mo)
        if image and not masks:
            out, _ = warp_pair(x, x.new_empty((x.shape[0], 0, x.shape[2], x.shape[3]), dtype=torch.uint8), m, **kw)
        return out, res

    def _forward_masks(self, x: torch.Tensor, masks: list, params: Mapping[str, Any], own: bool, image_dtype: torch.dtype):
        """One call of the container with masks: x (B,C,H,W) and masks (B,Cm,H,W) -> (x', masks')."""
        if not own:
            self._st["host_buf"] = None
        self._st["params"] = dict(params)
        self._st["device"] = x.device
        p = self._device_params(self._st["params"], x.device, own)
        B, _, H, W = x.shape
        m, _, apply = self._chain(p, x.device, H, W)
        if torch.is_grad_enabled() and x.requires_grad:  # the image through the differentiable composition, the masks on the chain's matrix
            return self._apply(x, p), self._warp_with_masks(x, masks, m, apply, image_dtype, image=False)[1]
        return self._warp_with_masks(x, masks, m, apply, image_dtype)

    def _inverse_masks(self, x: torch.Tensor, masks: list, params: Mapping[str, Any], image_dtype: torch.dtype):
        """The inverse warp of this module's draw (kornia/augmentation/_2d/geometric/base.py:352-378): Minv by the closed form, samples whose
        draw failed copied, masks nearest."""
        if torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError("inverse() is forward-only here (no autograd through the inverse warp)")
        p = self._device_params(dict(params), x.device, False)
        B, _, H, W = x.shape
        _, M, apply = self._chain(p, x.device, H, W, with_matrix=True)
        return self._warp_with_masks(x, masks, inverse_chain(M, H, W, self._AFFINE), apply, image_dtype)

    def inverse(self, input: torch.Tensor, params: Optional[Mapping[str, Any]] = None, **kwargs) -> torch.Tensor:
        """``kornia.augmentation``'s module inverse (kornia/augmentation/_2d/geometric/base.py:352-378) for an image: the inverse warp of the
        last call's draw (or of ``params``), samples whose probability draw failed returned as they are."""
        if kwargs:
            raise NotImplementedError(f"inverse(): keyword overrides {sorted(kwargs)} are not supported here")
        params = self._params if params is None else params
        if not params:
            raise ValueError("No parameters available for inversing, please run a forward pass first or passing valid params into this function.")
        N.require_device(input, "input")
        x = input.unsqueeze(0) if input.dim() == 3 else input
        out, _ = self._inverse_masks(x, [], params, x.dtype)
        return out[0] if (input.dim() == 3 and self.keepdim) else out

    @property
    def transform_matrix(self) -> Optional[torch.Tensor]:
        """(B,3,3) pixel matrix of the last call (identity for the samples whose probability draw failed), computed on demand on the device of
        the last input."""
        if not self._params:
            return None
        shp = self._params["forward_input_shape"].tolist()
        dev = self._st.get("device") or torch.device("cuda")
        _, M, apply = self._chain(self._params, dev, shp[-2], shp[-1], with_matrix=True)
        if apply is not None:
            M = torch.where(apply.bool().view(-1, 1, 1), M, torch.eye(3, device=M.device).expand_as(M))
        return M


class RandomAffine(_GeometricOp):
    """``kornia.augmentation.RandomAffine`` (kornia/augmentation/_2d/geometric/affine.py:33-162) on the native path: the same constructor,
    the same parameter draws, parameters -> matrix -> normalise / invert in one launch, the warp with the probability switch inside it."""

    _FLOATS_PER_SAMPLE = 10  # batch_prob, angle, shear x / y, scale (2), translation (2), centre (2)

    def __init__(self, degrees, translate=None, scale=None, shear=None, resample="BILINEAR", same_on_batch: bool = False, align_corners: bool = False,
                 padding_mode="ZEROS", fill_value=None, p: float = 0.5, keepdim: bool = False) -> None:
        super().__init__(p, same_on_batch, keepdim)
        self.degrees = _range_pair(degrees, "degrees", 0.0, (-360.0, 360.0))
        self.translate = None
        if translate is not None:
            t = torch.as_tensor(translate, dtype=torch.float32)
            if t.shape != (2,) or not bool(((t >= 0) & (t <= 1)).all()):
                raise ValueError(f"translate must be two fractions in [0, 1]. Got {translate}.")
            self.translate = t
        self.scale = None
        if scale is not None:
            s = torch.as_tensor(scale, dtype=torch.float32)
            if s.shape not in ((2,), (4,)) or not bool((s >= 0).all()):
                raise ValueError(f"'scale' expected to be either 2 or 4 non-negative elements. Got {scale}")
            self.scale = s
        self.shear = None
        if shear is not None:
            sh = torch.as_tensor(shear, dtype=torch.float32)
            if sh.dim() == 0:
                self.shear = torch.stack([_range_pair(sh, "shear-x", 0.0, (-360.0, 360.0)), torch.zeros(2)])
            elif sh.shape == (2,):
                self.shear = torch.stack([_range_pair(sh, "shear-x", 0.0, (-360.0, 360.0)), torch.zeros(2)])
            elif sh.shape == (4,):
                self.shear = torch.stack([_range_pair(sh[:2], "shear-x", 0.0, (-360.0, 360.0)), _range_pair(sh[2:], "shear-y", 0.0, (-360.0, 360.0))])
            elif sh.shape == (2, 2):
                self.shear = sh
            else:
                raise ValueError(f"shear must be a number, a pair, four numbers or a 2 x 2 tensor. Got {shear}.")
        self.resample = str(getattr(resample, "name", resample)).lower()
        self.padding_mode = str(getattr(padding_mode, "name", padding_mode)).lower()
        self.align_corners = bool(align_corners)
        self.fill_value = fill_value
        self._lo = self._span = None

    def _ranges(self):
        """(lo, span) of the module's draws in the reference's order - angle, scale x (, scale y), translation x, y, shear x, y - as float32 vectors,
        formed once (``high - low`` in float32, as torch.distributions.Uniform does)."""
        if getattr(self, "_lo", None) is None:
            pairs = [self.degrees]
            if self.scale is not None:
                pairs.append(self.scale[:2])
                if self.scale.numel() == 4:
                    pairs.append(self.scale[2:])
            if self.translate is not None:
                pairs += [torch.stack([-self.translate[0], self.translate[0]]), torch.stack([-self.translate[1], self.translate[1]])]
            if self.shear is not None:
                pairs += [self.shear[0], self.shear[1]]
            p = torch.stack(pairs).to(torch.float32)
            self._lo, self._span = p[:, 0].contiguous(), (p[:, 1] - p[:, 0]).contiguous()
        return self._lo, self._span

    def _sample(self, d: _Draws, shape, params: dict) -> None:
        # random_generator/_2d/affine.py:161-213: angle, scale (x, then y when four numbers were given), translation x, y, shear x, y
        B, H, W = int(shape[0]), int(shape[-2]), int(shape[-1])
        angle, shx, shy = d.piece(B), d.piece(B), d.piece(B)
        scale, trans, center = d.piece(B, 2), d.piece(B, 2), d.piece(B, 2)
        lo, span = self._ranges()
        geo = self._st.get("geo")
        if geo is None or geo[2] != (H, W):  # ((W, H) and the centre (W / 2 - 0.5, H / 2 - 0.5) as float32 rows, formed once per image size)
            geo = self._st["geo"] = (torch.tensor([float(W), float(H)], dtype=torch.float32), torch.tensor([W / 2.0 - 0.5, H / 2.0 - 0.5], dtype=torch.float32), (H, W))
        v = d.uniforms(lo, span, B, self.same_on_batch)  # (k, B): every draw of the module from ONE call of the generator
        angle.copy_(v[0])
        k = 1
        if self.scale is not None:
            if self.scale.numel() == 4:
                scale.copy_(v[k:k + 2].t())
                k += 2
            else:
                scale.copy_(v[k:k + 1].t().expand(B, 2))
                k += 1
        else:
            scale.fill_(1.0)
        if self.translate is not None:
            trans.copy_(v[k:k + 2].t())
            trans.mul_(geo[0])  # (x by W, y by H: the same float32 products as two column-wise multiplications)
            k += 2
        else:
            trans.zero_()
        center.copy_(geo[1])
        if self.shear is not None:
            shx.copy_(v[k])
            shy.copy_(v[k + 1])
        else:
            shx.zero_()
            shy.zero_()
        params.update(translations=trans, center=center, scale=scale, angle=angle, shear_x=shx, shear_y=shy)

    def _apply(self, x: torch.Tensor, params: dict) -> torch.Tensor:
        fill = self.fill_value
        if fill is not None and not isinstance(fill, torch.Tensor):
            fill = torch.full((x.shape[1],), float(fill))
        return random_affine(x, params, self.resample, self.align_corners, self.padding_mode, fill)

    def _chain(self, params, device, H, W, with_matrix=False):
        return affine_chain(params, device, H, W, with_matrix)


class RandomPerspective(_GeometricOp):
    """``kornia.augmentation.RandomPerspective`` (kornia/augmentation/_2d/geometric/perspective.py:30-130, random_generator/_2d/perspective.py)
    on the native path: the same constructor and draws, corners -> homography -> normalise / invert in one launch
    (``km_perspective_params_chain_fwd``), the warp with the probability switch inside it."""

    _FLOATS_PER_SAMPLE = 17  # batch_prob, start points (8), end points (8)
    _AFFINE = False

    def __init__(self, distortion_scale=0.5, resample="BILINEAR", same_on_batch: bool = False, align_corners: bool = False, p: float = 0.5,
                 keepdim: bool = False, sampling_method: str = "basic") -> None:
        super().__init__(p, same_on_batch, keepdim)
        if sampling_method not in ("basic", "area_preserving"):
            raise NotImplementedError(f"Sampling method {sampling_method} not yet implemented.")
        d = distortion_scale.detach().to(torch.float32).cpu() if isinstance(distortion_scale, torch.Tensor) else torch.as_tensor(distortion_scale, dtype=torch.float32)
        if not (d.dim() == 0 and 0 <= float(d) <= 1):
            raise AssertionError(f"'distortion_scale' must be a scalar within [0, 1]. Got {d}.")
        self.distortion_scale = d
        self.sampling_method = sampling_method
        self.resample = str(getattr(resample, "name", resample)).lower()
        self.align_corners = bool(align_corners)
        self.padding_mode = "zeros"
        self.fill_value = None

    def _sample(self, d: _Draws, shape, params: dict) -> None:
        # random_generator/_2d/perspective.py: the image corners, factor = (d W / 2, d H / 2), ONE draw of (B, 4, 2) uniforms (1 x 4 x 2 with
        # same_on_batch), offset = factor * rand * corner signs ('basic') or 2 factor (rand - 0.5) ('area_preserving'), all in float32
        B, H, W = int(shape[0]), int(shape[-2]), int(shape[-1])
        start, end = d.piece(B, 4, 2), d.piece(B, 4, 2)
        geo = self._st.get("geo")
        if geo is None or geo[2] != (H, W):
            corners = torch.tensor([[[0.0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]]], dtype=torch.float32)
            factor = torch.stack([self.distortion_scale * W / 2, self.distortion_scale * H / 2], dim=0).view(-1, 1, 2)
            geo = self._st["geo"] = (corners, factor, (H, W))
        corners, factor = geo[0], geo[1]
        rand = torch.rand(1 if self.same_on_batch else B, 4, 2, dtype=torch.float32)
        if self.same_on_batch:
            rand = rand.expand(B, 4, 2)
        if self.sampling_method == "basic":
            offset = factor * rand * torch.tensor([[[1.0, 1], [-1, 1], [-1, -1], [1, -1]]], dtype=torch.float32)
        else:
            offset = 2 * factor * (rand - 0.5)
        start.copy_(corners.expand(B, 4, 2))
        torch.add(corners, offset, out=end)
        params.update(start_points=start, end_points=end)

    def _apply(self, x: torch.Tensor, params: dict) -> torch.Tensor:
        if x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16, torch.float16) and not (torch.is_grad_enabled() and x.requires_grad):
            B, C, H, W = x.shape
            m, _, apply = perspective_chain(params, x.device, H, W)
            return self._warp_with_masks(x, [], m, apply, x.dtype)[0]
        return random_perspective(x, params, self.resample, self.align_corners)

    def _chain(self, params, device, H, W, with_matrix=False):
        return perspective_chain(params, device, H, W, with_matrix)


class ColorJitter(_RandomOp):
    """``kornia.augmentation.ColorJitter`` (kornia/augmentation/_2d/intensity/color_jitter.py:34-159): brightness, contrast, saturation and hue
    factors per sample, applied in a random (or the given) order by ONE fused kernel (+ the reduction pass of the contrast mean)."""

    _FLOATS_PER_SAMPLE = 5  # batch_prob, brightness, contrast, hue, saturation

    def __init__(self, brightness=0.0, contrast=0.0, saturation=0.0, hue=0.0, same_on_batch: bool = False, p: float = 1.0, keepdim: bool = False,
                 order: Optional[Sequence[int]] = None) -> None:
        super().__init__(p, same_on_batch, keepdim)
        inf = float("inf")
        self.brightness = _range_pair(brightness, "brightness", 1.0, (0.0, inf))
        self.contrast = _range_pair(contrast, "contrast", 1.0, (0.0, inf))
        self.saturation = _range_pair(saturation, "saturation", 1.0, (0.0, inf))
        self.hue = _range_pair(hue, "hue", 0.0, (-0.5, 0.5))
        if order is not None:
            order = tuple(int(i) for i in order)
            if not set(order) <= {0, 1, 2, 3}:
                raise ValueError(f"`order` entries must be in 0..3 (brightness, contrast, saturation, hue). Got {order}")
        self._fixed_order = order

    def _sample(self, d: _Draws, shape, params: dict) -> None:
        # random_generator/_2d/color_jitter.py:97-110: brightness, contrast, HUE, saturation, then the order of the four stages
        B = int(shape[0])
        if getattr(self, "_lo", None) is None:
            p = torch.stack([self.brightness, self.contrast, self.hue, self.saturation])
            self._lo, self._span = p[:, 0].contiguous(), (p[:, 1] - p[:, 0]).contiguous()
        out = d.piece(4, B)
        out.copy_(d.uniforms(self._lo, self._span, B, self.same_on_batch))
        params["brightness_factor"], params["contrast_factor"], params["hue_factor"], params["saturation_factor"] = out[0], out[1], out[2], out[3]
        params["order"] = torch.randperm(4, dtype=torch.long)

    def _apply(self, x: torch.Tensor, params: dict) -> torch.Tensor:
        return color_jitter(x, params, self._fixed_order)


class RandomGaussianBlur(_RandomOp):
    """``kornia.augmentation.RandomGaussianBlur`` (kornia/augmentation/_2d/intensity/gaussian_blur.py:31-114): one sigma per sample, the
    taps of every sample in one launch, the fused separable blur."""

    _FLOATS_PER_SAMPLE = 2  # batch_prob, sigma

    def __init__(self, kernel_size, sigma, border_type: str = "reflect", separable: bool = True, same_on_batch: bool = False, p: float = 0.5,
                 keepdim: bool = False) -> None:
        super().__init__(p, same_on_batch, keepdim)
        self.kernel_size = (kernel_size, kernel_size) if isinstance(kernel_size, int) else (int(kernel_size[0]), int(kernel_size[1]))
        s = torch.as_tensor(sigma, dtype=torch.float32)
        if s.shape != (2,):
            raise TypeError(f"sigma must be a (min, max) pair. Got {sigma}.")
        if float(s[1]) < float(s[0]):
            raise TypeError(f"sigma_max should be higher than sigma_min: {sigma} passed.")
        if float(s[0]) < 0:
            raise ValueError(f"sigma out of bounds. Expected inside (0, inf), got {s.tolist()}.")
        self.sigma = s
        self.border_type = str(getattr(border_type, "name", border_type)).lower()
        self.separable = bool(separable)

    def _sample(self, d: _Draws, shape, params: dict) -> None:
        params["sigma"] = d.uniform(self.sigma, int(shape[0]), self.same_on_batch, d.piece(int(shape[0])))

    def _apply(self, x: torch.Tensor, params: dict) -> torch.Tensor:
        return random_gaussian_blur(x, params, self.kernel_size, self.border_type, self.separable)


def _inv3x3(M: torch.Tensor) -> torch.Tensor:
    """(B,3,3) -> the inverse by the adjugate, in torch float32 ops on M's device (no host synchronisation, no solver library)."""
    a, b, c = M[:, :, 0], M[:, :, 1], M[:, :, 2]
    r0, r1, r2 = torch.linalg.cross(b, c), torch.linalg.cross(c, a), torch.linalg.cross(a, b)
    det = (a * r0).sum(-1).view(-1, 1, 1)
    return torch.stack([r0, r1, r2], 1) / det


class _CropFlipOp(_GeometricOp):
    """What RandomResizedCrop and the two flips share: the image and the first mask in ONE launch of the batched crop -> resize (-> flip)
    kernel (``km_crop_resize_fwd``, :func:`kornia_amd.geometry.transform.crop_resize`), further masks in mask-only launches, masks always nearest
    and through the image dtype and back (augment.py:596-618)."""

    _NATIVE_DTYPES = (torch.float32, torch.bfloat16, torch.float16)

    def _crop(self, x: Optional[torch.Tensor], mask: Optional[torch.Tensor], p: Mapping[str, Any], image_dtype: torch.dtype, flips=(None, None, 0)):
        raise NotImplementedError

    def _flip_switch(self, p: Mapping[str, Any], device):
        """(switch, bits): this flip's per-sample switch for the launch - its device ``batch_prob`` (thresholded in the launch) - or, when every
        sample flips, None and the axis bit."""
        if p.get("batch_prob") is None:
            return None, self._AXIS_BIT
        return _p(p, "batch_prob", device), 0

    def _run(self, x: torch.Tensor, masks: list, p: Mapping[str, Any], image_dtype: torch.dtype, flips=(None, None, 0)):
        if x.dtype not in self._NATIVE_DTYPES:
            raise TypeError(f"{type(self).__name__}: the native crop / flip takes float32 / bfloat16 / float16 images, got {x.dtype}")
        out, res = x, []
        for k, mk in enumerate(masks):
            o, mo = self._crop(x if k == 0 else None, mk, p, image_dtype, flips)
            if k == 0:
                out = o
            res.append(mo)
        if not masks:
            out, _ = self._crop(x, None, p, image_dtype, flips)
        return out, res

    def _forward_masks(self, x: torch.Tensor, masks: list, params: Mapping[str, Any], own: bool, image_dtype: torch.dtype, flips=(None, None, 0)):
        if not own:
            self._st["host_buf"] = None
        self._st["params"] = dict(params)
        self._st["device"] = x.device
        p = self._device_params(self._st["params"], x.device, own)
        if torch.is_grad_enabled() and x.requires_grad:  # the image through the differentiable composition, the masks through the kernel
            return self._apply(x, p), self._run(x.detach(), masks, p, image_dtype)[1]
        return self._run(x, masks, p, image_dtype, flips)

    def _params_for_device(self, params: Mapping[str, Any], own: bool, device) -> dict:
        """A fused child's share of the call (the container folds it into the crop's launch): the state a call leaves, the device parameters."""
        if not own:
            self._st["host_buf"] = None
        self._st["params"] = dict(params)
        self._st["device"] = device
        return self._device_params(self._st["params"], device, own)


class RandomResizedCrop(_CropFlipOp):
    """``kornia.augmentation.RandomResizedCrop`` (kornia/augmentation/_2d/geometric/resized_crop.py:28-170, random_generator/_2d/crop.py:36-291) on
    the native path: the same constructor, parameter keys and draws (``ResizedCropGenerator`` then ``CropGenerator``, restated in host float32
    torch), ``cropping_mode="slice"`` as ONE launch of the batched crop -> resize for the image and its first mask (flips that follow it in a
    container ride in the same launch), ``"resample"`` as ``crop_by_transform_mat`` (the native warp).  Refused: ``p < 1`` (the reference's
    batch-level gate would return some batches at another size) and ``inverse()`` in slice mode (as in the reference)."""

    _FLOATS_PER_SAMPLE = 17  # batch_prob, src (8), dst (8)

    def __init__(self, size: Tuple[int, int], scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), resample="BILINEAR", same_on_batch: bool = False,
                 align_corners: bool = True, p: float = 1.0, keepdim: bool = False, cropping_mode: str = "slice") -> None:
        super().__init__(1.0, same_on_batch, keepdim, p_batch=p)
        if not (len(size) == 2 and isinstance(size[0], int) and isinstance(size[1], int) and size[0] > 0 and size[1] > 0):
            raise AssertionError(f"`output_size` must be a tuple of 2 positive integers. Got {size}.")
        self.scale = self._range_check(scale, "scale")
        self.ratio = self._range_check(ratio, "ratio")
        self._scale_arg, self._ratio_arg = scale, ratio
        if float(p) < 1.0:
            raise NotImplementedError(f"RandomResizedCrop: p={p} < 1 (the reference's batch-level gate: a batch left alone keeps its size, another "
                                      "is cropped) is not supported on the native path")
        if cropping_mode not in ("slice", "resample"):
            raise NotImplementedError(f"Not supported type: {cropping_mode}.")
        self.size = (int(size[0]), int(size[1]))
        self.resample = str(getattr(resample, "name", resample)).lower()
        if self.resample not in ("bilinear", "nearest"):
            raise NotImplementedError(f"RandomResizedCrop: resample={resample!r} - the native path resamples 'bilinear' or 'nearest'")
        self.align_corners = bool(align_corners)
        self.cropping_mode = cropping_mode
        self.padding_mode = "zeros"
        self.fill_value = None

    @staticmethod
    def _range_check(v, name: str) -> torch.Tensor:
        t = torch.as_tensor(v, dtype=torch.float32)
        # (_joint_range_check, kornia/augmentation/utils/param_validation.py:106-119, with unbounded limits)
        if not (t.dim() == 1 and len(t) == 2):
            raise TypeError(f"{name} should be a torch.Tensor with length 2 whose values between {(float('-inf'), float('inf'))}. Got {t}.")
        if not float(t[0]) <= float(t[1]):
            raise ValueError(f"{name}[0] should be smaller than {name}[1] got {t}")
        return t

    def _sample(self, d: _Draws, shape, params: dict) -> None:
        # ResizedCropGenerator.forward (crop.py:224-291) then CropGenerator.forward (:81-170), operation for operation in float32
        B, H, W = int(shape[0]), int(shape[-2]), int(shape[-1])
        src, dst = d.piece(B, 4, 2), d.piece(B, 4, 2)
        same = self.same_on_batch

        def rand(*shp):
            r = torch.rand(1 if same else B, *shp, dtype=torch.float32)
            return r.repeat(B, *([1] * len(shp))) if same else r

        rand_tensor = rand(10)  # (Uniform(0, 1).rsample: 0 + r * 1, the same bits)
        area = (rand_tensor * (self.scale[1] - self.scale[0]) + self.scale[0]) * H * W
        lo, hi = torch.log(self.ratio[0]), torch.log(self.ratio[1])
        aspect_ratio = torch.exp(lo + rand(10) * (hi - lo))
        w = torch.sqrt(area * aspect_ratio).round().floor()
        h = torch.sqrt(area / aspect_ratio).round().floor()
        cond = ((0 < w) * (w < W) * (0 < h) * (h < H)).int()
        cond_bool, argmax_dim1 = ((cond.cumsum(1) == 1) & cond.bool()).max(1)
        rows = torch.arange(0, B, dtype=torch.long)
        h_out, w_out = h[rows, argmax_dim1], w[rows, argmax_dim1]
        in_ratio = float(H) / float(W)
        _min = float(self._ratio_arg.min()) if isinstance(self._ratio_arg, torch.Tensor) else min(self._ratio_arg)
        if in_ratio < _min:
            h_ct = torch.tensor(H, dtype=torch.float32)
            w_ct = torch.round(h_ct / _min)
        elif in_ratio > _min:
            w_ct = torch.tensor(W, dtype=torch.float32)
            h_ct = torch.round(w_ct * _min)
        else:
            h_ct, w_ct = torch.tensor(H, dtype=torch.float32), torch.tensor(W, dtype=torch.float32)
        h_out = torch.clamp(torch.where(cond_bool, h_out, h_ct.floor()), min=1, max=H)
        w_out = torch.clamp(torch.where(cond_bool, w_out, w_ct.floor()), min=1, max=W)
        size = torch.stack([h_out, w_out], dim=1).floor()
        x_diff = (W - size[:, 1] + 1).clamp(0)
        y_diff = (H - size[:, 0] + 1).clamp(0)
        if same:
            x_start = (rand() * x_diff[0]).floor()
            y_start = (rand() * y_diff[0]).floor()
        else:
            x_start = (rand() * x_diff).floor()
            y_start = (rand() * y_diff).floor()
        cw = torch.where(size[:, 1] == 0, torch.tensor(W, dtype=torch.float32), size[:, 1])
        ch = torch.where(size[:, 0] == 0, torch.tensor(H, dtype=torch.float32), size[:, 0])
        x0, y0 = x_start.view(-1), y_start.view(-1)
        x1, y1 = x0 + cw - 1, y0 + ch - 1
        torch.stack([torch.stack([x0, y0], -1), torch.stack([x1, y0], -1), torch.stack([x1, y1], -1), torch.stack([x0, y1], -1)], -2, out=src)
        oh, ow = self.size
        geo = self._st.get("geo")
        if geo is None or geo[0] != (B, H, W):  # (the constant tensors of this batch shape, formed once)
            geo = self._st["geo"] = ((B, H, W), torch.tensor([[[0.0, 0.0], [ow - 1, 0.0], [ow - 1, oh - 1], [0.0, oh - 1]]], dtype=torch.float32),
                                     torch.tensor((H, W), dtype=torch.long).expand(B, -1), torch.tensor(self.size, dtype=torch.long).expand(B, -1))
        dst.copy_(geo[1].expand(B, 4, 2))
        params.update(src=src, dst=dst, input_size=geo[2], output_size=geo[3])

    def _matrix(self, p: Mapping[str, Any], device) -> torch.Tensor:
        return get_perspective_transform(_p(p, "src", device), _p(p, "dst", device))

    def _crop(self, x, mask, p, image_dtype, flips=(None, None, 0)):
        from .geometry.transform.crop2d import crop_resize

        ref = x if x is not None else mask
        if self.cropping_mode == "slice":
            if self.resample == "nearest" and x is not None:
                raise ValueError("align_corners option can only be set with the interpolating modes: linear | bilinear | bicubic | trilinear")
            return crop_resize(x, mask, _p(p, "src", ref.device), self.size, self.resample, self.align_corners, "resize", *flips, image_dtype=image_dtype)
        # resample: the warp of the box's matrix to the output size (crop_by_transform_mat), masks nearest with the module's align_corners
        M = self._matrix(p, ref.device)[:, :2, :]
        out = warp_affine(x, M, self.size, self.resample, "zeros", self.align_corners) if x is not None else None
        mout = None
        if mask is not None:
            mout = warp_affine(mask.to(image_dtype), M, self.size, "nearest", "zeros", self.align_corners).to(mask.dtype)
        return out, mout

    def _apply(self, x: torch.Tensor, params: dict) -> torch.Tensor:
        from .geometry.transform.crop2d import crop_by_indices, crop_by_transform_mat

        if torch.is_grad_enabled() and x.requires_grad:
            if self.cropping_mode == "slice":
                return crop_by_indices(x, _p(params, "src", x.device), self.size, self.resample, self.align_corners)
            return crop_by_transform_mat(x, self._matrix(params, x.device)[:, :2, :], self.size, self.resample, "zeros", self.align_corners)
        return self._run(x, [], params, x.dtype)[0]

    def _inverse_masks(self, x: torch.Tensor, masks: list, params: Mapping[str, Any], image_dtype: torch.dtype):
        """resized_crop.py:146-170: the warp of the inverse matrix back to the input size (resample mode only)."""
        if self.cropping_mode != "resample":
            raise NotImplementedError(f"`inverse` is only applicable for resample cropping mode. Got {self.cropping_mode}.")
        if torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError("inverse() is forward-only here (no autograd through the inverse warp)")
        p = self._device_params(dict(params), x.device, False)
        shp = torch.as_tensor(params["forward_input_shape"]).tolist()
        size = (int(shp[-2]), int(shp[-1]))
        Minv = _inv3x3(self._matrix(p, x.device))[:, :2, :]
        out = warp_affine(x, Minv, size, self.resample, "zeros", self.align_corners)
        return out, [warp_affine(mk.to(image_dtype), Minv, size, "nearest", "zeros", self.align_corners).to(mk.dtype) for mk in masks]

    @property
    def transform_matrix(self) -> Optional[torch.Tensor]:
        """(B,3,3) ``get_perspective_transform(src, dst)`` of the last call, on the device of the last input."""
        if not self._params:
            return None
        return self._matrix(self._params, self._st.get("device") or torch.device("cuda"))


class _RandomFlip(_CropFlipOp):
    """A random flip on the native path: one launch of the batched crop kernel with the whole image as the window, the per-sample switch
    (``batch_prob > 0.5``) read inside the launch; its own inverse."""

    _FLOATS_PER_SAMPLE = 1  # batch_prob
    _AXIS_BIT = 1
    _DIM = -1

    def __init__(self, p: float = 0.5, same_on_batch: bool = False, keepdim: bool = False) -> None:
        super().__init__(p, same_on_batch, keepdim)
        self.resample, self.align_corners, self.padding_mode, self.fill_value = "nearest", False, "zeros", None

    def _sample(self, d: _Draws, shape, params: dict) -> None:
        return None  # (the probability draw is all a flip samples)

    def _crop(self, x, mask, p, image_dtype, flips=(None, None, 0)):
        from .geometry.transform.crop2d import crop_resize

        ref = x if x is not None else mask
        sw, bits = self._flip_switch(p, ref.device)
        fx, fy = (sw, None) if self._AXIS_BIT == 1 else (None, sw)
        return crop_resize(x, mask, None, tuple(ref.shape[-2:]), "nearest", False, "resize", fx, fy, bits, image_dtype=image_dtype)

    def _apply(self, x: torch.Tensor, params: dict) -> torch.Tensor:
        if torch.is_grad_enabled() and x.requires_grad:
            return select_samples(torch.flip(x, [self._DIM]), x, _apply_mask(params, x.device))
        return self._run(x, [], params, x.dtype)[0]

    def _inverse_masks(self, x: torch.Tensor, masks: list, params: Mapping[str, Any], image_dtype: torch.dtype):
        """horizontal_flip.py:96-115: the same flip again (samples whose draw failed pass through)."""
        p = self._device_params(dict(params), x.device, False)
        if torch.is_grad_enabled() and x.requires_grad:
            return self._apply(x, p), self._run(x.detach(), masks, p, image_dtype)[1]
        return self._run(x, masks, p, image_dtype)

    @property
    def transform_matrix(self) -> Optional[torch.Tensor]:
        """(B,3,3) the reference's flip matrix (``[[-1, 0, w - 1], [0, 1, 0], [0, 0, 1]]`` horizontally, the vertical one likewise) of the last
        call, the identity for the samples whose probability draw failed, on the device of the last input."""
        if not self._params:
            return None
        shp = torch.as_tensor(self._params["forward_input_shape"]).tolist()
        dev = self._st.get("device") or torch.device("cuda")
        M = torch.eye(3, dtype=torch.float32)
        k = 0 if self._AXIS_BIT == 1 else 1
        M[k, k], M[k, 2] = -1.0, float(shp[-1] if k == 0 else shp[-2]) - 1.0
        M = M.to(dev).expand(int(shp[0]), 3, 3)
        apply = _apply_mask(self._params, dev)
        if apply is not None:
            M = torch.where(apply.view(-1, 1, 1), M, torch.eye(3, device=dev).expand_as(M))
        return M


class RandomHorizontalFlip(_RandomFlip):
    """``kornia.augmentation.RandomHorizontalFlip`` (kornia/augmentation/_2d/geometric/horizontal_flip.py:27-115) on the native path."""

    _AXIS_BIT = 1
    _DIM = -1


class RandomVerticalFlip(_RandomFlip):
    """``kornia.augmentation.RandomVerticalFlip`` (kornia/augmentation/_2d/geometric/vertical_flip.py:26-105) on the native path."""

    _AXIS_BIT = 2
    _DIM = -2


_MASK_REFUSED = ("keypoints, boxes, dictionaries, lists of masks and random_apply are not supported here; use Kornia's container with "
                 "kornia_amd.patch()")


class AugmentationSequential(torch.nn.Module):
    """``kornia.augmentation.AugmentationSequential`` (kornia/augmentation/container/augment.py:431-500) for one image tensor and any number of
    label masks: every child samples its parameters and transforms the previous child's output; ``params=`` replays a list of
    ``ParamItem(name, data)`` (this container's ``_params`` - or Kornia's own: the names and keys are the reference's).

    ``data_keys``: one ``"input"`` (or ``"image"``) and any number of ``"mask"`` entries, in any order; the call takes and returns the tensors in
    that order.  A mask is (B, Cm, H, W) - (Cm, H, W) with a (C, H, W) image - of dtype bool / uint8 / int32 / int64 / float32 / bfloat16 /
    float16, and takes the reference's round trip (augment.py:596-618): cast to the image dtype, warped by each geometric child with ``nearest``
    and that child's padding, ``align_corners`` and fill, cast back to the dtype of the LAST mask of ``data_keys`` (the reference's
    ``mask_dtype``); intensity children leave masks alone.  The first mask rides in the image's launch, further masks get mask-only launches on
    the same matrix and switch (``km_warp2d_pair_fwd``).  :meth:`inverse` walks the children backwards."""

    def __init__(self, *args: torch.nn.Module, data_keys=("input",), same_on_batch: Optional[bool] = None, keepdim: Optional[bool] = None,
                 random_apply=False, random_apply_weights=None, transformation_matrix_mode: str = "silent", extra_args=None) -> None:
        super().__init__()
        keys = self._parse_keys(data_keys)
        if random_apply not in (False, None) or random_apply_weights is not None:
            raise NotImplementedError(f"random_apply: {_MASK_REFUSED}")
        for i, m in enumerate(args):
            if not isinstance(m, _RandomOp):
                raise NotImplementedError(f"child {i} ({type(m).__name__}) is not one of this package's modules (RandomAffine, RandomPerspective, "
                                          "RandomResizedCrop, RandomHorizontalFlip, RandomVerticalFlip, ColorJitter, RandomGaussianBlur)")
            if same_on_batch is not None:
                m.same_on_batch = bool(same_on_batch)
            if keepdim is not None:
                m.keepdim = bool(keepdim)
            self.add_module(f"{type(m).__name__}_{i}", m)
        # (per-call state as plain attributes: torch.nn.Module.__setattr__ costs ~5 us per assignment; the children are fixed after construction)
        object.__setattr__(self, "_params", [])
        object.__setattr__(self, "_draws", None)
        object.__setattr__(self, "_kids", list(self.named_children()))
        object.__setattr__(self, "_keys", keys)
        object.__setattr__(self, "_fusion", self._plan_fusion())
        self._check_masks(keys)

    def _plan_fusion(self) -> dict:
        """{index of a slice-mode RandomResizedCrop: indices of the flips directly after it (one horizontal, one vertical at most)}: their
        per-sample switches ride in the crop's launch."""
        plan = {}
        kids = self._kids
        for i, (_, m) in enumerate(kids):
            if type(m) is RandomResizedCrop and m.cropping_mode == "slice":
                group, axes = [], 0
                for j in range(i + 1, len(kids)):
                    f = kids[j][1]
                    if not isinstance(f, _RandomFlip) or axes & f._AXIS_BIT:
                        break
                    group.append(j)
                    axes |= f._AXIS_BIT
                if group:
                    plan[i] = group
        return plan

    def _fused(self, i: int, x: torch.Tensor, masks: list, params, own: bool, image_dtype: torch.dtype):
        """Child i (a slice-mode crop) and the flips after it as ONE launch for the image and the first mask: each flip's call state is what
        its own call would leave, its device ``batch_prob`` the switch the launch reads.  Returns (x, masks, the next child's index)."""
        group = self._fusion[i]
        flips = [None, None, 0]
        for j in group:
            f = self._kids[j][1]
            sw, bits = f._flip_switch(f._params_for_device(params[j].data, own, x.device), x.device)
            flips[0 if f._AXIS_BIT == 1 else 1] = sw
            flips[2] |= bits
        x, masks = self._kids[i][1]._forward_masks(x, masks, params[i].data, own, image_dtype, tuple(flips))
        return x, masks, group[-1] + 1

    def _can_fuse(self, i: int, x: torch.Tensor) -> bool:
        return i in self._fusion and not (torch.is_grad_enabled() and x.requires_grad) and x.dtype in _CropFlipOp._NATIVE_DTYPES

    @staticmethod
    def _parse_keys(data_keys) -> list:
        if isinstance(data_keys, dict):
            raise NotImplementedError(f"data_keys={data_keys!r}: {_MASK_REFUSED}")
        keys = []
        for k in (data_keys or ("input",)):
            k = str(getattr(k, "name", k)).lower()
            keys.append("input" if k in ("input", "image", "0") else k)
        if keys.count("input") != 1 or any(k not in ("input", "mask") for k in keys):
            raise NotImplementedError(f"data_keys={list(data_keys)}: one image key ('input' / 'image') and any number of 'mask' keys are supported; {_MASK_REFUSED}")
        return keys

    def forward_parameters(self, batch_shape) -> list:
        """One ``ParamItem`` per child, sampled in order; the draws of ALL children in one host buffer.  A child whose parameters carry
        ``output_size`` (RandomResizedCrop) changes the shape the children after it sample at (the reference's ``_get_new_batch_shape``,
        container/image.py:401)."""
        B = int(batch_shape[0])
        children = self._kids
        d = _Draws(sum(m._FLOATS_PER_SAMPLE for _, m in children) * B)
        items = []
        for name, m in children:
            prm = m.forward_parameters(batch_shape, d)
            items.append(ParamItem(name, prm))
            osz = prm.get("output_size")
            if osz is not None:
                batch_shape = (*tuple(batch_shape)[:-2], *(int(v) for v in osz[0].tolist()))
        object.__setattr__(self, "_draws", d)
        return items

    def _prepare(self, input: torch.Tensor, params):
        """This call's parameters and whether the children may take the device copy handed to them (their own draws, or a replay whose float
        tensors share one host allocation)."""
        children = self._kids
        if params is not None and len(params) != len(children):
            raise ValueError(f"{len(params)} parameter items for {len(children)} children")
        own = params is None
        if own:
            shape = input.shape if input.dim() == 4 else (1, *input.shape)
            params = self.forward_parameters(shape)
            dev = self._draws.buf.to(input.device, non_blocking=True)  # the whole pipeline's draws: ONE copy
            for _, m in children:
                m._dev_buf = dev
        else:
            # a replay of parameters whose float tensors are pieces of ONE host allocation (this container's own `_params` are): one copy for the
            # whole pipeline here too, handed to the children the way their own draws are
            st_ptr, store = None, None
            for it in params:
                for v in it.data.values():
                    if type(v) is torch.Tensor and v.dtype is torch.float32 and v.device.type == "cpu" and v.numel():
                        sp = v.untyped_storage().data_ptr()
                        if st_ptr is None:
                            st_ptr, store = sp, v.untyped_storage()
                        elif sp != st_ptr:
                            st_ptr = 0
                            break
                if st_ptr == 0:
                    break
            if st_ptr:
                buf = torch.empty(0, dtype=torch.float32).set_(store)
                dev = buf.to(input.device, non_blocking=True)
                for _, m in children:
                    m._st["host_buf"] = buf
                    m._dev_buf = dev
                own = True
        return params, own

    def _split(self, args, keys):
        """(image, [masks], unbatched) from the call's tensors in ``keys`` order, masks checked against the image and made 4-D."""
        if len(args) != len(keys):
            raise NotImplementedError(f"{len(args)} inputs for data_keys={keys}; {_MASK_REFUSED}")
        for a in args:
            if not isinstance(a, torch.Tensor):
                raise NotImplementedError(f"inputs must be tensors, got {type(a).__name__}; {_MASK_REFUSED}")
        img = args[keys.index("input")]
        N.require_device(img, "input")
        if img.dim() not in (3, 4):
            raise ValueError(f"expected a (B, C, H, W) or (C, H, W) image tensor, got {tuple(img.shape)}")
        x = img.unsqueeze(0) if img.dim() == 3 else img
        masks = []
        for a, k in zip(args, keys):
            if k != "mask":
                continue
            N.require_device(a, "mask")
            mk = a.unsqueeze(0) if (a.dim() == 3 and img.dim() == 3) else a
            if mk.dim() != 4 or mk.shape[0] != x.shape[0] or mk.shape[-2:] != x.shape[-2:]:
                raise ValueError(f"a mask must be (B, Cm, H, W) with the image's B, H and W {tuple(x.shape)} (or (Cm, H, W) with a (C, H, W) image), "
                                 f"got {tuple(a.shape)}")
            N.mask_dtype_code(mk.dtype)
            masks.append(mk)
        return x, masks, img.dim() == 3

    def _run_masks(self, args, keys, walk):
        x, masks, unbatched = self._split(args, keys)
        out_dtype = masks[-1].dtype if masks else None  # (the reference's mask_dtype: the last mask's, for every mask)
        work = [mk if mk.dtype == out_dtype else mk.to(x.dtype) for mk in masks]  # (another dtype: cast once, so that its round trip is the reference's)
        x, work = walk(x, work, x.dtype)
        work = [mk if mk.dtype == out_dtype else mk.to(out_dtype) for mk in work]
        keep = unbatched and any(m.keepdim for _, m in self._kids)
        outs, it = [], iter(work)
        for k in keys:
            t = x if k == "input" else next(it)
            outs.append(t[0] if keep else t)
        return outs[0] if len(outs) == 1 else tuple(outs)

    def _check_masks(self, keys) -> None:
        if "mask" in keys and not any(m._GEOMETRIC for _, m in self._kids):
            # (a mask pipeline without a geometric child would only cast the masks there and back)
            raise NotImplementedError("masks go with a geometric child (RandomAffine, RandomPerspective); this pipeline has none")

    def forward(self, *args: torch.Tensor, params: Optional[Sequence[ParamItem]] = None, data_keys=None):
        keys = self._keys if data_keys is None else self._parse_keys(data_keys)
        if data_keys is not None:
            self._check_masks(keys)
        if len(args) == 2 and keys == ["input"] and (args[1] is None or isinstance(args[1], (list, tuple))):
            args, params = args[:1], args[1]  # (the image-only signature forward(input, params))
        children = self._kids
        if keys == ["input"] and len(args) == 1:
            input = args[0]
            params, own = self._prepare(input, params)
            out, used = input, []
            if not self._fusion:
                for i, (name, m) in enumerate(children):
                    out = m(out, params[i].data, _own=own)
                    used.append(ParamItem(name, m._params))
                object.__setattr__(self, "_params", used)
                return out
            x = out.unsqueeze(0) if out.dim() == 3 else out
            i = 0
            while i < len(children):
                if self._can_fuse(i, x):
                    x, _, nxt = self._fused(i, x, [], params, own, x.dtype)
                    used += [ParamItem(children[j][0], children[j][1]._params) for j in range(i, nxt)]
                    i = nxt
                    continue
                x = children[i][1](x, params[i].data, _own=own)
                used.append(ParamItem(children[i][0], children[i][1]._params))
                i += 1
            object.__setattr__(self, "_params", used)
            keep = input.dim() == 3 and any(m.keepdim for _, m in children)
            return x[0] if keep else x
        img = args[keys.index("input")] if len(args) == len(keys) else args[0]
        params, own = self._prepare(img.unsqueeze(0) if img.dim() == 3 else img, params)

        def walk(x, masks, image_dtype):
            used = []
            i = 0
            while i < len(children):
                name, m = children[i]
                if self._can_fuse(i, x):
                    x, masks, nxt = self._fused(i, x, masks, params, own, image_dtype)
                    used += [ParamItem(children[j][0], children[j][1]._params) for j in range(i, nxt)]
                    i = nxt
                    continue
                if m._GEOMETRIC:
                    x, masks = m._forward_masks(x, masks, params[i].data, own, image_dtype)
                else:
                    x = m(x, params[i].data, _own=own)
                used.append(ParamItem(name, m._params))
                i += 1
            object.__setattr__(self, "_params", used)
            return x, masks

        return self._run_masks(args, keys, walk)

    def inverse(self, *args: torch.Tensor, params: Optional[Sequence[ParamItem]] = None, data_keys=None):
        """The inverse of the last call (or of ``params``) for the image and masks (kornia/augmentation/container/augment.py:300-350): the children
        in reverse, geometric ones by the inverse warp of their draw (samples whose probability draw failed returned as they are, masks nearest),
        intensity ones the identity."""
        keys = self._keys if data_keys is None else self._parse_keys(data_keys)
        self._check_masks(keys)
        if params is None:
            if not self._params:
                raise ValueError("No parameters available for inversing, please run a forward pass first or passing valid params into this function.")
            params = self._params
        if len(params) != len(self._kids):
            raise ValueError(f"{len(params)} parameter items for {len(self._kids)} children")

        def walk(x, masks, image_dtype):
            for (name, m), item in reversed(list(zip(self._kids, params))):
                if m._GEOMETRIC:
                    x, masks = m._inverse_masks(x, masks, item.data, image_dtype)
            return x, masks

        return self._run_masks(args, keys, walk)
