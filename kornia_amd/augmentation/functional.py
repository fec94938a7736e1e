"""The augmentation layer's callers of the hot path, parameter-driven.

The reference's ``RandomAffine`` / ``ColorJitter`` / ``RandomGaussianBlur`` (kornia/augmentation/_2d/geometric/affine.py:125-162,
_2d/intensity/color_jitter.py:126-159, _2d/intensity/gaussian_blur.py:95-114) split every call into *sample parameters*
(host-side random generators) and *apply them* (``compute_transformation`` + ``apply_transform`` + the ``batch_prob``
blend of ``_AugmentationBase.transform_inputs``, augmentation/base.py:348-393).  This file is the second half, taking the
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
from typing import Any, Mapping, Optional, Sequence

import torch

from .. import _native as N
from ..enhance.adjust import color_jitter as _color_jitter, color_jitter_from_table
from ..filters.filter import filter2d_separable_taps
from ..filters.gaussian import gaussian_blur2d
from ..geometry.transform.builders import get_affine_matrix2d, get_perspective_transform
from ..geometry.transform.imgwarp import (COORD_PERSPECTIVE, _mode_codes, _prepare_fill, _warp, _warp_affine_from_chain, warp_affine,
                                          warp_perspective)

NATIVE_DTYPES = (torch.float32, torch.bfloat16, torch.float16)  # the image dtypes the kernels take


def _kernel_hw(kernel_size) -> tuple:
    """``kernel_size`` - one number or (ky, kx) - as the pair (ky, kx)."""
    return (kernel_size, kernel_size) if isinstance(kernel_size, int) else (int(kernel_size[0]), int(kernel_size[1]))


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
    if (transformed.shape != original.shape or transformed.dtype != original.dtype or transformed.dtype not in NATIVE_DTYPES
            or apply.shape[0] != transformed.shape[0] or (torch.is_grad_enabled() and (transformed.requires_grad or original.requires_grad))):
        return torch.where(apply.view(-1, *([1] * (transformed.dim() - 1))), transformed, original)
    t, o = transformed.contiguous(), original.contiguous()
    flags = apply.to(device=t.device, dtype=torch.uint8).contiguous()
    out = torch.empty_like(t)
    B = t.shape[0]
    N.launch("km_select_samples_fwd", t.device, t.data_ptr(), o.data_ptr(), flags.data_ptr(), out.data_ptr(), B, t.numel() // max(B, 1), N.dtype_code(t.dtype))
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
    ky, kx = _kernel_hw(kernel_size)
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
        N.launch("km_gaussian_taps_dtype_fwd", s.device, s.data_ptr(), int(s.dim() == 2), N.ptr(prob), tx.data_ptr(), ty.data_ptr(), B, kx, ky,
                 N.dtype_code(round_to or torch.float32))
        return tx, ty
    flags = None if apply is None else N.flags(apply, s.device, B)
    N.launch("km_gaussian_taps_fwd", s.device, s.data_ptr(), N.ptr(flags), tx.data_ptr(), ty.data_ptr(), B, kx, ky)
    return tx, ty


def affine_matrix(params: Mapping[str, Any], device) -> torch.Tensor:
    """RandomAffine.compute_transformation (affine.py:125-141): (B,3,3) float32 pixel matrix from the sampled
    ``translations, center, scale, angle, shear_x, shear_y`` (shears in degrees)."""
    d2r = math.pi / 180.0
    return get_affine_matrix2d(_p(params, "translations", device), _p(params, "center", device), _p(params, "scale", device),
                               _p(params, "angle", device), _p(params, "shear_x", device) * d2r, _p(params, "shear_y", device) * d2r)


def _params_chain(entry: str, inputs, params: Mapping[str, Any], B: int, device, height: int, width: int, with_matrix: bool):
    """What the two ``*_chain`` functions share: the outputs ``(m, M, apply)`` and the launch of ``entry`` (a ``km_*_params_chain_fwd``) on the
    contiguous float32 ``inputs`` for a same-size warp of a (height, width) image."""
    prob = _prob(params, device, B)
    m = torch.empty(B, 9, device=device, dtype=torch.float32)
    M = torch.empty(B, 3, 3, device=device, dtype=torch.float32) if with_matrix else None
    apply = torch.empty(B, device=device, dtype=torch.uint8) if prob is not None else None
    N.launch(entry, device, *(t.data_ptr() for t in inputs), N.ptr(prob), N.ptr(M), m.data_ptr(), N.ptr(apply), B, int(height), int(width), int(height), int(width))
    return m, M, apply


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
    return _params_chain("km_affine_params_chain_fwd", (t, c, sc, ang, sx, sy), params, B, device, height, width, with_matrix)


def random_affine(input: torch.Tensor, params: Mapping[str, Any], resample: str = "bilinear", align_corners: bool = False,
                  padding_mode: str = "zeros", fill_value: Optional[torch.Tensor] = None) -> torch.Tensor:
    """RandomAffine.apply_transform + the batch_prob blend (affine.py:143-162, base.py:380-393)."""
    N.require_device(input, "input")
    if input.dim() == 4 and input.dtype in NATIVE_DTYPES and not (torch.is_grad_enabled() and input.requires_grad):
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
    return _params_chain("km_perspective_params_chain_fwd", (sp, ep), params, B, device, height, width, with_matrix)


def inverse_chain(M: torch.Tensor, height: int, width: int, affine: bool) -> torch.Tensor:
    """(B,3,3) forward pixel matrix -> (B,9) float32, the normalised matrix the sampler reads for the INVERSE warp of a (height, width) image
    (``km_inverse_chain_fwd``: the closed-form 3x3 inverse, then warp_affine's - ``affine`` - or warp_perspective's normalise / invert chain)."""
    Mc = M.detach().to(torch.float32).reshape(-1, 3, 3).contiguous()
    B = Mc.shape[0]
    m = torch.empty(B, 9, device=Mc.device, dtype=torch.float32)
    N.launch("km_inverse_chain_fwd", Mc.device, Mc.data_ptr(), 2 if affine else 3, m.data_ptr(), B, int(height), int(width))
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
    dt = image.dtype if image is not None else image_dtype
    if dt not in NATIVE_DTYPES:
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
    N.launch("km_warp2d_pair_fwd", dev, N.ptr(x), N.ptr(out), mk.data_ptr(), mout.data_ptr(), m.data_ptr(), N.ptr(flags), B, C, Cm, H, W, 1 if affine else 0,
             interp, pad, int(bool(align_corners)), N.ptr(fill), N.ptr(mfill), N.dtype_code(dt), N.mask_dtype_code(mk.dtype))
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
        N.launch("km_color_params_ws_fwd", dev, bf.data_ptr(), cf.data_ptr(), sf.data_ptr(), hf.data_ptr(), N.ptr(prob), table.data_ptr(), enable.data_ptr(),
                 N.ptr(apply), gray_ws.data_ptr(), B)
        return color_jitter_from_table(input, table, enable, apply, order, gray_ws)
    enable = torch.stack([(bf != 0).any(), (cf != 1).any(), (sf != 1).any(), (hf != 0).any()])
    return _color_jitter(input, bf, cf, sf, hf, order, enable=enable, apply=_apply_mask(params, dev))


def random_gaussian_blur(input: torch.Tensor, params: Mapping[str, Any], kernel_size=(5, 5), border_type: str = "reflect",
                         separable: bool = True) -> torch.Tensor:
    """RandomGaussianBlur.apply_transform (gaussian_blur.py:95-114): per-sample ``sigma`` (B,), same in both directions."""
    N.require_device(input, "input")
    sigma1 = _p(params, "sigma", input.device)
    if separable and input.dtype in NATIVE_DTYPES and sigma1.dim() == 1:
        # taps in float32 from the float32 sigma (the reference rounds sigma to the image dtype first), rounded to the image dtype inside the
        # same launch - filter2d_separable's cast of any kernel (kornia/filters/filter.py:126) - and handed to the fused filter as they are
        ky, kx = _kernel_hw(kernel_size)
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
