"""The modules: BASELINE config 3 AS IT IS WRITTEN - ``AugmentationSequential(RandomAffine(...), ColorJitter(...),
RandomGaussianBlur(...))(x)`` - with the PARAMETER SAMPLING inside the call.

The functions of :mod:`.functional` take parameter dictionaries somebody else sampled; on a machine without Kornia (the GPU box of this project: the
reference tree may not travel) that left config 3's public spelling without an implementation and its sampling - which SURVEY.md 8(f) calls
the real wall time of the layer - outside every timing.  These classes are the missing half, written against the behaviour of
kornia/augmentation/base.py:179-272 (``__batch_prob_generator__``, ``forward_parameters``), random_generator/_2d/affine.py:161-213,
random_generator/_2d/color_jitter.py:97-110, random_generator/_2d/gaussian_blur.py:75-79 and container/augment.py:431-500:

  * the draws come from torch's GLOBAL CPU generator in the reference's order - batch_prob first (only for 0 < p < 1), then each quantity as
    ``low + torch.rand(n) * (high - low)`` in float32 (torch.distributions.Uniform.rsample), a degenerate range still consuming its draw,
    ``torch.randperm(4)`` last for the colour order - so ``torch.manual_seed(s)`` followed by the same pipeline gives THE SAME parameters as
    Kornia does (tests/golden/aug_modules.npz: the reference's ``_params`` for seeded calls, compared entry for entry);
  * a module's draws land in ONE host buffer and cross to the device as ONE copy (the reference moves every parameter tensor on its own);
    ``_params`` exposes host views with the reference's keys, so a replay through Kornia - or of Kornia's through this - works;
  * the apply step is the functions of :mod:`.functional`: the per-sample probability switch inside the launches, no blend pass, no host synchronisation.
Beyond config 3: RandomPerspective, label masks in the container (``data_keys`` with "mask" entries) and ``inverse()``; keypoints, boxes,
dictionaries, lists of masks and ``random_apply`` still raise.  RandomResizedCrop and the two random flips run on the batched crop kernel
(``km_crop_resize_fwd``); flips right after a slice-mode crop ride in its launch, and children after a crop sample at its size.

This file holds the matrix-chain family (RandomAffine, RandomPerspective) and the three intensity modules; what every module shares is in
:mod:`.base`, the crop / flip family in :mod:`.crop_flip`, the container in :mod:`.container`.
"""
from __future__ import annotations

from typing import Any, Mapping, Optional, Sequence

import torch

from .base import _GeometricOp, _RandomOp, fan_out
from .draws import _Draws, _range_pair
from .functional import (NATIVE_DTYPES, _kernel_hw, _prob, affine_chain, color_jitter, inverse_chain, perspective_chain, random_affine,
                         random_gaussian_blur, random_perspective, warp_pair)


class _MatrixChainOp(_GeometricOp):
    """What RandomAffine and RandomPerspective share beyond the draws: the parameters -> (m, M, apply) chain, label masks warped with the
    image's draw (``km_warp2d_pair_fwd``), the inverse warp (``km_inverse_chain_fwd`` + the same pair launch) and ``transform_matrix``."""

    _AFFINE = True  # the warp's coordinate generator: affine or perspective
    # _chain(params, device, H, W, with_matrix=False) -> (m, M, apply): the family's parameters -> matrix launch (affine_chain / perspective_chain)

    def _warp_with_masks(self, x: torch.Tensor, masks: list, m: torch.Tensor, apply, image_dtype: torch.dtype, image=True):
        """:func:`fan_out` of the pair launch (``km_warp2d_pair_fwd``) on one matrix and switch; with no mask, the image with an empty one."""
        kw = dict(affine=self._AFFINE, resample=self.resample, padding_mode=self.padding_mode, align_corners=self.align_corners,
                  fill_value=self.fill_value, apply=apply, image_dtype=image_dtype)

        def pair(im, mk):
            return warp_pair(im, mk if mk is not None else x.new_empty((x.shape[0], 0, x.shape[2], x.shape[3]), dtype=torch.uint8), m, **kw)

        return fan_out(pair, x, masks, image)

    def _forward_masks(self, x: torch.Tensor, masks: list, params: Mapping[str, Any], own: bool, image_dtype: torch.dtype):
        p = self._begin_call(params, x.device, own)
        if not masks:
            # the image alone goes the way ``forward`` takes it (``_apply``: RandomAffine's chain + plain / masked warp launch, not the pair
            # launch below), so that a pipeline without masks makes the native calls it always made
            return self._apply(x, p), masks
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


class RandomAffine(_MatrixChainOp):
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

    _chain = staticmethod(affine_chain)


class RandomPerspective(_MatrixChainOp):
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
        if x.dim() == 4 and x.dtype in NATIVE_DTYPES and not (torch.is_grad_enabled() and x.requires_grad):
            B, C, H, W = x.shape
            m, _, apply = perspective_chain(params, x.device, H, W)
            return self._warp_with_masks(x, [], m, apply, x.dtype)[0]
        return random_perspective(x, params, self.resample, self.align_corners)

    _chain = staticmethod(perspective_chain)


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
        self.kernel_size = _kernel_hw(kernel_size)
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


class RandomMedianBlur(_RandomOp):
    """``kornia.augmentation.RandomMedianBlur`` (kornia/augmentation/_2d/intensity/median_blur.py:26-68): it draws ``batch_prob`` only; the
    median filter and the per-sample switch are ONE launch (``km_median_blur_fwd`` copies the samples whose draw failed), differentiable."""

    def __init__(self, kernel_size=(3, 3), same_on_batch: bool = False, p: float = 0.5, keepdim: bool = False) -> None:
        super().__init__(p, same_on_batch, keepdim)
        self.kernel_size = _kernel_hw(kernel_size)

    def _sample(self, d: _Draws, shape, params: dict) -> None:
        pass  # (no parameter beyond the probability draw)

    def _apply(self, x: torch.Tensor, params: dict) -> torch.Tensor:
        from ..filters.median import _median_blur

        return _median_blur(x, self.kernel_size, _prob(params, x.device, x.shape[0]))
