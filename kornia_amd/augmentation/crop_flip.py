"""The crop / flip family of the geometric modules: RandomResizedCrop and the two random flips on the batched crop -> resize (-> flip) kernel
(``km_crop_resize_fwd``, :func:`kornia_amd.geometry.transform.crop2d.crop_resize`).  Flips right after a slice-mode crop ride in its launch
(the container plans that), and children after a crop sample at its size.
"""
from __future__ import annotations

from typing import Any, Mapping, Optional, Tuple

import torch

from ..geometry.transform.builders import get_perspective_transform
from ..geometry.transform.crop2d import crop_by_indices, crop_by_transform_mat, crop_resize
from ..geometry.transform.imgwarp import warp_affine
from .base import _GeometricOp, fan_out
from .draws import _Draws
from .functional import NATIVE_DTYPES, _apply_mask, _p, select_samples


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

    def _crop(self, x: Optional[torch.Tensor], mask: Optional[torch.Tensor], p: Mapping[str, Any], image_dtype: torch.dtype, flips=(None, None, 0)):
        """The pair launch of the module: (image or None, mask or None) -> (image_out, mask_out)."""
        raise NotImplementedError

    def _run(self, x: torch.Tensor, masks: list, p: Mapping[str, Any], image_dtype: torch.dtype, flips=(None, None, 0)):
        if x.dtype not in NATIVE_DTYPES:
            raise TypeError(f"{type(self).__name__}: the native crop / flip takes float32 / bfloat16 / float16 images, got {x.dtype}")
        return fan_out(lambda im, mk: self._crop(im, mk, p, image_dtype, flips), x, masks)

    def _forward_masks(self, x: torch.Tensor, masks: list, params: Mapping[str, Any], own: bool, image_dtype: torch.dtype, flips=(None, None, 0)):
        p = self._begin_call(params, x.device, own)
        if torch.is_grad_enabled() and x.requires_grad:  # the image through the differentiable composition, the masks through the kernel
            return self._apply(x, p), (self._run(x.detach(), masks, p, image_dtype)[1] if masks else masks)
        return self._run(x, masks, p, image_dtype, flips)


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

    def _flip_switch(self, p: Mapping[str, Any], device):
        """(switch, bits): this flip's per-sample switch for the launch - its device ``batch_prob`` (thresholded in the launch) - or, when every
        sample flips, None and the axis bit."""
        if p.get("batch_prob") is None:
            return None, self._AXIS_BIT
        return _p(p, "batch_prob", device), 0

    def _sample(self, d: _Draws, shape, params: dict) -> None:
        return None  # (the probability draw is all a flip samples)

    def _crop(self, x, mask, p, image_dtype, flips=(None, None, 0)):
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
