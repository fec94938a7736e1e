"""crop_by_transform_mat / crop_by_boxes / crop_and_resize / center_crop on the native warps.

Reference behaviour mirrored: kornia/geometry/transform/crop2d.py:41-124 (crop_and_resize), :125-208 (center_crop),
:209-298 (crop_by_boxes), :299-404 (crop_by_transform_mat); box size from kornia/geometry/bbox.py infer_bbox_shape
(``x1 - x0 + 1``, ``y2 - y0 + 1``); crop_by_indices (:405-500) is the batched native crop -> resize ``km_crop_resize_fwd``.  Boxes are four ``(x, y)`` corners in the order top-left, top-right, bottom-right,
bottom-left.  The homography is ``get_perspective_transform`` (one launch on HIP tensors), the resampling is
``warp_perspective`` / ``warp_affine``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .builders import get_perspective_transform
from .imgwarp import warp_affine, warp_perspective

__all__ = ["center_crop", "crop_and_resize", "crop_by_boxes", "crop_by_indices", "crop_by_transform_mat", "crop_resize"]


def crop_by_transform_mat(input_tensor: torch.Tensor, transform: torch.Tensor, out_size: Tuple[int, int], mode: str = "bilinear",
                          padding_mode: str = "zeros", align_corners: bool = True) -> torch.Tensor:
    """Crop with a source->destination transform: ``(B,2,3)`` takes ``warp_affine``, ``(B,3,3)`` ``warp_perspective``
    (with the destination-side reparametrisation the reference applies for ``align_corners=False``)."""
    T = transform.expand(input_tensor.shape[0], -1, -1).to(device=input_tensor.device, dtype=input_tensor.dtype)
    if transform.shape[-2:] == (2, 3):
        return warp_affine(input_tensor, T, out_size, mode=mode, padding_mode=padding_mode, align_corners=align_corners)
    h_out, w_out = out_size
    if not align_corners and (h_out == 1 or w_out == 1):
        return warp_affine(input_tensor, T[:, :2, :], out_size, mode=mode, padding_mode=padding_mode, align_corners=align_corners)
    if not align_corners:
        corr = torch.tensor([[w_out / (w_out - 1.0), 0.0, -0.5], [0.0, h_out / (h_out - 1.0), -0.5], [0.0, 0.0, 1.0]],
                            device=T.device, dtype=T.dtype)
        T = corr.unsqueeze(0) @ T
    return warp_perspective(input_tensor, T, out_size, mode=mode, padding_mode=padding_mode, align_corners=align_corners)


def crop_by_boxes(input_tensor: torch.Tensor, src_box: torch.Tensor, dst_box: torch.Tensor, mode: str = "bilinear",
                  padding_mode: str = "zeros", align_corners: bool = True, validate_boxes: bool = True) -> torch.Tensor:
    """Warp the quadrilaterals ``src_box`` (B,4,2) onto the axis-aligned ``dst_box`` (B,4,2); all crops of a batch share one size."""
    if input_tensor.dim() != 4:
        raise AssertionError(f"Only torch.Tensor with shape (B, C, H, W) supported. Got {input_tensor.shape}.")
    dst_trans_src = get_perspective_transform(src_box.to(input_tensor), dst_box.to(input_tensor))
    widths = dst_box[:, 1, 0] - dst_box[:, 0, 0] + 1
    heights = dst_box[:, 2, 1] - dst_box[:, 0, 1] + 1
    if not ((heights == heights[0]).all() and (widths == widths[0]).all()):
        raise AssertionError(f"Cropping height, width and depth must be exact same in a batch. Got height {heights} and width {widths}.")
    return crop_by_transform_mat(input_tensor, dst_trans_src, (int(heights[0].item()), int(widths[0].item())), mode=mode,
                                 padding_mode=padding_mode, align_corners=align_corners)


def _dst_box(size, like: torch.Tensor, n: int) -> torch.Tensor:
    dst_h, dst_w = size
    return torch.tensor([[[0, 0], [dst_w - 1, 0], [dst_w - 1, dst_h - 1], [0, dst_h - 1]]], device=like.device,
                        dtype=like.dtype).expand(n, -1, -1)


def _check_crop_args(input_tensor, size):
    if not isinstance(input_tensor, torch.Tensor):
        raise TypeError(f"Input torch.tensor type is not a torch.Tensor. Got {type(input_tensor)}")
    if not isinstance(size, (tuple, list)) or len(size) != 2:
        raise ValueError(f"Input size must be a tuple/list of length 2. Got {size}")
    if input_tensor.dim() != 4:
        raise AssertionError(f"Only torch.Tensor with shape (B, C, H, W) supported. Got {input_tensor.shape}.")


def crop_and_resize(input_tensor: torch.Tensor, boxes: torch.Tensor, size: Tuple[int, int], mode: str = "bilinear",
                    padding_mode: str = "zeros", align_corners: bool = True) -> torch.Tensor:
    """Extract the quadrilaterals ``boxes`` (B,4,2) and resample each to ``size`` = (h, w)."""
    _check_crop_args(input_tensor, size)
    if not isinstance(boxes, torch.Tensor):
        raise TypeError(f"Input boxes type is not a torch.Tensor. Got {type(boxes)}")
    points_src = boxes.to(input_tensor)
    return crop_by_boxes(input_tensor, points_src, _dst_box(size, input_tensor, points_src.shape[0]), mode, padding_mode, align_corners)


def center_crop(input_tensor: torch.Tensor, size: Tuple[int, int], mode: str = "bilinear", padding_mode: str = "zeros",
                align_corners: bool = True) -> torch.Tensor:
    """Crop the centred ``size`` = (h, w) window."""
    _check_crop_args(input_tensor, size)
    dst_h, dst_w = size
    src_h, src_w = input_tensor.shape[-2:]
    start_x, start_y = src_w / 2 - dst_w / 2, src_h / 2 - dst_h / 2
    end_x, end_y = start_x + dst_w - 1, start_y + dst_h - 1
    points_src = torch.tensor([[[start_x, start_y], [end_x, start_y], [end_x, end_y], [start_x, end_y]]],
                              device=input_tensor.device, dtype=input_tensor.dtype)
    return crop_by_boxes(input_tensor, points_src, _dst_box(size, input_tensor, 1), mode, padding_mode, align_corners)


_CROP_RESIZE, _CROP_PAD = 0, 1


def crop_resize(image, mask, src, size, interpolation: str = "bilinear", align_corners: bool = False, compensation: str = "resize",
                flip_x=None, flip_y=None, flip_all: int = 0, image_dtype=None):
    """The native batched crop -> resize (-> flip) of an image and its first label mask in one launch (``km_crop_resize_fwd``, forward only).

    ``image`` (B,C,H,W) float32 / bfloat16 / float16 or None; ``mask`` (B,Cm,H,W) label mask or None (always nearest, through the image dtype and
    back - ``image_dtype`` names it when ``image`` is None); ``src`` (B,4,2) corners as :func:`crop_by_indices` reads them (a device tensor is
    not read back), or None for the whole image (``size`` must then be (H, W): a pure flip); ``flip_x`` / ``flip_y`` (B,) float switches
    (mirror where > 0.5) or None; ``flip_all`` bit 0 / 1: mirror every sample in x / y.  Returns ``(image_out or None, mask_out or None)``."""
    from ... import _native as N

    ref = image if image is not None else mask
    N.require_device(ref, "input")
    dev = ref.device
    dt = image.dtype if image is not None else image_dtype
    if dt not in (torch.float32, torch.bfloat16, torch.float16):
        raise TypeError(f"the native crop takes float32 / bfloat16 / float16 images, got {dt}")
    B, _, H, W = ref.shape
    oh, ow = int(size[0]), int(size[1])
    if interpolation not in ("bilinear", "nearest"):
        raise NotImplementedError(f"interpolation={interpolation!r}: the native crop resizes 'bilinear' or 'nearest'")
    x = image.detach().contiguous() if image is not None else None
    mk = mask.detach().contiguous() if mask is not None else None
    for t, name in ((x, "image"), (mk, "mask")):
        if t is not None and (t.dim() != 4 or t.shape[0] != B or tuple(t.shape[-2:]) != (H, W) or t.device != dev):
            raise ValueError(f"{name} {tuple(t.shape)} does not match {tuple(ref.shape)}")
    s = None
    if src is not None:
        s = src.detach().to(device=dev, dtype=torch.float32).contiguous()
        if tuple(s.shape) != (B, 4, 2):
            raise ValueError(f"src_box must be (B, 4, 2) = ({B}, 4, 2), got {tuple(s.shape)}")
    elif (oh, ow) != (H, W):
        raise ValueError("without boxes the output size is the image's")
    fx = None if flip_x is None else flip_x.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    fy = None if flip_y is None else flip_y.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    for f in (fx, fy):
        if f is not None and f.numel() != B:
            raise ValueError(f"a flip switch has {f.numel()} entries, expected the batch size {B}")
    out = torch.empty(B, x.shape[1], oh, ow, device=dev, dtype=x.dtype) if x is not None else None
    mout = torch.empty(B, mk.shape[1], oh, ow, device=dev, dtype=mk.dtype) if mk is not None else None
    N.launch("km_crop_resize_fwd", dev, N.ptr(x), N.ptr(out), N.ptr(mk), N.ptr(mout), N.ptr(s), N.ptr(fx), N.ptr(fy), int(flip_all), B,
             x.shape[1] if x is not None else 0, mk.shape[1] if mk is not None else 0, H, W, oh, ow, 1 if interpolation == "bilinear" else 0,
             _CROP_RESIZE if compensation == "resize" else _CROP_PAD, int(bool(align_corners)), N.dtype_code(dt),
             N.mask_dtype_code(mk.dtype) if mk is not None else 0)
    return out, mout


def _box_windows(src: torch.Tensor):
    """The reference's integer windows (x1, x2, y1, y2) of (B,4,2) corners, as host lists (reads device boxes back)."""
    s = torch.as_tensor(src).detach().to(torch.long).cpu()
    return s[:, 0, 0].tolist(), (s[:, 1, 0] + 1).tolist(), s[:, 0, 1].tolist(), (s[:, 3, 1] + 1).tolist()


def crop_by_indices(input_tensor: torch.Tensor, src_box: torch.Tensor, size: Optional[Tuple[int, int]] = None, interpolation: str = "bilinear",
                    align_corners: Optional[bool] = None, antialias: bool = False, shape_compensation: str = "resize") -> torch.Tensor:
    """Crop every sample's integer window out of ``input_tensor`` (B,C,H,W) and bring it to ``size`` = (h, w): kornia's crop_by_indices
    (crop2d.py:405-500), the whole batch in ONE launch (``km_crop_resize_fwd``) instead of a host read-back of the boxes and a slice +
    ``F.interpolate`` per sample.

    ``src_box`` (B,4,2) corners (x, y) top-left, top-right, bottom-right, bottom-left, on the host or on the device; the window of sample b is
    ``[y1, y2) x [x1, x2)`` with ``x1 = (long)src[b,0,0]``, ``x2 = (long)src[b,1,0] + 1``, ``y1 = (long)src[b,0,1]``, ``y2 = (long)src[b,3,1] + 1``,
    clamped to the image as Python slicing clamps it.  A window of the output size is copied; another one is resized (``shape_compensation``
    "resize": ``F.interpolate`` with ``interpolation`` "bilinear" / "nearest" and ``align_corners``) or zero-padded / cut at the bottom and
    right ("pad"); when every box of the batch is the same the window is resized whatever ``shape_compensation`` says, as in the reference.
    ``size=None`` takes the boxes' common size - the one case that reads device boxes back (ValueError when they differ).  Device boxes are
    not otherwise validated: a window outside the image is empty and gives zeros (the reference fails in ``F.interpolate`` there).
    ``antialias=True`` raises NotImplementedError.  Under autograd (an input that requires grad) the result is the differentiable
    per-sample composition: slice -> :func:`resize_bilinear` / ``F.interpolate(mode="nearest")`` -> ``torch.cat``."""
    from ...core.check import KORNIA_CHECK_SHAPE
    from .pyramid import resize_bilinear

    KORNIA_CHECK_SHAPE(input_tensor, ["B", "C", "H", "W"])
    KORNIA_CHECK_SHAPE(src_box, ["B", "4", "2"])
    if antialias:
        raise NotImplementedError("crop_by_indices: antialias=True (a Gaussian blur before downscaling) is not implemented on the native path")
    interpolation = str(interpolation).lower()
    if interpolation not in ("bilinear", "nearest"):
        raise NotImplementedError(f"crop_by_indices: interpolation={interpolation!r} - the native path resizes 'bilinear' or 'nearest'")
    if interpolation == "nearest" and align_corners is not None:
        raise ValueError("align_corners option can only be set with the interpolating modes: linear | bilinear | bicubic | trilinear")
    B, C, H, W = input_tensor.shape
    if size is None:
        s = torch.as_tensor(src_box).detach().to(torch.long).cpu()
        h, w = s[:, 2, 1] - s[:, 0, 1] + 1, s[:, 1, 0] - s[:, 0, 0] + 1  # (infer_bbox_shape, kornia/geometry/bbox.py:140-142)
        if B > 0 and bool(((h != h[0]).any() | (w != w[0]).any())):
            raise ValueError("All boxes in the batch must have the same height and width when `size` is None. "
                             "Please pass `size` explicitly when box dimensions vary across the batch.")
        size = (int(h[0]), int(w[0])) if B > 0 else (0, 0)
    oh, ow = int(size[0]), int(size[1])
    if oh < 0 or ow < 0:
        raise RuntimeError(f"Trying to create tensor with negative dimension: size={tuple(size)}")
    if B == 0 or oh == 0 or ow == 0:
        return input_tensor.new_empty(B, C, oh, ow)
    align = bool(align_corners) if align_corners is not None else False
    if torch.is_grad_enabled() and input_tensor.requires_grad:
        x1, x2, y1, y2 = _box_windows(src_box)
        same = all(v.count(v[0]) == B for v in (x1, x2, y1, y2))
        outs = []
        for i in range(B):
            win = input_tensor[i:i + 1, :, y1[i]:y2[i], x1[i]:x2[i]]
            if tuple(win.shape[-2:]) == (oh, ow):
                outs.append(win)
            elif shape_compensation == "resize" or same:
                outs.append(resize_bilinear(win, (oh, ow), align) if interpolation == "bilinear"
                            else torch.nn.functional.interpolate(win, size=(oh, ow), mode="nearest"))
            else:
                outs.append(torch.nn.functional.pad(win, [0, ow - win.shape[-1], 0, oh - win.shape[-2]]))
        return torch.cat(outs, 0)
    return crop_resize(input_tensor, None, src_box, (oh, ow), interpolation, align, "resize" if shape_compensation == "resize" else "pad")[0]
