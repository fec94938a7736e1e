"""The container of the layer: :class:`AugmentationSequential` for one image tensor and any number of label masks - the whole pipeline's draws
in one host buffer and one copy, one walk over the children (a slice-mode crop and the flips after it as one launch), replay and ``inverse()``.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional, Sequence

import torch

from .. import _native as N
from .base import _GeometricOp, _RandomOp
from .crop_flip import RandomResizedCrop, _RandomFlip
from .draws import _Draws, single_allocation
from .functional import NATIVE_DTYPES

ParamItem = namedtuple("ParamItem", ["name", "data"])  # (module name, parameter dictionary): what ``AugmentationSequential._params`` holds
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
                                          "RandomResizedCrop, RandomHorizontalFlip, RandomVerticalFlip, ColorJitter, RandomGaussianBlur, RandomMedianBlur)")
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
            sw, bits = f._flip_switch(f._begin_call(params[j].data, x.device, own), x.device)
            flips[0 if f._AXIS_BIT == 1 else 1] = sw
            flips[2] |= bits
        x, masks = self._kids[i][1]._forward_masks(x, masks, params[i].data, own, image_dtype, tuple(flips))
        return x, masks, group[-1] + 1

    def _can_fuse(self, i: int, x: torch.Tensor) -> bool:
        return i in self._fusion and not (torch.is_grad_enabled() and x.requires_grad) and x.dtype in NATIVE_DTYPES

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
            buf = single_allocation((v for it in params for v in it.data.values()), subclasses=False, contiguous_only=False, at_least=1)
            if buf is not None:
                dev = buf.to(input.device, non_blocking=True)
                for _, m in children:
                    m._st["host_buf"] = buf
                    m._dev_buf = dev
                own = True
        return params, own

    def _split(self, args, keys):
        """(image, [masks], mask_dtype, unbatched) from the call's tensors in ``keys`` order, masks checked against the image and made 4-D.
        ``mask_dtype`` - the reference's: the LAST mask's - is the dtype every mask comes back in; a mask of another dtype is cast to the image
        dtype here, once, so that its round trip is the reference's."""
        if len(args) != len(keys):
            raise NotImplementedError(f"{len(args)} inputs for data_keys={keys}; {_MASK_REFUSED}")
        for a in args:
            if not isinstance(a, torch.Tensor):
                raise NotImplementedError(f"inputs must be tensors, got {type(a).__name__}; {_MASK_REFUSED}")
        img = args[keys.index("input")]
        N.require_device(img, "input")
        if img.dim() not in (3, 4):
            raise ValueError(f"expected a (B, C, H, W) or (C, H, W) image tensor, got {tuple(img.shape)}")
        unbatched = img.dim() == 3
        x = img.unsqueeze(0) if unbatched else img
        masks = []
        for a, k in zip(args, keys):
            if k != "mask":
                continue
            N.require_device(a, "mask")
            mk = a.unsqueeze(0) if (a.dim() == 3 and unbatched) else a
            if mk.dim() != 4 or mk.shape[0] != x.shape[0] or mk.shape[-2:] != x.shape[-2:]:
                raise ValueError(f"a mask must be (B, Cm, H, W) with the image's B, H and W {tuple(x.shape)} (or (Cm, H, W) with a (C, H, W) image), "
                                 f"got {tuple(a.shape)}")
            N.mask_dtype_code(mk.dtype)
            masks.append(mk)
        mask_dtype = masks[-1].dtype if masks else None
        return x, [mk if mk.dtype == mask_dtype else mk.to(x.dtype) for mk in masks], mask_dtype, unbatched

    @staticmethod
    def _pack(x: torch.Tensor, masks: list, keys, mask_dtype, keep: bool):
        """The call's result in ``keys`` order, masks in ``mask_dtype``; ``keep``: without the batch dimension (a (C, H, W) image came without)."""
        if not masks:
            return x[0] if keep else x
        outs, it = [], iter(masks)
        for k in keys:
            t = x if k == "input" else next(it)
            t = t if (k == "input" or t.dtype == mask_dtype) else t.to(mask_dtype)
            outs.append(t[0] if keep else t)
        return tuple(outs)

    def _check_masks(self, keys) -> None:
        if "mask" in keys and not any(isinstance(m, _GeometricOp) for _, m in self._kids):
            # (a mask pipeline without a geometric child would only cast the masks there and back)
            raise NotImplementedError("masks go with a geometric child (RandomAffine, RandomPerspective); this pipeline has none")

    def forward(self, *args: torch.Tensor, params: Optional[Sequence[ParamItem]] = None, data_keys=None):
        keys = self._keys if data_keys is None else self._parse_keys(data_keys)
        if data_keys is not None:
            self._check_masks(keys)
        if len(args) == 2 and keys == ["input"] and (args[1] is None or isinstance(args[1], (list, tuple))):
            args, params = args[:1], args[1]  # (the image-only signature forward(input, params))
        children = self._kids
        x, masks, mask_dtype, unbatched = self._split(args, keys)
        params, own = self._prepare(x, params)
        image_dtype = x.dtype
        i = 0
        while i < len(children):  # THE walk: a fusion group or one child at a time, with or without masks
            if self._can_fuse(i, x):
                x, masks, i = self._fused(i, x, masks, params, own, image_dtype)
            else:
                x, masks = children[i][1]._forward_masks(x, masks, params[i].data, own, image_dtype)
                i += 1
        object.__setattr__(self, "_params", [ParamItem(name, m._params) for name, m in children])
        # a (C, H, W) image comes back without a batch dimension when the children keep it so: EVERY child where each child's own ``forward``
        # used to decide (no mask, no fusion group), ANY child elsewhere - as it has been
        keep = unbatched and (any if (masks or self._fusion) else all)(m.keepdim for _, m in children)
        return self._pack(x, masks, keys, mask_dtype, keep)

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
        x, masks, mask_dtype, unbatched = self._split(args, keys)
        image_dtype = x.dtype
        for (_, m), item in zip(reversed(self._kids), reversed(params)):
            x, masks = m._inverse_masks(x, masks, item.data, image_dtype)
        return self._pack(x, masks, keys, mask_dtype, unbatched and any(m.keepdim for _, m in self._kids))
