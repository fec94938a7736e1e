"""What every module of the layer shares: :class:`_RandomOp` - p / same_on_batch / keepdim, the probability draw, one host buffer -> one device
copy, replay, how a call begins, and the two calls the container makes of a child (``_forward_masks``, ``_inverse_masks``) -, the one
mask fan-out (:func:`fan_out`) and the base of the geometric modules (:class:`_GeometricOp`).  The design note is in :mod:`.modules`.
"""
from __future__ import annotations

from typing import Any, Callable, Mapping, Optional

import torch

from .. import _native as N
from .draws import _Draws, device_views, single_allocation


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
        float tensors of ``params`` are pieces of it); foreign parameters (a replay) go tensor by tensor, as the entry functions take them."""
        out = dict(params)
        buf = self._host_buf if own else None
        dev = self._dev_buf if own else None
        if buf is None:
            # a replay: host float tensors that are pieces of ONE allocation (this package's own `_params` are) cross as one copy too
            buf, dev = single_allocation(params.values(), subclasses=True, contiguous_only=True, at_least=2), None
        if buf is not None:
            if dev is None:
                dev = buf.to(device, non_blocking=True)
            device_views(self._st, "layout" if own else "layout_replay", params, buf, dev, out)
        if self.p >= 1.0 and self.p_batch >= 1.0:
            out["batch_prob"] = None  # every sample is transformed: no switch in the launches at all
        return out

    def _begin_call(self, params: Mapping[str, Any], device, own: bool) -> dict:
        """What every call of the module starts with, whoever makes it (``forward``, the container's walk, a fused launch): the state the call
        leaves - ``_params``, the device, no host buffer unless the draw is this module's own - and the parameters for the device."""
        st = self._st
        if not own:
            st["host_buf"] = None
        st["params"] = dict(params)
        st["device"] = device
        return self._device_params(st["params"], device, own)

    def forward(self, input: torch.Tensor, params: Optional[Mapping[str, Any]] = None, _own: bool = False) -> torch.Tensor:
        N.require_device(input, "input")
        if input.dim() not in (3, 4):
            raise ValueError(f"expected a (B, C, H, W) or (C, H, W) image tensor, got {tuple(input.shape)}")
        x = input.unsqueeze(0) if input.dim() == 3 else input
        own = params is None or _own  # (_own: the container sampled these through this module's forward_parameters a moment ago)
        if params is None:
            params = self.forward_parameters(x.shape)
        out = self._apply(x, self._begin_call(params, x.device, own))
        return out[0] if (input.dim() == 3 and self.keepdim) else out

    # The two calls the container makes of every child: x (B,C,H,W) and masks [(B,Cm,H,W)] -> (x', masks').
    def _forward_masks(self, x: torch.Tensor, masks: list, params: Mapping[str, Any], own: bool, image_dtype: torch.dtype):
        """The image as ``forward`` transforms it; an intensity module leaves masks alone."""
        return self._apply(x, self._begin_call(params, x.device, own)), masks

    def _inverse_masks(self, x: torch.Tensor, masks: list, params: Mapping[str, Any], image_dtype: torch.dtype):
        """An intensity module's inverse is the identity."""
        return x, masks


def fan_out(pair: Callable, x: torch.Tensor, masks: list, image: bool = True):
    """An image and its masks through ``pair(image or None, mask or None) -> (image_out, mask_out)``: the image (unless ``image`` is False: it
    was transformed elsewhere) and the first mask in ONE launch, every further mask in a mask-only launch, no mask: the image alone."""
    out, res = x, []
    for k, mk in enumerate(masks):
        o, mo = pair(x if (image and k == 0) else None, mk)
        if image and k == 0:
            out = o
        res.append(mo)
    if image and not masks:
        out, _ = pair(x, None)
    return out, res


class _GeometricOp(_RandomOp):
    """A geometric module: it transforms label masks with the image's draw (nearest, through the image dtype and back,
    kornia/augmentation/container/augment.py:596-618), has an ``inverse()`` and a ``transform_matrix``.  Two families: the matrix chain
    (:class:`_MatrixChainOp`) and crop / flip (:mod:`.crop_flip`); each brings ``_forward_masks``, ``_inverse_masks`` and ``transform_matrix``."""

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
