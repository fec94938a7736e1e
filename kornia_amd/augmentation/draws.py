"""The host side of a call's random draws: one (pinned) buffer per call, handed out in pieces and copied to the device ONCE, and the device
views of those pieces.

A module's - or a whole container's - float parameters are contiguous pieces of one host allocation (:class:`_Draws`), so they cross to the
device as one copy and each parameter becomes an ``as_strided`` view of the device buffer (:func:`device_views`).  A replay of such parameters
is recognised by :func:`single_allocation` and takes the same route.
"""
from __future__ import annotations

from typing import Any, Iterable, Mapping, Optional

import torch


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


def single_allocation(values: Iterable[Any], *, subclasses: bool, contiguous_only: bool, at_least: int) -> Optional[torch.Tensor]:
    """The host float32 buffer that ``values`` are pieces of - a 1-D view of the whole allocation - or None when they are not pieces of ONE
    allocation.  Only non-empty float32 CPU tensors count (plain ``torch.Tensor`` alone unless ``subclasses``; only contiguous ones with
    ``contiguous_only``, the others are passed over); fewer than ``at_least`` of them is None too.  The two callers keep the inputs each has
    always accepted: a module's replay (``_RandomOp._device_params``) counts subclasses, contiguous pieces only and wants two at least; the
    container's (``AugmentationSequential._prepare``) counts plain tensors of any stride and is content with one."""
    store, n = None, 0
    for v in values:
        if not (isinstance(v, torch.Tensor) if subclasses else type(v) is torch.Tensor):
            continue
        if v.dtype is not torch.float32 or v.device.type != "cpu" or not v.numel() or (contiguous_only and not v.is_contiguous()):
            continue
        if store is None:
            store = v.untyped_storage()
        elif v.untyped_storage().data_ptr() != store.data_ptr():
            return None
        n += 1
    if n < at_least:
        return None
    return torch.empty(0, dtype=torch.float32).set_(store)


def device_views(cache: dict, key: str, params: Mapping[str, Any], buf: torch.Tensor, dev: torch.Tensor, out: dict) -> None:
    """``out[k]`` = the device-side view (of ``dev``, the copy of the host buffer ``buf``) of every float tensor of ``params`` that is a piece
    of ``buf``.  Where the pieces sit is the same for every call of a module at one batch size (they are handed out in a fixed order): found
    once, kept in ``cache[key]``, checked by (key, address offset) since, and each view made by ONE as_strided (a slice + a view per tensor
    were 30 us of a call whose host share bounds it: profiles/r06/run20_*)."""
    base = buf.data_ptr()
    lay = cache.get(key)
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
        lay = cache[key] = (buf.numel(), found)
    for k, off, shape, strides in lay[1]:
        out[k] = dev.as_strided(shape, strides, off)
