"""median_blur / MedianBlur on the native kernels (csrc/km_median.hip).

Reference: kornia/filters/median.py:35-72 (median_blur: a one-hot ``conv2d`` into a (B C, ky kx, H, W) copy of the image, then
``torch.median`` over it), :75-119 (MedianBlur).  Here one launch reads the image once and writes the result once; the forward is
bit-identical to the reference in float32 / float64 / bfloat16 / float16.

* border: zero padding by (ky // 2, kx // 2); the padding zeros take part in the selection;
* non-finite inputs: for ky * kx >= 2 an output is NaN exactly when its window holds a NaN or +-inf of the image (the reference's
  one-hot convolution multiplies the other taps by 0); 1 x 1 is the identity;
* gradient: ``grad_out`` of a pixel goes to the one window position that supplied the median - among EQUAL values the smallest row-major
  window position (the reference leaves that choice to ATen's sort; forward values do not depend on it).  The forward records the
  position in a uint8 plane only when the input needs a gradient; the backward is a gather through it - no atomics, deterministic;
* windows: odd sides up to 15 x 15; larger ones raise ``NotImplementedError`` (no ATen fallback here; under ``patch()`` they stay on
  Kornia's own function).
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from .. import _native as N
from ..core.check import KORNIA_CHECK_IS_TENSOR, KORNIA_CHECK_SHAPE
from .kernels import _unpack_2d_ks

__all__ = ["MedianBlur", "median_blur"]

MAX_KERNEL_SIDE = 15


def _launch_fwd(xc: torch.Tensor, ky: int, kx: int, apply: Optional[torch.Tensor], with_idx: bool):
    B, C, H, W = xc.shape
    out = torch.empty_like(xc)
    idx = torch.empty((B, C, H, W), device=xc.device, dtype=torch.uint8) if with_idx else None
    N.launch("km_median_blur_fwd", xc.device, xc.data_ptr(), out.data_ptr(), N.ptr(idx), N.ptr(apply), B, C, H, W, ky, kx, N.dtype_code(xc.dtype))
    return out, idx


class _MedianBlurFunction(torch.autograd.Function):
    """x (B,C,H,W); apply (B,) float32 on the device or None: samples with apply <= 0.5 pass through (forward and backward)."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, ky: int, kx: int, apply: Optional[torch.Tensor]):
        xc = x.detach().contiguous()
        need = bool(ctx.needs_input_grad[0])
        out, idx = _launch_fwd(xc, ky, kx, apply, need)
        if need:
            ctx.save_for_backward(idx, apply) if apply is not None else ctx.save_for_backward(idx)
        ctx.cfg = (ky, kx, apply is not None)
        return out

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        ky, kx, switched = ctx.cfg
        idx = ctx.saved_tensors[0]
        apply = ctx.saved_tensors[1] if switched else None
        B, C, H, W = idx.shape
        g = gy.detach().contiguous()
        gx = torch.empty_like(g)
        N.launch("km_median_blur_bwd", g.device, g.data_ptr(), idx.data_ptr(), N.ptr(apply), gx.data_ptr(), B, C, H, W, ky, kx, N.dtype_code(g.dtype))
        return gx, None, None, None


def _window(kernel_size) -> tuple:
    ky, kx = _unpack_2d_ks(kernel_size)
    ky, kx = int(ky), int(kx)
    if ky < 1 or kx < 1 or ky % 2 == 0 or kx % 2 == 0:
        # (the reference's `features.view(b, c, ky * kx, h, w)` fails on the even-size convolution's output: RuntimeError there too)
        raise RuntimeError(f"median_blur: kernel_size must be odd and positive in both directions, got ({ky}, {kx})")
    return ky, kx


def supported(kernel_size, dtype: torch.dtype) -> bool:
    """True when the native op takes this window and dtype (odd sides of 1 .. 15; float32 / float64 / bfloat16 / float16)."""
    try:
        ky, kx = _unpack_2d_ks(kernel_size)
        ky, kx = int(ky), int(kx)
    except Exception:
        return False
    return dtype in N._DTYPE_CODES and ky >= 1 and kx >= 1 and ky % 2 == 1 and kx % 2 == 1 and max(ky, kx) <= MAX_KERNEL_SIDE


def _median_blur(input: torch.Tensor, kernel_size, apply: Optional[torch.Tensor]) -> torch.Tensor:
    KORNIA_CHECK_IS_TENSOR(input)
    KORNIA_CHECK_SHAPE(input, ["B", "C", "H", "W"])
    ky, kx = _window(kernel_size)
    if max(ky, kx) > MAX_KERNEL_SIDE:
        raise NotImplementedError(f"median_blur: windows up to {MAX_KERNEL_SIDE} x {MAX_KERNEL_SIDE} are supported, got ({ky}, {kx})")
    N.require_device(input, "input")
    N.dtype_code(input.dtype)
    if not (torch.is_grad_enabled() and input.requires_grad):
        return _launch_fwd(input.detach().contiguous(), ky, kx, apply, False)[0]  # (no autograd node to build)
    return _MedianBlurFunction.apply(input, ky, kx, apply)


def median_blur(input: torch.Tensor, kernel_size) -> torch.Tensor:
    """Median filter over a ``kernel_size`` window (an int or ``(ky, kx)``, odd), zero padding; (B,C,H,W) in, the same shape and dtype out."""
    return _median_blur(input, kernel_size, None)


class MedianBlur(nn.Module):
    """Module form of :func:`median_blur`."""

    def __init__(self, kernel_size) -> None:
        super().__init__()
        self.kernel_size = kernel_size

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        return median_blur(input, self.kernel_size)
