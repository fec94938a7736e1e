"""bilateral_blur / joint_bilateral_blur / BilateralBlur / JointBilateralBlur on the native kernels (csrc/km_bilateral.hip).

Reference: kornia/filters/bilateral.py:32-84 (``_bilateral_blur``: ``F.pad``, two ``unfold`` copies of shape (B, C, H, W, ky kx), about ten
elementwise passes over tensors of that size, two reductions), :87-174 (the two functions), :178-338 (the modules).  Here one launch reads the
image (and the guidance) once and writes the result once; the backward is one launch too.

* what is computed: ``k_qi = s_i exp(coef D_qi)`` with ``D`` the squared l1 or l2 colour distance of the guidance between a tap and the centre,
  ``y_q = sum_i k_qi x(q+i) / sum_i k_qi``; taps go through ``F.pad``'s border rule; nothing is skipped or clamped, so NaN / inf behave as in
  the reference;
* the spatial kernel ``s`` is the package's ``get_gaussian_kernel2d`` (the reference's weights) in the compute type - float32 for float32 /
  bfloat16 / float16 images, float64 for float64 -; ``coef = -0.5 / sigma_color^2``: a float ``sigma_color`` as a host double rounded once to the
  compute type, a ``(B,)`` tensor through torch ops in the input dtype (as the reference forms it);
* 16-bit storage: the float32 arithmetic on the widened input, rounded once;
* gradients wrt ``input`` and ``guidance`` (a gather, no atomics, deterministic).  l1: a tap whose guidance equals the centre's in a channel
  contributes 0 through that channel (``sign(0) = 0``, as ``torch.abs``).  Gradients wrt ``sigma_color`` / ``sigma_space`` are out of scope:
  a sigma tensor that requires a gradient raises ``NotImplementedError``;
* limits: odd window sides up to 15, at most 16 channels of input and of guidance; beyond them ``NotImplementedError`` (no ATen fallback
  here; under ``patch()`` such calls stay on Kornia's own function).
"""
from __future__ import annotations

from functools import lru_cache
from typing import Optional, Union

import torch
from torch import nn

from .. import _native as N
from ..core.check import KORNIA_CHECK, KORNIA_CHECK_IS_TENSOR, KORNIA_CHECK_SHAPE
from .filter import _BORDER_CODE, _check_pad_fits
from .kernels import _unpack_2d_ks, get_gaussian_kernel2d

__all__ = ["BilateralBlur", "JointBilateralBlur", "bilateral_blur", "joint_bilateral_blur"]

MAX_KERNEL_SIDE = 15
MAX_CHANNELS = 16
_DIST_CODE = {"l1": 0, "l2": 1}


@lru_cache(maxsize=256)
def _cached_params(ky: int, kx: int, sigma_color: float, sigma_space: tuple, dtype: torch.dtype, device: torch.device):
    """(space (1, ky kx), coef (1,)) in the compute type ``dtype`` for Python-float sigmas: evaluated once on the host with the reference's
    own formulas and kept resident on the device - the steady state of a call is one launch and no H2D copy (as gaussian.py:_cached_taps)."""
    with torch.inference_mode(False), torch.no_grad():
        space = get_gaussian_kernel2d((ky, kx), sigma_space, dtype=dtype).reshape(1, ky * kx)
        coef = torch.tensor([-0.5 / sigma_color**2], dtype=dtype)  # a host double, rounded once
        return space.to(device).contiguous(), coef.to(device)


def _launch_fwd(xc, gc, space, coef, ky, kx, border, dist, with_wsum):
    B, C, H, W = xc.shape
    out = torch.empty_like(xc)
    wsum = torch.empty((B, H, W), device=xc.device, dtype=space.dtype) if with_wsum else None
    N.launch("km_bilateral_blur_fwd", xc.device, xc.data_ptr(), N.ptr(gc), space.data_ptr(), coef.data_ptr(), out.data_ptr(), N.ptr(wsum), B, C,
             C if gc is None else gc.shape[1], H, W, space.shape[0], coef.shape[0], ky, kx, border, dist, N.dtype_code(xc.dtype))
    return out, wsum


class _BilateralFunction(torch.autograd.Function):
    """x (B,C,H,W); guide (B,Cg,H,W) or None (self-guided); space (Bs, ky kx), coef (Bc,) in the compute type."""

    @staticmethod
    def forward(ctx, x, guide, space, coef, ky: int, kx: int, border: int, dist: int):
        xc = x.detach().contiguous()
        gc = None if guide is None else guide.detach().contiguous()
        need = bool(ctx.needs_input_grad[0]) or (guide is not None and bool(ctx.needs_input_grad[1]))
        out, wsum = _launch_fwd(xc, gc, space, coef, ky, kx, border, dist, need)
        if need:
            ctx.save_for_backward(xc, out, wsum, space, coef) if gc is None else ctx.save_for_backward(xc, out, wsum, space, coef, gc)
        ctx.cfg = (ky, kx, border, dist, gc is not None)
        return out

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        ky, kx, border, dist, joint = ctx.cfg
        xc, out, wsum, space, coef = ctx.saved_tensors[:5]
        gc = ctx.saved_tensors[5] if joint else None
        B, C, H, W = xc.shape
        g = gy.detach().to(xc.dtype).contiguous()
        gx = torch.empty_like(xc) if (ctx.needs_input_grad[0] or not joint) else None
        gg = torch.empty_like(gc) if (joint and ctx.needs_input_grad[1]) else None
        N.launch("km_bilateral_blur_bwd", xc.device, xc.data_ptr(), N.ptr(gc), space.data_ptr(), coef.data_ptr(), out.data_ptr(), wsum.data_ptr(), g.data_ptr(),
                 N.ptr(gx), N.ptr(gg), B, C, gc.shape[1] if joint else C, H, W, space.shape[0], coef.shape[0], ky, kx, border, dist, N.dtype_code(xc.dtype))
        return gx, gg, None, None, None, None, None, None


def _window(kernel_size) -> tuple:
    ky, kx = _unpack_2d_ks(kernel_size)
    if ky < 1 or kx < 1 or ky % 2 == 0 or kx % 2 == 0:
        # (the reference's unfolded windows no longer match the image for an even side: RuntimeError there too)
        raise RuntimeError(f"bilateral_blur: kernel_size must be odd and positive in both directions, got ({ky}, {kx})")
    return ky, kx


def _needs_grad(t) -> bool:
    return isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled()


def supported(input, guidance, kernel_size, sigma_color, sigma_space, border_type="reflect", color_distance_type="l1") -> bool:
    """True when the native op takes this call: (B,C,H,W) tensors of one supported dtype, odd window sides of 1 .. 15, at most 16 channels a
    side, a border and a distance it knows, a pad that fits the image, and no sigma tensor that needs a gradient."""
    try:
        ky, kx = _unpack_2d_ks(kernel_size)
    except Exception:
        return False
    if not (ky >= 1 and kx >= 1 and ky % 2 == 1 and kx % 2 == 1 and max(ky, kx) <= MAX_KERNEL_SIDE):
        return False
    if not (isinstance(input, torch.Tensor) and input.dim() == 4 and input.dtype in N._DTYPE_CODES and input.shape[1] <= MAX_CHANNELS):
        return False
    if guidance is not None and not (isinstance(guidance, torch.Tensor) and guidance.dim() == 4 and guidance.dtype == input.dtype
                                     and guidance.shape[1] <= MAX_CHANNELS and guidance.shape[0] == input.shape[0]
                                     and guidance.shape[-2:] == input.shape[-2:]):
        return False
    if border_type not in _BORDER_CODE or color_distance_type not in _DIST_CODE:
        return False
    if _needs_grad(sigma_color) or _needs_grad(sigma_space):
        return False
    B = input.shape[0]
    if isinstance(sigma_color, torch.Tensor):
        if sigma_color.dim() != 1 or sigma_color.shape[0] not in (1, B):
            return False
    elif not isinstance(sigma_color, (int, float)):
        return False
    if isinstance(sigma_space, torch.Tensor):
        if sigma_space.dim() != 2 or sigma_space.shape[1] != 2 or sigma_space.shape[0] not in (1, B):
            return False
    elif not (isinstance(sigma_space, tuple) and len(sigma_space) == 2):
        return False
    try:
        _check_pad_fits(border_type, ky, kx, input.shape[2], input.shape[3])
    except RuntimeError:
        return False
    return True


def _bilateral_blur(input, guidance, kernel_size, sigma_color, sigma_space, border_type: str = "reflect", color_distance_type: str = "l1") -> torch.Tensor:
    KORNIA_CHECK_IS_TENSOR(input)
    KORNIA_CHECK_SHAPE(input, ["B", "C", "H", "W"])
    if guidance is not None:
        KORNIA_CHECK_IS_TENSOR(guidance)
        KORNIA_CHECK_SHAPE(guidance, ["B", "C", "H", "W"])
        KORNIA_CHECK((guidance.shape[0] == input.shape[0]) and (guidance.shape[-2:] == input.shape[-2:]),
                     "guidance and input should have the same batch size and spatial dimensions")
    if isinstance(sigma_color, torch.Tensor):
        KORNIA_CHECK_SHAPE(sigma_color, ["B"])
    ky, kx = _window(kernel_size)
    if color_distance_type not in _DIST_CODE:
        raise ValueError("color_distance_type only accepts l1 or l2")
    if border_type not in _BORDER_CODE:
        raise NotImplementedError(f"bilateral_blur: border_type must be one of {sorted(_BORDER_CODE)}, got {border_type!r}")
    if max(ky, kx) > MAX_KERNEL_SIDE:
        raise NotImplementedError(f"bilateral_blur: windows up to {MAX_KERNEL_SIDE} x {MAX_KERNEL_SIDE} are supported, got ({ky}, {kx})")
    B, C, H, W = input.shape
    Cg = C if guidance is None else guidance.shape[1]
    if max(C, Cg) > MAX_CHANNELS:
        raise NotImplementedError(f"bilateral_blur: at most {MAX_CHANNELS} channels of input and of guidance are supported, got {C} and {Cg}")
    if _needs_grad(sigma_color) or _needs_grad(sigma_space):
        raise NotImplementedError("bilateral_blur: gradients wrt sigma_color / sigma_space are not implemented (pass tensors that do not require grad)")
    N.require_device(input, "input")
    N.dtype_code(input.dtype)
    if guidance is not None:
        N.require_device(guidance, "guidance")
        if guidance.dtype != input.dtype:
            raise TypeError(f"bilateral_blur: guidance must have the dtype of input ({input.dtype}), got {guidance.dtype}")
    _check_pad_fits(border_type, ky, kx, H, W)
    if B == 0:
        return torch.empty_like(input)

    compute = N.compute_dtype(input.dtype)
    if isinstance(sigma_color, torch.Tensor) or isinstance(sigma_space, torch.Tensor):
        if isinstance(sigma_color, torch.Tensor):
            sc = sigma_color.detach().to(device=input.device, dtype=input.dtype)
            coef = (-0.5 / sc**2).to(compute).contiguous()
        else:
            coef = torch.tensor([-0.5 / float(sigma_color) ** 2], dtype=compute).to(input.device)
        ss = sigma_space.detach().to(device=input.device, dtype=compute) if isinstance(sigma_space, torch.Tensor) else sigma_space
        space = get_gaussian_kernel2d((ky, kx), ss, device=input.device, dtype=compute)
        space = space.reshape(space.shape[0], ky * kx).contiguous()
        if space.shape[0] not in (1, B) or coef.shape[0] not in (1, B):
            raise RuntimeError(f"bilateral_blur: sigma_color has {coef.shape[0]} and sigma_space {space.shape[0]} entries, each must be 1 or the batch size {B}")
    else:
        KORNIA_CHECK(isinstance(sigma_space, tuple) and len(sigma_space) == 2, "Shape dimension mismatch: expected sigma_space of shape ['B', '2']")
        space, coef = _cached_params(ky, kx, float(sigma_color), (float(sigma_space[0]), float(sigma_space[1])), compute, input.device)

    border, dist = _BORDER_CODE[border_type], _DIST_CODE[color_distance_type]
    if not (torch.is_grad_enabled() and (input.requires_grad or (guidance is not None and guidance.requires_grad))):
        gc = None if guidance is None else guidance.detach().contiguous()
        return _launch_fwd(input.detach().contiguous(), gc, space, coef, ky, kx, border, dist, False)[0]  # (no autograd node to build)
    return _BilateralFunction.apply(input, guidance, space, coef, ky, kx, border, dist)


def bilateral_blur(input: torch.Tensor, kernel_size: Union[tuple[int, int], int], sigma_color: Union[float, torch.Tensor],
                   sigma_space: Union[tuple[float, float], torch.Tensor], border_type: str = "reflect", color_distance_type: str = "l1") -> torch.Tensor:
    """Edge-preserving blur of ``input`` (B,C,H,W): a Gaussian of ``sigma_space`` (floats (sy, sx) or a (B,2) tensor) over a ``kernel_size``
    window (int or (ky, kx), odd) whose taps are also weighted by ``exp(-0.5 D / sigma_color^2)``, ``D`` the squared ``'l1'`` (OpenCV) or
    ``'l2'`` (Matlab) colour distance to the centre pixel.  ``border_type``: ``'constant' | 'reflect' | 'replicate' | 'circular'``."""
    return _bilateral_blur(input, None, kernel_size, sigma_color, sigma_space, border_type, color_distance_type)


def joint_bilateral_blur(input: torch.Tensor, guidance: torch.Tensor, kernel_size: Union[tuple[int, int], int], sigma_color: Union[float, torch.Tensor],
                         sigma_space: Union[tuple[float, float], torch.Tensor], border_type: str = "reflect", color_distance_type: str = "l1") -> torch.Tensor:
    """:func:`bilateral_blur` with the colour distance taken in ``guidance`` (B,Cg,H,W; its channel count may differ from the input's)."""
    return _bilateral_blur(input, guidance, kernel_size, sigma_color, sigma_space, border_type, color_distance_type)


class _BilateralBlur(nn.Module):
    def __init__(self, kernel_size: Union[tuple[int, int], int], sigma_color: Union[float, torch.Tensor], sigma_space: Union[tuple[float, float], torch.Tensor],
                 border_type: str = "reflect", color_distance_type: str = "l1") -> None:
        super().__init__()
        self.kernel_size = kernel_size
        self.sigma_color = sigma_color
        self.sigma_space = sigma_space
        self.border_type = border_type
        self.color_distance_type = color_distance_type

    def __repr__(self) -> str:
        return (f"{self.__class__.__name__}(kernel_size={self.kernel_size}, sigma_color={self.sigma_color}, sigma_space={self.sigma_space}, "
                f"border_type={self.border_type}, color_distance_type={self.color_distance_type})")


class BilateralBlur(_BilateralBlur):
    """Module form of :func:`bilateral_blur`."""

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        return bilateral_blur(input, self.kernel_size, self.sigma_color, self.sigma_space, self.border_type, self.color_distance_type)


class JointBilateralBlur(_BilateralBlur):
    """Module form of :func:`joint_bilateral_blur`."""

    def forward(self, input: torch.Tensor, guidance: torch.Tensor) -> torch.Tensor:
        return joint_bilateral_blur(input, guidance, self.kernel_size, self.sigma_color, self.sigma_space, self.border_type, self.color_distance_type)
