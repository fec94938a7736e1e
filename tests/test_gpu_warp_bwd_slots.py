"""GPU: the slots of the one-read warp backward (csrc/km_warp_bwd_fused.hip, kmo_process) at the smallest shapes that reach each of their paths.

A workgroup walks the box of a 64 x 64 source tile in slabs of P = 1024 / (box width) rows, one slot per slab; a wave whose 64 threads
all sit below the box's last row skips the slot's position and matrix-gradient arithmetic (it would add zeros).  The shapes:

  one_tile_64      1x3x64x64     one tile, the box clipped to the 64 x 64 output: four full slabs of 16 rows, no wave without a pixel
  flagship_128     1x3x128x128   the benchmark's corner jitter scaled to the size (8 px at 512 -> 2 px): ~66-wide boxes, P = 15, the last
                                 slab holds ~6 of 15 rows - the waves below them have no valid lane
  flagship_128_b2  2x1x128x128   the same boxes through the one-channel instantiation, two images (the image-end sums between them)
  flagship_128_fill              flagship_128 with padding_mode="fill"
  edge_80          1x3x80x80     a 16-wide edge tile (and a 16-high one): its single slab is mostly waves without a pixel
  rotated_128      1x3x128x128   warp_affine, 20 degrees about the centre: boxes ~82 wide and ~82 high, P = 12, 6 slots x 12 = 72 rows a
                                 pass -> two passes; grad_out grows down the rows, so the second rescales what the first accumulated

Bounds: against the plain-C oracle those of tests/test_gpu_config_parity.py (grad wrt the image <= 1e-5 absolute, grad wrt the matrix <= 5e-5 of
its largest entry); against the two-launch form (km_warp2d_bwd without a workspace = the policy warp_bwd_fused 0) those of
tests/test_gpu_warp_fused.py: each form's image gradient is within 2e-6 max|grad_out| of the exact sum (fixed point), so the two
are within 5e-6 max|grad_out| of each other; the matrix gradients are fp64 sums of fp32 products in another order, 5e-5 like the oracle's.
Also runs on the host build of the kernels (tests/test_emulated_warp_bwd_slots.py)."""
import functools
import math

import pytest
import torch

from _util import flagship_homographies

pytestmark = pytest.mark.gpu

FILL = (0.2, 0.5, 0.7)
CASES = {
    #                  B, C, S,   matrices,   padding
    "one_tile_64": (1, 3, 64, "flagship", "zeros"),
    "flagship_128": (1, 3, 128, "flagship", "zeros"),
    "flagship_128_b2": (2, 1, 128, "flagship", "zeros"),
    "flagship_128_fill": (1, 3, 128, "flagship", "fill"),
    "edge_80": (1, 3, 80, "flagship", "zeros"),
    "rotated_128": (1, 3, 128, "rotated", "zeros"),
}


def _lib():
    from kornia_amd import _native as N

    return N.lib()


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(x, M, grad_out) of a case: seeded, built once, never written to"""
    B, C, S, kind, _ = CASES[name]
    g = torch.Generator().manual_seed(800 + 7 * S + B)
    x = torch.rand(B, C, S, S, generator=g)
    if kind == "flagship":
        M = flagship_homographies(B, S, S, S, S, g, jitter=8.0 * S / 512.0)
    else:  # 20 degrees about the centre, as a (B,2,3) affine matrix
        c, s, ctr = math.cos(math.radians(20.0)), math.sin(math.radians(20.0)), (S - 1) / 2.0
        M = torch.tensor([[c, s, (1 - c) * ctr - s * ctr], [-s, c, s * ctr + (1 - c) * ctr]]).repeat(B, 1, 1)
    go = torch.rand(B, C, S, S, generator=g) - 0.4
    if kind == "rotated":  # |grad_out| grows down the rows (x 2 every 8 rows, <= 0.6): every later pass of a box meets a larger maximum than its scale was chosen for
        go = go * torch.pow(2.0, (torch.arange(S, dtype=torch.float32) - (S - 1)) / 8.0).view(1, 1, S, 1)
    return x, M, go


def _kw(name):
    pad = CASES[name][4]
    return dict(padding_mode="fill", fill_value=torch.tensor(FILL)) if pad == "fill" else {}


def _op(name):
    import kornia_amd as K

    S, kind = CASES[name][2], CASES[name][3]
    kw = _kw(name)
    if kw:
        kw = dict(kw, fill_value=kw["fill_value"].cuda())
    warp = K.warp_affine if kind == "rotated" else K.warp_perspective
    return lambda a, m: warp(a, m, (S, S), **kw)


@functools.lru_cache(maxsize=None)
def _oracle_grads(name):
    """(grad_x, grad_M) of the plain-C oracle, once per case"""
    import oracle

    x, M, go = _inputs(name)
    S, kind = CASES[name][2], CASES[name][3]
    bwd = oracle.warp_affine_backward if kind == "rotated" else oracle.warp_perspective_backward
    return bwd(go, x, M, (S, S), **_kw(name))


def _grads(name, fused, x=None, M=None, go=None):
    """(grad_x, grad_M) through the public API, the one-read backward on (the workspace form) or off (the two launches)"""
    x0, M0, go0 = _inputs(name)
    x, M, go = (x0 if x is None else x), (M0 if M is None else M), (go0 if go is None else go)
    lib = _lib()
    prev = lib.km_config_set(b"warp_bwd_fused", 1 if fused else 0)
    try:
        xg, Mg = x.cuda().requires_grad_(), M.cuda().requires_grad_()
        _op(name)(xg, Mg).backward(go.cuda())
    finally:
        lib.km_config_set(b"warp_bwd_fused", prev)
    return xg.grad.cpu(), Mg.grad.cpu()


def _rel(a, b):  # (tests/test_gpu_config_parity.py)
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("name", list(CASES))
def test_both_gradients_against_the_oracle_and_the_two_launches(oracle, name):
    B, C, S, _, pad = CASES[name]
    assert _lib().km_warp2d_bwd_workspace_bytes(B, C, S, S, S, S, 1, 3 if pad == "fill" else 0, 0) > 0  # the one-read form is what runs
    _, _, go = _inputs(name)
    gx, gM = _grads(name, True)
    gxo, gMo = _oracle_grads(name)
    ex, em = (gx - gxo).abs().max().item(), _rel(gM, gMo)
    gx2, gM2 = _grads(name, False)
    ex2, em2 = (gx - gx2).abs().max().item(), _rel(gM, gM2)
    print(f"{name}: |d grad_x| {ex:.3e} (oracle) {ex2:.3e} (two launches)   rel d grad_M {em:.3e} (oracle) {em2:.3e} (two launches)")
    assert ex <= 1e-5
    assert em <= 5e-5
    assert ex2 <= 5e-6 * go.abs().max().item()
    assert em2 <= 5e-5


def test_image_gradient_is_bit_identical_from_run_to_run():
    """integer accumulators: the order in which the waves (the skipping ones among them) reach a cell does not show"""
    first = _grads("flagship_128", True)
    for _ in range(3):
        gx, gM = _grads("flagship_128", True)
        assert torch.equal(gx, first[0])
        assert _rel(gM, first[1]) <= 1e-6  # (fp64 atomics over the tiles of the image, rounded to fp32 once)


def test_bf16_storage_is_the_fp32_path_rounded_once():
    """tests/test_gpu_half_grads.py, contract 1: on the owner paths the 16-bit image gradient is the fp32 path's on the same (rounded) values,
    rounded once, bit for bit; the matrix gradient an fp64 sum of the same fp32 products in both (1e-6 of its largest entry)."""
    x, M, go = _inputs("flagship_128")
    x16, go16 = x.bfloat16(), go.bfloat16()
    gx16, gM16 = _grads("flagship_128", True, x=x16, go=go16)
    gx32, gM32 = _grads("flagship_128", True, x=x16.float(), go=go16.float())
    assert gx16.dtype == torch.bfloat16
    assert torch.equal(gx16, gx32.bfloat16()), (gx16.float() - gx32).abs().max().item()
    assert _rel(gM16, gM32) <= 1e-6, _rel(gM16, gM32)


def test_an_inf_in_grad_out_hands_the_tile_to_the_general_launch(oracle):
    """An inf in one image's grad_out: the tiles whose boxes hold it mark themselves in the persistent loop and are written by the general
    launch in IEEE arithmetic - the non-finite pattern is the oracle's, every finite entry within the fp32 bound, that image's matrix gradient
    not finite and the other image's untouched (within the bound)."""
    name = "flagship_128_b2"
    x, M, go = _inputs(name)
    go = go.clone()
    go[1, 0, 70, 45] = float("inf")
    gx, gM = _grads(name, True, go=go)
    gxo, gMo = oracle.warp_perspective_backward(go, x, M, (128, 128))
    assert torch.equal(torch.isnan(gx), torch.isnan(gxo)) and torch.equal(torch.isinf(gx), torch.isinf(gxo))
    assert not torch.isfinite(gxo[1]).all() and torch.isfinite(gxo[0]).all()  # (the case is what it says)
    fin = torch.isfinite(gxo)
    assert (gx[fin] - gxo[fin]).abs().max().item() <= 1e-5
    assert not torch.isfinite(gM[1]).all()
    assert _rel(gM[0], gMo[0]) <= 5e-5
    # the image without the inf: bit for bit what it is without any inf in the batch (its tiles never left the persistent loop)
    gx_clean, _ = _grads(name, True)
    assert torch.equal(gx[0], gx_clean[0])
