"""Generates tests/golden/median_blur.npz from the reference (Kornia) - run in a checkout next to the reference tree, not by the suite:

    python tests/make_golden_median.py

``kornia.filters.median_blur`` on the dtype x kernel-size x shape grid of tests/test_gpu_median.py, the two non-finite images, the
reference's ``x.grad`` on tie-free images, and what ``RandomMedianBlur`` - alone and behind ``RandomAffine`` in an ``AugmentationSequential``
with a mask - draws and returns for ``torch.manual_seed(s)``.  Arrays only.  The images hold multiples of 1/64 in [-2, 2]: exact in all four
dtypes (bfloat16 arrays are stored widened to float32, numpy has no bfloat16) and small once compressed."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

DTYPES = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}
KERNELS = [(3, 3), (5, 5), (7, 7), (3, 5), (5, 1), (1, 1), (9, 3), (15, 15)]
SHAPES = [(2, 3, 13, 17), (1, 1, 2, 3), (1, 2, 1, 9), (2, 2, 16, 24)]
GRAD_KERNELS = [(3, 3), (5, 5), (3, 7)]
GRAD_SHAPE = (2, 2, 12, 20)  # H W = 240: a permutation of 1 .. 240 is exact in bfloat16


def store(t: torch.Tensor) -> np.ndarray:
    return (t.float() if t.dtype == torch.bfloat16 else t).contiguous().numpy()


def sname(shape) -> str:
    return "x".join(str(v) for v in shape)


def kname(k) -> str:
    return f"{k[0]}x{k[1]}"


def main() -> None:
    from ref_shim import import_reference

    K = import_reference()
    A = K.augmentation
    g = torch.Generator().manual_seed(1405)
    d = {}
    # i. parity grid
    for shape in SHAPES:
        x = torch.randint(-128, 129, shape, generator=g).float() / 64
        d[f"x__{sname(shape)}"] = x
        for dn, dt in DTYPES.items():
            for k in KERNELS:
                y = K.filters.median_blur(x.to(dt), k)
                assert y.dtype == dt and y.shape == x.shape
                d[f"y__{sname(shape)}__{kname(k)}__{dn}"] = y
    # an int kernel size is the square window
    assert torch.equal(K.filters.median_blur(d["x__2x3x13x17"], 3), d["y__2x3x13x17__3x3__f32"])
    # ii. non-finite: one NaN / one inf at a corner of a 3 x 3 image
    for name, bad in (("nan", float("nan")), ("inf", float("inf"))):
        x = torch.arange(1.0, 10.0).view(1, 1, 3, 3).clone()
        x[0, 0, 0, 0] = bad
        d[f"nf_{name}__x"] = x
        d[f"nf_{name}__y"] = K.filters.median_blur(x, (3, 3))
    # iii. tie-free gradients: every channel a permutation of 1 .. H W, integer grad_out in [-2, 2]
    B, C, H, W = GRAD_SHAPE
    xg = torch.stack([torch.randperm(H * W, generator=g).float() + 1 for _ in range(B * C)]).view(GRAD_SHAPE)
    go = torch.randint(-2, 3, GRAD_SHAPE, generator=g).float()
    d["grad__x"], d["grad__gout"] = xg, go
    for k in GRAD_KERNELS:
        xr = xg.clone().requires_grad_()
        K.filters.median_blur(xr, k).backward(go)
        d[f"grad__{kname(k)}"] = xr.grad
    # iv. RandomMedianBlur alone, v. behind RandomAffine in the container with a mask
    xa = torch.randint(-128, 129, (5, 3, 16, 24), generator=g).float() / 64
    mk = torch.randint(0, 21, (5, 1, 16, 24), generator=g, dtype=torch.uint8)
    d["aug__x"], d["aug__mask"] = xa, mk
    for seed in (3, 11):
        torch.manual_seed(seed)
        aug = A.RandomMedianBlur((3, 3), p=0.5)
        out = aug(xa)
        d[f"rmb__seed{seed}__rng_after"] = torch.get_rng_state()[:64].clone()
        d[f"rmb__seed{seed}__batch_prob"] = aug._params["batch_prob"]
        d[f"rmb__seed{seed}__out"] = out
        torch.manual_seed(seed)
        seq = A.AugmentationSequential(A.RandomAffine(degrees=15.0, translate=(0.1, 0.1), scale=(0.8, 1.2), p=0.7), A.RandomMedianBlur((5, 5)),
                                       data_keys=["input", "mask"])
        out, mout = seq(xa, mk)
        key = f"seq__seed{seed}"
        d[key + "__rng_after"] = torch.get_rng_state()[:64].clone()
        for item in seq._params:
            for k, v in item.data.items():
                if isinstance(v, torch.Tensor):
                    d[f"{key}__{item.name}__{k}"] = v
        d[key + "__out"], d[key + "__mask_out"] = out, mout
    # vi. what the reference raises for even sizes
    names = []
    for k in ((4, 4), (3, 4), (2, 3)):
        try:
            K.filters.median_blur(torch.zeros(1, 1, 6, 6), k)
            names.append("none")
        except Exception as e:  # noqa: BLE001
            names.append(type(e).__name__)
    arrays = {k: store(v) for k, v in d.items()}
    arrays["even__kernels"] = np.array([[4, 4], [3, 4], [2, 3]], dtype=np.int64)
    arrays["even__raises"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "median_blur.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes", names)


if __name__ == "__main__":
    torch.set_num_threads(4)
    main()
