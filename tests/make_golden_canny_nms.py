"""Generates tests/golden/canny_nms.npz from the reference (Kornia) - run in a checkout next to the reference tree, not by the suite:

    python tests/make_golden_canny_nms.py

The reference's own ``canny(..., hysteresis=False)`` with its two front stages replaced inside its module: ``gaussian_blur2d`` is the
identity and ``spatial_gradient`` returns prepared planes, so what is recorded is the reference's magnitude, direction binning,
neighbour table, suppression and thresholds applied to gradients that this script chooses - for
tests/test_zz_gpu_canny.py::test_nms_equals_the_reference_tail_exactly (km_canny_nms_fwd on the same planes, compared by equality).

The planes are integers in -12 .. 12 over 32: every product and sum of the magnitude is exact in float32, sqrt is correctly rounded on
both sides, and atan2 * 4 / pi of such vectors stays more than 2e-3 away from every half-integer, so a few ulp of atan2 cannot move a
direction.  Columns 40-43 repeat column 40 and rows 10-12 repeat row 10 (plateaus: equal magnitudes along a gradient direction), a
(3, 4) / 32 gradient has magnitude exactly `low` and a (6, 8) / 32 one exactly `high`."""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

B, H, W = 2, 37, 130  # 64 x 16 blocks of 4 rows per thread: a 2-column last tile, a 5-row last block, a part-filled group of 4 rows
SCALE = 32
LOW, HIGH = 5 / SCALE, 10 / SCALE
EPS = (0.0, 1e-6)


def planes() -> torch.Tensor:
    """(B,2,H,W) int8: gx plane, gy plane, in units of 1 / SCALE"""
    g = torch.Generator().manual_seed(2024)
    p = torch.randint(-12, 13, (B, 2, H, W), generator=g)
    p[..., 40:44] = p[..., 40:41]
    p[..., 10:13, :] = p[..., 10:11, :]
    return p.to(torch.int8)


def main() -> None:
    from ref_shim import import_reference

    import_reference()
    ref = importlib.import_module("kornia.filters.canny")
    p = planes()
    grads = (p.float() / SCALE)[:, None]  # (B,1,2,H,W), what spatial_gradient returns for one channel
    ref.gaussian_blur2d = lambda x, *a, **k: x
    ref.spatial_gradient = lambda x, *a, **k: grads
    d = {"planes": p, "scale": torch.tensor(SCALE), "low": torch.tensor(LOW, dtype=torch.float64), "high": torch.tensor(HIGH, dtype=torch.float64),
         "eps": torch.tensor(EPS, dtype=torch.float64)}
    for n, eps in enumerate(EPS):
        mag, edges = ref.canny(torch.zeros(B, 1, H, W), LOW, HIGH, hysteresis=False, eps=eps)
        assert mag.dtype == torch.float32 and mag.shape == (B, 1, H, W) and set(edges.unique().tolist()) == {0.0, 0.5, 1.0}
        d[f"mag_eps{n}"] = mag
        d[f"edges2_eps{n}"] = (edges * 2).to(torch.uint8)
    arrays = {k: v.contiguous().numpy() for k, v in d.items()}
    path = os.path.join(ROOT, "tests", "golden", "canny_nms.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    torch.set_num_threads(4)
    main()
