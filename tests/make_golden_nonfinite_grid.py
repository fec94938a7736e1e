"""Generates tests/golden/nonfinite_grid.npz from ATen's CPU ``F.grid_sample`` (the sampler the reference calls) - run by hand on a CPU, not by
the suite:

    python tests/make_golden_nonfinite_grid.py

What the sampler returns when the GRID itself holds NaN, +inf or -inf: every pairing of the coordinates VALUES below (a non-finite x with a
non-finite y, with a finite y, and the other way round; the finite ones among themselves), on a 5 x 7 source and on a 1 x 6 one (whose
align_corners=True unnormalise scale along y is 0: inf * 0), 3 interpolation modes x 3 padding modes x both align_corners, fp32 and fp64.
FORWARD ONLY: ATen's CPU backward reads out of bounds for a NaN grid under border / reflection padding (and for +-inf under reflection) and
takes the process down; nothing here - and no test - calls it.

A fixture and not a live call, because what the result is under border / reflection - NaN clipped to coordinate 0 - rests on what the vector
max / min of the CPU build that ran it do with a NaN operand; that build's CPU capability is recorded in the file (`cpu_capability`).  The
image and the finite coordinates are dyadic, so the fp32 and the fp64 cases sample the very same values."""
from __future__ import annotations

import os
import re

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
nan, inf = float("nan"), float("inf")
VALUES = [nan, inf, -inf, 0.25, -1.0, 1.0, -0.375, 1.5]
SOURCES = {"5x7": (5, 7), "1x6": (1, 6)}
MODES = ["bilinear", "nearest", "bicubic"]
PADS = ["zeros", "border", "reflection"]
DTYPES = {"f32": torch.float32, "f64": torch.float64}


def inputs(name: str, dtype: torch.dtype):
    """(image (1,2,H,W) of multiples of 1/64 in [0, 1), grid (1,8,8,2): x = VALUES along the columns, y = VALUES along the rows)"""
    H, W = SOURCES[name]
    g = torch.Generator().manual_seed(H * 16 + W)
    x = torch.randint(0, 64, (1, 2, H, W), generator=g).to(dtype) / 64
    gx, gy = torch.meshgrid(torch.tensor(VALUES, dtype=dtype), torch.tensor(VALUES, dtype=dtype), indexing="xy")
    return x, torch.stack([gx, gy], -1)[None].contiguous()


def key(name: str, dn: str, mode: str, pad: str, align: bool) -> str:
    return f"y__{name}__{dn}__{mode}__{pad}__{int(align)}"


def main() -> None:
    d = {}
    for name in SOURCES:
        for dn, dt in DTYPES.items():
            x, grid = inputs(name, dt)
            for mode in MODES:
                for pad in PADS:
                    for align in (False, True):
                        d[key(name, dn, mode, pad, align)] = F.grid_sample(x, grid, mode, pad, align).numpy()
    cap = re.search(r"CPU capability usage: (\S+)", torch.__config__.show())
    d["cpu_capability"] = np.array(cap.group(1) if cap else "unknown")
    d["torch_version"] = np.array(torch.__version__)
    path = os.path.join(ROOT, "tests", "golden", "nonfinite_grid.npz")
    np.savez_compressed(path, **d)
    print(path, os.path.getsize(path), "bytes,", len(d), "arrays, CPU capability", d["cpu_capability"])


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
