"""Generates tests/golden/nonfinite_pixels.npz from the reference (Kornia) - run in a checkout next to the reference tree, not by the suite:

    python tests/make_golden_nonfinite_pixels.py

What the reference returns when the IMAGE holds a NaN, a +inf or a -inf (one image per kind, so the patterns do not merge; the planted
pixels and the case table are tests/nonfinite_pixel_cases.py, shared with tests/test_zz_gpu_nonfinite_pixels.py): the forward of every case
in fp32 and, for the cases that list them, fp64 / bf16 / f16; for the linear ops marked `grad`, the reference's ``x.grad`` of the CLEAN image
for a ``grad_out`` with a planted value; for ``color_jitter`` the image and factor gradients with a non-finite pixel; for ``filter2d`` the tap
gradient.  Arrays only; bfloat16 arrays are stored widened to float32 (numpy has no bfloat16).  To stay small the file holds sample 0 of every
result - the sample that carries the planted pixels; the tests compare the clean sample with the same call on that sample alone.

Left out, with the reason:
  * ``canny``: the reference raises an IndexError on any non-finite pixel.
  * A dtype whose CPU op the reference does not have (it raises "not implemented for 'Half'" or the like): the case is recorded without that
    dtype and printed as skipped (with this torch: none); the test then uses the fp32 result's NaN / inf pattern on the rounded inputs.

A committed file holds at most 1 MiB, so the record is two files: tests/golden/nonfinite_pixels.npz (the table's CASES and the gradients of the
linear and colour ops) and tests/golden/nonfinite_pixels_2.npz (CASES2 - crop_by_indices, remap / grid_sample, homography_warp, warp + blur -
the further dtypes of MORE_DTYPES, masked_warp_loss, transform_points and both gradients of the bilinear warp with non-finite pixels)."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def store(t: torch.Tensor) -> np.ndarray:
    return (t.float() if t.dtype == torch.bfloat16 else t).detach().contiguous().numpy()


def main() -> None:
    import nonfinite_pixel_cases as P
    from ref_shim import import_reference

    K = import_reference()
    d, d2, skipped = {}, {}, []
    for case in P.ALL_CASES:
        for sn in case.shapes:
            for dn in case.dtypes_for(sn):
                k = P.key(case, sn, dn)
                try:
                    ys = [case.ref(K, P.image(sn, kind).to(P.DTYPES[dn])) for kind in P.KINDS]
                except (RuntimeError, NotImplementedError) as e:
                    skipped.append(f"{k}: {type(e).__name__}: {str(e).splitlines()[0][:120]}")
                    continue
                assert all(y.dtype == P.DTYPES[dn] for y in ys), k
                (d2 if P.in_second_file(case, dn) else d)[k] = torch.stack([y[0] for y in ys], -1)
            if case.grad:  # the adjoint of a linear op: the clean image, a planted grad_out
                gs = []
                for kind in P.KINDS:
                    x = P.image(sn, None).requires_grad_()
                    y = case.ref(K, x)
                    y.backward(P.grad_out(y.shape, kind))
                    gs.append(x.grad[0])
                d[P.key(case, sn, "f32", "gx")] = torch.stack(gs, -1)
    for sn in P.OVERFLOW.shapes:
        d[P.key(P.OVERFLOW, sn, "f16")] = P.OVERFLOW.ref(K, P.overflow_image(sn).half())[0]
    # non-finite pixels through the non-linear gradients: colour (image and factors), the filter2d taps
    for sn in ("w24", "w23"):
        for kind in P.KINDS:
            for order in ("0123", "2031", "0", "1", "2", "3"):
                x = P.image(sn, kind).requires_grad_()
                f = [torch.tensor(v, requires_grad=True) for v in (P.BF, P.CF, P.SF, P.HF)]
                out = x
                for s in order:
                    s = int(s)
                    out = getattr(K.enhance, P._STAGE[s])(out, f[s])
                g = torch.Generator().manual_seed(5)
                w = torch.randint(-2, 3, out.shape, generator=g).float()
                (out * w).sum().backward()
                base = f"jitterbwd_{order}__{sn}__{kind}__f32__"
                d[base + "gx"] = x.grad[:1]
                for s in order:
                    d[base + f"gf{s}"] = f[int(s)].grad
            x = P.image(sn, kind)
            taps = torch.tensor(P.K33Z).requires_grad_()
            y = K.filters.filter2d(x, taps, "reflect")
            g = torch.Generator().manual_seed(6)
            (y * torch.randint(-2, 3, y.shape, generator=g).float()).sum().backward()
            d[f"f2dtaps__{sn}__{kind}__f32__gk"] = taps.grad
    for sn in P.TWO:
        for kind in P.KINDS:
            for loss, thr in P.LOSSES:
                d2[f"loss_{loss}_{thr}__{sn}__{kind}__f32__y"] = P.loss_reference(K, P.image(sn, kind), P.image(sn, None).flip(-1), loss, thr)
    for kind in P.KINDS:
        d2[f"points__{kind}__f32__y"] = K.geometry.linalg.transform_points(torch.tensor(P.PER), P.points(kind))
    for pad, sn in P.WARP_GRADS:
        for kind in P.KINDS:
            x, M = P.image(sn, kind).requires_grad_(), torch.tensor(P.PER).requires_grad_()
            y = P.warp_grad_call(K, x, M, pad)
            y.backward(P.grad_out(y.shape, None))
            d2[f"warpbwd_{pad}__{sn}__{kind}__f32__gx"] = x.grad[0]
            d2[f"warpbwd_{pad}__{sn}__{kind}__f32__gM"] = M.grad
    for name, dd in (("nonfinite_pixels", d), ("nonfinite_pixels_2", d2)):
        arrays = {k: store(v) for k, v in dd.items()}
        path = os.path.join(ROOT, "tests", "golden", name + ".npz")
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path), "bytes,", len(arrays), "arrays")
    for s in skipped:
        print("skipped", s)


if __name__ == "__main__":
    torch.set_num_threads(4)
    main()
